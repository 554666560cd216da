"""The Cholesky chain (``qt_cholesky_inverse_upper``, its batched and bounded forms; csrc/cholesky.hip) on exactly
factorable matrices (``tests/exact_inputs.py``: ``factorable_spd`` / ``assert_exactly_factorable``): the factor, the
inverse factor and every intermediate of the chain are short dyadic numbers, so every schedule, block size, split and
arithmetic mode (f32 fmaf chain, three bf16 planes, two fp16 planes) has ONE correct answer to the bit.  Every
comparison here is ``exact_inputs.assert_exact`` against the constructed ``U[i][j] = Y[K-1-i][K-1-j]``; a mismatch is a
term that is missing, doubled or misplaced, and the report names its tile.  Every input has its strict lower triangle
poisoned with NaN.

Equal bits cannot show that a knob reached other code.  The witnesses at the end of the file run each variant that
changes the order of a sum and its baseline on the graded random Hessian of ``test_gpu_chol_f16x2.case`` and require the
bits to differ there; the forced-plane cases also require ``qt_chol_g3_plan_check`` to count product launches."""
import ctypes

import numpy as np
import pytest
import torch

from . import exact_inputs as ex
from .test_gpu_chol_f16x2 import case  # noqa: F401  (the module-scoped graded Hessians, for the witnesses)

pytestmark = pytest.mark.gpu

KNOBS = ("QT_CHOL_G3", "QT_CHOL_G3_MIN_CHUNKS", "QT_CHOL_PLANES", "QT_CHOL_MERGE", "QT_CHOL_TRINV", "QT_CHOL_NBO",
         "QT_CHOL_NBI", "QT_G3_LOOP", "QT_G3_TARGET_ITEMS")
MODES = ("f32", "bf16x3", "f16x2")      # the f32 chain; plane products forced, without / with a bound on lambda_min
NB_PAIRS = [(128, 128), (256, 256), (512, 512), (128, 256), (256, 512), (512, 128), (512, 256)]   # unequal: two phases
ZERO_PIVOTS = (0, 31, 32, 127, 128, 511, 512, -70, -1)                                            # negative: from K


def _env(monkeypatch, mode, **knobs):
    """Every schedule knob unset, then the mode's and the variant's own (CHOL_NBO=128 -> QT_CHOL_NBO=128)."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if mode == "f32":
        monkeypatch.setenv("QT_CHOL_G3", "0")
    else:
        monkeypatch.setenv("QT_CHOL_G3", "1")
        monkeypatch.setenv("QT_CHOL_G3_MIN_CHUNKS", "1")
    for k, v in knobs.items():
        monkeypatch.setenv("QT_" + k, str(v))


def _poisoned(A64, dev):
    """fp32 device copy of A's upper triangle over a NaN strict lower triangle."""
    A = np.triu(A64).astype(np.float32)
    assert np.array_equal(A.astype(np.float64), np.triu(A64))
    A[np.tril_indices(A.shape[0], -1)] = np.nan
    return torch.from_numpy(A).to(dev)


class Exact:
    """One guarded matrix on the device: A (poisoned), want = the chain's U, lb = a bound on lambda_min, R for pivots."""

    def __init__(self, K, seed, dev):
        A, R, Y = ex.chol_case(K, seed)
        self.bounds = ex.assert_exactly_factorable(A, R, Y)
        self.K, self.A64, self.R = K, A, R
        self.A = _poisoned(A, dev)
        self.want = torch.from_numpy(ex.chol_expected(Y).astype(np.float32)).to(dev)
        self.lb = torch.tensor([ex.min_eig_lb(A)], dtype=torch.float32, device=dev)
        assert float(self.lb) > 0

    def scaled(self, s):
        """(4^s A, 2^-s U, 4^s lb): a power of two moves no significand, in A, in the chain or in the fp16 planes (the
        scale exponents follow by s: x * 2^e is the same fp16 value)."""
        return self.A * 4.0 ** s, self.want * 2.0 ** -s, self.lb * 4.0 ** s


@pytest.fixture(scope="module")
def mats(dev):
    cache = {}

    def get(K, seed=None):
        key = (K, K if seed is None else seed)
        if key not in cache:
            cache[key] = Exact(K, key[1], dev)
        return cache[key]

    return get


def _poison_workspace(ops, dev, K, n=1):
    """Every byte of the scratch buffer the next call will be handed set to 0xFF -- a NaN as fp32, bf16 and fp16: what a
    step reads without an earlier step of the SAME call having written it (a plane copy another schedule left behind,
    say) reaches U instead of passing by luck.  Called under the environment of the call: the size depends on it."""
    from quantool_amd.hip import _lib

    nbytes = int(_lib.load().qt_cholesky_inverse_upper_batched_workspace_bytes(K, n))
    ops.workspace(nbytes, dev, "chol").fill_(0xFF)


def _run(ops, A, lb=None):
    _poison_workspace(ops, A.device, A.shape[0])
    U, info = ops.cholesky_inverse_upper(A.clone(), min_eig_lb=lb)
    torch.cuda.synchronize()
    return U, int(info.item())


def _check(ops, m, mode, what, s=0):
    A, want, lb = m.scaled(s) if s else (m.A, m.want, m.lb)
    U, info = _run(ops, A, lb if mode == "f16x2" else None)
    assert info == 0, (what, info)
    ex.assert_exact(U, want, what=what)


def _plan_launches(K, merged):
    from quantool_amd.hip import _lib

    out = (ctypes.c_longlong * 5)()
    assert _lib.load().qt_chol_g3_plan_check(K, merged, 1, ctypes.cast(out, ctypes.c_void_p)) == 0
    return int(out[0])


# ---- pivots: rsq + one Newton step at exactly representable roots ----------------------------------------------------
@pytest.mark.parametrize("trinv", ["mfma", "div"])
@pytest.mark.parametrize("span", [6, 12])
def test_pivots_that_are_powers_of_four(ops, dev, monkeypatch, span, trinv):
    """A = diag(4^k), k cycling over -span .. span: U = flip(diag(2^-k)), info 0.  Nothing but potf2_kernel's
    ``__builtin_amdgcn_rsqf`` + one Newton step, the multiplication by it and the block inverse touches a value.  span
    6 is the probe proper; 12 covers the pivots of the scaled cases below (4^-11 .. 4^11)."""
    _env(monkeypatch, "f32", **({"CHOL_TRINV": "div"} if trinv == "div" else {}))
    K = 128
    k = np.arange(K) % (2 * span + 1) - span
    A = np.diag(4.0 ** k)
    U, info = _run(ops, _poisoned(A, dev))
    assert info == 0
    want = np.diag(2.0 ** -k)[::-1, ::-1].copy()
    got = np.diag(U.cpu().numpy()).astype(np.float64)
    inexact = sorted({int(e) for e in k[::-1][got != np.diag(want)]})
    print(f"\n[pivot probe] trinv={trinv} span={span}: powers 4^k whose root is not exact: {inexact or 'none'}")
    ex.assert_exact(U, want, what=f"diag(4^k), |k| <= {span}")


# ---- sizes, f32 chain -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [129, 333, 640, 1000, 1536])
def test_f32_chain_sizes(ops, mats, monkeypatch, K):
    """129 and 333: K % 4 != 0 -- scalar fills in potf2, unaligned rows in every product, a last block of 1 / 77 rows."""
    _env(monkeypatch, "f32")
    _check(ops, mats(K), "f32", f"f32 chain K={K}")


# ---- plane products forced on for every step that has one -----------------------------------------------------------
@pytest.mark.parametrize("merge", ["0", "order", "1"])
@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("K", [640, 1000, 1536])
def test_forced_plane_products(ops, mats, monkeypatch, K, mode, merge):
    _env(monkeypatch, mode, CHOL_MERGE=merge)
    assert _plan_launches(K, 1 if merge == "1" else 0) > 0, "no block row of this K has a plane product"
    _check(ops, mats(K), mode, f"{mode} merge={merge} K={K}")


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
def test_a_width_the_planes_refuse_falls_back_to_the_f32_chain(ops, mats, monkeypatch, mode):
    """K = 333 (K % 8 != 0): no plane product is planned, the chain runs on f32 with or without a bound."""
    _env(monkeypatch, mode)
    assert _plan_launches(333, 1) == 0
    _check(ops, mats(333), mode, f"{mode} K=333")


# ---- knobs: every variant equals the same reference -----------------------------------------------------------------
def _knob_variants():
    out = [("trinv-div", m, {"CHOL_TRINV": "div"}) for m in ("f32", "bf16x3")]
    out += [(f"nb{o}-{i}", m, {"CHOL_NBO": o, "CHOL_NBI": i}) for m in MODES for o, i in NB_PAIRS]
    out += [(f"loop-chunk-merge{mg}", "bf16x3", {"G3_LOOP": "chunk", "CHOL_MERGE": mg}) for mg in ("0", "1")]
    out += [(f"items8-merge{mg}", m, {"G3_TARGET_ITEMS": 8, "CHOL_MERGE": mg}) for m in ("bf16x3", "f16x2") for mg in ("0", "1")]
    return [pytest.param(m, kn, id=f"{name}-{m}") for name, m, kn in out]


@pytest.mark.parametrize("mode,knobs", _knob_variants())
@pytest.mark.parametrize("K", [1536, 640])
def test_knobs(ops, mats, monkeypatch, K, mode, knobs):
    _env(monkeypatch, mode, **knobs)
    _check(ops, mats(K), mode, f"{mode} {knobs} K={K}")


# ---- scale ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s", [-10, 10])
@pytest.mark.parametrize("K", [640, 1536])
def test_scaled_by_a_power_of_four(ops, mats, monkeypatch, K, s, mode):
    """4^s A gives 2^-s U: both f16x2 scale exponents move by 10 and the planes hold the same fp16 values."""
    _env(monkeypatch, mode)
    _check(ops, mats(K), mode, f"{mode} 4^{s} A K={K}", s=s)


# ---- batch ----------------------------------------------------------------------------------------------------------
SENTINEL = -12345.5


def _batch(ops, dev, mats_, lbs):
    """Problems at padded strides (K K + 256 / K K + 512) in one chain -> (U [n, K, K], info); pads keep SENTINEL."""
    n, K = len(mats_), mats_[0].shape[0]
    Abuf = torch.full((n, K * K + 256), SENTINEL, dtype=torch.float32, device=dev)
    Ubuf = torch.full((n, K * K + 512), SENTINEL, dtype=torch.float32, device=dev)
    A = Abuf[:, :K * K].view(n, K, K)
    U = Ubuf[:, :K * K].view(n, K, K)
    for b, m in enumerate(mats_):
        A[b].copy_(m)
    _poison_workspace(ops, dev, K, n)
    info = ops.cholesky_inverse_upper_batched(A, U, min_eig_lb=None if lbs is None else torch.cat(lbs).contiguous())
    torch.cuda.synchronize()
    assert bool((Abuf[:, K * K:] == SENTINEL).all()) and bool((Ubuf[:, K * K:] == SENTINEL).all()), "a pad was written"
    return U, info.cpu().numpy().tolist()


@pytest.mark.parametrize("zero_pivot", [False, True], ids=["pd", "zero-pivot"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [640, 1536])
def test_batch_of_three(ops, dev, mats, monkeypatch, K, mode, zero_pivot):
    """Three problems from three seeds, problem 1 scaled by 4^5; every problem equals its own reference.  With a zero
    pivot placed in problem 1: info = [0, j + 1, 0], U[1] = I, the neighbours still exact."""
    _env(monkeypatch, mode)
    ms = [mats(K, K + b) for b in range(3)]
    trip = [(ms[0].A, ms[0].want, ms[0].lb), ms[1].scaled(5), (ms[2].A, ms[2].want, ms[2].lb)]
    As = [t[0] for t in trip]
    j = K - 70
    if zero_pivot:
        As[1] = As[1].clone()
        As[1][j, j] = float(ex.with_zero_pivot(ms[1].A64, ms[1].R, j)[j, j] * 4.0 ** 5)
    U, info = _batch(ops, dev, As, [t[2] for t in trip] if mode == "f16x2" else None)
    assert info == ([0, j + 1, 0] if zero_pivot else [0, 0, 0])
    for b in range(3):
        want = torch.eye(K, dtype=torch.float32, device=dev) if zero_pivot and b == 1 else trip[b][1]
        ex.assert_exact(U[b], want, what=f"{mode} batch K={K} problem {b}")


# ---- zero and negative pivots ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("factor", [1, 2], ids=["zero", "negative"])
@pytest.mark.parametrize("K", [640, 1536])
def test_a_pivot_that_the_updates_make_non_positive(ops, dev, mats, monkeypatch, K, factor, mode):
    """A - factor R[j][j]^2 e_j e_j^T: the diagonal entry stays positive, the pivot becomes exactly 0 (or -R[j][j]^2)
    through the updates alone, at the edges of the 32-row sub-blocks, the 128-row panels and the 512-row block rows:
    info = j + 1 and U = I, exactly."""
    _env(monkeypatch, mode)
    m = mats(K)
    eye = torch.eye(K, dtype=torch.float32, device=dev)
    js = [p % K for p in ZERO_PIVOTS]
    # column j of R has off-diagonal entries for all but the first few j: there the DIAGONAL of the input stays positive
    assert sum(ex.with_zero_pivot(m.A64, m.R, j, 1)[j, j] > 0 for j in js) >= 6
    for j in js:
        B = ex.with_zero_pivot(m.A64, m.R, j, factor)
        A = m.A.clone()
        A[j, j] = float(B[j, j])
        assert float(A[j, j]) == B[j, j]
        U, info = _run(ops, A, m.lb if mode == "f16x2" else None)
        assert info == j + 1, (j, info)
        ex.assert_exact(U, eye, what=f"{mode} K={K} pivot {j} x{factor}")


# ---- witnesses: the variant reached other code ----------------------------------------------------------------------
def _witnesses():
    """(variant, baseline), both (mode, knobs): every variant above that changes the order of a sum by design."""
    out = [("planes-vs-f32", ("bf16x3", {}), ("f32", {})),
           ("f16x2-vs-bf16x3", ("f16x2", {}), ("bf16x3", {})),
           ("merge1-vs-0", ("bf16x3", {"CHOL_MERGE": "1"}), ("bf16x3", {"CHOL_MERGE": "0"})),
           ("merge1-vs-0-f16x2", ("f16x2", {"CHOL_MERGE": "1"}), ("f16x2", {"CHOL_MERGE": "0"})),
           ("trinv-div", ("f32", {"CHOL_TRINV": "div"}), ("f32", {})),
           ("trinv-div-planes", ("bf16x3", {"CHOL_TRINV": "div"}), ("bf16x3", {}))]
    for m in MODES:
        dflt = 256 if m == "f32" else 512
        out += [(f"nb{o}-{i}-{m}", (m, {"CHOL_NBO": o, "CHOL_NBI": i}), (m, {})) for o, i in NB_PAIRS if (o, i) != (dflt, dflt)]
    for mg in ("0", "1"):
        out.append((f"loop-chunk-merge{mg}", ("bf16x3", {"G3_LOOP": "chunk", "CHOL_MERGE": mg}), ("bf16x3", {"CHOL_MERGE": mg})))
        for m in ("bf16x3", "f16x2"):
            out.append((f"items8-merge{mg}-{m}", (m, {"G3_TARGET_ITEMS": 8, "CHOL_MERGE": mg}), (m, {"CHOL_MERGE": mg})))
    return [pytest.param(name, v, b, id=name) for name, v, b in out]


# (witness, K) -> why the chain ignores the knob at this size: those runs must give the BASELINE's bits
_NO_LAUNCH_ABOVE_8 = ("K = 640 has one block row with products, 20 k-chunks in 3 tiles: pieces are at least 2 chunks, the two "
                      "separate launches have 4 and 6 items, and the merged one is cut under the separate tables' slab "
                      "budget (6) to 5 items -- a cap of 8 items binds nowhere and the tables are the default's")
IGNORED = {(f"items8-merge{mg}-{m}", 640): _NO_LAUNCH_ABOVE_8 for mg in ("0", "1") for m in ("bf16x3", "f16x2")}


def test_the_item_cap_of_8_changes_the_tables_at_1536_only(monkeypatch):
    """The host side of IGNORED: the plan's (launches, items, slabs) with and without QT_G3_TARGET_ITEMS=8."""
    from quantool_amd.hip import _lib

    def counts(K, merged):
        out = (ctypes.c_longlong * 5)()
        assert _lib.load().qt_chol_g3_plan_check(K, merged, 1, ctypes.cast(out, ctypes.c_void_p)) == 0
        return list(out)[:3]

    monkeypatch.delenv("QT_G3_TARGET_ITEMS", raising=False)
    dflt = {(K, mg): counts(K, mg) for K in (640, 1536) for mg in (0, 1)}
    monkeypatch.setenv("QT_G3_TARGET_ITEMS", "8")
    for (K, mg), c in dflt.items():
        assert (counts(K, mg) == c) == (K == 640), (K, mg, c, counts(K, mg))


@pytest.mark.parametrize("name,variant,baseline", _witnesses())
def test_witness_the_variant_changes_bits_on_a_graded_hessian(case, ops, monkeypatch, name, variant, baseline):  # noqa: F811
    runs = []
    for mode, knobs in (variant, baseline):
        _env(monkeypatch, mode, **knobs)
        U, info = _run(ops, case["A"], case["lb"] if mode == "f16x2" else None)
        assert info == 0
        runs.append(U)
    same = torch.equal(runs[0], runs[1])
    print(f"\n[witness] K={case['K']} {name}: {variant} vs {baseline}: bits {'EQUAL' if same else 'differ'}")
    why = IGNORED.get((name, case["K"]))
    if why:
        assert same, f"{name} is listed as ignored at K={case['K']} ({why}) but changed the bits"
    else:
        assert not same, f"{variant} gave the bits of {baseline}: the knob did not reach other code"
