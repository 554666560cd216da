"""The GPTQ column sweep (csrc/sweep.hip) against ``oracle/gptq_oracle.c`` over what the entry points accept:
every bit width the schemes use, both block kernels (``QT_SWEEP_BLOCK``), every far-update batch length
(``QT_SWEEP_BATCH``), the row and column edges of a workgroup and of a 128-column block, dead columns, and
``qt_gptq_sweep_grouped`` called directly with a padded factor stride.

Bars (the same as ``test_gpu_kernels.py::test_sweep_bit_exact_given_same_U``): given the same factor U
the integer levels and the dequantised W are bit-exact; the per-row loss agrees to 1e-6 (``1 / d^2`` is formed once
per column on the device, sweep.hip: "tolerance 1e-6, not part of the bit-exact contract").  Every case is small:
the shapes are chosen to reach code paths, not job sizes.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_sweep_fused import chain_launches, fused_launches, sweep_launches
from tests.util import synth_activations, synth_weight

pytestmark = pytest.mark.gpu

SWEEP_ENV = ("QT_SWEEP_FUSED", "QT_SWEEP_LANES", "QT_SWEEP_BLOCK", "QT_SWEEP_BATCH", "QT_SWEEP_FAR", "QT_SGEMM_RING",
             "QT_SGEMM_RING_MIN_TILES")


@pytest.fixture(autouse=True)
def _default_sweep_form(monkeypatch):
    """Every test starts from the default kernel form, whatever the caller's environment holds."""
    for name in SWEEP_ENV:
        monkeypatch.delenv(name, raising=False)


_FACTORS = {}


def _factor(oracle, K, seed, dead=()):
    """U = chol((H + damp)^-1, upper) in fp64, rounded to fp32, for synthetic activations; cached per input."""
    key = (K, seed, tuple(dead))
    if key not in _FACTORS:
        xb = synth_activations(2 * K, K, seed=seed)
        if dead:
            xb[:, list(dead)] = 0
        H = oracle.hessian_from_gram(oracle.gram_f64(xb), 4)
        Hd, dmask, _ = oracle.hessian_dead_and_damp(H)
        Un = oracle.cholesky_inverse_upper_f64(Hd).astype(np.float32)
        _FACTORS[key] = (Un, dmask)
    return _FACTORS[key]


def _group_size(K, gs):
    return K if gs <= 0 else gs


def _permuted_g_idx(K, gs, seed):
    g_idx = (np.arange(K) // _group_size(K, gs)).astype(np.int32)
    return g_idx[np.random.default_rng(seed).permutation(K)]      # as under activation ordering


def _case(oracle, R, K, gs, sym, bits, seed=None, dead=(), zero_group=None):
    """Inputs and the oracle's outputs of one sweep.  ``dead``: activation columns zeroed (and W there, as
    ``quantize_weight`` does).  ``zero_group = (rows, g)``: W is zero wherever ``g_idx == g`` in those rows, and
    the qparams are taken from W gathered by group, so that group's scale is the observer's F32_EPS floor."""
    seed = R + K + bits if seed is None else seed
    Wn = synth_weight(R, K, seed=seed)
    Un, dmask = _factor(oracle, K, seed + 1, dead)
    g_idx = _permuted_g_idx(K, gs, seed)
    if dead:
        assert sorted(np.flatnonzero(dmask).tolist()) == sorted(dead)
        Wn[:, dmask] = 0
    if zero_group is None:
        scale, zp = oracle.minmax_qparams(Wn, gs, sym, bits)
    else:
        rows, g = zero_group
        Wn[np.ix_(rows, np.flatnonzero(g_idx == g))] = 0
        scale, zp = oracle.minmax_qparams(Wn[:, np.argsort(g_idx, kind="stable")], gs, sym, bits)
        assert np.all(scale[rows, g] == oracle.F32_EPS)
    Qo, Wo, lo = oracle.gptq_sweep_c(Wn, Un, scale, zp, g_idx, 128, bits)
    return dict(R=R, K=K, bits=bits, W=Wn, U=Un, scale=scale, zp=zp, g_idx=g_idx, Qo=Qo, Wo=Wo, lo=lo)


def _assert_oracle_hits_the_clamp(c):
    qmin, qmax = -(1 << (c["bits"] - 1)), (1 << (c["bits"] - 1)) - 1
    assert c["Qo"].min() == qmin and c["Qo"].max() == qmax, (int(c["Qo"].min()), int(c["Qo"].max()))


def _check(ops, dev, c):
    """Run ``ops.gptq_sweep`` on the case and hold it to the oracle's outputs.  At 2 and 8 bits the oracle's levels
    must touch both ends of the range, so the clamp and the int8 cast are exercised (seeds are chosen for it)."""
    bits = c["bits"]
    qmin, qmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if bits in (2, 8):
        _assert_oracle_hits_the_clamp(c)
    W = torch.from_numpy(c["W"].copy()).to(dev)
    Qt, loss = ops.gptq_sweep(W, torch.from_numpy(c["U"]).to(dev),
                              torch.from_numpy(np.ascontiguousarray(c["scale"].T)).to(dev),
                              torch.from_numpy(np.ascontiguousarray(c["zp"].T)).to(dev),
                              torch.from_numpy(c["g_idx"]).to(dev), 128, bits)
    torch.cuda.synchronize()
    assert int(Qt.min()) >= qmin and int(Qt.max()) <= qmax
    q = Qt.cpu().numpy().T
    assert np.array_equal(q, c["Qo"]), f"{(q != c['Qo']).sum()} of {q.size} levels differ"
    np.testing.assert_array_equal(W.cpu().numpy(), c["Wo"])          # dequantised weights, bit-exact
    np.testing.assert_allclose(loss.cpu().numpy(), c["lo"], rtol=1e-6)
    return q, W.cpu().numpy()


# ------------------------------------------------------------------------------------ a. width x scheme
# 1100 = 8 blocks + 76 columns (channel-wise: 1100 has no divisor among the group sizes), 1152 = 9 blocks; with the
# default batch of 4 both have far updates that carry four chains.  R = 130: a ragged workgroup of either kernel.
WIDTH_SCHEME = [(bits, sym, gs) for bits in (2, 3, 4, 5, 8) for sym in (True, False) for gs in (64, 128, -1)
                # every width with both symmetries; each (width, symmetry) channel-wise and with one of the group
                # sizes (64 and 128 alternate), so every width meets both group sizes
                if gs == -1 or (gs == 64) == ((bits + sym) % 2 == 0)]


@pytest.mark.parametrize("bits,sym,gs", WIDTH_SCHEME)
def test_width_and_scheme(ops, oracle, dev, bits, sym, gs):
    _check(ops, dev, _case(oracle, 130, 1100 if gs == -1 else 1152, gs, sym, bits))


# ------------------------------------------------------------------------------------ b. row and column edges
# Rows: one row, fewer than a quad's lanes, either side of the quad kernel's 64-row and the row kernel's 128-row
# workgroup, two full row-kernel workgroups plus one row.  Columns: a lone column group (4), single ragged blocks
# (20, 124), a last block of one column group (132: a near update with N = 4; 516 and 1028: a far update with
# N = 4), batches that end on a block boundary (640, 1028's second) and inside a ragged block (1156).
EDGE_R = (1, 3, 63, 64, 65, 127, 129, 257)
EDGE_K = (4, 20, 124, 132, 516, 640, 1028, 1156)


def _edge_gs(K):
    return {640: 128, 20: 4}.get(K, -1)       # group size -1 where K is not a multiple of the group


@pytest.mark.parametrize("bits,sym", [(4, True), (8, False)])
@pytest.mark.parametrize("K", EDGE_K)
@pytest.mark.parametrize("R", EDGE_R)
def test_row_and_column_edges(ops, oracle, dev, R, K, bits, sym):
    # (one row, 124 columns, 8 bits: the default seed's levels stop at -127; seed 1 reaches both ends of the range)
    seed = 1 if (R, K, bits) == (1, 124, 8) else None
    _check(ops, dev, _case(oracle, R, K, _edge_gs(K), sym, bits, seed=seed))


# ------------------------------------------------------------------------------------ c. both block kernels
ROW_FORM = [(129, 1156, -1, False, 8), (129, 1152, 64, True, 2), (130, 1100, -1, False, 2), (130, 1152, 128, True, 8),
            (257, 516, -1, True, 4), (65, 132, -1, False, 8), (127, 640, 128, False, 3), (1, 4, -1, True, 4),
            (3, 20, 4, False, 8), (128, 124, -1, True, 5), (200, 1028, -1, False, 4)]


@pytest.mark.parametrize("R,K,gs,sym,bits", ROW_FORM)
def test_row_per_lane_kernel_against_the_oracle(ops, oracle, dev, monkeypatch, R, K, gs, sym, bits):
    """``QT_SWEEP_BLOCK=row`` (``sweep_block_kernel``): the form the quad kernel's comments define their own bits
    by.  Held to the oracle itself, and to the quad kernel on the same inputs."""
    c = _case(oracle, R, K, gs, sym, bits)
    q_quad, w_quad = _check(ops, dev, c)
    monkeypatch.setenv("QT_SWEEP_BLOCK", "row")
    q_row, w_row = _check(ops, dev, c)
    assert np.array_equal(q_row, q_quad) and np.array_equal(w_row, w_quad)


# ------------------------------------------------------------------------------------ d. batch length
@pytest.mark.parametrize("bits,sym", [(4, True), (8, False)])
@pytest.mark.parametrize("K", [1152, 1156])
@pytest.mark.parametrize("batch", [1, 2, 3, 8])
def test_far_update_batch_length(ops, oracle, dev, monkeypatch, batch, K, bits, sym):
    """``QT_SWEEP_BATCH``: how many 128-deep chains one far update carries.  Nine blocks (1152) and nine plus a
    ragged one (1156): with 8 the first far update folds eight chains and leaves N = 128 / 132 columns; with 1
    every update is a single chain; 2 and 3 end the last batch at and before the matrix edge."""
    monkeypatch.setenv("QT_SWEEP_BATCH", str(batch))
    _check(ops, dev, _case(oracle, 130, K, 128 if K == 1152 else -1, sym, bits))


@pytest.mark.parametrize("batch,form", [(3, "chain"), (8, "chain"), (3, "fused"), (8, "fused")],
                         ids=["3", "8", "3-fused", "8-fused"])
def test_chained_far_update_on_the_ring_kernel(ops, oracle, dev, monkeypatch, batch, form):
    """R = 256, K = 1152: whole 128 x 128 tiles, so with ``QT_SGEMM_RING_MIN_TILES=1`` every update product of the
    chain of launches (``QT_SWEEP_FUSED=0``: a shape of whole tiles takes the fused form otherwise) -- the chained
    far updates (three or eight chains) included -- is served by ``sgemm_ring_kernel``.  "fused": the same case in
    the form the default takes, whose far update walks the same tiles inside ``sweep_fused_kernel``'s launch.  The
    count of block-kernel launches tells which of the two ran."""
    monkeypatch.setenv("QT_SWEEP_BATCH", str(batch))
    monkeypatch.setenv("QT_SGEMM_RING", "1")
    monkeypatch.setenv("QT_SGEMM_RING_MIN_TILES", "1")
    if form == "chain":
        monkeypatch.setenv("QT_SWEEP_FUSED", "0")
    c = _case(oracle, 256, 1152, 128, False, 8)
    _, launches = sweep_launches(lambda: _check(ops, dev, c))
    assert launches == (chain_launches(1152) if form == "chain" else fused_launches(1152, batch))


# ------------------------------------------------------------------------------------ e. dead columns
@pytest.mark.parametrize("form", ["quad", "row"])
@pytest.mark.parametrize("bits,sym", [(4, True), (8, False), (4, False)])
def test_dead_columns_and_an_all_zero_group(ops, oracle, dev, monkeypatch, bits, sym, form):
    """Two activation columns that never fire (one of them in the ragged last block, K = 1100 = 8 * 128 + 76): the
    Hessian's dead flags, W zeroed there, and the sweep must return the level of 0.0 -- the zero point -- and a
    dequantised weight of exactly (q - zp) * scale.  One group of the first rows is all zero as well: its scale
    is the observer's F32_EPS floor, and whatever error feedback puts there is clamped."""
    if form == "row":
        monkeypatch.setenv("QT_SWEEP_BLOCK", "row")
    R, K, gs = 70, 1100, 44
    dead = (300, 1090)
    c = _case(oracle, R, K, gs, sym, bits, dead=dead, zero_group=(np.arange(9), 7))
    q, w = _check(ops, dev, c)
    for d in dead:
        g = c["g_idx"][d]
        np.testing.assert_array_equal(q[:, d].astype(np.float32), c["zp"][:, g])
        np.testing.assert_array_equal(w[:, d], (q[:, d].astype(np.float32) - c["zp"][:, g]) * c["scale"][:, g])
        assert np.all(w[:, d] == 0)


# ------------------------------------------------------------------------------------ f. the grouped entry point
def _grouped_rows(n):
    sizes = [128 if g % 2 == 0 else 256 for g in range(n - 1)] + [200]      # ends 128, 384, 512, ..., last + 200
    return np.cumsum(sizes).tolist()


def _grouped_gs(K):
    return 128 if K % 128 == 0 else 68        # 1156 = 17 * 68


@functools.lru_cache(maxsize=2)      # the parameter that changes least often is the case's: a case is built once
def _grouped_case(oracle, row_end, K, bits, sym):
    """Inputs of one stacked sweep and, per group, the oracle's outputs for that group's rows alone (its own factor
    and ``g_idx``).  At 8 bits every group's levels must reach both ends of the range."""
    n = len(row_end)
    gs = _grouped_gs(K)
    row_begin = (0,) + row_end[:-1]
    Wn = synth_weight(row_end[-1], K, seed=n + K + bits)
    scale, zp = oracle.minmax_qparams(Wn, gs, sym, bits)
    g_idx = np.stack([_permuted_g_idx(K, gs, 100 + g) for g in range(n)])
    factors = [_factor(oracle, K, 1000 + g)[0] for g in range(n)]
    qmin, qmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    want = []
    for g in range(n):
        r0, r1 = row_begin[g], row_end[g]
        Qo, Wo, lo = oracle.gptq_sweep_c(Wn[r0:r1], factors[g], scale[r0:r1], zp[r0:r1], g_idx[g], 128, bits)
        if bits == 8:
            assert Qo.min() == qmin and Qo.max() == qmax
        want.append((Qo, Wo, lo))
    return dict(row_end=list(row_end), row_begin=list(row_begin), K=K, bits=bits, W=Wn, scale=scale, zp=zp, g_idx=g_idx,
                factors=factors, want=want)


def _check_grouped(ops, dev, c):
    """``ops.gptq_sweep_grouped`` on the case, the factors as [K, K] slices of a wider buffer whose gaps hold NaN; each
    group's rows of the levels, of W and of the loss against the oracle on that group alone."""
    n, K, bits = len(c["row_end"]), c["K"], c["bits"]
    pad = 256
    ubuf = torch.full((n, K * K + pad), float("nan"), dtype=torch.float32, device=dev)
    U = ubuf[:, :K * K].view(n, K, K)
    for g in range(n):
        U[g].copy_(torch.from_numpy(c["factors"][g]))
    assert U.stride(0) > K * K
    W = torch.from_numpy(c["W"].copy()).to(dev)
    Qt, loss = ops.gptq_sweep_grouped(W, U, c["row_end"], torch.from_numpy(np.ascontiguousarray(c["scale"].T)).to(dev),
                                      torch.from_numpy(np.ascontiguousarray(c["zp"].T)).to(dev),
                                      torch.from_numpy(c["g_idx"]).to(dev), 128, bits)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ubuf[:, K * K:]).all()), "the gap between two factors was written"
    qmin, qmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    assert int(Qt.min()) >= qmin and int(Qt.max()) <= qmax
    q, w, ls = Qt.cpu().numpy().T, W.cpu().numpy(), loss.cpu().numpy()
    for g, (Qo, Wo, lo) in enumerate(c["want"]):
        r0, r1 = c["row_begin"][g], c["row_end"][g]
        assert np.array_equal(q[r0:r1], Qo), f"group {g}: {(q[r0:r1] != Qo).sum()} of {Qo.size} levels differ"
        np.testing.assert_array_equal(w[r0:r1], Wo, err_msg=f"group {g}")
        np.testing.assert_allclose(ls[r0:r1], lo, rtol=1e-6, err_msg=f"group {g}")


@pytest.mark.parametrize("form", ["quad", "row"])
@pytest.mark.parametrize("bits,sym", [(4, True), (8, False)])
@pytest.mark.parametrize("K", [640, 1156])
@pytest.mark.parametrize("n", [2, 5, 16])
def test_grouped_sweep_each_group_against_the_oracle(ops, oracle, dev, monkeypatch, n, K, bits, sym, form):
    """``qt_gptq_sweep_grouped`` called directly: every group has its own factor (its own activations) and its own
    permuted ``g_idx``; the factors are [K, K] slices of a wider buffer whose gaps hold NaN; the last group is
    ragged (200 rows: a full update tile, a full quad workgroup and parts of both).  Each group's rows of the
    levels, of W and of the loss are held to ``gptq_sweep_c`` on that group alone.  n = 16 is SG_MAX_GROUPS."""
    if form == "row":
        monkeypatch.setenv("QT_SWEEP_BLOCK", "row")
    _check_grouped(ops, dev, _grouped_case(oracle, tuple(_grouped_rows(n)), K, bits, sym))


def test_grouped_sweep_refuses_bad_boundaries_and_strides(ops, dev):
    """A group boundary that is not a multiple of 128, and a factor stride below K * K, come back as QT_ERR_INVALID
    from the C ABI before anything is launched (the Python wrapper has host checks of its own in front)."""
    from quantool_amd.hip._lib import QT_ERR_INVALID, load

    lib = load()
    R, K, n = 256, 128, 2
    W = torch.ones((R, K), dtype=torch.float32, device=dev)
    U = torch.eye(K, dtype=torch.float32, device=dev).repeat(n, 1, 1).contiguous()
    st = torch.ones((1, R), dtype=torch.float32, device=dev)
    zt = torch.zeros((1, R), dtype=torch.float32, device=dev)
    g_idx = torch.zeros((n, K), dtype=torch.int32, device=dev)
    Qt = torch.full((K, R), 77, dtype=torch.int8, device=dev)
    loss = torch.full((R,), -1.0, dtype=torch.float32, device=dev)
    ws = ops.workspace(lib.qt_gptq_sweep_workspace_bytes(R, K, 128), dev, "sweep")
    stream = torch.cuda.current_stream().cuda_stream

    def call(row_end, stride, groups=n):
        ends = (ctypes.c_int32 * len(row_end))(*row_end)
        rc = lib.qt_gptq_sweep_grouped(W.data_ptr(), R, K, U.data_ptr(), stride, groups, ctypes.cast(ends, ctypes.c_void_p),
                                       st.data_ptr(), zt.data_ptr(), 1, g_idx.data_ptr(), 128, 4, Qt.data_ptr(),
                                       loss.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        return rc, lib.qt_last_error().decode()

    rc, msg = call([100, 256], K * K)
    assert rc == QT_ERR_INVALID and "multiple of 128" in msg
    rc, msg = call([128, 256], K * K - 4)
    assert rc == QT_ERR_INVALID and "strideU" in msg
    rc, msg = call([128, 200], K * K)                      # the last group does not end at R
    assert rc == QT_ERR_INVALID and "R = 256" in msg
    rc, msg = call([128, 256], K * K, groups=17)           # beyond SG_MAX_GROUPS
    assert rc == QT_ERR_INVALID and "n_groups" in msg
    with pytest.raises(ValueError):
        ops.gptq_sweep_grouped(W, U, [100, 256], st, zt, g_idx, 128, 4)
    torch.cuda.synchronize()
    assert bool((Qt == 77).all()) and bool((loss == -1).all()) and bool((W == 1).all())
