"""The factor chain with a lower bound on lambda_min (``cholesky_inverse_upper(..., min_eig_lb=)``): its long block-row
products run on two fp16 planes per operand and three plane products (csrc/cholesky.hip, csrc/gemm3_tn.hip G3_F16X2).

The matrix is the benchmark's kind -- bf16 N(0,1) activations, 1 % of the channels x 10, damp 0.01, static order --
built by ``ops.hessian_prepare``, whose damping term (read back on the device, halved) is the bound.  K = 1536 and the
ragged K = 640, with the products forced on for every step that has one, the way
``test_cholesky_inverse_upper_bf16x3_products`` forces them.

Bars: factor, max|U - U64| / max|U64| <= max(4 x fp32 LAPACK three-step's, 5e-6) (``test_gpu_factor_fullsize``); end
to end, nibble mismatch rate against the oracle swept with the LAPACK factor <= max(5 x the fp64-factor yardstick's,
2e-5)."""
import numpy as np
import pytest
import torch

from .test_gpu_fullsize_oracle import _acts, _gpu_run

pytestmark = pytest.mark.gpu

KS = [1536, 640]


def _force_products(monkeypatch):
    monkeypatch.setenv("QT_CHOL_G3", "1")
    monkeypatch.setenv("QT_CHOL_G3_MIN_CHUNKS", "1")
    monkeypatch.delenv("QT_CHOL_PLANES", raising=False)


@pytest.fixture(scope="module", params=KS)
def case(request, dev, ops, oracle):
    from quantool_amd.engine.gptq_linear import HessianAccumulator

    K = request.param
    T, n_samples = 384, 16
    X = _acts(n_samples * T, K, dev, seed=K + 3)
    acc = HessianAccumulator(K, dev)
    for s in range(n_samples):
        acc.add(X[s * T:(s + 1) * T])
    perm, _ = ops.argsort_desc(ops.hessian_diag(acc.G, acc.n))        # static activation order
    damp = torch.zeros(1, dtype=torch.float32, device=dev)
    A, dead, _ = ops.hessian_prepare(acc.G, acc.n, 0.01, perm, damp_out=damp)
    torch.cuda.synchronize()
    assert not bool(dead.any()) and float(damp.item()) > 0
    Au = np.triu(A.cpu().numpy())
    Hd = np.ascontiguousarray((Au + np.triu(Au, 1).T)[::-1, ::-1])    # the damped Hessian the chain factors
    truth = oracle.cholesky_inverse_upper_f64_lapack(Hd)
    U_lapack, ok = oracle.cholesky_inverse_upper_lapack(Hd)
    assert ok
    return dict(K=K, A=torch.triu(A), lb=damp * 0.5, truth=truth, U_lapack=U_lapack)


def _err(U, truth):
    return float(np.abs(U - truth).max() / np.abs(truth).max())


def _factor(ops, case, bounded=True, A=None, lb=None):
    A = case["A"].clone() if A is None else A.clone()
    lb = case["lb"] if lb is None else lb
    U, info = ops.cholesky_inverse_upper(A, min_eig_lb=lb if bounded else None)
    torch.cuda.synchronize()
    return U, int(info.item())


def test_factor_vs_fp64_and_lapack(case, ops, monkeypatch):
    _force_products(monkeypatch)
    K = case["K"]
    U2, info2 = _factor(ops, case)
    U3, info3 = _factor(ops, case, bounded=False)
    assert info2 == 0 and info3 == 0
    assert bool((torch.tril(U2, -1) == 0).all())
    e2, e3 = _err(U2.cpu().numpy(), case["truth"]), _err(U3.cpu().numpy(), case["truth"])
    e_lap = _err(case["U_lapack"], case["truth"])
    print(f"\n[factor] K={K}: max err / max|U| vs fp64: f16x2 {e2:.3e}, bf16x3 {e3:.3e}, fp32 LAPACK three-step {e_lap:.3e}")
    assert not torch.equal(U2, U3), "the two-plane products were not taken"
    assert e2 <= max(4 * e_lap, 5e-6), (e2, e_lap)


def test_without_a_bound_the_bits_are_those_of_bf16x3(case, ops, monkeypatch):
    _force_products(monkeypatch)
    U_plain, _ = _factor(ops, case, bounded=False)
    monkeypatch.setenv("QT_CHOL_PLANES", "bf16x3")
    U_forced, _ = _factor(ops, case)                 # a bound is given, the mode is forced back
    U_forced_nb, _ = _factor(ops, case, bounded=False)
    assert torch.equal(U_plain, U_forced) and torch.equal(U_plain, U_forced_nb)


def test_forcing_f16x2_without_a_bound_is_an_argument_error(case, ops, monkeypatch):
    from quantool_amd.hip._lib import HipBackendError

    _force_products(monkeypatch)
    monkeypatch.setenv("QT_CHOL_PLANES", "f16x2")
    with pytest.raises(HipBackendError, match="bound"):
        _factor(ops, case, bounded=False)
    U, info = _factor(ops, case)                     # with one it is the default path
    monkeypatch.delenv("QT_CHOL_PLANES")
    U0, _ = _factor(ops, case)
    assert info == 0 and torch.equal(U, U0)


def _batch(ops, dev, mats, lbs):
    """Three problems at padded strides in one chain of launches -> (U [n, K, K], info)."""
    n, K = len(mats), mats[0].shape[0]
    Abuf = torch.zeros((n, K * K + 256), dtype=torch.float32, device=dev)
    Ubuf = torch.zeros((n, K * K + 512), dtype=torch.float32, device=dev)
    A = Abuf[:, :K * K].view(n, K, K)
    U = Ubuf[:, :K * K].view(n, K, K)
    for b, m in enumerate(mats):
        A[b].copy_(m)
    info = ops.cholesky_inverse_upper_batched(A, U, min_eig_lb=torch.cat(lbs).contiguous())
    torch.cuda.synchronize()
    return U, info.cpu().numpy()


def test_batched_equals_single_bit_for_bit(case, ops, dev, monkeypatch):
    """Three problems with different scale exponents (A, 64 A, A / 1024: eR and eY move by 3 and 5 binades)."""
    _force_products(monkeypatch)
    fac = [1.0, 64.0, 1.0 / 1024.0]
    mats = [case["A"] * f for f in fac]
    lbs = [case["lb"] * f for f in fac]
    U, info = _batch(ops, dev, mats, lbs)
    assert (info == 0).all()
    for b in range(3):
        Us, i_s = _factor(ops, case, A=mats[b], lb=lbs[b])
        assert i_s == 0 and torch.equal(U[b], Us), f"problem {b}"


def test_non_pd_problem_in_a_batch(case, ops, dev, monkeypatch):
    """A problem that is not positive definite may fill its planes with inf / NaN: it gets info != 0 and U = I, and its
    neighbours in the batch are the single-call factors."""
    _force_products(monkeypatch)
    K = case["K"]
    bad = case["A"].clone()
    j = K // 3
    bad[j, j] = -1.0
    mats = [case["A"], bad, case["A"] * 4.0]
    lbs = [case["lb"], case["lb"], case["lb"] * 4.0]
    U, info = _batch(ops, dev, mats, lbs)
    assert info[0] == 0 and info[2] == 0 and info[1] == j + 1
    assert torch.equal(U[1], torch.eye(K, dtype=torch.float32, device=dev))
    for b in (0, 2):
        Us, _ = _factor(ops, case, A=mats[b], lb=lbs[b])
        assert torch.equal(U[b], Us), f"neighbour {b}"
        assert bool(torch.isfinite(U[b]).all())
    # a bound that is not a positive number cannot scale Y: that problem alone fails (info = K + 1, U = I)
    U, info = _batch(ops, dev, [case["A"], case["A"]], [case["lb"], case["lb"] * 0.0])
    assert info[0] == 0 and info[1] == K + 1
    assert torch.equal(U[1], torch.eye(K, dtype=torch.float32, device=dev))


def test_nan_poisoned_strict_lower_triangle_is_ignored(case, ops, monkeypatch):
    _force_products(monkeypatch)
    U0, info0 = _factor(ops, case)
    poison = torch.full_like(case["A"], float("nan"))
    poison[::3] = float("inf")
    U1, info1 = _factor(ops, case, A=torch.triu(case["A"]) + torch.tril(poison, -1))
    assert info0 == 0 and info1 == 0
    assert torch.equal(U0, U1)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("offset", [0, 16], ids=["aligned", "off16"])
def test_bounded_entry_points_stay_inside_the_workspace(case, ops, dev, monkeypatch, n, offset):
    """The two plane modes share one size function: with exactly ``*_workspace_bytes()`` between two guards, the bounded
    chain -- two planes per operand, the scale exponents in the third plane's slot -- writes nothing outside it, refuses
    a workspace one byte short, and gives the bits of the call through ``ops`` (``test_gpu_workspace_contract``)."""
    from .test_gpu_workspace_contract import BF16X3_CHAIN, Case, _run, _stream

    K = case["K"]
    fac = [1.0, 16.0][:n]

    def make(dev_):
        return dict(A=torch.stack([case["A"] * f for f in fac]), U=torch.zeros((n, K, K), dtype=torch.float32, device=dev_),
                    info=torch.full((n,), 7, dtype=torch.int32, device=dev_),
                    lb=torch.cat([case["lb"] * f for f in fac]).contiguous())

    def via_ops(ops_, t):
        if n == 1:
            _, t["info"] = ops_.cholesky_inverse_upper(t["A"][0], U_out=t["U"][0], min_eig_lb=t["lb"])
        else:
            t["info"] = ops_.cholesky_inverse_upper_batched(t["A"], t["U"], min_eig_lb=t["lb"])

    if n == 1:
        entry = Case(f"qt_cholesky_inverse_upper_bounded K={K}", "two fp16 planes", make,
                     lambda lib, t: lib.qt_cholesky_inverse_upper_workspace_bytes(K),
                     lambda lib, t, ws, nb: lib.qt_cholesky_inverse_upper_bounded(
                         t["A"].data_ptr(), K, t["U"].data_ptr(), t["info"].data_ptr(), t["lb"].data_ptr(), ws, nb, _stream()),
                     via_ops, ["U", "info"], BF16X3_CHAIN)
    else:
        entry = Case(f"qt_cholesky_inverse_upper_batched_bounded K={K} n={n}", "two fp16 planes", make,
                     lambda lib, t: lib.qt_cholesky_inverse_upper_batched_workspace_bytes(K, n),
                     lambda lib, t, ws, nb: lib.qt_cholesky_inverse_upper_batched_bounded(
                         t["A"].data_ptr(), K * K, K, t["U"].data_ptr(), K * K, t["info"].data_ptr(), n, t["lb"].data_ptr(),
                         ws, nb, _stream()),
                     via_ops, ["U", "info"], BF16X3_CHAIN)
    monkeypatch.delenv("QT_CHOL_PLANES", raising=False)
    _run(entry, dev, ops, monkeypatch, offset)


def test_end_to_end_nibble_mismatch_rate_vs_lapack_factor_oracle(dev, oracle, monkeypatch):
    """256 rows x K = 1536 through ``gptq_quantize_shared`` -- the engine passes the bound by itself -- against the
    oracle swept with the fp32 LAPACK factor.  The sweep is bit-exact given U, so the rate measures the factor."""
    _force_products(monkeypatch)
    R, K = 256, 1536
    Wf, res, keep, Gfull, n = _gpu_run(dev, R, K, n_samples=16, T=384, seed=41)
    assert int(res.info.item()) == 0
    monkeypatch.setenv("QT_CHOL_PLANES", "bf16x3")
    _, _, keep3, _, _ = _gpu_run(dev, R, K, n_samples=16, T=384, seed=41)
    monkeypatch.delenv("QT_CHOL_PLANES")
    assert not torch.equal(keep["U"], keep3["U"]), "the engine did not take the two-plane products"
    H = oracle.hessian_from_gram_f32(Gfull, n)
    perm = keep["perm"].cpu().numpy().astype(np.int64)
    Hd, dead, _ = oracle.hessian_dead_and_damp(H[perm][:, perm], 0.01)
    assert not dead.any()
    truth = oracle.cholesky_inverse_upper_f64_lapack(Hd)
    U_lapack, ok = oracle.cholesky_inverse_upper_lapack(Hd)
    assert ok
    o = oracle.quantize_weight(Wf, H, actorder="static", U_override=U_lapack)
    np.testing.assert_array_equal(res.scale_f32.cpu().numpy(), o["scale"])
    q_gpu = oracle.unpack_int4(res.weight_packed.cpu().numpy(), K)
    rate = float((q_gpu != o["q"]).mean())
    o64 = oracle.quantize_weight(Wf, H, actorder="static", U_override=truth.astype(np.float32))
    rate64 = float((o64["q"] != o["q"]).mean())
    print(f"\n[e2e] K={K} R={R}: nibble mismatch rate GPU (f16x2 factor) vs LAPACK-factor oracle = {rate:.3e}; "
          f"fp64-factor oracle vs LAPACK-factor oracle = {rate64:.3e}")
    assert rate <= max(5 * rate64, 2e-5), (rate, rate64)
