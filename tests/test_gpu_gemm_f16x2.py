"""The TN product on TWO fp16 planes per operand and three plane products (csrc/gemm3_tn.hip, G3_F16X2), through the
test face ``ops.gemm3_tn_f16x2``, against an fp64 product of the same fp32 inputs.

The criterion is the project's own for a product that replaces the f32 chain (``test_gemm3_error_is_fp32_class``):
the maximum of err / sum_k |a||b| is at most max(4 x the same figure of ``sgemm_tn`` on the same inputs, 2 * 2^-24).
The reference for the bar is the f32 chain, never the kernel under test."""
import numpy as np
import pytest
import torch

from .test_gpu_gemm3 import EPS, _bound, _inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from quantool_amd.hip import ops as _ops

    return _ops


def _absmax(X):
    return float(np.abs(X).max())


def _run(ops, dev, A, B, kind, bound_a, bound_b):
    """-> A^T B as float64 of the fp32 result (kind 0 subtracts from a zero C)."""
    M, N = A.shape[1], B.shape[1]
    C = torch.zeros((M, N), dtype=torch.float32, device=dev) if kind == 0 else \
        torch.full((M, N), float("nan"), dtype=torch.float32, device=dev)
    ops.gemm3_tn_f16x2(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), C, bound_a, bound_b, kind=kind)
    torch.cuda.synchronize()
    got = C.cpu().numpy()
    return -got if kind == 0 else got


def _figures(ops, dev, A, B, got):
    """(max err / sum|a||b| of `got`, the same of sgemm_tn on the same inputs)"""
    ref = A.astype(np.float64).T @ B.astype(np.float64)
    S = ops.sgemm_tn(torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), None, 1)
    torch.cuda.synchronize()
    scale = _bound(A, B)
    r2 = float((np.abs(got.astype(np.float64) - ref) / scale).max())
    rs = float((np.abs(S.cpu().numpy().astype(np.float64) - ref) / scale).max())
    return r2, rs


# SUB on whole tiles; ragged (edge tiles in both directions); split-k SET through slabs and the ordered reduction
SHAPES = [(0, 256, 512, 512), (0, 128, 264, 520), (1, 1024, 256, 768)]


@pytest.mark.parametrize("kind,k,M,N", SHAPES)
def test_f16x2_error_is_fp32_class_and_deterministic(ops, dev, kind, k, M, N):
    A, B = _inputs(k, M, N, seed=k + M + N, spread=2.0)
    got = _run(ops, dev, A, B, kind, _absmax(A), _absmax(B))
    r2, rs = _figures(ops, dev, A, B, got)
    print(f"\nkind {kind} k={k} {M}x{N}: max error / sum|a||b|: f16x2 {r2 / EPS:.2f} eps, sgemm {rs / EPS:.2f} eps")
    assert np.isfinite(got).all()
    assert r2 <= max(4 * rs, 2 * EPS), (r2 / EPS, rs / EPS)
    again = _run(ops, dev, A, B, kind, _absmax(A), _absmax(B))
    assert np.array_equal(got, again), "two runs differ"


@pytest.mark.parametrize("kind,k,M,N", [(0, 128, 264, 520), (1, 512, 256, 512)])
def test_f16x2_batch_of_three_equals_three_single_calls(ops, dev, kind, k, M, N):
    """One launch for three problems at padded batch strides, each with its own bounds (its own scale exponents)."""
    n = 3
    Ab = torch.zeros((n, k + 8, M), dtype=torch.float32, device=dev)[:, :k]
    Bb = torch.zeros((n, k + 4, N), dtype=torch.float32, device=dev)[:, :k]
    Cb = torch.zeros((n, M + 1, N), dtype=torch.float32, device=dev)[:, :M]
    singles, ba, bb = [], [], []
    for b in range(n):
        A, B = _inputs(k, M, N, seed=31 + b, spread=2.0)
        A *= np.float32(4.0 ** b)                      # different exponents per problem
        Ab[b].copy_(torch.from_numpy(A))
        Bb[b].copy_(torch.from_numpy(B))
        ba.append(_absmax(A))
        bb.append(_absmax(B))
        singles.append(_run(ops, dev, A, B, kind, ba[-1], bb[-1]))
    assert Ab.stride(0) == (k + 8) * M and Cb.stride(0) == (M + 1) * N
    ops.gemm3_tn_f16x2(Ab, Bb, Cb, ba, bb, kind=kind)
    torch.cuda.synchronize()
    for b in range(n):
        got = Cb[b].cpu().numpy()
        assert np.array_equal(-got if kind == 0 else got, singles[b]), f"problem {b}"


def test_f16x2_entries_exactly_at_the_declared_bound(ops, dev):
    """The scale puts the declared bound at 2^3 (hi * 2^11 = 2^14): entries AT the bound stay finite and correct."""
    k, M, N = 256, 512, 512
    A, B = _inputs(k, M, N, seed=5, spread=2.0)
    bound = float(2.0 ** np.ceil(np.log2(_absmax(A))))
    A[::7, ::5] = np.float32(bound)
    A[3::7, 1::5] = np.float32(-bound)
    B[::3, ::11] = np.float32(_absmax(B))
    got = _run(ops, dev, A, B, 0, bound, _absmax(B))
    r2, rs = _figures(ops, dev, A, B, got)
    print(f"\nentries at the bound: f16x2 {r2 / EPS:.2f} eps, sgemm {rs / EPS:.2f} eps")
    assert np.isfinite(got).all()
    assert r2 <= max(4 * rs, 2 * EPS), (r2 / EPS, rs / EPS)


def test_f16x2_bound_2_to_the_6_too_loose(ops, dev):
    """A declared bound 64 times the true maximum -- what the lambda_min bound gives the Y operand in practice -- still
    meets the fp32-class criterion: the planes then sit six binades lower in fp16's range, above its subnormals for all
    but the smallest elements, and those keep an absolute error far below the sum's."""
    k, M, N = 256, 512, 512
    A, B = _inputs(k, M, N, seed=9, spread=2.0)
    got = _run(ops, dev, A, B, 0, _absmax(A), 64.0 * _absmax(B))
    r2, rs = _figures(ops, dev, A, B, got)
    print(f"\nB bound 2^6 too loose: f16x2 {r2 / EPS:.2f} eps, sgemm {rs / EPS:.2f} eps")
    assert r2 <= max(4 * rs, 2 * EPS), (r2 / EPS, rs / EPS)
    got = _run(ops, dev, A, B, 0, 64.0 * _absmax(A), 64.0 * _absmax(B))
    r2, rs = _figures(ops, dev, A, B, got)
    print(f"both bounds 2^6 too loose: f16x2 {r2 / EPS:.2f} eps, sgemm {rs / EPS:.2f} eps")
    assert r2 <= max(4 * rs, 2 * EPS), (r2 / EPS, rs / EPS)


def _subnormals_preserved(ops, dev):
    """One 32 x 32 product of a plane of fp16 SUBNORMALS against ones: with bound_a = 1 the scale is 2^3, so an A of
    2^-20 everywhere is split into hi = 2^-17 (a subnormal fp16, exact) and lo' = 0; B = 1 is the normal 2^3.  The exact
    result is k * 2^-20; a pipeline that flushes subnormal fp16 (in the conversion, the LDS path or the MFMA) gives 0."""
    k = 128
    A = np.full((k, 32), 2.0 ** -20, dtype=np.float32)
    B = np.ones((k, 32), dtype=np.float32)
    got = _run(ops, dev, A, B, 1, 1.0, 1.0)
    if np.all(got == k * 2.0 ** -20):
        return True
    assert np.all(got == 0.0), f"neither preserved nor flushed: {np.unique(got)}"
    return False


def test_f16x2_small_elements_error_floor(ops, dev):
    """One column of A whose entries lie 2^-20 below the declared bound (|a| in [2^-21, 2^-20] * bound_a).

    Derivation of the floor.  The planes hold xs = a * 2^e with the bound at 2^3, so these entries are |xs| <= 2^-17:
    below fp16's smallest normal 2^-14.
      * subnormals preserved: hi = fp16(xs) has the subnormal spacing 2^-24, so |xs - hi| <= 2^-25; that residual
        times 2^11 is <= 2^-14, again subnormal, rounded to spacing 2^-24: an error of <= 2^-25 in lo', i.e. 2^-36 of
        xs, i.e. 2^-39 of the scaled bound in the worst case and, as independent roundings uniform in +-2^-36, a sum of
        k of them of about sqrt(k / 3) * 2^-36 -- for k >= 128 several times below k * 2^-40 * 2^3.  The other operand
        adds 2^-24 relative to a term that is itself 2^-20 of the bound (2^-44), the fp32 accumulation the same order.
        Floor asserted: err <= 2^-40 * bound_a * sum_k |b|.
      * subnormals flushed: a split that then carries such an entry in the lo' plane alone (xs * 2^11 <= 2^-6, normal,
        11 significant bits) leaves 2^-12 of 2^-17 = 2^-29 of the scaled value per term; the floor asserted on such a
        chip is 2^-29 * bound_a * sum_k |b|, and the split as written (hi first) would have to change to meet it.
    Which of the two this GPU does is probed first and printed (MI355X: preserved; 2^-41.5 observed)."""
    preserved = _subnormals_preserved(ops, dev)
    print(f"\nfp16 subnormal plane entries are {'PRESERVED' if preserved else 'FLUSHED'} by split + LDS + MFMA")
    k, M, N = 256, 256, 256
    A, B = _inputs(k, M, N, seed=13, spread=2.0)
    bound_a = float(2.0 ** np.ceil(np.log2(_absmax(A))))
    rng = np.random.default_rng(2)
    col = 77
    A[:, col] = (rng.uniform(0.5, 1.0, k) * rng.choice([-1.0, 1.0], k) * bound_a * 2.0 ** -20).astype(np.float32)
    got = _run(ops, dev, A, B, 0, bound_a, _absmax(B))
    ref = A[:, col].astype(np.float64) @ B.astype(np.float64)
    err = np.abs(got[col].astype(np.float64) - ref)
    unit = bound_a * np.abs(B).astype(np.float64).sum(axis=0)
    floor = 2.0 ** -40 if preserved else 2.0 ** -29
    worst = float((err / unit).max())
    print(f"small column: max err / (bound_a * sum|b|) = 2^{np.log2(max(worst, 1e-300)):.2f}; floor 2^{np.log2(floor):.0f}")
    assert (err <= floor * unit).all(), (worst, floor)
    # the rest of the product is untouched by the small column
    r2, rs = _figures(ops, dev, A, B, got)
    assert r2 <= max(4 * rs, 2 * EPS), (r2 / EPS, rs / EPS)
