"""The tri-unit loop of ``gemm3_kernel`` (csrc/gemm3_tn.hip: 16 k-rows of all three bf16 planes of both operands per
ring slot, six plane products per phase) against the chunk loop it replaces (``QT_G3_LOOP=chunk``), on the same inputs
in one process, through the C-ABI test face (kind 0: whole tiles, ``C -= A^T B``; kind 1: k split into slabs).

Reference: the fp64 product of the fp32 inputs.  Error measure: max over the outputs of |C - ref| / sum_k |a||b| (the
scale both an fp32 fmaf chain and the plane products are bounded by).  Bound: the tri-unit loop's error <= 2 x the chunk
loop's -- both sum the same six plane products of the same planes into one fp32 accumulator and drop the same 2^-24
terms; only the order of the sum differs, and a reordered fp32 sum of the same terms moves the maximum by far less than
a factor of two.

Shapes: the smallest at which the loop takes another path -- k = 128 (8 tri-units: two trips round the ring of three
plus a two-phase tail, the drain starting in the second trip), k = 256 (16: tail of one), k = 384 (24: no tail); one and
several tiles; a plane pitch that makes the edge tiles clamp their loads; a block-triangular B whose tile columns start
their k range at their own column; a k-split with slabs and the ordered reduction; a batch of two in one launch.
Inputs carry a column scale spread of 10^3 (the factor's columns with x10 outlier channels differ that much), and the
triangular cases exact zeros above the diagonal of B.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def _inputs(k, M, N, seed, tri=False, batch=1):
    rng = np.random.default_rng(seed)

    def one(cols):
        x = rng.standard_normal((batch, k, cols)) * np.exp(rng.uniform(0.0, np.log(1e3), (batch, 1, cols)))
        return x.astype(np.float32)

    A, B = one(M), one(N)
    if tri:
        B *= (np.arange(k)[:, None] >= np.arange(N)[None, :])[None]     # B[k][n] = 0 for k < n, exactly
    return A, B


def _reference(A, B, C0, kind):
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    prod = np.einsum("bkm,bkn->bmn", A64, B64)
    scale = np.einsum("bkm,bkn->bmn", np.abs(A64), np.abs(B64))
    return (C0.astype(np.float64) - prod) if kind == 0 else prod, scale


def _run(ops, dev, A, B, C0, kind, tri, tight):
    """One call for the whole batch (or the single problem); returns the device result."""
    single = A.shape[0] == 1
    At, Bt = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    C = torch.from_numpy(C0.copy()).to(dev) if kind == 0 else torch.full(C0.shape, float("nan"), dtype=torch.float32, device=dev)
    if single:
        ops.gemm3_tn_ex(At[0], Bt[0], C[0], kind, tri=tri, tight=tight)
    else:
        ops.gemm3_tn_ex(At, Bt, C, kind, tri=tri, tight=tight)
    torch.cuda.synchronize()
    return C


def _rel_err(C, ref, scale):
    err = np.abs(C.cpu().numpy().astype(np.float64) - ref)
    assert np.isfinite(err).all()
    ok = scale > 0
    assert (err[~ok] == 0).all()
    return float((err[ok] / scale[ok]).max())


# (k, M, N, kind, tri, tight)
CASES = [
    (128, 256, 256, 0, False, False),     # 8 tri-units: prologue, two bodies, a tail of two, drain inside the body
    (256, 256, 256, 0, False, False),     # 16: tail of one
    (384, 256, 256, 0, False, False),     # 24: no tail
    (256, 512, 768, 0, False, False),     # six workgroups
    (384, 512, 768, 0, False, False),
    (256, 264, 520, 0, False, True),      # plane pitch 520: tile column 2 clamps its loads at colmax
    (384, 256, 512, 0, True, False),      # tile column 1 starts at k = 256: an item of two chunks beside one of six
    (384, 512, 768, 1, False, False),     # every tile cut into three slabs of two chunks, reduced in table order
    (512, 256, 512, 1, True, False),      # slabs over a k range that starts at the tile's column
]


@pytest.mark.parametrize("k,M,N,kind,tri,tight", CASES)
def test_triunit_loop_error_within_twice_the_chunk_loop(ops, dev, monkeypatch, k, M, N, kind, tri, tight):
    A, B = _inputs(k, M, N, seed=k + M + N + kind, tri=tri)
    C0 = np.random.default_rng(1).standard_normal((1, M, N)).astype(np.float32)
    if tri:
        C0[:] = 0        # columns with a few k rows only: the rounding of C0 - acc would hide the product's own error
    ref, scale = _reference(A, B, C0, kind)
    monkeypatch.delenv("QT_G3_LOOP", raising=False)
    C_new = _run(ops, dev, A, B, C0, kind, tri, tight)
    C_again = _run(ops, dev, A, B, C0, kind, tri, tight)
    monkeypatch.setenv("QT_G3_LOOP", "chunk")
    C_old = _run(ops, dev, A, B, C0, kind, tri, tight)
    e_new, e_old = _rel_err(C_new, ref, scale), _rel_err(C_old, ref, scale)
    print(f"\nk={k} {M}x{N} kind={kind} tri={tri} tight={tight}: max err / sum|a||b|: tri-unit loop {e_new / EPS:.3f} eps, "
          f"chunk loop {e_old / EPS:.3f} eps")
    assert e_new <= 2 * e_old, (e_new, e_old)
    assert torch.equal(C_new, C_again)                  # no atomics: run-to-run identical
    assert not torch.equal(C_new, C_old)                # the two loops are different sums (else the knob is dead)


@pytest.mark.parametrize("kind", [0, 1])
def test_triunit_batch_of_two_equals_the_single_calls(ops, dev, monkeypatch, kind):
    k, M, N = 256, 256, 520
    A, B = _inputs(k, M, N, seed=11 + kind, batch=2)
    C0 = np.random.default_rng(2).standard_normal((2, M, N)).astype(np.float32)
    ref, scale = _reference(A, B, C0, kind)
    monkeypatch.delenv("QT_G3_LOOP", raising=False)
    C_b = _run(ops, dev, A, B, C0, kind, False, False)
    for b in range(2):
        C_s = _run(ops, dev, A[b:b + 1], B[b:b + 1], C0[b:b + 1], kind, False, False)
        assert torch.equal(C_b[b], C_s[0]), f"batch member {b} differs from the single call"
    monkeypatch.setenv("QT_G3_LOOP", "chunk")
    C_old = _run(ops, dev, A, B, C0, kind, False, False)
    e_new, e_old = _rel_err(C_b, ref, scale), _rel_err(C_old, ref, scale)
    print(f"\nbatch of 2, kind={kind}: max err / sum|a||b|: tri-unit loop {e_new / EPS:.3f} eps, chunk loop {e_old / EPS:.3f} eps")
    assert e_new <= 2 * e_old, (e_new, e_old)


def test_factor_k1536_through_the_triunit_products(ops, oracle, dev, monkeypatch):
    """``qt_cholesky_inverse_upper`` at K = 1536 with every block-row product on the bf16x3 kernel
    (QT_CHOL_G3_MIN_CHUNKS=1), x10 outlier channels: the bar of tests/test_gpu_factor_fullsize.py --
    max |U - U_f64| / max|U_f64| <= max(4 x the same error of the fp32 LAPACK three-step, 5e-6) -- and a batch of two
    equal to the single factorisations bit for bit."""
    K = 1536
    rng = np.random.default_rng(17)
    Hd = []
    for b in range(2):
        X = rng.standard_normal((4 * K, K)).astype(np.float32)
        X[:, rng.choice(K, size=K // 50, replace=False)] *= 10.0
        H = oracle.hessian_from_gram(oracle.gram_f64(oracle.f32_to_bf16_bits(X)), 8)
        Hd.append(oracle.hessian_dead_and_damp(H, 0.01)[0])
    truth = oracle.cholesky_inverse_upper_f64(Hd[0])
    U_lapack, ok = oracle.cholesky_inverse_upper_lapack(Hd[0])
    assert ok
    scale = np.abs(truth).max()
    e_lap = np.abs(U_lapack.astype(np.float64) - truth).max() / scale

    flipped = [torch.from_numpy(np.ascontiguousarray(h[::-1, ::-1]).astype(np.float32)).to(dev) for h in Hd]
    monkeypatch.setenv("QT_CHOL_G3", "0")
    U_f32, info = ops.cholesky_inverse_upper(flipped[0].clone())
    assert int(info.item()) == 0
    monkeypatch.setenv("QT_CHOL_G3", "1")
    monkeypatch.setenv("QT_CHOL_G3_MIN_CHUNKS", "1")
    monkeypatch.delenv("QT_G3_LOOP", raising=False)
    singles = []
    for a in flipped:
        U, info = ops.cholesky_inverse_upper(a.clone())
        assert int(info.item()) == 0
        singles.append(U)
    torch.cuda.synchronize()
    assert not torch.equal(singles[0], U_f32), "the bf16x3 products were not taken"
    e_gpu = np.abs(singles[0].cpu().numpy().astype(np.float64) - truth).max() / scale
    print(f"\n[factor] K={K}: max err / max|U| vs fp64: tri-unit products {e_gpu:.3e}; fp32 LAPACK three-step {e_lap:.3e}")
    assert e_gpu <= max(4 * e_lap, 5e-6), (e_gpu, e_lap)

    Ub = torch.empty((2, K, K), dtype=torch.float32, device=dev)
    info = ops.cholesky_inverse_upper_batched(torch.stack(flipped), Ub)
    torch.cuda.synchronize()
    assert info.cpu().tolist() == [0, 0]
    for b in range(2):
        assert torch.equal(Ub[b], singles[b]), f"batched factor {b} differs from the single factorisation"
