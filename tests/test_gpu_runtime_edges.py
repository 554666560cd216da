"""The checkpoint runtimes' kernels at the shapes their contract accepts and the other tests never run: K not a multiple
of 8 (a partial packed word) or of 128 (a ragged last group), a partial GROUP_M group of m-tiles, the K = 32768
accumulator bound, misaligned operands, empty experts and 16-row tile boundaries.

Every case is checked twice: equal to the bit to the existing torch restatement of the kernel, and within an error bound
of fp64 derived from the header's arithmetic, on weights decoded by tests/ckpt_reference.py (which shares no code with
the package).  Packed words carry 0xF in the nibbles past K, which every reader must ignore."""
import numpy as np
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_qlinear import _acts, _bits_equal, ref_gemm
from tests.test_gpu_wq_linear import _ref_w

pytestmark = pytest.mark.gpu


def _leaves(q8, bits, G, seed, zp=False, g_idx=False, pow2=False):
    """Checkpoint leaves (CPU) of levels q8 int8 [N, K]: packed with 0xF past K, G scales per row."""
    N, K = q8.shape
    g = torch.Generator().manual_seed(seed)
    if pow2:
        s = torch.pow(2.0, -torch.randint(0, 5, (N, G), generator=g).float())
    else:
        s = (torch.rand(N, G, generator=g) * 0.02 + 1e-4).to(torch.bfloat16).float()
    t = {"weight_scale": s, "weight_shape": torch.tensor([N, K])}
    if bits == 4:
        t["weight_packed"] = torch.from_numpy(cr.encode_int4(q8.numpy().astype(np.int64), pad_nibble=0xF))
    else:
        t["weight"] = q8
    if zp:
        t["weight_zero_point"] = torch.randint(-3, 4, (N, G), generator=g, dtype=torch.int8)
    if g_idx:
        t["weight_g_idx"] = ((torch.arange(K) // 128) % G)[torch.randperm(K, generator=g)].to(torch.int32)
    return t


def _levels(shape, bits, seed):
    g = torch.Generator().manual_seed(seed)
    lo, hi = (-8, 8) if bits == 4 else (-128, 128)
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int8)


def _qweight(t, dev):
    return (t["weight_packed"] if "weight_packed" in t else t["weight"]).to(dev)


# ---- qt_gemm_i8 -----------------------------------------------------------------------------------------------------
def _run_gemm_i8(ops, dev, Xq, s_x, zp_x, t, q8, bias, out_dtype):
    G = t["weight_scale"].shape[1]
    wsum = cr_wsum(q8, G)
    Y = ops.gemm_i8(Xq, s_x, _qweight(t, dev), t["weight_scale"].to(dev), K=q8.shape[1], zp_x=zp_x,
                    wsum=None if zp_x is None else wsum.to(dev), bias=bias, out_dtype=out_dtype)
    torch.cuda.synchronize()
    _bits_equal(Y, ref_gemm(Xq, s_x, q8, t["weight_scale"], zp_x, wsum if zp_x is not None else None, bias,
                            out_dtype))
    y64, mag = cr.a8_linear(Xq, s_x, zp_x, t, bias)
    cr.assert_within(Y, y64, cr.gemm_i8_tolerance(Y.cpu(), mag, G), "gemm_i8")
    return Y


def cr_wsum(q8, G):
    """wsum [N, G] int32 of the levels, per group of 128 contiguous columns (a ragged last group sums what it has)."""
    N, K = q8.shape
    step = K if G == 1 else 128
    return torch.stack([q8[:, g * step:(g + 1) * step].to(torch.int64).sum(1) for g in range(G)], 1).to(torch.int32)


RAGGED_K = [1, 7, 9, 33, 129, 999, 1001, 4097]


@pytest.mark.parametrize("bits,grouped", [(8, False), (8, True), (4, False), (4, True)])
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("M,N", [(127, 15), (128, 1), (129, 17)])
@pytest.mark.parametrize("K", RAGGED_K)
def test_gemm_i8_ragged_k(ops, dev, bits, grouped, asym, M, N, K):
    dt = torch.bfloat16 if M != 128 else torch.float16
    X = _acts(M, K, dt, dev, seed=M + K)
    Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
    q8 = _levels((N, K), bits, seed=N * K + bits)
    G = (K + 127) // 128 if grouped else 1
    t = _leaves(q8, bits, G, seed=K)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(K)) * 0.1).to(dt).to(dev) if asym else None
    _run_gemm_i8(ops, dev, Xq, s_x, zp_x, t, q8, bias, dt)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("K", [129, 999])
def test_gemm_i8_full_and_partial_group_m(ops, dev, bits, K):
    """M = 2049: 17 m-tiles, one full GROUP_M group of 16 and a partial group of 1, over 3 n-tiles."""
    M, N = 2049, 257
    X = _acts(M, K, torch.bfloat16, dev, seed=K)
    Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=False)
    q8 = _levels((N, K), bits, seed=K + bits)
    t = _leaves(q8, bits, (K + 127) // 128, seed=bits)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(1)) * 0.1).to(torch.bfloat16).to(dev)
    _run_gemm_i8(ops, dev, Xq, s_x, zp_x, t, q8, bias, torch.bfloat16)


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("grouped", [False, True])
def test_gemm_i8_at_the_accumulator_bound(ops, dev, bits, grouped):
    """K = 32768 with every level at its extremes and asymmetric activations: |acc| reaches 2^29 and |t| 2^30, so with
    G = 1 the int32 -> fp32 conversion really rounds."""
    M, N, K = 40, 48, 32768
    g = torch.Generator().manual_seed(bits + grouped)
    lo, hi = (-8, 7) if bits == 4 else (-128, 127)
    Xq = torch.where(torch.rand(M, K, generator=g) < 0.5, -128, 127).to(torch.int8)
    Xq[: M // 2] = -128                                          # rows of one sign: the largest |acc|
    q8 = torch.where(torch.rand(N, K, generator=g) < 0.5, lo, hi).to(torch.int8)
    q8[: N // 2] = lo
    s_x = (torch.rand(M, generator=g) * 1e-3 + 1e-5)
    zp_x = torch.randint(-128, 128, (M,), generator=g, dtype=torch.int32)
    zp_x[:4] = torch.tensor([-128, 127, 0, 1], dtype=torch.int32)
    G = (K + 127) // 128 if grouped else 1
    t = _leaves(q8, bits, G, seed=3)
    bias = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    _run_gemm_i8(ops, dev, Xq.to(dev), s_x.to(dev), zp_x.to(dev), t, q8, bias, torch.bfloat16)


@pytest.mark.parametrize("bits", [8, 4])
def test_gemm_i8_misaligned_operand(ops, dev, bits):
    """K % 16 == 0 but Xq starts 1 byte past a 16-byte boundary: the element-wise (non-16-byte) load path."""
    M, N, K = 130, 70, 1024
    X = _acts(M, K, torch.bfloat16, dev, seed=4)
    Xq0, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=False)
    buf = torch.zeros(M * K + 16, dtype=torch.int8, device=dev)
    Xq = buf[1:1 + M * K].view(M, K)
    Xq.copy_(Xq0)
    assert Xq.is_contiguous() and Xq.data_ptr() % 16 == 1
    q8 = _levels((N, K), bits, seed=5)
    t = _leaves(q8, bits, K // 128, seed=6)
    _run_gemm_i8(ops, dev, Xq, s_x, zp_x, t, q8, None, torch.bfloat16)


# ---- qt_gemm_i8_grouped ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,grouped", [(8, False), (4, True), (8, True)])
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("K", [77, 999])
def test_gemm_i8_grouped_ragged(ops, dev, bits, grouped, asym, K):
    """Experts 0 and 4 empty (first and last), one with 129 rows; K ragged with G = ceil(K/128) or 1."""
    E, counts, N = 5, [0, 129, 5, 1, 0], 40
    T = sum(counts)
    idx = torch.cat([torch.full((c,), e, dtype=torch.int64) for e, c in enumerate(counts)])
    idx = idx[torch.randperm(T, generator=torch.Generator().manual_seed(K))].reshape(T, 1).to(dev)
    X = _acts(T, K, torch.bfloat16, dev, seed=K)
    Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
    G = (K + 127) // 128 if grouped else 1
    q8 = [_levels((N, K), bits, seed=K + e) for e in range(E)]
    ts = [_leaves(q8[e], bits, G, seed=e) for e in range(E)]
    Wq = torch.stack([_qweight(t, dev) for t in ts])
    s_w = torch.stack([t["weight_scale"] for t in ts]).to(dev)
    wsum = torch.stack([cr_wsum(q, G) for q in q8])
    offsets, src_token, _, _ = ops.moe_route(idx, E)
    Y = ops.gemm_i8_grouped(Xq, s_x, Wq, s_w, offsets, row_idx=src_token, K=K, zp_x=zp_x,
                            wsum=wsum.to(dev) if asym else None)
    torch.cuda.synchronize()
    off = offsets.cpu().tolist()
    assert [off[e + 1] - off[e] for e in range(E)] == counts
    src = src_token.long().cpu()
    for e in range(E):
        lo, hi = off[e], off[e + 1]
        if hi == lo:
            continue
        rows = src[lo:hi]
        zr = None if zp_x is None else zp_x.cpu()[rows]
        _bits_equal(Y[lo:hi], ref_gemm(Xq.cpu()[rows], s_x.cpu()[rows], q8[e], ts[e]["weight_scale"], zr,
                                       wsum[e] if asym else None, None, torch.bfloat16))
        y64, mag = cr.a8_linear(Xq.cpu()[rows], s_x.cpu()[rows], zr, ts[e])
        cr.assert_within(Y[lo:hi], y64, cr.gemm_i8_tolerance(Y[lo:hi].cpu(), mag, G), f"expert {e}")


# ---- qt_gemm_wq_skinny ----------------------------------------------------------------------------------------------
WQ_K = [1, 5, 77, 129, 999, 1001]


def _exact_x(M, K, dtype, seed):
    return torch.randint(-4, 5, (M, K), generator=torch.Generator().manual_seed(seed)).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("zp,g_idx", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("N", [1, 15, 17])
@pytest.mark.parametrize("K", WQ_K)
def test_skinny_ragged(ops, dev, dtype, bits, zp, g_idx, N, K):
    G = (K + 127) // 128
    q8 = _levels((N, K), bits, seed=K * N + bits)
    # exact inputs (|x| <= 4, power-of-two scales): every partial sum is exact, so the bits are round(x @ w.T)
    t = _leaves(q8, bits, G, seed=K + N, zp=zp, g_idx=g_idx, pow2=True)
    Wq, s = _qweight(t, dev), t["weight_scale"].to(dev)
    z = t["weight_zero_point"].to(dev) if zp else None
    gi = t["weight_g_idx"].to(dev) if g_idx else None
    W = _ref_w(t, dtype)
    for M in (1, 7, 16):
        X = _exact_x(M, K, dtype, seed=M + K)
        Y = ops.gemm_wq_skinny(X.to(dev), Wq, s, zp_w=z, g_idx=gi)
        torch.cuda.synchronize()
        # + 0.0: the kernel sums from +0, so an exactly zero output is +0 (fp64 would keep the -0 of a lone product)
        _bits_equal(Y, (X.double() @ W.double().T + 0.0).to(dtype))
    # random inputs and scales: within the header's bound of fp64 on the file's decoding
    t = _leaves(q8, bits, G, seed=K + N + 1, zp=zp, g_idx=g_idx)
    s = t["weight_scale"].to(dev)
    z = t["weight_zero_point"].to(dev) if zp else None
    gi = t["weight_g_idx"].to(dev) if g_idx else None
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.1).to(dtype)
    for M in (1, 7, 16):
        X = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(dtype)
        Y = ops.gemm_wq_skinny(X.to(dev), Wq, s, zp_w=z, g_idx=gi, bias=bias.to(dev))
        torch.cuda.synchronize()
        y64, mag = cr.a16_linear(X, t, bias)
        cr.assert_within(Y, y64, cr.gemv_tolerance(Y.cpu(), mag, K), f"skinny M={M}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits,zp", [(4, True), (8, False)])
def test_skinny_every_m_at_a_ragged_shape(ops, dev, dtype, bits, zp):
    N, K = 17, 1001
    q8 = _levels((N, K), bits, seed=bits)
    t = _leaves(q8, bits, (K + 127) // 128, seed=9, zp=zp, pow2=True)
    Wq, s = _qweight(t, dev), t["weight_scale"].to(dev)
    z = t["weight_zero_point"].to(dev) if zp else None
    W = _ref_w(t, dtype)
    bias = torch.randint(-8, 9, (N,), generator=torch.Generator().manual_seed(2)).to(dtype)
    for M in range(1, 17):
        X = _exact_x(M, K, dtype, seed=M)
        Y = ops.gemm_wq_skinny(X.to(dev), Wq, s, zp_w=z, bias=bias.to(dev))
        torch.cuda.synchronize()
        _bits_equal(Y, (X.double() @ W.double().T + bias.double()).to(dtype))
        y64, mag = cr.a16_linear(X, t, bias)
        cr.assert_within(Y, y64, cr.gemv_tolerance(Y.cpu(), mag, K), f"M={M}")


# ---- qt_gemm_wq_grouped ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits,zp,g_idx", [(4, False, False), (4, True, True), (8, True, False), (8, False, True)])
@pytest.mark.parametrize("K", WQ_K)
def test_wq_grouped_ragged(ops, dev, dtype, bits, zp, g_idx, K):
    """Experts of 15, 16 and 17 rows (one tile short, one tile, a tile and one row) between empty first and last
    experts; every row equal to the bit to qt_gemm_wq_skinny on its expert and within the bound of fp64."""
    E, counts, N = 5, [0, 15, 16, 17, 0], 24
    T = sum(counts)
    G = (K + 127) // 128
    idx = torch.cat([torch.full((c,), e, dtype=torch.int64) for e, c in enumerate(counts)])
    idx = idx[torch.randperm(T, generator=torch.Generator().manual_seed(K))].reshape(T, 1).to(dev)
    ts = [_leaves(_levels((N, K), bits, seed=K + e), bits, G, seed=e, zp=zp, g_idx=g_idx) for e in range(E)]
    Wq = torch.stack([_qweight(t, dev) for t in ts])
    s = torch.stack([t["weight_scale"] for t in ts]).to(dev)
    z = torch.stack([t["weight_zero_point"] for t in ts]).to(dev) if zp else None
    gi = torch.stack([t["weight_g_idx"] for t in ts]).to(dev) if g_idx else None
    X = torch.randn(T, K, generator=torch.Generator().manual_seed(K)).to(dtype)
    offsets, src_token, _, _ = ops.moe_route(idx, E)
    Y = ops.gemm_wq_grouped(X.to(dev), Wq, s, offsets, row_idx=src_token, K=K, zp_w=z, g_idx=gi)
    torch.cuda.synchronize()
    off = offsets.cpu().tolist()
    assert [off[e + 1] - off[e] for e in range(E)] == counts
    src = src_token.long().cpu()
    for e in range(E):
        lo, hi = off[e], off[e + 1]
        if hi == lo:
            continue
        rows = src[lo:hi]
        for a in range(0, hi - lo, 16):
            b = min(a + 16, hi - lo)
            want = ops.gemm_wq_skinny(X[rows[a:b]].to(dev), Wq[e], s[e], zp_w=None if z is None else z[e],
                                      g_idx=None if gi is None else gi[e])
            torch.cuda.synchronize()
            _bits_equal(Y[lo + a:lo + b], want)
        y64, mag = cr.a16_linear(X[rows], ts[e])
        cr.assert_within(Y[lo:hi], y64, cr.gemv_tolerance(Y[lo:hi].cpu(), mag, K), f"expert {e}")
