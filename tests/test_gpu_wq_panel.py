"""``qt_gemm_wq_panel`` on the GPU: every row bit for bit against the skinny kernel, one-hot rows that pin the LDS / lane /
column map against the dequantised weight, the fp64 bound, pitched and caller-owned operands, the raw ABI's refusals."""
import pytest
import torch

from tests.test_gpu_wq_linear import _bits_equal, _check_bound, _dev_args, _ref_w, _weight

pytestmark = pytest.mark.gpu

# A workgroup holds a row block of 16 MT rows, MT <= 4; M rows are ceil(M / 64) blocks of equal height.  At, one below and
# one above: the m-tile (16), the full block (64 -> two blocks of 3 m-tiles at 65), 3 -> 4 m-tiles in one block (48) and in
# two (96), two full blocks (128 -> three at 129), a last block with dead m-tiles (200 = 4 x 64 - 56), the largest M.
MS = (1, 16, 17, 48, 49, 63, 64, 65, 96, 97, 127, 128, 129, 200, 512)
# k-blocks of 128 columns, four to a stage, two LDS buffers: chains with no block at all (1, 3), one stage (4), a second
# stage of one block (5), two stages (8), the first buffer used again (9), a ragged fourth stage (13), many (35)
KBS = (1, 3, 4, 5, 8, 9, 13, 35)
NS = (1, 63, 64, 65, 130)           # a workgroup owns 64 columns, a wave two tiles of 16


def _case(i, j):
    c = len(KBS) * i + j
    return (MS[i], KBS[j], NS[(i + j) % 5], (4, 8)[(c >> 1) & 1], bool((c >> 2) & 1), bool((c >> 3) & 1),
            bool((i + j // 2) & 1), (torch.bfloat16, torch.float16)[(i // 2 + j) & 1])


def _x(M, K, dtype, dev, seed):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


@pytest.mark.parametrize("i", range(len(MS)), ids=[f"M{m}" for m in MS])
def test_rows_equal_the_skinny_kernel(ops, dev, i):
    for j in range(len(KBS)):
        M, kbs, N, bits, zp, grouped, with_bias, dtype = case = _case(i, j)
        K = 128 * kbs
        t, _ = _weight(N, K, bits, zp=zp, grouped=grouped, seed=11 * i + j)
        Wq, s, z, _ = _dev_args(t, dev)
        X = _x(M, K, dtype, dev, seed=300 + 11 * i + j)
        bias = (torch.randn(N, generator=torch.Generator().manual_seed(j)) * 0.1).to(dtype).to(dev) if with_bias else None
        Y = ops.gemm_wq_panel(X, Wq, s, zp_w=z, bias=bias)
        assert Y.shape == (M, N) and Y.dtype == dtype
        for lo in range(0, M, 16):
            ref = ops.gemm_wq_skinny(X[lo:lo + 16], Wq, s, zp_w=z, bias=bias)
            assert torch.equal(Y[lo:lo + 16].view(torch.int16), ref.view(torch.int16)), (case, lo)
        Y2 = ops.gemm_wq_panel(X, Wq, s, zp_w=z, bias=bias)
        assert torch.equal(Y.view(torch.int16), Y2.view(torch.int16)), case       # two runs, the same bits


@pytest.mark.parametrize("bits,zp,dtype", [(4, False, torch.bfloat16), (4, True, torch.float16),
                                           (8, False, torch.float16), (8, True, torch.bfloat16)])
def test_one_hot_rows_read_the_weight(ops, dev, bits, zp, dtype):
    N, K, M = 70, 768, 80               # two column tiles of a second wave-column; two row blocks, the second part dead
    t, _ = _weight(N, K, bits, zp=zp, seed=bits + zp)
    Wq, s, z, _ = _dev_args(t, dev)
    Wt = _ref_w(t, dtype).to(dev).t().contiguous().view(torch.int16)      # [K, N]
    rows = torch.arange(M, device=dev)
    for off in range(0, 530):                                             # a whole stage of 512 columns and its boundary
        X = torch.zeros(M, K, dtype=dtype, device=dev)
        X[rows, off + rows] = 1
        Y = ops.gemm_wq_panel(X, Wq, s, zp_w=z)
        assert torch.equal(Y.view(torch.int16), Wt[off:off + M]), off


@pytest.mark.parametrize("M,N,kbs,bits,zp,dtype", [(33, 65, 5, 4, True, torch.bfloat16),
                                                   (100, 130, 13, 8, False, torch.float16),
                                                   (512, 63, 35, 4, False, torch.bfloat16)])
def test_random_inputs_within_the_fp64_bound(ops, dev, M, N, kbs, bits, zp, dtype):
    K = 128 * kbs
    t, _ = _weight(N, K, bits, zp=zp, seed=M + N)
    Wq, s, z, _ = _dev_args(t, dev)
    X = _x(M, K, dtype, dev, seed=5)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(6)) * 0.1).to(dtype)
    Y = ops.gemm_wq_panel(X, Wq, s, zp_w=z, bias=bias.to(dev))
    _check_bound(Y, X, _ref_w(t, dtype), bias)


# ---- edges ----------------------------------------------------------------------------------------------------------
def _raw(X, M, K, ldx, Wq, fmt, N, s, G, zp, g_idx, bias, Y, ldy, code=None):
    from quantool_amd.hip import _lib

    p = lambda v: None if v is None else (v if isinstance(v, int) else v.data_ptr())   # noqa: E731
    code = _lib.QT_BF16 if code is None else code
    _lib.check("qt_gemm_wq_panel", _lib.load().qt_gemm_wq_panel(
        p(X), code, M, K, ldx, p(Wq), fmt, N, p(s), G, p(zp), p(g_idx), p(bias), p(Y), ldy,
        torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("bits,ldy_extra", [(4, 17), (8, 20)])      # ldy = 84: 8-byte stores up to the ragged end; 87: none
def test_pitched_activations_and_caller_owned_output(ops, dev, bits, ldy_extra):
    from quantool_amd.hip import _lib

    M, N, K = 81, 67, 640
    t, _ = _weight(N, K, bits, zp=True, seed=4)
    # operands as exact-size allocations: each ends with its storage
    Wq, s, z, _ = (None if v is None else v.clone() for v in _dev_args(t, dev))
    wide = _x(M, K + 8, torch.bfloat16, dev, seed=3).clone()
    X = wide[:, :K]                                                       # ldx = K + 8
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(1)) * 0.1).to(torch.bfloat16).to(dev)
    for v in (Wq, s, z, wide, bias):
        assert v.untyped_storage().nbytes() == v.numel() * v.element_size()
    assert ops.gemm_wq_panel_supported(X, Wq, s, z)
    want = ops.gemm_wq_panel(X, Wq, s, zp_w=z, bias=bias)
    for lo in range(0, M, 16):
        _bits_equal(want[lo:lo + 16], ops.gemm_wq_skinny(X[lo:lo + 16], Wq, s, zp_w=z, bias=bias))
    ldy, rows = N + ldy_extra, M + 3
    buf = torch.full((rows * ldy + 64,), 7.0, dtype=torch.bfloat16, device=dev)
    fmt = _lib.QT_W_INT4_PACKED if bits == 4 else _lib.QT_W_INT8
    _raw(X, M, K, K + 8, Wq, fmt, N, s, s.shape[1], z, None, bias, buf, ldy)
    grid = buf[:rows * ldy].view(rows, ldy)
    _bits_equal(grid[:M, :N].contiguous(), want)
    assert (grid[:M, N:] == 7).all() and (grid[M:] == 7).all() and (buf[rows * ldy:] == 7).all()


def test_raw_abi_refusals_launch_nothing(ops, dev):
    from quantool_amd.hip._lib import QT_ERR_INVALID, QT_F32, QT_W_INT4_PACKED, QT_W_INT8, HipBackendError

    N, K = 32, 1024
    wbuf = torch.zeros(N * K + 16, dtype=torch.int8, device=dev)
    Wq, Wq_off = wbuf[:N * K].view(N, K), wbuf[4:4 + N * K].view(N, K)
    xbuf = torch.zeros(513 * (K + 8) + 8, dtype=torch.bfloat16, device=dev)
    X, X_off = xbuf[:513 * K].view(513, K), xbuf[1:1 + 128 * K].view(128, K)
    s = torch.ones(N, 8, device=dev)
    gi = torch.zeros(K, dtype=torch.int32, device=dev)
    Y = torch.full((513, N), 7.0, dtype=torch.bfloat16, device=dev)
    base = dict(X=X, M=40, K=K, ldx=K, Wq=Wq, fmt=QT_W_INT8, N=N, s=s, G=1, zp=None, g_idx=None, bias=None, Y=Y, ldy=N)
    cases = {
        "g_idx": (dict(G=8, g_idx=gi), "actorder group runs on qt_dequantize_weight"),
        "ragged K": (dict(K=192), "not a multiple of the k-unit"),
        "M = 0": (dict(M=0), "1 <= M <= 512"), "M = 513": (dict(M=513), "1 <= M <= 512"),
        "X shifted": (dict(X=X_off), "16-byte aligned"), "Wq shifted": (dict(Wq=Wq_off), "16-byte aligned"),
        "pitch K + 1": (dict(ldx=K + 1), "16-byte aligned"), "pitch below K": (dict(ldx=K - 8), "ldx >= K"),
        "pitch above 2^24": (dict(M=1, ldx=(1 << 24) + 8), "ldx <= 16777216"),
        "ldy below N": (dict(ldy=N - 1), "ldy >= N"),
        "null X": (dict(X=None), "null pointer"), "null Wq": (dict(Wq=None), "null pointer"),
        "null s_w": (dict(s=None), "null pointer"), "null Y": (dict(Y=None), "null pointer"),
        "G = 3": (dict(G=3), "G must be 1 or K / 128 = 8"), "w_format": (dict(fmt=99), "w_format 99"),
        "fp32": (dict(fmt=QT_W_INT4_PACKED, G=8, code=QT_F32), "must be bf16 or fp16"),
    }
    for what, (change, reason) in cases.items():
        with pytest.raises(HipBackendError, match=reason) as e:
            _raw(**{**base, **change})
        assert e.value.status == QT_ERR_INVALID, what
    torch.cuda.synchronize()
    assert (Y == 7).all()
    _raw(**{**base, "G": 8})                                                          # and the same call, accepted
    assert (Y[:40] == 0).all() and (Y[40:] == 7).all()
