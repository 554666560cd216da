"""``qt_gemm_wq_tile`` on the GPU against its own contract: one-hot rows that pin the LDS images, the dequantise lane map
and the fragment map against the dequantised weight, exactly summable inputs against the fp64 product rounded once, the
fp64 bound, determinism and row independence, pitched and caller-owned operands, the raw ABI's refusals, the module."""
import pytest
import torch
import torch.nn.functional as F

from tests.exact_inputs import assert_exactly_summable
from tests.test_gpu_wq_linear import _bits_equal, _check_bound, _dev_args, _ref_w, _weight

pytestmark = pytest.mark.gpu

MS = (1, 127, 128, 129, 200)        # one ragged tile, a full one, a second tile of 1 and of 72 rows
NS = (1, 127, 128, 129, 200)
KTS = (2, 4, 6, 10, 18)             # K-tiles of 64: prologue only, one steady phase, every slot / image buffer reused
DT = (torch.bfloat16, torch.float16)


def _case(i, j):
    c = len(KTS) * i + j
    return (MS[i], 64 * KTS[j], NS[(i + j) % 5], (4, 8)[(c >> 1) & 1], bool((c >> 2) & 1), bool((c >> 3) & 1),
            bool((i + j // 2) & 1), DT[(i // 2 + j) & 1])


def _x(M, K, dtype, dev, seed):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


@pytest.mark.parametrize("bits,zp,dtype", [(4, False, torch.bfloat16), (4, True, torch.float16),
                                           (8, False, torch.float16), (8, True, torch.bfloat16)])
def test_one_hot_rows_read_the_weight(ops, dev, bits, zp, dtype):
    N, K, M = 130, 640, 130
    t, _ = _weight(N, K, bits, zp=zp, seed=bits + zp)
    Wq, s, z, _ = _dev_args(t, dev)
    Wt = _ref_w(t, dtype).to(dev).t().contiguous().view(torch.int16)      # [K, N]
    rows = torch.arange(M, device=dev)
    for off in range(0, 201):           # three K-tiles and their boundaries, a group boundary, the ring's first wrap
        X = torch.zeros(M, K, dtype=dtype, device=dev)
        X[rows, off + rows] = 1
        Y = ops.gemm_wq_tile(X, Wq, s, zp_w=z)
        assert torch.equal(Y.view(torch.int16), Wt[off:off + M]), off


@pytest.mark.parametrize("i", range(len(MS)), ids=[f"M{m}" for m in MS])
def test_exactly_summable_inputs_give_the_exact_result(ops, dev, i):
    for j in range(len(KTS)):
        M, K, N, bits, zp, grouped, with_bias, dtype = case = _case(i, j)
        t, _ = _weight(N, K, bits, zp=zp, grouped=grouped, seed=7 * i + j, pow2_scales=True)
        Wq, s, z, _ = _dev_args(t, dev)
        g = torch.Generator().manual_seed(50 + 7 * i + j)
        X = torch.randint(-4, 5, (M, K), generator=g).to(dtype)
        bias = torch.randint(-8, 9, (N,), generator=g).to(dtype) if with_bias else None
        w64 = _ref_w(t, dtype).double()
        want = X.double() @ w64.T + (0 if bias is None else bias.double())
        # every term is a multiple of the smallest scale 2^-4: sum |x w| (+ |bias|) in those units stays below 2^24
        assert_exactly_summable(X.double().abs() @ w64.abs().T + (0 if bias is None else bias.double().abs()), 4, case)
        Y = ops.gemm_wq_tile(X.to(dev), Wq, s, zp_w=z, bias=None if bias is None else bias.to(dev))
        assert Y.shape == (M, N) and Y.dtype == dtype
        assert torch.equal(Y.cpu().double(), want.to(dtype).double()), case


@pytest.mark.parametrize("M,N,kts,bits,zp,dtype", [(200, 129, 6, 4, True, torch.bfloat16),
                                                   (200, 200, 18, 8, False, torch.float16),
                                                   (200, 127, 10, 4, False, torch.bfloat16)])
def test_random_inputs_bound_determinism_and_row_independence(ops, dev, M, N, kts, bits, zp, dtype):
    K = 64 * kts
    t, _ = _weight(N, K, bits, zp=zp, seed=M + N)
    Wq, s, z, _ = _dev_args(t, dev)
    X = _x(M, K, dtype, dev, seed=5)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(6)) * 0.1).to(dtype)
    Y = ops.gemm_wq_tile(X, Wq, s, zp_w=z, bias=bias.to(dev))
    _check_bound(Y, X, _ref_w(t, dtype), bias)
    _bits_equal(ops.gemm_wq_tile(X, Wq, s, zp_w=z, bias=bias.to(dev)), Y)              # two runs, the same bits
    _bits_equal(ops.gemm_wq_tile(X[100:131], Wq, s, zp_w=z, bias=bias.to(dev)), Y[100:131])


def _raw(X, M, K, ldx, Wq, fmt, N, s, G, zp, g_idx, bias, Y, ldy, code=None):
    from quantool_amd.hip import _lib

    p = lambda v: None if v is None else (v if isinstance(v, int) else v.data_ptr())   # noqa: E731
    code = _lib.QT_BF16 if code is None else code
    _lib.check("qt_gemm_wq_tile", _lib.load().qt_gemm_wq_tile(
        p(X), code, M, K, ldx, p(Wq), fmt, N, p(s), G, p(zp), p(g_idx), p(bias), p(Y), ldy,
        torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("bits,ldy_extra", [(4, 17), (8, 20)])      # ldy = N + 20: 8-byte stores up to the ragged end
def test_pitched_activations_and_caller_owned_output(ops, dev, bits, ldy_extra):
    M, N, K = 131, 131, 640
    t, _ = _weight(N, K, bits, zp=True, seed=4)
    # operands as exact-size allocations: each ends with its storage
    Wq, s, z, _ = (None if v is None else v.clone() for v in _dev_args(t, dev))
    wide = _x(M, K + 8, torch.bfloat16, dev, seed=3).clone()
    X = wide[:, :K]                                                       # ldx = K + 8
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(1)) * 0.1).to(torch.bfloat16).to(dev)
    for v in (Wq, s, z, wide, bias):
        assert v.untyped_storage().nbytes() == v.numel() * v.element_size()
    assert ops.gemm_wq_tile_supported(X, Wq, s, z)
    want = ops.gemm_wq_tile(X.contiguous(), Wq, s, zp_w=z, bias=bias)
    ldy, rows = N + ldy_extra, M + 3
    buf = torch.full((rows * ldy + 64,), 7.0, dtype=torch.bfloat16, device=dev)
    grid = buf[:rows * ldy].view(rows, ldy)
    assert ops.gemm_wq_tile(X, Wq, s, zp_w=z, bias=bias, out=grid[:M, :N]).data_ptr() == buf.data_ptr()
    _bits_equal(grid[:M, :N].contiguous(), want)
    assert (grid[:M, N:] == 7).all() and (grid[M:] == 7).all() and (buf[rows * ldy:] == 7).all()


def test_raw_abi_refusals_launch_nothing(ops, dev):
    from quantool_amd.hip._lib import QT_ERR_INVALID, QT_F32, QT_W_INT4_PACKED, QT_W_INT8, HipBackendError

    N, K = 32, 1024
    wbuf = torch.zeros(N * K + 16, dtype=torch.int8, device=dev)
    Wq, Wq_off = wbuf[:N * K].view(N, K), wbuf[4:4 + N * K].view(N, K)
    xbuf = torch.zeros(130 * (K + 8) + 8, dtype=torch.bfloat16, device=dev)
    X, X_off = xbuf[:130 * K].view(130, K), xbuf[1:1 + 128 * K].view(128, K)
    s = torch.ones(N, 8, device=dev)
    gi = torch.zeros(K, dtype=torch.int32, device=dev)
    Y = torch.full((140, N), 7.0, dtype=torch.bfloat16, device=dev)
    base = dict(X=X, M=130, K=K, ldx=K, Wq=Wq, fmt=QT_W_INT8, N=N, s=s, G=1, zp=None, g_idx=None, bias=None, Y=Y, ldy=N)
    cases = {
        "g_idx": (dict(G=8, g_idx=gi), "actorder group runs on qt_dequantize_weight"),
        "ragged K": (dict(K=192), "not a multiple of the k-unit"),
        "M = 0": (dict(M=0), "M >= 1"), "M = -1": (dict(M=-1), "M >= 1"),
        "X shifted": (dict(X=X_off), "16-byte aligned"), "Wq shifted": (dict(Wq=Wq_off), "16-byte aligned"),
        "pitch K + 1": (dict(ldx=K + 1), "16-byte aligned"), "pitch below K": (dict(ldx=K - 8), "ldx >= K"),
        "pitch above 2^23": (dict(M=1, ldx=(1 << 23) + 8), "ldx <= 8388608"),
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
    assert (Y[:130] == 0).all() and (Y[130:] == 7).all()


def test_module_takes_the_tile_branch_only_when_asked(ops, dev):
    from quantool_amd.engine.qmodules import WeightOnlyLinear

    N, K, M = 130, 256, 200
    t, _ = _weight(N, K, 4, zp=True, seed=9)
    Wq, s, z, _ = _dev_args(t, dev)
    m = WeightOnlyLinear(K, N, Wq, s, z).to(dev)
    m.tile_min_k = m.tile_min_n = m.tile_max_n = 0          # the branch under test, whatever the measured size bounds
    x = _x(M, K, torch.bfloat16, dev, seed=2)
    _bits_equal(m(x), F.linear(x, _ref_w(t, torch.bfloat16).to(dev)))
    m.tile_max_m = 256
    _bits_equal(m(x), ops.gemm_wq_tile(x, Wq, s, zp_w=z))
    m.tile_max_m = 199
    _bits_equal(m(x), F.linear(x, _ref_w(t, torch.bfloat16).to(dev)))
