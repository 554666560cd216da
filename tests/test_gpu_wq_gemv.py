"""``qt_gemm_wq_gemv`` / ``qt_gemm_wq_gemv_act_mul`` on the GPU against their contract: one-hot rows that pin the lane map
and the unpack order against the dequantised weight, exactly summable inputs against the fp64 product rounded once, the
fp64 bound, determinism and row independence, pitched and caller-owned operands, the raw ABI's refusals, the fused
pair against torch's SiLU and multiply, the module.  The layout the shapes are chosen for (csrc/wq_gemv.hip): 4 weight
rows per workgroup; K split over 4 waves in whole 128-column groups; a lane piece of 8 columns below K = 3712, 16 from
there, 32 (int4 alone) from K = 7808; a slab is 64 pieces."""
import pytest
import torch
import torch.nn.functional as F

from tests.exact_inputs import assert_exactly_summable
from tests.test_gpu_wq_linear import _bits_equal, _check_bound, _dev_args, _ref_w, _weight

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 5, 10)               # R - 1, R, R + 1 around R = 4, and two workgroups and a half
# one group; three waves of one group; one slab per wave at each piece width (2048, 4096, 8192 for int4); one slab + 128
# in the last wave (2176); an uneven split with a slab boundary inside a wave's range (4352: 8, 9, 8, 9 k-blocks)
KS = (128, 384, 2048, 2176, 4096, 4352, 8192)
DT = (torch.bfloat16, torch.float16)


def _case(i, j):
    c = len(KS) * i + j
    bits = 4 if KS[j] == 8192 else (4, 8)[(c >> 1) & 1]      # int8 at K = 8192 is K = 4096's path with sums too long
    return (i + 1, KS[j], NS[(i + j) % 5], bits, bool((c >> 2) & 1), bool((c >> 3) & 1), bool((i + j // 2) & 1),
            DT[(i // 2 + j) & 1])


def _x(M, K, dtype, dev, seed):
    return torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


@pytest.mark.parametrize("bits,zp,dtype", [(4, False, torch.bfloat16), (4, True, torch.float16),
                                           (8, False, torch.float16), (8, True, torch.bfloat16)])
def test_one_hot_rows_read_the_weight(ops, dev, bits, zp, dtype):
    N, K, M = 9, 4352, 4
    t, _ = _weight(N, K, bits, zp=zp, seed=bits + zp)
    Wq, s, z, _ = _dev_args(t, dev)
    Wt = _ref_w(t, dtype).to(dev).t().contiguous().view(torch.int16)      # [K, N]
    rows = torch.arange(M, device=dev)
    # pieces of 16 columns: wave 0 ends and a group ends at 1024, wave 1's first slab at 2048, its range at 2176
    for off in [0, *range(1000, 1045), *range(2030, 2060), *range(2160, 2190), K - M]:
        X = torch.zeros(M, K, dtype=dtype, device=dev)
        X[rows, off + rows] = 1
        Y = ops.gemm_wq_gemv(X, Wq, s, zp_w=z)
        assert torch.equal(Y.view(torch.int16), Wt[off:off + M]), off


def _exact_case(i, j):
    M, K, N, bits, zp, grouped, with_bias, dtype = case = _case(i, j)
    t, _ = _weight(N, K, bits, zp=zp, grouped=grouped, seed=7 * i + j, pow2_scales=True)
    g = torch.Generator().manual_seed(50 + 7 * i + j)
    X = torch.randint(-4, 5, (M, K), generator=g).to(dtype)
    bias = torch.randint(-8, 9, (N,), generator=g).to(dtype) if with_bias else None
    w64 = _ref_w(t, dtype).double()
    want = X.double() @ w64.T + (0 if bias is None else bias.double())
    # every term is a multiple of the smallest scale 2^-4: sum |x w| (+ |bias|) in those units stays below 2^24
    assert_exactly_summable(X.double().abs() @ w64.abs().T + (0 if bias is None else bias.double().abs()), 4, case)
    return case, t, X, bias, want.to(dtype)


@pytest.mark.parametrize("i", range(4), ids=[f"M{m}" for m in range(1, 5)])
def test_exactly_summable_inputs_give_the_exact_result(ops, dev, i):
    for j in range(len(KS)):
        case, t, X, bias, want = _exact_case(i, j)
        Wq, s, z, _ = _dev_args(t, dev)
        Y = ops.gemm_wq_gemv(X.to(dev), Wq, s, zp_w=z, bias=None if bias is None else bias.to(dev))
        assert Y.shape == want.shape and Y.dtype == want.dtype
        assert torch.equal(Y.cpu().double(), want.double()), case


def test_fp16_subnormal_activations_count(ops, dev):
    # x = 2^-16 is subnormal in fp16, w a small multiple of 2^-4: fp16 holds every product; a flushed input shows as 0
    N, K = 5, 384
    t, _ = _weight(N, K, 4, seed=3, pow2_scales=True)
    Wq, s, z, _ = _dev_args(t, dev)
    X = torch.zeros(2, K, dtype=torch.float16)
    X[0, 7] = X[1, 200] = 2.0 ** -16
    want = (X.double() @ _ref_w(t, torch.float16).double().T).to(torch.float16)
    assert want.abs().max() > 0
    _bits_equal(ops.gemm_wq_gemv(X.to(dev), Wq, s, zp_w=z), want)


@pytest.mark.parametrize("N,K,bits,zp,dtype", [(37, 4352, 4, True, torch.bfloat16), (10, 8192, 4, False, torch.float16),
                                               (130, 2176, 8, False, torch.bfloat16)])
def test_random_inputs_bound_determinism_and_row_independence(ops, dev, N, K, bits, zp, dtype):
    t, _ = _weight(N, K, bits, zp=zp, seed=N + K)
    Wq, s, z, _ = _dev_args(t, dev)
    X = _x(4, K, dtype, dev, seed=5)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(6)) * 0.1).to(dtype)
    Y = ops.gemm_wq_gemv(X, Wq, s, zp_w=z, bias=bias.to(dev))
    _check_bound(Y, X, _ref_w(t, dtype), bias)
    _bits_equal(ops.gemm_wq_gemv(X, Wq, s, zp_w=z, bias=bias.to(dev)), Y)              # two runs, the same bits
    for m in range(4):
        _bits_equal(ops.gemm_wq_gemv(X[m:m + 1], Wq, s, zp_w=z, bias=bias.to(dev)), Y[m:m + 1])


@pytest.mark.parametrize("bits", [4, 8])
def test_pitched_activations_and_caller_owned_output(ops, dev, bits):
    M, N, K = 3, 10, 2176
    t, _ = _weight(N, K, bits, zp=True, seed=4)
    Wq, s, z, _ = (None if v is None else v.clone() for v in _dev_args(t, dev))
    wide = _x(M, K + 8, torch.bfloat16, dev, seed=3).clone()
    X = wide[:, :K]                                                       # ldx = K + 8
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(1)) * 0.1).to(torch.bfloat16).to(dev)
    want = ops.gemm_wq_gemv(X.contiguous(), Wq, s, zp_w=z, bias=bias)
    _check_bound(want, X, _ref_w(t, torch.bfloat16), bias)
    ldy, rows = N + 7, M + 2
    buf = torch.full((rows * ldy + 64,), 7.0, dtype=torch.bfloat16, device=dev)
    grid = buf[:rows * ldy].view(rows, ldy)
    assert ops.gemm_wq_gemv(X, Wq, s, zp_w=z, bias=bias, out=grid[:M, :N]).data_ptr() == buf.data_ptr()
    _bits_equal(grid[:M, :N].contiguous(), want)
    assert (grid[:M, N:] == 7).all() and (grid[M:] == 7).all() and (buf[rows * ldy:] == 7).all()


def test_raw_abi_refusals_launch_nothing(ops, dev):
    from quantool_amd.hip import _lib
    from quantool_amd.hip._lib import QT_BF16, QT_ERR_INVALID, QT_F32, QT_W_INT4_PACKED, QT_W_INT8, HipBackendError

    def _raw(X, M, K, ldx, Wq, fmt, N, s, G, zp, g_idx, bias, Y, ldy, code=QT_BF16):
        p = lambda v: None if v is None else v.data_ptr()   # noqa: E731
        _lib.check("qt_gemm_wq_gemv", _lib.load().qt_gemm_wq_gemv(
            p(X), code, M, K, ldx, p(Wq), fmt, N, p(s), G, p(zp), p(g_idx), p(bias), p(Y), ldy,
            torch.cuda.current_stream().cuda_stream))

    N, K = 6, 1024
    wbuf = torch.zeros(N * K + 16, dtype=torch.int8, device=dev)
    Wq, Wq_off = wbuf[:N * K].view(N, K), wbuf[4:4 + N * K].view(N, K)
    xbuf = torch.zeros(5 * (K + 8) + 8, dtype=torch.bfloat16, device=dev)
    X, X_off = xbuf[:5 * K].view(5, K), xbuf[1:1 + 4 * K].view(4, K)
    s = torch.ones(N, 8, device=dev)
    gi = torch.zeros(K, dtype=torch.int32, device=dev)
    Y = torch.full((6, N), 7.0, dtype=torch.bfloat16, device=dev)
    base = dict(X=X, M=4, K=K, ldx=K, Wq=Wq, fmt=QT_W_INT8, N=N, s=s, G=1, zp=None, g_idx=None, bias=None, Y=Y, ldy=N)
    cases = {
        "g_idx": (dict(G=8, g_idx=gi), "g_idx is not taken"),
        "ragged K": (dict(K=192), "not a multiple of the k-unit"),
        "M = 0": (dict(M=0), "1 <= M <= 4"), "M = 5": (dict(M=5), "1 <= M <= 4"),
        "X shifted": (dict(X=X_off), "16-byte aligned"), "Wq shifted": (dict(Wq=Wq_off), "16-byte aligned"),
        "pitch K + 1": (dict(ldx=K + 1), "16-byte aligned"), "null Y": (dict(Y=None), "null pointer"),
        "G = 3": (dict(G=3), "G must be 1 or K / 128 = 8"),
        "fp32": (dict(fmt=QT_W_INT4_PACKED, G=8, code=QT_F32), "must be bf16 or fp16"),
    }
    for what, (change, reason) in cases.items():
        with pytest.raises(HipBackendError, match=reason) as e:
            _raw(**{**base, **change})
        assert e.value.status == QT_ERR_INVALID, what
    torch.cuda.synchronize()
    assert (Y == 7).all()
    _raw(**{**base, "G": 8})                                                          # and the same call, accepted
    assert (Y[:4] == 0).all() and (Y[4:] == 7).all()


@pytest.mark.parametrize("M", [1, 4])
@pytest.mark.parametrize("I,K,bits,zp,dtype", [(10, 384, 8, True, torch.float16), (37, 4352, 4, False, torch.bfloat16)])
def test_act_mul_equals_silu_and_multiply_of_the_two_gemvs(ops, dev, M, I, K, bits, zp, dtype):
    gate, up = (_dev_args(_weight(I, K, bits, zp=zp, seed=sd)[0], dev)[:3] for sd in (1, 2))
    X = _x(M, K, dtype, dev, seed=M)
    H = ops.gemm_wq_gemv_act_mul(X, gate, up)
    _bits_equal(H, F.silu(ops.gemm_wq_gemv(X, *gate)) * ops.gemm_wq_gemv(X, *up))


def test_module_takes_the_gemv_only_when_asked(ops, dev):
    from quantool_amd.engine.qmodules import WeightOnlyLinear

    N, K = 10, 384
    t, _ = _weight(N, K, 4, zp=True, seed=9)
    Wq, s, z, _ = _dev_args(t, dev)
    m = WeightOnlyLinear(K, N, Wq, s, z).to(dev)
    x = _x(5, K, torch.bfloat16, dev, seed=2)
    _bits_equal(m(x[:1]), ops.gemm_wq_skinny(x[:1], Wq, s, zp_w=z))       # gemv_max_m = 0, the default
    m.gemv_max_m = 4
    for M in (1, 4):
        _bits_equal(m(x[:M]), ops.gemm_wq_gemv(x[:M], Wq, s, zp_w=z))
    _bits_equal(m(x), ops.gemm_wq_skinny(x, Wq, s, zp_w=z))
