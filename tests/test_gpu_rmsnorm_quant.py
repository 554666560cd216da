"""``qt_rmsnorm_quantize_i8`` on the device (include/quantool_amd.h).

The kernel's order of summation over K is its own, so the contract has three parts.  Given the kernel's ``rstd``, ``Y``
is exactly the two roundings of the header's step 5 (computed by torch from that ``rstd``); ``(Xq, s_x, zp_x)`` is
exactly ``quantize_tokens_i8(Y)``; and ``rstd`` lies within one rounding per operation on the longest path of the fp64
value -- and equals torch's own chain to the bit on rows whose sum of squares is exact in fp32, where ``Y`` then equals
``LlamaRMSNorm`` to the bit.  A row's result depends on the row alone, whatever its index, pitch and alignment; and
nothing outside the five outputs is written."""
import pytest
import torch

from tests.exact_inputs import assert_exactly_summable

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}                 # unit roundoff
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}
HALF_SUBNORMAL = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}     # half the spacing below MIN_NORMAL
KS = [1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 2056, 4104]
MS = [1, 3, 65]
LAYOUTS = ["contiguous", "pitch+8", "pitch+3", "shifted"]
EPS = 1e-5


def _bits(t):
    return t.contiguous().view(torch.int16)


def _perm(K, dev, seed=5):
    return torch.randperm(K, generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(dev)


def _n_roundings(K):
    """One rounding per operation on the longest path to ``rstd``: the square, the lane's 8 ceil(K/2048) adds (the first
    onto 0 is exact, the count is kept as the bound states it), 6 butterfly steps, 3 waves, the mean, the eps add and 2
    for the reciprocal square root (the kernel's is correctly rounded and spends one)."""
    return 8 * ((K + 2047) // 2048) + 13


def _inputs(M, K, dt, seed):
    """(x, weight) on the CPU: randn * 3 with every fifth column times 40, weight = randn * 0.5 + 1."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 3
    x[:, ::5] *= 40
    w = torch.randn(K, generator=g) * 0.5 + 1
    return x.to(dt), w.to(dt)


def _layout(x, layout, dev):
    """The same values as a device view of the given layout (unit column stride throughout)."""
    M, K = x.shape
    if layout == "contiguous":
        return x.to(dev)
    if layout in ("pitch+8", "pitch+3"):
        pad = 8 if layout == "pitch+8" else 3
        buf = torch.full((M, K + pad), 7.0, dtype=x.dtype, device=dev)
        buf[:, :K] = x.to(dev)
        return buf[:, :K]
    if layout == "shifted":                                  # one element behind a 16-byte boundary
        buf = torch.zeros(M * K + 8, dtype=x.dtype, device=dev)
        v = buf[1:1 + M * K].view(M, K)
        v.copy_(x)
        assert v.data_ptr() % 16 == 2
        return v
    raise KeyError(layout)


def _triple_equal(got, want, what):
    for name, a, b in zip(("Xq", "s_x", "zp_x"), got, want):
        assert (a is None) == (b is None), f"{what}: {name}"
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} places"


def _step5(x, w, rstd):
    """The header's step 5 by torch on the device, from the kernel's own rstd."""
    return w * (x.float() * rstd[:, None]).to(x.dtype)


# ---- B1: the decomposition, any finite input ------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K", KS)
def test_decomposition_and_bounds(ops, dev, K, layout):
    perm = _perm(K, dev, seed=K)
    n = _n_roundings(K)
    worst_r, worst_y = 0.0, 0.0
    for M in MS:
        for dt in DTYPES:
            xc, wc = _inputs(M, K, dt, seed=M * 100003 + K)
            x, w = _layout(xc, layout, dev), wc.to(dev)
            assert x.stride(1) == 1 and x.stride(0) == K + {"pitch+8": 8, "pitch+3": 3}.get(layout, 0)
            x64, w64 = x.double(), w.double()
            r64 = 1.0 / torch.sqrt(x64.pow(2).mean(-1) + EPS)
            y64 = w64 * x64 * r64[:, None]
            n64 = x64 * r64[:, None]
            u, tiny, eta = UNIT[dt], MIN_NORMAL[dt], HALF_SUBNORMAL[dt]
            rel = 2 * u + u * u + 2 * n * 2.0 ** -24
            bound = y64.abs() * rel
            # the unit-roundoff model of the bound holds where both roundings land in the normal range; an fp16 result
            # below 2^-14 is rounded to a multiple of 2^-24 instead, so there each rounding adds at most half of that
            # (without the term the first fp16 case of K = 257 and of K = 4104 stands at 3.6 and 3.8 of the plain bound
            # on the device, in elements with |x r| < 2^-14; bf16 alone passes the plain bound, at 0.89 and 0.96 of it)
            under = (n64.abs() < tiny * (1 + 4 * u)) | (y64.abs() < tiny * (1 + 4 * u))
            bound = torch.where(under, bound + (w64.abs() * (1 + u) + 1) * eta, bound)
            for symmetric in (True, False):
                for col_perm in (None, perm):
                    what = f"{M}x{K} {layout} {dt} sym={symmetric} perm={col_perm is not None}"
                    Y, Xq, s_x, zp_x, rstd = ops.rmsnorm_quantize_i8(x, w, EPS, symmetric=symmetric, col_perm=col_perm,
                                                                     return_rstd=True)
                    torch.cuda.synchronize()
                    assert Y.shape == (M, K) and Y.dtype == dt and Y.is_contiguous() and rstd.dtype == torch.float32
                    assert torch.isfinite(rstd).all() and torch.isfinite(Y.float()).all(), what
                    assert torch.equal(_bits(Y), _bits(_step5(x, w, rstd))), what
                    _triple_equal((Xq, s_x, zp_x), ops.quantize_tokens_i8(Y, symmetric=symmetric, col_perm=col_perm),
                                  what)
                    err_r = ((rstd.double() - r64).abs() / r64).max().item() / (n * 2.0 ** -24)
                    err_y = ((Y.double() - y64).abs() / bound.clamp_min(1e-300)).max().item()
                    worst_r, worst_y = max(worst_r, err_r), max(worst_y, err_y)
                    assert err_r <= 1.0, f"{what}: rstd is {err_r} of its bound"
                    assert err_y <= 1.0, f"{what}: Y is {err_y} of its bound"
                    four = ops.rmsnorm_quantize_i8(x, w, EPS, symmetric=symmetric, col_perm=col_perm)
                    assert len(four) == 4 and torch.equal(_bits(four[0]), _bits(Y))
                    _triple_equal(four[1:], (Xq, s_x, zp_x), what + " (no rstd)")
    print(f"K={K} {layout}: rstd at most {worst_r:.3f} of its bound, Y at most {worst_y:.3f} of its bound")


@pytest.mark.parametrize("K", [8, 257, 2056])
def test_a_row_whose_squares_overflow_is_zero_as_torchs_is(ops, dev, K):
    """A row holding 2^70 (bf16): its squares overflow fp32, the sum is infinite whatever its order, rstd is 0 and the
    row is zeros, as ``LlamaRMSNorm`` leaves it, to the bit."""
    from transformers.models.llama.modeling_llama import LlamaRMSNorm

    dt = torch.bfloat16
    xc, wc = _inputs(3, K, dt, seed=K)
    xc[1, K // 2] = 2.0 ** 70
    x, w = xc.to(dev), wc.to(dev)
    ref = LlamaRMSNorm(K, EPS).to(dev, dt)
    ref.weight.data.copy_(w)
    with torch.no_grad():
        want = ref(x)
    for symmetric in (True, False):
        Y, Xq, s_x, zp_x, rstd = ops.rmsnorm_quantize_i8(x, w, EPS, symmetric=symmetric, return_rstd=True)
        torch.cuda.synchronize()
        assert float(rstd[1]) == 0.0 and bool((Y[1] == 0).all()) and bool((rstd[[0, 2]] > 0).all())
        assert torch.equal(_bits(Y[1]), _bits(want[1]))
        assert torch.equal(_bits(Y), _bits(_step5(x, w, rstd)))
        _triple_equal((Xq, s_x, zp_x), ops.quantize_tokens_i8(Y, symmetric=symmetric), f"K={K} sym={symmetric}")
        assert float(s_x[1]) == 2.0 ** -23 and bool((Xq[1] == (0 if symmetric else -128)).all())


# ---- B2: exact rows equal torch to the bit --------------------------------------------------------------------------
def _exact_rows(K, dt, seed):
    """13 rows of +-k/16, k in 1 ... 31, row i times 2^(i - 6): exact in bf16 and fp16, and the sum of squares of a
    row is exact in fp32 in every order (guarded)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(1, 32, (13, K), generator=g)
    sign = torch.randint(0, 2, (13, K), generator=g) * 2 - 1
    # before the row's power of two (which scales every partial sum alike): sum (k/16)^2 in units of 2^-8
    assert_exactly_summable((k.double() / 16).pow(2).sum(1), 8, f"K={K}")
    x = (k * sign).double() / 16 * torch.exp2(torch.arange(-6, 7).double())[:, None]
    xt = x.to(dt)
    assert torch.equal(xt.double(), x)
    return xt


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("K", [1, 7, 8, 257, 2048, 2056, 4104])
def test_exact_rows_equal_torch_to_the_bit(ops, dev, K, eps):
    from transformers.models.llama.modeling_llama import LlamaRMSNorm

    assert K <= 17458                                              # 961 K < 2^24
    for dt in DTYPES:
        x = _exact_rows(K, dt, seed=K).to(dev)
        w = _inputs(1, K, dt, seed=K + 1)[1].to(dev)
        ref = LlamaRMSNorm(K, eps).to(dev, dt)
        ref.weight.data.copy_(w)
        with torch.no_grad():
            want_y = ref(x)
            want_r = torch.rsqrt(x.float().pow(2).mean(-1) + eps)
        Y, Xq, s_x, zp_x, rstd = ops.rmsnorm_quantize_i8(x, w, eps, symmetric=False, return_rstd=True)
        torch.cuda.synchronize()
        ulps = (rstd.view(torch.int32) - want_r.view(torch.int32)).abs()
        print(f"K={K} eps={eps} {dt}: rstd differs from torch's in {int((ulps != 0).sum())} of 13 rows, by at most "
              f"{int(ulps.max())} ulp")
        assert torch.equal(rstd.view(torch.int32), want_r.view(torch.int32)), f"K={K} {dt}: rstd {ulps.tolist()}"
        assert torch.equal(_bits(Y), _bits(want_y)), f"K={K} {dt}"
        _triple_equal((Xq, s_x, zp_x), ops.quantize_tokens_i8(want_y, symmetric=False), f"K={K} {dt}")


# ---- B3: a row's result depends on the row alone --------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_a_rows_result_depends_on_the_row_alone(ops, dev, dt):
    K = 2056
    row, w = _inputs(1, K, dt, seed=77)
    others = _inputs(64, K, dt, seed=78)[0]
    w = w.to(dev)
    perm = _perm(K, dev, seed=3)
    for symmetric, col_perm in ((False, None), (True, perm)):
        first = None
        for M, m in ((1, 0), (64, 37)):
            for pad in (0, 8, 3):
                for shift in (0, 1):
                    xc = others[:M].clone()
                    xc[m] = row[0]
                    buf = torch.zeros(M * (K + pad) + 8, dtype=dt, device=dev)
                    x = buf[shift:shift + M * (K + pad)].view(M, K + pad)[:, :K]
                    x.copy_(xc)
                    assert x.data_ptr() % 16 == 2 * shift and x.stride() == (K + pad, 1)
                    Y, Xq, s_x, zp_x, rstd = ops.rmsnorm_quantize_i8(x, w, EPS, symmetric=symmetric, col_perm=col_perm,
                                                                     return_rstd=True)
                    torch.cuda.synchronize()
                    got = (rstd[m:m + 1].view(torch.int32), _bits(Y[m]), Xq[m], s_x[m:m + 1].view(torch.int32),
                           None if zp_x is None else zp_x[m:m + 1])
                    if first is None:
                        first = got
                        continue
                    for name, a, b in zip(("rstd", "Y", "Xq", "s_x", "zp_x"), got, first):
                        assert (a is None and b is None) or torch.equal(a, b), \
                            f"{dt} sym={symmetric}: {name} of the row at ({m} of {M}, pitch K+{pad}, shift {shift}) differs"


# ---- B4: only the outputs are written -------------------------------------------------------------------------------
PAD = 64


@pytest.mark.parametrize("M,K", [(3, 1000), (5, 1031), (1, 32768)])
@pytest.mark.parametrize("symmetric", [True, False])
def test_only_the_outputs_are_written(ops, dev, M, K, symmetric):
    from quantool_amd.hip import _lib

    lib = _lib.load()
    dt = torch.bfloat16
    xc, wc = _inputs(M, K, dt, seed=21)
    x, w = xc.to(dev), wc.to(dev)
    ldy = K + 5
    xq = torch.full((PAD + M * K + PAD,), 0x5A, dtype=torch.int8, device=dev)
    sx = torch.full((PAD + M + PAD,), -7.5, dtype=torch.float32, device=dev)
    zp = torch.full((PAD + M + PAD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    rs = torch.full((PAD + M + PAD,), -7.5, dtype=torch.float32, device=dev)
    yb = torch.full((PAD + M * ldy + PAD,), 0x5A5A, dtype=torch.int16, device=dev)
    st = lib.qt_rmsnorm_quantize_i8(
        x.data_ptr(), x.stride(0), w.data_ptr(), _lib.QT_BF16, M, K, EPS, None, int(symmetric), xq.data_ptr() + PAD,
        sx.data_ptr() + 4 * PAD, zp.data_ptr() + 4 * PAD, yb.data_ptr() + 2 * PAD, ldy, rs.data_ptr() + 4 * PAD,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, lib.qt_last_error()
    for name, buf, n in (("Xq", xq, M * K), ("s_x", sx, M), ("zp_x", zp, M), ("rstd", rs, M), ("Y", yb, M * ldy)):
        poison = buf[0].item()
        assert bool((buf[:PAD] == poison).all()) and bool((buf[PAD + n:] == poison).all()), name
    y = yb[PAD:PAD + M * ldy].view(M, ldy)
    assert bool((y[:, K:] == 0x5A5A).all())                  # the pitch gap of Y
    rstd = rs[PAD:PAD + M]
    want_y = _step5(x, w, rstd)
    assert torch.equal(y[:, :K], _bits(want_y))
    want = ops.quantize_tokens_i8(want_y, symmetric=symmetric)
    assert torch.equal(xq[PAD:PAD + M * K].view(M, K), want[0])
    assert torch.equal(sx[PAD:PAD + M], want[1])
    if symmetric:
        assert bool((zp == 0x5A5A5A5A).all())                # never written when symmetric
    else:
        assert torch.equal(zp[PAD:PAD + M], want[2])
    again = ops.rmsnorm_quantize_i8(x, w, EPS, symmetric=symmetric, return_rstd=True)
    assert torch.equal(again[4], rstd) and torch.equal(_bits(again[0]), _bits(want_y))


def test_col_perm_is_clamped_into_the_row(ops, dev):
    """An index outside [0, K) reads the row's first or last element: never anything outside the row."""
    xc, wc = _inputs(3, 100, torch.bfloat16, seed=4)
    x, w = xc.to(dev), wc.to(dev)
    perm = torch.arange(100, dtype=torch.int32)
    perm[5], perm[50], perm[99] = -7, 100000, 100
    got = ops.rmsnorm_quantize_i8(x, w, EPS, symmetric=False, col_perm=perm.to(dev))
    want = ops.rmsnorm_quantize_i8(x, w, EPS, symmetric=False, col_perm=perm.clamp(0, 99).to(dev))
    assert torch.equal(_bits(got[0]), _bits(want[0]))
    _triple_equal(got[1:], want[1:], "clamped col_perm")


def test_refusals_through_ops(ops, dev):
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    w = torch.ones(64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(TypeError, match="X's dtype"):
        ops.rmsnorm_quantize_i8(x, w.to(torch.float16), EPS)
    with pytest.raises(ValueError, match="X's device"):
        ops.rmsnorm_quantize_i8(x, w.cpu(), EPS)
    with pytest.raises(ValueError, match="device tensor"):
        ops.rmsnorm_quantize_i8(x.cpu(), w, EPS)
    with pytest.raises(ValueError, match="unit column stride"):
        ops.rmsnorm_quantize_i8(x[:, ::2], w[:32], EPS)
    with pytest.raises(TypeError, match="bf16 or fp16"):
        ops.rmsnorm_quantize_i8(x.float(), w.float(), EPS)
    with pytest.raises(ValueError, match="weight must be contiguous"):
        ops.rmsnorm_quantize_i8(x, w[:63], EPS)
    with pytest.raises(ValueError, match="col_perm"):
        ops.rmsnorm_quantize_i8(x, w, EPS, col_perm=torch.zeros(63, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="col_perm"):
        ops.rmsnorm_quantize_i8(x, w, EPS, col_perm=torch.zeros(128, dtype=torch.int32, device=dev)[::2])
    with pytest.raises(ValueError, match="non-empty"):
        ops.rmsnorm_quantize_i8(x[:0], w, EPS)
    with pytest.raises(ValueError, match="eps"):
        ops.rmsnorm_quantize_i8(x, w, -1.0)
    big = torch.zeros(1, 32768 + 8, dtype=torch.bfloat16, device=dev)
    with pytest.raises(Exception, match="32768"):
        ops.rmsnorm_quantize_i8(big, torch.ones(32768 + 8, dtype=torch.bfloat16, device=dev), EPS)
