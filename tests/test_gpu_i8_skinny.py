"""qt_gemm_i8_skinny / qt_gemm_i8_skinny_grouped: the A8 decode GEMV.

Its contract is bit equality with the tiled qt_gemm_i8 / qt_gemm_i8_grouped on the same arguments, so every comparison
here is on bit patterns (``.view(torch.int16)`` + ``torch.equal``).  That alone would pass two kernels wrong in the same
way, so the same cases also go against the fp64 reference of tests/ckpt_reference.py within the project's own bound for
this sequence (``gemm_i8_tolerance``), and a one-hot test pins which weight element every lane slot multiplies."""
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_runtime_edges import _leaves, _levels, _qweight, cr_wsum

pytestmark = pytest.mark.gpu

SHAPES = [(200, 1024), (96, 128), (160, 320), (64, 1000), (4096, 4096), (4096, 14336), (6144, 4096)]
SENTINEL = 0x7B7B          # a bf16 / fp16 bit pattern no case below produces in bulk


def _same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    a16, b16 = a.view(torch.int16), b.view(torch.int16)
    if not torch.equal(a16, b16):
        bad = (a16 != b16).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {a.numel()} elements differ in bits, first at "
                             f"{bad[0].tolist()}: {a[tuple(bad[0])].item()} vs {b[tuple(bad[0])].item()}")


def _acts16(K, dev, seed):
    """16 activation rows with outlier channels, an all-zero row (the eps clamp) and an all-positive one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(16, K, generator=g)
    x[:, torch.randperm(K, generator=g)[: max(1, K // 64)]] *= 10
    x[9] = 0.0
    x[3] = x[3].abs() + 0.5
    return x.to(torch.bfloat16).to(dev)


def _bias(N, dtype, dev, seed):
    return (torch.randn(N, generator=torch.Generator().manual_seed(seed)) * 0.1).to(dtype).to(dev)


# ---- 1 + 2: every M, every form, against the tiled kernel's bits and against fp64 -------------------------------------
@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("bits", [8, 4])
def test_skinny_equals_tiled_bits_and_fp64(ops, dev, N, K, bits):
    q8 = _levels((N, K), bits, seed=N + 3 * K + bits)
    X = _acts16(K, dev, seed=K + N)
    for grouped in (False, True):
        G = (K + 127) // 128 if grouped else 1
        t = _leaves(q8, bits, G, seed=K + G)
        Wq, s_w, wsum = _qweight(t, dev), t["weight_scale"].to(dev), cr_wsum(q8, G).to(dev)
        for asym in (False, True):
            Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
            y64, mag = cr.a8_linear(Xq, s_x, zp_x, t)
            for dt in (torch.bfloat16, torch.float16):
                for with_bias in (False, True):
                    bias = _bias(N, dt, dev, seed=N) if with_bias else None
                    what = f"N={N} K={K} bits={bits} G={G} asym={asym} {dt} bias={with_bias}"
                    for M in range(1, 17):
                        kw = dict(K=K, zp_x=None if zp_x is None else zp_x[:M], wsum=wsum if asym else None,
                                  bias=bias, out_dtype=dt)
                        want = ops.gemm_i8(Xq[:M], s_x[:M], Wq, s_w, **kw)
                        got = ops.gemm_i8_skinny(Xq[:M], s_x[:M], Wq, s_w, **kw)
                        torch.cuda.synchronize()
                        _same_bits(got, want, f"{what} M={M}")
                        if M in (1, 7, 16):
                            y, m = y64[:M], mag[:M]
                            if with_bias:
                                b = bias.cpu().double()
                                y, m = y + b, m + b.abs()
                            cr.assert_within(got, y, cr.gemm_i8_tolerance(got.cpu(), m, G), f"{what} M={M} vs fp64")


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("grouped", [False, True])
def test_skinny_misaligned_operands(ops, dev, bits, grouped):
    """K % 16 == 0, but Xq starts one byte and Wq one byte (int8) / one word (packed int4) past a 16-byte boundary."""
    M, N, K = 11, 70, 1024
    q8 = _levels((N, K), bits, seed=5)
    G = K // 128 if grouped else 1
    t = _leaves(q8, bits, G, seed=6)
    W0 = _qweight(t, dev)
    wbuf = torch.zeros(W0.numel() + 16, dtype=W0.dtype, device=dev)
    Wq = wbuf[1:1 + W0.numel()].view(W0.shape)
    Wq.copy_(W0)
    X = _acts16(K, dev, seed=4)[:M]
    Xq0, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=False)
    xbuf = torch.zeros(M * K + 16, dtype=torch.int8, device=dev)
    Xq = xbuf[1:1 + M * K].view(M, K)
    Xq.copy_(Xq0)
    assert Xq.data_ptr() % 16 == 1 and Wq.data_ptr() % 16 == (1 if bits == 8 else 4)
    assert Xq.is_contiguous() and Wq.is_contiguous()
    kw = dict(K=K, zp_x=zp_x, wsum=cr_wsum(q8, G).to(dev), out_dtype=torch.bfloat16)
    s_w = t["weight_scale"].to(dev)
    got = ops.gemm_i8_skinny(Xq, s_x, Wq, s_w, **kw)
    torch.cuda.synchronize()
    _same_bits(got, ops.gemm_i8(Xq, s_x, Wq, s_w, **kw), "misaligned")
    _same_bits(got, ops.gemm_i8_skinny(Xq0, s_x, W0, s_w, **kw), "misaligned vs aligned")
    y64, mag = cr.a8_linear(Xq, s_x, zp_x, t)
    cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, G), "misaligned vs fp64")


# ---- raw C ABI calls: a caller-owned Y (row pitch, sentinels) ---------------------------------------------------------
def _raw(ops, name, *args):
    from quantool_amd.hip import _lib

    _lib.check(name, getattr(_lib.load(), name)(*args))


def _raw_skinny(ops, Xq, M, K, Wq, N, s_x, zp_x, s_w, G, wsum, bias, Y, ldy):
    from quantool_amd.hip import _lib

    fmt = _lib.QT_W_INT8 if Wq.dtype == torch.int8 else _lib.QT_W_INT4_PACKED
    _raw(ops, "qt_gemm_i8_skinny", Xq.data_ptr(), M, K, Wq.data_ptr(), fmt, N, s_x.data_ptr(), ops._ptr(zp_x),
         s_w.data_ptr(), G, ops._ptr(wsum), ops._ptr(bias), Y.data_ptr(), ops._dtype_code(Y), ldy, ops._stream())


def _raw_grouped(ops, name, Xq, K, row_idx, R, offsets, E, Wq, N, s_x, zp_x, s_w, G, wsum, Y, ldy):
    from quantool_amd.hip import _lib

    fmt = _lib.QT_W_INT8 if Wq.dtype == torch.int8 else _lib.QT_W_INT4_PACKED
    _raw(ops, name, Xq.data_ptr(), K, ops._ptr(row_idx), R, offsets.data_ptr(), E, Wq.data_ptr(), fmt, N,
         s_x.data_ptr(), ops._ptr(zp_x), s_w.data_ptr(), G, ops._ptr(wsum), Y.data_ptr(), ops._dtype_code(Y), ldy,
         ops._stream())


def _sentinel(shape, dtype, dev):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=dev).view(dtype)


def _untouched(Y):
    return bool((Y.view(torch.int16) == SENTINEL).all())


@pytest.mark.parametrize("bits", [8, 4])
def test_skinny_row_pitch_leaves_the_padding_columns(ops, dev, bits):
    M, N, K, ldy = 7, 200, 1024, 217
    q8 = _levels((N, K), bits, seed=8)
    G = K // 128
    t = _leaves(q8, bits, G, seed=9)
    Wq, s_w, wsum = _qweight(t, dev), t["weight_scale"].to(dev), cr_wsum(q8, G).to(dev)
    Xq, s_x, zp_x = ops.quantize_tokens_i8(_acts16(K, dev, seed=2)[:M], symmetric=False)
    Y = _sentinel((M + 1, ldy), torch.bfloat16, dev)
    _raw_skinny(ops, Xq, M, K, Wq, N, s_x, zp_x, s_w, G, wsum, None, Y, ldy)
    torch.cuda.synchronize()
    _same_bits(Y[:M, :N].contiguous(), ops.gemm_i8(Xq, s_x, Wq, s_w, K=K, zp_x=zp_x, wsum=wsum), "ldy > N")
    assert _untouched(Y[:M, N:]) and _untouched(Y[M:])


# ---- 3: the lane map ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("K", [1056, 1000])
@pytest.mark.parametrize("grouped", [False, True])
def test_skinny_one_hot_rows_read_the_weight(ops, dev, bits, K, grouped):
    """Xq row m = e_{k_m} (value 1, s_x = 1) against an asymmetric random W with power-of-two scales:
    Y[m, n] = s_w[n, g(k_m)] q[n, k_m] exactly.  k_m runs over every column, so over every 16-byte slot of every lane
    of every wave, on the 16-byte path (K = 1056: a last group of 32 columns) and the element-wise one (K = 1000: a last
    group of 104 columns, a partial 16-byte chunk)."""
    N = 40
    G = (K + 127) // 128 if grouped else 1
    q8 = _levels((N, K), bits, seed=K + bits)
    assert not torch.equal(q8[:, :N], q8[:, :N].T)
    t = _leaves(q8, bits, G, seed=K, pow2=True)
    Wq, s_w = _qweight(t, dev), t["weight_scale"].to(dev)
    w = q8.float() * (t["weight_scale"][:, torch.arange(K) // 128] if grouped else t["weight_scale"])   # exact
    ones = torch.ones(16, device=dev)
    for k0 in range(0, K, 16):
        ks = torch.arange(k0, min(k0 + 16, K))
        M = len(ks)
        Xq = torch.zeros(M, K, dtype=torch.int8)
        Xq[torch.arange(M), ks] = 1
        Y = ops.gemm_i8_skinny(Xq.to(dev), ones[:M], Wq, s_w, K=K, out_dtype=torch.float16)
        torch.cuda.synchronize()
        _same_bits(Y.cpu(), (w[:, ks].T + 0.0).to(torch.float16).contiguous(), f"columns {k0}..")


# ---- 4: the accumulator bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("grouped", [False, True])
def test_skinny_at_the_accumulator_bound(ops, dev, bits, grouped):
    M, N, K = 16, 48, 32768
    g = torch.Generator().manual_seed(bits + grouped)
    lo, hi = (-8, 7) if bits == 4 else (-128, 127)
    Xq = torch.where(torch.rand(M, K, generator=g) < 0.5, -128, 127).to(torch.int8)
    Xq[: M // 2] = -128                                          # rows of one sign: the largest |acc|
    q8 = torch.where(torch.rand(N, K, generator=g) < 0.5, lo, hi).to(torch.int8)
    q8[: N // 2] = lo
    s_x = (torch.rand(M, generator=g) * 1e-3 + 1e-5).to(dev)
    zp_x = torch.randint(-128, 128, (M,), generator=g, dtype=torch.int32)
    zp_x[:4] = torch.tensor([-128, 127, 0, 1], dtype=torch.int32)
    G = K // 128 if grouped else 1
    t = _leaves(q8, bits, G, seed=3)
    Wq, s_w, wsum = _qweight(t, dev), t["weight_scale"].to(dev), cr_wsum(q8, G).to(dev)
    Xq, zp_x = Xq.to(dev), zp_x.to(dev)
    for z in (None, zp_x):
        kw = dict(K=K, zp_x=z, wsum=None if z is None else wsum, bias=_bias(N, torch.bfloat16, dev, 1))
        got = ops.gemm_i8_skinny(Xq, s_x, Wq, s_w, **kw)
        torch.cuda.synchronize()
        _same_bits(got, ops.gemm_i8(Xq, s_x, Wq, s_w, **kw), f"K = 32768, zp_x {z is not None}")
        y64, mag = cr.a8_linear(Xq, s_x, z, t, kw["bias"])
        cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, G), "K = 32768 vs fp64")


# ---- 5: refusals ----------------------------------------------------------------------------------------------------
def test_skinny_refusals_write_nothing(ops, dev):
    from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

    N, K = 32, 256
    Wq = torch.zeros(N, K, dtype=torch.int8, device=dev)
    s_w = torch.ones(N, 1, device=dev)
    Xq = torch.ones(17, K, dtype=torch.int8, device=dev)
    s_x = torch.ones(17, device=dev)
    Y = _sentinel((17, N), torch.bfloat16, dev)
    for M in (0, 17, -1):
        with pytest.raises(HipBackendError) as e:
            _raw_skinny(ops, Xq, M, K, Wq, N, s_x, None, s_w, 1, None, None, Y, N)
        assert e.value.status == QT_ERR_INVALID
        with pytest.raises(ValueError):
            ops.gemm_i8_skinny(Xq[:max(M, 0)], s_x[:max(M, 0)], Wq, s_w)
    Kbig = 32768 + 128
    Xb = torch.ones(1, Kbig, dtype=torch.int8, device=dev)
    Wb = torch.zeros(N, Kbig, dtype=torch.int8, device=dev)
    with pytest.raises(HipBackendError) as e:
        _raw_skinny(ops, Xb, 1, Kbig, Wb, N, s_x, None, s_w, 1, None, None, Y, N)
    assert e.value.status == QT_ERR_INVALID
    with pytest.raises(ValueError):
        ops.gemm_i8_skinny(Xb, s_x[:1], Wb, s_w)
    # zp_x without wsum, a G that is neither 1 nor ceil(K/128), a row pitch below N: qt_gemm_i8's refusals
    zp = torch.zeros(17, dtype=torch.int32, device=dev)
    for args in ((Xq, 4, K, Wq, N, s_x, zp, s_w, 1, None, None, Y, N), (Xq, 4, K, Wq, N, s_x, None, s_w, 3, None, None, Y, N),
                 (Xq, 4, K, Wq, N, s_x, None, s_w, 1, None, None, Y, N - 1)):
        with pytest.raises(HipBackendError):
            _raw_skinny(ops, *args)
    # grouped: floor(R/16) + min(E, R) = 65535 + 8 slots
    E, R = 8, 16 * 65535
    Wg = torch.zeros(E, 16, K, dtype=torch.int8, device=dev)
    sg = torch.ones(E, 16, 1, device=dev)
    off = torch.zeros(E + 1, dtype=torch.int32, device=dev)
    row_idx = torch.zeros(R, dtype=torch.int32, device=dev)
    Yg = _sentinel((R, 16), torch.bfloat16, dev)
    with pytest.raises(HipBackendError) as e:
        _raw_grouped(ops, "qt_gemm_i8_skinny_grouped", Xq, K, row_idx, R, off, E, Wg, 16, s_x, None, sg, 1, None, Yg, 16)
    assert e.value.status == QT_ERR_INVALID
    with pytest.raises(HipBackendError):
        ops.gemm_i8_skinny_grouped(Xq, s_x, Wg, sg, off, row_idx=row_idx)
    with pytest.raises(HipBackendError):
        _raw_grouped(ops, "qt_gemm_i8_skinny_grouped", Xb, Kbig, None, 1, off, E, Wg, 16, s_x, None, sg, 1, None, Yg, 16)
    torch.cuda.synchronize()
    assert _untouched(Y) and _untouched(Yg)


# ---- 6: the grouped form --------------------------------------------------------------------------------------------
GROUPED_COUNTS = [
    [0, 1, 15, 16, 17, 0, 3, 0],          # empty first / middle / last, one tile short, one tile, a tile and one row
    [0, 0, 0, 40, 0, 0, 0, 0],            # one expert holds every row
    [5, 2, 1, 1, 33, 1, 7, 2],
]


@pytest.mark.parametrize("counts", GROUPED_COUNTS)
@pytest.mark.parametrize("bits,grouped", [(8, False), (4, True), (8, True), (4, False)])
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("gather", [True, False])
def test_skinny_grouped_equals_tiled_grouped(ops, dev, counts, bits, grouped, asym, gather):
    from tests.test_gpu_moe import _grouped_case

    E = len(counts)
    for N, K, dt in ((200, 1024, torch.bfloat16), (72, 1000, torch.float16)):
        idx, Xq, s_x, zp_x, Wq, s_w, wsum, q8 = _grouped_case(dev, E, counts, N, K, bits, grouped, asym, dt,
                                                              seed=sum(counts) + K)
        offsets, src_token, _, _ = ops.moe_route(idx, E)
        ws = wsum if asym else None
        if gather:
            A, sa, za, ri = Xq, s_x, zp_x, src_token
        else:
            src = src_token.long()
            A, sa, ri = Xq[src].contiguous(), s_x[src].contiguous(), None
            za = None if zp_x is None else zp_x[src].contiguous()
        kw = dict(row_idx=ri, K=K, zp_x=za, wsum=ws, out_dtype=dt)
        want = ops.gemm_i8_grouped(A, sa, Wq, s_w, offsets, **kw)
        got = ops.gemm_i8_skinny_grouped(A, sa, Wq, s_w, offsets, **kw)
        torch.cuda.synchronize()
        assert offsets.cpu().tolist()[-1] == sum(counts)
        _same_bits(got, want, f"counts {counts} N={N} K={K}")
        # and every expert's rows against fp64 on that expert's weight
        off = offsets.cpu().tolist()
        G = s_w.shape[-1]
        for e in range(E):
            lo, hi = off[e], off[e + 1]
            if hi == lo:
                continue
            rows = src_token.long()[lo:hi].cpu() if gather else torch.arange(lo, hi)
            t = {"weight": q8[e], "weight_scale": s_w[e].cpu(), "weight_shape": torch.tensor([N, K])}
            y64, mag = cr.a8_linear(A.cpu()[rows], sa.cpu()[rows], None if za is None else za.cpu()[rows], t)
            cr.assert_within(got[lo:hi], y64, cr.gemm_i8_tolerance(got[lo:hi].cpu(), mag, G), f"expert {e} vs fp64")


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("asym", [False, True])
def test_skinny_grouped_leaves_rows_past_the_last_offset(ops, dev, bits, asym):
    """Dropped routing slots: offsets[E] < R, and the rows past it keep their sentinel (as do the padding columns)."""
    from tests.test_gpu_moe import _grouped_case

    E, counts, N, K, ldy = 8, [3, 0, 17, 1, 0, 16, 2, 4], 56, 640, 64
    idx, Xq, s_x, zp_x, Wq, s_w, wsum, _ = _grouped_case(dev, E, counts, N, K, bits, True, asym, torch.bfloat16, seed=7)
    idx[::5] = E                                             # dropped
    offsets, src_token, _, _ = ops.moe_route(idx, E)
    R = idx.numel()
    live = int(offsets[-1])
    assert 0 < live < R
    ws = wsum if asym else None
    G = s_w.shape[-1]
    Ys = [_sentinel((R, ldy), torch.bfloat16, dev) for _ in range(2)]
    for name, Y in zip(("qt_gemm_i8_grouped", "qt_gemm_i8_skinny_grouped"), Ys):
        _raw_grouped(ops, name, Xq, K, src_token, R, offsets, E, Wq, N, s_x, zp_x, s_w, G, ws, Y, ldy)
    torch.cuda.synchronize()
    _same_bits(Ys[1], Ys[0], "offsets[E] < R")
    assert _untouched(Ys[1][live:]) and _untouched(Ys[1][:, N:]) and not _untouched(Ys[1][:live, :N])


# ---- 7: the modules -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic_checkpoints(dev, tmp_path_factory):
    """{(arch, scheme): directory} of write_synthetic A8 checkpoints over the odd-width models of test_gpu_ckpt_e2e."""
    import os

    from tests.test_gpu_ckpt_e2e import _plugin_checkpoint

    root = tmp_path_factory.mktemp("a8_skinny_ckpts")
    cwd = os.getcwd()
    os.chdir(root)
    made = {}
    try:
        def get(arch, scheme):
            if (arch, scheme) not in made:
                if (arch, "base") not in made:
                    made[(arch, "base")] = _plugin_checkpoint(dev, arch, "gptq", "W8A16", root / f"{arch}_base")
                cfg, dense, linears = cr.from_checkpoint(made[(arch, "base")])
                bits, act = {"W8A8": (8, "sym"), "W4A8": (4, "asym")}[scheme]
                cr.write_synthetic(root / f"{arch}_{scheme}", cfg, dense, linears, bits=bits, act=act, seed=bits)
                made[(arch, scheme)] = root / f"{arch}_{scheme}"
            return made[(arch, scheme)]
        yield get
    finally:
        os.chdir(cwd)


class _Counter:
    def __init__(self, monkeypatch, ops, name):
        self.n = 0
        real = getattr(ops, name)

        def counted(*a, **kw):
            self.n += 1
            return real(*a, **kw)

        monkeypatch.setattr(ops, name, counted)


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_quantized_linear_forward_is_the_same_with_and_without_the_gemv(ops, dev, synthetic_checkpoints, monkeypatch,
                                                                        scheme):
    from quantool_amd.engine.qlinear import QuantizedLinear, load_quantized

    model = load_quantized(synthetic_checkpoints("llama", scheme), device=dev)
    lins = {n: m for n, m in model.named_modules() if isinstance(m, QuantizedLinear)}
    assert len(lins) == 14
    default = QuantizedLinear.skinny_max_m
    counter = _Counter(monkeypatch, ops, "gemm_i8_skinny")
    for M in (1, 7, 16, 17):
        for name, m in lins.items():
            x = (torch.randn(M, m.in_features, generator=torch.Generator().manual_seed(M)) * 2).to(torch.bfloat16).to(dev)
            before = counter.n
            with torch.no_grad():
                y1 = m(x)
                assert counter.n - before == int(1 <= M <= min(default, 16))
                monkeypatch.setattr(QuantizedLinear, "skinny_max_m", 0)
                y0 = m(x)
                assert counter.n - before == int(1 <= M <= min(default, 16))
                monkeypatch.setattr(QuantizedLinear, "skinny_max_m", 16)
                y16 = m(x)
                monkeypatch.setattr(QuantizedLinear, "skinny_max_m", default)
            torch.cuda.synchronize()
            _same_bits(y1, y0, f"{name} M={M} default vs 0")
            _same_bits(y16, y0, f"{name} M={M} 16 vs 0")
    assert counter.n > 0


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_quantized_experts_forward_is_the_same_with_and_without_the_gemv(ops, dev, synthetic_checkpoints, monkeypatch,
                                                                         scheme):
    from quantool_amd.engine.qlinear import QuantizedExperts, load_quantized

    model = load_quantized(synthetic_checkpoints("mixtral", scheme), device=dev)
    banks = [m for m in model.modules() if isinstance(m, QuantizedExperts)]
    assert len(banks) == 2
    default = QuantizedExperts.grouped_max_tokens
    counter = _Counter(monkeypatch, ops, "gemm_i8_skinny_grouped")
    ran = 0
    for T in (1, 7, 16, 17):
        g = torch.Generator().manual_seed(T)
        for qe in banks:
            E, k = qe.num_experts, 2
            x = (torch.randn(T, qe.hidden_dim, generator=g) * 2).to(torch.bfloat16).to(dev)
            idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(dev)
            w = torch.softmax(torch.randn(T, k, generator=g), -1).to(dev)
            outs = {}
            for setting in (default, 0, 16):
                monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", setting)
                before = counter.n
                with torch.no_grad():
                    outs[setting] = qe(x, idx, w)
                assert counter.n - before == (2 if 1 <= T <= setting else 0)
                ran += counter.n - before
            monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", default)
            torch.cuda.synchronize()
            _same_bits(outs[default], outs[0], f"T={T} default vs 0")
            _same_bits(outs[16], outs[0], f"T={T} 16 vs 0")
    assert ran > 0


# ---- 8: end to end --------------------------------------------------------------------------------------------------
def _greedy_logits(model, prompt, steps):
    """Every step's logits of a greedy decode with the KV cache: the prompt's, then one token at a time."""
    logits, tokens = [], []
    with torch.no_grad():
        out = model(input_ids=prompt, use_cache=True)
        for _ in range(steps):
            logits.append(out.logits[:, -1].clone())
            nxt = logits[-1].argmax(-1, keepdim=True)
            tokens.append(nxt)
            out = model(input_ids=nxt, past_key_values=out.past_key_values, use_cache=True)
        logits.append(out.logits[:, -1].clone())
    return logits, torch.cat(tokens, 1)


def bank_present(model):
    from quantool_amd.engine.qlinear import QuantizedExperts

    return any(isinstance(m, QuantizedExperts) for m in model.modules())


def _end_to_end(dev, monkeypatch, ckpt, ops):
    from quantool_amd.engine.qlinear import QuantizedExperts, QuantizedLinear, load_quantized
    from quantool_amd.evaluate import perplexity

    model = load_quantized(ckpt, device=dev)
    defaults = (QuantizedLinear.skinny_max_m, QuantizedExperts.grouped_max_tokens)
    ids = torch.randint(0, 512, (6, 96), generator=torch.Generator().manual_seed(11))
    prompt = ids[:1, :5].to(dev)
    lin = _Counter(monkeypatch, ops, "gemm_i8_skinny")
    bank = _Counter(monkeypatch, ops, "gemm_i8_skinny_grouped")
    ppl = perplexity(model, ids, batch_size=4)["perplexity"]
    logits, tokens = _greedy_logits(model, prompt, 32)
    ran = (lin.n, bank.n)
    monkeypatch.setattr(QuantizedLinear, "skinny_max_m", 0)
    monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", 0)
    ppl0 = perplexity(model, ids, batch_size=4)["perplexity"]
    logits0, tokens0 = _greedy_logits(model, prompt, 32)
    assert (lin.n, bank.n) == ran, "the tiled setting still reached the decode kernels"
    assert ppl == ppl0
    assert torch.equal(tokens, tokens0)
    for step, (a, b) in enumerate(zip(logits, logits0)):
        _same_bits(a, b, f"logits of step {step}")
    # the decode kernels ran exactly where the class defaults enable them
    assert (ran[0] > 0, ran[1] > 0) == (defaults[0] > 0, defaults[1] > 0 and bank_present(model))


@pytest.mark.parametrize("level", ["W8A8", "W4A8"])
def test_tiny_llama_decodes_to_the_same_logits(ops, dev, tmp_path, monkeypatch, level):
    from tests.test_gpu_qlinear import _quantize_and_save

    monkeypatch.chdir(tmp_path)
    _quantize_and_save("smoothquant", level, dev, tmp_path / "ckpt")
    _end_to_end(dev, monkeypatch, tmp_path / "ckpt", ops)


@pytest.mark.parametrize("level", ["W8A8", "W4A8"])
def test_tiny_mixtral_decodes_to_the_same_logits(ops, dev, tmp_path, monkeypatch, level):
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry
    from tests.test_gpu_moe import _tiny_mixtral

    monkeypatch.chdir(tmp_path)
    model = _tiny_mixtral(dev)
    g = torch.Generator().manual_seed(2)
    data = [{"input_ids": torch.randint(0, 512, (48,), generator=g)} for _ in range(8)]
    q = QuantizerRegistry.create("smoothquant", model_id="synthetic/tiny-mixtral")
    q.quantize(model=model, level=level, dataset=data, num_calibration_samples=8, max_seq_length=64,
               shuffle_calibration_samples=False)
    torch.cuda.synchronize()
    q.save_pretrained(str(tmp_path / "ckpt"))
    del q, model
    _end_to_end(dev, monkeypatch, tmp_path / "ckpt", ops)
