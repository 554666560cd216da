"""qt_gemm_i8_mid: the A8 GEMM for 1 .. 128 rows (batched decode, speculative verification, short prompts).

Its contract is bit equality with the tiled qt_gemm_i8 on the same arguments, so every comparison here is on bit patterns.
That alone would pass two kernels wrong in the same way, so the same cases also go against the fp64 reference of
tests/ckpt_reference.py within the project's own bound for this sequence (``gemm_i8_tolerance``), and a one-hot test
pins which weight element every lane slot of every m-tile multiplies.

The shapes come from the kernel's own constants (csrc/qlinear_mid.hip), restated here:"""
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_i8_skinny import _bias, _same_bits, _sentinel, _untouched
from tests.test_gpu_runtime_edges import _leaves, _levels, _qweight, cr_wsum

pytestmark = pytest.mark.gpu

COLS = 16                       # MID_COLS: output columns per workgroup (one width)
WAVES = 4                       # MID_WAVES: k-block kb goes to wave kb % 4
KB = 128                        # MID_KB: columns per k-block
BATCH = {2: 16, 4: 16, 8: 8}    # MID_WAVES * mid_unroll(MT): k-blocks per batch of the MT = 2 / 4 / 8 instances
# M: 1, 15 .. 17 (the skinny edge), every m-tile count's edge +- 1 (MT = 2 up to 32, 4 up to 64, 8 up to 128)
MS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128]
# N: 1, the column tile +- 1, two tiles + 1 (the kernel has one tile width, so no N switches to another)
NS = [1, COLS - 1, COLS, COLS + 1, 2 * COLS + 1]
# K in k-blocks, by the pipeline's depth: 1, waves - 1, waves, waves + 1, one batch, one batch + 1, two batches + 3 --
# for both batch lengths
KBLOCKS = sorted({1, WAVES - 1, WAVES, WAVES + 1, *BATCH.values(), *(b + 1 for b in BATCH.values()),
                  *(2 * b + 3 for b in BATCH.values())})
assert KBLOCKS == [1, 3, 4, 5, 8, 9, 16, 17, 19, 35]


@pytest.fixture(scope="module", autouse=True)
def _release_cached_blocks():
    """The later memory tests of the suite measure ``max_memory_allocated`` deltas, which count a reused cached block at
    its full size: hand this module's blocks back so that it leaves no cache behind."""
    yield
    import gc

    gc.collect()
    torch.cuda.empty_cache()


def _acts(M, K, dev, seed):
    """M activation rows with outlier channels, an all-zero row (the eps clamp) and an all-positive one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[:, torch.randperm(K, generator=g)[: max(1, K // 64)]] *= 10
    if M > 9:
        x[9] = 0.0
    x[M // 3] = x[M // 3].abs() + 0.5
    return x.to(torch.bfloat16).to(dev)


def _case(ops, dev, N, K, bits, grouped, seed):
    q8 = _levels((N, K), bits, seed=seed)
    G = K // KB if grouped else 1
    t = _leaves(q8, bits, G, seed=seed + 1)
    return q8, G, t, _qweight(t, dev), t["weight_scale"].to(dev), cr_wsum(q8, G).to(dev)


def _check(ops, Xq, s_x, zp_x, Wq, s_w, wsum, t, G, K, M, dt, bias, what, fp64=True):
    kw = dict(K=K, zp_x=None if zp_x is None else zp_x[:M], wsum=None if zp_x is None else wsum, bias=bias,
              out_dtype=dt)
    want = ops.gemm_i8(Xq[:M], s_x[:M], Wq, s_w, **kw)
    got = ops.gemm_i8_mid(Xq[:M], s_x[:M], Wq, s_w, **kw)
    torch.cuda.synchronize()
    _same_bits(got, want, what)
    if fp64:
        y64, mag = cr.a8_linear(Xq[:M], s_x[:M], kw["zp_x"], t, bias)
        cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, G), f"{what} vs fp64")


# ---- every M and K depth, every form, against the tiled kernel's bits and against fp64 -------------------------------
@pytest.mark.parametrize("kblocks", KBLOCKS)
@pytest.mark.parametrize("bits,grouped", [(8, False), (8, True), (4, False), (4, True)])
def test_mid_equals_tiled_bits_and_fp64_over_m_and_k(ops, dev, bits, grouped, kblocks):
    N, K = 2 * COLS + 8, kblocks * KB
    q8, G, t, Wq, s_w, wsum = _case(ops, dev, N, K, bits, grouped, seed=K + bits)
    X = _acts(128, K, dev, seed=K)
    quant = {asym: ops.quantize_tokens_i8(X, symmetric=not asym) for asym in (False, True)}
    for i, M in enumerate(MS):
        for asym in (False, True):
            Xq, s_x, zp_x = quant[asym]
            # bias and the output dtype alternate over the cases: every (M, asym) meets both of each over the K sweep
            dt = (torch.bfloat16, torch.float16)[(i + asym + kblocks) % 2]
            bias = _bias(N, dt, dev, seed=N) if (i // 2 + asym + kblocks) % 2 else None
            _check(ops, Xq, s_x, zp_x, Wq, s_w, wsum, t, G, K, M, dt, bias,
                   f"bits={bits} G={G} K={K} M={M} asym={asym} {dt} bias={bias is not None}")


@pytest.mark.parametrize("N", NS + [4 * COLS + 3])
@pytest.mark.parametrize("bits,grouped", [(8, False), (8, True), (4, False), (4, True)])
def test_mid_equals_tiled_bits_and_fp64_over_n(ops, dev, bits, grouped, N):
    K = (WAVES + 1) * KB
    q8, G, t, Wq, s_w, wsum = _case(ops, dev, N, K, bits, grouped, seed=N + bits)
    X = _acts(128, K, dev, seed=N)
    for asym in (False, True):
        Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
        for M in (1, 17, 33, 65, 128):
            for dt in (torch.bfloat16, torch.float16):
                for with_bias in (False, True):
                    bias = _bias(N, dt, dev, seed=N) if with_bias else None
                    _check(ops, Xq, s_x, zp_x, Wq, s_w, wsum, t, G, K, M, dt, bias,
                           f"bits={bits} G={G} N={N} M={M} asym={asym} {dt} bias={with_bias}")


# ---- the lane / row map ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("rows", [32, 64, 128])
def test_mid_one_hot_rows_read_the_weight(ops, dev, bits, grouped, rows):
    """Xq row m = e_{k_m} (value 1, s_x = 1) against a random W with power-of-two scales: Y[m, n] = s_w[n, g(k_m)]
    q[n, k_m] exactly.  k_m runs over every column, so over every 16-byte slot of every lane of every wave, and m over
    every row of every m-tile of the MT = 2 / 4 / 8 instance (``rows`` at a time)."""
    N, K = 2 * COLS + 8, (WAVES + 1) * KB
    G = K // KB if grouped else 1
    q8 = _levels((N, K), bits, seed=K + bits)
    assert not torch.equal(q8[:, :N], q8[:, :N].T)
    t = _leaves(q8, bits, G, seed=K, pow2=True)
    Wq, s_w = _qweight(t, dev), t["weight_scale"].to(dev)
    w = q8.float() * (t["weight_scale"][:, torch.arange(K) // KB] if grouped else t["weight_scale"])   # exact
    ones = torch.ones(rows, device=dev)
    for k0 in range(0, K, rows):
        ks = torch.arange(k0, k0 + rows)
        Xq = torch.zeros(rows, K, dtype=torch.int8)
        Xq[torch.arange(rows), ks] = 1
        Y = ops.gemm_i8_mid(Xq.to(dev), ones, Wq, s_w, K=K, out_dtype=torch.float16)
        torch.cuda.synchronize()
        _same_bits(Y.cpu(), (w[:, ks].T + 0.0).to(torch.float16).contiguous(), f"columns {k0}..")


# ---- raw C ABI calls: a caller-owned Y, exact-size operands, refusals ------------------------------------------------
def _raw_mid(ops, Xq, M, K, Wq, N, s_x, zp_x, s_w, G, wsum, bias, Y, ldy):
    from quantool_amd.hip import _lib

    fmt = _lib.QT_W_INT8 if Wq.dtype == torch.int8 else _lib.QT_W_INT4_PACKED
    _lib.check("qt_gemm_i8_mid", _lib.load().qt_gemm_i8_mid(
        Xq.data_ptr(), M, K, Wq.data_ptr(), fmt, N, s_x.data_ptr(), ops._ptr(zp_x), s_w.data_ptr(), G, ops._ptr(wsum),
        ops._ptr(bias), Y.data_ptr(), ops._dtype_code(Y), ldy, ops._stream()))


@pytest.mark.parametrize("bits,grouped", [(8, False), (4, True)])
@pytest.mark.parametrize("M", [17, 65, 127])
def test_mid_row_pitch_leaves_the_gap_the_extra_rows_and_the_tail(ops, dev, bits, grouped, M):
    N, K = 2 * COLS + 1, (WAVES + 1) * KB
    ldy = N + 17
    q8, G, t, Wq, s_w, wsum = _case(ops, dev, N, K, bits, grouped, seed=M)
    Xq, s_x, zp_x = ops.quantize_tokens_i8(_acts(M, K, dev, seed=2), symmetric=False)
    rows = 16 * ((M + 15) // 16) + 2                      # past the kernel's last m-tile
    buf = _sentinel((rows * ldy + 4096,), torch.bfloat16, dev)
    Y = buf[:rows * ldy].view(rows, ldy)
    bias = _bias(N, torch.bfloat16, dev, seed=3)
    _raw_mid(ops, Xq, M, K, Wq, N, s_x, zp_x, s_w, G, wsum, bias, Y, ldy)
    torch.cuda.synchronize()
    _same_bits(Y[:M, :N].contiguous(), ops.gemm_i8(Xq, s_x, Wq, s_w, K=K, zp_x=zp_x, wsum=wsum, bias=bias), "ldy > N")
    assert _untouched(Y[:M, N:]) and _untouched(Y[M:]) and _untouched(buf[rows * ldy:])


@pytest.mark.parametrize("bits,grouped", [(8, True), (4, False)])
def test_mid_operands_that_end_with_their_allocations(ops, dev, bits, grouped):
    """Xq, Wq, s_w, wsum, s_x and zp_x as exact-size views that end where their allocations end, M and N off the tile."""
    M, N, K = 33, COLS + 1, (WAVES + 1) * KB
    q8, G, t, W0, s_w0, wsum0 = _case(ops, dev, N, K, bits, grouped, seed=21)
    X0, s_x0, zp0 = ops.quantize_tokens_i8(_acts(M, K, dev, seed=5), symmetric=False)

    def at_end(src, lead=64):
        buf = torch.zeros(lead + src.numel(), dtype=src.dtype, device=dev)
        v = buf[lead:].view(src.shape)
        v.copy_(src)
        assert v.data_ptr() + v.numel() * v.element_size() == buf.data_ptr() + buf.numel() * buf.element_size()
        return v

    Xq, Wq, s_w, wsum, s_x, zp_x = (at_end(v) for v in (X0, W0, s_w0, wsum0, s_x0, zp0))
    assert Xq.data_ptr() % 16 == 0 and Wq.data_ptr() % 16 == 0
    kw = dict(K=K, zp_x=zp_x, wsum=wsum, out_dtype=torch.bfloat16)
    got = ops.gemm_i8_mid(Xq, s_x, Wq, s_w, **kw)
    torch.cuda.synchronize()
    _same_bits(got, ops.gemm_i8(X0, s_x0, W0, s_w0, K=K, zp_x=zp0, wsum=wsum0), "exact-size views")
    y64, mag = cr.a8_linear(X0, s_x0, zp0, t)
    cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, G), "exact-size views vs fp64")


def test_mid_refusals_write_nothing(ops, dev):
    from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

    N, K = 32, 512
    wbuf = torch.zeros(N * K + 16, dtype=torch.int8, device=dev)
    xbuf = torch.ones(129 * K + 16, dtype=torch.int8, device=dev)
    Wq, W1 = wbuf[:N * K].view(N, K), wbuf[1:1 + N * K].view(N, K)
    Xq, X1 = xbuf[:129 * K].view(129, K), xbuf[1:1 + 129 * K].view(129, K)
    assert Wq.data_ptr() % 16 == 0 and Xq.data_ptr() % 16 == 0 and W1.data_ptr() % 16 == 1 and X1.data_ptr() % 16 == 1
    s_w = torch.ones(N, 4, device=dev)
    s_x = torch.ones(129, device=dev)
    Y = _sentinel((129, N), torch.bfloat16, dev)
    cases = {
        "M = 0": ((Xq, 0, K, Wq, N, s_x, None, s_w, 1, None, None, Y, N), "outside 1"),
        "M = 129": ((Xq, 129, K, Wq, N, s_x, None, s_w, 1, None, None, Y, N), "outside 1"),
        "K = 192": ((Xq, 32, 192, Wq, N, s_x, None, s_w, 1, None, None, Y, N), "not a multiple"),
        "misaligned Xq": ((X1, 32, K, Wq, N, s_x, None, s_w, 1, None, None, Y, N), "16-byte aligned"),
        "misaligned Wq": ((Xq, 32, K, W1, N, s_x, None, s_w, 1, None, None, Y, N), "16-byte aligned"),
        "G = 2 at K = 512": ((Xq, 32, K, Wq, N, s_x, None, s_w, 2, None, None, Y, N), "must be 1 or"),
    }
    for what, (args, reason) in cases.items():
        with pytest.raises(HipBackendError, match=reason) as e:
            _raw_mid(ops, *args)
        assert e.value.status == QT_ERR_INVALID, what
    # null pointers, zp_x without wsum, a row pitch below N: qt_gemm_i8's refusals
    zp = torch.zeros(129, dtype=torch.int32, device=dev)
    for args in ((Xq, 32, K, Wq, N, s_x, zp, s_w, 1, None, None, Y, N),
                 (Xq, 32, K, Wq, N, s_x, None, s_w, 1, None, None, Y, N - 1)):
        with pytest.raises(HipBackendError) as e:
            _raw_mid(ops, *args)
        assert e.value.status == QT_ERR_INVALID
    # and the Python face, before the library
    for bad in (Xq[:0], Xq, X1[:32], Xq[:32, :192].contiguous()):
        assert not ops.gemm_i8_mid_supported(bad, Wq if bad.shape[1] == K else Wq[:, :192].contiguous(), s_w[:, :1])
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.gemm_i8_mid(Xq[:32], s_x[:32], W1, s_w[:, :1].contiguous())
    torch.cuda.synchronize()
    assert _untouched(Y)


# ---- the modules ----------------------------------------------------------------------------------------------------
def _with_mid(monkeypatch, on):
    from quantool_amd.engine.qlinear import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "mid_max_m", 128 if on else 0)
    monkeypatch.setattr(QuantizedLinear, "mid_min_k", 0)
    monkeypatch.setattr(QuantizedLinear, "mid_max_n", 0)


class _Counter:
    def __init__(self, monkeypatch, ops, name):
        self.n = 0
        real = getattr(ops, name)

        def counted(*a, **kw):
            self.n += 1
            return real(*a, **kw)

        monkeypatch.setattr(ops, name, counted)


@pytest.mark.parametrize("int4", [False, True])
def test_quantized_linear_forward_is_the_same_with_and_without_the_mid_kernel(ops, dev, monkeypatch, int4):
    from quantool_amd.engine.qlinear import QuantizedLinear

    N, K = 2 * COLS + 8, 1024
    bits = 4 if int4 else 8
    q8, G, t, Wq, s_w, _ = _case(ops, dev, N, K, bits, int4, seed=1)
    lin = QuantizedLinear(K, N, Wq, s_w, act_symmetric=not int4, bias=_bias(N, torch.bfloat16, dev, 4)).to(dev)
    counter = _Counter(monkeypatch, ops, "gemm_i8_mid")
    for M in (16, 17, 40, 128, 129):
        x = (torch.randn(M, K, generator=torch.Generator().manual_seed(M)) * 2).to(torch.bfloat16).to(dev)
        with torch.no_grad():
            _with_mid(monkeypatch, True)
            before = counter.n
            y1 = lin(x)
            assert counter.n - before == int(17 <= M <= 128)
            _with_mid(monkeypatch, False)
            y0 = lin(x)
            assert counter.n - before == int(17 <= M <= 128)
        torch.cuda.synchronize()
        _same_bits(y1, y0, f"M={M} mid vs tiled")


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_tiny_llama_logits_are_the_same_with_and_without_the_mid_kernel(ops, dev, tmp_path, monkeypatch, scheme):
    """A Llama 256 wide with intermediate 640 (2 and 5 k-blocks), 40 tokens: every Linear runs on the mid kernel."""
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantool_amd.engine.qlinear import QuantizedLinear, load_quantized

    cfg = LlamaConfig(hidden_size=256, intermediate_size=640, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=128, tie_word_embeddings=False)
    torch.manual_seed(0)
    base = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    linears = {n: tuple(m.weight.shape) for n, m in base.named_modules()
               if isinstance(m, torch.nn.Linear) and n.startswith("model.layers.")}
    dense = {k: v for k, v in base.state_dict().items()
             if k.rpartition(".")[0] not in linears or not k.endswith(".weight")}
    bits, act = {"W8A8": (8, "sym"), "W4A8": (4, "asym")}[scheme]
    cr.write_synthetic(tmp_path / "ckpt", base.config.to_dict(), dense, linears, bits=bits, act=act, seed=bits)
    model = load_quantized(tmp_path / "ckpt", device=dev, dtype=torch.bfloat16)
    assert sum(isinstance(m, QuantizedLinear) for m in model.modules()) == 14
    ids = torch.randint(0, 512, (1, 40), generator=torch.Generator().manual_seed(3)).to(dev)
    counter = _Counter(monkeypatch, ops, "gemm_i8_mid")
    with torch.no_grad():
        _with_mid(monkeypatch, True)
        on = model(input_ids=ids).logits
        ran = counter.n
        _with_mid(monkeypatch, False)
        off = model(input_ids=ids).logits
    torch.cuda.synchronize()
    assert ran == 14 and counter.n == ran
    assert torch.isfinite(on.float()).all()
    _same_bits(on, off, f"{scheme} logits")
