"""qt_gemm_i8_ring: the 256 x 256 LDS-ring int8 GEMM for W8A8 / INT8 prefill.

Its contract is bit equality with the tiled qt_gemm_i8 on the same arguments, so every comparison here is on bit
patterns (``.view(torch.int16)`` + ``torch.equal``).  That alone would pass two kernels wrong in the same way, so the
same cases also go against the fp64 reference of tests/ckpt_reference.py within the project's own bound for this
sequence (``gemm_i8_tolerance``), and an identity test pins which weight byte every A slot multiplies.  Shapes are in
the kernel's own constants: U = the k-unit, R = the ring's slots, L = its lead."""
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_i8_skinny import _bias, _same_bits, _sentinel, _untouched
from tests.test_gpu_runtime_edges import _leaves, _levels, _qweight, cr_wsum

pytestmark = pytest.mark.gpu


def _url():
    from quantool_amd.hip import ops

    return ops.I8_RING_K_UNIT, ops.I8_RING_SLOTS, ops.I8_RING_LEAD


def _acts(M, K, dev, seed):
    """M activation rows with outlier channels, an all-zero row (the eps clamp) and an all-positive one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[:, torch.randperm(K, generator=g)[: max(1, K // 64)]] *= 10
    x[M // 2] = 0.0
    x[M // 3] = x[M // 3].abs() + 0.5
    return x.to(torch.bfloat16).to(dev)


def _case(ops, dev, M, N, K, seed):
    """One weight and both quantisations of one activation matrix, with their fp64 references (computed once)."""
    q8 = _levels((N, K), 8, seed=seed)
    t = _leaves(q8, 8, 1, seed=seed + 1)
    X = _acts(M, K, dev, seed=seed + 2)
    out = {"Wq": _qweight(t, dev), "s_w": t["weight_scale"].to(dev), "wsum": cr_wsum(q8, 1).to(dev)}
    for asym in (False, True):
        Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
        out[asym] = (Xq, s_x, zp_x, *cr.a8_linear(Xq, s_x, zp_x, t))
    return out


def _check(ops, c, asym, dt, bias, what):
    Xq, s_x, zp_x, y64, mag = c[asym]
    kw = dict(zp_x=zp_x, wsum=c["wsum"] if asym else None, bias=bias, out_dtype=dt)
    want = ops.gemm_i8(Xq, s_x, c["Wq"], c["s_w"], **kw)
    got = ops.gemm_i8_ring(Xq, s_x, c["Wq"], c["s_w"], **kw)
    torch.cuda.synchronize()
    _same_bits(got, want, what)
    if bias is not None:
        b = bias.cpu().double()
        y64, mag = y64 + b, mag + b.abs()
    cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, 1), f"{what} vs fp64")


# ---- 1: the ring's depth ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("units", ["1", "L-1", "L", "L+1", "R", "R+1", "2R+3"])
def test_ring_depth(ops, dev, units):
    """2 x 2 tiles, both edges ragged, over a reduction shorter than the lead, exactly the lead, one past it, exactly one
    trip round the ring, the first wrap, and two trips with a partial third."""
    U, R, L = _url()
    K = U * {"1": 1, "L-1": L - 1, "L": L, "L+1": L + 1, "R": R, "R+1": R + 1, "2R+3": 2 * R + 3}[units]
    M, N = 300, 384
    c = _case(ops, dev, M, N, K, seed=K)
    for asym in (False, True):
        for dt in (torch.bfloat16, torch.float16):
            for with_bias in (False, True):
                bias = _bias(N, dt, dev, seed=N) if with_bias else None
                _check(ops, c, asym, dt, bias, f"K={K} asym={asym} {dt} bias={with_bias}")


# ---- 2: tile edges and tile order -----------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(256, 256), (255, 256), (257, 200), (1, 257), (513, 1), (1100, 1600)])
def test_tile_edges_and_order(ops, dev, M, N):
    """Full, one short and one over in either direction, one row, one column, and 5 x 7 = 35 tiles (more than 8 and no
    multiple of 8: any remap of workgroups onto tiles has to be a bijection there)."""
    U, R, L = _url()
    K = (R + 1) * U
    c = _case(ops, dev, M, N, K, seed=M + N)
    _check(ops, c, True, torch.bfloat16, _bias(N, torch.bfloat16, dev, seed=M), f"M={M} N={N}")


# ---- 3: lane and slot maps ------------------------------------------------------------------------------------------
def test_identity_activations_read_the_weight(ops, dev):
    """Xq = the K x K identity, unit scales, no zero-point: Y[m, n] = (float)W[n, m] exactly, which pins the weight byte
    every A slot multiplies, across k-halves, units and ring slots."""
    U, R, L = _url()
    K, N = (R + 1) * U, 96
    W = _levels((N, K), 8, seed=77)
    assert len({tuple(r) for r in W.tolist()}) == N and not torch.equal(W[:, :N], W[:, :N].T)
    assert not torch.equal(W, W.flip(1))
    Xq = torch.eye(K, dtype=torch.int8, device=dev)
    Y = ops.gemm_i8_ring(Xq, torch.ones(K, device=dev), W.to(dev), torch.ones(N, 1, device=dev),
                         out_dtype=torch.float16)
    torch.cuda.synchronize()
    _same_bits(Y.cpu(), W.T.to(torch.float16).contiguous(), "identity")


# ---- 4 + 5: raw C ABI calls -----------------------------------------------------------------------------------------
def _raw_ring(ops, Xq_ptr, M, K, Wq_ptr, fmt, N, s_x, zp_x, s_w, G, wsum, bias, Y, ldy, name="qt_gemm_i8_ring"):
    from quantool_amd.hip import _lib

    _lib.check(name, getattr(_lib.load(), name)(
        Xq_ptr, M, K, Wq_ptr, fmt, N, s_x.data_ptr(), ops._ptr(zp_x), s_w.data_ptr(), G, ops._ptr(wsum),
        ops._ptr(bias), Y.data_ptr(), ops._dtype_code(Y), ldy, ops._stream()))


def test_caller_owned_y_keeps_its_padding(ops, dev):
    from quantool_amd.hip import _lib

    U, R, L = _url()
    M, N, K = 257, 200, (R + 1) * U
    ldy = N + 17
    c = _case(ops, dev, M, N, K, seed=4)
    Xq, s_x, zp_x, _, _ = c[True]
    bias = _bias(N, torch.bfloat16, dev, seed=5)
    Ys = {}
    for name in ("qt_gemm_i8", "qt_gemm_i8_ring"):
        Ys[name] = _sentinel((M + 3, ldy), torch.bfloat16, dev)
        _raw_ring(ops, Xq.data_ptr(), M, K, c["Wq"].data_ptr(), _lib.QT_W_INT8, N, s_x, zp_x, c["s_w"], 1, c["wsum"],
                  bias, Ys[name], ldy, name=name)
    torch.cuda.synchronize()
    Y = Ys["qt_gemm_i8_ring"]
    assert _untouched(Y[:, N:]) and _untouched(Y[M:]) and not _untouched(Y[:M, :N])
    _same_bits(Y[:M, :N].contiguous(), Ys["qt_gemm_i8"][:M, :N].contiguous(), "ldy > N")


def test_refusals_write_nothing_and_name_the_reason(ops, dev):
    from quantool_amd.hip import _lib
    from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

    U, R, L = _url()
    M, N, K = 20, 32, 4 * 128
    assert K % U == 0
    # every pointer below lies inside one of these buffers with room for the whole operand behind it
    xbuf = torch.ones(M * (K + 16) + 32, dtype=torch.int8, device=dev)
    wbuf = torch.zeros(N * (K + 16) + 32, dtype=torch.int8, device=dev)
    assert xbuf.data_ptr() % 16 == 0 and wbuf.data_ptr() % 16 == 0
    s_x = torch.ones(M, device=dev)
    s_w = torch.ones(N, K // 128, device=dev)
    Y = _sentinel((M, N), torch.bfloat16, dev)
    X, W = xbuf.data_ptr(), wbuf.data_ptr()
    cases = {
        "int4 format": ((X, M, K, W, _lib.QT_W_INT4_PACKED, N, s_x, None, s_w, 1), "int8 weights only"),
        "G > 1": ((X, M, K, W, _lib.QT_W_INT8, N, s_x, None, s_w, K // 128), "one scale group"),
        "K % U != 0": ((X, M, K + 16, W, _lib.QT_W_INT8, N, s_x, None, s_w, 1), "not a multiple of the k-unit"),
        "Xq misaligned": ((X + 1, M, K, W, _lib.QT_W_INT8, N, s_x, None, s_w, 1), "Xq is not 16-byte aligned"),
        "Wq misaligned": ((X, M, K, W + 1, _lib.QT_W_INT8, N, s_x, None, s_w, 1), "Wq is not 16-byte aligned"),
    }
    for what, (args, reason) in cases.items():
        with pytest.raises(HipBackendError) as e:
            _raw_ring(ops, *args, None, None, Y, N)
        assert e.value.status == QT_ERR_INVALID, what
        assert reason in str(e.value), (what, str(e.value))
    torch.cuda.synchronize()
    assert _untouched(Y)


# ---- 6: the module, end to end --------------------------------------------------------------------------------------
class _Counter:
    def __init__(self, monkeypatch, ops, name):
        self.n = 0
        real = getattr(ops, name)

        def counted(*a, **kw):
            self.n += 1
            return real(*a, **kw)

        monkeypatch.setattr(ops, name, counted)


@pytest.mark.parametrize("level", ["W8A8", "W4A8"])
def test_module_is_the_same_with_and_without_the_ring(ops, dev, tmp_path, monkeypatch, level):
    from quantool_amd.engine.qlinear import QuantizedLinear, load_quantized
    from quantool_amd.evaluate import perplexity
    from tests.test_gpu_qlinear import _eval_ids, _quantize_and_save

    monkeypatch.chdir(tmp_path)
    _quantize_and_save("smoothquant", level, dev, tmp_path / "ckpt")
    model = load_quantized(tmp_path / "ckpt", device=dev)
    assert sum(isinstance(m, QuantizedLinear) for m in model.modules()) == 14
    ids = _eval_ids()
    monkeypatch.setattr(QuantizedLinear, "skinny_max_m", 0)
    counter = _Counter(monkeypatch, ops, "gemm_i8_ring")
    logits, ppl, calls = {}, {}, {}
    for ring_min_m in (0, 1):
        monkeypatch.setattr(QuantizedLinear, "ring_min_m", ring_min_m)
        before = counter.n
        with torch.no_grad():
            logits[ring_min_m] = model(input_ids=ids[:2].to(dev)).logits
        ppl[ring_min_m] = perplexity(model, ids, batch_size=4)["perplexity"]
        torch.cuda.synchronize()
        calls[ring_min_m] = counter.n - before
    assert calls[0] == 0
    if level == "W8A8":
        assert calls[1] >= 14
    else:                                  # packed int4, G = K/128: never the ring
        assert calls[1] == 0
    assert torch.isfinite(logits[1].float()).all()
    _same_bits(logits[1], logits[0], f"{level} logits, ring_min_m 1 vs 0")
    assert ppl[1] == ppl[0]
