"""The A8 runtime on the GPU: ``qt_quantize_tokens_i8`` and ``qt_gemm_i8`` bit for bit against torch restatements of
the header's arithmetic (fp32 steps on the CPU, integer products in fp64 -- exact below 2^53), and
``load_quantized`` end to end on a tiny random-init Llama quantised through the plugins."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = torch.finfo(torch.float32).eps


# ---- torch restatements (test helpers, not part of the package) -----------------------------------------------------
def ref_quantize_tokens(X, symmetric, col_perm=None):
    x = X.detach().cpu().float()
    mn = torch.clamp(x.amin(1), max=0.0)
    mx = torch.clamp(x.amax(1), min=0.0)
    if symmetric:
        s = torch.maximum(-mn, mx) / 127.5
        s = torch.clamp(s, min=EPS)
        zp = torch.zeros_like(s)
    else:
        s = (mx - mn) / 255.0
        s = torch.clamp(s, min=EPS)
        zp = torch.clamp(torch.round(-128.0 - mn / s), -128.0, 127.0)
    if col_perm is not None:
        x = x[:, col_perm.cpu().long()]
    q = torch.round(torch.clamp(x / s[:, None] + zp[:, None], -128.0, 127.0)).to(torch.int8)
    return q, s, (None if symmetric else zp.to(torch.int32))


def ref_acc(Xq, Wq8, G):
    """acc_g [G, M, N] int64 from exact fp64 products."""
    X = Xq.cpu().double()
    W = Wq8.cpu().double()
    K = X.shape[1]
    step = K if G == 1 else 128
    return torch.stack([(X[:, g * step:(g + 1) * step] @ W[:, g * step:(g + 1) * step].T).round().long()
                        for g in range(G)])


def ref_gemm(Xq, s_x, Wq8, s_w, zp_x=None, wsum=None, bias=None, out_dtype=torch.bfloat16):
    G = s_w.shape[1]
    acc = ref_acc(Xq, Wq8, G)
    s_w = s_w.cpu()
    tot = torch.zeros(acc.shape[1:], dtype=torch.float32)
    for g in range(G):
        a = acc[g]
        if zp_x is not None:
            a = a - zp_x.cpu().long()[:, None] * wsum.cpu().long()[None, :, g]
        t = a.to(torch.float32)
        prod = s_w[None, :, g] * t
        tot = tot + prod
    y = s_x.cpu()[:, None] * tot
    if bias is not None:
        y = y + bias.cpu().float()[None, :]
    return y.to(out_dtype)


def _wsum(q8, G):
    from quantool_amd.engine.qlinear import group_sums

    return group_sums(q8, G)


def _bits_equal(a, b):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.is_floating_point():
        a, b = a.view(torch.int16), b.view(torch.int16)
    bad = (a != b).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {a.numel()} differ, first at {bad[0].tolist()}"


# ---- qt_quantize_tokens_i8 ------------------------------------------------------------------------------------------
def _acts(M, K, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[:, torch.randperm(K, generator=g)[: max(1, K // 64)]] *= 10     # outlier channels
    if M > 1:
        x[M // 2] = 0.0                                                # the eps clamp
    if M > 2:
        x[1] = x[1].abs() + 0.5                                        # all positive: min clamps to 0
    return x.to(dtype).to(dev)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("M", [1, 7, 4096])
@pytest.mark.parametrize("K", [128, 4096, 14336, 999])
def test_quantize_tokens_bit_exact(ops, dev, dtype, symmetric, M, K):
    X = _acts(M, K, dtype, dev, seed=M * 31 + K)
    Xq, s, zp = ops.quantize_tokens_i8(X, symmetric=symmetric)
    torch.cuda.synchronize()
    rq, rs, rzp = ref_quantize_tokens(X, symmetric)
    _bits_equal(s.view(torch.int32), rs.view(torch.int32))
    if not symmetric:
        _bits_equal(zp, rzp)
    else:
        assert zp is None
    _bits_equal(Xq, rq)


@pytest.mark.parametrize("symmetric", [True, False])
def test_quantize_tokens_col_perm_and_row_pitch(ops, dev, symmetric):
    M, K = 33, 640
    wide = _acts(M, K + 24, torch.bfloat16, dev, seed=5)
    X = wide[:, 8:8 + K]                    # row pitch K + 24, unaligned start
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(6)).to(torch.int32).to(dev)
    Xq, s, zp = ops.quantize_tokens_i8(X, symmetric=symmetric, col_perm=perm)
    torch.cuda.synchronize()
    rq, rs, rzp = ref_quantize_tokens(X, symmetric, perm)
    _bits_equal(s.view(torch.int32), rs.view(torch.int32))
    _bits_equal(Xq, rq)
    if not symmetric:
        _bits_equal(zp, rzp)


def test_quantize_tokens_refuses_bad_input(ops, dev):
    with pytest.raises(TypeError):
        ops.quantize_tokens_i8(torch.zeros(4, 8, device=dev))
    with pytest.raises(ValueError):
        ops.quantize_tokens_i8(torch.zeros(8, 4, device=dev, dtype=torch.bfloat16).t())
    with pytest.raises(ValueError):
        ops.quantize_tokens_i8(torch.zeros(4, 8, device=dev, dtype=torch.bfloat16),
                               col_perm=torch.zeros(7, dtype=torch.int32, device=dev))


# ---- qt_gemm_i8 -----------------------------------------------------------------------------------------------------
def _levels(shape, bits, seed):
    g = torch.Generator().manual_seed(seed)
    lo, hi = (-8, 8) if bits == 4 else (-128, 128)
    return torch.randint(lo, hi, shape, generator=g, dtype=torch.int8)


def _weights(q8, bits, dev):
    from quantool_amd.engine.qlinear import pack_int4

    return (pack_int4(q8) if bits == 4 else q8).to(dev)


GEMM_SHAPES = [(1, 256, 4096), (33, 200, 1000), (33, 130, 136), (4096, 256, 4096), (4096, 77, 14336),
               (33, 1000, 256), (1, 96, 14336)]


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_integer_core_is_exact(ops, dev, bits, M, N, K):
    Xq = _levels((M, K), 8, seed=M + K).to(dev)
    q8 = _levels((N, K), bits, seed=N + 7 * K)
    Wq = _weights(q8, bits, dev)
    ones_x = torch.ones(M, dtype=torch.float32, device=dev)
    ones_w = torch.ones(N, 1, dtype=torch.float32, device=dev)
    Y = ops.gemm_i8(Xq, ones_x, Wq, ones_w, K=K)
    torch.cuda.synchronize()
    exact = Xq.cpu().double() @ q8.double().T
    _bits_equal(Y, exact.float().to(torch.bfloat16))


@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("N,K", [(96, 128), (160, 320), (64, 1000)])
def test_gemm_identity_rows_read_the_weight(ops, dev, bits, N, K):
    """A = identity rows, W asymmetric: Y[m, n] = W[n, m] -- catches a swapped lane map or C write."""
    M = min(K, 160)
    Xq = torch.zeros(M, K, dtype=torch.int8)
    Xq[torch.arange(M), torch.arange(M)] = 1
    q8 = (torch.arange(N)[:, None] * 3 + torch.arange(K)[None, :] * 7) % (16 if bits == 4 else 256)
    q8 = (q8 - (8 if bits == 4 else 128)).to(torch.int8)
    Wq = _weights(q8, bits, dev)
    Y = ops.gemm_i8(Xq.to(dev), torch.ones(M, device=dev), Wq, torch.ones(N, 1, device=dev), K=K,
                    out_dtype=torch.float16)
    torch.cuda.synchronize()
    _bits_equal(Y, q8[:, :M].T.to(torch.float16))


@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits,grouped", [(8, False), (4, True), (4, False), (8, True)])
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("M,N,K", [(33, 200, 1024), (300, 384, 4096), (4096, 128, 640)])
def test_gemm_full_epilogue_bit_exact(ops, dev, out_dtype, bits, grouped, asym, M, N, K):
    X = _acts(M, K, out_dtype, dev, seed=K + M)
    Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
    q8 = _levels((N, K), bits, seed=3 * N + K)
    Wq = _weights(q8, bits, dev)
    G = K // 128 if grouped else 1
    g = torch.Generator().manual_seed(9)
    s_w = (torch.rand(N, G, generator=g) * 0.02 + 1e-4).to(torch.bfloat16).float().to(dev)
    wsum = _wsum(q8, G).to(dev)
    bias = (torch.randn(N, generator=g) * 0.1).to(out_dtype).to(dev) if M != 33 else None
    Y = ops.gemm_i8(Xq, s_x, Wq, s_w, K=K, zp_x=zp_x, wsum=wsum, bias=bias, out_dtype=out_dtype)
    torch.cuda.synchronize()
    ref = ref_gemm(Xq, s_x, q8, s_w, zp_x, wsum, bias, out_dtype)
    _bits_equal(Y, ref)


def test_gemm_refuses_bad_shapes(ops, dev):
    Xq = torch.zeros(4, 256, dtype=torch.int8, device=dev)
    s_x = torch.ones(4, device=dev)
    W = torch.zeros(8, 256, dtype=torch.int8, device=dev)
    with pytest.raises(ValueError):
        ops.gemm_i8(Xq, s_x, W, torch.ones(8, 3, device=dev))          # neither 1 nor K/128 groups
    with pytest.raises(ValueError):
        ops.gemm_i8(Xq, s_x, W[:, :128], torch.ones(8, 1, device=dev))
    with pytest.raises(ValueError):
        ops.gemm_i8(Xq, s_x, W, torch.ones(8, 1, device=dev), zp_x=torch.zeros(4, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        ops.gemm_i8(Xq, s_x, W.float(), torch.ones(8, 1, device=dev))


# ---- end to end -----------------------------------------------------------------------------------------------------
def _tiny_llama(dev):
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=128, tie_word_embeddings=False)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev)


def _quantize_and_save(method, level, dev, out_dir, **kw):
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry

    model = _tiny_llama(dev)
    g = torch.Generator().manual_seed(2)
    data = [{"input_ids": torch.randint(0, 512, (48,), generator=g)} for _ in range(8)]
    q = QuantizerRegistry.create(method, model_id="synthetic/tiny-llama")
    q.quantize(model=model, level=level, dataset=data, num_calibration_samples=8, max_seq_length=64,
               shuffle_calibration_samples=False, **kw)
    torch.cuda.synchronize()
    q.save_pretrained(str(out_dir))
    return q.last_model


def _eval_ids():
    return torch.randint(0, 512, (6, 96), generator=torch.Generator().manual_seed(11))


@pytest.mark.parametrize("method,level", [("smoothquant", "W8A8"), ("smoothquant", "W4A8"), ("gptq", "W4A16")])
def test_end_to_end_on_tiny_llama(dev, tmp_path, monkeypatch, method, level):
    from quantool_amd.engine.qlinear import QuantizedLinear, load_quantized, unpack_int4
    from quantool_amd.evaluate import perplexity

    monkeypatch.chdir(tmp_path)
    mem = _quantize_and_save(method, level, dev, tmp_path / "ckpt")
    ids = _eval_ids()
    ppl_mem = perplexity(mem, ids, batch_size=4)["perplexity"]
    del mem
    model = load_quantized(tmp_path / "ckpt", device=dev)
    qls = {n: m for n, m in model.named_modules() if isinstance(m, QuantizedLinear)}
    assert (len(qls) == 14) == (level != "W4A16")
    seen = {}

    def hook(name):
        def f(mod, inp, out):
            seen[name] = (inp[0].detach().clone(), out.detach().clone())
        return f

    handles = [m.register_forward_hook(hook(n)) for n, m in qls.items()]
    with torch.no_grad():
        logits = model(input_ids=ids[:2].to(dev)).logits
    for h in handles:
        h.remove()
    assert torch.isfinite(logits.float()).all()
    assert len(seen) == len(qls)
    for name, (x, y) in seen.items():
        m = qls[name]
        x2 = x.reshape(-1, m.in_features)
        rq, rs, rzp = ref_quantize_tokens(x2, m.act_symmetric, m.col_perm)
        q8 = unpack_int4(m.weight, m.in_features) if m.int4 else m.weight
        ref = ref_gemm(rq, rs, q8, m.weight_scale, rzp, m.wsum if rzp is not None else None, m.bias, x.dtype)
        _bits_equal(y.reshape(-1, m.out_features), ref)
    ppl = perplexity(model, ids, batch_size=4)["perplexity"]
    assert math.isfinite(ppl)
    if level == "W4A16":
        # the in-memory model differs only in the scale rounding (fp32 there, the stored bf16 scale here)
        assert abs(ppl - ppl_mem) / ppl_mem < 1e-2, (ppl, ppl_mem)
    else:
        # activations really are quantised: the weight-only in-memory model gives another number
        assert ppl != ppl_mem, ppl
    # a path goes through load_quantized
    assert perplexity(str(tmp_path / "ckpt"), ids, batch_size=4, device=dev)["perplexity"] == pytest.approx(ppl,
                                                                                                            rel=1e-9)
    # every quantized module against what the checkpoint files define (an fp64 reference that shares no decoding)
    from tests.test_gpu_ckpt_e2e import check_modules_against_files

    assert check_modules_against_files(model, tmp_path / "ckpt", dev, tokens=(1, 17)) == 2 * 14
