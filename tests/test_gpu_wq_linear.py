"""The A16 runtime on the GPU: ``qt_dequantize_weight`` bit for bit against ``dequantized_weight``, the decode GEMV
``qt_gemm_wq_skinny`` against exact and fp64 references, ``WeightOnlyLinear`` on both of its paths, and
``load_quantized(..., a16="packed")`` end to end on a tiny Llama quantised through the plugins and ``oneshot``."""
import math

import pytest
import torch

from tests.test_gpu_qlinear import _eval_ids, _quantize_and_save, _tiny_llama

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.is_floating_point():
        a, b = a.view(torch.int16), b.view(torch.int16)
    bad = (a != b).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {a.numel()} differ, first at {bad[0].tolist()}"


def _weight(N, K, bits, *, zp=False, g_idx=False, grouped=True, seed=0, pow2_scales=False):
    """(checkpoint leaves on the CPU, levels int8 [N, K]) of a random quantized Linear."""
    from quantool_amd.engine.qlinear import pack_int4

    g = torch.Generator().manual_seed(seed)
    lo, hi = (-8, 8) if bits == 4 else (-128, 128)
    q = torch.randint(lo, hi, (N, K), generator=g, dtype=torch.int8)
    G = (K + 127) // 128 if grouped else 1
    if pow2_scales:
        scale = torch.pow(2.0, -torch.randint(0, 5, (N, G), generator=g).float())
    else:
        scale = (torch.rand(N, G, generator=g) * 0.01 + 1e-3).to(torch.bfloat16).float()
    t = {"weight_scale": scale, "weight_shape": torch.tensor([N, K])}
    if bits == 4:
        t["weight_packed"] = pack_int4(q)
    else:
        t["weight"] = q
    if zp:
        t["weight_zero_point"] = torch.randint(-8, 8, (N, G), generator=g, dtype=torch.int8)
    if g_idx:
        t["weight_g_idx"] = (torch.randperm(K, generator=g) % G).to(torch.int32)
    return t, q


def _dev_args(t, dev):
    Wq = (t["weight_packed"] if "weight_packed" in t else t["weight"]).to(dev)
    zp = t["weight_zero_point"].to(dev) if "weight_zero_point" in t else None
    gi = t["weight_g_idx"].to(dev) if "weight_g_idx" in t else None
    return Wq, t["weight_scale"].to(dev), zp, gi


def _ref_w(t, dtype):
    from quantool_amd.engine.qlinear import dequantized_weight

    return dequantized_weight("w", t, dtype)


# ---- qt_dequantize_weight -------------------------------------------------------------------------------------------
DQ_CASES = [(64, 256), (48, 1000), (33, 130), (17, 77), (96, 4096)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("zp,g_idx", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("N,K", DQ_CASES)
def test_dequantize_weight_bit_exact(ops, dev, dtype, bits, zp, g_idx, N, K):
    t, _ = _weight(N, K, bits, zp=zp, g_idx=g_idx, seed=N + K)
    Wq, s, z, gi = _dev_args(t, dev)
    W = ops.dequantize_weight(Wq, s, K=K, zp_w=z, g_idx=gi, dtype=dtype)
    torch.cuda.synchronize()
    _bits_equal(W, _ref_w(t, dtype))


@pytest.mark.parametrize("bits", [4, 8])
def test_dequantize_weight_channelwise_and_pitched_output(ops, dev, bits):
    t, _ = _weight(40, 520, bits, zp=True, grouped=False, seed=7)
    Wq, s, z, gi = _dev_args(t, dev)
    buf = torch.full((40, 600), 7.0, dtype=torch.bfloat16, device=dev)
    ops.dequantize_weight(Wq, s, K=520, zp_w=z, out=buf[:, 40:560])
    torch.cuda.synchronize()
    _bits_equal(buf[:, 40:560], _ref_w(t, torch.bfloat16))
    assert (buf[:, :40] == 7).all() and (buf[:, 560:] == 7).all()


@pytest.mark.parametrize("bits", [4, 8])
def test_dequantize_weight_production_shape(ops, dev, bits):
    t, _ = _weight(28672, 4096, bits, zp=bits == 4, seed=11)
    Wq, s, z, gi = _dev_args(t, dev)
    W = ops.dequantize_weight(Wq, s, K=4096, zp_w=z)
    torch.cuda.synchronize()
    ref = _ref_w({k: v.to(dev) for k, v in t.items()}, torch.bfloat16)
    assert torch.equal(W.view(torch.int16), ref.view(torch.int16))


# ---- qt_gemm_wq_skinny ----------------------------------------------------------------------------------------------
def _ulp(y, dtype):
    mant = 7 if dtype == torch.bfloat16 else 10
    tiny = torch.finfo(dtype).tiny
    a = y.abs().clamp(min=tiny)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - mant)


def _check_bound(Y, X, W, bias=None):
    x, w = X.cpu().double(), W.cpu().double()
    y64 = x @ w.T
    if bias is not None:
        y64 = y64 + bias.cpu().double()
    K = x.shape[1]
    mag = x.abs() @ w.abs().T
    y = Y.cpu().double()
    tol = 0.5 * _ulp(Y.cpu().float(), Y.dtype).double() + K * 2.0 ** -24 * mag
    err = (y - y64).abs()
    assert torch.isfinite(y).all()
    assert (err <= tol).all(), f"max excess {(err - tol).max().item()}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("zp,g_idx", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("N,K,off", [(80, 1024, 0), (80, 1024, 300), (50, 1000, 980), (33, 136, 120)])
def test_skinny_identity_rows_read_the_weight(ops, dev, dtype, bits, zp, g_idx, N, K, off):
    t, _ = _weight(N, K, bits, zp=zp, g_idx=g_idx, seed=N * K + off)
    Wq, s, z, gi = _dev_args(t, dev)
    W = _ref_w(t, dtype)
    for M in (1, 5, 16):
        M = min(M, K - off)
        X = torch.zeros(M, K, dtype=dtype)
        X[torch.arange(M), off + torch.arange(M)] = 1
        Y = ops.gemm_wq_skinny(X.to(dev), Wq, s, zp_w=z, g_idx=gi)
        torch.cuda.synchronize()
        _bits_equal(Y, W[:, off:off + M].T.contiguous())


# |x| <= 4, |q - zp| <= 16 (int4) or 136 (int8), scales 2^0 .. 2^-4: every partial sum is a multiple of 2^-4 below
# 2^20 (int4, K <= 4096) or 2^20 (int8, K <= 1024), so exact in fp32
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("zp", [False, True])
@pytest.mark.parametrize("bits,N,K", [(4, 96, 1024), (4, 40, 520), (4, 300, 4096), (8, 96, 1024), (8, 40, 520)])
def test_skinny_exact_inputs_bit_exact(ops, dev, dtype, bits, zp, N, K):
    t, _ = _weight(N, K, bits, zp=zp, seed=3 * N + K, pow2_scales=True)
    Wq, s, z, gi = _dev_args(t, dev)
    W = _ref_w(t, dtype)
    g = torch.Generator().manual_seed(K)
    bias = torch.randint(-8, 9, (N,), generator=g).to(dtype)
    for M in range(1, 17):
        X = torch.randint(-4, 5, (M, K), generator=g).to(dtype)
        for b in (None, bias):
            Y = ops.gemm_wq_skinny(X.to(dev), Wq, s, zp_w=z, bias=None if b is None else b.to(dev))
            torch.cuda.synchronize()
            ref = X.double() @ W.double().T
            if b is not None:
                ref = ref + b.double()
            _bits_equal(Y, ref.to(dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("zp,g_idx", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("M,N,K", [(1, 256, 4096), (7, 200, 1000), (16, 128, 14336), (3, 6144, 4096)])
def test_skinny_random_inputs_within_bound_and_deterministic(ops, dev, dtype, bits, zp, g_idx, M, N, K):
    t, _ = _weight(N, K, bits, zp=zp, g_idx=g_idx, seed=M + N + K)
    Wq, s, z, gi = _dev_args(t, dev)
    W = _ref_w(t, dtype)
    g = torch.Generator().manual_seed(5)
    X = torch.randn(M, K, generator=g).to(dtype).to(dev)
    bias = (torch.randn(N, generator=g) * 0.1).to(dtype)
    Y1 = ops.gemm_wq_skinny(X, Wq, s, zp_w=z, g_idx=gi, bias=bias.to(dev))
    Y2 = ops.gemm_wq_skinny(X, Wq, s, zp_w=z, g_idx=gi, bias=bias.to(dev))
    torch.cuda.synchronize()
    _bits_equal(Y1, Y2)
    _check_bound(Y1, X, W, bias)


def test_skinny_pitched_activations(ops, dev):
    t, _ = _weight(64, 1024, 4, seed=2)
    Wq, s, z, gi = _dev_args(t, dev)
    wide = torch.randn(4, 1100, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(dev)
    X = wide[:, 8:1032]
    Y = ops.gemm_wq_skinny(X, Wq, s)
    torch.cuda.synchronize()
    _bits_equal(Y, ops.gemm_wq_skinny(X.contiguous(), Wq, s))
    _check_bound(Y, X, _ref_w(t, torch.bfloat16))


def test_skinny_and_dequant_refuse_bad_input(ops, dev):
    t, _ = _weight(32, 256, 4, seed=1)
    Wq, s, _, _ = _dev_args(t, dev)
    X = torch.zeros(2, 256, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError):
        ops.gemm_wq_skinny(torch.zeros(17, 256, dtype=torch.bfloat16, device=dev), Wq, s)
    with pytest.raises(TypeError):
        ops.gemm_wq_skinny(X.float(), Wq, s)
    with pytest.raises(ValueError):
        ops.gemm_wq_skinny(torch.zeros(256, 2, dtype=torch.bfloat16, device=dev).t(), Wq, s)
    with pytest.raises(ValueError):
        ops.gemm_wq_skinny(X, Wq, torch.ones(32, 3, device=dev))                 # neither 1 nor K/128 groups
    with pytest.raises(ValueError):
        ops.gemm_wq_skinny(X[:, :200], Wq, s)                                    # packed width != ceil(K/8)
    with pytest.raises(TypeError):
        ops.gemm_wq_skinny(X, Wq, s, zp_w=torch.zeros(32, 2, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.gemm_wq_skinny(X, Wq, s, g_idx=torch.zeros(255, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        ops.gemm_wq_skinny(X, Wq, s, bias=torch.zeros(32, device=dev))
    with pytest.raises(TypeError):
        ops.gemm_wq_skinny(X, Wq.float(), s)
    with pytest.raises(ValueError):
        ops.dequantize_weight(Wq, s)                                             # packed int4 needs K
    with pytest.raises(TypeError):
        ops.dequantize_weight(Wq, s, K=256, dtype=torch.float32)
    with pytest.raises(ValueError):
        ops.dequantize_weight(Wq, s, K=256, out=torch.empty(32, 255, dtype=torch.bfloat16, device=dev))


# ---- WeightOnlyLinear -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,zp,g_idx", [(4, False, False), (4, True, True), (8, False, False)])
def test_module_paths(dev, bits, zp, g_idx):
    import torch.nn.functional as F

    from quantool_amd.engine.qlinear import weight_only_linear_from_tensors

    N, K = 384, 1024
    t, _ = _weight(N, K, bits, zp=zp, g_idx=g_idx, seed=bits + 10 * zp)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(0)) * 0.1).to(torch.bfloat16).to(dev)
    m = weight_only_linear_from_tensors("m", {k: v.to(dev) for k, v in t.items()}, bias=bias)
    W = _ref_w(t, torch.bfloat16).to(dev)
    g = torch.Generator().manual_seed(1)
    big = torch.randn(2, 40, K, generator=g).to(torch.bfloat16).to(dev)
    small = torch.randn(1, 5, K, generator=g).to(torch.bfloat16).to(dev)
    with torch.no_grad():
        assert torch.equal(m(big), F.linear(big, W, bias))                    # 80 rows: dequantise + F.linear
        y = m(small)                                                          # 5 rows: the skinny kernel
        _check_bound(y.reshape(5, N), small.reshape(5, K), W, bias)
        m.skinny_max_m = 4
        assert torch.equal(m(small), F.linear(small, W, bias))
        m.skinny_max_m = 16
        y2 = m(small)
    _bits_equal(y, y2)


# ---- end to end -----------------------------------------------------------------------------------------------------
def _save_oneshot_group(dev, out_dir):
    from quantool_amd.engine.modifiers import GPTQModifier
    from quantool_amd.engine.oneshot import oneshot

    model = _tiny_llama(dev)
    g = torch.Generator().manual_seed(2)
    data = [{"input_ids": torch.randint(0, 512, (48,), generator=g)} for _ in range(8)]
    oneshot(model=model, dataset=data, recipe=GPTQModifier(scheme="W4A16", actorder="group"), output_dir=str(out_dir),
            num_calibration_samples=8, max_seq_length=64, shuffle_calibration_samples=False)
    torch.cuda.synchronize()


def _greedy_logits(model, prompt, steps, feed=None):
    """Per-step last-position logits of a KV-cached greedy decode (tokens from ``feed`` when given)."""
    out = model(input_ids=prompt, use_cache=True)
    past, logits, toks = out.past_key_values, [out.logits[:, -1].float()], []
    for i in range(steps):
        tok = logits[-1].argmax(-1, keepdim=True) if feed is None else feed[i]
        toks.append(tok)
        out = model(input_ids=tok, past_key_values=past, use_cache=True)
        past = out.past_key_values
        logits.append(out.logits[:, -1].float())
    return torch.stack(logits), toks


@pytest.mark.parametrize("source", ["gptq", "awq_asym", "oneshot_group"])
def test_end_to_end_packed_model(dev, tmp_path, monkeypatch, source):
    from quantool_amd.engine.qlinear import WeightOnlyLinear, load_quantized
    from quantool_amd.evaluate import perplexity
    from quantool_amd.hip import ops

    monkeypatch.chdir(tmp_path)
    ckpt = tmp_path / "ckpt"
    if source == "gptq":
        _quantize_and_save("gptq", "W4A16", dev, ckpt)
    elif source == "awq_asym":
        _quantize_and_save("awq", "W4A16_ASYM", dev, ckpt)
    else:
        _save_oneshot_group(dev, ckpt)
    dense = load_quantized(ckpt, device=dev)
    packed = load_quantized(ckpt, device=dev, a16="packed")
    wols = {n: m for n, m in packed.named_modules() if isinstance(m, WeightOnlyLinear)}
    assert len(wols) == 14
    if source == "awq_asym":
        assert all(m.weight_zero_point is not None for m in wols.values())
    if source == "oneshot_group":
        assert all(m.g_idx is not None for m in wols.values())
    # every forward of the perplexity run has 4 x 96 rows: the dequantise path, equal to the bit
    ids = _eval_ids()
    p_dense = perplexity(dense, ids, batch_size=4)["perplexity"]
    p_packed = perplexity(packed, ids, batch_size=4)["perplexity"]
    assert math.isfinite(p_dense) and p_packed == p_dense, (p_packed, p_dense)

    # a KV-cached greedy decode: the 24-token prompt takes the dequantise path, every later step one row through the
    # skinny kernel
    calls = {"skinny": 0, "dequant": 0}
    real_skinny, real_dequant = ops.gemm_wq_skinny, ops.dequantize_weight

    def skinny(*a, **k):
        calls["skinny"] += 1
        return real_skinny(*a, **k)

    def dequant(*a, **k):
        calls["dequant"] += 1
        return real_dequant(*a, **k)

    rows = []
    handles = [m.register_forward_hook(lambda mod, inp, out: rows.append(inp[0].reshape(-1, mod.in_features).shape[0]))
               for m in wols.values()]
    prompt = ids[:1, :24].to(dev)
    steps = 16
    with torch.no_grad():
        ref, toks = _greedy_logits(dense, prompt, steps)
        monkeypatch.setattr(ops, "gemm_wq_skinny", skinny)
        monkeypatch.setattr(ops, "dequantize_weight", dequant)
        got, _ = _greedy_logits(packed, prompt, steps, feed=toks)
    for h in handles:
        h.remove()
    assert rows[:14] == [24] * 14 and rows[14:] == [1] * (14 * steps)
    assert calls == {"skinny": 14 * steps, "dequant": 14}
    # Each skinny output differs from the dense Linear's by at most its own rounding (1/2 ulp) plus the summation-order
    # bound, i.e. about one bf16 ulp (2^-8 relative); through 2 layers of 7 Linears, the residual adds and the norms
    # these stay a few ulps.  Allow 2^-4 of the logit scale: a wrong weight, scale or zero-point moves logits by O(1).
    diff = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert diff <= 2.0 ** -4 * scale, (diff, scale)
    # every WeightOnlyLinear against what the checkpoint files define (fp64, no shared decoding): the GEMV and the
    # dequantise paths
    from tests.test_gpu_ckpt_e2e import check_modules_against_files

    assert check_modules_against_files(packed, ckpt, dev, tokens=(1, 17)) == 2 * 14
