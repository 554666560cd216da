"""qt_gemm_i8_ring_w4: the 256 x 256 LDS-ring int8 GEMM for W4A8 prefill (packed int4 weights, one scale per 128 columns).

Its contract is bit equality with the tiled qt_gemm_i8 on the same arguments, so every comparison here is on bit
patterns.  That alone would pass two kernels wrong in the same way, so the same cases also go against the fp64 reference
of tests/ckpt_reference.py within the project's own bound for this sequence (``gemm_i8_tolerance`` with G groups), an
identity test pins which nibble every A byte multiplies and which group every k belongs to, and a test whose inputs are
shown on the CPU to be sensitive to the order of the fp32 group fold pins that order.  Shapes are in the kernel's own
constants: U = the K-tile = one weight group, R = the ring's slots, L = its lead."""
import numpy as np
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_i8_ring import _acts, _raw_ring
from tests.test_gpu_i8_skinny import _bias, _same_bits, _sentinel, _untouched
from tests.test_gpu_runtime_edges import _leaves, _levels, _qweight, cr_wsum

pytestmark = pytest.mark.gpu


def _url():
    from quantool_amd.hip import ops

    return ops.I8_RING_W4_K_UNIT, ops.I8_RING_W4_SLOTS, ops.I8_RING_W4_LEAD


def _case(ops, dev, M, N, K, seed):
    """One packed weight and both quantisations of one activation matrix, with their fp64 references (computed once)."""
    G = K // 128
    q4 = _levels((N, K), 4, seed=seed)
    t = _leaves(q4, 4, G, seed=seed + 1)
    X = _acts(M, K, dev, seed=seed + 2)
    out = {"Wq": _qweight(t, dev), "s_w": t["weight_scale"].to(dev), "wsum": cr_wsum(q4, G).to(dev), "G": G, "K": K}
    for asym in (False, True):
        Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
        out[asym] = (Xq, s_x, zp_x, *cr.a8_linear(Xq, s_x, zp_x, t))
    return out


def _check(ops, c, asym, dt, bias, what):
    Xq, s_x, zp_x, y64, mag = c[asym]
    kw = dict(K=c["K"], zp_x=zp_x, wsum=c["wsum"] if asym else None, bias=bias, out_dtype=dt)
    want = ops.gemm_i8(Xq, s_x, c["Wq"], c["s_w"], **kw)
    got = ops.gemm_i8_ring_w4(Xq, s_x, c["Wq"], c["s_w"], **kw)
    torch.cuda.synchronize()
    _same_bits(got, want, what)
    if bias is not None:
        b = bias.cpu().double()
        y64, mag = y64 + b, mag + b.abs()
    cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, c["G"]), f"{what} vs fp64")


# ---- 1: the ring's depth ----------------------------------------------------------------------------------------------
# in K-tiles (4 units each: the ring holds R/4 of them and leads by L/4), and in test_ring_depth's own counts
@pytest.mark.parametrize("tiles", ["1", "R/4", "R/4+1", "R/2+1", "L-1", "L", "L+1", "R", "R+1", "2R+3"])
def test_ring_depth(ops, dev, tiles):
    """2 x 2 tiles, both edges ragged, over one K-tile (the prologue alone), exactly one trip round the ring, the first
    wrap, two trips with an odd K-tile left over, and the unit counts around the lead and the ring length."""
    U, R, L = _url()
    n = {"1": 1, "R/4": R // 4, "R/4+1": R // 4 + 1, "R/2+1": R // 2 + 1, "L-1": L - 1, "L": L, "L+1": L + 1, "R": R,
         "R+1": R + 1, "2R+3": 2 * R + 3}[tiles]
    K = U * n
    M, N = 300, 384
    c = _case(ops, dev, M, N, K, seed=K)
    for asym in (False, True):
        for dt in (torch.bfloat16, torch.float16):
            for with_bias in (False, True):
                bias = _bias(N, dt, dev, seed=N) if with_bias else None
                _check(ops, c, asym, dt, bias, f"K={K} asym={asym} {dt} bias={with_bias}")


# ---- 2: the order of the group fold -----------------------------------------------------------------------------------
def _fold32(t, s_w, s_x, bias, order):
    """The header's fp32 sequence on the CPU, every product and sum rounded on its own, groups in ``order``."""
    tot = np.zeros(t.shape[:2], np.float32)
    for g in order:
        prod = (s_w[None, :, g] * t[:, :, g].astype(np.float32)).astype(np.float32)
        tot = (tot + prod).astype(np.float32)
    y = (s_x[:, None] * tot).astype(np.float32)
    return (y + bias[None, :]).astype(np.float32)


def test_groups_are_folded_in_ascending_order(ops, dev):
    """9 groups, s_w[n, g] = 2^u with u uniform in [-6, 6], asymmetric activations.  The fp32 fold of such terms depends
    on its order in about 5 % of the elements, but a 16-bit output hides nearly all of that.  So every row is the same
    activation row and bias[n] = -(what the ascending fold gives for column n, rounded to fp16): y + bias is then the
    exact fp32 residual, and the fp16 outputs themselves differ between the ascending and the descending fold in more
    than 1 % of the elements (asserted below, on the CPU).  The kernel has to match the ascending fold -- and the tiled
    kernel -- to the bit."""
    G, M, N = 9, 300, 384
    K = G * 128
    g = torch.Generator().manual_seed(1)
    q = torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int8)
    x_row = torch.randint(-128, 128, (1, K), generator=g, dtype=torch.int8)
    s_w = torch.exp2(torch.randint(-6, 7, (N, G), generator=g).float())
    Xq = x_row.repeat(M, 1).contiguous()
    zp_x = torch.full((M,), 37, dtype=torch.int32)
    s_x = torch.full((M,), 0.0123, dtype=torch.float32)
    wsum = cr_wsum(q, G)
    # t_g on the CPU, in integers
    xi, qi = Xq[:4].numpy().astype(np.int64), q.numpy().astype(np.int64)
    t = np.stack([xi[:, j * 128:(j + 1) * 128] @ qi[:, j * 128:(j + 1) * 128].T
                  - zp_x[:4].numpy().astype(np.int64)[:, None] * wsum[:, j].numpy().astype(np.int64)[None, :]
                  for j in range(G)], 2)
    zero = np.zeros(N, np.float32)
    y_asc = _fold32(t, s_w.numpy(), s_x[:4].numpy(), zero, range(G))
    assert (y_asc.view(np.int32) != _fold32(t, s_w.numpy(), s_x[:4].numpy(), zero, range(G - 1, -1, -1)).view(np.int32)
            ).mean() >= 0.01                                            # the fp32 sequence is order-sensitive ...
    bias = -torch.from_numpy(y_asc[0]).to(torch.float16)
    b32 = bias.float().numpy()
    asc = torch.from_numpy(_fold32(t, s_w.numpy(), s_x[:4].numpy(), b32, range(G))).to(torch.float16)
    desc = torch.from_numpy(_fold32(t, s_w.numpy(), s_x[:4].numpy(), b32, range(G - 1, -1, -1))).to(torch.float16)
    differ = (asc.view(torch.int16) != desc.view(torch.int16)).float().mean().item()
    print(f"fp16 outputs that differ between the ascending and the descending fold: {differ:.4f}")
    assert differ >= 0.01                                               # ... and so are these 16-bit outputs

    t4 = _leaves(q, 4, G, seed=0)
    Wq = _qweight(t4, dev)
    kw = dict(K=K, zp_x=zp_x.to(dev), wsum=wsum.to(dev), bias=bias.to(dev), out_dtype=torch.float16)
    want = ops.gemm_i8(Xq.to(dev), s_x.to(dev), Wq, s_w.to(dev), **kw)
    got = ops.gemm_i8_ring_w4(Xq.to(dev), s_x.to(dev), Wq, s_w.to(dev), **kw)
    torch.cuda.synchronize()
    _same_bits(got, want, "group order vs the tiled kernel")
    _same_bits(got.cpu(), asc[:1].expand(M, N).contiguous(), "group order vs the ascending CPU fold")
    t4["weight_scale"] = s_w
    y64, mag = cr.a8_linear(Xq, s_x, zp_x, t4)
    b = bias.double()
    cr.assert_within(got, y64 + b, cr.gemm_i8_tolerance(got.cpu(), mag + b.abs(), G), "group order vs fp64")


# ---- 3: tile edges and tile order -----------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(256, 256), (255, 256), (257, 200), (1, 257), (513, 1), (1100, 1600)])
def test_tile_edges_and_order(ops, dev, M, N):
    """Full, one short and one over in either direction, one row, one column, and 5 x 7 = 35 tiles (more than 8 and no
    multiple of 8: any remap of workgroups onto tiles has to be a bijection there), at the first-wrap K."""
    U, R, L = _url()
    K = (R + 1) * U
    c = _case(ops, dev, M, N, K, seed=M + N)
    _check(ops, c, True, torch.bfloat16, _bias(N, torch.bfloat16, dev, seed=M), f"M={M} N={N}")


# ---- 4: lane, slot and nibble maps ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scales", ["unit", "g+1"])
def test_identity_activations_read_the_weight(ops, dev, scales):
    """Xq = the K x K identity, unit s_x, no zero-point: with unit s_w Y[m, n] = (float)W[n, m] exactly, which pins the
    nibble every A byte multiplies, across k-steps, units and ring slots; with s_w[n, g] = g + 1 it is
    (m // 128 + 1) W[n, m], which pins the group every k belongs to."""
    U, R, L = _url()
    K, N = (R + 1) * U, 96
    G = K // U
    W = _levels((N, K), 4, seed=77)
    assert len({tuple(r) for r in W.tolist()}) == N and not torch.equal(W[:, :N], W[:, :N].T)
    assert not torch.equal(W, W.flip(1))
    s_w = torch.ones(N, G) if scales == "unit" else (torch.arange(G).float() + 1).repeat(N, 1).contiguous()
    want = W.T.float() * (1.0 if scales == "unit" else (torch.arange(K) // U + 1).float()[:, None])
    assert float(want.abs().max()) <= 2048                              # exact in fp16
    Wq = _qweight(_leaves(W, 4, G, seed=1), dev)
    Xq = torch.eye(K, dtype=torch.int8, device=dev)
    Y = ops.gemm_i8_ring_w4(Xq, torch.ones(K, device=dev), Wq, s_w.to(dev), K=K, out_dtype=torch.float16)
    torch.cuda.synchronize()
    _same_bits(Y.cpu(), want.to(torch.float16).contiguous(), f"identity, {scales} scales")


# ---- 5 + 6: raw C ABI calls -----------------------------------------------------------------------------------------
NAME = "qt_gemm_i8_ring_w4"


def test_caller_owned_y_keeps_its_padding(ops, dev):
    from quantool_amd.hip import _lib

    U, R, L = _url()
    M, N, K = 257, 200, (R + 1) * U
    ldy = N + 17
    c = _case(ops, dev, M, N, K, seed=4)
    Xq, s_x, zp_x, _, _ = c[True]
    bias = _bias(N, torch.bfloat16, dev, seed=5)
    Ys = {}
    for name in ("qt_gemm_i8", NAME):
        Ys[name] = _sentinel((M + 3, ldy), torch.bfloat16, dev)
        _raw_ring(ops, Xq.data_ptr(), M, K, c["Wq"].data_ptr(), _lib.QT_W_INT4_PACKED, N, s_x, zp_x, c["s_w"], c["G"],
                  c["wsum"], bias, Ys[name], ldy, name=name)
    torch.cuda.synchronize()
    Y = Ys[NAME]
    assert _untouched(Y[:, N:]) and _untouched(Y[M:]) and not _untouched(Y[:M, :N])
    _same_bits(Y[:M, :N].contiguous(), Ys["qt_gemm_i8"][:M, :N].contiguous(), "ldy > N")


def test_refusals_write_nothing_and_name_the_reason(ops, dev):
    from quantool_amd.hip import _lib
    from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

    U, R, L = _url()
    M, N, K = 20, 32, 4 * 128
    KBIG = 32768 + U
    # every pointer below lies inside one of these buffers with room for the whole operand behind it
    xbuf = torch.ones(M * KBIG + 32, dtype=torch.int8, device=dev)
    wbuf = torch.zeros(N * KBIG + 32, dtype=torch.int8, device=dev)
    assert xbuf.data_ptr() % 16 == 0 and wbuf.data_ptr() % 16 == 0
    s_x = torch.ones(M, device=dev)
    s_w = torch.ones(N, KBIG // 128, device=dev)
    zp = torch.zeros(M, dtype=torch.int32, device=dev)
    Y = _sentinel((M, N), torch.bfloat16, dev)
    Y32 = _sentinel((M, 2 * N), torch.float32, dev)
    assert Y32.shape == (M, N)
    X, W, I4, G = xbuf.data_ptr(), wbuf.data_ptr(), _lib.QT_W_INT4_PACKED, K // 128
    cases = {
        "int8 weights": ((X, M, K, W, _lib.QT_W_INT8, N, s_x, None, s_w, G, None, None, Y), "packed int4 weights only"),
        "G == 1": ((X, M, K, W, I4, N, s_x, None, s_w, 1, None, None, Y), "one scale per group"),
        "K % 128 != 0": ((X, M, K + 16, W, I4, N, s_x, None, s_w, G, None, None, Y), "not a multiple of the k-unit"),
        "K > 32768": ((X, M, KBIG, W, I4, N, s_x, None, s_w, KBIG // 128, None, None, Y), "> 32768"),
        "Xq misaligned": ((X + 1, M, K, W, I4, N, s_x, None, s_w, G, None, None, Y), "Xq is not 16-byte aligned"),
        "Wq misaligned": ((X, M, K, W + 4, I4, N, s_x, None, s_w, G, None, None, Y), "Wq is not 16-byte aligned"),
        "fp32 output": ((X, M, K, W, I4, N, s_x, None, s_w, G, None, None, Y32), "must be bf16 or fp16"),
        "zp_x without wsum": ((X, M, K, W, I4, N, s_x, zp, s_w, G, None, None, Y), "zp_x needs wsum"),
    }
    for what, (args, reason) in cases.items():
        with pytest.raises(HipBackendError) as e:
            _raw_ring(ops, *args, N, name=NAME)
        assert e.value.status == QT_ERR_INVALID, what
        assert reason in str(e.value), (what, str(e.value))
    torch.cuda.synchronize()
    assert _untouched(Y) and _untouched(Y32)


# ---- 7: the module, end to end --------------------------------------------------------------------------------------
def test_module_is_the_same_with_and_without_the_w4_ring(ops, dev, tmp_path, monkeypatch):
    """A tiny Llama W4A8 checkpoint (hidden 256, intermediate 512: 2 and 4 groups): logits and perplexity with every
    Linear on the ring equal those with none on it, to the bit."""
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry
    from quantool_amd.engine.qlinear import QuantizedLinear, load_quantized
    from quantool_amd.evaluate import perplexity
    from transformers import LlamaConfig, LlamaForCausalLM

    monkeypatch.chdir(tmp_path)
    cfg = LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=128, tie_word_embeddings=False)
    torch.manual_seed(0)
    dense = LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev)
    g = torch.Generator().manual_seed(2)
    data = [{"input_ids": torch.randint(0, 512, (48,), generator=g)} for _ in range(8)]
    q = QuantizerRegistry.create("smoothquant", model_id="synthetic/tiny-llama")
    q.quantize(model=dense, level="W4A8", dataset=data, num_calibration_samples=8, max_seq_length=64,
               shuffle_calibration_samples=False)
    torch.cuda.synchronize()
    q.save_pretrained(str(tmp_path / "ckpt"))
    del dense, q
    model = load_quantized(tmp_path / "ckpt", device=dev)
    lins = [m for m in model.modules() if isinstance(m, QuantizedLinear)]
    assert len(lins) == 14 and all(m.int4 and m.weight_scale.shape[1] * 128 == m.in_features for m in lins)
    ids = torch.randint(0, 512, (6, 96), generator=torch.Generator().manual_seed(11))
    monkeypatch.setattr(QuantizedLinear, "skinny_max_m", 0)
    calls = {"n": 0}
    real = ops.gemm_i8_ring_w4

    def counted(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "gemm_i8_ring_w4", counted)
    logits, ppl, used = {}, {}, {}
    for min_m in (0, 1):
        monkeypatch.setattr(QuantizedLinear, "ring_w4_min_m", min_m)
        before = calls["n"]
        with torch.no_grad():
            logits[min_m] = model(input_ids=ids[:2].to(dev)).logits
        ppl[min_m] = perplexity(model, ids, batch_size=4)["perplexity"]
        torch.cuda.synchronize()
        used[min_m] = calls["n"] - before
    assert used[0] == 0 and used[1] >= 14
    assert torch.isfinite(logits[1].float()).all()
    _same_bits(logits[1], logits[0], "W4A8 logits, ring_w4_min_m 1 vs 0")
    assert ppl[1] == ppl[0]
