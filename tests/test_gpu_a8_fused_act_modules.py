"""The fused SiLU(gate) * up + quantise pass inside the A8 modules, on the device: a ``QuantizedExperts`` bank with
``fused_act`` on, a ``QuantizedMLP`` and whole checkpoints loaded with ``a8_fused_act=True`` give, to the bit, what the
three separate passes give."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _levels(shape, bits, seed):
    lo, hi = (-8, 8) if bits == 4 else (-128, 128)
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int8)


def _scales(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 1e-2 + 1e-4


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.isfinite(a.float()).all() and bool(a.any()), what
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


def _count(monkeypatch, ops, name):
    calls = []
    real = getattr(ops, name)

    def counted(*a, **kw):
        calls.append(name)
        return real(*a, **kw)

    monkeypatch.setattr(ops, name, counted)
    return calls


# ---- QuantizedExperts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", [False, True])
def test_bank_is_the_same_with_and_without_the_fused_pass(ops, dev, monkeypatch, int4):
    from quantool_amd.engine.qlinear import QuantizedExperts, pack_int4

    E, H, I, k = 4, 256, 384, 2
    bits = 4 if int4 else 8
    gu, dn = _levels((E, 2 * I, H), bits, 1), _levels((E, H, I), bits, 2)
    s_gu, s_dn = _scales((E, 2 * I, H // 128 if int4 else 1), 3), _scales((E, H, I // 128 if int4 else 1), 4)
    if int4:
        gu, dn = torch.stack([pack_int4(w) for w in gu]), torch.stack([pack_int4(w) for w in dn])
    qe = QuantizedExperts(H, I, gu, s_gu, dn, s_dn, nn.SiLU(), act_symmetric=not int4).to(dev)
    fused = _count(monkeypatch, ops, "act_mul_quantize_i8")
    plain = _count(monkeypatch, ops, "quantize_tokens_i8")
    for T in (1, 5, 40, 300):
        g = torch.Generator().manual_seed(T)
        x = (torch.randn(T, H, generator=g) * 2).to(torch.bfloat16).to(dev)
        idx = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(T)]).to(dev)
        w = torch.softmax(torch.randn(T, k, generator=g), -1).to(dev)
        outs = {}
        for on in (False, True):
            qe.fused_act = on
            fused.clear()
            plain.clear()
            with torch.no_grad():
                outs[on] = qe(x, idx, w)
            assert (len(fused), len(plain)) == ((1, 1) if on else (0, 2))
        torch.cuda.synchronize()
        _same(outs[True], outs[False], f"int4={int4} T={T}")


# ---- QuantizedMLP ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int4", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_mlp_is_the_three_linears_and_torchs_glue(ops, dev, monkeypatch, int4, dt):
    from quantool_amd.engine.qlinear import QuantizedLinear, QuantizedMLP, pack_int4

    HID, INTER = 256, 640
    bits = 4 if int4 else 8

    def linear(K, N, seed, col_perm=None, bias=None):
        q = _levels((N, K), bits, seed)
        return QuantizedLinear(K, N, pack_int4(q) if int4 else q, _scales((N, K // 128 if int4 else 1), seed + 50),
                               act_symmetric=not int4, col_perm=col_perm, bias=bias).to(dev)

    perm = torch.randperm(INTER, generator=torch.Generator().manual_seed(8)).to(torch.int32)
    bias = (torch.randn(HID, generator=torch.Generator().manual_seed(9)) * 0.5).to(dt)
    gate, up, down = linear(HID, INTER, 1), linear(HID, INTER, 2), linear(INTER, HID, 3, col_perm=perm, bias=bias)
    mlp = QuantizedMLP(gate, up, down, nn.SiLU())
    fused = _count(monkeypatch, ops, "act_mul_quantize_i8")
    plain = _count(monkeypatch, ops, "quantize_tokens_i8")
    for M in (1, 16, 33, 200):
        x = (torch.randn(M, HID, generator=torch.Generator().manual_seed(M)) * 2).to(dt).to(dev)
        if M == 200:
            x = x.view(2, 100, HID)
        with torch.no_grad():
            plain.clear()
            want = down(F.silu(gate(x)) * up(x))
            assert len(plain) == 3 and not fused
            plain.clear()
            got = mlp(x)
            assert (len(fused), len(plain)) == (1, 1)
            fused.clear()
        torch.cuda.synchronize()
        _same(got, want, f"int4={int4} {dt} M={M}")


# ---- whole checkpoints ----------------------------------------------------------------------------------------------
def _logits_both_ways(path, dev, module_type):
    from quantool_amd.engine.qlinear import load_quantized

    ids = torch.randint(0, 320, (2, 24), generator=torch.Generator().manual_seed(11)).to(dev)
    out = {}
    for on in (False, True):
        model = load_quantized(path, device=dev, a8_fused_act=on)
        mods = [m for m in model.modules() if isinstance(m, module_type)]
        if on:      # a QuantizedMLP exists only when asked for; a bank exists either way and carries the switch
            assert mods and all(getattr(m, "fused_act", True) is True for m in mods)
        else:
            assert not any(getattr(m, "fused_act", True) for m in mods)
        with torch.no_grad():
            out[on] = model(input_ids=ids).logits
        torch.cuda.synchronize()
        del model
    return out


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_dense_checkpoint_logits(ops, dev, tmp_path, monkeypatch, scheme):
    from quantool_amd.engine.qlinear import QuantizedMLP
    from tests.a8_fused_ckpt import write_llama

    write_llama(tmp_path, scheme, layers=2, bias=True)
    fused = _count(monkeypatch, ops, "act_mul_quantize_i8")
    out = _logits_both_ways(tmp_path, dev, QuantizedMLP)
    assert len(fused) == 2                                   # one per layer, in the second load alone
    _same(out[True], out[False], f"{scheme} dense logits")


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_moe_checkpoint_logits(ops, dev, tmp_path, monkeypatch, scheme):
    from quantool_amd.engine.qlinear import QuantizedExperts
    from tests.a8_fused_ckpt import write_mixtral

    write_mixtral(tmp_path, scheme)
    fused = _count(monkeypatch, ops, "act_mul_quantize_i8")
    out = _logits_both_ways(tmp_path, dev, QuantizedExperts)
    assert len(fused) == 1
    _same(out[True], out[False], f"{scheme} MoE logits")
