"""The fused RMSNorm + quantise pass (``qt_rmsnorm_quantize_i8``) in the A8 modules and the loader, without a GPU:
``quantool_amd.hip.ops`` is replaced by a recording fake whose ``rmsnorm_quantize_i8`` is the five-line torch sequence
plus the fake's quantiser.  ``load_quantized(..., a8_fused_norm=True)`` puts a ``QuantizingRMSNorm`` in front of q/k/v
and gate/up without moving a state-dict key; the consumers take the norm's rows only for the very tensor it returned,
unwritten since, and nothing stays pinned after a forward; with the switch off no new ``ops`` name is read."""
import importlib
import inspect
import textwrap

import pytest
import torch
import torch.nn as nn

from tests.a8_fused_ckpt import write_llama, write_mixtral
from tests.i8_fake_ops import fake_ops  # noqa: F401
from tests.norm_fake_ops import NormRecorder, quantizing_norms, tag_linears, torch_rmsnorm

IDS = torch.arange(48).reshape(2, 24) % 320


@pytest.fixture
def rec(monkeypatch):
    """A NormRecorder in the place of ``ops``; the norms take CPU tensors to it as they take device tensors to the
    kernel."""
    import quantool_amd.hip as hip
    from quantool_amd.engine.qmodules import QuantizingRMSNorm
    from quantool_amd.hip import ops as real   # noqa: F401  (the attribute the modules import must exist first)

    r = NormRecorder()
    monkeypatch.setattr(hip, "ops", r)
    monkeypatch.setattr(QuantizingRMSNorm, "device_types", ("cuda", "cpu"))
    return r


def _linear(K, N, sym=True, col_perm=None):
    from quantool_amd.engine.qmodules import QuantizedLinear

    return QuantizedLinear(K, N, torch.zeros(N, K, dtype=torch.int8), torch.ones(N, 1), sym, col_perm=col_perm)


def _norm(K=64, consumers=None, eps=1e-5, takes=None):
    from quantool_amd.engine.qmodules import QuantizingRMSNorm

    g = torch.Generator().manual_seed(4)
    w = nn.Parameter((torch.randn(K, generator=g) * 0.5 + 1).to(torch.bfloat16), requires_grad=False)
    consumers = [_linear(K, 32), _linear(K, 48), _linear(K, 16)] if consumers is None else consumers
    return QuantizingRMSNorm(w, eps, consumers, takes=takes), consumers


def _run(model):
    with torch.no_grad():
        return model(IDS).logits


# ---- the switch -----------------------------------------------------------------------------------------------------
def test_the_switch_is_off_by_default(tmp_path):
    from quantool_amd.engine.qlinear import QuantizedLinear, load_quantized

    assert inspect.signature(load_quantized).parameters["a8_fused_norm"].default is False
    assert QuantizedLinear.rows_from is None
    write_llama(tmp_path, "W8A8", layers=1)
    model = load_quantized(tmp_path, device="cpu")
    assert model._qt_checkpoint["a8_fused_norm"] is False and quantizing_norms(model) == {}
    assert all("rows_from" not in vars(m) for m in model.modules())


def test_off_reads_no_new_name(tmp_path, fake_ops):
    """``fake_ops`` is the shared Recorder, which carries no ``rmsnorm_quantize_i8``: reading it would raise."""
    from quantool_amd.engine.qlinear import load_quantized

    assert not hasattr(fake_ops, "rmsnorm_quantize_i8")
    write_llama(tmp_path, "W8A8", layers=1)
    assert _run(load_quantized(tmp_path, device="cpu")).shape == (2, 24, 320)
    assert len(fake_ops.calls) == 7


def test_loader_rejects_a_value_that_is_no_bool(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    write_llama(tmp_path, "W8A8", layers=1)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="a8_fused_norm"):
            load_quantized(tmp_path, device="cpu", a8_fused_norm=bad)


def test_a16_checkpoints_ignore_it(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    write_llama(tmp_path, "W4A16", layers=1)
    for kw in (dict(), dict(a16="packed")):
        model = load_quantized(tmp_path, device="cpu", a8_fused_norm=True, **kw)
        assert "a8_fused_norm" not in model._qt_checkpoint and quantizing_norms(model) == {}


# ---- the loader on a Llama ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_act", [False, True])
@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_loader_wraps_both_norms_and_the_consumers_take_their_rows(tmp_path, rec, scheme, fused_act):
    from quantool_amd.engine.qlinear import QuantizedMLP, load_quantized

    write_llama(tmp_path, scheme, bias=True)
    plain = load_quantized(tmp_path, device="cpu", a8_fused_act=fused_act)
    model = load_quantized(tmp_path, device="cpu", a8_fused_act=fused_act, a8_fused_norm=True)
    assert model._qt_checkpoint["a8_fused_norm"] is True and model._qt_checkpoint["a8_fused_act"] is fused_act
    norms = quantizing_norms(model)
    assert sorted(norms) == sorted(f"model.layers.{i}.{n}" for i in range(2)
                                   for n in ("input_layernorm", "post_attention_layernorm"))
    assert type(model.model.norm).__name__ == "LlamaRMSNorm"
    for layer in model.model.layers:
        assert isinstance(layer.mlp, QuantizedMLP) is fused_act
        assert layer.post_attention_layernorm.takes == (1 if fused_act else 2)
        assert layer.input_layernorm.takes == 3
        attn, mlp = layer.self_attn, layer.mlp
        assert all(p.rows_from is layer.input_layernorm.shared for p in (attn.q_proj, attn.k_proj, attn.v_proj))
        assert all(p.rows_from is layer.post_attention_layernorm.shared for p in (mlp.gate_proj, mlp.up_proj))
        assert attn.o_proj.rows_from is None and mlp.down_proj.rows_from is None
    a, b = plain.state_dict(), model.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)

    tag_linears(model, rec)
    rec.clear()
    out = _run(model)
    assert out.shape == (2, 24, 320)
    own = [f"model.layers.{i}.{n}" for i in range(2)
           for n in (("self_attn.o_proj",) if fused_act else ("self_attn.o_proj", "mlp.down_proj"))]
    assert [c for c, _ in rec.quantised] == own
    sym = scheme != "W4A8" or model.model.layers[0].self_attn.q_proj.act_symmetric
    assert rec.norms == [((48, 256), sym, None)] * 4
    assert len(rec.fused) == (2 if fused_act else 0)
    assert len(rec.calls) == 14                                # every GEMM still runs
    assert not any(n.shared.holds_tensors for n in norms.values())

    # the same forward with the default norms: fake GEMMs return zeros, so the logits are those of the embedding
    # path alone and must agree, and the default model quantises for all seven Linears of a layer
    tag_linears(plain, rec)
    rec.clear()
    ref = _run(plain)
    assert torch.equal(out, ref)
    assert len(rec.quantised) == (10 if fused_act else 14) and rec.norms == []


def test_loader_leaves_norms_whose_consumers_permute_differently(tmp_path):
    """actorder ``group`` gives every Linear a column permutation of its own: no rows can be shared."""
    from quantool_amd.engine.qlinear import load_quantized

    write_llama(tmp_path, "W4A8", g_idx=True)
    model = load_quantized(tmp_path, device="cpu", a8_fused_norm=True)
    assert model._qt_checkpoint["a8_fused_norm"] is True and quantizing_norms(model) == {}
    for layer in model.model.layers:
        assert type(layer.input_layernorm).__name__ == "LlamaRMSNorm"
        assert type(layer.post_attention_layernorm).__name__ == "LlamaRMSNorm"
        assert layer.self_attn.q_proj.col_perm is not None and layer.self_attn.q_proj.rows_from is None


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_mixtral_gets_the_first_norm_only(tmp_path, rec, scheme):
    from quantool_amd.engine.qlinear import load_quantized

    write_mixtral(tmp_path, scheme)
    plain = load_quantized(tmp_path, device="cpu")
    model = load_quantized(tmp_path, device="cpu", a8_fused_norm=True)
    assert sorted(quantizing_norms(model)) == ["model.layers.0.input_layernorm"]
    assert type(model.model.layers[0].post_attention_layernorm).__name__ == "MixtralRMSNorm"
    assert list(plain.state_dict()) == list(model.state_dict())
    tag_linears(model, rec)
    rec.clear()
    assert _run(model).shape == (2, 24, 320)
    assert len(rec.norms) == 1
    assert [c for c, _ in rec.quantised if c is not None] == ["model.layers.0.self_attn.o_proj"]
    assert not model.model.layers[0].input_layernorm.shared.holds_tensors


# ---- the hand-off ---------------------------------------------------------------------------------------------------
def test_take_gives_the_rows_for_that_tensor_only(rec):
    norm, consumers = _norm()
    x = torch.randn(2, 5, 64, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    y = norm(x)
    assert y.shape == x.shape and torch.equal(y, torch_rmsnorm(x, norm.weight, 1e-5))
    assert norm.shared.holds_tensors and norm.shared.left == 3 and rec.quantised == []
    rows = [c.quantize_rows(y) for c in consumers]
    assert rec.quantised == [] and not norm.shared.holds_tensors and norm.shared.left == 0
    assert all(r[0] is rows[0][0] and r[1] is rows[0][1] for r in rows)
    again = consumers[0].quantize_rows(y)                      # a fourth asker quantises for itself
    assert rec.quantised == [(None, (10, 64))]
    assert torch.equal(again[0], rows[0][0]) and torch.equal(again[1], rows[0][1]) and again[2] is None


@pytest.mark.parametrize("sym", [True, False])
def test_a_clone_or_a_written_tensor_is_quantised_afresh(rec, sym):
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(1)).to(torch.int32)
    consumers = [_linear(64, 32, sym, perm), _linear(64, 48, sym, perm.clone())]
    norm, _ = _norm(consumers=consumers)
    x = torch.randn(7, 64, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)

    y = norm(x)
    kept = consumers[0].quantize_rows(y)
    assert rec.quantised == [] and rec.norms[-1][1] is sym and rec.norms[-1][2] is consumers[0].col_perm
    own = consumers[1].quantize_rows(y.clone())                # not the tensor the norm returned
    assert len(rec.quantised) == 1
    for a, b in zip(kept, own):
        assert (a is None and b is None) or torch.equal(a, b)
    assert (kept[2] is None) is sym

    y = norm(x)
    y.mul_(2)                                                  # written in place since
    stale = consumers[0].quantize_rows(y)
    assert len(rec.quantised) == 2
    fresh = rec.quantize_tokens_i8(y, sym, perm)
    for a, b in zip(stale, fresh):
        assert (a is None and b is None) or torch.equal(a, b)
    assert not torch.equal(stale[1], kept[1])                  # and they are the doubled rows, not the norm's

    y = norm(x)                                                # the next forward starts over
    assert norm.shared.left == 2 and consumers[1].quantize_rows(y)[0] is norm.shared.rows[0]


def test_the_torch_sequence_runs_where_the_kernel_does_not(rec, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizingRMSNorm

    norm, consumers = _norm()
    x = torch.randn(3, 64, generator=torch.Generator().manual_seed(3))
    for bad in (x, x.to(torch.float16)):                       # fp32; 16-bit, but not the weight's dtype
        y = norm(bad)
        assert y.dtype == torch.promote_types(bad.dtype, torch.bfloat16)
        assert rec.norms == [] and not norm.shared.holds_tensors
    xb = x.to(torch.bfloat16)
    grad = xb.clone().requires_grad_(True)
    y = norm(grad)
    assert rec.norms == [] and y.requires_grad and torch.equal(y, torch_rmsnorm(xb, norm.weight, 1e-5))
    monkeypatch.setattr(QuantizingRMSNorm, "MAX_K", 63)
    assert torch.equal(norm(xb), y) and rec.norms == []
    monkeypatch.setattr(QuantizingRMSNorm, "MAX_K", 32768)
    monkeypatch.setattr(QuantizingRMSNorm, "device_types", ("cuda",))
    assert torch.equal(norm(xb), y) and rec.norms == []        # a CPU tensor, as the class ships
    assert QuantizingRMSNorm.MAX_K == 32768
    consumers[0].quantize_rows(y)
    assert len(rec.quantised) == 1


class LlamaRMSNorm(nn.Module):
    """A stand-in with the name and the attributes of the transformers class."""

    def __init__(self, K=64):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(K, dtype=torch.bfloat16))
        self.variance_epsilon = 1e-6


class GemmaRMSNorm(LlamaRMSNorm):
    pass


def test_refusal():
    from quantool_amd.engine.qmodules import QuantizingRMSNorm

    perm = torch.randperm(64, generator=torch.Generator().manual_seed(5)).to(torch.int32)
    no = QuantizingRMSNorm.refusal
    three = [_linear(64, 32), _linear(64, 48), _linear(64, 16)]
    assert no(LlamaRMSNorm(), three) is None
    assert no(LlamaRMSNorm(), [_linear(64, 32, False, perm), _linear(64, 8, False, perm.clone())]) is None
    assert "GemmaRMSNorm" in no(GemmaRMSNorm(), three)
    assert "QuantizedLinears" in no(LlamaRMSNorm(), three[:2] + [nn.Linear(64, 16)])
    assert "QuantizedLinears" in no(LlamaRMSNorm(), [])
    assert "QuantizedLinears" in no(LlamaRMSNorm(), [three[0], None])
    assert "in_features" in no(LlamaRMSNorm(), [three[0], _linear(128, 32)])
    assert "width" in no(LlamaRMSNorm(128), three)
    assert "act_symmetric" in no(LlamaRMSNorm(), [three[0], _linear(64, 32, sym=False)])
    assert "col_perm" in no(LlamaRMSNorm(), [three[0], _linear(64, 32, col_perm=perm)])
    assert "col_perm" in no(LlamaRMSNorm(), [_linear(64, 32, col_perm=perm), _linear(64, 32, col_perm=perm.flip(0))])
    with pytest.raises(ValueError, match="col_perm"):
        QuantizingRMSNorm(LlamaRMSNorm().weight, 1e-6, [three[0], _linear(64, 32, col_perm=perm)])


def test_the_norm_keeps_its_state_dict_key():
    norm, _ = _norm()
    assert list(norm.state_dict()) == ["weight"] and [n for n, _ in norm.named_children()] == []
    assert norm.variance_epsilon == 1e-5


EXPECTED_FORWARD = """\
input_dtype = hidden_states.dtype
hidden_states = hidden_states.to(torch.float32)
variance = hidden_states.pow(2).mean(-1, keepdim=True)
hidden_states = hidden_states * torch.rsqrt(variance + self.variance_epsilon)
return self.weight * hidden_states.to(input_dtype)
"""


def test_the_listed_norms_are_the_five_line_sequence():
    """Every class name ``QuantizingRMSNorm`` accepts is, in the installed transformers, exactly the sequence the kernel
    restates; and the listed decoder layers hand each norm's output straight to its consumers' parent."""
    from quantool_amd.engine.qmodules import QuantizingRMSNorm

    assert QuantizingRMSNorm.PLAIN_NORMS == ("LlamaRMSNorm", "MistralRMSNorm", "Qwen2RMSNorm", "Qwen3RMSNorm",
                                             "MixtralRMSNorm")
    for name in QuantizingRMSNorm.PLAIN_NORMS:
        arch = name[:-len("RMSNorm")].lower()
        mod = importlib.import_module(f"transformers.models.{arch}.modeling_{arch}")
        body = inspect.getsource(getattr(mod, name).forward).split("\n", 1)[1]
        assert textwrap.dedent(body) == EXPECTED_FORWARD, name
        layer = inspect.getsource(getattr(mod, f"{name[:-len('RMSNorm')]}DecoderLayer").forward)
        flat = " ".join(layer.split())
        assert "hidden_states = self.input_layernorm(hidden_states)" in flat, name
        assert "self.self_attn( hidden_states=hidden_states," in flat, name
        assert ("hidden_states = self.post_attention_layernorm(hidden_states) hidden_states = self.mlp(hidden_states)"
                in flat), name
        assert f"{name[:-len('RMSNorm')]}DecoderLayer" in QuantizingRMSNorm.PLAIN_LAYERS
