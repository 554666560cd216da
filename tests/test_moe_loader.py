"""CPU side of the routed-expert runtime: ``load_quantized`` on tiny Mixtral checkpoints written the way the save path
writes them (``save_state`` after ``expert_bank_checkpoint_names``) -- A16 experts dequantised into the fused bank, A8
experts gathered into a ``QuantizedExperts``, the ``block_sparse_moe`` rename undone, and the refusals.  No GPU call."""
import pytest
import torch
import torch.nn as nn

from quantool_amd.engine.schemes import PRESET_SCHEMES
from quantool_amd.engine.sequential import expert_bank_checkpoint_names
from quantool_amd.engine.serialization import quantization_config, save_state

E, H, I = 4, 256, 384
BANK = "model.layers.0.mlp.experts"
ATTN = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj")


def _tiny_mixtral():
    from transformers import MixtralConfig, MixtralForCausalLM

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=4,
                        num_key_value_heads=2, num_local_experts=E, num_experts_per_tok=2, vocab_size=320,
                        max_position_embeddings=64, tie_word_embeddings=False)
    torch.manual_seed(0)
    return MixtralForCausalLM(cfg).to(torch.bfloat16)


def _qtensors(N, K, wa, g, *, g_idx=False, zero_point=False):
    """(levels int8 [N, K], checkpoint leaves) of one random quantized Linear under the weight args ``wa``."""
    lo, hi = (-8, 8) if wa.num_bits == 4 else (-128, 128)
    q = torch.randint(lo, hi, (N, K), generator=g, dtype=torch.int8)
    G = (K + 127) // 128 if wa.strategy == "group" else 1
    t = {"weight_scale": (torch.rand(N, G, generator=g) * 0.01 + 1e-3).to(torch.bfloat16),
         "weight_shape": torch.tensor([N, K])}
    if wa.num_bits == 4:
        from quantool_amd.engine.qlinear import pack_int4

        t["weight_packed"] = pack_int4(q)
    else:
        t["weight"] = q
    if zero_point or not wa.symmetric:
        t["weight_zero_point"] = torch.randint(-8, 8, (N, G), generator=g, dtype=torch.int8)
    if g_idx:
        t["weight_g_idx"] = (torch.randperm(K, generator=g) // 128).to(torch.int32)
    return q, t


def _write(path, scheme_name, *, g_idx=False, zero_point=False, drop=None, dense_expert=None, bias=False,
           quantize_attn=True):
    """A tiny Mixtral checkpoint under ``scheme_name``: every expert's fused gate_up [2I, H] and down [H, I] quantized
    as the save path holds them (``<bank>.experts.{e}.gate_up_proj.*``), then renamed by
    ``expert_bank_checkpoint_names`` into ``block_sparse_moe.experts.{e}.w1 / w3 / w2``.
    Returns (model, {(e, proj): (levels, leaves)} with proj in gate_up_proj / down_proj, attention levels)."""
    scheme = PRESET_SCHEMES[scheme_name]
    wa = scheme.weights
    model = _tiny_mixtral()
    state = dict(model.state_dict())
    del state[f"{BANK}.gate_up_proj"], state[f"{BANK}.down_proj"]
    g = torch.Generator().manual_seed(3)
    experts = {}
    for e in range(E):
        for proj, (N, K) in (("gate_up_proj", (2 * I, H)), ("down_proj", (H, I))):
            pre = f"{BANK}.experts.{e}.{proj}"
            if dense_expert == (e, proj):
                state[f"{pre}.weight"] = torch.randn(N, K, generator=g).to(torch.bfloat16)
                continue
            q, t = _qtensors(N, K, wa, g, g_idx=g_idx, zero_point=zero_point)
            experts[(e, proj)] = (q, t)
            for k, v in t.items():
                state[f"{pre}.{k}"] = v
            if bias:
                state[f"{pre}.bias"] = torch.zeros(N, dtype=torch.bfloat16)
    attn = {}
    if quantize_attn:
        for lin in ATTN:
            name = f"model.layers.0.{lin}"
            N, K = model.get_submodule(name).weight.shape
            del state[f"{name}.weight"]
            q, t = _qtensors(N, K, wa, g)
            attn[name] = (q, t)
            for k, v in t.items():
                state[f"{name}.{k}"] = v
    state = expert_bank_checkpoint_names(state, {BANK: None}, "mixtral")
    if drop:
        state = {k: v for k, v in state.items() if not k.startswith(drop)}
    acts = scheme.input_activations.to_config() if scheme.input_activations is not None else None
    # the save path renames ignore entries with the tensors
    ignore = ["lm_head", "model.layers.0.block_sparse_moe.gate"]
    qcfg = quantization_config(wa.to_config(), scheme.format, ignore, acts)
    save_state(state, qcfg, path, model.config.to_dict())
    return model, experts, attn


def _ckpt_name(e, role):
    return f"model.layers.0.block_sparse_moe.experts.{e}.{role}"


def test_checkpoint_is_in_the_mixtral_layout(tmp_path):
    from quantool_amd.engine.serialization import load_state

    _write(tmp_path, "W4A16")
    names = set(load_state(tmp_path))
    assert f"{_ckpt_name(2, 'w3')}.weight_packed" in names and f"{_ckpt_name(2, 'w2')}.weight_scale" in names
    assert "model.layers.0.block_sparse_moe.gate.weight" in names
    assert not any(".mlp." in n for n in names)


@pytest.mark.parametrize("scheme,g_idx", [("W4A16", False), ("W4A16", True), ("W4A16_ASYM", False),
                                          ("W4A16_ASYM", True), ("W8A16", False)])
def test_a16_experts_are_dequantized_into_the_fused_bank(tmp_path, scheme, g_idx):
    from quantool_amd.engine.qlinear import QuantizedExperts, dequantized_weight, load_quantized

    ref, experts, _ = _write(tmp_path, scheme, g_idx=g_idx)
    model = load_quantized(tmp_path, device="cpu")
    bank = model.model.layers[0].mlp.experts
    assert not isinstance(bank, QuantizedExperts)
    assert bank.gate_up_proj.dtype == torch.bfloat16
    # the checkpoint's own split halves, dequantised one by one
    from quantool_amd.engine.serialization import load_state

    state = load_state(tmp_path)
    for e in range(E):
        leaves = {r: {k.rpartition(".")[2]: v for k, v in state.items() if k.startswith(_ckpt_name(e, r) + ".")}
                  for r in ("w1", "w3", "w2")}
        w1, w3, w2 = (dequantized_weight(r, leaves[r], torch.bfloat16) for r in ("w1", "w3", "w2"))
        assert torch.equal(bank.gate_up_proj.data[e, :I], w1)
        assert torch.equal(bank.gate_up_proj.data[e, I:], w3)
        assert torch.equal(bank.down_proj.data[e], w2)
        # and they are the fused matrices' own dequantisation: the split is exact
        q, t = experts[(e, "gate_up_proj")]
        assert torch.equal(bank.gate_up_proj.data[e], dequantized_weight("gu", t, torch.bfloat16))
    # router and every other dense tensor under its transformers-5 name
    assert torch.equal(model.model.layers[0].mlp.gate.weight, ref.model.layers[0].mlp.gate.weight)
    assert torch.equal(model.model.embed_tokens.weight, ref.model.embed_tokens.weight)
    assert torch.equal(model.model.layers[0].post_attention_layernorm.weight,
                       ref.model.layers[0].post_attention_layernorm.weight)
    assert model._qt_checkpoint["ignore"] == ["lm_head", "model.layers.0.mlp.gate"]
    with torch.no_grad():
        assert torch.isfinite(model(input_ids=torch.tensor([[1, 2, 3]])).logits.float()).all()


@pytest.mark.parametrize("scheme", ["W8A8", "INT8", "W4A8"])
def test_a8_experts_become_quantized_experts(tmp_path, scheme):
    from quantool_amd.engine.qlinear import QuantizedExperts, QuantizedLinear, load_quantized, unpack_int4

    ref, experts, attn = _write(tmp_path, scheme)
    model = load_quantized(tmp_path, device="cpu")
    qe = model.model.layers[0].mlp.experts
    assert isinstance(qe, QuantizedExperts)
    assert qe.act_symmetric == PRESET_SCHEMES[scheme].input_activations.symmetric
    assert (qe.num_experts, qe.hidden_dim, qe.intermediate_dim) == (E, H, I)
    int4 = PRESET_SCHEMES[scheme].weights.num_bits == 4
    assert qe.int4 == int4
    shapes = {"gate_up": (E, 2 * I, (H + 7) // 8 if int4 else H), "down": (E, H, (I + 7) // 8 if int4 else I)}
    for part, proj, K in (("gate_up", "gate_up_proj", H), ("down", "down_proj", I)):
        w = getattr(qe, part)
        s = getattr(qe, f"{part}_scale")
        ws = getattr(qe, f"{part}_wsum")
        assert tuple(w.shape) == shapes[part] and w.dtype == (torch.int32 if int4 else torch.int8)
        G = s.shape[2]
        assert s.dtype == torch.float32 and ws.dtype == torch.int32 and ws.shape == s.shape
        for e in range(E):
            q, t = experts[(e, proj)]
            stored = unpack_int4(w[e], K) if int4 else w[e]
            assert torch.equal(stored, q)              # gate rows then up rows: the fused matrix again
            assert torch.equal(s[e], t["weight_scale"].float())
            qp = torch.nn.functional.pad(q.int(), (0, G * 128 - K)) if G > 1 else q.int()
            assert torch.equal(ws[e], qp.reshape(q.shape[0], G, -1).sum(-1))
    assert qe.act_fn.__class__ is ref.model.layers[0].mlp.experts.act_fn.__class__
    for name in attn:
        assert isinstance(model.get_submodule(name), QuantizedLinear)
    assert torch.equal(model.model.layers[0].mlp.gate.weight, ref.model.layers[0].mlp.gate.weight)


def test_a8_expert_refusals(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    d = tmp_path / "gidx"
    _write(d, "W4A8", g_idx=True)
    with pytest.raises(NotImplementedError, match="weight_g_idx"):
        load_quantized(d, device="cpu")
    d = tmp_path / "zp"
    _write(d, "W8A8", zero_point=True, quantize_attn=False)
    with pytest.raises(ValueError, match="weight_zero_point"):
        load_quantized(d, device="cpu")


@pytest.mark.parametrize("scheme", ["W4A16", "W8A8"])
def test_bank_refusals(tmp_path, scheme):
    from quantool_amd.engine.qlinear import load_quantized

    d = tmp_path / "missing"
    _write(d, scheme, drop=_ckpt_name(3, "w2") + ".")
    with pytest.raises(ValueError, match="missing from the checkpoint"):
        load_quantized(d, device="cpu")
    d = tmp_path / "partly"
    _write(d, scheme, dense_expert=(1, "down_proj"))
    with pytest.raises(ValueError, match="partly quantized"):
        load_quantized(d, device="cpu")
    d = tmp_path / "bias"
    _write(d, scheme, bias=True)
    with pytest.raises(NotImplementedError, match="bias"):
        load_quantized(d, device="cpu")


def test_experts_without_a_fused_bank_are_still_refused(tmp_path):
    """A dense Llama has no bank at ``mlp.experts``: per-expert names there stay a routed-expert refusal."""
    from transformers import LlamaConfig, LlamaForCausalLM

    from quantool_amd.engine.qlinear import load_quantized

    cfg = LlamaConfig(hidden_size=256, intermediate_size=384, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=320, max_position_embeddings=64, tie_word_embeddings=False)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    state = dict(model.state_dict())
    del state["model.layers.0.mlp.gate_proj.weight"]
    wa = PRESET_SCHEMES["W8A16"].weights
    _, t = _qtensors(384, 256, wa, torch.Generator().manual_seed(1))
    for k, v in t.items():
        state[f"model.layers.0.mlp.experts.0.gate_proj.{k}"] = v
    save_state(state, quantization_config(wa.to_config(), "pack-quantized", ["lm_head"], None), tmp_path,
               model.config.to_dict())
    with pytest.raises(NotImplementedError, match="routed-expert"):
        load_quantized(tmp_path, device="cpu")
    assert isinstance(model.model.layers[0].mlp.gate_proj, nn.Linear)
