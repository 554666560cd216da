"""AWQ mapping resolver on a sparse-MoE layer (host logic, no GPU): with an unfused expert bank and the default
table the mappings come from the layer's structure -- the two attention mappings, one bank mapping (norm -> every
expert's gate_up_proj, parent = the MoE block, router scale-only) and one up -> down mapping per expert
(DESIGN.md 4.4)."""
import torch

from quantool_amd.engine.awq_module import normalise_mappings, resolve_mappings
from quantool_amd.engine.modifiers import AWQModifier
from quantool_amd.engine.sequential import unfuse_expert_banks

H, I, E = 256, 256, 4
L0 = "model.layers.0"
BANK = f"{L0}.mlp.experts"


def _mixtral_layer(kv_heads=2):
    from transformers import MixtralConfig, MixtralForCausalLM

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=1, num_attention_heads=4,
                        num_key_value_heads=kv_heads, num_local_experts=E, num_experts_per_tok=2, vocab_size=64,
                        max_position_embeddings=32, tie_word_embeddings=False)
    torch.manual_seed(0)
    model = MixtralForCausalLM(cfg)
    assert unfuse_expert_banks(model) == 1
    return model.model.layers[0]


def _resolve(layer, modifier=None):
    return resolve_mappings(layer, L0, normalise_mappings(None), (modifier or AWQModifier()).wants)


def test_unfused_layer_resolves_attention_bank_and_per_expert_mappings():
    layer = _mixtral_layer(kv_heads=4)          # MHA: v -> o applies
    got = _resolve(layer)
    assert len(got) == 2 + 1 + E
    assert [(m.smooth_name, m.balance_names, m.parent_name) for m in got[:2]] == [
        (f"{L0}.input_layernorm", [f"{L0}.self_attn.{p}_proj" for p in "qkv"], f"{L0}.self_attn"),
        (f"{L0}.self_attn.v_proj", [f"{L0}.self_attn.o_proj"], f"{L0}.self_attn.o_proj"),
    ]
    assert all(not m.scale_only and m.smooth_rows is None and not m.stats_at_parent for m in got[:2])

    bank = got[2]
    assert bank.smooth is layer.post_attention_layernorm and bank.smooth_rows is None
    assert type(bank.parent).__name__ == "MixtralSparseMoeBlock" and bank.parent is layer.mlp
    assert bank.parent_name == f"{L0}.mlp" and not bank.single and bank.stats_at_parent
    assert bank.balance_names == [f"{BANK}.experts.{e}.gate_up_proj" for e in range(E)]
    assert all(b is layer.mlp.experts.experts[e].gate_up_proj for e, b in enumerate(bank.balance))
    assert bank.scale_only_names == [f"{L0}.mlp.gate"] and bank.scale_only == [layer.mlp.gate]
    assert layer.mlp.gate not in bank.balance

    for e, m in enumerate(got[3:]):
        blk = layer.mlp.experts.experts[e]
        assert m.smooth is blk.gate_up_proj and m.smooth_rows == (I, 2 * I)
        assert m.balance == [blk.down_proj] and m.parent is blk.down_proj and m.single
        assert m.balance_names == [f"{BANK}.experts.{e}.down_proj"] and not m.scale_only


def test_gqa_drops_v_to_o_only():
    got = _resolve(_mixtral_layer(kv_heads=2))
    assert len(got) == 1 + 1 + E and got[0].smooth_name.endswith("input_layernorm") and got[1].stats_at_parent


def test_extra_consumer_of_the_block_input_drops_the_bank_mapping():
    layer = _mixtral_layer(kv_heads=4)
    layer.mlp.shared_gate = torch.nn.Linear(H, 1, bias=False)       # a second reader of the block input
    got = _resolve(layer)
    assert len(got) == 2 + E
    assert not any(m.scale_only or m.stats_at_parent for m in got)
    assert [m.smooth_rows for m in got[2:]] == [(I, 2 * I)] * E


def test_ignored_expert_linear_drops_only_the_mappings_that_balance_it():
    layer = _mixtral_layer(kv_heads=4)
    got = _resolve(layer, AWQModifier(ignore=["lm_head", f"{BANK}.experts.2.down_proj"]))
    assert len(got) == 2 + 1 + (E - 1) and got[2].stats_at_parent
    assert [m.balance_names[0] for m in got[3:]] == [f"{BANK}.experts.{e}.down_proj" for e in (0, 1, 3)]
    got = _resolve(layer, AWQModifier(ignore=["lm_head", f"{BANK}.experts.1.gate_up_proj"]))
    assert len(got) == 2 + E and not any(m.stats_at_parent for m in got)
    assert [m.smooth_rows for m in got[2:]] == [(I, 2 * I)] * E


def test_user_mappings_pair_each_smooth_hit_with_the_balance_hits_beside_it():
    """Names are matched as they are: a smooth pattern that hits every expert is paired per expert.  The fused
    gate_up_proj is 2I wide, so the width check drops up -> down here; a pattern over modules of equal width
    shows the pairing."""
    layer = _mixtral_layer(kv_heads=4)
    for blk in layer.mlp.experts.experts:
        blk.pre = torch.nn.Linear(I, I, bias=False)
    spec = [["re:.*experts\\.\\d+\\.pre$", ["re:.*down_proj$"]]]
    got = resolve_mappings(layer, L0, normalise_mappings(spec), AWQModifier(mappings=spec).wants)
    assert [(m.smooth_name, m.balance_names) for m in got] == [
        (f"{BANK}.experts.{e}.pre", [f"{BANK}.experts.{e}.down_proj"]) for e in range(E)]
    spec = [["re:.*gate_up_proj$", ["re:.*down_proj$"]]]
    assert resolve_mappings(layer, L0, normalise_mappings(spec), AWQModifier(mappings=spec).wants) == []


def test_llama_layer_resolves_as_before():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=4, vocab_size=64, max_position_embeddings=32)
    torch.manual_seed(0)
    layer = LlamaForCausalLM(cfg).model.layers[0]
    got = _resolve(layer)
    assert [(m.smooth_name.split(".")[-1], [b.split(".")[-1] for b in m.balance_names], m.parent_name) for m in got] == [
        ("input_layernorm", ["q_proj", "k_proj", "v_proj"], f"{L0}.self_attn"),
        ("v_proj", ["o_proj"], f"{L0}.self_attn.o_proj"),
        ("post_attention_layernorm", ["gate_proj", "up_proj"], f"{L0}.mlp"),
        ("up_proj", ["down_proj"], f"{L0}.mlp.down_proj"),
    ]
    assert all(not m.scale_only and m.smooth_rows is None and not m.stats_at_parent for m in got)
