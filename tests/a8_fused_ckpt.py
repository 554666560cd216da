"""Tiny saved checkpoints for the fused-glue tests (test_a8_fused_act_dispatch.py, test_gpu_a8_fused_act_modules.py):
a two-layer Llama and a one-layer Mixtral with random levels and scales, written as the save path writes them and as the
loader tests build theirs (test_qlinear_loader.py, test_moe_loader.py)."""
import torch

from quantool_amd.engine.schemes import PRESET_SCHEMES
from quantool_amd.engine.serialization import quantization_config, save_state

LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
           "mlp.up_proj", "mlp.down_proj")


def _quantized_leaves(state, name, N, K, wa, g, g_idx=False):
    """The checkpoint leaves of one quantized Linear [N, K] under the weight args ``wa``, random, into ``state``."""
    from quantool_amd.engine.qlinear import pack_int4

    lo, hi = (-8, 8) if wa.num_bits == 4 else (-128, 128)
    q = torch.randint(lo, hi, (N, K), generator=g, dtype=torch.int8)
    G = (K + 127) // 128 if wa.strategy == "group" else 1
    state[f"{name}.weight_scale"] = (torch.rand(N, G, generator=g) * 0.01 + 1e-3).to(torch.bfloat16)
    state[f"{name}.weight_shape"] = torch.tensor([N, K])
    if wa.num_bits == 4:
        state[f"{name}.weight_packed"] = pack_int4(q)
    else:
        state[f"{name}.weight"] = q
    if not wa.symmetric:
        state[f"{name}.weight_zero_point"] = torch.randint(-8, 8, (N, G), generator=g, dtype=torch.int8)
    if g_idx:
        state[f"{name}.weight_g_idx"] = (torch.randperm(K, generator=g) // 128).to(torch.int32)


def write_llama(path, scheme_name, layers=2, g_idx=False, bias=False):
    """A tiny two-layer Llama checkpoint (hidden 256, intermediate 384) under ``scheme_name`` with random levels and
    scales, written as the save path writes it.  With ``g_idx`` every Linear draws its own actorder grouping."""
    from transformers import LlamaConfig, LlamaForCausalLM

    scheme = PRESET_SCHEMES[scheme_name]
    wa = scheme.weights
    cfg = LlamaConfig(hidden_size=256, intermediate_size=384, num_hidden_layers=layers, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=320, max_position_embeddings=64, tie_word_embeddings=False,
                      mlp_bias=bias)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    state = dict(model.state_dict())
    g = torch.Generator().manual_seed(3)
    for layer in range(layers):
        for lin in LINEARS:
            name = f"model.layers.{layer}.{lin}"
            N, K = model.get_submodule(name).weight.shape
            del state[f"{name}.weight"]
            _quantized_leaves(state, name, N, K, wa, g, g_idx=g_idx)
    acts = scheme.input_activations.to_config() if scheme.input_activations is not None else None
    save_state(state, quantization_config(wa.to_config(), scheme.format, ["lm_head"], acts), path,
               model.config.to_dict())
    return path


MIXTRAL_BANK = "model.layers.0.mlp.experts"


def write_mixtral(path, scheme_name, experts=4, hidden=256, intermediate=384):
    """A tiny one-layer Mixtral checkpoint under ``scheme_name``: every expert's fused gate_up [2I, H] and down [H, I]
    and the attention Linears quantized with random levels, the bank renamed per expert by
    ``expert_bank_checkpoint_names`` (``block_sparse_moe.experts.{e}.w1 / w3 / w2``)."""
    from transformers import MixtralConfig, MixtralForCausalLM

    from quantool_amd.engine.sequential import expert_bank_checkpoint_names

    scheme = PRESET_SCHEMES[scheme_name]
    wa = scheme.weights
    cfg = MixtralConfig(hidden_size=hidden, intermediate_size=intermediate, num_hidden_layers=1, num_attention_heads=4,
                        num_key_value_heads=2, num_local_experts=experts, num_experts_per_tok=2, vocab_size=320,
                        max_position_embeddings=64, tie_word_embeddings=False)
    torch.manual_seed(0)
    model = MixtralForCausalLM(cfg).to(torch.bfloat16)
    state = dict(model.state_dict())
    del state[f"{MIXTRAL_BANK}.gate_up_proj"], state[f"{MIXTRAL_BANK}.down_proj"]
    g = torch.Generator().manual_seed(3)
    names = [(f"{MIXTRAL_BANK}.experts.{e}.{proj}", shape) for e in range(experts)
             for proj, shape in (("gate_up_proj", (2 * intermediate, hidden)), ("down_proj", (hidden, intermediate)))]
    for lin in LINEARS[:4]:
        name = f"model.layers.0.{lin}"
        names.append((name, tuple(model.get_submodule(name).weight.shape)))
        del state[f"{name}.weight"]
    for name, (N, K) in names:
        _quantized_leaves(state, name, N, K, wa, g)
    state = expert_bank_checkpoint_names(state, {MIXTRAL_BANK: None}, "mixtral")
    acts = scheme.input_activations.to_config() if scheme.input_activations is not None else None
    ignore = ["lm_head", "model.layers.0.block_sparse_moe.gate"]
    save_state(state, quantization_config(wa.to_config(), scheme.format, ignore, acts), path, model.config.to_dict())
    return path
