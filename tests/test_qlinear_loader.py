"""CPU side of the A8 runtime: ``perplexity`` on stub models, and ``load_quantized`` on tiny Llama checkpoints written
with ``save_state`` -- the A16 dequantisation, the A8 ``QuantizedLinear`` buffers, and the refusals.  No GPU call."""
import math

import pytest
import torch
import torch.nn as nn

from quantool_amd.engine.schemes import PRESET_SCHEMES
from quantool_amd.engine.serialization import quantization_config, save_state

LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
           "mlp.up_proj", "mlp.down_proj")


# ---- perplexity -----------------------------------------------------------------------------------------------------
class _Fixed(nn.Module):
    """Logits of token position t: table[ids[t]] (a bigram model with known log-probabilities)."""

    def __init__(self, table):
        super().__init__()
        self.table = nn.Parameter(table, requires_grad=False)

    def forward(self, input_ids):
        return self.table[input_ids]


def test_uniform_logits_give_the_vocabulary_size():
    from quantool_amd.evaluate import perplexity

    V = 512
    model = _Fixed(torch.zeros(V, V))
    ids = torch.randint(0, V, (3, 17), generator=torch.Generator().manual_seed(0))
    r = perplexity(model, ids, batch_size=2)
    assert r["tokens"] == 3 * 16
    # exp of the fp32 log(V) that log_softmax returns: V up to fp32 rounding of log V
    assert r["perplexity"] == pytest.approx(V, rel=1e-6)


def test_known_logits_match_a_hand_computation_and_do_not_depend_on_batching():
    from quantool_amd.evaluate import perplexity

    V = 7
    g = torch.Generator().manual_seed(1)
    table = torch.randn(V, V, generator=g) * 3
    model = _Fixed(table)
    seqs = [torch.randint(0, V, (n,), generator=g) for n in (9, 9, 9, 5, 12, 12)]
    nll = 0.0
    n = 0
    for s in seqs:
        for a, b in zip(s[:-1].tolist(), s[1:].tolist()):
            row = table[a].double()
            nll += float(torch.logsumexp(row, 0) - row[b])
            n += 1
    want = math.exp(nll / n)
    results = [perplexity(model, seqs, batch_size=bs, chunk_rows=cr) for bs in (1, 2, 8) for cr in (1, 3, 1024)]
    for r in results:
        assert r["tokens"] == n
        assert r["perplexity"] == pytest.approx(want, rel=1e-6)
        assert r["perplexity"] == pytest.approx(results[0]["perplexity"], rel=1e-12)
    # a [B, T] tensor is the same as its rows
    same = torch.stack(seqs[:3])
    assert perplexity(model, same)["perplexity"] == pytest.approx(perplexity(model, seqs[:3])["perplexity"], rel=1e-12)


def test_dataset_ids_are_refused():
    from quantool_amd.evaluate import perplexity

    with pytest.raises(ValueError, match="dataset id"):
        perplexity(_Fixed(torch.zeros(4, 4)), dataset="wikitext/wikitext-2-raw-v1", tokenizer=object())


# ---- checkpoints ----------------------------------------------------------------------------------------------------
def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=256, intermediate_size=384, num_hidden_layers=1, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=320, max_position_embeddings=64, tie_word_embeddings=False)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).to(torch.bfloat16)


def _pack(q):
    from quantool_amd.engine.qlinear import pack_int4

    return pack_int4(q)


def _write(tmp_path, scheme_name, *, g_idx=False, zero_point=False, acts_override=None, rename=None, fmt=None):
    """A checkpoint of the tiny Llama under ``scheme_name`` with random levels / scales; returns (dir, model, levels)."""
    scheme = PRESET_SCHEMES[scheme_name]
    wa = scheme.weights
    model = _tiny_llama()
    state = dict(model.state_dict())
    levels = {}
    g = torch.Generator().manual_seed(3)
    for i, (name, lin) in enumerate((f"model.layers.0.{l}", model.model.layers[0].get_submodule(l)) for l in LINEARS):
        N, K = lin.weight.shape
        del state[f"{name}.weight"]
        lo, hi = (-8, 8) if wa.num_bits == 4 else (-128, 128)
        q = torch.randint(lo, hi, (N, K), generator=g, dtype=torch.int8)
        G = K // 128 if wa.strategy == "group" else 1
        scale = (torch.rand(N, G, generator=g) * 0.01 + 1e-3).to(torch.bfloat16)
        t = {"weight_scale": scale, "weight_shape": torch.tensor([N, K])}
        if wa.num_bits == 4:
            t["weight_packed"] = _pack(q)
        else:
            t["weight"] = q
        if zero_point or not wa.symmetric:
            t["weight_zero_point"] = torch.randint(-8, 8, (N, G), generator=g, dtype=torch.int8)
        if g_idx:
            t["weight_g_idx"] = (torch.randperm(K, generator=g) // 128).to(torch.int32)
        for k, v in t.items():
            state[f"{name}.{k}"] = v
        levels[name] = (q, t)
    if rename:
        state = {rename(k): v for k, v in state.items()}
    acts = scheme.input_activations.to_config() if scheme.input_activations is not None else None
    if acts_override is not None:
        acts = acts_override
    qcfg = quantization_config(wa.to_config(), fmt or scheme.format, ["lm_head"], acts)
    base = model.config.to_dict()
    save_state(state, qcfg, tmp_path, base)
    return tmp_path, model, levels


@pytest.mark.parametrize("scheme", ["W4A16", "W4A16_ASYM", "W8A16"])
def test_a16_checkpoint_gives_dequantized_linears(tmp_path, scheme):
    from quantool_amd.engine.qlinear import QuantizedLinear, load_quantized

    path, ref, levels = _write(tmp_path, scheme, g_idx=scheme == "W4A16")
    model = load_quantized(path, device="cpu")
    assert not any(isinstance(m, QuantizedLinear) for m in model.modules())
    for name, (q, t) in levels.items():
        lin = model.get_submodule(name)
        assert type(lin) is nn.Linear and lin.weight.dtype == torch.bfloat16
        K = q.shape[1]
        G = t["weight_scale"].shape[1]
        gcol = t["weight_g_idx"].long() if "weight_g_idx" in t else (torch.arange(K) // 128 if G > 1 else
                                                                      torch.zeros(K, dtype=torch.long))
        w = q.float()
        if "weight_zero_point" in t:
            w = w - t["weight_zero_point"].float()[:, gcol]
        want = (w * t["weight_scale"].float()[:, gcol]).to(torch.bfloat16)
        assert torch.equal(lin.weight.data, want), name
    # the dense tensors came through
    assert torch.equal(model.model.embed_tokens.weight, ref.model.embed_tokens.weight)
    assert torch.equal(model.lm_head.weight, ref.lm_head.weight)
    with torch.no_grad():
        assert torch.isfinite(model(input_ids=torch.tensor([[1, 2, 3]])).logits.float()).all()


@pytest.mark.parametrize("scheme,g_idx", [("W8A8", False), ("INT8", False), ("W4A8", False), ("W4A8", True)])
def test_a8_checkpoint_gives_quantized_linears(tmp_path, scheme, g_idx):
    from quantool_amd.engine.qlinear import QuantizedLinear, load_quantized, unpack_int4

    path, _, levels = _write(tmp_path, scheme, g_idx=g_idx)
    model = load_quantized(path, device="cpu")
    sym = PRESET_SCHEMES[scheme].input_activations.symmetric
    for name, (q, t) in levels.items():
        ql = model.get_submodule(name)
        assert isinstance(ql, QuantizedLinear), name
        N, K = q.shape
        assert (ql.out_features, ql.in_features) == (N, K)
        assert ql.act_symmetric == sym
        assert ql.weight_scale.dtype == torch.float32
        assert torch.equal(ql.weight_scale, t["weight_scale"].float())
        G = ql.weight_scale.shape[1]
        if g_idx:
            perm = torch.argsort(t["weight_g_idx"].long(), stable=True)
            assert torch.equal(ql.col_perm.long(), perm)
            qp = q[:, perm]
        else:
            assert ql.col_perm is None
            qp = q
        stored = unpack_int4(ql.weight, K) if ql.int4 else ql.weight
        assert torch.equal(stored, qp)
        want = qp.int().reshape(N, G, K // G).sum(-1)
        assert ql.wsum.dtype == torch.int32 and torch.equal(ql.wsum, want)


def test_int4_pack_roundtrip_matches_the_checkpoint_layout():
    from quantool_amd.engine.qlinear import pack_int4, unpack_int4

    q = torch.randint(-8, 8, (5, 45), generator=torch.Generator().manual_seed(4), dtype=torch.int8)
    p = pack_int4(q)
    assert p.shape == (5, 6) and p.dtype == torch.int32
    # nibble j of word w is column 8w + j, stored + 8
    assert int(p[2, 1]) & 0xF == int(q[2, 8]) + 8 and (int(p[2, 1]) >> 28) & 0xF == int(q[2, 15]) + 8
    assert torch.equal(unpack_int4(p, 45), q)


def test_refusals(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    d = tmp_path / "experts"
    _write(d, "W4A16", rename=lambda k: k.replace("mlp.gate_proj", "mlp.experts.0.gate_proj"))
    with pytest.raises(NotImplementedError, match="routed-expert"):
        load_quantized(d, device="cpu")
    d = tmp_path / "float"
    _write(d, "W8A16", fmt="float-quantized")
    with pytest.raises(NotImplementedError, match="float preset"):
        load_quantized(d, device="cpu")
    d = tmp_path / "static"
    acts = dict(PRESET_SCHEMES["W8A8"].input_activations.to_config(), dynamic=False, strategy="tensor")
    _write(d, "W8A8", acts_override=acts)
    with pytest.raises(NotImplementedError, match="input_activations"):
        load_quantized(d, device="cpu")
    d = tmp_path / "zp"
    _write(d, "W8A8", zero_point=True)
    with pytest.raises(ValueError, match="weight_zero_point"):
        load_quantized(d, device="cpu")


def test_unexpected_tensors_are_refused(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    _write(tmp_path, "W8A16", rename=lambda k: k.replace("input_layernorm", "input_layer_norm"))
    with pytest.raises(ValueError, match="unexpected tensors"):
        load_quantized(tmp_path, device="cpu")
