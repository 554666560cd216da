"""Batch-1 greedy decoding of a W4A16 g128 checkpoint, loaded dequantised and packed.

  python tools/decode_bench.py <checkpoint dir> [--layers 32] [--prompt 128] [--new 128] [--modes dequantized,packed]
  python tools/decode_bench.py <checkpoint dir> --model mixtral --layers 8 [--modes dequantized,packed,packed_experts]

Writes (once: an existing checkpoint in the directory is reused) a W4A16 g128 checkpoint of a random-init
Llama-3-8B-shaped model: round-to-nearest levels of every decoder Linear, scale = absmax / 7.5 per group of 128 columns
(no calibration: the timing does not depend on the values).  Then, per mode, ``load_quantized(dir, a16=mode)`` and a
KV-cached greedy decode of --new tokens after a --prompt-token prompt.  Prints one JSON line: per mode ms per generated
token (the decode steps after the prompt, wall time with the device synchronised), the resident bytes of the decoder
Linears, ``memory_allocated`` after loading and ``max_memory_allocated`` during the decode; and how many generated tokens
agree between the modes (and the first position where they differ).

``--model mixtral``: a Mixtral-8x7B-shaped model instead (8 experts, top-2, H = 4096, I = 14336; ``--layers 8`` keeps
the write and the three loads short).  Every expert's gate / up / down and the attention Linears are quantised the same
way and written per expert through ``expert_bank_checkpoint_names`` (``block_sparse_moe.experts.{e}.w1 / w3 / w2``).
``--scheme W4A16 --batch B --modes packed,packed_stream`` compares the packed runtime with and without
``a16_stream_rows=128`` (B rows per decode-step GEMM: ``qt_gemm_wq_stream`` against dequantise + ``F.linear``), each mode
decoded twice.

Modes ``dequantized``, ``packed`` (``a16="packed"``: the banks stay dense bf16) and ``packed_experts`` (``a16="packed",
a16_experts="packed"``: ``WeightOnlyExperts``); each mode also reports the resident bytes of the expert banks.

  python tools/decode_bench.py <checkpoint dir> --scheme W8A8 [--model mixtral --layers 8]      # or --scheme W4A8

An A8 checkpoint instead (W8A8: int8 levels, one scale per row = absmax / 127.5, symmetric activations; W4A8: int4
g128 with asymmetric activations; both round-to-nearest), loaded once and decoded in two modes in the same process:
``a8_tiled`` (``QuantizedLinear.skinny_max_m`` and ``QuantizedExperts.grouped_max_tokens`` set to 0: every Linear on
the 128 x 128-tile ``qt_gemm_i8``) and ``a8_skinny`` (the class defaults: the decode GEMV).  The two compute the same
bits, so ``tokens_agree`` must equal --new (B x --new with ``--batch B``).

  python tools/decode_bench.py <checkpoint dir> --scheme W4A8 --layers 8 --batch 32 --pair mid

``--batch B`` (default 1) decodes B sequences at once (B random prompts of --prompt tokens): every decode step is a
B-row GEMM per Linear, and in every scheme and mode (the W4A16 ones included) ``tokens_agree``, ``first_difference``
and ``tokens_agree_with_dequantized`` count over all B x --new generated tokens, sequence by sequence.
``--pair mid`` (A8 schemes) replaces the mode pair by one that differs only in ``QuantizedLinear.mid_max_m``:
``a8_mid_off`` (0: rows 17 .. 128 on the tiled ``qt_gemm_i8``) against ``a8_mid`` (the class default:
``qt_gemm_i8_mid``); everything else stays at its default in both.  ``--pair wide`` (A8 schemes, ``--model mixtral``)
likewise differs only in ``QuantizedExperts.wide_max_rows_per_expert`` / ``wide_w4_max_rows_per_expert`` /
``wide_max_n``: ``a8_wide_off`` (all 0: the banks' products past the decode range on the tiled ``qt_gemm_i8_grouped``)
against ``a8_wide`` (the class defaults: ``qt_moe_gemm_i8_wide``).  ``--pair fused`` (A8 schemes, either model) loads
the checkpoint twice, ``a8_fused_off`` with the default loader and ``a8_fused`` with ``a8_fused_act=True`` (every
``QuantizedExperts`` with ``fused_act``, every dense MLP a ``QuantizedMLP``: SiLU(gate) * up and the quantiser in one
``qt_act_mul_quantize_i8`` pass); the prompt's logits are asserted equal to the bit before anything is timed.
``--pair norm`` (A8 schemes) loads it twice with ``a8_fused_act=True``, ``a8_norm_off`` without and ``a8_norm`` with
``a8_fused_norm=True`` (the RMSNorms in front of q/k/v and gate/up as ``QuantizingRMSNorm``s: the norm and the
quantiser its consumers share in one ``qt_rmsnorm_quantize_i8`` pass).  The kernel's sum over K runs in its own order,
so nothing is asserted of the logits: how many of the prompt's differ, and by how much at most, is reported
(``logits_differ``, ``logits_max_abs_diff``) beside ``quantizing_norms``.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantool_amd.engine.qlinear import (A16_MODES, WeightOnlyExperts, WeightOnlyLinear, load_quantized,  # noqa: E402
                                         pack_int4)
from quantool_amd.engine.schemes import PRESET_SCHEMES  # noqa: E402
from quantool_amd.engine.serialization import quantization_config, save_state  # noqa: E402

LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
           "mlp.up_proj", "mlp.down_proj")


def _rtn(W: torch.Tensor, scheme: str = "W4A16"):
    """Round-to-nearest int4 g128 of W [N, K]: (packed int32 [N, K/8], bf16 scales [N, K/128]) on the CPU; for W8A8,
    int8 levels [N, K] and one scale per row."""
    W = W.float()
    N, K = W.shape
    if scheme == "W8A8":
        s = (W.abs().amax(-1, keepdim=True) / 127.5).clamp(min=1e-8).to(torch.bfloat16)
        return torch.round(W / s.float()).clamp(-128, 127).to(torch.int8).cpu(), s.cpu()
    s = (W.reshape(N, K // 128, 128).abs().amax(-1) / 7.5).clamp(min=1e-8).to(torch.bfloat16)
    q = torch.round(W.reshape(N, K // 128, 128) / s.float()[..., None]).clamp(-8, 7).reshape(N, K).to(torch.int8)
    return pack_int4(q).cpu(), s.cpu()


def _leaves(state: dict, pre: str, W: torch.Tensor, scheme: str) -> None:
    q, s = _rtn(W, scheme)
    state[f"{pre}.weight" if scheme == "W8A8" else f"{pre}.weight_packed"], state[f"{pre}.weight_scale"] = q, s
    state[f"{pre}.weight_shape"] = torch.tensor(list(W.shape))


def _qconfig(scheme: str, ignore):
    wa = PRESET_SCHEMES[scheme]
    acts = None if wa.input_activations is None else wa.input_activations.to_config()
    return quantization_config(wa.weights.to_config(), wa.format, ignore, acts)


def write_mixtral_checkpoint(path: Path, layers: int, dev, scheme: str = "W4A16") -> None:
    from transformers import MixtralConfig, MixtralForCausalLM

    from quantool_amd.engine.sequential import expert_bank_checkpoint_names

    cfg = MixtralConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers, num_attention_heads=32,
                        num_key_value_heads=8, num_local_experts=8, num_experts_per_tok=2, vocab_size=32000,
                        max_position_embeddings=8192, rope_theta=1e6, tie_word_embeddings=False)
    torch.manual_seed(0)
    with dev:
        model = MixtralForCausalLM(cfg).to(torch.bfloat16)
    attn = {f"model.layers.{i}.{l}" for i in range(layers) for l in LINEARS[:4]}
    banks = {f"model.layers.{i}.mlp.experts": None for i in range(layers)}
    state = {}
    for k, v in model.state_dict().items():
        mod, _, leaf = k.rpartition(".")
        if mod in banks:                                   # the fused bank, per expert as the save path holds it
            proj = leaf
            for e in range(v.shape[0]):
                _leaves(state, f"{mod}.experts.{e}.{proj}", v[e], scheme)
        elif mod in attn:
            _leaves(state, mod, v, scheme)
        else:
            state[k] = v.cpu()
    state = expert_bank_checkpoint_names(state, banks, "mixtral")
    ignore = ["lm_head"] + [f"model.layers.{i}.block_sparse_moe.gate" for i in range(layers)]
    save_state(state, _qconfig(scheme, ignore), path, model.config.to_dict())
    del model, state
    torch.cuda.empty_cache()


def write_checkpoint(path: Path, layers: int, dev, scheme: str = "W4A16") -> None:
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=4096, intermediate_size=14336, num_hidden_layers=layers, num_attention_heads=32,
                      num_key_value_heads=8, vocab_size=128256, max_position_embeddings=8192, rope_theta=500000.0,
                      tie_word_embeddings=False)
    torch.manual_seed(0)
    with dev:
        model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    state = {}
    quantized = {f"model.layers.{i}.{l}" for i in range(layers) for l in LINEARS}
    for k, v in model.state_dict().items():
        mod = k.rpartition(".")[0]
        if mod not in quantized:
            state[k] = v.cpu()
            continue
        _leaves(state, mod, v, scheme)
    save_state(state, _qconfig(scheme, ["lm_head"]), path, model.config.to_dict())
    del model, state
    torch.cuda.empty_cache()


def decode(model, prompt: torch.Tensor, new: int):
    """Greedy tokens and the wall time of the decode steps after the prompt."""
    with torch.no_grad():
        out = model(input_ids=prompt, use_cache=True)
        past = out.past_key_values
        tok = out.logits[:, -1].argmax(-1, keepdim=True)
        toks = [tok]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(new - 1):
            out = model(input_ids=tok, past_key_values=past, use_cache=True)
            past = out.past_key_values
            tok = out.logits[:, -1].argmax(-1, keepdim=True)
            toks.append(tok)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
    return torch.cat(toks, 1).flatten().tolist(), (t1 - t0) / max(new - 1, 1)


def a8_mid_modes(path: Path, dev, prompt: torch.Tensor, new: int, result: dict) -> None:
    """One loaded A8 model decoded as ``a8_mid_off`` (``mid_max_m`` = 0) and ``a8_mid`` (its default)."""
    from quantool_amd.engine.qlinear import QuantizedLinear

    model = load_quantized(path, device=dev)
    default = QuantizedLinear.mid_max_m
    for name in ("skinny_max_m", "mid_max_m", "mid_max_n", "mid_min_k", "ring_min_m"):
        result[name] = getattr(QuantizedLinear, name)
    result["quantized_linears"] = sum(isinstance(m, QuantizedLinear) for m in model.modules())
    tokens = {}
    for rep in range(2):                                       # both modes twice: the second pass is the spread
        for mode, a in (("a8_mid_off", 0), ("a8_mid", default)):
            QuantizedLinear.mid_max_m = a
            decode(model, prompt[:, :8], 4)                    # warm-up: kernels, allocator
            toks, per_tok = decode(model, prompt, new)
            result["modes"].setdefault(mode, {"ms_per_step": []})["ms_per_step"].append(round(per_tok * 1e3, 3))
            assert tokens.setdefault(mode, toks) == toks, f"{mode}: two runs gave different tokens"
    QuantizedLinear.mid_max_m = default
    same = [x == y for x, y in zip(tokens["a8_mid_off"], tokens["a8_mid"])]
    result["tokens_agree"] = sum(same)
    result["first_difference"] = same.index(False) if not all(same) else None
    t, k = (min(result["modes"][m]["ms_per_step"]) for m in ("a8_mid_off", "a8_mid"))
    result["speedup"] = round(t / k, 3)


def a8_wide_modes(path: Path, dev, prompt: torch.Tensor, new: int, result: dict) -> None:
    """One loaded A8 sparse-MoE model decoded as ``a8_wide_off`` (``QuantizedExperts``' three wide attributes 0) and
    ``a8_wide`` (their defaults)."""
    from quantool_amd.engine.qlinear import QuantizedExperts

    names = ("wide_max_rows_per_expert", "wide_w4_max_rows_per_expert", "wide_max_n")
    model = load_quantized(path, device=dev)
    defaults = {n: getattr(QuantizedExperts, n) for n in names}
    result.update(defaults, wide_min_k=QuantizedExperts.wide_min_k, grouped_max_tokens=QuantizedExperts.grouped_max_tokens)
    result["quantized_expert_banks"] = sum(isinstance(m, QuantizedExperts) for m in model.modules())
    tokens = {}
    for rep in range(2):                                       # both modes twice: the second pass is the spread
        for mode, values in (("a8_wide_off", dict.fromkeys(names, 0)), ("a8_wide", defaults)):
            for n, v in values.items():
                setattr(QuantizedExperts, n, v)
            decode(model, prompt[:, :8], 4)                    # warm-up: kernels, allocator
            toks, per_tok = decode(model, prompt, new)
            result["modes"].setdefault(mode, {"ms_per_step": []})["ms_per_step"].append(round(per_tok * 1e3, 3))
            assert tokens.setdefault(mode, toks) == toks, f"{mode}: two runs gave different tokens"
    for n, v in defaults.items():
        setattr(QuantizedExperts, n, v)
    same = [x == y for x, y in zip(tokens["a8_wide_off"], tokens["a8_wide"])]
    result["tokens_agree"] = sum(same)
    result["first_difference"] = same.index(False) if not all(same) else None
    t, k = (min(result["modes"][m]["ms_per_step"]) for m in ("a8_wide_off", "a8_wide"))
    result["speedup"] = round(t / k, 3)


def a8_fused_modes(path: Path, dev, prompt: torch.Tensor, new: int, result: dict) -> None:
    """The A8 checkpoint loaded as ``a8_fused_off`` (the default loader) and as ``a8_fused`` (``a8_fused_act=True``),
    decoded in turn."""
    from quantool_amd.engine.qlinear import QuantizedExperts, QuantizedMLP

    models = {"a8_fused_off": load_quantized(path, device=dev),
              "a8_fused": load_quantized(path, device=dev, a8_fused_act=True)}
    fused = models["a8_fused"]
    result["quantized_mlps"] = sum(isinstance(m, QuantizedMLP) for m in fused.modules())
    result["fused_expert_banks"] = sum(isinstance(m, QuantizedExperts) and m.fused_act for m in fused.modules())
    assert result["quantized_mlps"] + result["fused_expert_banks"] > 0, "nothing in this checkpoint runs fused"
    with torch.no_grad():
        a, b = (m(input_ids=prompt).logits for m in models.values())
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "the prompt's logits differ with a8_fused_act"
    result["logits_bits_equal"] = True
    del a, b
    tokens = {}
    for rep in range(2):                                       # both modes twice: the second pass is the spread
        for mode, model in models.items():
            decode(model, prompt[:, :8], 4)                    # warm-up: kernels, allocator
            toks, per_tok = decode(model, prompt, new)
            result["modes"].setdefault(mode, {"ms_per_step": []})["ms_per_step"].append(round(per_tok * 1e3, 3))
            assert tokens.setdefault(mode, toks) == toks, f"{mode}: two runs gave different tokens"
    same = [x == y for x, y in zip(tokens["a8_fused_off"], tokens["a8_fused"])]
    result["tokens_agree"] = sum(same)
    result["first_difference"] = same.index(False) if not all(same) else None
    t, k = (min(result["modes"][m]["ms_per_step"]) for m in ("a8_fused_off", "a8_fused"))
    result["speedup"] = round(t / k, 3)


def a8_norm_modes(path: Path, dev, prompt: torch.Tensor, new: int, result: dict) -> None:
    """The A8 checkpoint loaded with ``a8_fused_act=True`` as ``a8_norm_off`` and, with ``a8_fused_norm=True`` besides,
    as ``a8_norm``, decoded in turn."""
    from quantool_amd.engine.qlinear import QuantizedMLP, QuantizingRMSNorm

    models = {"a8_norm_off": load_quantized(path, device=dev, a8_fused_act=True),
              "a8_norm": load_quantized(path, device=dev, a8_fused_act=True, a8_fused_norm=True)}
    fused = models["a8_norm"]
    result["quantized_mlps"] = sum(isinstance(m, QuantizedMLP) for m in fused.modules())
    result["quantizing_norms"] = sum(isinstance(m, QuantizingRMSNorm) for m in fused.modules())
    assert result["quantizing_norms"] > 0, "no norm of this checkpoint runs fused"
    assert not any(isinstance(m, QuantizingRMSNorm) for m in models["a8_norm_off"].modules())
    with torch.no_grad():
        a, b = (m(input_ids=prompt).logits.float() for m in models.values())
    result["logits"] = a.numel()
    result["logits_differ"] = int((a != b).sum())
    result["logits_max_abs_diff"] = float((a - b).abs().max())
    result["logits_max_abs"] = float(a.abs().max())
    result["prompt_argmax_agree"] = int((a.argmax(-1) == b.argmax(-1)).sum())
    result["prompt_positions"] = a.shape[0] * a.shape[1]
    del a, b
    tokens = {}
    for rep in range(2):                                       # both modes twice: the second pass is the spread
        for mode, model in models.items():
            decode(model, prompt[:, :8], 4)                    # warm-up: kernels, allocator
            toks, per_tok = decode(model, prompt, new)
            result["modes"].setdefault(mode, {"ms_per_step": []})["ms_per_step"].append(round(per_tok * 1e3, 3))
            assert tokens.setdefault(mode, toks) == toks, f"{mode}: two runs gave different tokens"
    same = [x == y for x, y in zip(tokens["a8_norm_off"], tokens["a8_norm"])]
    result["tokens_agree"] = sum(same)                         # a random-init model's logits are near ties
    result["first_difference"] = same.index(False) if not all(same) else None
    t, k = (min(result["modes"][m]["ms_per_step"]) for m in ("a8_norm_off", "a8_norm"))
    result["speedup"] = round(t / k, 3)
    off = result["modes"]["a8_norm_off"]["ms_per_step"]
    result["off_spread"] = round(abs(off[0] / off[1] - 1.0), 4)


def a16_wide_modes(path: Path, dev, prompt: torch.Tensor, new: int, wide_min_tokens: int, result: dict) -> None:
    """One packed A16 sparse-MoE model (``a16_experts="packed"``) decoded as ``a16_wide_off`` (``WeightOnlyExperts``'
    ``wide_min_tokens`` = 0: the grouped GEMV) and ``a16_wide`` (``wide_min_tokens`` = the class default, or
    --wide-min-tokens).  The two kernels agree to the bit, so the tokens must."""
    model = load_quantized(path, device=dev, a16="packed", a16_experts="packed")
    default = WeightOnlyExperts.wide_min_tokens
    chosen = default if wide_min_tokens < 0 else wide_min_tokens
    result.update(wide_min_tokens=chosen, wide_min_tokens_default=default,
                  grouped_max_tokens=WeightOnlyExperts.grouped_max_tokens,
                  weight_only_expert_banks=sum(isinstance(m, WeightOnlyExperts) for m in model.modules()))
    tokens = {}
    for rep in range(2):                                       # both modes twice: the second pass is the spread
        for mode, value in (("a16_wide_off", 0), ("a16_wide", chosen)):
            WeightOnlyExperts.wide_min_tokens = value
            decode(model, prompt[:, :8], 4)                    # warm-up: kernels, allocator
            toks, per_tok = decode(model, prompt, new)
            result["modes"].setdefault(mode, {"ms_per_step": []})["ms_per_step"].append(round(per_tok * 1e3, 3))
            assert tokens.setdefault(mode, toks) == toks, f"{mode}: two runs gave different tokens"
    WeightOnlyExperts.wide_min_tokens = default
    same = [x == y for x, y in zip(tokens["a16_wide_off"], tokens["a16_wide"])]
    result["tokens_agree"] = sum(same)
    result["first_difference"] = same.index(False) if not all(same) else None
    t, k = (min(result["modes"][m]["ms_per_step"]) for m in ("a16_wide_off", "a16_wide"))
    result["speedup"] = round(t / k, 3)


def a8_modes(path: Path, dev, prompt: torch.Tensor, new: int, result: dict) -> None:
    """One loaded A8 model decoded as ``a8_tiled`` (class attributes 0) and ``a8_skinny`` (their defaults)."""
    from quantool_amd.engine.qlinear import QuantizedExperts, QuantizedLinear

    model = load_quantized(path, device=dev)
    defaults = (QuantizedLinear.skinny_max_m, QuantizedExperts.grouped_max_tokens)
    result["skinny_max_m"], result["grouped_max_tokens"] = defaults
    result["quantized_linears"] = sum(isinstance(m, QuantizedLinear) for m in model.modules())
    result["quantized_expert_banks"] = sum(isinstance(m, QuantizedExperts) for m in model.modules())
    tokens = {}
    for rep in range(2):                                       # both modes twice: the second pass is the spread
        for mode, (a, b) in (("a8_tiled", (0, 0)), ("a8_skinny", defaults)):
            QuantizedLinear.skinny_max_m, QuantizedExperts.grouped_max_tokens = a, b
            decode(model, prompt[:, :8], 4)                    # warm-up: kernels, allocator
            toks, per_tok = decode(model, prompt, new)
            result["modes"].setdefault(mode, {"ms_per_token": []})["ms_per_token"].append(round(per_tok * 1e3, 3))
            assert tokens.setdefault(mode, toks) == toks, f"{mode}: two runs gave different tokens"
    QuantizedLinear.skinny_max_m, QuantizedExperts.grouped_max_tokens = defaults
    same = [x == y for x, y in zip(tokens["a8_tiled"], tokens["a8_skinny"])]
    result["tokens_agree"] = sum(same)
    result["first_difference"] = same.index(False) if not all(same) else None
    t, k = (min(result["modes"][m]["ms_per_token"]) for m in ("a8_tiled", "a8_skinny"))
    result["speedup"] = round(t / k, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--model", default="llama", choices=["llama", "mixtral"])
    ap.add_argument("--scheme", default="W4A16", choices=["W4A16", "W8A8", "W4A8"],
                    help="W8A8 / W4A8: an A8 checkpoint, decoded as a8_tiled and a8_skinny")
    ap.add_argument("--batch", type=int, default=1, help="sequences decoded at once (rows of every decode-step GEMM)")
    ap.add_argument("--pair", default="skinny", choices=["skinny", "mid", "wide", "fused", "norm"],
                    help="A8 schemes: skinny = a8_tiled vs a8_skinny; mid = a8_mid_off (mid_max_m = 0) vs a8_mid; "
                         "wide = a8_wide_off (QuantizedExperts' wide attributes 0) vs a8_wide; fused = a8_fused_off vs a8_fused "
                         "(load_quantized(..., a8_fused_act=True)); norm = a8_norm_off vs a8_norm (a8_fused_norm=True, "
                         "a8_fused_act=True in both); W4A16 with --model "
                         "mixtral: wide = a16_wide_off (WeightOnlyExperts.wide_min_tokens = 0) vs a16_wide")
    ap.add_argument("--wide-min-tokens", type=int, default=-1,
                    help="with --scheme W4A16 --pair wide: WeightOnlyExperts.wide_min_tokens of a16_wide (default: "
                         "the class's)")
    ap.add_argument("--modes", default=None,
                    help="default: dequantized,packed (llama) / dequantized,packed,packed_experts (mixtral)")
    args = ap.parse_args()
    mixtral = args.model == "mixtral"
    modes = (args.modes or ",".join(A16_MODES + (("packed_experts",) if mixtral else ()))).split(",")
    vocab = 32000 if mixtral else 128256
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs a GPU")
    dev = torch.device("cuda:0")
    path = Path(args.checkpoint)
    if not (path / "config.json").exists():
        path.mkdir(parents=True, exist_ok=True)
        (write_mixtral_checkpoint if mixtral else write_checkpoint)(path, args.layers, dev, args.scheme)
    if args.batch < 1:
        raise SystemExit("--batch must be at least 1")
    prompt = torch.randint(0, vocab, (args.batch, args.prompt), generator=torch.Generator().manual_seed(0)).to(dev)
    result = {"tool": "decode_bench", "model": args.model, "checkpoint": str(path), "prompt": args.prompt,
              "new": args.new, "batch": args.batch, "scheme": args.scheme, "layers": args.layers, "modes": {}}
    if args.scheme != "W4A16":
        {"mid": a8_mid_modes, "wide": a8_wide_modes, "skinny": a8_modes, "fused": a8_fused_modes,
         "norm": a8_norm_modes}[args.pair](path, dev, prompt, args.new, result)
        print(json.dumps(result))
        return
    if args.pair == "wide":
        if not mixtral:
            raise SystemExit("--scheme W4A16 --pair wide compares expert-bank kernels: it needs --model mixtral")
        a16_wide_modes(path, dev, prompt, args.new, args.wide_min_tokens, result)
        print(json.dumps(result))
        return
    tokens = {}
    for mode in modes:
        torch.cuda.empty_cache()
        if mode == "packed_experts":
            model = load_quantized(path, device=dev, a16="packed", a16_experts="packed")
        elif mode == "packed_stream":                            # 17 - 128 rows on qt_gemm_wq_stream
            model = load_quantized(path, device=dev, a16="packed", a16_stream_rows=128)
        else:
            model = load_quantized(path, device=dev, a16=mode)
        lin_bytes = bank_bytes = 0
        for n, m in model.named_modules():
            own = sum(t.numel() * t.element_size() for t in list(m.parameters(recurse=False)) +
                      list(m.buffers(recurse=False)))
            if n.endswith(".mlp.experts"):
                bank_bytes += own
            elif n.rpartition(".")[2] in {l.rpartition(".")[2] for l in LINEARS} and ".layers." in n:
                lin_bytes += own
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()
        decode(model, prompt[:, :8], 4)                          # warm-up: kernels, allocator
        torch.cuda.reset_peak_memory_stats()
        toks, per_tok = decode(model, prompt, args.new)
        steps = [round(per_tok * 1e3, 3)]
        if "packed_stream" in modes:                             # each mode twice: the second pass is the spread
            toks2, per_tok2 = decode(model, prompt, args.new)
            assert toks2 == toks, f"{mode}: two runs gave different tokens"
            steps.append(round(per_tok2 * 1e3, 3))
        result["modes"][mode] = {
            "ms_per_token": round(per_tok * 1e3, 3), "ms_per_step": steps, "decoder_linear_bytes": lin_bytes,
            "expert_bank_bytes": bank_bytes,
            "weight_only_expert_banks": sum(isinstance(m, WeightOnlyExperts) for m in model.modules()),
            "memory_allocated_after_load": resident, "max_memory_allocated_decode": torch.cuda.max_memory_allocated(),
            "weight_only_linears": sum(isinstance(m, WeightOnlyLinear) for m in model.modules())}
        tokens[mode] = toks
        del model
    if not mixtral and set(tokens) == {"packed", "packed_stream"}:
        same = [x == y for x, y in zip(tokens["packed"], tokens["packed_stream"])]
        result["tokens_agree"] = sum(same)                       # not expected on a random-init model
        result["first_difference"] = same.index(False) if not all(same) else None
        p, k = (min(result["modes"][m]["ms_per_step"]) for m in ("packed", "packed_stream"))
        result["speedup"] = round(p / k, 3)
    if not mixtral and set(tokens) == set(A16_MODES):
        a, b = tokens.values()
        same = [x == y for x, y in zip(a, b)]
        result["tokens_agree"] = sum(same)
        result["first_difference"] = same.index(False) if not all(same) else None
        d, p = (result["modes"][m] for m in A16_MODES)
        result["linear_bytes_ratio"] = round(p["decoder_linear_bytes"] / d["decoder_linear_bytes"], 4)
        result["speedup"] = round(d["ms_per_token"] / p["ms_per_token"], 3)
    if mixtral and "dequantized" in tokens:
        d = result["modes"]["dequantized"]
        for mode in (m for m in tokens if m != "dequantized"):
            same = [x == y for x, y in zip(tokens["dequantized"], tokens[mode])]
            r = result["modes"][mode]
            r["tokens_agree_with_dequantized"] = sum(same)
            r["first_difference"] = same.index(False) if not all(same) else None
            r["speedup_over_dequantized"] = round(d["ms_per_token"] / r["ms_per_token"], 3)
            r["expert_bytes_ratio"] = round(r["expert_bank_bytes"] / d["expert_bank_bytes"], 4)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
