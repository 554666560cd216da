"""Reading back the checkpoints this project writes, and running them.

``load_quantized`` rebuilds the model from ``config.json`` and the dense tensors, then puts in place of every quantized
Linear either

* a ``QuantizedLinear`` (W8A8 / INT8 / W4A8: the checkpoint's 8-bit dynamic per-token ``input_activations`` block):
  activations are quantised per row on the fly and multiplied with the stored integer weights on the int8 MFMA
  (``qt_quantize_tokens_i8`` + ``qt_gemm_i8``, or its bit-identical decode form ``qt_gemm_i8_skinny`` for up to
  ``skinny_max_m`` rows, its bit-identical weight-streaming form ``qt_gemm_i8_mid`` above that up to ``mid_max_m``
  rows and, for int8 weights with channel-wise scales, its bit-identical prefill form ``qt_gemm_i8_ring`` from
  ``ring_min_m`` rows; include/quantool_amd.h), as a served W8A8 runtime does; or
* a plain ``nn.Linear`` holding the dequantised weight ``(q - zp) * scale`` (W4A16, W4A16_ASYM, W8A16), computed once in
  fp32 from the STORED scale and rounded once to the model dtype (the default, ``a16="dequantized"``); or
* with ``a16="packed"``, a ``WeightOnlyLinear`` that keeps the stored integer weights on the device: decode-sized inputs
  (M <= ``skinny_max_m`` rows) run the GEMV ``qt_gemm_wq_skinny``, larger ones dequantise the weight into a transient
  buffer (``qt_dequantize_weight``, bit-identical to the dequantised ``nn.Linear``) and call ``F.linear``; with
  ``a16_stream_rows`` inputs of 17 to that many rows run the weight-streaming ``qt_gemm_wq_stream`` instead.

Routed-expert banks (transformers >= 5 fuses them: ``<layer>.mlp.experts.gate_up_proj [E, 2I, H]`` / ``down_proj
[E, H, I]``) are written per expert by ``sequential.expert_bank_checkpoint_names`` (Mixtral:
``<layer>.block_sparse_moe.experts.{e}.w1 / w3 / w2``, otherwise ``<layer>.mlp.experts.{e}.gate_proj / up_proj /
down_proj``).  The loader inverts that write: A16 experts are dequantised into the fused parameters
(``gate_up_proj[e] = cat(w1, w3)``, ``down_proj[e] = w2``), or with ``a16_experts="packed"`` replace the bank with a
``WeightOnlyExperts`` on the stored integer weights (``qt_gemm_wq_grouped`` at decode, ``qt_moe_gemm_wq_wide`` from
``wide_min_tokens`` tokens and, with ``a16_experts_wide_tokens``, past 128); A8 experts replace the bank with
a ``QuantizedExperts`` that runs the routed rows on the grouped int8 GEMM (``qt_moe_route`` + ``qt_gemm_i8_grouped`` +
``qt_moe_combine``; ``qt_gemm_i8_skinny_grouped`` in place of the GEMM for up to ``grouped_max_tokens`` tokens, and
``qt_gemm_i8_ring_grouped`` for an int8 bank from ``ring_min_rows_per_expert`` routed rows per expert,
``qt_moe_gemm_i8_ring_w4`` for a packed int4 bank from ``ring_w4_min_rows_per_expert``, and between the decode range and
the rings ``qt_moe_gemm_i8_wide`` up to ``wide_max_rows_per_expert`` / ``wide_w4_max_rows_per_expert`` routed rows per
expert for products with K >= ``wide_min_k`` and N <= ``wide_max_n``).

Loading needs no GPU: every load-time step (int4 unpacking, the column permutation of actorder ``group``, the per-group
weight sums) is integer torch work on whatever device the model is built on.  Only ``QuantizedLinear.forward``,
``QuantizedExperts.forward``, ``WeightOnlyLinear.forward`` and ``WeightOnlyExperts.forward`` on device tensors need
the HIP library.

With ``a8_fused_act=True`` an A8 checkpoint's MLP glue -- SiLU(gate) * up and the quantiser of the down product -- runs
as one pass (``qt_act_mul_quantize_i8``): ``QuantizedExperts.fused_act`` in a bank, a ``QuantizedMLP`` in place of a
Llama-style dense MLP.  With ``a8_fused_norm=True`` the RMSNorms in front of q/k/v and gate/up become
``QuantizingRMSNorm``s: the norm and the quantiser its consumers share run as one pass (``qt_rmsnorm_quantize_i8``).

The modules are defined in ``qmodules.py`` and one stored weight as a value (``StoredWeight``: the only reader of a
module's checkpoint tensors, the kernels' layout rules, ``dequantize``, the stacking of experts into a bank) in
``stored_weight.py``; both are re-exported here, and this file is the loader.
"""
from __future__ import annotations

import json
import re
from pathlib import Path
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from .qmodules import (QuantizedExperts, QuantizedLinear, QuantizedMLP, QuantizingRMSNorm, SharedRows,  # noqa: F401
                       WeightOnlyExperts, WeightOnlyLinear)
from .serialization import load_state
from .stored_weight import GROUP, StoredWeight, group_sums, pack_int4, unpack_int4  # noqa: F401 (re-exported)

_LEAVES = ("weight", "weight_packed", "weight_scale", "weight_zero_point", "weight_g_idx", "weight_shape")
# per-expert names expert_bank_checkpoint_names writes (<bank>.experts.{e}.<proj>)
_EXPERT_RE = re.compile(r"\.experts\.\d+\.")
# <bank>.{e}.<proj> -- a per-expert module name, split
_EXPERT_NAME = re.compile(r"^(?P<bank>.+\.experts)\.(?P<e>\d+)\.(?P<proj>[^.]+)$")
_A16_HINT = "; load it with a16='dequantized'"


def _is_a8(block) -> bool:
    """The 8-bit dynamic per-token integer block W8A8 / INT8 / W4A8 write (schemes.py _A8_TOKEN_DYN)."""
    return (isinstance(block, dict) and block.get("num_bits") == 8 and block.get("type", "int") == "int"
            and block.get("strategy") == "token" and bool(block.get("dynamic")))


def _split_state(state: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], Dict[str, Dict[str, torch.Tensor]]]:
    """(dense tensors, {module name: {leaf: tensor}}) -- a module is quantized when it has a ``weight_scale``."""
    qmods = {k[: -len(".weight_scale")] for k in state if k.endswith(".weight_scale")}
    quant: Dict[str, Dict[str, torch.Tensor]] = {m: {} for m in qmods}
    dense: Dict[str, torch.Tensor] = {}
    for k, v in state.items():
        mod, _, leaf = k.rpartition(".")
        if mod in quant and leaf in _LEAVES:
            quant[mod][leaf] = v
        else:
            dense[k] = v
    return dense, quant


def dequantized_weight(name: str, t: Dict[str, torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """(q - zp) * scale in fp32 from the stored scale (and zero-point), rounded once to ``dtype``: [N, K]."""
    return StoredWeight.from_leaves(name, t).dequantize(dtype)


def _refuse_zero_point(name: str, w: StoredWeight) -> None:
    if w.zero_point is not None:
        raise ValueError(f"{name}: an A8 checkpoint with weight_zero_point -- the int8 GEMM has no weight zero-point "
                         "term (W8A8, INT8 and W4A8 weights are symmetric)")


def quantized_linear_from_tensors(name: str, t: Dict[str, torch.Tensor], act_symmetric: bool,
                                  bias: Optional[torch.Tensor] = None) -> QuantizedLinear:
    """A ``QuantizedLinear`` from one module's checkpoint tensors (A8 schemes)."""
    w = StoredWeight.from_leaves(name, t)
    _refuse_zero_point(name, w)
    w = w.require_kernel_layout(name)
    levels, col_perm = w.levels, None
    if w.g_idx is not None:             # actorder "group": the GEMM takes contiguous groups, so permute the columns
        g = w.g_idx.to(torch.int64)
        perm = torch.argsort(g, stable=True)
        if not torch.equal(g[perm], torch.arange(w.K, device=g.device) // GROUP):
            raise ValueError(f"{name}: weight_g_idx groups are not {GROUP} columns each")
        q = (unpack_int4(levels, w.K) if w.int4 else levels)[:, perm]
        levels = pack_int4(q) if w.int4 else q.contiguous()
        col_perm = perm.to(torch.int32)
    return QuantizedLinear(w.K, w.N, levels, w.scale, act_symmetric, col_perm=col_perm, bias=bias)


def weight_only_linear_from_tensors(name: str, t: Dict[str, torch.Tensor],
                                    bias: Optional[torch.Tensor] = None) -> WeightOnlyLinear:
    """A ``WeightOnlyLinear`` from one module's checkpoint tensors (A16 schemes, ``a16="packed"``)."""
    w = StoredWeight.from_leaves(name, t).require_kernel_layout(name, _A16_HINT)
    return WeightOnlyLinear(w.K, w.N, w.levels, w.scale, weight_zero_point=w.zero_point, g_idx=w.g_idx, bias=bias)


def _read_config(path: Path) -> Tuple[dict, dict]:
    cfg = json.loads((path / "config.json").read_text())
    qcfg = cfg.pop("quantization_config", None)
    if not qcfg:
        raise ValueError(f"{path}: config.json has no quantization_config")
    return cfg, qcfg


def _model_dtype(cfg: dict, dtype) -> torch.dtype:
    if dtype is not None:
        return dtype
    name = cfg.get("torch_dtype") or cfg.get("dtype") or "bfloat16"
    name = str(name).replace("torch.", "")
    return {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32}.get(name, torch.bfloat16)


def _is_fused_bank(m: nn.Module) -> bool:
    """A transformers >= 5 expert bank: 3-d ``gate_up_proj`` / ``down_proj`` parameters and an ``act_fn``."""
    gu, dn = getattr(m, "gate_up_proj", None), getattr(m, "down_proj", None)
    return (isinstance(gu, nn.Parameter) and isinstance(dn, nn.Parameter) and gu.dim() == 3 and dn.dim() == 3
            and hasattr(m, "act_fn"))


def _expert_banks(path, model: nn.Module, model_type, dense: Dict[str, torch.Tensor],
                  quant: Dict[str, Dict[str, torch.Tensor]]):
    """Undo ``expert_bank_checkpoint_names``: rename ``dense`` back to the model's names in place, and take every
    per-expert tensor out of ``dense`` / ``quant``.  Returns ({bank name: module}, {bank name: {e: {proj: ("q", leaves) |
    ("dense", tensor)}}}, {checkpoint prefix: model prefix}).  proj is gate_proj / up_proj / down_proj."""
    from .sequential import expert_bank_module_renames, expert_layout, rename_module_prefix as _rename

    banks = {n: m for n, m in model.named_modules() if _is_fused_bank(m)}
    inverse = {v: k for k, v in expert_bank_module_renames(banks, model_type).items()}
    _, leafs = expert_layout(model_type)
    proj_of = {v: k for k, v in leafs.items()}            # checkpoint leaf (w1) -> fused role (gate_proj)
    renamed = {_rename(k, inverse): v for k, v in dense.items()}
    dense.clear()
    dense.update(renamed)
    found: Dict[str, Dict[int, Dict[str, tuple]]] = {}

    def place(name: str, kind: str, value) -> bool:
        m = _EXPERT_NAME.match(_rename(name, inverse))
        if m is None:
            return False
        bank, e, proj = m.group("bank"), int(m.group("e")), m.group("proj")
        if bank not in banks:
            return False
        if proj not in proj_of:
            raise ValueError(f"{path}: {name}: {proj!r} is none of the expert Linears {sorted(proj_of)}")
        E = banks[bank].gate_up_proj.shape[0]
        if e >= E:
            raise ValueError(f"{path}: {name}: expert {e} of a bank of {E}")
        found.setdefault(bank, {}).setdefault(e, {})[proj_of[proj]] = (kind, value)
        return True

    for name in [n for n in quant if _EXPERT_RE.search(n + ".")]:
        m = _EXPERT_NAME.match(_rename(name, inverse))
        if m is None or m.group("bank") not in banks:
            raise NotImplementedError(
                f"{path}: routed-expert weights ({name}) without a fused expert bank at that place in the "
                f"{type(model).__name__} built from config.json; this loader maps per-expert Linears back to a "
                "transformers >= 5 gate_up_proj / down_proj bank only")
        place(name, "q", quant.pop(name))
    for key in [k for k in dense if _EXPERT_RE.search(k)]:
        mod, _, leaf = key.rpartition(".")
        if _EXPERT_NAME.match(mod) is None or _EXPERT_NAME.match(mod).group("bank") not in banks:
            continue                                       # not ours: load_state_dict reports it
        if leaf != "weight":
            raise NotImplementedError(f"{path}: {key}: experts with a {leaf} are not supported (the expert bank "
                                      "this loader rebuilds has no bias)")
        place(mod, "dense", dense.pop(key))
    for bank in found:
        if any("bias" in n for n, _ in banks[bank].named_parameters()):
            raise NotImplementedError(f"{path}: {bank} has expert biases, which this loader does not read")
    return banks, found, inverse


def _check_shape(name: str, shape, lin_shape) -> None:
    if tuple(shape) != tuple(lin_shape):
        raise ValueError(f"{name} has shape {tuple(shape)} in the checkpoint, {tuple(lin_shape)} in the model")


def _set_submodule(model: nn.Module, name: str, new: nn.Module) -> None:
    parent_name, _, leaf = name.rpartition(".")
    setattr(model.get_submodule(parent_name) if parent_name else model, leaf, new)


def _load_bank(path, bank_name: str, bank: nn.Module, experts: Dict[int, Dict[str, tuple]], a8: bool,
               act_symmetric: bool, mdtype: torch.dtype, dev, packed_experts: bool = False) -> Optional[nn.Module]:
    """Fill (A16, dense) or replace (A8: the returned ``QuantizedExperts``; A16 with ``packed_experts``: the returned
    ``WeightOnlyExperts``) one fused bank from its experts."""
    gu, dn = bank.gate_up_proj, bank.down_proj
    E, I2, H = gu.shape
    I = I2 // 2
    want = {"gate_proj": (I, H), "up_proj": (I, H), "down_proj": (H, I)}
    missing = [f"{e}.{r}" for e in range(E) for r in want if r not in experts.get(e, {})]
    if missing:
        raise ValueError(f"{path}: {bank_name}: experts missing from the checkpoint: {missing[:6]}")
    kinds = {experts[e][r][0] for e in range(E) for r in want}
    if len(kinds) > 1:
        raise ValueError(f"{path}: {bank_name} is only partly quantized (some expert Linears are dense); the bank "
                         "runs as one unit, so every expert Linear must share a scheme")

    def read(e: int, r: str):
        """(name, expert e's Linear r on ``dev``: a ``StoredWeight``, or the tensor of a dense one), shape checked."""
        name = f"{path}: {bank_name}.{e}.{r}"
        kind, v = experts[e][r]
        if kind == "dense":
            w = v.to(dev)
            _check_shape(name, w.shape, want[r])
        else:
            w = StoredWeight.from_leaves(name, {k: t.to(dev) for k, t in v.items()})
            _check_shape(name, (w.N, w.K), want[r])
        return name, w

    if kinds == {"dense"} or not (a8 or packed_experts):
        for e in range(E):
            W = {}
            for r in want:
                w = read(e, r)[1]
                W[r] = w.dequantize(mdtype) if isinstance(w, StoredWeight) else w.to(mdtype)
            gu.data[e] = torch.cat([W["gate_proj"], W["up_proj"]], 0)
            dn.data[e] = W["down_proj"]
        return None

    def kernel_weight(e: int, r: str) -> StoredWeight:
        name, w = read(e, r)
        if a8:
            if w.g_idx is not None:
                raise NotImplementedError(f"{name}: A8 expert weights with weight_g_idx (actorder 'group') need a "
                                          "per-expert column permutation, which the grouped GEMM does not take; "
                                          "quantise with actorder 'static'")
            _refuse_zero_point(name, w)
        return w.require_kernel_layout(name, "" if a8 else _A16_HINT)

    # gate rows before up rows
    gate_up = StoredWeight.stack(f"{path}: {bank_name} gate_up",
                                 [[kernel_weight(e, r) for r in ("gate_proj", "up_proj")] for e in range(E)])
    down = StoredWeight.stack(f"{path}: {bank_name} down", [[kernel_weight(e, "down_proj")] for e in range(E)])
    if gate_up.int4 != down.int4:
        raise ValueError(f"{path}: {bank_name}: gate_up and down weights differ in format")
    if a8:
        return QuantizedExperts(H, I, gate_up.levels, gate_up.scale, down.levels, down.scale, bank.act_fn,
                                act_symmetric)
    return WeightOnlyExperts(bank, gate_up.levels, gate_up.scale, down.levels, down.scale,
                             gate_up_zero_point=gate_up.zero_point, gate_up_g_idx=gate_up.g_idx,
                             down_zero_point=down.zero_point, down_g_idx=down.g_idx)


def _install_quantizing_norms(model: nn.Module) -> None:
    """``a8_fused_norm``: in every decoder layer of ``QuantizingRMSNorm.PLAIN_LAYERS``, ``input_layernorm`` quantises for
    ``self_attn.{q,k,v}_proj`` and ``post_attention_layernorm`` for ``mlp.{gate,up}_proj`` (a plain MLP, or a
    ``QuantizedMLP``, which quantises once for both), wherever ``QuantizingRMSNorm.refusal`` is None."""
    for name, layer in [(n, m) for n, m in model.named_modules()
                        if type(m).__name__ in QuantizingRMSNorm.PLAIN_LAYERS]:
        feeds = [("input_layernorm", getattr(layer, "self_attn", None), ("q_proj", "k_proj", "v_proj"))]
        mlp = getattr(layer, "mlp", None)
        if isinstance(mlp, QuantizedMLP) or type(mlp).__name__ in QuantizedMLP.PLAIN_MLPS:
            feeds.append(("post_attention_layernorm", mlp, ("gate_proj", "up_proj")))
        for norm_name, parent, names in feeds:
            norm = getattr(layer, norm_name, None)
            consumers = [getattr(parent, n, None) for n in names]
            if norm is None or parent is None or QuantizingRMSNorm.refusal(norm, consumers) is not None:
                continue
            takes = 1 if isinstance(parent, QuantizedMLP) else len(consumers)
            _set_submodule(model, f"{name}.{norm_name}",
                           QuantizingRMSNorm(norm.weight, norm.variance_epsilon, consumers, takes=takes))


A16_MODES = ("dequantized", "packed")
# The largest ``a16_experts_wide_tokens``: the largest call size at which qt_moe_gemm_wq_wide was measured (DESIGN.md
# 4.19).
A16_EXPERTS_WIDE_MAX_TOKENS = 2048


def load_quantized(path, device="cuda", dtype: Optional[torch.dtype] = None, a16: str = "dequantized",
                   a16_experts: str = "dequantized", a16_stream_rows: int = 0,
                   a16_experts_wide_tokens: int = 0, a8_fused_act: bool = False,
                   a8_fused_norm: bool = False) -> nn.Module:
    """Rebuild the model a ``save_pretrained`` / ``_save_compressed`` directory describes (one file or shards) with
    ``QuantizedLinear``s (A8 schemes) or, for A16 schemes, dequantised ``nn.Linear``s (``a16="dequantized"``, the
    default) or ``WeightOnlyLinear``s on the stored integer weights (``a16="packed"``) in place of its quantized Linears.
    A8 checkpoints ignore ``a16`` and ``a16_experts``.  In packed mode A16 routed-expert banks are still dequantised
    into the fused bank unless ``a16_experts="packed"`` (which needs ``a16="packed"``) replaces each with a
    ``WeightOnlyExperts``; ``model._qt_checkpoint`` then records ``"a16": "packed"``, the banks left dense under
    ``"dense_expert_banks"`` and, with ``a16_experts="packed"``, the packed ones under ``"packed_expert_banks"``.
    ``a16_stream_rows`` (0, the default, or 17 ... 128; needs ``a16="packed"``) sets ``stream_max_m`` on every
    ``WeightOnlyLinear`` built, so inputs of 17 to that many rows run ``qt_gemm_wq_stream`` on the stored weights
    instead of dequantise + ``F.linear`` (``WeightOnlyExperts`` are not touched); it is recorded under
    ``"a16_stream_rows"``.  A8 checkpoints ignore it.
    ``a16_experts_wide_tokens`` (0, the default, or 129 ... ``A16_EXPERTS_WIDE_MAX_TOKENS``; needs
    ``a16_experts="packed"``) sets ``wide_max_tokens`` on every ``WeightOnlyExperts`` built, so calls of 129 to that many
    tokens route their rows and run ``qt_moe_gemm_wq_wide`` on the stored weights instead of dequantising both banks; it
    is recorded under ``"a16_experts_wide_tokens"``.  A8 checkpoints ignore it.
    ``a8_fused_act`` (False, the default, or True) runs the glue between the two products of every A8 MLP as one pass,
    ``qt_act_mul_quantize_i8``, equal to the bit to the SiLU, the multiply and the quantiser it replaces: it sets
    ``fused_act`` on every ``QuantizedExperts`` built and puts a ``QuantizedMLP`` in place of every dense MLP for which
    ``QuantizedMLP.eligible`` holds (a Llama-style MLP of three ``QuantizedLinear``s with SiLU); state-dict keys do not
    move, and it is recorded under ``"a8_fused_act"``.  A16 checkpoints ignore it.
    ``a8_fused_norm`` (False, the default, or True) runs the RMSNorm in front of q/k/v and of gate/up and the quantiser
    those Linears share as one pass, ``qt_rmsnorm_quantize_i8``: in every decoder layer of
    ``QuantizingRMSNorm.PLAIN_LAYERS`` it puts a ``QuantizingRMSNorm`` in place of ``input_layernorm`` and (not in a
    Mixtral layer, whose second norm feeds the router and the bank) of ``post_attention_layernorm`` wherever
    ``QuantizingRMSNorm.refusal`` is None.  The norm's sum over K runs in the kernel's order, not torch's, so outputs may
    differ from the default loader's in rare last bits; state-dict keys do not move, and it is recorded
    under ``"a8_fused_norm"``.  A16 checkpoints ignore it.

    Routed-expert banks written per expert (``sequential.expert_bank_checkpoint_names``) are mapped back to the fused
    bank of the model built from ``config.json`` (undoing the Mixtral ``block_sparse_moe`` rename of every tensor and of
    ``quantization_config.ignore``): A16 experts are dequantised into ``gate_up_proj`` / ``down_proj``; A8 experts
    replace the bank with a ``QuantizedExperts``.

    Refused with ``ValueError`` / ``NotImplementedError``: float-quantized checkpoints, any ``input_activations`` block
    other than 8-bit dynamic per-token, an A8 checkpoint that carries ``weight_zero_point``, routed-expert weights
    where the model has no fused bank, A8 expert weights with ``weight_g_idx``, experts with a bias, banks with
    experts missing or only partly quantized, and (packed A16 experts) banks whose experts mix formats, group counts
    or zero-points, or whose gate and up halves group their columns differently."""
    from transformers import AutoConfig, AutoModelForCausalLM

    if a16 not in A16_MODES:
        raise ValueError(f"a16={a16!r}: expected one of {A16_MODES}")
    if a16_experts not in A16_MODES:
        raise ValueError(f"a16_experts={a16_experts!r}: expected one of {A16_MODES}")
    if a16_experts == "packed" and a16 != "packed":
        raise ValueError("a16_experts='packed' needs a16='packed' (packed expert banks beside dequantised Linears "
                         "is not a mode this loader offers)")
    if type(a16_stream_rows) is not int or not (a16_stream_rows == 0 or 17 <= a16_stream_rows <= 128):
        raise ValueError(f"a16_stream_rows={a16_stream_rows!r}: expected 0 or 17 ... 128")
    if a16_stream_rows and a16 != "packed":
        raise ValueError("a16_stream_rows needs a16='packed' (dequantised Linears have no stored weights to stream)")
    if type(a16_experts_wide_tokens) is not int or not (
            a16_experts_wide_tokens == 0 or 129 <= a16_experts_wide_tokens <= A16_EXPERTS_WIDE_MAX_TOKENS):
        raise ValueError(f"a16_experts_wide_tokens={a16_experts_wide_tokens!r}: expected 0 or 129 ... "
                         f"{A16_EXPERTS_WIDE_MAX_TOKENS}")
    if a16_experts_wide_tokens and a16_experts != "packed":
        raise ValueError("a16_experts_wide_tokens needs a16_experts='packed' (dequantised banks have no stored weights "
                         "to run on)")
    if type(a8_fused_act) is not bool:
        raise ValueError(f"a8_fused_act={a8_fused_act!r}: expected True or False")
    if type(a8_fused_norm) is not bool:
        raise ValueError(f"a8_fused_norm={a8_fused_norm!r}: expected True or False")
    path = Path(path)
    cfg, qcfg = _read_config(path)
    fmt = str(qcfg.get("format", ""))
    group = (qcfg.get("config_groups") or {}).get("group_0") or {}
    wcfg = group.get("weights") or {}
    if fmt.startswith(("float", "nvfp4")) or wcfg.get("type") == "float":
        raise NotImplementedError(f"{path}: format {fmt!r} is a float preset; this loader reads the integer "
                                  "checkpoints (pack-quantized / int-quantized) this backend writes")
    acts = group.get("input_activations")
    if acts is not None and not _is_a8(acts):
        raise NotImplementedError(f"{path}: input_activations {acts!r} is not supported; the runtime quantises "
                                  "activations to 8-bit integers per token, dynamically")
    state = load_state(path)
    dense, quant = _split_state(state)

    mdtype = _model_dtype(cfg, dtype)
    model_type = cfg.pop("model_type")
    for k in ("torch_dtype", "dtype", "transformers_version"):
        cfg.pop(k, None)
    config = AutoConfig.for_model(model_type, **cfg)
    dev = torch.device(device)
    with dev:
        model = AutoModelForCausalLM.from_config(config, torch_dtype=mdtype)
    model.eval()

    banks, experts, inverse = _expert_banks(path, model, model_type, dense, quant)
    missing, unexpected = model.load_state_dict(dense, strict=False)
    if unexpected:
        raise ValueError(f"{path}: unexpected tensors {sorted(unexpected)[:8]}")
    allowed = {f"{m}.weight" for m in quant}
    allowed |= {f"{b}.{p}" for b in experts for p in ("gate_up_proj", "down_proj")}
    bad = sorted(set(missing) - allowed)
    if bad:
        raise ValueError(f"{path}: tensors missing from the checkpoint: {bad[:8]}")

    a8 = acts is not None
    act_symmetric = bool(acts.get("symmetric", True)) if a8 else True
    packed_experts = not a8 and a16_experts == "packed"
    replaced = []
    for bank_name, by_expert in experts.items():
        new = _load_bank(path, bank_name, banks[bank_name], by_expert, a8, act_symmetric, mdtype, dev,
                         packed_experts=packed_experts)
        if new is not None:
            replaced.append(bank_name)
            if packed_experts and a16_experts_wide_tokens:
                new.wide_max_tokens = a16_experts_wide_tokens
            if a8 and a8_fused_act:
                new.fused_act = True
            _set_submodule(model, bank_name, new)
    for name, t in quant.items():
        lin = model.get_submodule(name)
        if not isinstance(lin, nn.Linear):
            raise ValueError(f"{path}: {name} is quantized in the checkpoint but is a {type(lin).__name__} here")
        t = {k: v.to(dev) for k, v in t.items()}
        if a8 or a16 == "packed":
            bias = None if lin.bias is None else lin.bias.data
            new = (quantized_linear_from_tensors(name, t, act_symmetric, bias=bias) if a8
                   else weight_only_linear_from_tensors(name, t, bias=bias))
            _check_shape(f"{path}: {name}", (new.out_features, new.in_features), lin.weight.shape)
            if not a8 and a16_stream_rows:
                new.stream_max_m = a16_stream_rows
            _set_submodule(model, name, new)
        else:
            W = dequantized_weight(name, t, mdtype)
            _check_shape(f"{path}: {name}", W.shape, lin.weight.shape)
            lin.weight.data = W
    if a8 and a8_fused_act:
        for name, mlp in [(n, m) for n, m in model.named_modules() if QuantizedMLP.eligible(m)]:
            _set_submodule(model, name, QuantizedMLP(mlp.gate_proj, mlp.up_proj, mlp.down_proj, mlp.act_fn))
    if a8 and a8_fused_norm:
        _install_quantizing_norms(model)
    from .sequential import rename_module_prefix as _rename

    ignore = [_rename(n, inverse) for n in qcfg.get("ignore") or []]
    model._qt_checkpoint = {"path": str(path), "format": fmt, "input_activations": acts, "ignore": ignore}
    if a8:
        model._qt_checkpoint["a8_fused_act"] = a8_fused_act
        model._qt_checkpoint["a8_fused_norm"] = a8_fused_norm
    if not a8 and a16 == "packed":
        model._qt_checkpoint["a16"] = "packed"
        model._qt_checkpoint["a16_stream_rows"] = a16_stream_rows
        model._qt_checkpoint["dense_expert_banks"] = sorted(set(experts) - set(replaced))
        if packed_experts:
            model._qt_checkpoint["packed_expert_banks"] = sorted(replaced)
            model._qt_checkpoint["a16_experts_wide_tokens"] = a16_experts_wide_tokens
    return model
