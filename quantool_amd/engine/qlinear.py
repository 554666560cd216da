"""Reading back the checkpoints this project writes, and running them.

``load_quantized`` rebuilds the model from ``config.json`` and the dense tensors, then puts in place of every quantized
Linear either

* a ``QuantizedLinear`` (W8A8 / INT8 / W4A8: the checkpoint's 8-bit dynamic per-token ``input_activations`` block):
  activations are quantised per row on the fly and multiplied with the stored integer weights on the int8 MFMA
  (``qt_quantize_tokens_i8`` + ``qt_gemm_i8``, include/quantool_amd.h), as a served W8A8 runtime does; or
* a plain ``nn.Linear`` holding the dequantised weight ``(q - zp) * scale`` (W4A16, W4A16_ASYM, W8A16), computed once in
  fp32 from the STORED scale and rounded once to the model dtype.

Loading needs no GPU: every load-time step (int4 unpacking, the column permutation of actorder ``group``, the per-group
weight sums) is integer torch work on whatever device the model is built on.  Only ``QuantizedLinear.forward`` needs the
HIP library.
"""
from __future__ import annotations

import json
import re
from pathlib import Path
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from .serialization import load_state

GROUP = 128   # the W4A8 group size the GEMM takes
_LEAVES = ("weight", "weight_packed", "weight_scale", "weight_zero_point", "weight_g_idx", "weight_shape")
# per-expert names expert_bank_checkpoint_names writes (<bank>.experts.{e}.<proj>)
_EXPERT_RE = re.compile(r"\.experts\.\d+\.")


def unpack_int4(packed: torch.Tensor, K: int) -> torch.Tensor:
    """int32 [R, ceil(K/8)] (nibble j of word w = level of column 8w + j, plus 8) -> int8 levels [R, K]."""
    shifts = torch.arange(0, 32, 4, device=packed.device, dtype=torch.int32)
    nib = (packed.unsqueeze(-1) >> shifts) & 0xF
    return (nib.reshape(packed.shape[0], -1)[:, :K] - 8).to(torch.int8)


def pack_int4(q: torch.Tensor) -> torch.Tensor:
    """int8 levels [R, K] in [-8, 7] -> int32 [R, ceil(K/8)], the inverse of ``unpack_int4``."""
    R, K = q.shape
    Kw = (K + 7) // 8
    v = torch.full((R, Kw * 8), 8, dtype=torch.int64, device=q.device)
    v[:, :K] = q.to(torch.int64) + 8
    shifts = torch.arange(0, 32, 4, device=q.device, dtype=torch.int64)
    words = (v.reshape(R, Kw, 8) << shifts).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def group_sums(q: torch.Tensor, G: int) -> torch.Tensor:
    """wsum [R, G] int32: sums of the levels q [R, K] over each group of 128 contiguous columns (G = 1: whole rows)."""
    R, K = q.shape
    if G == 1:
        return q.to(torch.int32).sum(1, dtype=torch.int32).reshape(R, 1).contiguous()
    pad = G * GROUP - K
    qp = torch.nn.functional.pad(q.to(torch.int32), (0, pad)) if pad else q.to(torch.int32)
    return qp.reshape(R, G, GROUP).sum(-1, dtype=torch.int32).contiguous()


class QuantizedLinear(nn.Module):
    """One W8A8 / INT8 / W4A8 Linear of a checkpoint: ``forward(x)`` quantises the rows of ``x`` to int8 (per token,
    dynamic) and runs the int8 x int8 GEMM with the checkpoint's weight scales.

    Buffers: ``weight`` int8 [N, K] or packed int4 int32 [N, ceil(K/8)] (columns permuted by ``col_perm`` when the
    checkpoint used actorder ``group``), ``weight_scale`` fp32 [N, G], ``wsum`` int32 [N, G], ``col_perm`` int32 [K]
    (optional), ``bias`` (optional, model dtype)."""

    def __init__(self, in_features: int, out_features: int, weight: torch.Tensor, weight_scale: torch.Tensor,
                 act_symmetric: bool, col_perm: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
        super().__init__()
        self.in_features = int(in_features)
        self.out_features = int(out_features)
        self.act_symmetric = bool(act_symmetric)
        self.int4 = weight.dtype == torch.int32
        levels = unpack_int4(weight, in_features) if self.int4 else weight
        G = weight_scale.shape[1]
        self.register_buffer("weight", weight.contiguous())
        self.register_buffer("weight_scale", weight_scale.to(torch.float32).contiguous())
        self.register_buffer("wsum", group_sums(levels, G))
        self.register_buffer("col_perm", None if col_perm is None else col_perm.to(torch.int32).contiguous())
        self.register_buffer("bias", None if bias is None else bias.contiguous())

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"weights={'int4 g128' if self.int4 else 'int8'}, groups={self.weight_scale.shape[1]}, "
                f"act={'sym' if self.act_symmetric else 'asym'} int8 per-token, "
                f"col_perm={self.col_perm is not None}, bias={self.bias is not None}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from ..hip import ops

        lead = x.shape[:-1]
        x2 = x.reshape(-1, self.in_features)
        if x2.stride(1) != 1:
            x2 = x2.contiguous()
        Xq, s_x, zp_x = ops.quantize_tokens_i8(x2, symmetric=self.act_symmetric, col_perm=self.col_perm)
        bias = None if self.bias is None else self.bias.to(x.dtype)
        y = ops.gemm_i8(Xq, s_x, self.weight, self.weight_scale, K=self.in_features, zp_x=zp_x,
                        wsum=None if zp_x is None else self.wsum, bias=bias, out_dtype=x.dtype)
        return y.reshape(*lead, self.out_features)


# ---- the loader ------------------------------------------------------------------------------------------------------
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


def _levels_and_shape(name: str, t: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, int, int, bool]:
    """(stored weight tensor, N, K, packed int4?) of one quantized module."""
    if "weight_shape" in t:
        N, K = (int(v) for v in t["weight_shape"].tolist())
    elif "weight" in t:
        N, K = t["weight"].shape
    else:
        raise ValueError(f"{name}: packed weight without weight_shape")
    if "weight_packed" in t:
        w = t["weight_packed"]
        if w.dtype != torch.int32 or tuple(w.shape) != (N, (K + 7) // 8):
            raise ValueError(f"{name}: weight_packed must be int32 [{N}, {(K + 7) // 8}], got {w.dtype} "
                             f"{tuple(w.shape)}")
        return w, N, K, True
    w = t.get("weight")
    if w is None or w.dtype != torch.int8 or tuple(w.shape) != (N, K):
        raise ValueError(f"{name}: expected an int8 weight [{N}, {K}] or a weight_packed tensor")
    return w, N, K, False


def _group_of_columns(name: str, t: Dict[str, torch.Tensor], K: int, G: int) -> torch.Tensor:
    """int64 [K]: the group of every original column (weight_g_idx when present, else column // (K / G))."""
    if "weight_g_idx" in t:
        g = t["weight_g_idx"].to(torch.int64)
        if g.numel() != K or int(g.min()) < 0 or int(g.max()) >= G:
            raise ValueError(f"{name}: weight_g_idx does not match {G} groups of {K} columns")
        return g
    if G == 1:
        return torch.zeros(K, dtype=torch.int64, device=t["weight_scale"].device)
    return torch.arange(K, device=t["weight_scale"].device) // GROUP


def dequantized_weight(name: str, t: Dict[str, torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """(q - zp) * scale in fp32 from the stored scale (and zero-point), rounded once to ``dtype``: [N, K]."""
    w, N, K, packed = _levels_and_shape(name, t)
    q = unpack_int4(w, K) if packed else w
    scale = t["weight_scale"].to(torch.float32)
    G = scale.shape[1]
    g = _group_of_columns(name, t, K, G)
    s_col = scale[:, g]
    q = q.to(torch.float32)
    if "weight_zero_point" in t:
        q = q - t["weight_zero_point"].to(torch.float32)[:, g]
    return (q * s_col).to(dtype)


def quantized_linear_from_tensors(name: str, t: Dict[str, torch.Tensor], act_symmetric: bool,
                                  bias: Optional[torch.Tensor] = None) -> QuantizedLinear:
    """A ``QuantizedLinear`` from one module's checkpoint tensors (A8 schemes)."""
    if "weight_zero_point" in t:
        raise ValueError(f"{name}: an A8 checkpoint with weight_zero_point -- the int8 GEMM has no weight zero-point "
                         "term (W8A8, INT8 and W4A8 weights are symmetric)")
    w, N, K, packed = _levels_and_shape(name, t)
    scale = t["weight_scale"].to(torch.float32)            # bf16 / fp16 -> fp32 is exact
    G = scale.shape[1]
    if scale.shape[0] != N or G not in (1, (K + GROUP - 1) // GROUP):
        raise ValueError(f"{name}: weight_scale {tuple(scale.shape)} is neither channel-wise nor groups of {GROUP} "
                         f"over {K} columns")
    col_perm = None
    if "weight_g_idx" in t:
        g = _group_of_columns(name, t, K, G)
        perm = torch.argsort(g, stable=True)
        if not torch.equal(g[perm], torch.arange(K, device=g.device) // GROUP):
            raise ValueError(f"{name}: weight_g_idx groups are not {GROUP} columns each")
        q = unpack_int4(w, K) if packed else w
        q = q[:, perm]
        w = pack_int4(q) if packed else q.contiguous()
        col_perm = perm.to(torch.int32)
    return QuantizedLinear(K, N, w, scale, act_symmetric, col_perm=col_perm, bias=bias)


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


def load_quantized(path, device="cuda", dtype: Optional[torch.dtype] = None) -> nn.Module:
    """Rebuild the model a ``save_pretrained`` / ``_save_compressed`` directory describes (one file or shards) with
    ``QuantizedLinear``s (A8 schemes) or dequantised ``nn.Linear``s (A16 schemes) in place of its quantized Linears.

    Refused with ``ValueError`` / ``NotImplementedError``: float-quantized checkpoints, routed-expert banks (a grouped
    expert GEMM does not exist yet), any ``input_activations`` block other than 8-bit dynamic per-token, and an A8
    checkpoint that carries ``weight_zero_point``."""
    from transformers import AutoConfig, AutoModelForCausalLM

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
    experts = sorted(m for m in quant if _EXPERT_RE.search(m + "."))
    if experts:
        raise NotImplementedError(f"{path}: routed-expert weights ({experts[0]}, ... {len(experts)} modules) need a "
                                  "grouped expert GEMM, which this runtime does not have yet")

    mdtype = _model_dtype(cfg, dtype)
    model_type = cfg.pop("model_type")
    for k in ("torch_dtype", "dtype", "transformers_version"):
        cfg.pop(k, None)
    config = AutoConfig.for_model(model_type, **cfg)
    dev = torch.device(device)
    with dev:
        model = AutoModelForCausalLM.from_config(config, torch_dtype=mdtype)
    model.eval()

    missing, unexpected = model.load_state_dict(dense, strict=False)
    if unexpected:
        raise ValueError(f"{path}: unexpected tensors {sorted(unexpected)[:8]}")
    allowed = {f"{m}.weight" for m in quant}
    bad = sorted(set(missing) - allowed)
    if bad:
        raise ValueError(f"{path}: tensors missing from the checkpoint: {bad[:8]}")

    a8 = acts is not None
    act_symmetric = bool(acts.get("symmetric", True)) if a8 else True
    for name, t in quant.items():
        lin = model.get_submodule(name)
        if not isinstance(lin, nn.Linear):
            raise ValueError(f"{path}: {name} is quantized in the checkpoint but is a {type(lin).__name__} here")
        t = {k: v.to(dev) for k, v in t.items()}
        if a8:
            new = quantized_linear_from_tensors(name, t, act_symmetric, bias=lin.bias.data if lin.bias is not None
                                                else None)
        else:
            W = dequantized_weight(name, t, mdtype)
            if tuple(W.shape) != tuple(lin.weight.shape):
                raise ValueError(f"{path}: {name} has shape {tuple(W.shape)} in the checkpoint, "
                                 f"{tuple(lin.weight.shape)} in the model")
            lin.weight.data = W
            continue
        if (new.out_features, new.in_features) != tuple(lin.weight.shape):
            raise ValueError(f"{path}: {name} has shape {(new.out_features, new.in_features)} in the checkpoint, "
                             f"{tuple(lin.weight.shape)} in the model")
        parent_name, _, leaf = name.rpartition(".")
        setattr(model.get_submodule(parent_name) if parent_name else model, leaf, new)
    model._qt_checkpoint = {"path": str(path), "format": fmt, "input_activations": acts}
    return model
