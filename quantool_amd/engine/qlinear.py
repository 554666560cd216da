"""Reading back the checkpoints this project writes, and running them.

``load_quantized`` rebuilds the model from ``config.json`` and the dense tensors, then puts in place of every quantized
Linear either

* a ``QuantizedLinear`` (W8A8 / INT8 / W4A8: the checkpoint's 8-bit dynamic per-token ``input_activations`` block):
  activations are quantised per row on the fly and multiplied with the stored integer weights on the int8 MFMA
  (``qt_quantize_tokens_i8`` + ``qt_gemm_i8``, include/quantool_amd.h), as a served W8A8 runtime does; or
* a plain ``nn.Linear`` holding the dequantised weight ``(q - zp) * scale`` (W4A16, W4A16_ASYM, W8A16), computed once in
  fp32 from the STORED scale and rounded once to the model dtype (the default, ``a16="dequantized"``); or
* with ``a16="packed"``, a ``WeightOnlyLinear`` that keeps the stored integer weights on the device: decode-sized inputs
  (M <= ``skinny_max_m`` rows) run the GEMV ``qt_gemm_wq_skinny``, larger ones dequantise the weight into a transient
  buffer (``qt_dequantize_weight``, bit-identical to the dequantised ``nn.Linear``) and call ``F.linear``.

Routed-expert banks (transformers >= 5 fuses them: ``<layer>.mlp.experts.gate_up_proj [E, 2I, H]`` / ``down_proj
[E, H, I]``) are written per expert by ``sequential.expert_bank_checkpoint_names`` (Mixtral:
``<layer>.block_sparse_moe.experts.{e}.w1 / w3 / w2``, otherwise ``<layer>.mlp.experts.{e}.gate_proj / up_proj /
down_proj``).  The loader inverts that write: A16 experts are dequantised into the fused parameters
(``gate_up_proj[e] = cat(w1, w3)``, ``down_proj[e] = w2``), or with ``a16_experts="packed"`` replace the bank with a
``WeightOnlyExperts`` on the stored integer weights (``qt_gemm_wq_grouped`` at decode); A8 experts replace the bank with
a ``QuantizedExperts`` that runs the routed rows on the grouped int8 GEMM (``qt_moe_route`` + ``qt_gemm_i8_grouped`` +
``qt_moe_combine``).

Loading needs no GPU: every load-time step (int4 unpacking, the column permutation of actorder ``group``, the per-group
weight sums) is integer torch work on whatever device the model is built on.  Only ``QuantizedLinear.forward``,
``QuantizedExperts.forward``, ``WeightOnlyLinear.forward`` and ``WeightOnlyExperts.forward`` on device tensors need
the HIP library.
"""
from __future__ import annotations

import json
import re
from pathlib import Path
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .serialization import load_state

GROUP = 128   # the W4A8 group size the GEMM takes
_LEAVES = ("weight", "weight_packed", "weight_scale", "weight_zero_point", "weight_g_idx", "weight_shape")
# per-expert names expert_bank_checkpoint_names writes (<bank>.experts.{e}.<proj>)
_EXPERT_RE = re.compile(r"\.experts\.\d+\.")
# <bank>.{e}.<proj> -- a per-expert module name, split
_EXPERT_NAME = re.compile(r"^(?P<bank>.+\.experts)\.(?P<e>\d+)\.(?P<proj>[^.]+)$")


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


class WeightOnlyLinear(nn.Module):
    """One W4A16 / W4A16_ASYM / W8A16 Linear of a checkpoint on its stored integer weights.

    ``forward(x)`` with M = rows of ``x``: M <= ``skinny_max_m`` runs ``qt_gemm_wq_skinny`` (the weights read once,
    dequantised on chip; fp32 sums in the kernel's own fixed order); otherwise ``qt_dequantize_weight`` fills a transient
    dense weight -- bit-identical to the default loader's ``nn.Linear.weight`` -- and ``F.linear`` runs on it, so the
    output equals that ``nn.Linear``'s to the bit.  On CPU tensors ``forward`` is ``F.linear`` on ``dequantized_weight``.

    Buffers: ``weight_packed`` int32 [N, ceil(K/8)] (int4) or ``weight`` int8 [N, K]; ``weight_scale`` fp32 [N, G];
    ``weight_zero_point`` int8 [N, G] (optional); ``g_idx`` int32 [K] (optional, actorder ``group``); ``bias``
    (optional, model dtype).  Columns stay in their original order."""

    # Decode GEMV up to this many rows, dequantise + F.linear above: at 16 rows the GEMV is still faster than the
    # dequantise + F.linear pair on every measured Llama-3-8B shape.
    skinny_max_m = 16

    def __init__(self, in_features: int, out_features: int, weight: torch.Tensor, weight_scale: torch.Tensor,
                 weight_zero_point: Optional[torch.Tensor] = None, g_idx: Optional[torch.Tensor] = None,
                 bias: Optional[torch.Tensor] = None):
        super().__init__()
        self.in_features = int(in_features)
        self.out_features = int(out_features)
        self.int4 = weight.dtype == torch.int32
        self.register_buffer("weight_packed" if self.int4 else "weight", weight.contiguous())
        self.register_buffer("weight_scale", weight_scale.to(torch.float32).contiguous())
        self.register_buffer("weight_zero_point", None if weight_zero_point is None
                             else weight_zero_point.to(torch.int8).contiguous())
        self.register_buffer("g_idx", None if g_idx is None else g_idx.to(torch.int32).contiguous())
        self.register_buffer("bias", None if bias is None else bias.contiguous())

    @property
    def qweight(self) -> torch.Tensor:
        return self.weight_packed if self.int4 else self.weight

    def checkpoint_tensors(self) -> Dict[str, torch.Tensor]:
        """The module's weight as the checkpoint leaves ``dequantized_weight`` reads."""
        t = {"weight_packed" if self.int4 else "weight": self.qweight, "weight_scale": self.weight_scale,
             "weight_shape": torch.tensor([self.out_features, self.in_features])}
        if self.weight_zero_point is not None:
            t["weight_zero_point"] = self.weight_zero_point
        if self.g_idx is not None:
            t["weight_g_idx"] = self.g_idx
        return t

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"weights={'int4' if self.int4 else 'int8'}, groups={self.weight_scale.shape[1]}, "
                f"zero_point={self.weight_zero_point is not None}, g_idx={self.g_idx is not None}, "
                f"bias={self.bias is not None}, skinny_max_m={self.skinny_max_m}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        bias = None if self.bias is None else self.bias.to(x.dtype)
        if not x.is_cuda:
            return F.linear(x, dequantized_weight("WeightOnlyLinear", self.checkpoint_tensors(), x.dtype), bias)
        from ..hip import ops

        x2 = x.reshape(-1, self.in_features)
        M = x2.shape[0]
        if 1 <= M <= min(self.skinny_max_m, ops.SKINNY_MAX_M):
            if x2.stride(1) != 1:
                x2 = x2.contiguous()
            y = ops.gemm_wq_skinny(x2, self.qweight, self.weight_scale, zp_w=self.weight_zero_point, g_idx=self.g_idx,
                                   bias=bias)
            return y.reshape(*x.shape[:-1], self.out_features)
        W = ops.dequantize_weight(self.qweight, self.weight_scale, K=self.in_features, zp_w=self.weight_zero_point,
                                  g_idx=self.g_idx, dtype=x.dtype)
        return F.linear(x, W, bias)


class QuantizedExperts(nn.Module):
    """A W8A8 / INT8 / W4A8 routed-expert bank: ``forward(hidden_states, top_k_index, top_k_weights)`` as
    transformers' ``MixtralExperts`` with its two ``F.linear`` calls on the int8 GEMM.

    The routed rows are ordered by expert (``qt_moe_route``); the T tokens are quantised once per token and the gate_up
    GEMM gathers them by token; ``act_fn(gate) * up`` runs in torch as the fused module does; the routed rows are
    quantised per row and the down GEMM reads them in place; ``qt_moe_combine`` sums each token's weighted rows in
    ascending expert order, rounding as ``index_add_`` does.  include/quantool_amd.h states every step.

    Buffers: ``gate_up`` int8 [E, 2I, H] or packed int4 int32 [E, 2I, ceil(H/8)] (rows [0, I) gate, [I, 2I) up),
    ``gate_up_scale`` fp32 [E, 2I, G], ``gate_up_wsum`` int32 [E, 2I, G]; ``down`` int8 [E, H, I] or int32
    [E, H, ceil(I/8)], ``down_scale`` fp32 [E, H, G'], ``down_wsum`` int32 [E, H, G']."""

    def __init__(self, hidden_size: int, intermediate_size: int, gate_up: torch.Tensor, gate_up_scale: torch.Tensor,
                 down: torch.Tensor, down_scale: torch.Tensor, act_fn: nn.Module, act_symmetric: bool):
        super().__init__()
        self.num_experts = int(gate_up.shape[0])
        self.hidden_dim = int(hidden_size)
        self.intermediate_dim = int(intermediate_size)
        self.act_fn = act_fn
        self.act_symmetric = bool(act_symmetric)
        self.int4 = gate_up.dtype == torch.int32
        for name, w, s, K in (("gate_up", gate_up, gate_up_scale, self.hidden_dim),
                              ("down", down, down_scale, self.intermediate_dim)):
            E, N = w.shape[:2]
            levels = unpack_int4(w.reshape(E * N, -1), K) if self.int4 else w.reshape(E * N, K)
            G = s.shape[2]
            self.register_buffer(name, w.contiguous())
            self.register_buffer(f"{name}_scale", s.to(torch.float32).contiguous())
            self.register_buffer(f"{name}_wsum", group_sums(levels, G).reshape(E, N, G))

    def extra_repr(self) -> str:
        return (f"num_experts={self.num_experts}, hidden={self.hidden_dim}, intermediate={self.intermediate_dim}, "
                f"weights={'int4 g128' if self.int4 else 'int8'}, "
                f"groups=({self.gate_up_scale.shape[2]}, {self.down_scale.shape[2]}), "
                f"act={'sym' if self.act_symmetric else 'asym'} int8 per-token")

    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor):
        from ..hip import ops

        x = hidden_states.reshape(-1, self.hidden_dim)
        if x.stride(1) != 1:
            x = x.contiguous()
        offsets, src_token, _, row_of = ops.moe_route(top_k_index, self.num_experts)
        sym = self.act_symmetric
        Xq, s_x, zp_x = ops.quantize_tokens_i8(x, symmetric=sym)
        gu = ops.gemm_i8_grouped(Xq, s_x, self.gate_up, self.gate_up_scale, offsets, row_idx=src_token,
                                 K=self.hidden_dim, zp_x=zp_x, wsum=None if sym else self.gate_up_wsum,
                                 out_dtype=x.dtype)
        gate, up = gu.chunk(2, dim=-1)
        h = self.act_fn(gate) * up
        Hq, s_h, zp_h = ops.quantize_tokens_i8(h, symmetric=sym)
        y = ops.gemm_i8_grouped(Hq, s_h, self.down, self.down_scale, offsets, K=self.intermediate_dim, zp_x=zp_h,
                                wsum=None if sym else self.down_wsum, out_dtype=x.dtype)
        return ops.moe_combine(y, row_of, top_k_weights).reshape(hidden_states.shape)


class WeightOnlyExperts(nn.Module):
    """A W4A16 / W4A16_ASYM / W8A16 routed-expert bank on its stored integer weights: ``forward(hidden_states,
    top_k_index, top_k_weights)`` as the fused transformers bank it replaces.

    With T = rows of ``hidden_states`` (known on the host) and 1 <= T <= ``grouped_max_tokens``: ``qt_moe_route`` orders
    the routed rows by expert, the gate_up GEMV (``qt_gemm_wq_grouped``) gathers them by token, ``act_fn(gate) * up``
    runs in torch as the fused module does, the down GEMV reads the routed rows in place and ``qt_moe_combine`` sums
    each token's weighted rows in ascending expert order.  Only the experts that were hit are read, and nothing waits on
    the host.  Larger T: both banks are dequantised into transient [E, 2I, H] / [E, H, I] tensors
    (``qt_dequantize_weight``, bit-identical to the dense bank ``a16_experts="dequantized"`` loads) and the bank's own
    transformers forward runs on them (honouring ``config._experts_implementation``), so the output equals the dense
    bank's to the bit.  On CPU tensors ``forward`` is that bank forward on ``dequantized_weight``.

    Buffers: ``gate_up`` packed int4 int32 [E, 2I, ceil(H/8)] or int8 [E, 2I, H] (rows [0, I) gate, [I, 2I) up),
    ``gate_up_scale`` fp32 [E, 2I, G], ``gate_up_zero_point`` int8 [E, 2I, G] (optional), ``gate_up_g_idx`` int32
    [E, H] (optional, actorder ``group``); ``down`` int32 [E, H, ceil(I/8)] or int8 [E, H, I] and its ``down_scale``,
    ``down_zero_point``, ``down_g_idx`` likewise.  Columns stay in the checkpoint's order.

    ``bank`` is the fused module replaced: its ``gate_up_proj`` / ``down_proj`` are swapped for empty stand-ins and it
    is kept (not as a submodule) for its forward alone."""

    # Grouped GEMV up to this many tokens, dequantise + the bank's forward above.  At Mixtral-8x7B's shapes the GEMV pair
    # re-reads an expert's weights once per 16 of its rows and still beats the dequantise path (2.7 ms) up to T = 192;
    # at 128 it takes 1.2 ms.
    grouped_max_tokens = 128

    def __init__(self, bank: nn.Module, gate_up: torch.Tensor, gate_up_scale: torch.Tensor, down: torch.Tensor,
                 down_scale: torch.Tensor, *, gate_up_zero_point: Optional[torch.Tensor] = None,
                 gate_up_g_idx: Optional[torch.Tensor] = None, down_zero_point: Optional[torch.Tensor] = None,
                 down_g_idx: Optional[torch.Tensor] = None):
        super().__init__()
        E, I2, H = bank.gate_up_proj.shape
        self.num_experts, self.hidden_dim, self.intermediate_dim = int(E), int(H), int(I2) // 2
        self.act_fn = bank.act_fn
        self.int4 = gate_up.dtype == torch.int32
        for name, w, s, zp, gi in (("gate_up", gate_up, gate_up_scale, gate_up_zero_point, gate_up_g_idx),
                                   ("down", down, down_scale, down_zero_point, down_g_idx)):
            self.register_buffer(name, w.contiguous())
            self.register_buffer(f"{name}_scale", s.to(torch.float32).contiguous())
            self.register_buffer(f"{name}_zero_point", None if zp is None else zp.to(torch.int8).contiguous())
            self.register_buffer(f"{name}_g_idx", None if gi is None else gi.to(torch.int32).contiguous())
        p = bank.gate_up_proj
        for n in ("gate_up_proj", "down_proj"):
            setattr(bank, n, nn.Parameter(torch.empty(0, dtype=p.dtype, device=p.device), requires_grad=False))
        self.__dict__["_bank"] = bank

    def extra_repr(self) -> str:
        return (f"num_experts={self.num_experts}, hidden={self.hidden_dim}, intermediate={self.intermediate_dim}, "
                f"weights={'int4' if self.int4 else 'int8'}, "
                f"groups=({self.gate_up_scale.shape[2]}, {self.down_scale.shape[2]}), "
                f"zero_point={self.gate_up_zero_point is not None}, g_idx={self.gate_up_g_idx is not None}, "
                f"grouped_max_tokens={self.grouped_max_tokens}")

    def _part(self, part: str):
        return (getattr(self, part), getattr(self, f"{part}_scale"), getattr(self, f"{part}_zero_point"),
                getattr(self, f"{part}_g_idx"), self.hidden_dim if part == "gate_up" else self.intermediate_dim)

    def dense_weight(self, part: str, dtype: torch.dtype) -> torch.Tensor:
        """The ``part`` ("gate_up" / "down") bank dequantised, [E, N, K] in ``dtype``: the dense bank's parameter."""
        w, s, zp, gi, K = self._part(part)
        E, N = w.shape[:2]
        if not w.is_cuda:
            def leaves(e):
                t = {"weight_packed" if self.int4 else "weight": w[e], "weight_scale": s[e],
                     "weight_shape": torch.tensor([N, K])}
                if zp is not None:
                    t["weight_zero_point"] = zp[e]
                if gi is not None:
                    t["weight_g_idx"] = gi[e]
                return t

            return torch.stack([dequantized_weight(f"{part}[{e}]", leaves(e), dtype) for e in range(E)])
        from ..hip import ops

        out = torch.empty((E, N, K), dtype=dtype, device=w.device)
        if gi is None:                      # one call over the stacked [E N, .] rows
            ops.dequantize_weight(w.view(E * N, -1), s.view(E * N, -1), K=K,
                                  zp_w=None if zp is None else zp.view(E * N, -1), dtype=dtype, out=out.view(E * N, K))
        else:
            for e in range(E):
                ops.dequantize_weight(w[e], s[e], K=K, zp_w=None if zp is None else zp[e], g_idx=gi[e], dtype=dtype,
                                      out=out[e])
        return out

    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor):
        x = hidden_states.reshape(-1, self.hidden_dim)
        T = x.shape[0]
        if not x.is_cuda or not 1 <= T <= self.grouped_max_tokens:
            dense = {"gate_up_proj": self.dense_weight("gate_up", hidden_states.dtype),
                     "down_proj": self.dense_weight("down", hidden_states.dtype)}
            return torch.func.functional_call(self._bank, dense, (hidden_states, top_k_index, top_k_weights))
        from ..hip import ops

        if x.stride(1) != 1:
            x = x.contiguous()
        offsets, src_token, _, row_of = ops.moe_route(top_k_index, self.num_experts)
        w, s, zp, gi, K = self._part("gate_up")
        gu = ops.gemm_wq_grouped(x, w, s, offsets, row_idx=src_token, K=K, zp_w=zp, g_idx=gi)
        gate, up = gu.chunk(2, dim=-1)
        h = self.act_fn(gate) * up
        w, s, zp, gi, K = self._part("down")
        y = ops.gemm_wq_grouped(h, w, s, offsets, K=K, zp_w=zp, g_idx=gi)
        return ops.moe_combine(y, row_of, top_k_weights).reshape(hidden_states.shape)


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


def weight_only_linear_from_tensors(name: str, t: Dict[str, torch.Tensor],
                                    bias: Optional[torch.Tensor] = None) -> WeightOnlyLinear:
    """A ``WeightOnlyLinear`` from one module's checkpoint tensors (A16 schemes, ``a16="packed"``)."""
    w, N, K, packed = _levels_and_shape(name, t)
    scale = t["weight_scale"].to(torch.float32)            # bf16 / fp16 -> fp32 is exact
    G = scale.shape[1]
    if scale.dim() != 2 or scale.shape[0] != N or G not in (1, (K + GROUP - 1) // GROUP):
        raise ValueError(f"{name}: weight_scale {tuple(scale.shape)} is neither channel-wise nor groups of {GROUP} "
                         f"over {K} columns; load it with a16='dequantized'")
    zp = t.get("weight_zero_point")
    if zp is not None:
        if tuple(zp.shape) != (N, G) or zp.is_floating_point() or int(zp.min()) < -128 or int(zp.max()) > 127:
            raise ValueError(f"{name}: weight_zero_point must be integers in [-128, 127] of shape {(N, G)}")
    g_idx = _group_of_columns(name, t, K, G).to(torch.int32) if "weight_g_idx" in t else None
    return WeightOnlyLinear(K, N, w, scale, weight_zero_point=zp, g_idx=g_idx, bias=bias)


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
    per-expert tensor out of ``dense`` / ``quant``.  Returns ({bank: {e: {proj: ("q", leaves) | ("dense", tensor)}}},
    {checkpoint prefix: model prefix}).  proj is gate_proj / up_proj / down_proj."""
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
    return banks, found


def _load_bank(path, bank_name: str, bank: nn.Module, experts: Dict[int, Dict[str, tuple]], a8: bool,
               act_symmetric: bool, mdtype: torch.dtype, dev, packed_experts: bool = False) -> Optional[nn.Module]:
    """Fill (A16, dense) or replace (A8: the returned ``QuantizedExperts``; A16 with ``packed_experts``: the returned
    ``WeightOnlyExperts``) one fused bank from its experts."""
    gu, dn = bank.gate_up_proj, bank.down_proj
    E, I2, H = gu.shape
    I = I2 // 2
    roles = ("gate_proj", "up_proj", "down_proj")
    missing = [f"{e}.{r}" for e in range(E) for r in roles if r not in experts.get(e, {})]
    if missing:
        raise ValueError(f"{path}: {bank_name}: experts missing from the checkpoint: {missing[:6]}")
    kinds = {experts[e][r][0] for e in range(E) for r in roles}
    if len(kinds) > 1:
        raise ValueError(f"{path}: {bank_name} is only partly quantized (some expert Linears are dense); the bank "
                         "runs as one unit, so every expert Linear must share a scheme")
    want = {"gate_proj": (I, H), "up_proj": (I, H), "down_proj": (H, I)}

    def shape_check(e, r, shape):
        if tuple(shape) != want[r]:
            raise ValueError(f"{path}: {bank_name}.{e}.{r} has shape {tuple(shape)} in the checkpoint, {want[r]} in "
                             "the model")

    if kinds == {"dense"} or not (a8 or packed_experts):
        for e in range(E):
            W = {}
            for r in roles:
                kind, v = experts[e][r]
                W[r] = v.to(dev).to(mdtype) if kind == "dense" else dequantized_weight(
                    f"{bank_name}.{e}.{r}", {k: t.to(dev) for k, t in v.items()}, mdtype)
                shape_check(e, r, W[r].shape)
            gu.data[e] = torch.cat([W["gate_proj"], W["up_proj"]], 0)
            dn.data[e] = W["down_proj"]
        return None

    # stacked[part] = (weights, scales, zero-points or None, g_idx [E, K] or None), gate rows before up rows
    stacked = {}
    for part, rs in (("gate_up", ("gate_proj", "up_proj")), ("down", ("down_proj",))):
        ws, ss, zs, gs = [], [], [], []
        for e in range(E):
            for r in rs:
                name = f"{bank_name}.{e}.{r}"
                t = {k: v.to(dev) for k, v in experts[e][r][1].items()}
                if not a8:                 # A16: the checks and buffers of a WeightOnlyLinear
                    m = weight_only_linear_from_tensors(name, t)
                    shape_check(e, r, (m.out_features, m.in_features))
                    ws.append(m.qweight)
                    ss.append(m.weight_scale)
                    zs.append(m.weight_zero_point)
                    gs.append(m.g_idx)
                    continue
                if "weight_g_idx" in t:
                    raise NotImplementedError(f"{path}: {name}: A8 expert weights with weight_g_idx (actorder "
                                              "'group') need a per-expert column permutation, which the grouped "
                                              "GEMM does not take; quantise with actorder 'static'")
                if "weight_zero_point" in t:
                    raise ValueError(f"{path}: {name}: an A8 checkpoint with weight_zero_point -- the int8 GEMM has "
                                     "no weight zero-point term (W8A8, INT8 and W4A8 weights are symmetric)")
                w, N, K, _ = _levels_and_shape(name, t)
                shape_check(e, r, (N, K))
                scale = t["weight_scale"].to(torch.float32)
                if scale.shape[0] != N or scale.shape[1] not in (1, (K + GROUP - 1) // GROUP):
                    raise ValueError(f"{path}: {name}: weight_scale {tuple(scale.shape)} is neither channel-wise nor "
                                     f"groups of {GROUP} over {K} columns")
                ws.append(w)
                ss.append(scale)
                zs.append(None)
                gs.append(None)
        if (len({w.dtype for w in ws}) > 1 or len({s.shape[1] for s in ss}) > 1 or len({z is None for z in zs}) > 1
                or len({g is None for g in gs}) > 1):
            raise ValueError(f"{path}: {bank_name}: the {part} weights of the experts mix formats or group counts")
        per = len(rs)
        g_idx = None
        if gs[0] is not None:
            for e in range(E):
                if not all(torch.equal(gs[e * per], g) for g in gs[e * per:(e + 1) * per]):
                    raise ValueError(f"{path}: {bank_name}.{e}: gate_proj and up_proj group their columns differently "
                                     "(weight_g_idx); the grouped GEMV takes one column grouping per expert")
            g_idx = torch.stack(gs[::per])

        def stack(xs):
            return None if xs[0] is None else torch.stack([torch.cat(xs[e * per:(e + 1) * per], 0) for e in range(E)])

        stacked[part] = (stack(ws), stack(ss), stack(zs), g_idx)
    if stacked["gate_up"][0].dtype != stacked["down"][0].dtype:
        raise ValueError(f"{path}: {bank_name}: gate_up and down weights differ in format")
    (gu_w, gu_s, gu_z, gu_g), (dn_w, dn_s, dn_z, dn_g) = stacked["gate_up"], stacked["down"]
    if a8:
        return QuantizedExperts(H, I, gu_w, gu_s, dn_w, dn_s, bank.act_fn, act_symmetric)
    return WeightOnlyExperts(bank, gu_w, gu_s, dn_w, dn_s, gate_up_zero_point=gu_z, gate_up_g_idx=gu_g,
                             down_zero_point=dn_z, down_g_idx=dn_g)


A16_MODES = ("dequantized", "packed")


def load_quantized(path, device="cuda", dtype: Optional[torch.dtype] = None, a16: str = "dequantized",
                   a16_experts: str = "dequantized") -> nn.Module:
    """Rebuild the model a ``save_pretrained`` / ``_save_compressed`` directory describes (one file or shards) with
    ``QuantizedLinear``s (A8 schemes) or, for A16 schemes, dequantised ``nn.Linear``s (``a16="dequantized"``, the
    default) or ``WeightOnlyLinear``s on the stored integer weights (``a16="packed"``) in place of its quantized Linears.
    A8 checkpoints ignore ``a16`` and ``a16_experts``.  In packed mode A16 routed-expert banks are still dequantised
    into the fused bank unless ``a16_experts="packed"`` (which needs ``a16="packed"``) replaces each with a
    ``WeightOnlyExperts``; ``model._qt_checkpoint`` then records ``"a16": "packed"``, the banks left dense under
    ``"dense_expert_banks"`` and, with ``a16_experts="packed"``, the packed ones under ``"packed_expert_banks"``.

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

    banks, experts = _expert_banks(path, model, model_type, dense, quant)
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
            parent_name, _, leaf = bank_name.rpartition(".")
            setattr(model.get_submodule(parent_name) if parent_name else model, leaf, new)
    for name, t in quant.items():
        lin = model.get_submodule(name)
        if not isinstance(lin, nn.Linear):
            raise ValueError(f"{path}: {name} is quantized in the checkpoint but is a {type(lin).__name__} here")
        t = {k: v.to(dev) for k, v in t.items()}
        if a8:
            new = quantized_linear_from_tensors(name, t, act_symmetric, bias=lin.bias.data if lin.bias is not None
                                                else None)
        elif a16 == "packed":
            new = weight_only_linear_from_tensors(name, t, bias=lin.bias.data if lin.bias is not None else None)
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
    from .sequential import expert_bank_module_renames, rename_module_prefix as _rename

    inverse = {v: k for k, v in expert_bank_module_renames(banks, model_type).items()}
    ignore = [_rename(n, inverse) for n in qcfg.get("ignore") or []]
    model._qt_checkpoint = {"path": str(path), "format": fmt, "input_activations": acts, "ignore": ignore}
    if not a8 and a16 == "packed":
        model._qt_checkpoint["a16"] = "packed"
        model._qt_checkpoint["dense_expert_banks"] = sorted(set(experts) - set(replaced))
        if packed_experts:
            model._qt_checkpoint["packed_expert_banks"] = sorted(replaced)
    return model
