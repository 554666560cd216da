"""The modules ``load_quantized`` (engine/qlinear.py) installs in place of a checkpoint's quantized Linears,
routed-expert banks and, on request, Llama-style MLPs of three quantized Linears (``QuantizedMLP``).  Each keeps the
checkpoint's integer weights in registered buffers; the weight-only pair hands them to the kernels, to ``dequantize``
and back to checkpoint tensors as one ``StoredWeight`` (engine/stored_weight.py).  Only ``forward`` on device tensors
needs the HIP library."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .stored_weight import StoredWeight, group_sums, unpack_int4


def _rows(x: torch.Tensor, K: int) -> torch.Tensor:
    """x [..., K] as the [M, K] rows with unit column stride the kernels read (a copy only where no view gives them)."""
    x2 = x.reshape(-1, K)
    return x2 if x2.stride(1) == 1 else x2.contiguous()


class QuantizedLinear(nn.Module):
    """One W8A8 / INT8 / W4A8 Linear of a checkpoint: ``forward(x)`` quantises the rows of ``x`` to int8 (per token,
    dynamic) and runs the int8 x int8 GEMM with the checkpoint's weight scales.

    Buffers: ``weight`` int8 [N, K] or packed int4 int32 [N, ceil(K/8)] (columns permuted by ``col_perm`` when the
    checkpoint used actorder ``group``), ``weight_scale`` fp32 [N, G], ``wsum`` int32 [N, G], ``col_perm`` int32 [K]
    (optional), ``bias`` (optional, model dtype).

    M = rows of ``x``: 1 <= M <= ``skinny_max_m`` runs the decode form ``qt_gemm_i8_skinny`` (the weights read once, 16
    output columns per workgroup), larger M the 128 x 128-tile ``qt_gemm_i8``.  The two agree to the bit, so the
    attribute changes speed alone; 0 sends every M to the tiled kernel.  M >= ``ring_min_m`` (when that is not 0) runs
    an int8 weight with one scale group on the 256 x 256 LDS-ring kernel ``qt_gemm_i8_ring`` where
    ``ops.gemm_i8_ring_supported`` holds; it agrees with the tiled kernel to the bit as well, and 0 never uses it.
    M >= ``ring_w4_min_m`` (when that is not 0) runs a packed int4 weight with one scale per 128 columns on the same
    ring with packed weight panels, ``qt_gemm_i8_ring_w4``, where ``ops.gemm_i8_ring_w4_supported`` holds: bit-identical
    again, and 0 never uses it.
    Between the two, ``skinny_max_m`` < M <= ``mid_max_m`` runs the weight-streaming ``qt_gemm_i8_mid`` (both weight
    formats, bit-identical too) on a Linear with ``in_features`` >= ``mid_min_k`` and, when ``mid_max_n`` is not 0,
    ``out_features`` <= ``mid_max_n``, where ``ops.gemm_i8_mid_supported`` holds; ``mid_max_m`` = 0 never uses it.
    Below the ring, ``splitk_min_m`` <= M < ``ring_min_m`` (or any M >= ``splitk_min_m`` when ``ring_min_m`` is 0) runs an
    int8 weight with one scale group and ``in_features`` >= ``splitk_min_k`` on the ring's tile over S k-ranges plus an
    int32 reduce pass, ``qt_splitk_gemm_i8``, where ``ops.splitk_gemm_i8_supported`` holds: bit-identical again, and
    ``splitk_min_m`` = 0 never uses it."""

    # Decode GEMV up to this many rows: the measured crossover.
    skinny_max_m = 16
    # LDS-ring GEMM from this many rows (0: never): the smallest measured M from which the ring is no slower than the
    # tiled kernel on all three Llama-3-8B shapes, in both runs.
    ring_min_m = 2048
    # The same for packed int4 weights (qt_gemm_i8_ring_w4; 0: never): the smallest of M = 2048, 4096, 8192 at which the
    # ring beats the tiled kernel on all three Llama-3-8B shapes, in both runs, by more than the tiled kernel's largest
    # run-to-run spread in those runs (3.9 %).  At 2048 down loses (0.74x), at 4096 q/k/v wins by 1.4 / 1.8 % only
    # (gate/up 1.26x, down 1.40x), at 8192 the margins are 1.27 - 1.37x.  Never below 2048.
    ring_w4_min_m = 8192
    # Mid-M GEMM up to this many rows (0: never), up to this many output features (0: no bound) and from this many
    # input features: the measured crossovers against the tiled kernel.  N = 28672 (gate/up) loses from
    # 17 rows on; K = 256 would qualify, but Linears below 512 are launch-bound and stay on the tiled kernel.
    # 128 rests on a tie on one shape (q/k/v W8A8: 52.0 against 51.7 / 51.4 us); the next clear win is 96 (1.20x).
    mid_max_m = 128
    mid_max_n = 6144
    mid_min_k = 512
    # Split-K GEMM from this many rows up to the ring (0: never) and from this many input features: the loosest measured
    # values for which every admitted (shape, M) cell is no slower than the tiled kernel in both runs.
    # K = 14336 (down) and 28672 (70B's down) win at every M from 129 to 2047: 1.56 - 2.85x and 1.50 - 3.17x.  K = 4096
    # does not qualify: q/k/v wins everywhere (1.05 - 1.58x) and o up to 1536 rows (1.02 - 1.97x), but o at 2047 rows
    # loses (0.96 / 0.97x) and gate/up ties or loses at 129, 320, 384 and 640 rows (0.97 - 1.00x in one run or both);
    # there is no bound on M from above or on N that would keep them out, so they stay on the tiled kernel.
    splitk_min_m = 129
    splitk_min_k = 14336

    def __init__(self, in_features: int, out_features: int, weight: torch.Tensor, weight_scale: torch.Tensor,
                 act_symmetric: bool, col_perm: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None):
        super().__init__()
        self.in_features = int(in_features)
        self.out_features = int(out_features)
        self.act_symmetric = bool(act_symmetric)
        self.int4 = weight.dtype == torch.int32
        levels = unpack_int4(weight, in_features) if self.int4 else weight
        self.register_buffer("weight", weight.contiguous())
        self.register_buffer("weight_scale", weight_scale.to(torch.float32).contiguous())
        self.register_buffer("wsum", group_sums(levels, weight_scale.shape[1]))
        self.register_buffer("col_perm", None if col_perm is None else col_perm.to(torch.int32).contiguous())
        self.register_buffer("bias", None if bias is None else bias.contiguous())

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"weights={'int4 g128' if self.int4 else 'int8'}, groups={self.weight_scale.shape[1]}, "
                f"act={'sym' if self.act_symmetric else 'asym'} int8 per-token, "
                f"col_perm={self.col_perm is not None}, bias={self.bias is not None}, "
                f"ring_w4_min_m={self.ring_w4_min_m}")

    # A ``SharedRows`` a ``QuantizingRMSNorm`` in front of this Linear fills (None, the default: nobody does).
    rows_from = None

    def quantize_rows(self, x: torch.Tensor):
        """The rows of ``x`` as this Linear's GEMMs take them: (Xq int8 [M, K], s_x, zp_x or None).  Where a norm in
        front has quantised exactly this tensor already (``rows_from``), its rows are taken."""
        if self.rows_from is not None:
            rows = self.rows_from.take(x)
            if rows is not None:
                return rows
        from ..hip import ops

        return ops.quantize_tokens_i8(_rows(x, self.in_features), symmetric=self.act_symmetric, col_perm=self.col_perm)

    def gemm_rows(self, Xq: torch.Tensor, s_x: torch.Tensor, zp_x: Optional[torch.Tensor],
                  out_dtype: torch.dtype) -> torch.Tensor:
        """Quantised rows (``quantize_rows``, or any pass that equals it) times the weight: [M, N] in ``out_dtype``, on
        the GEMM form the class docstring gives for M."""
        from ..hip import ops

        bias = None if self.bias is None else self.bias.to(out_dtype)
        M = Xq.shape[0]
        if 1 <= M <= min(self.skinny_max_m, ops.I8_SKINNY_MAX_M):
            gemm = ops.gemm_i8_skinny
        elif (self.ring_min_m > 0 and M >= self.ring_min_m and not self.int4 and self.weight_scale.shape[1] == 1
              and ops.gemm_i8_ring_supported(Xq, self.weight, self.weight_scale)):
            gemm = ops.gemm_i8_ring
        elif (self.ring_w4_min_m > 0 and M >= self.ring_w4_min_m and self.int4
              and self.weight_scale.shape[1] * 128 == self.in_features
              and ops.gemm_i8_ring_w4_supported(Xq, self.weight, self.weight_scale)):
            # the attribute and M decide first: ops' ring_w4 names are read only past them
            gemm = ops.gemm_i8_ring_w4
        elif (self.mid_max_m > 0 and self.skinny_max_m < M <= self.mid_max_m and self.in_features >= self.mid_min_k
              and (self.mid_max_n == 0 or self.out_features <= self.mid_max_n) and M <= ops.I8_MID_MAX_M
              and ops.gemm_i8_mid_supported(Xq, self.weight, self.weight_scale)):
            # the attributes and the two sizes decide first: ops' mid names are read only past them
            gemm = ops.gemm_i8_mid
        elif (self.splitk_min_m > 0 and M >= self.splitk_min_m and (self.ring_min_m == 0 or M < self.ring_min_m)
              and not self.int4 and self.weight_scale.shape[1] == 1 and self.in_features >= self.splitk_min_k
              and ops.splitk_gemm_i8_supported(Xq, self.weight, self.weight_scale)):
            # the attributes and the sizes decide first: ops' splitk names are read only past them
            gemm = ops.splitk_gemm_i8
        else:
            gemm = ops.gemm_i8
        return gemm(
            Xq, s_x, self.weight, self.weight_scale, K=self.in_features, zp_x=zp_x,
            wsum=None if zp_x is None else self.wsum, bias=bias, out_dtype=out_dtype)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        Xq, s_x, zp_x = self.quantize_rows(x)
        return self.gemm_rows(Xq, s_x, zp_x, x.dtype).reshape(*x.shape[:-1], self.out_features)


def is_silu(act_fn) -> bool:
    """Whether ``act_fn`` is SiLU as ``qt_act_mul_quantize_i8`` states it: ``nn.SiLU``, ``F.silu`` or what
    ``transformers.activations.ACT2FN["silu"]`` yields (a module whose forward is ``F.silu``)."""
    if isinstance(act_fn, nn.SiLU) or act_fn is F.silu:
        return True
    try:
        from transformers.activations import ACT2FN
    except ImportError:
        return False
    ref = ACT2FN["silu"]
    return act_fn is ref or (isinstance(ref, nn.Module) and type(act_fn) is type(ref))


class QuantizedMLP(nn.Module):
    """A Llama-style MLP ``down_proj(act_fn(gate_proj(x)) * up_proj(x))`` of three ``QuantizedLinear``s with the glue
    between the products fused: ``x`` is quantised once for gate and up, and ``qt_act_mul_quantize_i8`` turns their
    outputs into down's quantised rows in one pass (five launches, not eight).  The three GEMMs are the ones the
    stand-alone Linears choose, and the fused pass equals torch's SiLU, its multiply and ``qt_quantize_tokens_i8`` to
    the bit (include/quantool_amd.h), so the module changes speed alone.  Opt-in: ``load_quantized(...,
    a8_fused_act=True)`` builds it where ``eligible`` holds.  The children keep their names, so state-dict keys do not
    move."""

    # parents whose forward is the plain down(act(gate(x)) * up(x)), by class name (transformers 5.x)
    PLAIN_MLPS = ("LlamaMLP", "MistralMLP", "Qwen2MLP", "Qwen3MLP")

    def __init__(self, gate_proj: QuantizedLinear, up_proj: QuantizedLinear, down_proj: QuantizedLinear, act_fn):
        super().__init__()
        reason = self.refusal(gate_proj, up_proj, down_proj, act_fn)
        if reason:
            raise ValueError(f"QuantizedMLP: {reason}")
        self.gate_proj, self.up_proj, self.down_proj, self.act_fn = gate_proj, up_proj, down_proj, act_fn

    @staticmethod
    def refusal(gate, up, down, act_fn) -> Optional[str]:
        """Why these four cannot run fused (None: they can)."""
        if not all(isinstance(m, QuantizedLinear) for m in (gate, up, down)):
            return "gate_proj, up_proj and down_proj must all be QuantizedLinears"
        if not is_silu(act_fn):
            return "act_fn is not SiLU"
        if gate.in_features != up.in_features or gate.act_symmetric != up.act_symmetric:
            return "gate_proj and up_proj differ in in_features or act_symmetric, so they cannot share quantised rows"
        if (gate.col_perm is None) != (up.col_perm is None) or (
                gate.col_perm is not None and not torch.equal(gate.col_perm, up.col_perm)):
            return "gate_proj and up_proj differ in col_perm, so they cannot share quantised rows"
        if not gate.out_features == up.out_features == down.in_features:
            return "gate_proj / up_proj outputs are not down_proj's inputs"
        return None

    @classmethod
    def eligible(cls, mlp: nn.Module) -> bool:
        """Whether ``mlp`` is one of ``PLAIN_MLPS`` whose three Linears and activation can run fused."""
        if type(mlp).__name__ not in cls.PLAIN_MLPS:
            return False
        parts = [getattr(mlp, n, None) for n in ("gate_proj", "up_proj", "down_proj", "act_fn")]
        return cls.refusal(*parts) is None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from ..hip import ops

        gate, up, down = self.gate_proj, self.up_proj, self.down_proj
        Xq, s_x, zp_x = gate.quantize_rows(x)
        g = gate.gemm_rows(Xq, s_x, zp_x, x.dtype)
        u = up.gemm_rows(Xq, s_x, zp_x, x.dtype)
        Hq, s_h, zp_h = ops.act_mul_quantize_i8(g, u, symmetric=down.act_symmetric, col_perm=down.col_perm)
        return down.gemm_rows(Hq, s_h, zp_h, x.dtype).reshape(*x.shape[:-1], down.out_features)


def _version_of(t: torch.Tensor) -> Optional[int]:
    """``t``'s in-place write counter, or None where torch keeps none (inference tensors)."""
    try:
        return t._version
    except RuntimeError:
        return None


class SharedRows:
    """The hand-off between a ``QuantizingRMSNorm`` and the ``QuantizedLinear``s behind it: the tensor ``y`` the norm
    returned, its version when it was returned, its quantised rows ``(Xq, s_x, zp_x)`` and how many consumers are
    still to come.  ``take(x)`` gives the rows only for that very tensor, unwritten since; after the last consumer
    every reference is dropped, so between forwards nothing is pinned."""

    def __init__(self):
        self.clear()

    def clear(self) -> None:
        self.y = self.version = self.rows = None
        self.left = 0

    def put(self, y: torch.Tensor, Xq: torch.Tensor, s_x: torch.Tensor, zp_x: Optional[torch.Tensor],
            consumers: int) -> None:
        self.clear()
        version = _version_of(y)
        if version is None or consumers <= 0:      # staleness could not be seen: every consumer quantises for itself
            return
        self.y, self.version, self.rows, self.left = y, version, (Xq, s_x, zp_x), int(consumers)

    @property
    def holds_tensors(self) -> bool:
        return self.y is not None or self.rows is not None

    def take(self, x: torch.Tensor):
        """``(Xq, s_x, zp_x)`` when ``x`` is the tensor the norm returned and nothing has written to it; else None."""
        if self.y is None or x is not self.y or _version_of(x) != self.version:
            return None
        rows = self.rows
        self.left -= 1
        if self.left <= 0:
            self.clear()
        return rows


class QuantizingRMSNorm(nn.Module):
    """An RMSNorm whose output feeds only ``QuantizedLinear``s that share their quantised rows (q/k/v, or gate/up), with
    the quantiser fused in: ``forward(x)`` runs ``qt_rmsnorm_quantize_i8`` -- one launch in place of torch's chain of
    elementwise and reduction kernels and of the consumers' quantiser launches -- returns ``Y`` shaped like ``x`` and
    leaves ``(Xq, s_x, zp_x)`` in the ``SharedRows`` its consumers ask first.  ``Y`` and the rows are the header's fixed
    sequence: the five lines of ``LlamaRMSNorm.forward`` with the kernel's own order of summation over K, then exactly
    ``qt_quantize_tokens_i8(Y)``.  Opt-in: ``load_quantized(..., a8_fused_norm=True)`` builds it where
    ``refusal`` is None.  ``weight`` keeps its name, so state-dict keys do not move.

    The installed torch sequence runs instead when ``x`` is not a 16-bit device tensor of the weight's dtype, when
    K > ``MAX_K`` or when a gradient is required; the consumers then quantise for themselves.

    ``takes``: how many ``quantize_rows`` calls follow one forward (the default: one per consumer; a ``QuantizedMLP``
    quantises once for gate and up)."""

    # norms whose forward is the five-line sequence the kernel restates, by class name (transformers 5.x)
    PLAIN_NORMS = ("LlamaRMSNorm", "MistralRMSNorm", "Qwen2RMSNorm", "Qwen3RMSNorm", "MixtralRMSNorm")
    # decoder layers whose forward hands input_layernorm's output to self_attn and post_attention_layernorm's to mlp
    PLAIN_LAYERS = ("LlamaDecoderLayer", "MistralDecoderLayer", "Qwen2DecoderLayer", "Qwen3DecoderLayer",
                    "MixtralDecoderLayer")
    MAX_K = 32768              # qt_rmsnorm_quantize_i8's bound
    device_types = ("cuda",)   # where the kernel exists

    def __init__(self, weight: nn.Parameter, eps: float, consumers, takes: Optional[int] = None):
        super().__init__()
        consumers = list(consumers)
        if not consumers or not all(isinstance(c, QuantizedLinear) for c in consumers):
            raise ValueError("QuantizingRMSNorm: the consumers must all be QuantizedLinears")
        reason = self._consumers_refusal(consumers, weight.numel())
        if reason:
            raise ValueError(f"QuantizingRMSNorm: {reason}")
        self.weight = weight if isinstance(weight, nn.Parameter) else nn.Parameter(weight, requires_grad=False)
        self.variance_epsilon = float(eps)
        self.takes = len(consumers) if takes is None else int(takes)
        self.__dict__["_shared"] = SharedRows()
        self.__dict__["_consumers"] = consumers      # not submodules: they keep their own names in the model
        for c in consumers:
            c.rows_from = self._shared

    @property
    def shared(self) -> SharedRows:
        return self._shared

    @staticmethod
    def _consumers_refusal(consumers, K: int) -> Optional[str]:
        first = consumers[0]
        if first.in_features != K:
            return "the consumers' in_features is not the norm's width"
        for c in consumers[1:]:
            if c.in_features != first.in_features or c.act_symmetric != first.act_symmetric:
                return "the consumers differ in in_features or act_symmetric, so they cannot share quantised rows"
            if (c.col_perm is None) != (first.col_perm is None) or (
                    c.col_perm is not None and not torch.equal(c.col_perm, first.col_perm)):
                return "the consumers differ in col_perm, so they cannot share quantised rows"
        return None

    @classmethod
    def refusal(cls, norm: nn.Module, consumers) -> Optional[str]:
        """Why ``norm`` cannot quantise for ``consumers`` (None: it can)."""
        if type(norm).__name__ not in cls.PLAIN_NORMS:
            return f"{type(norm).__name__} is not one of {cls.PLAIN_NORMS}"
        consumers = list(consumers)
        if not consumers or not all(isinstance(c, QuantizedLinear) for c in consumers):
            return "the consumers must all be QuantizedLinears"
        weight = getattr(norm, "weight", None)
        if not isinstance(weight, torch.Tensor) or weight.dim() != 1 or not hasattr(norm, "variance_epsilon"):
            return "the norm has no 1-d weight or no variance_epsilon"
        return cls._consumers_refusal(consumers, weight.numel())

    def extra_repr(self) -> str:
        return f"{tuple(self.weight.shape)}, eps={self.variance_epsilon}, consumers={len(self._consumers)}"

    def _torch_forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        input_dtype = hidden_states.dtype
        hidden_states = hidden_states.to(torch.float32)
        variance = hidden_states.pow(2).mean(-1, keepdim=True)
        hidden_states = hidden_states * torch.rsqrt(variance + self.variance_epsilon)
        return self.weight * hidden_states.to(input_dtype)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        w = self.weight
        K = w.numel()
        if (x.device.type not in self.device_types or x.dtype not in (torch.bfloat16, torch.float16)
                or x.dtype != w.dtype or x.device != w.device or K > self.MAX_K or x.numel() == 0
                or (torch.is_grad_enabled() and (x.requires_grad or w.requires_grad))):
            self._shared.clear()
            return self._torch_forward(x)
        from ..hip import ops

        first = self._consumers[0]
        Y, Xq, s_x, zp_x = ops.rmsnorm_quantize_i8(_rows(x, K), w, self.variance_epsilon,
                                                   symmetric=first.act_symmetric, col_perm=first.col_perm)
        y = Y.reshape(x.shape)
        self._shared.put(y, Xq, s_x, zp_x, self.takes)
        return y


class WeightOnlyLinear(nn.Module):
    """One W4A16 / W4A16_ASYM / W8A16 Linear of a checkpoint on its stored integer weights.

    ``forward(x)`` with M = rows of ``x``: M <= ``skinny_max_m`` runs ``qt_gemm_wq_skinny`` (the weights read once,
    dequantised on chip; fp32 sums in the kernel's own fixed order); otherwise ``qt_dequantize_weight`` fills a transient
    dense weight -- bit-identical to the default loader's ``nn.Linear.weight`` -- and ``F.linear`` runs on it, so the
    output equals that ``nn.Linear``'s to the bit.  On CPU tensors ``forward`` is ``F.linear`` on
    ``stored.dequantize``.

    Opt-in: with ``stream_max_m`` > 0, ``skinny_max_m`` < M <= ``stream_max_m`` runs ``qt_gemm_wq_stream`` (the weights
    read once as well; every row bit-identical to the skinny kernel's, not to ``F.linear``'s) on a Linear with
    ``in_features`` >= ``stream_min_k`` and, when ``stream_max_n`` is not 0, ``out_features`` <= ``stream_max_n``, where
    ``ops.gemm_wq_stream_supported`` holds (no ``g_idx``, K a multiple of 128, aligned rows).

    Buffers: ``weight_packed`` int32 [N, ceil(K/8)] (int4) or ``weight`` int8 [N, K]; ``weight_scale`` fp32 [N, G];
    ``weight_zero_point`` int8 [N, G] (optional); ``g_idx`` int32 [K] (optional, actorder ``group``); ``bias``
    (optional, model dtype).  Columns stay in their original order."""

    # Decode GEMV up to this many rows, dequantise + F.linear above: at 16 rows the GEMV is still faster than the
    # dequantise + F.linear pair on every measured Llama-3-8B shape.
    skinny_max_m = 16
    # Weight-streaming GEMM up to this many rows.  0, the default: never -- a fused kernel cannot equal F.linear's
    # summation order, so it is the caller's choice (``load_quantized(..., a16_stream_rows=)``; the measurements support
    # 32: from 48 rows on the first Llama-3-8B shapes lose to dequantise + F.linear).  Used only when
    # it is not 0: up to this many output features (0: no bound) and from this many input features, the largest N and
    # the smallest K measured, at both of which the kernel wins at 17 and 32 rows in both runs and all three schemes.
    stream_max_m = 0
    stream_max_n = 28672
    stream_min_k = 512

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

    @property
    def stored(self) -> StoredWeight:
        """The buffers as they are now (after any ``.to(device)``), as one value."""
        b = self._buffers   # on the decode path: four lookups through nn.Module.__getattr__ cost more than all the rest
        return StoredWeight(b["weight_packed" if self.int4 else "weight"], b["weight_scale"], b["weight_zero_point"],
                            b["g_idx"], self.out_features, self.in_features)

    def checkpoint_tensors(self) -> Dict[str, torch.Tensor]:
        """The module's weight as the checkpoint leaves ``dequantized_weight`` reads."""
        return self.stored.leaves()

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"weights={'int4' if self.int4 else 'int8'}, groups={self.weight_scale.shape[1]}, "
                f"zero_point={self.weight_zero_point is not None}, g_idx={self.g_idx is not None}, "
                f"bias={self.bias is not None}, skinny_max_m={self.skinny_max_m}, stream_max_m={self.stream_max_m}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        bias = None if self.bias is None else self.bias.to(x.dtype)
        w = self.stored
        if not x.is_cuda:
            return F.linear(x, w.dequantize(x.dtype), bias)
        from ..hip import ops

        M = x.numel() // w.K
        if 1 <= M <= min(self.skinny_max_m, ops.SKINNY_MAX_M):
            y = ops.gemm_wq_skinny(_rows(x, w.K), w.levels, w.scale, zp_w=w.zero_point, g_idx=w.g_idx, bias=bias)
            return y.reshape(*x.shape[:-1], w.N)
        if (self.stream_max_m > 0 and self.skinny_max_m < M <= self.stream_max_m and w.K >= self.stream_min_k
                and (self.stream_max_n == 0 or w.N <= self.stream_max_n) and M <= ops.WQ_STREAM_MAX_M):
            # the attributes and the sizes decide first: ops' stream names are read only past them
            x2 = _rows(x, w.K)
            if ops.gemm_wq_stream_supported(x2, w.levels, w.scale, w.zero_point, w.g_idx):
                y = ops.gemm_wq_stream(x2, w.levels, w.scale, zp_w=w.zero_point, bias=bias)
                return y.reshape(*x.shape[:-1], w.N)
        W = ops.dequantize_weight(w.levels, w.scale, K=w.K, zp_w=w.zero_point, g_idx=w.g_idx, dtype=x.dtype)
        return F.linear(x, W, bias)


class _RoutedExperts(nn.Module):
    """The forward both expert banks run on the device, as transformers' fused bank with its two ``F.linear`` calls
    replaced: ``qt_moe_route`` orders the routed rows by expert, the gate_up product gathers them by token,
    ``act_fn(gate) * up`` runs in torch as the fused module does, the down product reads the routed rows in place and
    ``qt_moe_combine`` sums each token's weighted rows in ascending expert order, rounding as ``index_add_`` does.
    Nothing waits on the host.  A subclass gives the product: ``_product(part, x, offsets, row_idx, tokens)``, rows
    ``x[row_idx]`` (or ``x``) times the ``part`` ("gate_up" / "down") weights of the expert that owns each row."""

    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor):
        from ..hip import ops

        x = _rows(hidden_states, self.hidden_dim)
        offsets, src_token, _, row_of = ops.moe_route(top_k_index, self.num_experts)
        T = x.shape[0]
        gate, up = self._product("gate_up", x, offsets, src_token, T).chunk(2, dim=-1)
        y = self._product("down", self.act_fn(gate) * up, offsets, None, T)
        return ops.moe_combine(y, row_of, top_k_weights).reshape(hidden_states.shape)


class QuantizedExperts(_RoutedExperts):
    """A W8A8 / INT8 / W4A8 routed-expert bank: ``forward(hidden_states, top_k_index, top_k_weights)`` as
    transformers' ``MixtralExperts`` with its two ``F.linear`` calls on the int8 GEMM (``_RoutedExperts``): the T tokens
    are quantised once per token for the gate_up GEMM, the routed rows of ``act_fn(gate) * up`` per row for the down
    GEMM.  include/quantool_amd.h states every step.

    Buffers: ``gate_up`` int8 [E, 2I, H] or packed int4 int32 [E, 2I, ceil(H/8)] (rows [0, I) gate, [I, 2I) up),
    ``gate_up_scale`` fp32 [E, 2I, G], ``gate_up_wsum`` int32 [E, 2I, G]; ``down`` int8 [E, H, I] or int32
    [E, H, ceil(I/8)], ``down_scale`` fp32 [E, H, G'], ``down_wsum`` int32 [E, H, G'].

    With T = rows of ``hidden_states`` (known on the host) and 1 <= T <= ``grouped_max_tokens`` both products run the
    decode form ``qt_gemm_i8_skinny_grouped`` (16-row tiles, only the experts that were hit are read), otherwise the
    128-row-tile ``qt_gemm_i8_grouped``.  The two agree to the bit; 0 sends every T to the tiled kernel.  Past the
    decode range a product of R routed rows with R / E >= ``ring_min_rows_per_expert`` (when that is not 0) runs an
    int8 bank with one scale group on the 256-row LDS-ring tile ``qt_gemm_i8_ring_grouped`` where
    ``ops.gemm_i8_ring_grouped_supported`` holds; it agrees with the tiled kernel to the bit as well, so the attribute
    changes speed alone, and 0 never uses it.  A packed int4 (W4A8) bank with one scale per 128 columns has its own
    ring and its own bound: from R / E >= ``ring_w4_min_rows_per_expert`` (0: never) a product runs on
    ``qt_moe_gemm_i8_ring_w4`` where ``ops.moe_gemm_i8_ring_w4_supported`` holds, equal to the tiled kernel to the bit
    again; every other int4 product stays on the tiled kernel.

    Between the decode range and the rings a product of R routed rows with K >= ``wide_min_k`` and, when ``wide_max_n``
    is not 0, N <= ``wide_max_n`` runs on the weight-streaming 16-column tile ``qt_moe_gemm_i8_wide`` where
    ``ops.moe_gemm_i8_wide_supported`` holds, up to R / E <= ``wide_max_rows_per_expert`` for an int8 bank and up to
    R / E <= ``wide_w4_max_rows_per_expert`` for a packed int4 bank (0: never; each format reads its own attribute
    alone).  It agrees with the tiled kernel to the bit too, so these attributes change speed alone; the skinny range
    and the two rings keep precedence, and everything else runs the tiled kernel.

    Opt-in: with ``fused_act`` and a SiLU ``act_fn``, ``act_fn(gate) * up`` and the down product's quantiser run as one
    pass, ``qt_act_mul_quantize_i8``, on the two halves of the gate_up output; the GEMM choice sees the same rows and
    the output is the same to the bit."""

    # Decode form up to this many tokens: the measured crossover at Mixtral-8x7B's bank shapes.
    grouped_max_tokens = 16
    # LDS-ring form from this many routed rows per expert (R / E; 0: never): the smallest measured R / E from which the
    # ring is no slower than the tiled grouped kernel on both products at Mixtral-8x7B's bank shapes, at that size and
    # every larger one, in both runs.
    ring_min_rows_per_expert = 1024
    # The same bound for a packed int4 bank with G = K / 128 and qt_moe_gemm_i8_ring_w4 (0: never; never below 1024): the
    # smallest measured R / E from which the ring beats the tiled grouped kernel on both products by more than the tiled
    # kernel's own run-to-run spread, at that size and every larger one, in both runs.  At 1024 the down
    # product is level (0.6 - 1.2 % against a spread of 1.0 %).
    ring_w4_min_rows_per_expert = 2048
    # qt_moe_gemm_i8_wide up to this many routed rows per expert (R / E; 0: never), for an int8 bank and for a packed
    # int4 bank: per format and product, the largest measured R / E at which, and at every smaller measured size past the
    # decode range, the form beat the tiled grouped kernel in both runs by more than the tiled kernel's largest
    # run-to-run spread in those runs (Mixtral-8x7B's bank shapes, R / E = 4.25 ... 1024).  Int8: the down
    # product wins 1.54 / 1.39 / 1.16x at R / E = 4.25 / 8 / 16 and loses from 32 (0.92x); gate_up never wins (0.88x at
    # best).  Packed int4: down wins 2.2 / 2.2 / 1.5 / 1.3x at 4.25 / 8 / 16 / 32 and loses from 64 (0.94x); gate_up wins
    # 1.10 / 1.07x at 4.25 / 8 and loses from 16 (0.78x).
    wide_max_rows_per_expert = 16
    wide_w4_max_rows_per_expert = 32
    # Products with a smaller K stay on the tiled kernel: they are launch-bound (as QuantizedLinear.mid_min_k).
    wide_min_k = 512
    # Products with more output columns stay on the tiled kernel (0: no bound): every 16-column tile re-reads its
    # activation rows.  The down product's N at the measured shapes: only down qualifies for an int8 bank, and with
    # gate_up (N = 28672) held back the int4 bound above is down's own; what this gives up is int4 gate_up's 7 - 11 % at
    # R / E <= 8.
    wide_max_n = 4096
    # SiLU(gate) * up and the down product's quantiser in one pass, qt_act_mul_quantize_i8, when act_fn is SiLU: equal
    # to the three passes it replaces to the bit.  Off by default: opt-in through
    # ``load_quantized(..., a8_fused_act=True)``; any other act_fn keeps the three passes.
    fused_act = False

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
            self.register_buffer(name, w.contiguous())
            self.register_buffer(f"{name}_scale", s.to(torch.float32).contiguous())
            self.register_buffer(f"{name}_wsum", group_sums(unpack_int4(w, K) if self.int4 else w, s.shape[2]))

    def extra_repr(self) -> str:
        return (f"num_experts={self.num_experts}, hidden={self.hidden_dim}, intermediate={self.intermediate_dim}, "
                f"weights={'int4 g128' if self.int4 else 'int8'}, "
                f"groups=({self.gate_up_scale.shape[2]}, {self.down_scale.shape[2]}), "
                f"act={'sym' if self.act_symmetric else 'asym'} int8 per-token")

    def _product(self, part: str, x: torch.Tensor, offsets: torch.Tensor, row_idx: Optional[torch.Tensor],
                 tokens: int):
        from ..hip import ops

        Xq, s_x, zp_x = ops.quantize_tokens_i8(x, symmetric=self.act_symmetric)
        return self._gemm(part, Xq, s_x, zp_x, offsets, row_idx, tokens, x.dtype)

    def _gemm(self, part: str, Xq: torch.Tensor, s_x: torch.Tensor, zp_x: Optional[torch.Tensor],
              offsets: torch.Tensor, row_idx: Optional[torch.Tensor], tokens: int, out_dtype: torch.dtype):
        """Quantised rows times the ``part`` weights, on the GEMM form the class docstring gives for ``tokens`` and
        the R routed rows."""
        from ..hip import ops

        w, s_w = getattr(self, part), getattr(self, f"{part}_scale")
        K = Xq.shape[1]
        R = Xq.shape[0] if row_idx is None else row_idx.numel()
        ring, ring_w4 = self.ring_min_rows_per_expert, self.ring_w4_min_rows_per_expert
        wide = self.wide_w4_max_rows_per_expert if self.int4 else self.wide_max_rows_per_expert
        if 1 <= tokens <= self.grouped_max_tokens:
            gemm = ops.gemm_i8_skinny_grouped
        elif (ring > 0 and R >= ring * self.num_experts and not self.int4 and s_w.shape[2] == 1
              and ops.gemm_i8_ring_grouped_supported(Xq, w, s_w, row_idx)):
            gemm = ops.gemm_i8_ring_grouped
        elif (ring_w4 > 0 and R >= ring_w4 * self.num_experts and self.int4 and s_w.shape[2] * 128 == K
              and ops.moe_gemm_i8_ring_w4_supported(Xq, w, s_w, row_idx)):
            gemm = ops.moe_gemm_i8_ring_w4
        elif (wide > 0 and R <= wide * self.num_experts and K >= self.wide_min_k
              and (self.wide_max_n == 0 or w.shape[1] <= self.wide_max_n)
              and ops.moe_gemm_i8_wide_supported(Xq, w, s_w, row_idx)):
            gemm = ops.moe_gemm_i8_wide
        else:
            gemm = ops.gemm_i8_grouped
        return gemm(Xq, s_x, w, s_w, offsets, row_idx=row_idx,
                    K=K, zp_x=zp_x, wsum=None if zp_x is None else getattr(self, f"{part}_wsum"),
                    out_dtype=out_dtype)

    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor):
        # the attribute decides first: ops' fused name is read only past it
        if not (self.fused_act and is_silu(self.act_fn)):
            return super().forward(hidden_states, top_k_index, top_k_weights)
        from ..hip import ops

        x = _rows(hidden_states, self.hidden_dim)
        offsets, src_token, _, row_of = ops.moe_route(top_k_index, self.num_experts)
        T, I = x.shape[0], self.intermediate_dim
        Y = self._product("gate_up", x, offsets, src_token, T)
        Xq, s_x, zp_x = ops.act_mul_quantize_i8(Y[:, :I], Y[:, I:], symmetric=self.act_symmetric)
        y = self._gemm("down", Xq, s_x, zp_x, offsets, None, T, Y.dtype)
        return ops.moe_combine(y, row_of, top_k_weights).reshape(hidden_states.shape)


class WeightOnlyExperts(_RoutedExperts):
    """A W4A16 / W4A16_ASYM / W8A16 routed-expert bank on its stored integer weights: ``forward(hidden_states,
    top_k_index, top_k_weights)`` as the fused transformers bank it replaces.

    With T = rows of ``hidden_states`` (known on the host) and 1 <= T <= ``grouped_max_tokens``: the routed forward of
    ``_RoutedExperts`` on the grouped GEMV (``qt_gemm_wq_grouped``).  Only the experts that were hit are read.  Larger
    T: both banks are dequantised into transient [E, 2I, H] / [E, H, I] tensors
    (``qt_dequantize_weight``, bit-identical to the dense bank ``a16_experts="dequantized"`` loads) and the bank's own
    transformers forward runs on them (honouring ``config._experts_implementation``), so the output equals the dense
    bank's to the bit.  On CPU tensors ``forward`` is that bank forward on ``stored(part).dequantize``.

    Inside the routed forward a product with T >= ``wide_min_tokens`` (when that is not 0) runs
    ``qt_moe_gemm_wq_wide`` (several 16-row tiles of one expert per workgroup, the expert's weights read once for all of
    them) where ``ops.moe_gemm_wq_wide_supported`` holds; the two kernels agree to the bit, so the attribute changes speed
    alone.  Opt-in: with ``wide_max_tokens`` > 0, ``grouped_max_tokens`` < T <= ``wide_max_tokens`` takes the routed
    forward on that kernel instead of the dequantise path, on a bank where both products are supported (no ``g_idx``,
    H and I multiples of 128); its rows are bit-identical to the grouped GEMV's, not to the dense bank's.

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
    # qt_moe_gemm_wq_wide inside the routed forward from this many tokens (0: never): the smallest measured T from which
    # the form beat the grouped GEMV on both products, in both runs and all three schemes, by more than the GEMV's own
    # run-to-run spread (at most 1.8 %), at that size and at every larger measured size up to 128 (Mixtral-8x7B's bank
    # shapes, E = 8, top-2).  At 96 tokens (2 m-tiles) it wins 1.21 - 1.29x and at 128 1.11 - 1.20x; at 17,
    # 32 and 64 (1 m-tile: the GEMV's own tile) it is 0.95 - 1.05x.
    wide_min_tokens = 96
    # The routed forward on qt_moe_gemm_wq_wide up to this many tokens, past grouped_max_tokens.  0, the default: never
    # -- a fused kernel cannot equal the dense bank's summation order, so it is the caller's choice
    # (``load_quantized(..., a16_experts_wide_tokens=)``; the measurements support 384: the routed forward takes 0.47 - 0.83
    # of the dequantise path's time at 192 - 384 tokens and 1.08 - 1.19 of it at 512).
    wide_max_tokens = 0

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
                f"grouped_max_tokens={self.grouped_max_tokens}, wide_min_tokens={self.wide_min_tokens}, "
                f"wide_max_tokens={self.wide_max_tokens}")

    def stored(self, part: str) -> StoredWeight:
        """The ``part`` ("gate_up" / "down") buffers as they are now, as one bank weight [E, ...]."""
        b = self._buffers   # on the decode path, as ``WeightOnlyLinear.stored``
        H, I = self.hidden_dim, self.intermediate_dim
        N, K = (2 * I, H) if part == "gate_up" else (H, I)
        return StoredWeight(b[part], b[f"{part}_scale"], b[f"{part}_zero_point"], b[f"{part}_g_idx"], N, K)

    def dense_weight(self, part: str, dtype: torch.dtype) -> torch.Tensor:
        """The ``part`` ("gate_up" / "down") bank dequantised, [E, N, K] in ``dtype``: the dense bank's parameter."""
        w = self.stored(part)
        if not w.levels.is_cuda:
            return w.dequantize(dtype)
        from ..hip import ops

        E = self.num_experts
        out = torch.empty((E, w.N, w.K), dtype=dtype, device=w.levels.device)
        if w.g_idx is None:                 # one call over the stacked [E N, .] rows
            ops.dequantize_weight(w.levels.flatten(0, 1), w.scale.flatten(0, 1), K=w.K,
                                  zp_w=None if w.zero_point is None else w.zero_point.flatten(0, 1), dtype=dtype,
                                  out=out.flatten(0, 1))
        else:
            for e in range(E):
                ops.dequantize_weight(w.levels[e], w.scale[e], K=w.K, zp_w=None if w.zero_point is None
                                      else w.zero_point[e], g_idx=w.g_idx[e], dtype=dtype, out=out[e])
        return out

    def _product(self, part: str, x: torch.Tensor, offsets: torch.Tensor, row_idx: Optional[torch.Tensor],
                 tokens: int):
        from ..hip import ops

        w = self.stored(part)
        gemm = ops.gemm_wq_grouped
        if tokens > self.grouped_max_tokens:
            gemm = ops.moe_gemm_wq_wide         # the extended range: forward() has checked both products
        elif self.wide_min_tokens > 0 and tokens >= self.wide_min_tokens:
            # the attribute and T decide first: ops' wide names are read only past them
            if ops.moe_gemm_wq_wide_supported(x, w.levels, w.scale, w.zero_point, w.g_idx, row_idx):
                gemm = ops.moe_gemm_wq_wide
        return gemm(x, w.levels, w.scale, offsets, row_idx=row_idx, K=w.K, zp_w=w.zero_point, g_idx=w.g_idx)

    def _wide_range(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor) -> bool:
        """Whether both products of this call run on ``qt_moe_gemm_wq_wide``: the gate_up product on the rows of
        ``hidden_states`` gathered by token, the down product on the R = ``top_k_index.numel()`` routed rows (a
        stand-in of that shape on the meta device is judged: the rows themselves are a fresh contiguous tensor)."""
        from ..hip import ops

        x = _rows(hidden_states, self.hidden_dim)
        routed = top_k_index.reshape(-1)        # its length alone is read
        act = torch.empty((routed.numel(), self.intermediate_dim), dtype=x.dtype, device="meta")
        for part, rows, row_idx in (("gate_up", x, routed), ("down", act, None)):
            w = self.stored(part)
            if not ops.moe_gemm_wq_wide_supported(rows, w.levels, w.scale, w.zero_point, w.g_idx, row_idx):
                return False
        return True

    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor):
        T = hidden_states.numel() // self.hidden_dim
        if hidden_states.is_cuda and 1 <= T <= self.grouped_max_tokens:
            return super().forward(hidden_states, top_k_index, top_k_weights)
        if (hidden_states.is_cuda and self.wide_max_tokens > 0 and self.grouped_max_tokens < T <= self.wide_max_tokens
                and self._wide_range(hidden_states, top_k_index)):
            return super().forward(hidden_states, top_k_index, top_k_weights)
        dense = {"gate_up_proj": self.dense_weight("gate_up", hidden_states.dtype),
                 "down_proj": self.dense_weight("down", hidden_states.dtype)}
        return torch.func.functional_call(self._bank, dense, (hidden_states, top_k_index, top_k_weights))
