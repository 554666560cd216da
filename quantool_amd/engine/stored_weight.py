"""One stored weight of a checkpoint as a value, and the integer helpers around it: no ``nn.Module`` here.

``StoredWeight`` is what a quantized Linear is on disk -- integer levels (int8, or int4 packed eight to an int32 word),
``scale`` per row and column group, an optional zero-point and an optional group of every column (actorder ``group``).
A routed-expert bank is the same value with a leading expert dimension.  ``from_leaves`` is the one reader of the
checkpoint's tensors, ``require_kernel_layout`` the one statement of what the kernels ask of a weight, ``dequantize`` the
torch definition of the dense weight that ``qt_dequantize_weight`` reproduces to the bit (include/quantool_amd.h)."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence

import torch

GROUP = 128   # the column group size the kernels take


def unpack_int4(packed: torch.Tensor, K: int) -> torch.Tensor:
    """int32 [..., R, ceil(K/8)] (nibble j of word w = level of column 8w + j, plus 8) -> int8 levels [..., R, K]."""
    shifts = torch.arange(0, 32, 4, device=packed.device, dtype=torch.int32)
    nib = (packed.unsqueeze(-1) >> shifts) & 0xF
    return (nib.flatten(-2)[..., :K] - 8).to(torch.int8)


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
    """wsum [..., R, G] int32: sums of the levels q [..., R, K] over each group of 128 contiguous columns (G = 1: whole
    rows)."""
    q = q.to(torch.int32)
    if G == 1:
        return q.sum(-1, keepdim=True, dtype=torch.int32).contiguous()
    q = torch.nn.functional.pad(q, (0, G * GROUP - q.shape[-1]))
    return q.unflatten(-1, (G, GROUP)).sum(-1, dtype=torch.int32).contiguous()


class StoredWeight(NamedTuple):
    """``levels`` int8 [N, K] or packed int4 int32 [N, ceil(K/8)]; ``scale`` fp32 [N, G]; ``zero_point`` [N, G] or None
    (int8 once ``require_kernel_layout`` has passed); ``g_idx`` int32 [K], the group of every column, or None (column k
    is in group k // 128, or 0 when G = 1).  A bank of E experts carries a leading E on all four."""
    levels: torch.Tensor
    scale: torch.Tensor
    zero_point: Optional[torch.Tensor]
    g_idx: Optional[torch.Tensor]
    N: int
    K: int

    @property
    def int4(self) -> bool:
        return self.levels.dtype == torch.int32

    @property
    def G(self) -> int:
        return self.scale.shape[-1]

    @classmethod
    def from_leaves(cls, name: str, t: Dict[str, torch.Tensor]) -> "StoredWeight":
        """One quantized module's checkpoint tensors (``weight`` or ``weight_packed``, ``weight_scale``, and optionally
        ``weight_shape``, ``weight_zero_point``, ``weight_g_idx``) as a value.  Checks what reading them needs: the
        level tensor against its shape and ``weight_g_idx`` against the groups.  Any scale layout passes."""
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
        else:
            w = t.get("weight")
            if w is None or w.dtype != torch.int8 or tuple(w.shape) != (N, K):
                raise ValueError(f"{name}: expected an int8 weight [{N}, {K}] or a weight_packed tensor")
        scale = t["weight_scale"].to(torch.float32)            # bf16 / fp16 -> fp32 is exact
        g_idx = t.get("weight_g_idx")
        if g_idx is not None:
            G = scale.shape[1]
            if g_idx.numel() != K or int(g_idx.min()) < 0 or int(g_idx.max()) >= G:
                raise ValueError(f"{name}: weight_g_idx does not match {G} groups of {K} columns")
            g_idx = g_idx.to(torch.int32)
        return cls(w, scale, t.get("weight_zero_point"), g_idx, N, K)

    def require_kernel_layout(self, name: str, hint: str = "") -> "StoredWeight":
        """What the GEMMs, the GEMVs and ``qt_dequantize_weight`` ask of a weight: scales channel-wise or per group of
        128 columns, zero-points int8 beside every scale.  Returns the weight with its zero-point as int8."""
        rows = (*self.levels.shape[:-2], self.N)
        if tuple(self.scale.shape) not in ((*rows, 1), (*rows, (self.K + GROUP - 1) // GROUP)):
            raise ValueError(f"{name}: weight_scale {tuple(self.scale.shape)} is neither channel-wise nor groups of "
                             f"{GROUP} over {self.K} columns{hint}")
        zp = self.zero_point
        if zp is None:
            return self
        if tuple(zp.shape) != (*rows, self.G) or zp.is_floating_point() or int(zp.min()) < -128 or int(zp.max()) > 127:
            raise ValueError(f"{name}: weight_zero_point must be integers in [-128, 127] of shape {(*rows, self.G)}")
        return self._replace(zero_point=zp.to(torch.int8))

    def dequantize(self, dtype: torch.dtype) -> torch.Tensor:
        """(q - zp) * scale in fp32 from the stored scale (and zero-point), rounded once to ``dtype``: [N, K]."""
        if self.g_idx is not None:
            g = self.g_idx.to(torch.int64).unsqueeze(-2)
        elif self.G == 1:
            g = torch.zeros(self.K, dtype=torch.int64, device=self.scale.device)
        else:
            g = torch.arange(self.K, device=self.scale.device) // GROUP

        def of_column(per_group: torch.Tensor) -> torch.Tensor:
            return per_group.to(torch.float32).gather(-1, g.expand(*per_group.shape[:-1], self.K))

        q = (unpack_int4(self.levels, self.K) if self.int4 else self.levels).to(torch.float32)
        if self.zero_point is not None:
            q = q - of_column(self.zero_point)
        return (q * of_column(self.scale)).to(dtype)

    @classmethod
    def stack(cls, name: str, experts: Sequence[Sequence["StoredWeight"]]) -> "StoredWeight":
        """One bank weight [E, ...] from ``experts[e]``, the weights whose rows expert e holds one after the other (gate
        before up).  The kernels take one format, group count and column grouping per bank and expert."""
        flat = [w for ws in experts for w in ws]
        if len({(w.levels.dtype, w.G, w.zero_point is None, w.g_idx is None) for w in flat}) > 1:
            raise ValueError(f"{name}: the weights of the experts mix formats or group counts")
        grouped = flat[0].g_idx is not None
        for e, ws in enumerate(experts):
            if grouped and not all(torch.equal(ws[0].g_idx, w.g_idx) for w in ws[1:]):
                raise ValueError(f"{name}: the Linears of expert {e} group their columns differently (weight_g_idx); "
                                 "the grouped GEMV takes one column grouping per expert")

        def rows(field: str) -> Optional[torch.Tensor]:
            if getattr(flat[0], field) is None:
                return None
            return torch.stack([torch.cat([getattr(w, field) for w in ws], 0) for ws in experts])

        return cls(rows("levels"), rows("scale"), rows("zero_point"),
                   torch.stack([ws[0].g_idx for ws in experts]) if grouped else None,
                   sum(w.N for w in experts[0]), flat[0].K)

    def leaves(self) -> Dict[str, torch.Tensor]:
        """Back to the checkpoint tensors ``from_leaves`` reads (one weight, no expert dimension)."""
        t = {"weight_packed" if self.int4 else "weight": self.levels, "weight_scale": self.scale,
             "weight_shape": torch.tensor([self.N, self.K])}
        if self.zero_point is not None:
            t["weight_zero_point"] = self.zero_point
        if self.g_idx is not None:
            t["weight_g_idx"] = self.g_idx
        return t
