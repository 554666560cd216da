"""Thin torch-tensor wrappers over the C ABI (``include/quantool_amd.h``).

torch is plumbing here: device memory, the current HIP stream and shape checks before a raw
pointer crosses the boundary (a wrong shape in a hand-written kernel is a GPU fault, so every
assumption the kernels make is asserted on the host first).  No arithmetic happens in torch.
"""
from __future__ import annotations

import ctypes
import logging
import os
from collections import namedtuple
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import QT_BF16, QT_F16, QT_F32, HipBackendError, check, load

_WS_CACHE: dict = {}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return QT_F32
    if t.dtype == torch.bfloat16:
        return QT_BF16
    if t.dtype == torch.float16:
        return QT_F16
    raise TypeError(f"unsupported dtype {t.dtype} (fp32 / bf16 / fp16 only)")


def _act16(X: torch.Tensor, name: str) -> int:
    """Activations cross the boundary in the model's own 16-bit dtype."""
    if not X.is_cuda:
        raise ValueError(f"{name} must be a device tensor (no CPU path exists)")
    if X.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{name} must be bf16 or fp16, got {X.dtype}")
    return QT_BF16 if X.dtype == torch.bfloat16 else QT_F16


def _rows16(X2: torch.Tensor) -> torch.Tensor:
    """[n, K] 16-bit rows as the Gram and statistics kernels load them (16 bytes per lane): unit column stride, a start
    that is 16-byte aligned and a pitch that is a multiple of 8 elements.  A view that is none of that (a column range
    of a wider tensor) is copied to a contiguous tensor first, as ``xtx_accumulate_f32`` does."""
    if X2.stride(1) != 1 or X2.data_ptr() % 16 or (X2.shape[0] > 1 and X2.stride(0) % 8):
        X2 = X2.contiguous()
    return X2


_FP32_ACT_WARNED = False


def as_act16(X: torch.Tensor) -> torch.Tensor:
    """Activations as the kernels take them: the model's own 16-bit dtype, untouched.  Upstream
    accumulates ``inp.float()``; bf16 and fp16 widen exactly, so nothing is lost.

    fp32 activations (an fp32 checkpoint): the Gram accumulation has its own fp32-accurate path
    (``xtx_accumulate_f32`` / ``HessianAccumulator``) and does not come here.  The STATISTICS passes (AWQ's mean |x|,
    SmoothQuant's channel min / max) take 16-bit rows, so for them -- and for the Gram pass under
    ``QT_FP32_ACTIVATIONS=bf16`` -- fp32 activations are rounded to bf16 (range over mantissa: an fp16 cast could
    overflow on outlier channels).  That downgrade is never silent: it is logged once per process, and with
    ``QT_FP32_ACTIVATIONS=error`` it is refused (``ValueError``)."""
    if X.dtype in (torch.bfloat16, torch.float16):
        return X
    wide_activation_policy(X.dtype)
    return X.to(torch.bfloat16)


def wide_gram_mode() -> str:
    """How the Gram accumulation takes fp32 activations: "exact" (default: the three-plane fp32-accurate product,
    6x the MFMA work), "bf16" (round them, logged once) or "error" -- ``QT_FP32_ACTIVATIONS``."""
    mode = os.environ.get("QT_FP32_ACTIVATIONS", "exact").lower()
    if mode not in ("exact", "bf16", "warn", "error"):
        raise ValueError(f"QT_FP32_ACTIVATIONS={mode!r}: expected exact, bf16 or error")
    return "bf16" if mode == "warn" else mode


def wide_activation_policy(dtype) -> None:
    """Log (once) or refuse the bf16 rounding of activations wider than 16 bits: see ``as_act16``."""
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"calibration activations must be floating point, got {dtype}")
    global _FP32_ACT_WARNED
    policy = os.environ.get("QT_FP32_ACTIVATIONS", "exact").lower()
    if policy == "error":
        raise ValueError(f"{dtype} calibration activations: this backend accumulates X^T X from 16-bit activations; "
                         "load the model in bf16 / fp16 (oneshot(precision=...)) or unset QT_FP32_ACTIVATIONS=error to "
                         "accept rounding them to bf16")
    if not _FP32_ACT_WARNED:
        _FP32_ACT_WARNED = True
        logging.getLogger(__name__).warning(
            f"{dtype} calibration activations are rounded to bf16 for the Gram / statistics passes (upstream accumulates "
            "them in fp32): Hessians differ at the 2^-9 level per activation.  Load the model in bf16 / fp16 to calibrate "
            "in its own dtype, or set QT_FP32_ACTIVATIONS=error to refuse")


def _req(t: torch.Tensor, dtype, name: str, ndim: Optional[int] = None):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (no CPU path exists)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-d, got shape {tuple(t.shape)}")


def workspace(nbytes: int, device, tag: str = "default") -> torch.Tensor:
    """Grow-only scratch buffer per (device, tag); reused across calls on the same stream."""
    # one scratch buffer per (device, stream, tag): groups running on different streams never share
    key = (str(device), _stream(), tag)
    buf = _WS_CACHE.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        _WS_CACHE[key] = buf
    return buf


def release_workspaces() -> None:
    _WS_CACHE.clear()


# ---- a7 -----------------------------------------------------------------------------------
XTX_CHAIN_STEP = 640    # chain_tokens is 0 or a positive multiple of this (one cut grid for both MFMA shapes)


def _chain_arg(chain_tokens) -> int:
    chain = int(chain_tokens)
    if chain < 0 or chain % XTX_CHAIN_STEP:
        raise ValueError(f"chain_tokens={chain_tokens!r} must be 0 or a positive multiple of {XTX_CHAIN_STEP}")
    return chain


def xtx_accumulate(X: torch.Tensor, G: torch.Tensor, chain_tokens: int = 0) -> None:
    """G[K,K] fp32 (lower triangle) += X^T X for X[..., K] bf16 / fp16 (leading dims flattened).

    ``chain_tokens`` > 0 (a multiple of 640): no fp32 accumulator chain inside the launch covers more than that many
    tokens -- the workgroups fold their accumulators into G (or their slab) at every cut and start again
    (``qt_xtx_accumulate_chained``).  0: the plain call."""
    lib = load()
    chain = _chain_arg(chain_tokens)
    xdt = _act16(X, "X")
    _req(G, torch.float32, "G", 2)
    K = G.shape[0]
    if G.shape[1] != K or not G.is_contiguous():
        raise ValueError("G must be contiguous [K, K]")
    if X.shape[-1] != K:
        raise ValueError(f"X last dim {X.shape[-1]} != K {K}")
    X2 = _rows16(X.reshape(-1, K))
    n = X2.shape[0]
    if n == 0:
        return
    ldx = X2.stride(0) if n > 1 else K
    nbytes = lib.qt_xtx_workspace_bytes(n, K)
    ws = workspace(nbytes, X.device, "xtx")
    if chain:
        check("qt_xtx_accumulate_chained", lib.qt_xtx_accumulate_chained(X2.data_ptr(), xdt, n, K, ldx, G.data_ptr(), chain,
                                                                         ws.data_ptr(), ws.numel(), _stream()))
        return
    check("qt_xtx_accumulate", lib.qt_xtx_accumulate(X2.data_ptr(), xdt, n, K, ldx, G.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), _stream()))


XTX_BATCH_MAX = 16      # problems per qt_xtx_accumulate_batched call


def xtx_batched_plan(n_tokens, K: int):
    """The item table ``qt_xtx_accumulate_batched`` would launch for these token counts (host only, no device):
    ``(items, n_slabs)``, ``items`` a list of ``(problem, ti, tj, first token tile, token tiles, slab or -1)``."""
    import ctypes

    lib = load()
    n = len(n_tokens)
    counts = (ctypes.c_int64 * n)(*[int(t) for t in n_tokens])
    n_items, n_slabs = ctypes.c_int(0), ctypes.c_int(0)
    check("qt_xtx_batched_plan", lib.qt_xtx_batched_plan(counts, n, K, None, 0, ctypes.byref(n_items),
                                                         ctypes.byref(n_slabs), None))
    rows = (ctypes.c_int32 * (6 * max(1, n_items.value)))()
    check("qt_xtx_batched_plan", lib.qt_xtx_batched_plan(counts, n, K, rows, n_items.value, ctypes.byref(n_items),
                                                         ctypes.byref(n_slabs), None))
    return [tuple(rows[6 * i:6 * i + 6]) for i in range(n_items.value)], n_slabs.value


def xtx_batched_workspace_bytes(n_tokens, K: int) -> int:
    """Workspace bytes ``qt_xtx_accumulate_batched`` needs for these token counts: a property of its plan, returned by
    ``qt_xtx_batched_plan`` (host only)."""
    import ctypes

    n = len(n_tokens)
    counts = (ctypes.c_int64 * n)(*[int(t) for t in n_tokens])
    need = ctypes.c_size_t(0)
    check("qt_xtx_batched_plan", load().qt_xtx_batched_plan(counts, n, K, None, 0, None, None, ctypes.byref(need)))
    return int(need.value)


def xtx_accumulate_batched(Xs, Gs, chain_tokens: int = 0) -> None:
    """``Gs[p]`` [K, K] fp32 (lower triangle) += ``Xs[p]``^T ``Xs[p]`` for every p, in one launch per 16 problems.
    One K, one 16-bit dtype and one device for the whole list; the token counts may differ.  Empty inputs are dropped;
    a strided input with a ragged token count (which the batched entry point refuses) goes through
    ``xtx_accumulate``.  Bits: see ``qt_xtx_accumulate_batched`` in the header.  ``chain_tokens`` as in
    ``xtx_accumulate``, counted from each work item's own first token (``qt_xtx_accumulate_batched_chained``)."""
    import ctypes

    lib = load()
    chain = _chain_arg(chain_tokens)
    Xs, Gs = list(Xs), list(Gs)
    if len(Xs) != len(Gs):
        raise ValueError(f"{len(Xs)} inputs for {len(Gs)} Gram matrices")
    if not Xs:
        return
    xdt = _act16(Xs[0], "Xs[0]")
    K = Gs[0].shape[0]
    batch = []
    for i, (X, G) in enumerate(zip(Xs, Gs)):
        if _act16(X, f"Xs[{i}]") != xdt:
            raise TypeError(f"Xs[{i}] is {X.dtype}, Xs[0] is {Xs[0].dtype}: one dtype per batch")
        _req(G, torch.float32, f"Gs[{i}]", 2)
        if tuple(G.shape) != (K, K) or not G.is_contiguous():
            raise ValueError(f"Gs[{i}] must be contiguous [{K}, {K}], got {tuple(G.shape)}")
        if X.shape[-1] != K:
            raise ValueError(f"Xs[{i}] last dim {X.shape[-1]} != K {K}")
        if X.device != Xs[0].device or G.device != Xs[0].device:
            raise ValueError(f"problem {i} is not on {Xs[0].device}: one device per batch")
        if any(G.data_ptr() == g.data_ptr() for _, g in batch):
            raise ValueError(f"Gs[{i}] is also an earlier problem's Gram matrix")
        X2 = _rows16(X.reshape(-1, K))
        n = X2.shape[0]
        if n == 0:
            continue
        if n % 64 and n > 1 and X2.stride(0) != K:
            xtx_accumulate(X2, G, chain)    # ragged and strided: two launches of the single entry point
            continue
        batch.append((X2, G))
    for b0 in range(0, len(batch), XTX_BATCH_MAX):
        part = batch[b0:b0 + XTX_BATCH_MAX]
        m = len(part)
        counts = (ctypes.c_int64 * m)(*[x.shape[0] for x, _ in part])
        pitches = (ctypes.c_int64 * m)(*[x.stride(0) if x.shape[0] > 1 else K for x, _ in part])
        xp = (ctypes.c_void_p * m)(*[x.data_ptr() for x, _ in part])
        gp = (ctypes.c_void_p * m)(*[g.data_ptr() for _, g in part])
        ws = workspace(xtx_batched_workspace_bytes([x.shape[0] for x, _ in part], K), Xs[0].device, "xtx_batched")
        if chain:
            check("qt_xtx_accumulate_batched_chained",
                  lib.qt_xtx_accumulate_batched_chained(xp, xdt, counts, pitches, K, gp, m, chain, ws.data_ptr(), ws.numel(),
                                                        _stream()))
            continue
        check("qt_xtx_accumulate_batched", lib.qt_xtx_accumulate_batched(xp, xdt, counts, pitches, K, gp, m, ws.data_ptr(),
                                                                         ws.numel(), _stream()))


def xtx_accumulate_f32(X: torch.Tensor, G: torch.Tensor) -> None:
    """G[K,K] fp32 (lower triangle) += X^T X for fp32 X[..., K]: the fp32-accurate three-plane product (an fp32
    checkpoint's activations, which upstream accumulates as `inp.float()`)."""
    lib = load()
    _req(X, torch.float32, "X")
    _req(G, torch.float32, "G", 2)
    K = G.shape[0]
    if G.shape[1] != K or not G.is_contiguous():
        raise ValueError("G must be contiguous [K, K]")
    if X.shape[-1] != K:
        raise ValueError(f"X last dim {X.shape[-1]} != K {K}")
    if K % 4:
        raise ValueError(f"fp32 activations need in_features % 4 == 0 (K = {K})")
    X2 = X.reshape(-1, K)
    if X2.stride(1) != 1 or X2.stride(0) % 4 or X2.data_ptr() % 16:
        X2 = X2.contiguous()
    n = X2.shape[0]
    if n == 0:
        return
    ldx = X2.stride(0) if n > 1 else K
    ws = workspace(lib.qt_xtx_accumulate_f32_workspace_bytes(n, K), X.device, "xtx_f32")
    check("qt_xtx_accumulate_f32", lib.qt_xtx_accumulate_f32(X2.data_ptr(), n, K, ldx, G.data_ptr(), ws.data_ptr(),
                                                             ws.numel(), _stream()))


# ---- a12 / a13 ----------------------------------------------------------------------------
def act_stats_accumulate(X: torch.Tensor, abs_sum: Optional[torch.Tensor] = None,
                         cmin: Optional[torch.Tensor] = None, cmax: Optional[torch.Tensor] = None) -> None:
    lib = load()
    xdt = _act16(X, "X")
    K = X.shape[-1]
    X2 = _rows16(X.reshape(-1, K))
    n = X2.shape[0]
    for name, t in (("abs_sum", abs_sum), ("cmin", cmin), ("cmax", cmax)):
        if t is not None:
            _req(t, torch.float32, name, 1)
            if t.numel() != K or not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous [K]")
    if n == 0:
        return
    ldx = X2.stride(0) if n > 1 else K
    ws = workspace(lib.qt_act_stats_workspace_bytes(n, K), X.device, "stats")
    check("qt_act_stats_accumulate", lib.qt_act_stats_accumulate(
        X2.data_ptr(), xdt, n, K, ldx, _ptr(abs_sum), _ptr(cmin), _ptr(cmax), ws.data_ptr(), ws.numel(), _stream()))


# ---- a8 / a9 ------------------------------------------------------------------------------
def hessian_diag(G: torch.Tensor, n_samples: int) -> torch.Tensor:
    lib = load()
    _req(G, torch.float32, "G", 2)
    K = G.shape[0]
    out = torch.empty(K, dtype=torch.float32, device=G.device)
    check("qt_hessian_diag", lib.qt_hessian_diag(G.data_ptr(), K, n_samples, out.data_ptr(), _stream()))
    return out


def argsort_desc(values: torch.Tensor):
    """Stable descending argsort on the device: returns (perm int32[K], inv int32[K])."""
    lib = load()
    _req(values, torch.float32, "values", 1)
    K = values.numel()
    assert values.is_contiguous()
    perm = torch.empty(K, dtype=torch.int32, device=values.device)
    inv = torch.empty(K, dtype=torch.int32, device=values.device)
    check("qt_argsort_desc", lib.qt_argsort_desc(values.data_ptr(), K, perm.data_ptr(), inv.data_ptr(), _stream()))
    return perm, inv


def factor_buffer(K: int, device) -> torch.Tensor:
    """Flat fp32 buffer that holds the factor U ([K, K], its first K*K elements: ``factor_view``) and, before U is
    written, serves ``hessian_prepare`` as scratch (``scratch=``): the two-pass prepare needs a K x K symmetric copy
    of G -- 0.8 GB at K = 14336, 3.3 GB at K = 28672 -- which would otherwise sit in a grow-only per-stream workspace
    for the life of the process next to the factor it precedes."""
    return torch.empty(K * K + 256, dtype=torch.float32, device=device)


def factor_view(buf: torch.Tensor, K: int) -> torch.Tensor:
    return buf[:K * K].view(K, K)


def hessian_prepare(G: torch.Tensor, n_samples: int, percdamp: float, perm: Optional[torch.Tensor] = None,
                    A_out: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None,
                    damp_out: Optional[torch.Tensor] = None):
    """Returns (A flipped+damped [K,K] fp32 upper-valid, dead uint8[K], diag fp32[K]).  ``scratch``: a contiguous
    device tensor whose bytes may be used as the workspace (e.g. ``factor_buffer``: the buffer the factor will be
    written to afterwards); too small or absent: the cached per-stream workspace.  ``damp_out``: fp32 device tensor
    whose first element receives the damping term that was added to the diagonal (no host read)."""
    lib = load()
    _req(G, torch.float32, "G", 2)
    K = G.shape[0]
    if not G.is_contiguous() or G.shape[1] != K:
        raise ValueError("G must be contiguous [K, K]")
    if perm is not None:
        _req(perm, torch.int32, "perm", 1)
        if perm.numel() != K or not perm.is_contiguous():
            raise ValueError("perm must be contiguous int32[K]")
    A = A_out if A_out is not None else torch.empty((K, K), dtype=torch.float32, device=G.device)
    _req(A, torch.float32, "A", 2)
    if A.shape != (K, K) or not A.is_contiguous():
        raise ValueError("A must be contiguous [K, K]")
    dead = torch.empty(K, dtype=torch.uint8, device=G.device)
    diag = torch.empty(K, dtype=torch.float32, device=G.device)
    need = lib.qt_hessian_prepare_workspace_bytes(K)
    if scratch is not None and scratch.is_cuda and scratch.is_contiguous() and scratch.numel() * scratch.element_size() >= need:
        ws = scratch.view(torch.uint8).reshape(-1)
    else:
        ws = workspace(need, G.device, "prep")
    if damp_out is not None:
        _req(damp_out, torch.float32, "damp_out", damp_out.dim())
        if damp_out.numel() < 1 or damp_out.device != G.device:
            raise ValueError("damp_out must be a non-empty fp32 tensor on G's device")
        check("qt_hessian_prepare_damp", lib.qt_hessian_prepare_damp(
            G.data_ptr(), K, int(n_samples), float(percdamp), _ptr(perm), A.data_ptr(), dead.data_ptr(), diag.data_ptr(),
            damp_out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return A, dead, diag
    check("qt_hessian_prepare", lib.qt_hessian_prepare(G.data_ptr(), K, int(n_samples), float(percdamp), _ptr(perm),
                                                       A.data_ptr(), dead.data_ptr(), diag.data_ptr(), ws.data_ptr(),
                                                       ws.numel(), _stream()))
    return A, dead, diag


def _min_eig_lb(lb: torch.Tensor, n: int, device) -> torch.Tensor:
    _req(lb, torch.float32, "min_eig_lb", lb.dim())
    if lb.numel() != n or not lb.is_contiguous() or lb.device != device:
        raise ValueError(f"min_eig_lb must be a contiguous fp32 device tensor of {n} value(s)")
    return lb


def cholesky_inverse_upper(A: torch.Tensor, U_out: Optional[torch.Tensor] = None,
                           min_eig_lb: Optional[torch.Tensor] = None):
    """A (flipped damped Hessian, destroyed) -> (U upper [K,K] fp32, info int32[1] device).  ``min_eig_lb``: fp32 device
    tensor of one value, a lower bound on lambda_min(A): the long block-row products then run on two fp16 planes."""
    lib = load()
    _req(A, torch.float32, "A", 2)
    K = A.shape[0]
    if A.shape != (K, K) or not A.is_contiguous():
        raise ValueError("A must be contiguous [K, K]")
    U = U_out if U_out is not None else torch.empty((K, K), dtype=torch.float32, device=A.device)
    if U.shape != (K, K) or not U.is_contiguous() or U.dtype != torch.float32:
        raise ValueError("U must be contiguous fp32 [K, K]")
    info = torch.zeros(1, dtype=torch.int32, device=A.device)
    ws = workspace(lib.qt_cholesky_inverse_upper_workspace_bytes(K), A.device, "chol")
    if min_eig_lb is not None:
        lb = _min_eig_lb(min_eig_lb, 1, A.device)
        check("qt_cholesky_inverse_upper_bounded", lib.qt_cholesky_inverse_upper_bounded(
            A.data_ptr(), K, U.data_ptr(), info.data_ptr(), lb.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return U, info
    check("qt_cholesky_inverse_upper", lib.qt_cholesky_inverse_upper(A.data_ptr(), K, U.data_ptr(), info.data_ptr(),
                                                                     ws.data_ptr(), ws.numel(), _stream()))
    return U, info


MAX_BATCH = 16      # problems per batched factorisation / groups per grouped sweep (SG_MAX_BATCH / SG_MAX_GROUPS)


def cholesky_inverse_upper_batched(A: torch.Tensor, U: torch.Tensor, min_eig_lb: Optional[torch.Tensor] = None):
    """n problems of one size in every launch of the chain.  ``A``: [n, K, K] fp32 (flipped damped Hessians, destroyed)
    -- or any tensor whose [b] slices are contiguous K x K matrices at a uniform stride -- ``U`` likewise (written).
    Returns info int32[n] (device).  Bit-identical per problem to ``cholesky_inverse_upper``.  ``min_eig_lb``: fp32[n]
    on the device, as in ``cholesky_inverse_upper``."""
    lib = load()
    _req(A, torch.float32, "A", 3)
    _req(U, torch.float32, "U", 3)
    n, K, K2 = A.shape
    if K != K2 or tuple(U.shape) != (n, K, K) or not (1 <= n <= MAX_BATCH):
        raise ValueError(f"A / U must be [n <= {MAX_BATCH}, K, K], got {tuple(A.shape)} / {tuple(U.shape)}")
    for name, t in (("A", A), ("U", U)):
        if t.stride(2) != 1 or t.stride(1) != K or (n > 1 and (t.stride(0) < K * K or t.stride(0) % 4)):
            raise ValueError(f"{name}: every [b] slice must be a contiguous K x K matrix at a stride that is a multiple of 4")
    info = torch.zeros(n, dtype=torch.int32, device=A.device)
    ws = workspace(lib.qt_cholesky_inverse_upper_batched_workspace_bytes(K, n), A.device, "chol")
    if min_eig_lb is not None:
        lb = _min_eig_lb(min_eig_lb, n, A.device)
        check("qt_cholesky_inverse_upper_batched_bounded", lib.qt_cholesky_inverse_upper_batched_bounded(
            A.data_ptr(), A.stride(0) if n > 1 else K * K, K, U.data_ptr(), U.stride(0) if n > 1 else K * K,
            info.data_ptr(), n, lb.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return info
    check("qt_cholesky_inverse_upper_batched", lib.qt_cholesky_inverse_upper_batched(
        A.data_ptr(), A.stride(0) if n > 1 else K * K, K, U.data_ptr(), U.stride(0) if n > 1 else K * K, info.data_ptr(), n,
        ws.data_ptr(), ws.numel(), _stream()))
    return info


# ---- a10 ----------------------------------------------------------------------------------
def group_minmax_qparams(W: torch.Tensor, group_size: int, symmetric: bool = True, num_bits: int = 4):
    """Returns (scale[R,G], zp[R,G], scale_t[G,R], zp_t[G,R]) fp32."""
    lib = load()
    if W.dim() != 2 or not W.is_cuda or W.stride(1) != 1:
        raise ValueError("W must be a 2-d device tensor with unit column stride")
    R, K = W.shape
    gs = K if group_size <= 0 else group_size
    if K % gs:
        raise ValueError(f"K={K} not divisible by group_size={gs}")
    G = K // gs
    dev = W.device
    scale = torch.empty((R, G), dtype=torch.float32, device=dev)
    zp = torch.empty((R, G), dtype=torch.float32, device=dev)
    scale_t = torch.empty((G, R), dtype=torch.float32, device=dev)
    zp_t = torch.empty((G, R), dtype=torch.float32, device=dev)
    check("qt_group_minmax_qparams", lib.qt_group_minmax_qparams(
        W.data_ptr(), _dtype_code(W), R, K, W.stride(0), gs, int(bool(symmetric)), num_bits, scale.data_ptr(),
        zp.data_ptr(), scale_t.data_ptr(), zp_t.data_ptr(), _stream()))
    return scale, zp, scale_t, zp_t


def weight_gather_f32(W: torch.Tensor, perm: Optional[torch.Tensor] = None, dead: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = load()
    if W.dim() != 2 or not W.is_cuda or W.stride(1) != 1:
        raise ValueError("W must be a 2-d device tensor with unit column stride")
    R, K = W.shape
    if perm is not None:
        _req(perm, torch.int32, "perm", 1)
        assert perm.numel() == K and perm.is_contiguous()
    if dead is not None:
        _req(dead, torch.uint8, "dead", 1)
        assert dead.numel() == K and dead.is_contiguous()
    if out is None:
        out = torch.empty((R, K), dtype=torch.float32, device=W.device)
    assert out.shape == (R, K) and out.is_contiguous() and out.dtype == torch.float32
    check("qt_weight_gather_f32", lib.qt_weight_gather_f32(W.data_ptr(), _dtype_code(W), R, K, W.stride(0),
                                                           _ptr(perm), _ptr(dead), out.data_ptr(), _stream()))
    return out


def weight_gather_qparams(W: torch.Tensor, perm: Optional[torch.Tensor], dead: Optional[torch.Tensor], group_size: int,
                          symmetric: bool, num_bits: int, out: torch.Tensor, scale: torch.Tensor, zp: torch.Tensor,
                          scale_t: Optional[torch.Tensor] = None, zp_t: Optional[torch.Tensor] = None) -> None:
    """``group_minmax_qparams(W)`` and ``weight_gather_f32(W, perm, dead)`` in one read of W.  ``out`` fp32 [R, K],
    ``scale`` / ``zp`` fp32 [R, G] contiguous; ``scale_t`` / ``zp_t``: [G, R] views with unit column stride (a column
    range of a table spanning more rows is fine: the row stride is passed on)."""
    lib = load()
    if W.dim() != 2 or not W.is_cuda or W.stride(1) != 1:
        raise ValueError("W must be a 2-d device tensor with unit column stride")
    R, K = W.shape
    gs = K if group_size <= 0 else group_size
    if K % gs:
        raise ValueError(f"K={K} not divisible by group_size={gs}")
    G = K // gs
    for name, t, shape in (("out", out, (R, K)), ("scale", scale, (R, G)), ("zp", zp, (R, G))):
        _req(t, torch.float32, name, 2)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous {shape}")
    ld_t = 0
    for name, t in (("scale_t", scale_t), ("zp_t", zp_t)):
        if t is not None:
            _req(t, torch.float32, name, 2)
            if tuple(t.shape) != (G, R) or t.stride(1) != 1 or (ld_t and t.stride(0) != ld_t):
                raise ValueError(f"{name} must be a [G, R] view with unit column stride (and the row stride of its twin)")
            ld_t = t.stride(0) if G > 1 else max(R, t.stride(0))
    for name, t, dt in (("perm", perm, torch.int32), ("dead", dead, torch.uint8)):
        if t is not None:
            _req(t, dt, name, 1)
            if t.numel() != K or not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous [K]")
    check("qt_weight_gather_qparams", lib.qt_weight_gather_qparams(
        W.data_ptr(), _dtype_code(W), R, K, W.stride(0), _ptr(perm), _ptr(dead), group_size, int(bool(symmetric)), num_bits,
        out.data_ptr(), scale.data_ptr(), zp.data_ptr(), _ptr(scale_t), _ptr(zp_t), ld_t, _stream()))


# ---- a11 ----------------------------------------------------------------------------------
def gptq_sweep(W: torch.Tensor, U: torch.Tensor, scale_t: torch.Tensor, zp_t: torch.Tensor, g_idx: torch.Tensor,
               blocksize: int = 128, num_bits: int = 4):
    """In-place on W (fp32 [R,K], sweep order).  Returns (Qt int8 [K,R], loss fp32 [R])."""
    lib = load()
    _req(W, torch.float32, "W", 2)
    _req(U, torch.float32, "U", 2)
    _req(scale_t, torch.float32, "scale_t", 2)
    _req(zp_t, torch.float32, "zp_t", 2)
    _req(g_idx, torch.int32, "g_idx", 1)
    R, K = W.shape
    G = scale_t.shape[0]
    if not (W.is_contiguous() and U.is_contiguous() and scale_t.is_contiguous() and zp_t.is_contiguous()
            and g_idx.is_contiguous()):
        raise ValueError("all sweep operands must be contiguous")
    if U.shape != (K, K) or scale_t.shape != (G, R) or zp_t.shape != (G, R) or g_idx.numel() != K:
        raise ValueError("sweep operand shapes inconsistent")
    Qt = torch.empty((K, R), dtype=torch.int8, device=W.device)
    loss = torch.empty(R, dtype=torch.float32, device=W.device)
    ws = workspace(lib.qt_gptq_sweep_workspace_bytes(R, K, blocksize), W.device, "sweep")
    check("qt_gptq_sweep", lib.qt_gptq_sweep(W.data_ptr(), R, K, U.data_ptr(), scale_t.data_ptr(), zp_t.data_ptr(), G,
                                             g_idx.data_ptr(), blocksize, num_bits, Qt.data_ptr(), loss.data_ptr(),
                                             ws.data_ptr(), ws.numel(), _stream()))
    return Qt, loss


def gptq_sweep_grouped(W: torch.Tensor, U: torch.Tensor, row_end, scale_t: torch.Tensor, zp_t: torch.Tensor,
                       g_idx: torch.Tensor, blocksize: int = 128, num_bits: int = 4):
    """Several Linear groups of one in_features as ONE stacked sweep.  W fp32 [R_total, K] (in place), U [n, K, K] (its
    [g] slices contiguous K x K at a uniform stride), ``row_end``: list of n cumulative row counts (every boundary but
    the last a multiple of 128), g_idx int32 [n, K].  Returns (Qt int8 [K, R_total], loss fp32 [R_total])."""
    import ctypes

    lib = load()
    _req(W, torch.float32, "W", 2)
    _req(U, torch.float32, "U", 3)
    _req(scale_t, torch.float32, "scale_t", 2)
    _req(zp_t, torch.float32, "zp_t", 2)
    _req(g_idx, torch.int32, "g_idx", 2)
    R, K = W.shape
    n = U.shape[0]
    G = scale_t.shape[0]
    row_end = [int(r) for r in row_end]
    if not (W.is_contiguous() and scale_t.is_contiguous() and zp_t.is_contiguous() and g_idx.is_contiguous()):
        raise ValueError("all sweep operands must be contiguous")
    if (tuple(U.shape) != (n, K, K) or U.stride(2) != 1 or U.stride(1) != K or scale_t.shape != (G, R) or zp_t.shape != (G, R)
            or tuple(g_idx.shape) != (n, K) or len(row_end) != n or not (1 <= n <= MAX_BATCH)):
        raise ValueError("grouped sweep operand shapes inconsistent")
    if row_end[-1] != R or any(b <= a for a, b in zip([0] + row_end[:-1], row_end)) or any(r % 128 for r in row_end[:-1]):
        raise ValueError(f"row_end={row_end}: ascending, every boundary but the last a multiple of 128, last == R ({R})")
    Qt = torch.empty((K, R), dtype=torch.int8, device=W.device)
    loss = torch.empty(R, dtype=torch.float32, device=W.device)
    ws = workspace(lib.qt_gptq_sweep_workspace_bytes(R, K, blocksize), W.device, "sweep")
    ends = (ctypes.c_int32 * n)(*row_end)
    check("qt_gptq_sweep_grouped", lib.qt_gptq_sweep_grouped(
        W.data_ptr(), R, K, U.data_ptr(), U.stride(0) if n > 1 else K * K, n, ctypes.cast(ends, ctypes.c_void_p),
        scale_t.data_ptr(), zp_t.data_ptr(), G, g_idx.data_ptr(), blocksize, num_bits, Qt.data_ptr(), loss.data_ptr(),
        ws.data_ptr(), ws.numel(), _stream()))
    return Qt, loss


# ---- a14 ----------------------------------------------------------------------------------
def pack_int4(Qt: torch.Tensor, col_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = load()
    _req(Qt, torch.int8, "Qt", 2)
    K, R = Qt.shape
    assert Qt.is_contiguous()
    if col_src is not None:
        _req(col_src, torch.int32, "col_src", 1)
        assert col_src.numel() == K and col_src.is_contiguous()
    packed = torch.empty((R, (K + 7) // 8), dtype=torch.int32, device=Qt.device)
    check("qt_pack_int4", lib.qt_pack_int4(Qt.data_ptr(), R, K, _ptr(col_src), packed.data_ptr(), _stream()))
    return packed


def dequantize(Qt: torch.Tensor, scale: torch.Tensor, zp: torch.Tensor, g_of_col: torch.Tensor,
               col_src: Optional[torch.Tensor] = None, dtype=torch.float32) -> torch.Tensor:
    lib = load()
    _req(Qt, torch.int8, "Qt", 2)
    K, R = Qt.shape
    _req(scale, torch.float32, "scale", 2)
    _req(zp, torch.float32, "zp", 2)
    _req(g_of_col, torch.int32, "g_of_col", 1)
    G = scale.shape[1]
    assert scale.shape == (R, G) and zp.shape == (R, G) and g_of_col.numel() == K
    assert Qt.is_contiguous() and scale.is_contiguous() and zp.is_contiguous() and g_of_col.is_contiguous()
    if col_src is not None:
        _req(col_src, torch.int32, "col_src", 1)
        assert col_src.numel() == K and col_src.is_contiguous()
    out = torch.empty((R, K), dtype=dtype, device=Qt.device)
    check("qt_dequantize", lib.qt_dequantize(Qt.data_ptr(), R, K, _ptr(col_src), scale.data_ptr(), zp.data_ptr(), G,
                                             g_of_col.data_ptr(), out.data_ptr(), _dtype_code(out), out.stride(0),
                                             _stream()))
    return out


# ---- A8 runtime: dynamic per-token int8 activations, int8 x int8 GEMM ------------------------------
def _x2d(X: torch.Tensor, name: str) -> int:
    """The dtype code of ``X``, a bf16 / fp16 device matrix [rows, columns] with unit column stride (any row pitch)."""
    code = _act16(X, name)
    if X.dim() != 2 or X.stride(1) != 1:
        raise ValueError(f"{name} must be 2-d [rows, columns] with unit column stride, got shape {tuple(X.shape)} "
                         f"strides {X.stride()}")
    return code


def quantize_tokens_i8(X: torch.Tensor, symmetric: bool = True, col_perm: Optional[torch.Tensor] = None):
    """X [M, K] bf16 / fp16 (unit column stride, any row pitch) -> (Xq int8 [M, K], s_x fp32 [M], zp_x int32 [M] or
    None when symmetric); with ``col_perm`` (int32 [K]) Xq[m, k] = q(X[m, col_perm[k]])."""
    lib = load()
    code = _x2d(X, "X")
    M, K = X.shape
    if M == 0 or K == 0:
        raise ValueError(f"X must be non-empty, got shape {tuple(X.shape)}")
    if col_perm is not None:
        _req(col_perm, torch.int32, "col_perm", 1)
        if col_perm.numel() != K or not col_perm.is_contiguous():
            raise ValueError(f"col_perm must be contiguous int32 [{K}]")
    Xq = torch.empty((M, K), dtype=torch.int8, device=X.device)
    s_x = torch.empty(M, dtype=torch.float32, device=X.device)
    zp_x = None if symmetric else torch.empty(M, dtype=torch.int32, device=X.device)
    check("qt_quantize_tokens_i8", lib.qt_quantize_tokens_i8(
        X.data_ptr(), code, M, K, X.stride(0), _ptr(col_perm), int(bool(symmetric)), Xq.data_ptr(), s_x.data_ptr(),
        _ptr(zp_x), _stream()))
    return Xq, s_x, zp_x


ACTS = {"silu": 0}   # qt_act


def act_mul_quantize_i8(gate: torch.Tensor, up: torch.Tensor, symmetric: bool = True,
                        col_perm: Optional[torch.Tensor] = None, act: str = "silu", return_h: bool = False):
    """``quantize_tokens_i8(act(gate) * up, symmetric, col_perm)`` in one pass (``qt_act_mul_quantize_i8``): gate and up
    [M, K] bf16 / fp16 of one dtype (unit column stride, any row pitch each: the two halves of one [M, 2K] tensor are
    taken as they are) -> (Xq, s_x, zp_x), and with ``return_h`` the intermediate ``act(gate) * up`` [M, K] as well."""
    lib = load()
    code = _x2d(gate, "gate")
    if _x2d(up, "up") != code or up.shape != gate.shape or up.device != gate.device:
        raise ValueError(f"gate and up must agree in shape, dtype and device, got {tuple(gate.shape)} {gate.dtype} "
                         f"and {tuple(up.shape)} {up.dtype}")
    if act not in ACTS:
        raise ValueError(f"act must be one of {sorted(ACTS)}, got {act!r}")
    M, K = gate.shape
    if M == 0 or K == 0:
        raise ValueError(f"gate must be non-empty, got shape {tuple(gate.shape)}")
    if col_perm is not None:
        _req(col_perm, torch.int32, "col_perm", 1)
        if col_perm.numel() != K or not col_perm.is_contiguous():
            raise ValueError(f"col_perm must be contiguous int32 [{K}]")
    Xq = torch.empty((M, K), dtype=torch.int8, device=gate.device)
    s_x = torch.empty(M, dtype=torch.float32, device=gate.device)
    zp_x = None if symmetric else torch.empty(M, dtype=torch.int32, device=gate.device)
    H = torch.empty((M, K), dtype=gate.dtype, device=gate.device) if return_h else None
    # a one-row view may carry any stride(0): the pitch of a single row is never used, K keeps the host check quiet
    ldg = gate.stride(0) if M > 1 else max(gate.stride(0), K)
    ldu = up.stride(0) if M > 1 else max(up.stride(0), K)
    check("qt_act_mul_quantize_i8", lib.qt_act_mul_quantize_i8(
        gate.data_ptr(), ldg, up.data_ptr(), ldu, code, M, K, ACTS[act], _ptr(col_perm), int(bool(symmetric)),
        Xq.data_ptr(), s_x.data_ptr(), _ptr(zp_x), _ptr(H), K, _stream()))
    return (Xq, s_x, zp_x, H) if return_h else (Xq, s_x, zp_x)


def rmsnorm_quantize_i8(X: torch.Tensor, weight: torch.Tensor, eps: float, symmetric: bool = True,
                        col_perm: Optional[torch.Tensor] = None, return_rstd: bool = False):
    """``Y = weight * RMSNorm(X)`` as transformers' ``LlamaRMSNorm.forward`` leaves it, and ``quantize_tokens_i8(Y,
    symmetric, col_perm)``, in one pass (``qt_rmsnorm_quantize_i8``): X [M, K] bf16 / fp16 (unit column stride, any row
    pitch), weight [K] of the same dtype on the same device -> (Y [M, K], Xq, s_x, zp_x), and with ``return_rstd`` the
    rows' fp32 ``rsqrt(mean(x^2) + eps)`` [M] as well."""
    code = _x2d(X, "X")
    if not weight.is_cuda or weight.device != X.device:
        raise ValueError(f"weight must be a device tensor on X's device {X.device}, got {weight.device}")
    if weight.dtype != X.dtype:
        raise TypeError(f"weight must be of X's dtype {X.dtype}, got {weight.dtype}")
    M, K = X.shape
    if M == 0 or K == 0:
        raise ValueError(f"X must be non-empty, got shape {tuple(X.shape)}")
    if weight.dim() != 1 or weight.numel() != K or not weight.is_contiguous():
        raise ValueError(f"weight must be contiguous [{K}], got shape {tuple(weight.shape)}")
    if col_perm is not None:
        _req(col_perm, torch.int32, "col_perm", 1)
        if col_perm.numel() != K or not col_perm.is_contiguous():
            raise ValueError(f"col_perm must be contiguous int32 [{K}]")
    eps = float(eps)
    if not (eps >= 0.0 and eps != float("inf")):
        raise ValueError(f"eps must be finite and not negative, got {eps!r}")
    lib = load()
    Y = torch.empty((M, K), dtype=X.dtype, device=X.device)
    Xq = torch.empty((M, K), dtype=torch.int8, device=X.device)
    s_x = torch.empty(M, dtype=torch.float32, device=X.device)
    zp_x = None if symmetric else torch.empty(M, dtype=torch.int32, device=X.device)
    rstd = torch.empty(M, dtype=torch.float32, device=X.device) if return_rstd else None
    # a one-row view may carry any stride(0): the pitch of a single row is never used, K keeps the host check quiet
    ldx = X.stride(0) if M > 1 else max(X.stride(0), K)
    check("qt_rmsnorm_quantize_i8", lib.qt_rmsnorm_quantize_i8(
        X.data_ptr(), ldx, weight.data_ptr(), code, M, K, eps, _ptr(col_perm), int(bool(symmetric)), Xq.data_ptr(),
        s_x.data_ptr(), _ptr(zp_x), Y.data_ptr(), K, _ptr(rstd), _stream()))
    return (Y, Xq, s_x, zp_x, rstd) if return_rstd else (Y, Xq, s_x, zp_x)


def _i8_operands(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, K: Optional[int],
                 zp_x: Optional[torch.Tensor], wsum: Optional[torch.Tensor], out_dtype, experts: bool = False):
    """Checks the operands of ``qt_gemm_i8`` -- or, with ``experts``, of ``qt_gemm_i8_grouped``: E weights stacked
    along a leading dimension; returns (format, N, K, G)."""
    _req(Xq, torch.int8, "Xq", 2)
    M, Kx = Xq.shape
    if not Xq.is_contiguous():
        raise ValueError("Xq must be contiguous [M, K]")
    nd = 3 if experts else 2
    if not Wq.is_cuda or Wq.dim() != nd or not Wq.is_contiguous():
        raise ValueError(f"Wq must be a contiguous {nd}-d device tensor")
    E = "E, " if experts else ""
    rows = list(Wq.shape[:-1])                             # [E, N] or [N]
    N = rows[-1]
    if K is not None and K != Kx:
        raise ValueError(f"K={K} but Xq has {Kx} columns")
    K = Kx
    if Wq.dtype == torch.int8:
        fmt = _lib.QT_W_INT8
        if Wq.shape[-1] != K:
            raise ValueError(f"int8 Wq must be [{E}N, {K}], got {tuple(Wq.shape)}")
    elif Wq.dtype == torch.int32:
        fmt = _lib.QT_W_INT4_PACKED
        if Wq.shape[-1] != (K + 7) // 8:
            raise ValueError(f"packed int4 Wq must be [{E}N, ceil(K/8) = {(K + 7) // 8}], got {tuple(Wq.shape)}")
    else:
        raise TypeError(f"Wq must be int8 [{E}N, K] or packed int4 int32 [{E}N, ceil(K/8)], got {Wq.dtype}")
    if 0 in (M, K, *rows):
        raise ValueError(f"empty GEMM: Xq {tuple(Xq.shape)}, Wq {tuple(Wq.shape)}")
    if K > 32768:
        raise ValueError(f"K={K} > 32768: the int32 accumulator could overflow")
    _req(s_x, torch.float32, "s_x", 1)
    _req(s_w, torch.float32, "s_w", nd)
    G = s_w.shape[-1]
    if s_x.numel() != M or not s_x.is_contiguous():
        raise ValueError(f"s_x must be contiguous fp32 [{M}]")
    if list(s_w.shape[:-1]) != rows or G not in (1, (K + 127) // 128) or not s_w.is_contiguous():
        raise ValueError(f"s_w must be contiguous fp32 [{E}{N}, 1 or {(K + 127) // 128}], got {tuple(s_w.shape)}")
    if zp_x is not None:
        _req(zp_x, torch.int32, "zp_x", 1)
        if zp_x.numel() != M or not zp_x.is_contiguous():
            raise ValueError(f"zp_x must be contiguous int32 [{M}]")
        if wsum is None:
            raise ValueError("zp_x needs wsum (per-group row sums of the weight levels)")
    if wsum is not None:
        _req(wsum, torch.int32, "wsum", nd)
        if list(wsum.shape) != rows + [G] or not wsum.is_contiguous():
            raise ValueError(f"wsum must be contiguous int32 [{E}{N}, {G}]")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"out_dtype must be bf16 or fp16, got {out_dtype}")
    return fmt, N, K, G


@dataclass(frozen=True)
class I8Form:
    """One int8 GEMM entry point and what it takes of the operands ``_i8_operands`` admits.  ``groups`` is the rule for
    G = s_w.shape[-1]: "any" (1 or ceil(K/128)), "one", "per_unit" (K / k_unit) or "one_or_per_unit".  A form without
    a ``k_unit`` takes every K, weight format, G and alignment the tiled kernel takes."""
    entry: str
    min_m: int = 1
    max_m: Optional[int] = None
    dtypes: tuple = (torch.int8, torch.int32)
    k_unit: Optional[int] = None
    groups: str = "any"
    aligned16: bool = False
    experts: bool = False
    max_e: Optional[int] = None      # experts a workgroup walks
    x_rows: bool = False             # the entry point takes the number of rows of Xq behind ldy
    slots: Optional[int] = None      # half panels resident in LDS
    lead: Optional[int] = None       # half panels the LDS-DMA runs ahead of the MFMAs
    # an expert form whose grid's second dimension holds R // tile_rows + min(E, R) row-tile slots (<= 65535); None:
    # the rings' count of 256-row tiles
    tile_rows: Optional[int] = None


_RING = dict(dtypes=(torch.int8,), k_unit=128, groups="one", aligned16=True, slots=8, lead=6)
I8_FORMS = {f.entry: f for f in (
    I8Form("qt_gemm_i8"),
    I8Form("qt_gemm_i8_skinny", max_m=16),
    I8Form("qt_gemm_i8_mid", max_m=128, k_unit=128, groups="one_or_per_unit", aligned16=True),
    I8Form("qt_gemm_i8_ring", **_RING),
    I8Form("qt_gemm_i8_ring_w4", **{**_RING, "dtypes": (torch.int32,), "groups": "per_unit"}),
    I8Form("qt_gemm_i8_grouped", experts=True),
    I8Form("qt_gemm_i8_skinny_grouped", experts=True),
    I8Form("qt_gemm_i8_ring_grouped", experts=True, max_e=4096, x_rows=True, **_RING),
)}
# The W4A8 bank's ring form.  Its entry point is of the qt_moe_* family and its row stands beside the table, not in it,
# because the table is the set of qt_gemm_i8* entry points; to fold it in, rename the entry point and move this row.
I8_MOE_RING_W4_FORM = I8Form("qt_moe_gemm_i8_ring_w4", experts=True, max_e=4096, x_rows=True,
                             **{**_RING, "dtypes": (torch.int32,), "groups": "per_unit"})
# The bank form between the decode range and the rings: qt_gemm_i8_mid's tile over E weight matrices.  Beside the table
# for the same reason.
I8_MOE_WIDE_FORM = I8Form("qt_moe_gemm_i8_wide", experts=True, x_rows=True, max_e=4096, k_unit=128,
                          groups="one_or_per_unit", aligned16=True, tile_rows=128)
# The short-prompt form: qt_gemm_i8_ring's tile over a k-range plus a reduce pass; it takes what the dense ring takes.
# Beside the table for the same reason (its entry point carries a split count and a workspace behind ldy).
I8_SPLITK_FORM = I8Form("qt_splitk_gemm_i8", **_RING)

I8_SKINNY_MAX_M = I8_FORMS["qt_gemm_i8_skinny"].max_m   # rows of Xq qt_gemm_i8_skinny takes
# k-bytes qt_gemm_i8_ring fetches per row at a time (QT_I8_RING_K_UNIT): K must be a multiple
I8_RING_K_UNIT = I8_FORMS["qt_gemm_i8_ring"].k_unit
I8_RING_SLOTS = I8_FORMS["qt_gemm_i8_ring"].slots       # half panels (128 rows x 128 k-bytes) resident in LDS
I8_RING_LEAD = I8_FORMS["qt_gemm_i8_ring"].lead         # half panels the LDS-DMA runs ahead of the MFMAs
# k per K-tile of qt_gemm_i8_ring_w4 = the weight group (QT_I8_RING_W4_K_UNIT): K a multiple
I8_RING_W4_K_UNIT = I8_FORMS["qt_gemm_i8_ring_w4"].k_unit
I8_RING_W4_SLOTS = I8_FORMS["qt_gemm_i8_ring_w4"].slots
I8_RING_W4_LEAD = I8_FORMS["qt_gemm_i8_ring_w4"].lead
I8_MID_MAX_M = I8_FORMS["qt_gemm_i8_mid"].max_m         # rows of Xq qt_gemm_i8_mid takes (QT_I8_MID_MAX_M)
I8_MID_K_UNIT = I8_FORMS["qt_gemm_i8_mid"].k_unit       # columns per k-block of qt_gemm_i8_mid: K must be a multiple
I8_RING_GROUPED_MAX_E = I8_FORMS["qt_gemm_i8_ring_grouped"].max_e   # experts qt_gemm_i8_ring_grouped walks per workgroup
MOE_I8_WIDE_K_UNIT = I8_MOE_WIDE_FORM.k_unit            # columns per k-block of qt_moe_gemm_i8_wide: K must be a multiple
MOE_I8_WIDE_TILE_ROWS = I8_MOE_WIDE_FORM.tile_rows      # rows of one expert a workgroup of qt_moe_gemm_i8_wide holds at most
MOE_I8_WIDE_MAX_E = I8_MOE_WIDE_FORM.max_e              # experts qt_moe_gemm_i8_wide walks per workgroup
MOE_I8_WIDE_MAX_SLOTS = 65535                           # row-tile slots: the grid's second dimension
SPLITK_I8_K_UNIT = I8_SPLITK_FORM.k_unit                # k-bytes per K-tile of qt_splitk_gemm_i8 (QT_SPLITK_I8_K_UNIT)
SPLITK_I8_MAX_SPLITS = 32                               # slabs its reduce pass adds at most (QT_SPLITK_I8_MAX_SPLITS)
SPLITK_I8_MIN_K_TILES = 4                               # K-tiles of the shortest split the rule deals (QT_SPLITK_I8_MIN_K_TILES)


def _i8_refusal(form: I8Form, Xq: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                row_idx: Optional[torch.Tensor] = None) -> Optional[str]:
    """Why ``form``'s entry point would refuse these operands, or None.  Host-only: touches no library."""
    if form.max_m is not None:
        M = Xq.shape[0] if Xq.dim() == 2 else -1
        if not form.min_m <= M <= form.max_m:
            return f"{form.min_m} <= M <= {form.max_m} rows only, got Xq {tuple(Xq.shape)}"
    U = form.k_unit
    if U is None:
        return None
    tiled = "gemm_i8_grouped" if form.experts else "gemm_i8"
    if Wq.dtype not in form.dtypes:
        if form.dtypes == (torch.int8,):
            return f"int8 weights only, got {Wq.dtype} (packed int4 runs on {tiled})"
        if form.dtypes == (torch.int32,):
            ring = "gemm_i8_ring_grouped" if form.experts else "gemm_i8_ring"
            return f"packed int4 (int32) weights only, got {Wq.dtype} (int8 weights run on {ring})"
        return f"int8 or packed int4 (int32) weights only, got {Wq.dtype}"
    x_rows, K = Xq.shape[0], Xq.shape[-1]
    if K % U != 0:
        return f"K={K} is not a multiple of the k-unit {U}"
    if K > 32768:
        return f"K={K} > 32768: the int32 accumulator could overflow"
    G = s_w.shape[-1] if s_w.dim() == (3 if form.experts else 2) else -1
    if form.groups == "one" and G != 1:
        return f"one scale group per row only, got s_w {tuple(s_w.shape)} (grouped scales run on {tiled})"
    if form.groups == "per_unit" and G != K // U:
        return (f"one scale per group of {U} columns only, G = K / {U} = {K // U}, got s_w {tuple(s_w.shape)} "
                f"(channel-wise scales run on {tiled})")
    if form.groups == "one_or_per_unit" and G not in (1, K // U):
        return f"G must be 1 or K / {U} = {K // U}, got s_w {tuple(s_w.shape)}"
    if form.aligned16 and (Xq.data_ptr() % 16 != 0 or Wq.data_ptr() % 16 != 0):
        return "Xq and Wq must be 16-byte aligned"
    if form.experts:
        if row_idx is not None and x_rows * K > 2 ** 32:
            return f"Xq has {x_rows} rows x K={K} > 2^32 bytes: a gathered row is addressed by a 32-bit offset"
        E, N = Wq.shape[0], Wq.shape[-2]
        if E > form.max_e:
            return f"E={E} > {form.max_e} experts"
        R = x_rows if row_idx is None else row_idx.numel()
        if form.tile_rows is not None:
            # up to R = 64 the entry point holds 32 or 64 rows per slot, at most 65 slots in all: the bound only bites
            # where a slot holds tile_rows
            slots = R // form.tile_rows + min(E, R)
            if slots > MOE_I8_WIDE_MAX_SLOTS:
                return f"{slots} row-tile slots (R={R}, E={E}) exceed the grid's {MOE_I8_WIDE_MAX_SLOTS}"
        elif ((R + 255) // 256 + E) * ((N + 255) // 256) > 0x7fffffff:
            return f"too many tiles: R={R}, E={E}, N={N}"
    return None


def _gemm_i8_dense(form: I8Form, Xq, s_x, Wq, s_w, K, zp_x, wsum, bias, out_dtype) -> torch.Tensor:
    """The refusal, the operand checks and the call the dense int8 GEMMs share; ``form`` is the entry point's row of
    ``I8_FORMS``."""
    why = _i8_refusal(form, Xq, Wq, s_w)
    if why is not None:
        raise ValueError(f"{form.entry[3:]}: {why}")
    lib = load()
    fmt, N, K, G = _i8_operands(Xq, s_x, Wq, s_w, K, zp_x, wsum, out_dtype)
    M = Xq.shape[0]
    if bias is not None:
        _req(bias, out_dtype, "bias", 1)
        if bias.numel() != N or not bias.is_contiguous():
            raise ValueError(f"bias must be contiguous [{N}] in the output dtype")
    Y = torch.empty((M, N), dtype=out_dtype, device=Xq.device)
    check(form.entry, getattr(lib, form.entry)(
        Xq.data_ptr(), M, K, Wq.data_ptr(), fmt, N, s_x.data_ptr(), _ptr(zp_x), s_w.data_ptr(), G, _ptr(wsum),
        _ptr(bias), Y.data_ptr(), _dtype_code(Y), Y.stride(0), _stream()))
    return Y


def gemm_i8(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, *, K: Optional[int] = None,
            zp_x: Optional[torch.Tensor] = None, wsum: Optional[torch.Tensor] = None,
            bias: Optional[torch.Tensor] = None, out_dtype=torch.bfloat16) -> torch.Tensor:
    """Y [M, N] = s_x[m] * sum_g s_w[n, g] * (acc_g - zp_x[m] * wsum[n, g]) (+ bias): the fixed sequence of
    ``qt_gemm_i8`` (include/quantool_amd.h).  Wq int8 [N, K], or packed int4 int32 [N, ceil(K/8)] (then ``K`` is
    required); s_w fp32 [N, G], G = 1 or ceil(K/128); zp_x int32 [M] needs wsum int32 [N, G]."""
    return _gemm_i8_dense(I8_FORMS["qt_gemm_i8"], Xq, s_x, Wq, s_w, K, zp_x, wsum, bias, out_dtype)


def gemm_i8_skinny(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, *,
                   K: Optional[int] = None, zp_x: Optional[torch.Tensor] = None,
                   wsum: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                   out_dtype=torch.bfloat16) -> torch.Tensor:
    """``gemm_i8`` for 1 <= M <= 16 rows (``qt_gemm_i8_skinny``): the decode GEMV.  Same arguments; Y equals
    ``gemm_i8``'s to the bit."""
    return _gemm_i8_dense(I8_FORMS["qt_gemm_i8_skinny"], Xq, s_x, Wq, s_w, K, zp_x, wsum, bias, out_dtype)


def gemm_i8_ring_supported(Xq: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor) -> bool:
    """Whether ``gemm_i8_ring`` takes these operands: an int8 weight with one scale group, K a multiple of
    ``I8_RING_K_UNIT`` and at most 32768, both operands 16-byte aligned.  Host-only."""
    return _i8_refusal(I8_FORMS["qt_gemm_i8_ring"], Xq, Wq, s_w) is None


def gemm_i8_ring(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, *,
                 K: Optional[int] = None, zp_x: Optional[torch.Tensor] = None,
                 wsum: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                 out_dtype=torch.bfloat16) -> torch.Tensor:
    """``gemm_i8`` on the 256 x 256 LDS-ring kernel (``qt_gemm_i8_ring``): the prefill form for W8A8 / INT8.  Same
    arguments; Y equals ``gemm_i8``'s to the bit.  ``ValueError`` where ``gemm_i8_ring_supported`` is false."""
    return _gemm_i8_dense(I8_FORMS["qt_gemm_i8_ring"], Xq, s_x, Wq, s_w, K, zp_x, wsum, bias, out_dtype)


def gemm_i8_ring_w4_supported(Xq: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor) -> bool:
    """Whether ``gemm_i8_ring_w4`` takes these operands: a packed int4 weight with one scale per 128 columns, K a
    multiple of ``I8_RING_W4_K_UNIT`` and at most 32768, both operands 16-byte aligned.  Host-only."""
    return _i8_refusal(I8_FORMS["qt_gemm_i8_ring_w4"], Xq, Wq, s_w) is None


def gemm_i8_ring_w4(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, *,
                    K: Optional[int] = None, zp_x: Optional[torch.Tensor] = None,
                    wsum: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                    out_dtype=torch.bfloat16) -> torch.Tensor:
    """``gemm_i8`` on the 256 x 256 LDS-ring kernel for packed int4 weights (``qt_gemm_i8_ring_w4``): the prefill form
    for W4A8.  Same arguments; Y equals ``gemm_i8``'s to the bit.  ``ValueError`` where ``gemm_i8_ring_w4_supported``
    is false."""
    return _gemm_i8_dense(I8_FORMS["qt_gemm_i8_ring_w4"], Xq, s_x, Wq, s_w, K, zp_x, wsum, bias, out_dtype)


def gemm_i8_mid_supported(Xq: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor) -> bool:
    """Whether ``gemm_i8_mid`` takes these operands: 1 to ``I8_MID_MAX_M`` rows, K a multiple of ``I8_MID_K_UNIT`` and at
    most 32768, G = 1 or K/128, both operands 16-byte aligned.  Host-only."""
    return _i8_refusal(I8_FORMS["qt_gemm_i8_mid"], Xq, Wq, s_w) is None


def gemm_i8_mid(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, *,
                K: Optional[int] = None, zp_x: Optional[torch.Tensor] = None,
                wsum: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                out_dtype=torch.bfloat16) -> torch.Tensor:
    """``gemm_i8`` for 1 <= M <= 128 rows on the weight-streaming 16-column tile (``qt_gemm_i8_mid``): batched decode,
    speculative verification, short prompts.  Same arguments; Y equals ``gemm_i8``'s to the bit.  ``ValueError`` where
    ``gemm_i8_mid_supported`` is false."""
    return _gemm_i8_dense(I8_FORMS["qt_gemm_i8_mid"], Xq, s_x, Wq, s_w, K, zp_x, wsum, bias, out_dtype)


def splitk_gemm_i8_supported(Xq: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor) -> bool:
    """Whether ``splitk_gemm_i8`` takes these operands: what ``gemm_i8_ring`` takes -- an int8 weight with one scale
    group, K a multiple of ``SPLITK_I8_K_UNIT`` and at most 32768, both operands 16-byte aligned.  Host-only."""
    return _i8_refusal(I8_SPLITK_FORM, Xq, Wq, s_w) is None


def splitk_gemm_i8_plan(M: int, N: int, K: int, cus: Optional[int] = None, splits: int = 0):
    """(S, workspace bytes) of ``qt_splitk_gemm_i8_plan``: with ``splits`` = 0 the rule
    S = clamp(cus / (ceil(M/256) ceil(N/256)), 1, min(max(K/128 / SPLITK_I8_MIN_K_TILES, 1), SPLITK_I8_MAX_SPLITS)),
    else that S (up to min(K/128, SPLITK_I8_MAX_SPLITS)) or ``ValueError``; the
    size is S * Mp * Np * 4.  ``cus`` None: the current device's compute units.  The rule itself needs no device."""
    if cus is None:
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    S, size = ctypes.c_int(0), ctypes.c_size_t(0)
    try:
        check("qt_splitk_gemm_i8_plan", load().qt_splitk_gemm_i8_plan(
            M, N, K, cus, splits, ctypes.addressof(S), ctypes.addressof(size)))
    except HipBackendError as e:
        if e.status == _lib.QT_ERR_INVALID:
            raise ValueError(str(e)) from None
        raise
    return S.value, size.value


def splitk_ranges(K: int, splits: int):
    """The K-tile ranges [(t0, t1), ...] ``qt_splitk_gemm_i8_range`` deals to ``splits`` splits of a reduction of K."""
    lib, out = load(), []
    t0, t1 = ctypes.c_int(0), ctypes.c_int(0)
    for s in range(splits):
        check("qt_splitk_gemm_i8_range", lib.qt_splitk_gemm_i8_range(
            K // SPLITK_I8_K_UNIT, splits, s, ctypes.addressof(t0), ctypes.addressof(t1)))
        out.append((t0.value, t1.value))
    return out


def splitk_gemm_i8(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, *,
                   K: Optional[int] = None, zp_x: Optional[torch.Tensor] = None,
                   wsum: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                   out_dtype=torch.bfloat16, splits: int = 0) -> torch.Tensor:
    """``gemm_i8`` on the ring tile over S k-ranges plus an int32 reduce pass (``qt_splitk_gemm_i8``): the short-prompt
    form for W8A8 / INT8, a few tiles of rows over a long reduction.  Same arguments; Y equals ``gemm_i8``'s to the bit.
    ``splits`` = 0 takes S from ``splitk_gemm_i8_plan``; where that gives S = 1 the call is ``gemm_i8_ring`` (the same
    tile, no slab).  ``ValueError`` where ``splitk_gemm_i8_supported`` is false or ``splits`` exceeds K / 128."""
    form = I8_SPLITK_FORM
    why = _i8_refusal(form, Xq, Wq, s_w)
    if why is not None:
        raise ValueError(f"{form.entry[3:]}: {why}")
    lib = load()
    fmt, N, K, G = _i8_operands(Xq, s_x, Wq, s_w, K, zp_x, wsum, out_dtype)
    M = Xq.shape[0]
    S, size = splitk_gemm_i8_plan(M, N, K, splits=splits)
    if S == 1:
        return gemm_i8_ring(Xq, s_x, Wq, s_w, K=K, zp_x=zp_x, wsum=wsum, bias=bias, out_dtype=out_dtype)
    if bias is not None:
        _req(bias, out_dtype, "bias", 1)
        if bias.numel() != N or not bias.is_contiguous():
            raise ValueError(f"bias must be contiguous [{N}] in the output dtype")
    ws = workspace(size, Xq.device, tag="splitk_gemm_i8")
    Y = torch.empty((M, N), dtype=out_dtype, device=Xq.device)
    check(form.entry, lib.qt_splitk_gemm_i8(
        Xq.data_ptr(), M, K, Wq.data_ptr(), fmt, N, s_x.data_ptr(), _ptr(zp_x), s_w.data_ptr(), G, _ptr(wsum),
        _ptr(bias), Y.data_ptr(), _dtype_code(Y), Y.stride(0), S, ws.data_ptr(), size, _stream()))
    return Y


def moe_route(top_k_index: torch.Tensor, num_experts: int):
    """top_k_index [T, k] int32 / int64 -> (offsets int32 [E+1], src_token int32 [T k], src_slot int32 [T k],
    row_of int32 [T k]): ``qt_moe_route`` (include/quantool_amd.h).  Rows sorted by expert, then by token; an index
    outside [0, E) is dropped (row_of -1).  All on the device, no host read."""
    lib = load()
    if not top_k_index.is_cuda or top_k_index.dtype not in (torch.int32, torch.int64) or top_k_index.dim() != 2:
        raise ValueError("top_k_index must be a 2-d int32 / int64 device tensor [T, k]")
    top_k_index = top_k_index.contiguous()
    T, k = top_k_index.shape
    E = int(num_experts)
    if T == 0 or k == 0 or not 0 < E <= 256:
        raise ValueError(f"moe_route: T={T}, k={k}, E={E} (need T, k > 0 and 0 < E <= 256)")
    dev = top_k_index.device
    offsets = torch.empty(E + 1, dtype=torch.int32, device=dev)
    src_token = torch.empty(T * k, dtype=torch.int32, device=dev)
    src_slot = torch.empty(T * k, dtype=torch.int32, device=dev)
    row_of = torch.empty(T * k, dtype=torch.int32, device=dev)
    check("qt_moe_route", lib.qt_moe_route(
        top_k_index.data_ptr(), int(top_k_index.dtype == torch.int64), T, k, E, offsets.data_ptr(),
        src_token.data_ptr(), src_slot.data_ptr(), row_of.data_ptr(), _stream()))
    return offsets, src_token, src_slot, row_of


def _gemm_i8_grouped(form: I8Form, Xq, s_x, Wq, s_w, offsets, rows, row_idx, K, zp_x, wsum, out_dtype) -> torch.Tensor:
    """The refusal, the operand checks and the call the grouped int8 GEMMs share; ``form`` is the entry point's row of
    ``I8_FORMS``."""
    why = _i8_refusal(form, Xq, Wq, s_w, row_idx)
    if why is not None:
        raise ValueError(f"{form.entry[3:]}: {why}")
    lib = load()
    fmt, N, K, G = _i8_operands(Xq, s_x, Wq, s_w, K, zp_x, wsum, out_dtype, experts=True)
    Mx, E = Xq.shape[0], Wq.shape[0]
    _req(offsets, torch.int32, "offsets", 1)
    if offsets.numel() != E + 1 or not offsets.is_contiguous():
        raise ValueError(f"offsets must be contiguous int32 [E + 1 = {E + 1}]")
    if row_idx is not None:
        _req(row_idx, torch.int32, "row_idx", 1)
        if not row_idx.is_contiguous():
            raise ValueError("row_idx must be contiguous int32 [R]")
        R = row_idx.numel() if rows is None else int(rows)
        if R > row_idx.numel():
            raise ValueError(f"rows={R} but row_idx has {row_idx.numel()} entries")
    else:
        R = Mx if rows is None else int(rows)
        if R > Mx:
            raise ValueError(f"rows={R} but Xq has {Mx} rows (contiguous A)")
    if R <= 0:
        raise ValueError(f"rows must be positive, got {R}")
    Y = torch.empty((R, N), dtype=out_dtype, device=Xq.device)
    check(form.entry, getattr(lib, form.entry)(
        Xq.data_ptr(), K, _ptr(row_idx), R, offsets.data_ptr(), E, Wq.data_ptr(), fmt, N, s_x.data_ptr(), _ptr(zp_x),
        s_w.data_ptr(), G, _ptr(wsum), Y.data_ptr(), _dtype_code(Y), Y.stride(0), *((Mx,) if form.x_rows else ()),
        _stream()))
    return Y


def gemm_i8_grouped(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, offsets: torch.Tensor,
                    *, rows: Optional[int] = None, row_idx: Optional[torch.Tensor] = None, K: Optional[int] = None,
                    zp_x: Optional[torch.Tensor] = None, wsum: Optional[torch.Tensor] = None,
                    out_dtype=torch.bfloat16) -> torch.Tensor:
    """``qt_gemm_i8`` over E weight matrices: Y [R, N], expert e owning rows [offsets[e], offsets[e+1]) (include/
    quantool_amd.h qt_gemm_i8_grouped).  Wq int8 [E, N, K] or packed int4 int32 [E, N, ceil(K/8)] (then ``K`` is
    required); s_w fp32 [E, N, G]; wsum int32 [E, N, G] (needed with zp_x).  A rows: Xq[row_idx[m]] when ``row_idx``
    (int32 [R], e.g. ``moe_route``'s src_token) is given, with s_x / zp_x read at the same index; else Xq[m] (then R
    defaults to Xq's rows).  Rows past offsets[E] are left unwritten."""
    return _gemm_i8_grouped(I8_FORMS["qt_gemm_i8_grouped"], Xq, s_x, Wq, s_w, offsets, rows, row_idx, K, zp_x, wsum, out_dtype)


def gemm_i8_skinny_grouped(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                           offsets: torch.Tensor, *, rows: Optional[int] = None,
                           row_idx: Optional[torch.Tensor] = None, K: Optional[int] = None,
                           zp_x: Optional[torch.Tensor] = None, wsum: Optional[torch.Tensor] = None,
                           out_dtype=torch.bfloat16) -> torch.Tensor:
    """``gemm_i8_grouped`` on the decode tile (``qt_gemm_i8_skinny_grouped``): every expert's rows in tiles of 16, only
    the experts that own rows read, each once per tile.  Same arguments; Y equals ``gemm_i8_grouped``'s to the bit.
    R // 16 + min(E, R) row-tile slots must fit a grid dimension (65535)."""
    return _gemm_i8_grouped(I8_FORMS["qt_gemm_i8_skinny_grouped"], Xq, s_x, Wq, s_w, offsets, rows, row_idx, K, zp_x, wsum,
                            out_dtype)


def gemm_i8_ring_grouped_supported(Xq: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                                   row_idx: Optional[torch.Tensor] = None) -> bool:
    """Whether ``gemm_i8_ring_grouped`` takes these operands: an int8 bank [E, N, K] with one scale group, K a multiple
    of ``I8_RING_K_UNIT`` and at most 32768, both operands 16-byte aligned, at most 4096 experts, a grid that fits,
    and, with ``row_idx``, an Xq of at most 2^32 bytes.  Host-only."""
    return _i8_refusal(I8_FORMS["qt_gemm_i8_ring_grouped"], Xq, Wq, s_w, row_idx) is None


def gemm_i8_ring_grouped(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                         offsets: torch.Tensor, *, rows: Optional[int] = None,
                         row_idx: Optional[torch.Tensor] = None, K: Optional[int] = None,
                         zp_x: Optional[torch.Tensor] = None, wsum: Optional[torch.Tensor] = None,
                         out_dtype=torch.bfloat16) -> torch.Tensor:
    """``gemm_i8_grouped`` on the 256 x 256 LDS-ring tile (``qt_gemm_i8_ring_grouped``): the prefill form for W8A8 /
    INT8 banks.  Same arguments; Y equals ``gemm_i8_grouped``'s to the bit; ``row_idx`` values are clamped into Xq's
    rows.  ``ValueError`` where ``gemm_i8_ring_grouped_supported`` is false."""
    return _gemm_i8_grouped(I8_FORMS["qt_gemm_i8_ring_grouped"], Xq, s_x, Wq, s_w, offsets, rows, row_idx, K, zp_x,
                            wsum, out_dtype)


def moe_gemm_i8_ring_w4_supported(Xq: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                                  row_idx: Optional[torch.Tensor] = None) -> bool:
    """Whether ``moe_gemm_i8_ring_w4`` takes these operands: a packed int4 bank [E, N, K/8] with one scale per 128
    columns, K a multiple of ``I8_RING_W4_K_UNIT`` and at most 32768, both operands 16-byte aligned, at most 4096
    experts, a grid that fits, and, with ``row_idx``, an Xq of at most 2^32 bytes.  Host-only."""
    return _i8_refusal(I8_MOE_RING_W4_FORM, Xq, Wq, s_w, row_idx) is None


def moe_gemm_i8_ring_w4(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                        offsets: torch.Tensor, *, rows: Optional[int] = None,
                        row_idx: Optional[torch.Tensor] = None, K: Optional[int] = None,
                        zp_x: Optional[torch.Tensor] = None, wsum: Optional[torch.Tensor] = None,
                        out_dtype=torch.bfloat16) -> torch.Tensor:
    """``gemm_i8_grouped`` on the 256 x 256 LDS-ring tile for packed int4 banks (``qt_moe_gemm_i8_ring_w4``): the
    prefill form for W4A8 banks.  Same arguments; Y equals ``gemm_i8_grouped``'s to the bit; ``row_idx`` values are
    clamped into Xq's rows.  ``ValueError`` where ``moe_gemm_i8_ring_w4_supported`` is false."""
    return _gemm_i8_grouped(I8_MOE_RING_W4_FORM, Xq, s_x, Wq, s_w, offsets, rows, row_idx, K, zp_x, wsum, out_dtype)


def moe_gemm_i8_wide_supported(Xq: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                               row_idx: Optional[torch.Tensor] = None) -> bool:
    """Whether ``moe_gemm_i8_wide`` takes these operands: an int8 or packed int4 bank with G = 1 or K/128, K a multiple
    of ``MOE_I8_WIDE_K_UNIT`` and at most 32768, both operands 16-byte aligned, at most ``MOE_I8_WIDE_MAX_E`` experts,
    R // ``MOE_I8_WIDE_TILE_ROWS`` + min(E, R) <= ``MOE_I8_WIDE_MAX_SLOTS`` row-tile slots, and, with ``row_idx``, an Xq
    of at most 2^32 bytes.  Host-only."""
    return _i8_refusal(I8_MOE_WIDE_FORM, Xq, Wq, s_w, row_idx) is None


def moe_gemm_i8_wide(Xq: torch.Tensor, s_x: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                     offsets: torch.Tensor, *, rows: Optional[int] = None,
                     row_idx: Optional[torch.Tensor] = None, K: Optional[int] = None,
                     zp_x: Optional[torch.Tensor] = None, wsum: Optional[torch.Tensor] = None,
                     out_dtype=torch.bfloat16) -> torch.Tensor:
    """``gemm_i8_grouped`` on the weight-streaming 16-column tile (``qt_moe_gemm_i8_wide``): the bank form between the
    decode range and the rings -- batched decode, speculative verification, short prompts.  Same arguments; Y equals
    ``gemm_i8_grouped``'s to the bit; ``row_idx`` values are clamped into Xq's rows.  ``ValueError`` where
    ``moe_gemm_i8_wide_supported`` is false."""
    return _gemm_i8_grouped(I8_MOE_WIDE_FORM, Xq, s_x, Wq, s_w, offsets, rows, row_idx, K, zp_x, wsum, out_dtype)


def moe_combine(Y: torch.Tensor, row_of: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
    """out [T, H] = each token's routed rows of Y [R, H] weighted by top_k_weights [T, k] and summed in ascending
    expert order, rounding to Y's dtype after every product and sum (``qt_moe_combine``)."""
    lib = load()
    code = _x2d(Y, "Y")
    _req(row_of, torch.int32, "row_of", 1)
    if not top_k_weights.is_cuda or top_k_weights.dim() != 2 or not top_k_weights.is_floating_point():
        raise ValueError("top_k_weights must be a 2-d floating device tensor [T, k]")
    T, k = top_k_weights.shape
    if row_of.numel() != T * k or not row_of.is_contiguous():
        raise ValueError(f"row_of must be contiguous int32 [{T * k}]")
    if T == 0 or not 0 < k <= 16:
        raise ValueError(f"moe_combine: T={T}, k={k} (need T > 0 and 0 < k <= 16)")
    w = top_k_weights.to(torch.float32).contiguous()      # bf16 / fp16 widen exactly
    H = Y.shape[1]
    out = torch.empty((T, H), dtype=Y.dtype, device=Y.device)
    check("qt_moe_combine", lib.qt_moe_combine(
        Y.data_ptr(), code, H, Y.stride(0), row_of.data_ptr(), w.data_ptr(), T, k, out.data_ptr(), _stream()))
    return out


# ---- A16 runtime: W4A16 / W8A16 weights dequantised on chip -------------------------------------------------------
def _wq_weight(Wq: torch.Tensor, s_w: torch.Tensor, zp_w: Optional[torch.Tensor], g_idx: Optional[torch.Tensor],
               K: Optional[int], experts: bool = False):
    """Checks one weight description of ``qt_dequantize_weight`` / ``qt_gemm_wq_skinny`` -- or, with ``experts``, E of
    them stacked along a leading dimension (``qt_gemm_wq_grouped``); returns (format, N, K, G)."""
    nd = 3 if experts else 2
    if not Wq.is_cuda or Wq.dim() != nd or not Wq.is_contiguous():
        raise ValueError(f"Wq must be a contiguous {nd}-d device tensor")
    L = [int(Wq.shape[0])] if experts else []
    E = "E, " if experts else ""
    N = Wq.shape[-2]
    if Wq.dtype == torch.int8:
        fmt = _lib.QT_W_INT8
        if K is not None and K != Wq.shape[-1]:
            raise ValueError(f"int8 Wq must be [{E}N, K = {K}], got {tuple(Wq.shape)}")
        K = Wq.shape[-1]
    elif Wq.dtype == torch.int32:
        fmt = _lib.QT_W_INT4_PACKED
        if K is None:
            raise ValueError("packed int4 Wq needs K")
        if Wq.shape[-1] != (K + 7) // 8:
            raise ValueError(f"packed int4 Wq must be [{E}N, ceil(K/8) = {(K + 7) // 8}], got {tuple(Wq.shape)}")
    else:
        raise TypeError(f"Wq must be int8 [{E}N, K] or packed int4 int32 [{E}N, ceil(K/8)], got {Wq.dtype}")
    K = int(K)
    if N == 0 or K <= 0 or 0 in L:
        raise ValueError(f"empty weight: {tuple(Wq.shape)}, K={K}")
    _req(s_w, torch.float32, "s_w", 2 + len(L))
    G = s_w.shape[-1]
    if list(s_w.shape[:-1]) != L + [N] or G not in (1, (K + 127) // 128) or not s_w.is_contiguous():
        raise ValueError(f"s_w must be contiguous fp32 [{E}{N}, 1 or {(K + 127) // 128}], got {tuple(s_w.shape)}")
    if zp_w is not None:
        _req(zp_w, torch.int8, "zp_w", 2 + len(L))
        if list(zp_w.shape) != L + [N, G] or not zp_w.is_contiguous():
            raise ValueError(f"zp_w must be contiguous int8 [{E}{N}, {G}], got {tuple(zp_w.shape)}")
    if g_idx is not None:
        _req(g_idx, torch.int32, "g_idx", 1 + len(L))
        if list(g_idx.shape) != L + [K] or not g_idx.is_contiguous():
            raise ValueError(f"g_idx must be contiguous int32 [{E}{K}]")
    for t, name in ((s_w, "s_w"), (zp_w, "zp_w"), (g_idx, "g_idx")):
        if t is not None and t.device != Wq.device:
            raise ValueError(f"{name} is on {t.device}, Wq on {Wq.device}")
    return fmt, N, K, G


def dequantize_weight(Wq: torch.Tensor, s_w: torch.Tensor, *, K: Optional[int] = None,
                      zp_w: Optional[torch.Tensor] = None, g_idx: Optional[torch.Tensor] = None,
                      dtype=torch.bfloat16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W [N, K] = round_to_dtype((q - zp) * s_w) per column group (``qt_dequantize_weight``, include/quantool_amd.h):
    bit-identical to ``engine.qlinear.dequantized_weight``.  Wq int8 [N, K] or packed int4 int32 [N, ceil(K/8)] (then
    ``K`` is required); s_w fp32 [N, G]; zp_w int8 [N, G]; g_idx int32 [K].  ``out`` (optional) receives W: [N, K] with
    unit column stride, any row pitch."""
    lib = load()
    fmt, N, K, G = _wq_weight(Wq, s_w, zp_w, g_idx, K)
    if dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"dtype must be bf16 or fp16, got {dtype}")
    if out is None:
        out = torch.empty((N, K), dtype=dtype, device=Wq.device)
    elif (out.dtype != dtype or tuple(out.shape) != (N, K) or out.stride(1) != 1 or out.device != Wq.device):
        raise ValueError(f"out must be a {dtype} [{N}, {K}] tensor on {Wq.device} with unit column stride")
    check("qt_dequantize_weight", lib.qt_dequantize_weight(
        Wq.data_ptr(), fmt, N, K, s_w.data_ptr(), G, _ptr(zp_w), _ptr(g_idx), out.data_ptr(), _dtype_code(out),
        out.stride(0), _stream()))
    return out


SKINNY_MAX_M = 16   # rows of X qt_gemm_wq_skinny takes


def gemm_wq_skinny(X: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, *, zp_w: Optional[torch.Tensor] = None,
                   g_idx: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y [M, N] = X [M, K] . w^T (+ bias) with w the dequantised weight, fp32 accumulation, one rounding to X's dtype
    (``qt_gemm_wq_skinny``): the decode GEMV, 1 <= M <= 16.  X bf16 / fp16 with unit column stride (any row pitch);
    weight arguments as ``dequantize_weight``; bias [N] in X's dtype."""
    lib = load()
    code = _x2d(X, "X")
    M, K = X.shape
    if not 1 <= M <= SKINNY_MAX_M:
        raise ValueError(f"gemm_wq_skinny takes 1 <= M <= {SKINNY_MAX_M} rows, got {M}")
    fmt, N, K, G = _wq_weight(Wq, s_w, zp_w, g_idx, K)
    if Wq.device != X.device:
        raise ValueError(f"Wq is on {Wq.device}, X on {X.device}")
    if bias is not None:
        _req(bias, X.dtype, "bias", 1)
        if bias.numel() != N or not bias.is_contiguous():
            raise ValueError(f"bias must be contiguous [{N}] in X's dtype")
    Y = torch.empty((M, N), dtype=X.dtype, device=X.device)
    check("qt_gemm_wq_skinny", lib.qt_gemm_wq_skinny(
        X.data_ptr(), code, M, K, X.stride(0), Wq.data_ptr(), fmt, N, s_w.data_ptr(), G, _ptr(zp_w), _ptr(g_idx),
        _ptr(bias), Y.data_ptr(), Y.stride(0), _stream()))
    return Y


WQ_STREAM_MAX_M = 128    # rows of X qt_gemm_wq_stream takes (QT_WQ_STREAM_MAX_M)
WQ_STREAM_K_UNIT = 128   # columns per k-block of qt_gemm_wq_stream: K must be a multiple (QT_WQ_STREAM_K_UNIT)
WQ_STREAM_MAX_LDX = 1 << 25   # largest row pitch of X in elements (QT_WQ_STREAM_MAX_LDX)


def _wq_stream_refusal(X: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, zp_w: Optional[torch.Tensor] = None,
                       g_idx: Optional[torch.Tensor] = None) -> Optional[str]:
    """Why ``qt_gemm_wq_stream`` would refuse these operands whatever the number of rows, or None.  Host-only: touches
    no library, and reads shapes, dtypes, strides and addresses alone, so CPU tensors are judged like device ones."""
    U = WQ_STREAM_K_UNIT
    if g_idx is not None:
        return "g_idx is not taken (actorder group runs on qt_dequantize_weight + a dense GEMM)"
    if X.dtype not in (torch.bfloat16, torch.float16):
        return f"X must be bf16 or fp16, got {X.dtype}"
    if X.dim() != 2 or X.stride(1) != 1:
        return f"X must be 2-d with unit column stride, got shape {tuple(X.shape)} strides {X.stride()}"
    if Wq.dtype not in (torch.int8, torch.int32):
        return f"int8 or packed int4 (int32) weights only, got {Wq.dtype}"
    K = X.shape[1]
    if K == 0 or K % U != 0:
        return f"K={K} is not a multiple of the k-unit {U}"
    G = s_w.shape[-1] if s_w.dim() == 2 else -1
    if G not in (1, K // U):
        return f"G must be 1 or K / {U} = {K // U}, got s_w {tuple(s_w.shape)}"
    if X.data_ptr() % 16 != 0 or Wq.data_ptr() % 16 != 0 or (X.stride(0) * 2) % 16 != 0:
        return "X, Wq and the row pitch of X must be 16-byte aligned"
    if X.stride(0) > WQ_STREAM_MAX_LDX:
        return f"the row pitch of X, {X.stride(0)} elements, is above {WQ_STREAM_MAX_LDX}"
    return None


def gemm_wq_stream_supported(X: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                             zp_w: Optional[torch.Tensor] = None, g_idx: Optional[torch.Tensor] = None) -> bool:
    """Whether ``gemm_wq_stream`` takes these operands at 1 to ``WQ_STREAM_MAX_M`` rows: no ``g_idx``, 16-bit X with unit
    column stride, K a multiple of ``WQ_STREAM_K_UNIT``, G = 1 or K/128, X, Wq and X's row pitch 16-byte aligned.
    Host-only."""
    return _wq_stream_refusal(X, Wq, s_w, zp_w, g_idx) is None


def gemm_wq_stream(X: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, *, zp_w: Optional[torch.Tensor] = None,
                   g_idx: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gemm_wq_skinny`` for 1 <= M <= ``WQ_STREAM_MAX_M`` rows (``qt_gemm_wq_stream``): batched decode, speculative
    verification, short prompts.  Same arguments; every row of Y equals ``gemm_wq_skinny`` of that row to the bit.
    ``ValueError`` where ``gemm_wq_stream_supported`` is false or M is out of range, before the library is touched."""
    M = X.shape[0] if X.dim() == 2 else -1
    why = _wq_stream_refusal(X, Wq, s_w, zp_w, g_idx)
    if why is None and not 1 <= M <= WQ_STREAM_MAX_M:
        why = f"1 <= M <= {WQ_STREAM_MAX_M} rows only, got X {tuple(X.shape)}"
    if why is not None:
        raise ValueError(f"gemm_wq_stream: {why}")
    lib = load()
    code = _x2d(X, "X")
    M, K = X.shape
    fmt, N, K, G = _wq_weight(Wq, s_w, zp_w, g_idx, K)
    if Wq.device != X.device:
        raise ValueError(f"Wq is on {Wq.device}, X on {X.device}")
    if bias is not None:
        _req(bias, X.dtype, "bias", 1)
        if bias.numel() != N or not bias.is_contiguous():
            raise ValueError(f"bias must be contiguous [{N}] in X's dtype")
    Y = torch.empty((M, N), dtype=X.dtype, device=X.device)
    check("qt_gemm_wq_stream", lib.qt_gemm_wq_stream(
        X.data_ptr(), code, M, K, X.stride(0), Wq.data_ptr(), fmt, N, s_w.data_ptr(), G, _ptr(zp_w), _ptr(g_idx),
        _ptr(bias), Y.data_ptr(), Y.stride(0), _stream()))
    return Y


def gemm_wq_grouped(X: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, offsets: torch.Tensor, *,
                    row_idx: Optional[torch.Tensor] = None, K: Optional[int] = None,
                    zp_w: Optional[torch.Tensor] = None, g_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``qt_gemm_wq_skinny`` over E weight matrices: Y [R, N] in X's dtype, expert e owning rows
    [offsets[e], offsets[e+1]) (include/quantool_amd.h qt_gemm_wq_grouped).  Wq int8 [E, N, K] or packed int4 int32
    [E, N, ceil(K/8)] (then ``K`` is required); s_w fp32 [E, N, G]; zp_w int8 [E, N, G]; g_idx int32 [E, K].  X rows:
    X[row_idx[m]] when ``row_idx`` (int32 [R], e.g. ``moe_route``'s src_token) is given, else X[m] with R = X's rows.
    Every row equals ``gemm_wq_skinny`` of that expert on that row, to the bit; rows past offsets[E] are left
    unwritten."""
    lib = load()
    code = _x2d(X, "X")
    Mx, Kx = X.shape
    if K is not None and K != Kx:
        raise ValueError(f"K={K} but X has {Kx} columns")
    fmt, N, K, G = _wq_weight(Wq, s_w, zp_w, g_idx, Kx, experts=True)
    E = Wq.shape[0]
    if Wq.device != X.device:
        raise ValueError(f"Wq is on {Wq.device}, X on {X.device}")
    _req(offsets, torch.int32, "offsets", 1)
    if offsets.numel() != E + 1 or not offsets.is_contiguous() or offsets.device != X.device:
        raise ValueError(f"offsets must be contiguous int32 [E + 1 = {E + 1}] on {X.device}")
    if row_idx is not None:
        _req(row_idx, torch.int32, "row_idx", 1)
        if not row_idx.is_contiguous() or row_idx.device != X.device:
            raise ValueError(f"row_idx must be contiguous int32 [R] on {X.device}")
        R = row_idx.numel()
    else:
        R = Mx
    if R == 0 or Mx == 0:
        raise ValueError(f"empty GEMV: R={R}, X rows={Mx}")
    Y = torch.empty((R, N), dtype=X.dtype, device=X.device)
    check("qt_gemm_wq_grouped", lib.qt_gemm_wq_grouped(
        X.data_ptr(), code, K, X.stride(0), _ptr(row_idx), R, offsets.data_ptr(), E, Wq.data_ptr(), fmt, N,
        s_w.data_ptr(), G, _ptr(zp_w), _ptr(g_idx), Y.data_ptr(), Y.stride(0), _stream()))
    return Y


MOE_WQ_WIDE_K_UNIT = 128        # columns per k-block of qt_moe_gemm_wq_wide: K must be a multiple (QT_MOE_WQ_WIDE_K_UNIT)
MOE_WQ_WIDE_MAX_E = 4096        # experts a workgroup of qt_moe_gemm_wq_wide walks (QT_MOE_WQ_WIDE_MAX_E)
MOE_WQ_WIDE_MAX_SLOTS = 65535   # row-tile slots of its grid (QT_MOE_WQ_WIDE_MAX_SLOTS)


def moe_wq_wide_mtiles(R: int, E: int) -> int:
    """The m-tiles of 16 rows a workgroup of ``qt_moe_gemm_wq_wide`` holds for R routed rows over E experts: the
    smallest of 1, 2, 4, 8 whose 16 MT rows hold ceil(R / E) (8 when none does), as the library chooses it."""
    per = -(-R // E)
    return 1 if per <= 16 else 2 if per <= 32 else 4 if per <= 64 else 8


def _moe_wq_wide_refusal(X: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, zp_w: Optional[torch.Tensor] = None,
                         g_idx: Optional[torch.Tensor] = None, row_idx: Optional[torch.Tensor] = None) -> Optional[str]:
    """Why ``qt_moe_gemm_wq_wide`` would refuse these operands, or None.  Host-only: touches no library, and reads
    shapes, dtypes, strides and addresses alone, so CPU tensors are judged like device ones."""
    U = MOE_WQ_WIDE_K_UNIT
    if g_idx is not None:
        return "g_idx is not taken (an actorder-group bank runs on gemm_wq_grouped or on the dequantised bank)"
    if X.dtype not in (torch.bfloat16, torch.float16):
        return f"X must be bf16 or fp16, got {X.dtype}"
    if X.dim() != 2 or X.stride(1) != 1:
        return f"X must be 2-d with unit column stride, got shape {tuple(X.shape)} strides {X.stride()}"
    if Wq.dtype not in (torch.int8, torch.int32):
        return f"int8 or packed int4 (int32) weights only, got {Wq.dtype}"
    if Wq.dim() != 3:
        return f"Wq must be a bank [E, N, .], got {tuple(Wq.shape)}"
    x_rows, K = X.shape
    if K == 0 or K % U != 0:
        return f"K={K} is not a multiple of the k-unit {U}"
    G = s_w.shape[-1] if s_w.dim() == 3 else -1
    if G not in (1, K // U):
        return f"G must be 1 or K / {U} = {K // U}, got s_w {tuple(s_w.shape)}"
    ldx = X.stride(0) if x_rows > 1 else K      # one row: its pitch is never used
    if X.data_ptr() % 16 != 0 or Wq.data_ptr() % 16 != 0 or (ldx * 2) % 16 != 0:
        return "X, Wq and the row pitch of X must be 16-byte aligned"
    E = Wq.shape[0]
    if E > MOE_WQ_WIDE_MAX_E:
        return f"E={E} experts are more than {MOE_WQ_WIDE_MAX_E}"
    R = x_rows if row_idx is None else row_idx.numel()
    if R < 1 or x_rows < 1:
        return f"empty product: R={R}, X rows={x_rows}"
    if x_rows * ldx * 2 + 2 * K >= 1 << 32:
        return (f"x_rows={x_rows} x pitch {ldx} x 2 + 2 K reaches 2^32 bytes: a row of X is addressed by a 32-bit "
                "offset")
    slots = R // (16 * moe_wq_wide_mtiles(R, E)) + min(E, R)
    if slots > MOE_WQ_WIDE_MAX_SLOTS:
        return f"{slots} row-tile slots (R={R}, E={E}) exceed the grid's {MOE_WQ_WIDE_MAX_SLOTS}"
    return None


def moe_gemm_wq_wide_supported(X: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor,
                               zp_w: Optional[torch.Tensor] = None, g_idx: Optional[torch.Tensor] = None,
                               row_idx: Optional[torch.Tensor] = None) -> bool:
    """Whether ``moe_gemm_wq_wide`` takes these operands: no ``g_idx``, 16-bit X with unit column stride, an int8 or
    packed int4 bank of at most ``MOE_WQ_WIDE_MAX_E`` experts, K a multiple of ``MOE_WQ_WIDE_K_UNIT``, G = 1 or K/128, X,
    Wq and X's row pitch 16-byte aligned, X below 2^32 bytes, at most ``MOE_WQ_WIDE_MAX_SLOTS`` row-tile slots.
    Host-only."""
    return _moe_wq_wide_refusal(X, Wq, s_w, zp_w, g_idx, row_idx) is None


def moe_gemm_wq_wide(X: torch.Tensor, Wq: torch.Tensor, s_w: torch.Tensor, offsets: torch.Tensor, *,
                     row_idx: Optional[torch.Tensor] = None, K: Optional[int] = None,
                     zp_w: Optional[torch.Tensor] = None, g_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``gemm_wq_grouped`` with several tiles of 16 rows of one expert per workgroup (``qt_moe_gemm_wq_wide``): the
    bank form for batched decode, speculative verification and short prompts.  Same arguments; every row of Y equals
    ``gemm_wq_grouped``'s to the bit, and ``row_idx`` values are clamped into X's rows.  ``ValueError`` where
    ``moe_gemm_wq_wide_supported`` is false, before the library is touched."""
    why = _moe_wq_wide_refusal(X, Wq, s_w, zp_w, g_idx, row_idx)
    if why is not None:
        raise ValueError(f"moe_gemm_wq_wide: {why}")
    lib = load()
    code = _x2d(X, "X")
    Mx, Kx = X.shape
    if K is not None and K != Kx:
        raise ValueError(f"K={K} but X has {Kx} columns")
    fmt, N, K, G = _wq_weight(Wq, s_w, zp_w, g_idx, Kx, experts=True)
    E = Wq.shape[0]
    if Wq.device != X.device:
        raise ValueError(f"Wq is on {Wq.device}, X on {X.device}")
    _req(offsets, torch.int32, "offsets", 1)
    if offsets.numel() != E + 1 or not offsets.is_contiguous() or offsets.device != X.device:
        raise ValueError(f"offsets must be contiguous int32 [E + 1 = {E + 1}] on {X.device}")
    if row_idx is not None:
        _req(row_idx, torch.int32, "row_idx", 1)
        if not row_idx.is_contiguous() or row_idx.device != X.device:
            raise ValueError(f"row_idx must be contiguous int32 [R] on {X.device}")
        R = row_idx.numel()
    else:
        R = Mx
    Y = torch.empty((R, N), dtype=X.dtype, device=X.device)
    check("qt_moe_gemm_wq_wide", lib.qt_moe_gemm_wq_wide(
        X.data_ptr(), code, K, X.stride(0) if Mx > 1 else K, _ptr(row_idx), R, offsets.data_ptr(), E, Wq.data_ptr(),
        fmt, N, s_w.data_ptr(), G, _ptr(zp_w), None, Y.data_ptr(), Y.stride(0), Mx, _stream()))
    return Y


# ---- a12  AWQ ------------------------------------------------------------------------------
def _w2d(W: torch.Tensor):
    if W.dim() != 2 or not W.is_cuda or W.stride(1) != 1:
        raise ValueError("W must be a 2-d device tensor with unit column stride")
    return W.shape


def awq_weight_mean_accumulate(W: torch.Tensor, group_size: int, w_sum: torch.Tensor) -> None:
    lib = load()
    R, K = _w2d(W)
    _req(w_sum, torch.float32, "w_sum", 1)
    assert w_sum.numel() == K and w_sum.is_contiguous()
    ws = workspace(lib.qt_awq_weight_mean_workspace_bytes(R, K), W.device, "awq_wm")
    check("qt_awq_weight_mean_accumulate", lib.qt_awq_weight_mean_accumulate(
        W.data_ptr(), _dtype_code(W), R, K, W.stride(0), group_size, w_sum.data_ptr(), ws.data_ptr(), ws.numel(),
        _stream()))


def awq_scales(x_abs_sum: torch.Tensor, n_tokens: int, w_sum: torch.Tensor, n_rows: int, n_grid: int = 20,
               duo_scaling: bool = True) -> torch.Tensor:
    lib = load()
    _req(x_abs_sum, torch.float32, "x_abs_sum", 1)
    _req(w_sum, torch.float32, "w_sum", 1)
    K = x_abs_sum.numel()
    assert w_sum.numel() == K
    out = torch.empty((n_grid, K), dtype=torch.float32, device=x_abs_sum.device)
    check("qt_awq_scales", lib.qt_awq_scales(x_abs_sum.data_ptr(), int(n_tokens), w_sum.data_ptr(), int(n_rows), K,
                                             n_grid, int(bool(duo_scaling)), out.data_ptr(), _stream()))
    return out


def symmetrize_lower(G: torch.Tensor) -> None:
    lib = load()
    _req(G, torch.float32, "G", 2)
    assert G.is_contiguous() and G.shape[0] == G.shape[1]
    check("qt_symmetrize_lower", lib.qt_symmetrize_lower(G.data_ptr(), G.shape[0], _stream()))


def awq_loss(W: torch.Tensor, s: torch.Tensor, group_size: int, symmetric: bool, num_bits: int, Gfull: torch.Tensor,
             n_tokens: int, out: torch.Tensor, *, exact: bool = False, weight: float = 1.0,
             accumulate: bool = False) -> None:
    """out[0] (device fp32) = (accumulate ? out[0] : 0) + weight * search loss for the scales s[K]."""
    lib = load()
    R, K = _w2d(W)
    _req(s, torch.float32, "s", 1)
    _req(Gfull, torch.float32, "Gfull", 2)
    _req(out, torch.float32, "out")
    assert s.numel() == K and s.is_contiguous() and Gfull.shape == (K, K) and Gfull.is_contiguous()
    ws = workspace(lib.qt_awq_loss_workspace_bytes(R, K), W.device, "awq_loss")
    check("qt_awq_loss", lib.qt_awq_loss(W.data_ptr(), _dtype_code(W), R, K, W.stride(0), s.data_ptr(), group_size,
                                         int(bool(symmetric)), num_bits, Gfull.data_ptr(), int(n_tokens),
                                         int(bool(exact)), float(weight), int(bool(accumulate)), out.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream()))


def awq_losses(W: torch.Tensor, scales: torch.Tensor, group_size: int, symmetric: bool, num_bits: int,
               Gfull: torch.Tensor, n_tokens: int, out: torch.Tensor, *, weight: float = 1.0,
               accumulate: bool = False) -> None:
    """out[g] (device fp32 [n_grid]) = (accumulate ? out[g] : 0) + weight * fast search loss for scales[g]."""
    lib = load()
    R, K = _w2d(W)
    _req(scales, torch.float32, "scales", 2)
    _req(Gfull, torch.float32, "Gfull", 2)
    _req(out, torch.float32, "out", 1)
    n_grid = scales.shape[0]
    assert scales.shape[1] == K and scales.is_contiguous() and Gfull.shape == (K, K) and Gfull.is_contiguous()
    assert out.numel() == n_grid and out.is_contiguous()
    ws = workspace(lib.qt_awq_losses_workspace_bytes(R, K, n_grid), W.device, "awq_losses")
    check("qt_awq_losses", lib.qt_awq_losses(W.data_ptr(), _dtype_code(W), R, K, W.stride(0), scales.data_ptr(), n_grid,
                                             group_size, int(bool(symmetric)), num_bits, Gfull.data_ptr(), int(n_tokens),
                                             float(weight), int(bool(accumulate)), out.data_ptr(), ws.data_ptr(),
                                             ws.numel(), _stream()))


def argmin_first(values: torch.Tensor) -> torch.Tensor:
    """Device int32[1]: index of the first minimum (ties keep the lowest index, as upstream's search loop)."""
    lib = load()
    _req(values, torch.float32, "values", 1)
    assert values.is_contiguous()
    out = torch.empty(1, dtype=torch.int32, device=values.device)
    check("qt_argmin_f32", lib.qt_argmin_f32(values.data_ptr(), values.numel(), out.data_ptr(), _stream()))
    return out


def awq_pseudo_quantize(W: torch.Tensor, s: torch.Tensor, group_size: int, symmetric: bool, num_bits: int,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pseudo_quant(W * s) / s in W's dtype (one grid point's trial weights)."""
    lib = load()
    R, K = _w2d(W)
    _req(s, torch.float32, "s", 1)
    assert s.numel() == K and s.is_contiguous()
    if out is None:
        out = torch.empty((R, K), dtype=W.dtype, device=W.device)
    assert out.shape == (R, K) and out.dtype == W.dtype and out.stride(1) == 1 and out.device == W.device
    check("qt_awq_pseudo_quantize",
          lib.qt_awq_pseudo_quantize(W.data_ptr(), _dtype_code(W), R, K, W.stride(0), s.data_ptr(), group_size,
                                     int(bool(symmetric)), num_bits, out.data_ptr(), out.stride(0), _stream()))
    return out


def scale_columns(W: torch.Tensor, s: torch.Tensor, divide: bool = False) -> torch.Tensor:
    lib = load()
    R, K = _w2d(W)
    _req(s, torch.float32, "s", 1)
    assert s.numel() == K and s.is_contiguous()
    out = torch.empty((R, K), dtype=W.dtype, device=W.device)
    check("qt_scale_columns", lib.qt_scale_columns(W.data_ptr(), _dtype_code(W), R, K, W.stride(0), s.data_ptr(),
                                                   int(bool(divide)), out.data_ptr(), out.stride(0), _stream()))
    return out


def rtn_quantize(W: torch.Tensor, scale: torch.Tensor, zp: torch.Tensor, group_size: int, num_bits: int = 4):
    """Plain round-to-nearest levels Qt[K, R] int8."""
    lib = load()
    R, K = _w2d(W)
    _req(scale, torch.float32, "scale", 2)
    _req(zp, torch.float32, "zp", 2)
    G = scale.shape[1]
    assert scale.shape == (R, G) and zp.shape == (R, G) and scale.is_contiguous() and zp.is_contiguous()
    Qt = torch.empty((K, R), dtype=torch.int8, device=W.device)
    check("qt_rtn_quantize", lib.qt_rtn_quantize(W.data_ptr(), _dtype_code(W), R, K, W.stride(0), scale.data_ptr(),
                                                 zp.data_ptr(), G, group_size, num_bits, Qt.data_ptr(), _stream()))
    return Qt


# ---- a13  SmoothQuant ----------------------------------------------------------------------
def col_absmax_accumulate(W: torch.Tensor, wmax: torch.Tensor) -> None:
    lib = load()
    R, K = _w2d(W)
    _req(wmax, torch.float32, "wmax", 1)
    assert wmax.numel() == K and wmax.is_contiguous()
    ws = workspace(lib.qt_col_absmax_workspace_bytes(R, K), W.device, "absmax")
    check("qt_col_absmax_accumulate", lib.qt_col_absmax_accumulate(W.data_ptr(), _dtype_code(W), R, K, W.stride(0),
                                                                   wmax.data_ptr(), ws.data_ptr(), ws.numel(),
                                                                   _stream()))


def smoothquant_scales(cmin: torch.Tensor, cmax: torch.Tensor, wmax: torch.Tensor, alpha: float) -> torch.Tensor:
    lib = load()
    for n, t in (("cmin", cmin), ("cmax", cmax), ("wmax", wmax)):
        _req(t, torch.float32, n, 1)
    K = cmin.numel()
    s = torch.empty(K, dtype=torch.float32, device=cmin.device)
    check("qt_smoothquant_scales", lib.qt_smoothquant_scales(cmin.data_ptr(), cmax.data_ptr(), wmax.data_ptr(), K,
                                                             float(alpha), s.data_ptr(), _stream()))
    return s


# ---- <H, X^T X>_F from the Gram kernel's accumulators (tests; the AWQ loss uses it internally) -------
def xtx_dot(X: torch.Tensor, H: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None,
            accumulate: bool = False) -> torch.Tensor:
    """scale * sum_ij H[i][j] (X^T X)[i][j] with H's lower triangle read; X [n, K] bf16 / fp16 contiguous."""
    lib = load()
    code = _act16(X, "X")
    _req(H, torch.float32, "H", 2)
    n, K = X.shape
    assert X.is_contiguous() and H.is_contiguous() and tuple(H.shape) == (K, K)
    if out is None:
        out = torch.zeros(1, dtype=torch.float32, device=X.device)
    ws = workspace(lib.qt_xtx_dot_workspace_bytes(n, K), X.device, "xtx_dot")
    check("qt_xtx_dot", lib.qt_xtx_dot(X.data_ptr(), code, n, K, K, H.data_ptr(), float(scale),
                                       out.data_ptr(), int(accumulate), ws.data_ptr(), ws.numel(), _stream()))
    return out


# ---- fp32-accurate TN product on the bf16 MFMA (tests / micro-benchmarks) ---------------------
def gemm3_tn(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, kind: int = 0):
    """kind 0: C -= A^T B in place; kind 1: C = A^T B through k-split slabs.  A [k, M], B [k, N] fp32."""
    lib = load()
    _req(A, torch.float32, "A", 2)
    _req(B, torch.float32, "B", 2)
    _req(C, torch.float32, "C", 2)
    k, M = A.shape
    k2, N = B.shape
    assert k == k2 and A.stride(1) == 1 and B.stride(1) == 1 and C.stride(1) == 1 and tuple(C.shape) == (M, N)
    ws = workspace(lib.qt_gemm3_tn_f32_workspace_bytes(M, N, k), A.device, "gemm3")
    check("qt_gemm3_tn_f32", lib.qt_gemm3_tn_f32(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), C.data_ptr(),
                                                 C.stride(0), M, N, k, kind, ws.data_ptr(), ws.numel(), _stream()))
    return C


def gemm3_tn_ex(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, kind: int = 0, tri: bool = False, tight: bool = False):
    """``gemm3_tn`` for one problem (A [k, M], B [k, N], C [M, N]) or a batch in one launch (A [n, k, M], B [n, k, N],
    C [n, M, N], contiguous).  tri: B is lower-triangular in 256-blocks and every tile column's k range starts at its own
    column; tight: unpadded internal planes (edge tiles clamp their loads)."""
    lib = load()
    if A.dim() == 2:
        A, B, C3 = A[None], B[None], C[None]
    else:
        C3 = C
    _req(A, torch.float32, "A", 3)
    _req(B, torch.float32, "B", 3)
    _req(C3, torch.float32, "C", 3)
    n, k, M = A.shape
    n2, k2, N = B.shape
    assert n == n2 and k == k2 and tuple(C3.shape) == (n, M, N)
    assert A.is_contiguous() and B.is_contiguous() and C3.is_contiguous()
    ws = workspace(n * lib.qt_gemm3_tn_f32_workspace_bytes(M, N, k), A.device, "gemm3")
    check("qt_gemm3_tn_f32_ex", lib.qt_gemm3_tn_f32_ex(A.data_ptr(), M, B.data_ptr(), N, C3.data_ptr(), N, M, N, k, kind,
                                                       int(tri), int(tight), n, k * M, k * N, M * N, ws.data_ptr(),
                                                       ws.numel(), _stream()))
    return C


def gemm3_tn_f16x2(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, bound_a, bound_b, kind: int = 0,
                   tri: bool = False, tight: bool = False):
    """``gemm3_tn_ex`` on two fp16 planes per operand and three plane products.  ``bound_a`` / ``bound_b``: a float, or
    one per problem of a batch, with |A_b| <= bound_a[b] and |B_b| <= bound_b[b] elementwise (host values)."""
    import ctypes

    lib = load()
    if A.dim() == 2:
        A, B, C3 = A[None], B[None], C[None]
    else:
        C3 = C
    _req(A, torch.float32, "A", 3)
    _req(B, torch.float32, "B", 3)
    _req(C3, torch.float32, "C", 3)
    n, k, M = A.shape
    n2, k2, N = B.shape
    assert n == n2 and k == k2 and tuple(C3.shape) == (n, M, N)
    # every [b] slice a contiguous matrix; the batch stride may be padded (a multiple of 4 elements)
    for t, cols in ((A, M), (B, N), (C3, N)):
        assert t.stride(2) == 1 and t.stride(1) == cols and (n == 1 or (t.stride(0) >= t.shape[1] * cols and t.stride(0) % 4 == 0))
    ba = [float(bound_a)] * n if not hasattr(bound_a, "__len__") else [float(x) for x in bound_a]
    bb = [float(bound_b)] * n if not hasattr(bound_b, "__len__") else [float(x) for x in bound_b]
    assert len(ba) == n and len(bb) == n
    ba_c, bb_c = (ctypes.c_float * n)(*ba), (ctypes.c_float * n)(*bb)
    ws = workspace(n * lib.qt_gemm3_tn_f32_workspace_bytes(M, N, k), A.device, "gemm3")
    check("qt_gemm3_tn_f16x2", lib.qt_gemm3_tn_f16x2(
        A.data_ptr(), M, B.data_ptr(), N, C3.data_ptr(), N, M, N, k, kind, int(tri), int(tight), n, A.stride(0), B.stride(0),
        C3.stride(0), ctypes.cast(ba_c, ctypes.c_void_p), ctypes.cast(bb_c, ctypes.c_void_p), ws.data_ptr(), ws.numel(), _stream()))
    return C


# ---- fp32 TN GEMM (tests / micro-benchmarks) ------------------------------------------------
def sgemm_tn(A: torch.Tensor, B: torch.Tensor, Cin: Optional[torch.Tensor] = None, mode: int = 1,
             skip_zero_k: bool = False, allow_split_k: bool = False, out: Optional[torch.Tensor] = None):
    """acc = A^T B with A [k, M], B [k, N] fp32 row-major; mode 0: Cin - acc, 1: acc, 2: -acc."""
    lib = load()
    _req(A, torch.float32, "A", 2)
    _req(B, torch.float32, "B", 2)
    k, M = A.shape
    k2, N = B.shape
    assert k == k2 and A.stride(1) == 1 and B.stride(1) == 1
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    ws = workspace(lib.qt_sgemm_tn_f32_workspace_bytes(M, N) if allow_split_k else 1, A.device, "sgemm")
    check("qt_sgemm_tn_f32", lib.qt_sgemm_tn_f32(
        A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), _ptr(Cin), Cin.stride(0) if Cin is not None else 0,
        out.data_ptr(), out.stride(0), M, N, k, int(skip_zero_k), mode, int(allow_split_k),
        ws.data_ptr() if allow_split_k else None, ws.numel() if allow_split_k else 0, _stream()))
    return out


# ---- evaluation: LM head + cross-entropy, logits never stored ---------------------------------
LM_HEAD_K_UNIT = 128        # include/quantool_amd.h: QT_LM_HEAD_K_UNIT / _MIN_K / _MAX_K / the pitch bound
LM_HEAD_MIN_K = 128
LM_HEAD_MAX_K = 32768
LM_HEAD_MAX_PITCH = 1 << 22


def lm_head_k_supported(K: int) -> bool:
    """Whether ``qt_lm_head_nll`` takes a hidden size of K."""
    return LM_HEAD_MIN_K <= K <= LM_HEAD_MAX_K and K % LM_HEAD_K_UNIT == 0


def _lm_head_operands(hidden, W: torch.Tensor, targets: torch.Tensor):
    """The checks that ``qt_lm_head_nll`` and ``qt_lm_head_kl`` share, made before the library is touched.  ``hidden``:
    (name, tensor) of each hidden-state operand; the first sets device, dtype and shape for the rest.  Returns
    (dtype code, M, K, V, the hidden operands' pitches, W's pitch)."""
    name0, H = hidden[0]
    code = _x2d(H, name0)
    M, K = H.shape
    for name, X in hidden[1:]:
        _x2d(X, name)
        if X.device != H.device:
            raise ValueError(f"{name} must be a device tensor on {name0}'s device {H.device}, got {X.device}")
        if X.dtype != H.dtype:
            raise TypeError(f"{name} must be of {name0}'s dtype {H.dtype}, got {X.dtype}")
        if X.shape != H.shape:
            raise ValueError(f"{name} must be of {name0}'s shape {tuple(H.shape)}, got {tuple(X.shape)}")
    if not W.is_cuda or W.device != H.device:
        raise ValueError(f"W must be a device tensor on {name0}'s device {H.device}, got {W.device}")
    if W.dtype != H.dtype:
        raise TypeError(f"W must be of {name0}'s dtype {H.dtype}, got {W.dtype}")
    if W.dim() != 2 or W.stride(1) != 1:
        raise ValueError(f"W must be 2-d [V, K] with unit column stride, got shape {tuple(W.shape)} strides {W.stride()}")
    V = W.shape[0]
    if W.shape[1] != K:
        raise ValueError(f"W must be [V, {K}], got {tuple(W.shape)}")
    if V < 1:
        raise ValueError("W must have at least one row")
    if not lm_head_k_supported(K):
        raise ValueError(f"K {K} unsupported: a multiple of {LM_HEAD_K_UNIT} in [{LM_HEAD_MIN_K}, {LM_HEAD_MAX_K}] only")
    if not targets.is_cuda or targets.device != H.device:
        raise ValueError(f"targets must be a device tensor on {name0}'s device {H.device}, got {targets.device}")
    if targets.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"targets must be torch.int32 or torch.int64, got {targets.dtype}")
    if targets.dim() != 1 or targets.numel() != M or not targets.is_contiguous():
        raise ValueError(f"targets must be contiguous [{M}], got shape {tuple(targets.shape)}")
    # a one-row matrix may carry any stride(0): the pitch of a single row is never used, K keeps the host check quiet
    ldhs = [X.stride(0) if M > 1 else K for _, X in hidden]
    ldw = W.stride(0) if V > 1 else K
    for name, t, ld in [(n, X, l) for (n, X), l in zip(hidden, ldhs)] + [("W", W, ldw)]:
        if ld < K or ld % 8 or ld > LM_HEAD_MAX_PITCH:
            raise ValueError(f"{name}: row pitch {ld} must be a multiple of 8 elements in [{K}, {LM_HEAD_MAX_PITCH}]")
        if t.data_ptr() % 16:
            raise ValueError(f"{name} must start on a 16-byte boundary")
    return code, M, K, V, ldhs, ldw


def lm_head_nll(H: torch.Tensor, W: torch.Tensor, targets: torch.Tensor, return_target_logit: bool = False):
    """Per-row cross-entropy of the LM head without the logits (``qt_lm_head_nll``): H [M, K] and W [V, K], both bf16
    or both fp16 (unit column stride, any 16-byte-aligned row pitch), targets [M] int32 / int64 -> (nll fp32 [M], lse
    fp32 [M], argmax int32 [M]); with ``return_target_logit`` the fp32 target logit [M] as a fourth.  A negative target
    is ignored (nll 0), a target >= V gives NaN."""
    code, M, K, V, (ldh,), ldw = _lm_head_operands((("H", H),), W, targets)
    lib = load()
    dev = H.device
    nll = torch.empty(M, dtype=torch.float32, device=dev)
    lse = torch.empty(M, dtype=torch.float32, device=dev)
    tgt = torch.empty(M, dtype=torch.float32, device=dev)
    argmax = torch.empty(M, dtype=torch.int32, device=dev)
    if M == 0:
        return (nll, lse, argmax, tgt) if return_target_logit else (nll, lse, argmax)
    ws = workspace(lib.qt_lm_head_nll_workspace_size(M, V), dev, "lm_head_nll")
    check("qt_lm_head_nll", lib.qt_lm_head_nll(
        H.data_ptr(), ldh, W.data_ptr(), ldw, code, M, K, V, targets.data_ptr(), targets.element_size(), nll.data_ptr(),
        lse.data_ptr(), tgt.data_ptr(), argmax.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return (nll, lse, argmax, tgt) if return_target_logit else (nll, lse, argmax)


LmHeadKl = namedtuple("LmHeadKl", "kl nll_p nll_q lse_p lse_q argmax_p argmax_q")


def lm_head_kl(Hp: torch.Tensor, Hq: torch.Tensor, W: torch.Tensor, targets: Optional[torch.Tensor] = None) -> LmHeadKl:
    """Per-row KL(P || Q) of two models that share the head weight W, without either logit matrix (``qt_lm_head_kl``):
    Hp, Hq [M, K] (the original's and the quantised model's hidden states) and W [V, K], all bf16 or all fp16 (unit
    column stride, any 16-byte-aligned row pitch, Hp's and Hq's may differ), targets [M] int32 / int64 or None (every
    row ignored) -> ``(kl, nll_p, nll_q, lse_p, lse_q, argmax_p, argmax_q)``, fp32 [M] and int32 [M].  Each side's lse,
    argmax and nll are ``lm_head_nll``'s for that side, to the bit; ``kl`` is not clamped at 0."""
    if targets is None:
        _x2d(Hp, "Hp")
        targets = torch.full((Hp.shape[0],), -100, dtype=torch.int64, device=Hp.device)
    code, M, K, V, (ldhp, ldhq), ldw = _lm_head_operands((("Hp", Hp), ("Hq", Hq)), W, targets)
    lib = load()
    dev = Hp.device
    f = [torch.empty(M, dtype=torch.float32, device=dev) for _ in range(5)]
    am = [torch.empty(M, dtype=torch.int32, device=dev) for _ in range(2)]
    out = LmHeadKl(*f, *am)
    if M == 0:
        return out
    ws = workspace(lib.qt_lm_head_kl_workspace_size(M, V), dev, "lm_head_kl")
    check("qt_lm_head_kl", lib.qt_lm_head_kl(
        Hp.data_ptr(), ldhp, Hq.data_ptr(), ldhq, W.data_ptr(), ldw, code, M, K, V, targets.data_ptr(),
        targets.element_size(), *(t.data_ptr() for t in out), ws.data_ptr(), ws.numel(), _stream()))
    return out
