"""An independent reader of the checkpoints this project writes, and fp64 reference outputs of the Linears and expert
banks they define (a test helper, not part of the package).

Nothing here imports ``quantool_amd``: the files are read with ``safetensors`` and decoded by the format
include/quantool_amd.h states, so a decoding rule the loader and its own tests share is checked against a second
statement of it.

* ``weight_packed`` int32 [N, ceil(K/8)]: nibble j of word w holds column 8w + j, offset by +8; bits past K are ignored.
* ``weight`` int8 [N, K]; ``weight_scale`` [N, G]; ``weight_zero_point`` [N, G]: w = (q - zp) * s.
* ``weight_g_idx`` [K]: the group of every original column.  Without it the group of column k is k // group_size
  (group_size from ``quantization_config``, 128 by default), or 0 when the weights are channel-wise (G = 1).
* Per-expert names: Mixtral's ``<layer>.block_sparse_moe.experts.{e}.w1 / w3 / w2`` and
  ``<layer>.mlp.experts.{e}.gate_proj / up_proj / down_proj`` are (gate, up, down) of expert e of ``<layer>``.
"""
from __future__ import annotations

import json
import re
from pathlib import Path
from typing import Dict, Tuple

import numpy as np
import torch

LEAVES = ("weight", "weight_packed", "weight_scale", "weight_zero_point", "weight_g_idx", "weight_shape")
ROLE = {"w1": "gate", "w3": "up", "w2": "down", "gate_proj": "gate", "up_proj": "up", "down_proj": "down"}
_EXPERT = re.compile(r"^(?P<layer>.+)\.(?:block_sparse_moe|mlp)\.experts\.(?P<e>\d+)\.(?P<proj>w1|w2|w3|gate_proj|"
                     r"up_proj|down_proj)$")
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}     # unit roundoff of the output dtype
U32 = 2.0 ** -24                                                   # of fp32


# ---- reading ----------------------------------------------------------------------------------------------------------
def read_checkpoint(path) -> Tuple[dict, Dict[str, torch.Tensor]]:
    """(config.json as a dict, every tensor of every ``*.safetensors`` shard, on the CPU)."""
    from safetensors.torch import load_file

    path = Path(path)
    cfg = json.loads((path / "config.json").read_text())
    tensors: Dict[str, torch.Tensor] = {}
    for f in sorted(path.glob("*.safetensors")):
        tensors.update(load_file(str(f), device="cpu"))
    return cfg, tensors


def group_size(cfg: dict) -> int:
    w = (((cfg.get("quantization_config") or {}).get("config_groups") or {}).get("group_0") or {}).get("weights") or {}
    return int(w.get("group_size") or 128)


def quantized_modules(tensors: Dict[str, torch.Tensor]) -> Dict[str, Dict[str, torch.Tensor]]:
    """{module name: {leaf: tensor}} of every module with a ``weight_scale``."""
    mods = {k[: -len(".weight_scale")] for k in tensors if k.endswith(".weight_scale")}
    out: Dict[str, Dict[str, torch.Tensor]] = {m: {} for m in mods}
    for k, v in tensors.items():
        mod, _, leaf = k.rpartition(".")
        if mod in out and leaf in LEAVES:
            out[mod][leaf] = v
    return out


def expert_of(name: str):
    """(layer prefix, expert, "gate" / "up" / "down") of a per-expert module name, else None."""
    m = _EXPERT.match(name)
    return None if m is None else (m.group("layer"), int(m.group("e")), ROLE[m.group("proj")])


# ---- decoding ---------------------------------------------------------------------------------------------------------
def decode_int4(packed, K: int) -> np.ndarray:
    """int32 words [N, ceil(K/8)] -> int64 levels [N, K]: nibble j of word w is column 8w + j, minus 8."""
    w = np.asarray(packed).astype(np.int64) & 0xFFFFFFFF
    N, Kw = w.shape
    assert Kw == (K + 7) // 8, (Kw, K)
    nib = (w[:, :, None] >> (4 * np.arange(8, dtype=np.int64))) & 0xF
    return nib.reshape(N, Kw * 8)[:, :K] - 8


def shape_of(t: Dict[str, torch.Tensor]) -> Tuple[int, int]:
    if "weight_shape" in t:
        N, K = (int(v) for v in t["weight_shape"].tolist())
        return N, K
    return tuple(t["weight"].shape)


def levels(t: Dict[str, torch.Tensor]) -> np.ndarray:
    """int64 [N, K]: the stored integer level of every weight, in the file's column order."""
    N, K = shape_of(t)
    if "weight_packed" in t:
        q = decode_int4(t["weight_packed"].numpy(), K)
    else:
        q = t["weight"].numpy().astype(np.int64)
    assert q.shape == (N, K), (q.shape, N, K)
    return q


def groups(t: Dict[str, torch.Tensor], gsize: int = 128) -> np.ndarray:
    """int64 [K]: the group of every column (weight_g_idx, else k // gsize, or 0 when channel-wise)."""
    N, K = shape_of(t)
    G = t["weight_scale"].shape[1]
    if "weight_g_idx" in t:
        g = t["weight_g_idx"].numpy().astype(np.int64)
    elif G == 1:
        g = np.zeros(K, np.int64)
    else:
        assert G == -(-K // gsize), (G, K, gsize)
        g = np.arange(K, dtype=np.int64) // gsize
    assert g.shape == (K,) and g.min() >= 0 and g.max() < G
    return g


def scales(t: Dict[str, torch.Tensor]) -> np.ndarray:
    return t["weight_scale"].to(torch.float32).numpy()


def zero_points(t: Dict[str, torch.Tensor]):
    return None if "weight_zero_point" not in t else t["weight_zero_point"].to(torch.float32).numpy()


def contract_weight(t: Dict[str, torch.Tensor], dtype: torch.dtype, gsize: int = 128) -> torch.Tensor:
    """The A16 contract's weight: round_to_dtype(fp32(q - zp) * fp32(s)), [N, K] in ``dtype``."""
    q = levels(t).astype(np.float32)
    g = groups(t, gsize)
    s = scales(t)
    zp = zero_points(t)
    if zp is not None:
        q = q - zp[:, g]                                      # exact in fp32
    w32 = (q * s[:, g]).astype(np.float32)                  # one fp32 rounding
    return torch.from_numpy(w32).to(dtype)                  # one rounding to the dtype (nearest even)


# ---- fp64 references --------------------------------------------------------------------------------------------------
def ulp(y: torch.Tensor) -> torch.Tensor:
    """ulp of every element of a bf16 / fp16 tensor (the subnormal spacing below the normal range), as fp64."""
    mant = 7 if y.dtype == torch.bfloat16 else 10
    a = y.detach().cpu().float().abs().clamp(min=torch.finfo(y.dtype).tiny)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - mant).double()


def a16_linear(x: torch.Tensor, t: Dict[str, torch.Tensor], bias=None, gsize: int = 128):
    """(y64, mag): y64 = x @ w.T + b in fp64 with the contract weight in x's dtype; mag = |x| @ |w|.T + |b|."""
    w = contract_weight(t, x.dtype, gsize).double()
    x = x.detach().cpu().double()
    y = x @ w.T
    mag = x.abs() @ w.abs().T
    if bias is not None:
        b = bias.detach().cpu().double()
        y = y + b
        mag = mag + b.abs()
    return y, mag


def a8_linear(Xq, s_x, zp_x, t: Dict[str, torch.Tensor], bias=None, gsize: int = 128):
    """(y64, mag): y64 = sum_k s_x (Xq[k] - zp_x) s_w[g(k)] q[k] + b in fp64, columns in the file's order, g(k) from
    the file; mag = |s_x| sum_g |s_w[g] t_g| + |b| with t_g = sum_{k in g} (Xq[k] - zp_x) q[k] (the GEMM's bound)."""
    q = torch.from_numpy(levels(t)).double()
    g = torch.from_numpy(groups(t, gsize))
    s_w = torch.from_numpy(scales(t)).double()
    xz = Xq.detach().cpu().double()
    if zp_x is not None:
        xz = xz - zp_x.detach().cpu().double()[:, None]
    G = s_w.shape[1]
    tot = torch.zeros(xz.shape[0], q.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(tot)
    for j in range(G):
        cols = (g == j).nonzero().flatten()
        tg = xz[:, cols] @ q[:, cols].T                      # integers below 2^53: exact
        tot = tot + tg * s_w[None, :, j]
        mag = mag + (tg * s_w[None, :, j]).abs()
    sx = s_x.detach().cpu().double()[:, None]
    y, mag = sx * tot, sx.abs() * mag
    if bias is not None:
        b = bias.detach().cpu().double()
        y, mag = y + b, mag + b.abs()
    return y, mag


def gemm_i8_tolerance(Y: torch.Tensor, mag: torch.Tensor, G: int) -> torch.Tensor:
    """|Y - y64| bound of qt_gemm_i8's fixed fp32 sequence: half an output ulp, plus (G + 4) 2^-24 mag.  Term g meets
    at most G + 3 fp32 roundings (t_g, s_w t_g, at most G - 1 sums, s_x tot, + bias); one more covers second order."""
    return 0.5 * ulp(Y) + (G + 4) * U32 * mag


def gemv_tolerance(Y: torch.Tensor, mag: torch.Tensor, K: int) -> torch.Tensor:
    """|Y - y64| bound of the A16 GEMV (header: ulp/2 + K 2^-24 sum |x w|), and of any fp32-accumulated F.linear on
    the contract weight (K - 1 fp32 sums): one more 2^-24 for the bias add."""
    return 0.5 * ulp(Y) + (K + 1) * U32 * mag


def assert_within(Y: torch.Tensor, y64: torch.Tensor, tol: torch.Tensor, what: str = ""):
    y = Y.detach().cpu().double().reshape(y64.shape)
    assert torch.isfinite(y).all(), f"{what}: non-finite output"
    err = (y - y64).abs()
    bad = (err > tol).nonzero()
    assert bad.numel() == 0, (f"{what}: {bad.shape[0]} of {y.numel()} outside the fp64 bound, first at "
                              f"{bad[0].tolist()}: got {y[tuple(bad[0])].item()}, fp64 {y64[tuple(bad[0])].item()}, "
                              f"bound {tol[tuple(bad[0])].item()}")


def _silu(v):
    return v / (1.0 + torch.exp(-v))


def expert_bank(x: torch.Tensor, top_k_index, top_k_weights, experts: Dict[int, Dict[str, Dict[str, torch.Tensor]]],
                a8_symmetric=None, gsize: int = 128):
    """transformers' MixtralExperts.forward in fp64 on the checkpoint's experts ({e: {"gate" / "up" / "down": leaves}})
    with act_fn = SiLU, and a first-order bound on how far a bf16 / fp16 run of the same operation may lie from it.

    A16 (``a8_symmetric`` None): every expert Linear is x @ w.T with the contract weight.  A8 (``a8_symmetric`` True /
    False): the tokens and the routed rows of act_fn(gate) * up are quantised to int8 per row and the expert Linears are
    sum_k s_x (Xq - zp_x) s_w[g(k)] q[k]; the reference quantises x by ``quantize_rows`` and keeps the routed rows
    unquantised, charging each element the rounding of its quantisation (at most one step s_h of its row).

    The bound charges, with u the unit roundoff of x's dtype: gate / up within u |v| + (K + 1) 2^-24 mag (their output
    rounding and fp32 sums); act_fn's rounding and its Lipschitz constant 1.1; the product's rounding; the down Linear's
    propagation of those, its sums and its rounding; the weight's rounding and the sums of the combine."""
    dt = x.dtype
    u = UNIT[dt]
    X = x.detach().cpu()
    idx = top_k_index.detach().cpu().long()
    wts = top_k_weights.detach().cpu().double()
    T, H = X.shape
    out = torch.zeros(T, H, dtype=torch.float64)
    tol = torch.zeros(T, H, dtype=torch.float64)
    run = torch.zeros(T, H, dtype=torch.float64)            # |partial sums| of the combine
    if a8_symmetric is not None:
        Xq, s_x, zp_x = quantize_rows(X, a8_symmetric)
    for e in sorted(experts):
        pos, tok = torch.where((idx == e).T)                 # slot-major, as transformers lists them
        if tok.numel() == 0:
            continue
        ex = experts[e]
        parts = {}
        for r in ("gate", "up"):
            if a8_symmetric is None:
                y, mag = a16_linear(X[tok], ex[r], gsize=gsize)
            else:
                y, mag = a8_linear(Xq[tok], s_x[tok], None if zp_x is None else zp_x[tok], ex[r], gsize=gsize)
            K = shape_of(ex[r])[1]
            parts[r] = (y, u * y.abs() + (K + 1) * U32 * mag)
        (g, dg), (up, dup) = parts["gate"], parts["up"]
        a = _silu(g)
        da = 1.1 * dg + u * (a.abs() + 1.1 * dg)                            # act_fn(rounded gate), rounded
        h = a * up
        dh = (a.abs() + da) * dup + up.abs() * da + u * (a.abs() + da) * (up.abs() + dup)
        if a8_symmetric is not None:
            hmax = (h.abs() + dh).amax(1, keepdim=True)
            dh = dh + 2.0 * hmax / 255.0 * (1 + u)                          # one quantisation step of the row
        wd = contract_weight(ex["down"], torch.float32, gsize).double() if a8_symmetric is None else \
            _a8_weight(ex["down"], gsize)
        y = h @ wd.T
        Kd = wd.shape[1]
        dy = dh @ wd.abs().T + (Kd + 1) * U32 * ((h.abs() + dh) @ wd.abs().T) + u * y.abs()
        w = wts[tok, pos][:, None]
        c = y * w
        dc = dy * w.abs() + u * (c.abs() + dy * w.abs())
        out.index_add_(0, tok, c)
        run.index_add_(0, tok, c.abs() + dc)
        tol.index_add_(0, tok, dc + u * run[tok])
    return out, tol


def _a8_weight(t, gsize):
    """fp64 [N, K]: s_w[g(k)] q[k] (exact: a product of an fp32 scale and a small integer)."""
    q = torch.from_numpy(levels(t)).double()
    g = torch.from_numpy(groups(t, gsize))
    return q * torch.from_numpy(scales(t)).double()[:, g]


def quantize_rows(X: torch.Tensor, symmetric: bool):
    """Dynamic per-token int8 quantisation as include/quantool_amd.h states it (fp32 steps): (Xq, s_x, zp_x or None)."""
    x = X.detach().cpu().float()
    mn = torch.clamp(x.amin(1), max=0.0)
    mx = torch.clamp(x.amax(1), min=0.0)
    eps = torch.finfo(torch.float32).eps
    if symmetric:
        s = torch.clamp(torch.maximum(-mn, mx) / 127.5, min=eps)
        zp = torch.zeros_like(s)
    else:
        s = torch.clamp((mx - mn) / 255.0, min=eps)
        zp = torch.clamp(torch.round(-128.0 - mn / s), -128.0, 127.0)
    q = torch.round(torch.clamp(x / s[:, None] + zp[:, None], -128.0, 127.0)).to(torch.int8)
    return q, s, (None if symmetric else zp.to(torch.int32))


# ---- synthetic checkpoints ----------------------------------------------------------------------------------------------
def encode_int4(q: np.ndarray, pad_nibble: int = 8) -> np.ndarray:
    """int levels [N, K] in [-8, 7] -> int32 words [N, ceil(K/8)] (nibble j of word w = level of column 8w + j, + 8);
    the nibbles past K hold ``pad_nibble`` (a reader must ignore them)."""
    N, K = q.shape
    Kw = (K + 7) // 8
    v = np.full((N, Kw * 8), pad_nibble, np.int64)
    v[:, :K] = q + 8
    words = (v.reshape(N, Kw, 8) << (4 * np.arange(8, dtype=np.int64))).sum(-1)
    return words.astype(np.uint32).view(np.int32)


def from_checkpoint(path):
    """(config, dense tensors, {quantized module: (N, K)}) of a saved checkpoint, its quantized leaves dropped."""
    cfg, tensors = read_checkpoint(path)
    quant = quantized_modules(tensors)
    dense = {k: v for k, v in tensors.items() if k.rpartition(".")[0] not in quant}
    return cfg, dense, {m: shape_of(t) for m, t in quant.items()}


def write_synthetic(dst, cfg: dict, dense: Dict[str, torch.Tensor], linears: Dict[str, Tuple[int, int]], *, bits: int,
                    zero_point: bool = False, act: str = None, g_idx: bool = False, seed: int = 0,
                    scale_dtype=torch.bfloat16, gsize: int = 128, resize: Dict[int, int] = None):
    """Write a grouped checkpoint (G = ceil(K/gsize), any K) of random levels and scales for ``linears`` beside the
    ``dense`` tensors.  ``act``: None (A16), "sym" / "asym" (the 8-bit dynamic per-token activation block of W8A8 /
    W4A8).  ``g_idx``: a permuted weight_g_idx (groups of gsize columns each, in shuffled order), shared by the gate and
    up Linears of an expert and left out of A8 experts (which the runtime refuses with one).  ``resize`` maps a width to
    another in ``cfg`` and in every Linear's shape (to give a model a width that is not a multiple of 8).  Packed words
    carry 0xF past K.  Returns the written {module: leaves}."""
    import copy

    from safetensors.torch import save_file

    dst = Path(dst)
    dst.mkdir(parents=True, exist_ok=True)
    cfg = copy.deepcopy(cfg)
    resize = resize or {}
    for k in ("intermediate_size", "hidden_size"):
        if cfg.get(k) in resize:
            cfg[k] = resize[cfg[k]]
    rng = np.random.default_rng(seed)
    lo, hi = (-8, 8) if bits == 4 else (-128, 128)
    base = 0.02 / (4.6 if bits == 4 else 74.0)             # weights of about Llama's init scale
    out: Dict[str, Dict[str, torch.Tensor]] = {}
    shared_g: Dict[Tuple[str, int, int], np.ndarray] = {}
    for name in sorted(linears):
        N, K = (resize.get(d, d) for d in linears[name])
        G = -(-K // gsize)
        q = rng.integers(lo, hi, (N, K))
        s = (base * rng.uniform(0.5, 1.5, (N, G))).astype(np.float32)
        t = {"weight_scale": torch.from_numpy(s).to(scale_dtype), "weight_shape": torch.tensor([N, K])}
        if bits == 4:
            t["weight_packed"] = torch.from_numpy(encode_int4(q, pad_nibble=0xF))
        else:
            t["weight"] = torch.from_numpy(q.astype(np.int8))
        if zero_point:
            t["weight_zero_point"] = torch.from_numpy(rng.integers(-3, 4, (N, G)).astype(np.int8))
        ex = expert_of(name)
        if g_idx and not (act is not None and ex is not None):
            key = (ex[0], ex[1], ex[2] == "down") if ex is not None else (name, 0, False)
            if key not in shared_g:
                shared_g[key] = (np.arange(K) // gsize)[rng.permutation(K)].astype(np.int32)
            t["weight_g_idx"] = torch.from_numpy(shared_g[key])
        out[name] = t
    state = dict(dense)
    for name, t in out.items():
        state.update({f"{name}.{leaf}": v.contiguous() for leaf, v in t.items()})
    for old in dst.glob("*.safetensors"):
        old.unlink()
    save_file(state, str(dst / "model.safetensors"), metadata={"format": "pt"})
    weights = {"num_bits": bits, "type": "int", "symmetric": not zero_point, "strategy": "group",
               "group_size": gsize, "dynamic": False, "actorder": "group" if g_idx else None, "observer": "minmax",
               "block_structure": None}
    acts = None if act is None else {"num_bits": 8, "type": "int", "symmetric": act == "sym", "strategy": "token",
                                     "group_size": None, "dynamic": True, "actorder": None, "observer": "",
                                     "block_structure": None}
    qcfg = dict(cfg.get("quantization_config") or {})
    qcfg.update({"quant_method": "compressed-tensors", "quantization_status": "compressed",
                 "format": "int-quantized" if act is not None else "pack-quantized",
                 "config_groups": {"group_0": {"targets": ["Linear"], "weights": weights, "input_activations": acts,
                                               "output_activations": None}}})
    qcfg.setdefault("ignore", ["lm_head"])
    cfg["quantization_config"] = qcfg
    (dst / "config.json").write_text(json.dumps(cfg, indent=2, default=str))
    return out
