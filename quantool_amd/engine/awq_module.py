"""AWQ on ``torch.nn.Module`` decoder layers: the mapping resolver and the per-layer search / apply /
quantise cycle (SURVEY.md 8f row N1 for ``method=awq``; upstream AWQModifier as recalled in SURVEY
Appendix A.3, reached from ``src/quantool/methods/llm_compressor/awq/awq.py:81`` / ``base.py:161``).

A *mapping* ties one smooth layer (a norm, or a Linear whose output feeds the balance layers
unchanged) to the balance Linears that read its output.  Per mapping, on the device:

1. ``x_mean`` = mean |x| per input channel of the balance layers  (``qt_act_stats_accumulate``)
2. ``w_mean`` = mean group-normalised |W| over all balance rows   (``qt_awq_weight_mean_accumulate``)
3. the 20 candidate scale vectors                                   (``qt_awq_scales``)
4. search loss of each candidate:
     * one balance Linear (v->o, up->down): the parent module *is* that Linear, so the loss is the
       Frobenius product <X^T X, D^T D> -- ``qt_awq_loss`` on the Gram sum taken in step 1's pass;
     * several balance Linears (norm->q/k/v, norm->gate/up): the parent is their common ancestor
       (self_attn, mlp); trial weights come from ``qt_awq_pseudo_quantize`` and the parent is run by
       torch on the cached inputs -- the model's own forward is the caller's code, not this path's.
5. apply the winner: ``W_balance *= s`` (``qt_scale_columns``), smooth layer ``/= s``.

After every mapping of the layer has been applied, each targeted Linear goes through the standard
observer + round-to-nearest + pack (``awq_linear.rtn_finalize``).

Sparse-MoE layers (an unfused expert bank, ``sequential._UnfusedExperts``, and no user mappings) get
mappings chosen by structure instead of by name (``_resolve_moe``): one *bank* mapping
norm -> every expert's ``gate_up_proj`` with the MoE block as the parent and the router as a
scale-only consumer, and per expert ``gate_up_proj`` rows ``[I, 2I)`` -> ``down_proj``.

A mapping whose capture saw no token (an expert nothing was routed to) or, with several balance
layers, no call of its parent is skipped with a warning: its Linears are still quantised, without
smoothing scales.  Non-finite losses raise.
"""
from __future__ import annotations

import logging
import re
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from ..hip import ops
from .awq_linear import AWQResult, rtn_finalize
from .schemes import QuantArgs

logger = logging.getLogger(__name__)

#: Llama-family defaults: smooth-layer pattern -> balance-layer patterns
DEFAULT_MAPPINGS: Tuple[Tuple[str, Tuple[str, ...]], ...] = (
    ("re:.*input_layernorm$", ("re:.*q_proj$", "re:.*k_proj$", "re:.*v_proj$")),
    ("re:.*v_proj$", ("re:.*o_proj$",)),
    ("re:.*post_attention_layernorm$", ("re:.*gate_proj$", "re:.*up_proj$")),
    ("re:.*up_proj$", ("re:.*down_proj$",)),
)


@dataclass
class ResolvedMapping:
    smooth_name: str
    smooth: nn.Module
    balance_names: List[str]
    balance: List[nn.Linear]
    parent_name: str
    parent: nn.Module
    #: consumers of the smooth layer's output that are rescaled with the balance layers (columns *= s) but take no
    #: part in the search and are not quantised: a sparse-MoE block's router
    scale_only_names: List[str] = field(default_factory=list)
    scale_only: List[nn.Module] = field(default_factory=list)
    #: the smooth layer is output rows [lo, hi) of a fused Linear (the up half of ``gate_up_proj``), not all of it
    smooth_rows: Optional[Tuple[int, int]] = None
    #: x_mean is taken from the parent's input (every token of the block), not from ``balance[0]``'s
    stats_at_parent: bool = False

    @property
    def single(self) -> bool:
        return self.parent is self.balance[0]


def _pattern_hits(pattern: str, name: str) -> bool:
    if pattern.startswith("re:"):
        return re.match(pattern[3:], name) is not None
    return name == pattern or name.endswith("." + pattern)


def normalise_mappings(mappings: Optional[Sequence[Any]]) -> List[Tuple[str, List[str]]]:
    """Accepts upstream's ``AWQMapping``-like objects / dicts (``smooth_layer``, ``balance_layers``)
    and plain ``[smooth, [balance, ...]]`` pairs as a quantool YAML would carry them."""
    if not mappings:
        return [(s, list(b)) for s, b in DEFAULT_MAPPINGS]
    out = []
    for m in mappings:
        if isinstance(m, dict):
            smooth, balance = m["smooth_layer"], m["balance_layers"]
        elif hasattr(m, "smooth_layer"):
            smooth, balance = m.smooth_layer, m.balance_layers
        else:
            smooth, balance = m[0], m[1]
        out.append((str(smooth), [balance] if isinstance(balance, str) else [str(b) for b in balance]))
    return out


def _common_parent(names: Sequence[str]) -> str:
    parts = [n.split(".") for n in names]
    common = []
    for segs in zip(*parts):
        if len(set(segs)) != 1:
            break
        common.append(segs[0])
    return ".".join(common)


def _resolve_one(named: Dict[str, nn.Module], smooth_name: str, bal: List[str], wanted) -> Optional[ResolvedMapping]:
    if not bal or not all(wanted(n, named[n]) for n in bal):
        return None
    smooth = named[smooth_name]
    K = named[bal[0]].in_features
    if any(named[n].in_features != K for n in bal):
        return None
    if isinstance(smooth, nn.Linear) and smooth.out_features != K:
        logger.info(f"AWQ mapping {smooth_name} -> {bal} skipped: widths {smooth.out_features} != {K}")
        return None
    if not isinstance(smooth, nn.Linear) and (getattr(smooth, "weight", None) is None
                                              or smooth.weight.numel() != K):
        return None
    parent_name = bal[0] if len(bal) == 1 else _common_parent(bal)
    if parent_name not in named:
        return None
    return ResolvedMapping(smooth_name, smooth, bal, [named[n] for n in bal], parent_name, named[parent_name])


def _under(name: str, prefix: str) -> bool:
    return name == prefix or name.startswith(prefix + ".")


def _resolve_moe(named: Dict[str, nn.Module], banks: List[str], wanted) -> List[ResolvedMapping]:
    """Default mappings of a layer that holds unfused expert banks: the name-pattern mappings
    that stay outside every MoE block, then per bank the bank mapping and one up -> down mapping per expert."""
    blocks = [b.rpartition(".")[0] for b in banks]
    resolved: List[ResolvedMapping] = []
    for smooth_pat, balance_pats in DEFAULT_MAPPINGS:
        hits = [n for n in named if _pattern_hits(smooth_pat, n) and not any(_under(n, b) for b in banks)]
        bal = [n for n in named if isinstance(named[n], nn.Linear) and any(_pattern_hits(p, n) for p in balance_pats)
               and not any(_under(n, b) for b in banks)]
        if len(hits) != 1:
            continue
        inside = [n for n in bal if any(blk and _under(n, blk) for blk in blocks)]
        if inside and not any(blk and _under(hits[0], blk) for blk in blocks):
            # a norm in front of a MoE block also feeds the router and the bank: rescaling it for some of the
            # block's Linears alone would change the others' inputs
            logger.info(f"AWQ mapping {hits[0]} -> {bal} skipped: balance layers inside a sparse-MoE block")
            continue
        mp = _resolve_one(named, hits[0], bal, wanted)
        if mp is not None:
            resolved.append(mp)
    norm_pat = DEFAULT_MAPPINGS[2][0]
    for bank_name, block_name in zip(banks, blocks):
        bank = named[bank_name]
        experts = [f"{bank_name}.experts.{e}" for e in range(len(bank.experts))]
        gate_up = [f"{x}.gate_up_proj" for x in experts]
        H = named[gate_up[0]].in_features
        mp = _bank_mapping(named, bank_name, block_name, gate_up, H, norm_pat, wanted)
        if mp is not None:
            resolved.append(mp)
        for x in experts:
            gu, dn = named[f"{x}.gate_up_proj"], named[f"{x}.down_proj"]
            inter = dn.in_features
            if not wanted(f"{x}.down_proj", dn):
                continue
            if gu.out_features != 2 * inter:
                logger.info(f"AWQ mapping {x}.gate_up_proj -> down_proj skipped: {gu.out_features} rows are not "
                            f"a gate and an up half of {inter}")
                continue
            resolved.append(ResolvedMapping(f"{x}.gate_up_proj", gu, [f"{x}.down_proj"], [dn], f"{x}.down_proj", dn,
                                            smooth_rows=(inter, 2 * inter)))
    return resolved


def _bank_mapping(named, bank_name: str, block_name: str, gate_up: List[str], H: int, norm_pat: str,
                  wanted) -> Optional[ResolvedMapping]:
    """norm -> every expert's gate_up_proj, parent = the MoE block, router scale-only; None (logged) when the
    rewrite cannot be shown to preserve the block's function."""
    def skip(why):
        logger.info(f"AWQ bank mapping of {bank_name} skipped: {why}")

    if not block_name or block_name not in named:
        return skip("the bank has no enclosing MoE block inside the layer")
    if not all(wanted(n, named[n]) for n in gate_up):
        return skip("an expert's gate_up_proj is not targeted")
    norms = [n for n in named if _pattern_hits(norm_pat, n) and not _under(n, block_name)]
    if len(norms) != 1 or getattr(named[norms[0]], "weight", None) is None or named[norms[0]].weight.numel() != H:
        return skip(f"no single norm of width {H} in front of the block")
    block = named[block_name]
    if any(True for _ in block.parameters(recurse=False)):
        return skip("the block holds parameters of its own")
    # every parameterised module of the block outside the bank may read the block input: exactly one, with a 2-d
    # weight [*, H], is the router; anything further (shared experts, a second gate) is a consumer that this
    # mapping does not rescale
    others = [n for n in named if _under(n, block_name) and n != block_name and not _under(n, bank_name)
              and any(True for _ in named[n].parameters(recurse=False))]
    if len(others) != 1:
        return skip(f"the block holds {len(others)} parameterised modules beside the bank ({others}): "
                    "a router alone is expected, further consumers of the block input are not rescaled")
    router = named[others[0]]
    w = getattr(router, "weight", None)
    extra = [k for k, p in router.named_parameters(recurse=False) if k != "weight" and p.dim() != 1]
    if w is None or w.dim() != 2 or w.shape[1] != H or extra:
        return skip(f"{others[0]} is no router with a weight [*, {H}]")
    return ResolvedMapping(norms[0], named[norms[0]], gate_up, [named[n] for n in gate_up], block_name, block,
                           scale_only_names=[others[0]], scale_only=[router], stats_at_parent=True)


def resolve_mappings(layer: nn.Module, layer_name: str, mappings: Sequence[Tuple[str, List[str]]],
                     wanted) -> List[ResolvedMapping]:
    """Match the patterns inside one decoder layer.  A mapping is dropped when its smooth layer or
    all balance layers are absent, when a balance layer is not targeted, or when a Linear smooth
    layer's output width differs from the balance input width (v_proj -> o_proj under GQA).

    A smooth pattern with several hits (per-expert modules) pairs each hit with the balance hits under the
    nearest ancestor that holds any.  A layer with an unfused expert bank, given the default table, resolves by
    structure instead (``_resolve_moe``)."""
    from .sequential import _UnfusedExperts

    named = {(f"{layer_name}.{n}" if n else layer_name): m for n, m in layer.named_modules()}
    banks = [n for n, m in named.items() if isinstance(m, _UnfusedExperts)]
    if banks and [(s, list(b)) for s, b in mappings] == normalise_mappings(None):
        return _resolve_moe(named, banks, wanted)
    resolved: List[ResolvedMapping] = []
    for smooth_pat, balance_pats in mappings:
        smooth_hits = [n for n in named if _pattern_hits(smooth_pat, n)]
        bal = [n for n in named if isinstance(named[n], nn.Linear) and any(_pattern_hits(p, n) for p in balance_pats)]
        if not smooth_hits or not bal:
            continue
        if len(smooth_hits) == 1:
            pairs = [(smooth_hits[0], bal)]
        else:
            pairs = []
            for hit in smooth_hits:
                anc = hit.rpartition(".")[0]
                while anc and not any(_under(n, anc) and n != hit for n in bal):
                    anc = anc.rpartition(".")[0]
                if anc:
                    pairs.append((hit, [n for n in bal if _under(n, anc) and n != hit]))
        for hit, its in pairs:
            mp = _resolve_one(named, hit, its, wanted)
            if mp is not None:
                resolved.append(mp)
    return resolved


def _first(out):
    return out[0] if isinstance(out, (tuple, list)) else out


def _as_rows16(x: torch.Tensor) -> torch.Tensor:
    x = x.reshape(-1, x.shape[-1])
    return ops.as_act16(x)


def _block_input(args, kwargs) -> torch.Tensor:
    """The hidden states a block was called with (first positional tensor, else ``hidden_states=``)."""
    for a in args:
        if torch.is_tensor(a):
            return a
    return kwargs["hidden_states"]


class _Capture:
    """What one mapping needs from the calibration pass over the layer."""

    def __init__(self, mp: ResolvedMapping, dev):
        K = mp.balance[0].in_features
        self.x_abs_sum = torch.zeros(K, dtype=torch.float32, device=dev)
        self.n_tokens = 0
        self.gram = torch.zeros((K, K), dtype=torch.float32, device=dev) if mp.single else None
        self.parent_calls: List[tuple] = []      # (args, kwargs) per batch, multi-balance mappings only
        self.stats_at_parent = mp.stats_at_parent

    def _stats(self, x):
        x = _as_rows16(x)
        ops.act_stats_accumulate(x, abs_sum=self.x_abs_sum)
        if self.gram is not None:
            ops.xtx_accumulate(x, self.gram)
        self.n_tokens += x.shape[0]

    def on_balance_input(self, _mod, args):
        self._stats(args[0])

    def on_parent_call(self, _mod, args, kwargs):
        if self.stats_at_parent:
            self._stats(_block_input(args, kwargs))
        self.parent_calls.append((args, kwargs))

    def skip_reason(self, mp: ResolvedMapping) -> Optional[str]:
        """Why this mapping has nothing to search on, or None."""
        if self.n_tokens == 0:
            return "its balance layers saw no calibration token"
        if not mp.single and not self.parent_calls:
            return f"its parent {mp.parent_name} ({type(mp.parent).__name__}) was never called"
        return None


def _require_finite(losses: torch.Tensor, mp: ResolvedMapping) -> None:
    if not bool(torch.isfinite(losses).all()):
        raise FloatingPointError(f"AWQ search of {mp.smooth_name} -> {mp.balance_names}: non-finite losses "
                                 f"{losses.tolist()}")


def _search(mp: ResolvedMapping, cap: _Capture, qargs: QuantArgs, n_grid: int, duo_scaling: bool):
    """Returns (scales[n_grid, K], losses[n_grid], best index tensor).  The caller has checked
    ``cap.skip_reason``: there are tokens, and parent calls where the parent is run."""
    dev = cap.x_abs_sum.device
    gs = qargs.kernel_group_size
    K = mp.balance[0].in_features
    w_sum = torch.zeros(K, dtype=torch.float32, device=dev)
    n_rows = 0
    for lin in mp.balance:
        ops.awq_weight_mean_accumulate(lin.weight.data, gs, w_sum)
        n_rows += lin.out_features
    scales = ops.awq_scales(cap.x_abs_sum, cap.n_tokens, w_sum, n_rows, n_grid, duo_scaling)
    losses = torch.zeros(n_grid, dtype=torch.float32, device=dev)
    if mp.single:
        from .awq_linear import search_losses_enqueue

        ops.symmetrize_lower(cap.gram)
        pending = search_losses_enqueue([mp.balance[0].weight.data], scales, cap.gram, cap.n_tokens, qargs)
        _require_finite(pending.losses, mp)
        losses, best = pending.resolve()
        return scales, losses, best
    else:
        # scale-only consumers (a MoE router) keep their weights throughout: every grid point routes alike
        originals = [lin.weight.data.clone() for lin in mp.balance]
        fp_out = [_first(mp.parent(*a, **kw)).float() for a, kw in cap.parent_calls]
        n_elem = float(sum(o.numel() for o in fp_out))
        try:
            for gi in range(n_grid):
                for lin, w0 in zip(mp.balance, originals):
                    ops.awq_pseudo_quantize(w0, scales[gi], gs, qargs.symmetric, qargs.num_bits, out=lin.weight.data)
                sq = torch.zeros((), dtype=torch.float32, device=dev)
                for (a, kw), ref in zip(cap.parent_calls, fp_out):
                    sq += (ref - _first(mp.parent(*a, **kw)).float()).pow(2).sum()
                losses[gi] = sq / n_elem
        finally:
            for lin, w0 in zip(mp.balance, originals):
                lin.weight.data.copy_(w0)
    _require_finite(losses, mp)
    # multi-consumer mapping: the parent module's own forward (the caller's torch code) produced the
    # losses above; the arg-min of the 20 numbers is the device kernel the Gram form uses
    return scales, losses, ops.argmin_first(losses).to(torch.int64).reshape(())


def _apply(mp: ResolvedMapping, s: torch.Tensor) -> None:
    for mod in list(mp.balance) + list(mp.scale_only):
        mod.weight.data.copy_(ops.scale_columns(mod.weight.data, s))
    K = s.numel()
    sm = mp.smooth
    if isinstance(sm, nn.Linear):
        # the named output rows (and bias entries) of the producing Linear; the last K where none are named
        lo, hi = mp.smooth_rows or (sm.out_features - K, sm.out_features)
        rows = sm.weight.data[lo:hi]
        rows.copy_((rows.float() / s[:, None]).to(rows.dtype))
        if sm.bias is not None:
            sm.bias.data[lo:hi].copy_((sm.bias.data[lo:hi].float() / s).to(sm.bias.dtype))
    else:
        sm.weight.data.copy_((sm.weight.data.float() / s).to(sm.weight.dtype))
        if getattr(sm, "bias", None) is not None:
            sm.bias.data.copy_((sm.bias.data.float() / s).to(sm.bias.dtype))


def awq_layer(layer: nn.Module, layer_name: str, cache: Sequence[tuple], modifier, dev) -> Dict[str, AWQResult]:
    """Search, smooth and quantise one decoder layer in place; returns the per-Linear results."""
    qargs = modifier.weight_args()
    named = {(f"{layer_name}.{n}" if n else layer_name): m for n, m in layer.named_modules()}
    linears = {n: m for n, m in named.items() if isinstance(m, nn.Linear) and modifier.wants(n, m)}
    mappings = resolve_mappings(layer, layer_name, normalise_mappings(modifier.mappings), modifier.wants)

    caps = [_Capture(mp, dev) for mp in mappings]
    hooks = []
    for mp, cap in zip(mappings, caps):
        if not mp.stats_at_parent:
            hooks.append(mp.balance[0].register_forward_pre_hook(cap.on_balance_input))
        if not mp.single:
            hooks.append(mp.parent.register_forward_pre_hook(cap.on_parent_call, with_kwargs=True))
    try:
        for args, kwargs in cache:
            layer(*args, **kwargs)
    finally:
        for hk in hooks:
            hk.remove()

    info: Dict[str, tuple] = {}
    n_skipped = 0
    for mp, cap in zip(mappings, caps):
        why = cap.skip_reason(mp)
        if why is not None:
            logger.warning(f"AWQ mapping {mp.smooth_name} -> {mp.balance_names} skipped: {why}; "
                           "its Linears are quantised without smoothing")
            n_skipped += 1
        else:
            scales, losses, best = _search(mp, cap, qargs, modifier.n_grid, modifier.duo_scaling)
            s = scales[best].contiguous()
            _apply(mp, s)
            for n in mp.balance_names:
                info[n] = (s, best, losses)
        cap.parent_calls.clear()
        cap.gram = None
    results: Dict[str, AWQResult] = {}
    for n, lin in linears.items():
        s, best, losses = info.get(n, (None, None, None))
        r = rtn_finalize(lin.weight.data, qargs, s, best, losses)
        lin.weight.data.copy_(r.dequantized(lin.weight.dtype))
        r.scaled_weight = None
        results[n] = r
    logger.info(f"AWQ {layer_name}: {len(mappings)} mappings ({n_skipped} skipped), {len(linears)} Linears quantised")
    return results
