"""Routed-expert A8 / A16 paths vs separate per-expert launches vs transformers' bf16 loop at Mixtral-8x7B's shapes.

  python tools/moe_bench.py [--tokens 2048,8192] [--schemes W4A8,W8A8] [--reps 10] [--warmup 3]
  python tools/moe_bench.py --schemes W4A16,W4A16_ASYM,W8A16 --tokens 1,2,4,8,16,32,64,2048

One MoE layer (8 experts, top-2 with random routing, H = 4096, I = 14336).  Per scheme (W8A8 = int8 channel-wise
weights, symmetric activations; W4A8 = packed int4 g128 weights, asymmetric activations) and token count T: device
time (HIP events, mean over --reps after --warmup) of

  route        qt_moe_route
  gate_up      qt_gemm_i8_grouped, rows gathered by token       [R = 2T rows, N = 2I, K = H]
  down         qt_gemm_i8_grouped, contiguous rows               [R rows, N = H, K = I]
  combine      qt_moe_combine
  separate     the same two GEMMs as E qt_gemm_i8 launches each on the same rows (A pre-gathered per expert, not timed)
  experts      QuantizedExperts.forward end to end (route, both quantise passes, act_fn(gate) * up, GEMMs, combine)
  hf_bf16      transformers' MixtralExperts.forward in bf16

and grouped / separate (the GEMM pair; <= 1.1 is the issue's bar).

A16 schemes (W4A16 = packed int4 g128, W4A16_ASYM = the same with int8 zero-points, W8A16 = int8 channel-wise; the
weights of a ``WeightOnlyExperts``), every time from cold weights (each call reads the next of several copies of the bank,
> 1.4 GB apart, so the hit experts are not in the 256 MB MALL):

  gate_up, down  qt_gemm_wq_grouped (rows gathered by token / contiguous); grouped = the pair
  separate       the same pair as one qt_gemm_wq_skinny launch per 16 rows of each hit expert (rows pre-gathered)
  experts        WeightOnlyExperts.forward end to end (the grouped pair up to grouped_max_tokens, else dequantise)
  dequant        WeightOnlyExperts.forward on the dequantise path (both banks dequantised, then the bf16 loop)
  hf_bf16        transformers' MixtralExperts.forward in bf16

with grouped_tbs = bytes of the hit experts' weights, scales and zero-points / grouped time.  Prints one JSON line.

  python tools/moe_bench.py --decode-tokens 1,8,16,32,64,128 [--schemes W8A8,W4A8]

The A8 decode comparison: the GEMM pair (gate_up gathered by token, then down) as qt_gemm_i8_grouped and as
qt_gemm_i8_skinny_grouped on the same operands, alternating call by call in one loop, each pair between its own HIP
events, the two forms reading different copies of the bank in a rep (a bank is 0.7 / 1.4 GB, so every call reads its
hit experts cold).  Reported per form: median microseconds and the hit experts' weight + scale (+ wsum) bytes over it.

  python tools/moe_bench.py --ring-tokens 512,1024,2048,4096,8192,16384

The A8 prefill comparison, per scheme of --schemes (W8A8, W4A8): per product (gate_up gathered by token, down
contiguous) and per T, qt_gemm_i8_grouped and the scheme's ring form (W8A8: qt_gemm_i8_ring_grouped, W4A8:
qt_moe_gemm_i8_ring_w4) on the same operands, alternating call by call in one loop, each call between its own HIP
events: median / mean / min microseconds per form, ring speedup (tiled median / ring median), bits_equal.  Then
QuantizedExperts.forward end to end with the scheme's attribute (ring_min_rows_per_expert /
ring_w4_min_rows_per_expert) at 0 and at the class default (or at --ring-min-rows-per-expert /
--ring-w4-min-rows-per-expert), alternating likewise.

  python tools/moe_bench.py --wide-tokens 17,32,64,128,256,512,1024,2048,4096 [--schemes W8A8,W4A8]

The A8 batched-decode comparison, per scheme: per product and per T, qt_gemm_i8_grouped and qt_moe_gemm_i8_wide on the
same operands, alternating call by call in one loop, each call between its own HIP events: median / mean / min
microseconds per form, wide speedup (tiled median / wide median), bits_equal.  Then QuantizedExperts.forward end to end
with wide_max_rows_per_expert, wide_w4_max_rows_per_expert and wide_max_n all 0 and at the class defaults (or at
--wide-max-rows-per-expert / --wide-w4-max-rows-per-expert / --wide-max-n), alternating likewise.

  python tools/moe_bench.py --schemes W4A16,W4A16_ASYM,W8A16 --a16-wide-tokens 17,32,64,96,128,192,256,384,512,768,1024,2048

The A16 batched-decode comparison, per scheme and T: per product and as a pair, qt_gemm_wq_grouped and
qt_moe_gemm_wq_wide on the same operands, alternating call by call in one loop, each call between its own HIP events,
the two forms reading different copies of the bank in a rep and the copies rotating from rep to rep (cold weights, as
above): median / mean / min microseconds per form, wide speedup (grouped median / wide median), bits_equal_grouped.
Then WeightOnlyExperts.forward end to end on the path it had before the wide form (wide_min_tokens = wide_max_tokens =
0: the grouped pair up to grouped_max_tokens, the dequantise path above) against the new path (wide_min_tokens =
--a16-wide-min-tokens, wide_max_tokens = the largest T asked for), alternating likewise.

  python tools/moe_bench.py --fused-act [--tokens 1,16,32,128,512,2048,8192] [--schemes W8A8,W4A8]

The A8 glue comparison, per scheme and T: ``act_fn(gate) * up`` in torch followed by qt_quantize_tokens_i8 (three
launches) against qt_act_mul_quantize_i8 on the two halves of the same gate_up output, and QuantizedExperts.forward end
to end with ``fused_act`` off and on, alternating call by call in one loop, each call between its own HIP events.  The
unfused form runs twice in that loop ("unfused" and "unfused_again"): their ratio is the yardstick's own spread.  Both
comparisons assert bit equality before anything is timed.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantool_amd.engine.qlinear import QuantizedExperts, pack_int4  # noqa: E402
from quantool_amd.hip import ops  # noqa: E402

E, TOPK, H, I = 8, 2, 4096, 14336


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _experts(scheme, dev, g):
    from transformers.activations import ACT2FN

    int4 = scheme == "W4A8"
    lo, hi = (-8, 8) if int4 else (-128, 128)
    q_gu = torch.randint(lo, hi, (E, 2 * I, H), device=dev, generator=g, dtype=torch.int8)
    q_dn = torch.randint(lo, hi, (E, H, I), device=dev, generator=g, dtype=torch.int8)
    G1, G2 = (H // 128, I // 128) if int4 else (1, 1)
    s_gu = torch.rand(E, 2 * I, G1, device=dev, generator=g) * (1e-2 if int4 else 1e-3)
    s_dn = torch.rand(E, H, G2, device=dev, generator=g) * (1e-2 if int4 else 1e-3)
    if int4:
        q_gu = torch.stack([pack_int4(q_gu[e]) for e in range(E)])
        q_dn = torch.stack([pack_int4(q_dn[e]) for e in range(E)])
    return QuantizedExperts(H, I, q_gu, s_gu, q_dn, s_dn, ACT2FN["silu"], act_symmetric=not int4)


A16 = ("W4A16", "W4A16_ASYM", "W8A16")


def _time_i(fn, reps, warmup):
    """Mean device time of fn(i), i = the call's index (cold-weight rotation)."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _wo_experts(scheme, bank, dev, g):
    """A WeightOnlyExperts with random levels in ``scheme``'s format (``bank`` gives its shape and act_fn)."""
    from quantool_amd.engine.qlinear import WeightOnlyExperts

    int4 = scheme != "W8A16"
    parts = []
    for N, K in ((2 * I, H), (H, I)):
        if int4:
            w = torch.randint(-2 ** 31, 2 ** 31 - 1, (E, N, K // 8), device=dev, generator=g, dtype=torch.int32)
        else:
            w = torch.randint(-128, 128, (E, N, K), device=dev, generator=g, dtype=torch.int8)
        G = K // 128 if int4 else 1
        s = torch.rand(E, N, G, device=dev, generator=g) * (1e-2 if int4 else 1e-3)
        zp = torch.randint(-8, 8, (E, N, G), device=dev, generator=g, dtype=torch.int8) if scheme == "W4A16_ASYM" \
            else None
        parts.append((w, s, zp))
    (gw, gs, gz), (dw, ds, dz) = parts
    return WeightOnlyExperts(bank, gw, gs, dw, ds, gate_up_zero_point=gz, down_zero_point=dz)


def _bench_a16(scheme, T, x, idx, w, banks, hf, args):
    """One A16 row: the grouped pair, the separate launches, the module's two paths and the bf16 loop, cold."""
    n = len(banks)
    woe = banks[0]
    offsets, src_token, _, row_of = ops.moe_route(idx, E)
    off = offsets.cpu().tolist()
    src = src_token.long()
    gu = ops.gemm_wq_grouped(x, woe.gate_up, woe.gate_up_scale, offsets, row_idx=src_token, K=H,
                             zp_w=woe.gate_up_zero_point)
    gate, up = gu.chunk(2, dim=-1)
    h = woe.act_fn(gate) * up
    chunks = []                                     # (expert, gathered x rows, h rows), <= 16 rows each
    for e in range(E):
        for lo in range(off[e], off[e + 1], 16):
            hi = min(lo + 16, off[e + 1])
            chunks.append((e, x[src[lo:hi]].contiguous(), h[lo:hi]))

    def grouped(i):
        b = banks[i % n]
        ops.gemm_wq_grouped(x, b.gate_up, b.gate_up_scale, offsets, row_idx=src_token, K=H,
                            zp_w=b.gate_up_zero_point)
        ops.gemm_wq_grouped(h, b.down, b.down_scale, offsets, K=I, zp_w=b.down_zero_point)

    def separate(i):
        b = banks[i % n]
        zg, zd = b.gate_up_zero_point, b.down_zero_point
        for e, a, hr in chunks:
            ops.gemm_wq_skinny(a, b.gate_up[e], b.gate_up_scale[e], zp_w=None if zg is None else zg[e])
            ops.gemm_wq_skinny(hr, b.down[e], b.down_scale[e], zp_w=None if zd is None else zd[e])

    def dequant(i):
        b = banks[i % n]
        keep, b.grouped_max_tokens = b.grouped_max_tokens, 0
        b(x, idx, w)
        b.grouped_max_tokens = keep

    reps, warm = args.reps, args.warmup
    with torch.no_grad():
        t = {"gate_up": _time_i(lambda i: ops.gemm_wq_grouped(x, banks[i % n].gate_up, banks[i % n].gate_up_scale,
                                                              offsets, row_idx=src_token, K=H,
                                                              zp_w=banks[i % n].gate_up_zero_point), reps, warm),
             "down": _time_i(lambda i: ops.gemm_wq_grouped(h, banks[i % n].down, banks[i % n].down_scale, offsets,
                                                           K=I, zp_w=banks[i % n].down_zero_point), reps, warm),
             "grouped": _time_i(grouped, reps, warm),
             "separate": _time_i(separate, reps, warm),
             "experts": _time_i(lambda i: banks[i % n](x, idx, w), reps, warm),
             "dequant": _time_i(dequant, max(2, reps // 4), 1),
             "hf_bf16": _time(lambda: hf(x, idx, w), reps, warm)}
    hit = [e for e in range(E) if off[e + 1] > off[e]]
    per_expert = sum(getattr(woe, f"{p}{s}")[0].numel() * getattr(woe, f"{p}{s}").element_size()
                     for p in ("gate_up", "down") for s in ("", "_scale", "_zero_point")
                     if getattr(woe, f"{p}{s}") is not None)
    nbytes = per_expert * len(hit)
    return {"scheme": scheme, "T": T, "rows_per_expert": [off[e + 1] - off[e] for e in range(E)],
            "cold_copies": n, "ms": {k: round(v, 4) for k, v in t.items()},
            "hit_expert_bytes": nbytes, "grouped_tbs": round(nbytes / (t["grouped"] * 1e-3) / 1e12, 3),
            "gate_up_tbs": round(nbytes * 2 / 3 / (t["gate_up"] * 1e-3) / 1e12, 3),
            "down_tbs": round(nbytes / 3 / (t["down"] * 1e-3) / 1e12, 3),
            "grouped_over_separate": round(t["grouped"] / t["separate"], 3),
            "hf_bf16_over_experts": round(t["hf_bf16"] / t["experts"], 3),
            "dequant_over_experts": round(t["dequant"] / t["experts"], 3)}


def _bench_a8_decode(scheme, T, banks, dev, g, args):
    """One decode row: both grouped forms of the GEMM pair on the same routing and rows, cold banks."""
    from qlinear_bench import summarize, time_pair

    qe = banks[0]
    sym = qe.act_symmetric
    x = torch.randn(T, H, device=dev, generator=g).to(torch.bfloat16)
    logits = torch.randn(T, E, device=dev, generator=g)
    _, idx = torch.topk(torch.softmax(logits, -1), TOPK, dim=-1)
    offsets, src_token, _, _ = ops.moe_route(idx, E)
    Xq, s_x, zp_x = ops.quantize_tokens_i8(x, symmetric=sym)

    def pair(gemm, b, h=None):
        gu = gemm(Xq, s_x, b.gate_up, b.gate_up_scale, offsets, row_idx=src_token, K=H, zp_x=zp_x,
                  wsum=None if sym else b.gate_up_wsum)
        if h is None:
            gate, up = gu.chunk(2, dim=-1)
            return ops.quantize_tokens_i8(b.act_fn(gate) * up, symmetric=sym)
        return gemm(h[0], h[1], b.down, b.down_scale, offsets, K=I, zp_x=h[2], wsum=None if sym else b.down_wsum)

    with torch.no_grad():
        h = pair(ops.gemm_i8_grouped, qe)
        n = len(banks)
        t = time_pair({"tiled": lambda i: pair(ops.gemm_i8_grouped, banks[i % n], h),
                       "skinny": lambda i: pair(ops.gemm_i8_skinny_grouped, banks[(i + 1) % n], h)},
                      args.reps, args.warmup)
        same = torch.equal(pair(ops.gemm_i8_grouped, qe, h).view(torch.int16),
                           pair(ops.gemm_i8_skinny_grouped, qe, h).view(torch.int16))
    off = offsets.cpu().tolist()
    hit = [e for e in range(E) if off[e + 1] > off[e]]
    per_expert = sum(getattr(qe, f"{p}{sfx}")[0].numel() * getattr(qe, f"{p}{sfx}").element_size()
                     for p in ("gate_up", "down") for sfx in ("", "_scale") + (() if sym else ("_wsum",)))
    nbytes = per_expert * len(hit)
    row = {"scheme": scheme, "T": T, "rows_per_expert": [off[e + 1] - off[e] for e in range(E)], "bits_equal": same,
           "hit_expert_bytes": nbytes, "tiled": summarize(t["tiled"], nbytes), "skinny": summarize(t["skinny"], nbytes)}
    row["speedup"] = round(row["tiled"]["us"] / row["skinny"]["us"], 2)
    return row


def _us(times):
    t = sorted(times)
    return {"us": round(t[len(t) // 2] * 1e6, 2), "mean_us": round(sum(t) / len(t) * 1e6, 2),
            "min_us": round(t[0] * 1e6, 2)}


def _bench_a8_ring(scheme, T, qe, dev, g, args):
    """One prefill row: both grouped forms of each product on the same routing and rows, and the bank's forward."""
    from qlinear_bench import time_pair

    int4, sym = scheme == "W4A8", qe.act_symmetric
    ring = ops.moe_gemm_i8_ring_w4 if int4 else ops.gemm_i8_ring_grouped
    attr = "ring_w4_min_rows_per_expert" if int4 else "ring_min_rows_per_expert"
    x = torch.randn(T, H, device=dev, generator=g).to(torch.bfloat16)
    logits = torch.randn(T, E, device=dev, generator=g)
    w, idx = torch.topk(torch.softmax(logits, -1), TOPK, dim=-1)
    w = w / w.sum(-1, keepdim=True)
    offsets, src_token, _, _ = ops.moe_route(idx, E)
    off = offsets.cpu().tolist()
    Xq, s_x, zp_x = ops.quantize_tokens_i8(x, symmetric=sym)
    gu_ws, dn_ws = (None, None) if sym else (qe.gate_up_wsum, qe.down_wsum)
    row = {"scheme": scheme, "T": T, "rows_per_expert": [off[e + 1] - off[e] for e in range(E)],
           "R_over_E": T * TOPK / E}
    default = getattr(QuantizedExperts, attr)
    asked = args.ring_w4_min_rows_per_expert if int4 else args.ring_min_rows_per_expert
    ring_at = default if asked < 0 else asked
    with torch.no_grad():
        gu = ops.gemm_i8_grouped(Xq, s_x, qe.gate_up, qe.gate_up_scale, offsets, row_idx=src_token, K=H, zp_x=zp_x,
                                 wsum=gu_ws)
        gate, up = gu.chunk(2, dim=-1)
        hq, s_h, zp_h = ops.quantize_tokens_i8(qe.act_fn(gate) * up, symmetric=sym)
        del gu, gate, up
        products = {"gate_up": lambda fn: fn(Xq, s_x, qe.gate_up, qe.gate_up_scale, offsets, row_idx=src_token, K=H,
                                             zp_x=zp_x, wsum=gu_ws),
                    "down": lambda fn: fn(hq, s_h, qe.down, qe.down_scale, offsets, K=I, zp_x=zp_h, wsum=dn_ws)}
        for name, call in products.items():
            t = time_pair({"tiled": lambda i: call(ops.gemm_i8_grouped), "ring": lambda i: call(ring)},
                          args.reps, args.warmup)
            same = torch.equal(call(ops.gemm_i8_grouped).view(torch.int16), call(ring).view(torch.int16))
            row[name] = {"tiled": _us(t["tiled"]), "ring": _us(t["ring"]), "bits_equal": same}
            row[name]["speedup"] = round(row[name]["tiled"]["us"] / row[name]["ring"]["us"], 3)

        def bank(setting):
            def run(i):
                setattr(QuantizedExperts, attr, setting)
                return qe(x, idx, w)
            return run

        try:
            t = time_pair({"attr_0": bank(0), "attr_ring": bank(ring_at)}, args.reps, args.warmup)
            same = torch.equal(bank(0)(0).view(torch.int16), bank(ring_at)(0).view(torch.int16))
        finally:
            setattr(QuantizedExperts, attr, default)
    row["experts"] = {attr: ring_at, "on_ring": bool(0 < ring_at <= T * TOPK / E), "bits_equal": same,
                      "attr_0": _us(t["attr_0"]), "attr_ring": _us(t["attr_ring"])}
    row["experts"]["speedup"] = round(row["experts"]["attr_0"]["us"] / row["experts"]["attr_ring"]["us"], 3)
    return row


WIDE_ATTRS = ("wide_max_rows_per_expert", "wide_w4_max_rows_per_expert", "wide_max_n")


def _bench_a8_wide(scheme, T, qe, dev, g, args):
    """One batched-decode row: the tiled and the wide form of each product on the same routing and rows, and the
    bank's forward with the wide attributes at 0 and at the chosen values."""
    from qlinear_bench import time_pair

    int4, sym = scheme == "W4A8", qe.act_symmetric
    x = torch.randn(T, H, device=dev, generator=g).to(torch.bfloat16)
    logits = torch.randn(T, E, device=dev, generator=g)
    w, idx = torch.topk(torch.softmax(logits, -1), TOPK, dim=-1)
    w = w / w.sum(-1, keepdim=True)
    offsets, src_token, _, _ = ops.moe_route(idx, E)
    off = offsets.cpu().tolist()
    Xq, s_x, zp_x = ops.quantize_tokens_i8(x, symmetric=sym)
    gu_ws, dn_ws = (None, None) if sym else (qe.gate_up_wsum, qe.down_wsum)
    row = {"scheme": scheme, "T": T, "rows_per_expert": [off[e + 1] - off[e] for e in range(E)],
           "R_over_E": T * TOPK / E}
    defaults = {name: getattr(QuantizedExperts, name) for name in WIDE_ATTRS}
    chosen = {name: (defaults[name] if getattr(args, name) < 0 else getattr(args, name)) for name in WIDE_ATTRS}
    with torch.no_grad():
        gu = ops.gemm_i8_grouped(Xq, s_x, qe.gate_up, qe.gate_up_scale, offsets, row_idx=src_token, K=H, zp_x=zp_x,
                                 wsum=gu_ws)
        gate, up = gu.chunk(2, dim=-1)
        hq, s_h, zp_h = ops.quantize_tokens_i8(qe.act_fn(gate) * up, symmetric=sym)
        del gu, gate, up
        products = {"gate_up": lambda fn: fn(Xq, s_x, qe.gate_up, qe.gate_up_scale, offsets, row_idx=src_token, K=H,
                                             zp_x=zp_x, wsum=gu_ws),
                    "down": lambda fn: fn(hq, s_h, qe.down, qe.down_scale, offsets, K=I, zp_x=zp_h, wsum=dn_ws)}
        for name, call in products.items():
            t = time_pair({"tiled": lambda i: call(ops.gemm_i8_grouped), "wide": lambda i: call(ops.moe_gemm_i8_wide)},
                          args.reps, args.warmup)
            same = torch.equal(call(ops.gemm_i8_grouped).view(torch.int16),
                               call(ops.moe_gemm_i8_wide).view(torch.int16))
            row[name] = {"tiled": _us(t["tiled"]), "wide": _us(t["wide"]), "bits_equal": same}
            row[name]["speedup"] = round(row[name]["tiled"]["us"] / row[name]["wide"]["us"], 3)

        def bank(settings):
            def run(i):
                for attr, value in settings.items():
                    setattr(QuantizedExperts, attr, value)
                return qe(x, idx, w)
            return run

        try:
            zero = {name: 0 for name in WIDE_ATTRS}
            t = time_pair({"attr_0": bank(zero), "attr_wide": bank(chosen)}, args.reps, args.warmup)
            same = torch.equal(bank(zero)(0).view(torch.int16), bank(chosen)(0).view(torch.int16))
        finally:
            for attr, value in defaults.items():
                setattr(QuantizedExperts, attr, value)
    at = chosen["wide_w4_max_rows_per_expert" if int4 else "wide_max_rows_per_expert"]
    row["experts"] = {**chosen, "on_wide": bool(T > QuantizedExperts.grouped_max_tokens and T * TOPK / E <= at),
                      "bits_equal": same, "attr_0": _us(t["attr_0"]), "attr_wide": _us(t["attr_wide"])}
    row["experts"]["speedup"] = round(row["experts"]["attr_0"]["us"] / row["experts"]["attr_wide"]["us"], 3)
    return row


def _bench_a8_fused(scheme, T, qe, dev, g, args):
    """One glue row: the three passes between the bank's products against the fused pass on the same gate_up output,
    and the bank's forward with ``fused_act`` off and on."""
    from qlinear_bench import time_pair

    sym = qe.act_symmetric
    x = torch.randn(T, H, device=dev, generator=g).to(torch.bfloat16)
    logits = torch.randn(T, E, device=dev, generator=g)
    w, idx = torch.topk(torch.softmax(logits, -1), TOPK, dim=-1)
    w = w / w.sum(-1, keepdim=True)
    offsets, src_token, _, _ = ops.moe_route(idx, E)
    row = {"scheme": scheme, "T": T, "R": T * TOPK}

    def unfused(Y):
        gate, up = Y.chunk(2, dim=-1)
        return ops.quantize_tokens_i8(qe.act_fn(gate) * up, symmetric=sym)

    def fused(Y):
        return ops.act_mul_quantize_i8(Y[:, :I], Y[:, I:], symmetric=sym)

    def bank(on):
        def run(i):
            qe.fused_act = on
            return qe(x, idx, w)
        return run

    def ratios(t):
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        return {**{k: _us(v) for k, v in t.items()}, "speedup": round(med["unfused"] / med["fused"], 3),
                "unfused_spread": round(abs(med["unfused"] / med["unfused_again"] - 1.0), 4)}

    with torch.no_grad():
        Y = qe._product("gate_up", x, offsets, src_token, T)
        for a, b in zip(unfused(Y), fused(Y)):
            assert (a is None and b is None) or torch.equal(a, b), "the fused pass differs from the three passes"
        try:
            assert torch.equal(bank(False)(0).view(torch.int16), bank(True)(0).view(torch.int16)), \
                "the bank's output differs with fused_act"
            row["bits_equal"] = True
            row["glue"] = ratios(time_pair({"unfused": lambda i: unfused(Y), "fused": lambda i: fused(Y),
                                            "unfused_again": lambda i: unfused(Y)}, args.reps, args.warmup))
            del Y
            row["experts"] = ratios(time_pair({"unfused": bank(False), "fused": bank(True),
                                               "unfused_again": bank(False)}, args.reps, args.warmup))
        finally:
            qe.fused_act = False
    return row


def _bench_a16_wide(scheme, T, banks, dev, g, args, wide_max):
    """One A16 batched-decode row: the grouped and the wide form of each product and of the pair on the same routing
    and rows, and the bank's forward on the old and on the new path, cold weights."""
    from qlinear_bench import time_pair

    n = len(banks)
    x = torch.randn(T, H, device=dev, generator=g).to(torch.bfloat16)
    logits = torch.randn(T, E, device=dev, generator=g)
    w, idx = torch.topk(torch.softmax(logits, -1), TOPK, dim=-1)
    w = (w / w.sum(-1, keepdim=True)).to(torch.bfloat16)
    offsets, src_token, _, _ = ops.moe_route(idx, E)
    off = offsets.cpu().tolist()
    R = T * TOPK
    row = {"scheme": scheme, "T": T, "rows_per_expert": [off[e + 1] - off[e] for e in range(E)], "R_over_E": R / E,
           "m_tiles": ops.moe_wq_wide_mtiles(R, E), "cold_copies": n}
    with torch.no_grad():
        b0 = banks[0]
        gu = ops.gemm_wq_grouped(x, b0.gate_up, b0.gate_up_scale, offsets, row_idx=src_token, K=H,
                                 zp_w=b0.gate_up_zero_point)
        gate, up = gu.chunk(2, dim=-1)
        h = b0.act_fn(gate) * up
        del gu, gate, up

        def gate_up(fn, b):
            return fn(x, b.gate_up, b.gate_up_scale, offsets, row_idx=src_token, K=H, zp_w=b.gate_up_zero_point)

        def down(fn, b):
            return fn(h, b.down, b.down_scale, offsets, K=I, zp_w=b.down_zero_point)

        def pair(fn, b):
            gate_up(fn, b)
            return down(fn, b)

        for name, call in (("gate_up", gate_up), ("down", down), ("pair", pair)):
            t = time_pair({"grouped": lambda i: call(ops.gemm_wq_grouped, banks[i % n]),
                           "wide": lambda i: call(ops.moe_gemm_wq_wide, banks[(i + 1) % n])}, args.reps, args.warmup)
            row[name] = {"grouped": _us(t["grouped"]), "wide": _us(t["wide"])}
            if name != "pair":
                row[name]["bits_equal_grouped"] = torch.equal(call(ops.gemm_wq_grouped, b0).view(torch.int16),
                                                              call(ops.moe_gemm_wq_wide, b0).view(torch.int16))
            row[name]["speedup"] = round(row[name]["grouped"]["us"] / row[name]["wide"]["us"], 3)

        def bank(wide_min_tokens, wide_max_tokens, shift):
            def run(i):
                b = banks[(i + shift) % n]
                b.wide_min_tokens, b.wide_max_tokens = wide_min_tokens, wide_max_tokens
                return b(x, idx, w)
            return run

        keep = [(b.wide_min_tokens, b.wide_max_tokens) for b in banks]
        try:
            reps = args.reps if T <= b0.grouped_max_tokens else max(3, args.reps // 2)
            t = time_pair({"before": bank(0, 0, 0), "wide": bank(args.a16_wide_min_tokens, wide_max, 1)}, reps,
                          min(args.warmup, 2))
            y0, y1 = bank(0, 0, 0)(0), bank(args.a16_wide_min_tokens, wide_max, 0)(0)
        finally:
            for b, (lo, hi) in zip(banks, keep):
                b.wide_min_tokens, b.wide_max_tokens = lo, hi
    row["experts"] = {"wide_min_tokens": args.a16_wide_min_tokens, "wide_max_tokens": wide_max,
                      "before_path": "grouped" if T <= b0.grouped_max_tokens else "dequantise",
                      "bits_equal": torch.equal(y0.view(torch.int16), y1.view(torch.int16)),
                      "max_abs_diff": float((y0.float() - y1.float()).abs().max()),
                      "before": _us(t["before"]), "wide": _us(t["wide"])}
    row["experts"]["speedup"] = round(row["experts"]["before"]["us"] / row["experts"]["wide"]["us"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="2048,8192")
    ap.add_argument("--decode-tokens", default="",
                    help="A8 schemes: compare the two grouped GEMM forms at these token counts instead")
    ap.add_argument("--ring-tokens", default="",
                    help="W8A8 / W4A8: compare qt_gemm_i8_grouped and the scheme's ring form at these token counts "
                         "instead")
    ap.add_argument("--ring-min-rows-per-expert", type=int, default=-1,
                    help="with --ring-tokens, W8A8: the attribute of the bank's second timing (default: the class's)")
    ap.add_argument("--ring-w4-min-rows-per-expert", type=int, default=-1,
                    help="with --ring-tokens, W4A8: the attribute of the bank's second timing (default: the class's)")
    ap.add_argument("--wide-tokens", default="",
                    help="W8A8 / W4A8: compare qt_gemm_i8_grouped and qt_moe_gemm_i8_wide at these token counts instead")
    for name in WIDE_ATTRS:
        ap.add_argument("--" + name.replace("_", "-"), type=int, default=-1,
                        help=f"with --wide-tokens: QuantizedExperts.{name} of the bank's second timing (default: the "
                             "class's)")
    ap.add_argument("--a16-wide-tokens", default="",
                    help="W4A16 / W4A16_ASYM / W8A16: compare qt_gemm_wq_grouped and qt_moe_gemm_wq_wide at these token "
                         "counts instead")
    ap.add_argument("--a16-wide-min-tokens", type=int, default=1,
                    help="with --a16-wide-tokens: WeightOnlyExperts.wide_min_tokens of the bank's second timing")
    ap.add_argument("--fused-act", action="store_true",
                    help="W8A8 / W4A8: compare the three glue passes and qt_act_mul_quantize_i8, and the bank's forward "
                         "with fused_act off and on, at --tokens (default then: 1,16,32,128,512,2048,8192)")
    ap.add_argument("--schemes", default="W4A8,W8A8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench needs a GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []

    if args.a16_wide_tokens:
        from transformers import MixtralConfig
        from transformers.models.mixtral.modeling_mixtral import MixtralExperts

        cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E, num_experts_per_tok=TOPK)
        tokens = [int(t) for t in args.a16_wide_tokens.split(",")]
        for scheme in args.schemes.split(","):
            if scheme not in A16:
                raise SystemExit("--a16-wide-tokens compares the A16 grouped GEMMs (W4A16 / W4A16_ASYM / W8A16)")
            n = 3 if scheme != "W8A16" else 2       # > 1.4 GB of bank copies in all, as the A16 rows above
            with torch.device("meta"):
                shells = [MixtralExperts(cfg) for _ in range(n)]
            banks = [_wo_experts(scheme, b, dev, g) for b in shells]
            for T in tokens:
                row = _bench_a16_wide(scheme, T, banks, dev, g, args, max(tokens))
                rows.append(row)
                print(json.dumps(row), file=sys.stderr)
                torch.cuda.empty_cache()
            del banks
            torch.cuda.empty_cache()
        print(json.dumps({"metric": "Mixtral-8x7B MoE layer, A16 batched decode: qt_gemm_wq_grouped vs "
                                    "qt_moe_gemm_wq_wide",
                          "schemes": args.schemes, "E": E, "top_k": TOPK, "H": H, "I": I,
                          "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}))
        return

    if args.fused_act:
        tokens = args.tokens if args.tokens != ap.get_default("tokens") else "1,16,32,128,512,2048,8192"
        for scheme in args.schemes.split(","):
            if scheme not in ("W8A8", "W4A8"):
                raise SystemExit("--fused-act compares the A8 banks' glue (W8A8 / W4A8)")
            qe = _experts(scheme, dev, g)
            for T in (int(t) for t in tokens.split(",")):
                row = _bench_a8_fused(scheme, T, qe, dev, g, args)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr)
                torch.cuda.empty_cache()
            del qe
            torch.cuda.empty_cache()
        print(json.dumps({"metric": "Mixtral-8x7B MoE layer, A8 glue: silu * up + qt_quantize_tokens_i8 vs "
                                    "qt_act_mul_quantize_i8",
                          "schemes": args.schemes, "E": E, "top_k": TOPK, "H": H, "I": I,
                          "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}))
        return

    if args.wide_tokens:
        for scheme in args.schemes.split(","):
            if scheme not in ("W8A8", "W4A8"):
                raise SystemExit("--wide-tokens compares the A8 grouped GEMMs (W8A8 / W4A8)")
            qe = _experts(scheme, dev, g)
            for T in (int(t) for t in args.wide_tokens.split(",")):
                row = _bench_a8_wide(scheme, T, qe, dev, g, args)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr)
                torch.cuda.empty_cache()
            del qe
            torch.cuda.empty_cache()
        print(json.dumps({"metric": "Mixtral-8x7B MoE layer, A8 batched decode: qt_gemm_i8_grouped vs qt_moe_gemm_i8_wide",
                          "schemes": args.schemes, "E": E, "top_k": TOPK, "H": H, "I": I,
                          "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}))
        return

    if args.ring_tokens:
        for scheme in args.schemes.split(","):
            if scheme not in ("W8A8", "W4A8"):
                raise SystemExit("--ring-tokens compares the A8 grouped GEMMs (W8A8 / W4A8)")
            qe = _experts(scheme, dev, g)
            for T in (int(t) for t in args.ring_tokens.split(",")):
                row = _bench_a8_ring(scheme, T, qe, dev, g, args)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr)
                torch.cuda.empty_cache()
            del qe
            torch.cuda.empty_cache()
        print(json.dumps({"metric": "Mixtral-8x7B MoE layer, A8 prefill: qt_gemm_i8_grouped vs "
                                    "qt_gemm_i8_ring_grouped (W8A8) / qt_moe_gemm_i8_ring_w4 (W4A8)",
                          "schemes": args.schemes, "E": E, "top_k": TOPK, "H": H, "I": I,
                          "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}))
        return

    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    hf = MixtralExperts(MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E,
                                      num_experts_per_tok=TOPK)).to(dev).to(torch.bfloat16)
    with torch.no_grad():
        hf.gate_up_proj.normal_(0, 0.02, generator=g)
        hf.down_proj.normal_(0, 0.02, generator=g)
    if args.decode_tokens:
        for scheme in args.schemes.split(","):
            if scheme in A16:
                raise SystemExit("--decode-tokens compares the A8 grouped GEMMs (W8A8 / W4A8)")
            banks = [_experts(scheme, dev, g) for _ in range(2)]
            for T in (int(t) for t in args.decode_tokens.split(",")):
                row = _bench_a8_decode(scheme, T, banks, dev, g, args)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr)
            del banks
            torch.cuda.empty_cache()
        print(json.dumps({"metric": "Mixtral-8x7B MoE layer, A8 decode: qt_gemm_i8_grouped vs qt_gemm_i8_skinny_grouped",
                          "E": E, "top_k": TOPK, "H": H, "I": I, "device": torch.cuda.get_device_name(0),
                          "rows": rows}))
        return
    for scheme in args.schemes.split(","):
        if scheme in A16:
            # copies of the bank > 1.4 GB in all, rotated per call (the int4 bank is 0.7 GB, the int8 one 1.4 GB)
            n = 3 if scheme != "W8A16" else 2
            with torch.device("meta"):          # the bank's shape and act_fn only: no dense weights anywhere
                shells = [MixtralExperts(hf.config) for _ in range(n)]
            banks = [_wo_experts(scheme, b, dev, g) for b in shells]
            for T in (int(t) for t in args.tokens.split(",")):
                x = torch.randn(T, H, device=dev, generator=g).to(torch.bfloat16)
                logits = torch.randn(T, E, device=dev, generator=g)
                w, idx = torch.topk(torch.softmax(logits, -1), TOPK, dim=-1)
                w = (w / w.sum(-1, keepdim=True)).to(torch.bfloat16)
                row = _bench_a16(scheme, T, x, idx, w, banks, hf, args)
                rows.append(row)
                print(json.dumps(row), file=sys.stderr)
                torch.cuda.empty_cache()
            del banks
            torch.cuda.empty_cache()
            continue
        qe = _experts(scheme, dev, g)
        sym = qe.act_symmetric
        for T in (int(t) for t in args.tokens.split(",")):
            x = torch.randn(T, H, device=dev, generator=g).to(torch.bfloat16)
            logits = torch.randn(T, E, device=dev, generator=g)
            w, idx = torch.topk(torch.softmax(logits, -1), TOPK, dim=-1)
            w = w / w.sum(-1, keepdim=True)
            offsets, src_token, _, row_of = ops.moe_route(idx, E)
            Xq, s_x, zp_x = ops.quantize_tokens_i8(x, symmetric=sym)
            gu_ws, dn_ws = (None, None) if sym else (qe.gate_up_wsum, qe.down_wsum)
            gu = ops.gemm_i8_grouped(Xq, s_x, qe.gate_up, qe.gate_up_scale, offsets, row_idx=src_token, K=H,
                                     zp_x=zp_x, wsum=gu_ws)
            gate, up = gu.chunk(2, dim=-1)
            hq, s_h, zp_h = ops.quantize_tokens_i8(qe.act_fn(gate) * up, symmetric=sym)
            y = ops.gemm_i8_grouped(hq, s_h, qe.down, qe.down_scale, offsets, K=I, zp_x=zp_h, wsum=dn_ws)
            # the separate launches' inputs: each expert's rows, gathered once (untimed)
            off = offsets.cpu().tolist()
            src = src_token.long()
            per = []
            for e in range(E):
                lo, hi = off[e], off[e + 1]
                if hi == lo:
                    continue
                r = src[lo:hi]
                per.append((e, Xq[r].contiguous(), s_x[r].contiguous(), None if sym else zp_x[r].contiguous(),
                            hq[lo:hi], s_h[lo:hi], None if sym else zp_h[lo:hi]))

            def separate():
                for e, a, sa, za, b, sb, zb in per:
                    ops.gemm_i8(a, sa, qe.gate_up[e], qe.gate_up_scale[e], K=H, zp_x=za,
                                wsum=None if sym else qe.gate_up_wsum[e])
                    ops.gemm_i8(b, sb, qe.down[e], qe.down_scale[e], K=I, zp_x=zb,
                                wsum=None if sym else qe.down_wsum[e])

            with torch.no_grad():
                t = {
                    "route": _time(lambda: ops.moe_route(idx, E), args.reps, args.warmup),
                    "gate_up": _time(lambda: ops.gemm_i8_grouped(Xq, s_x, qe.gate_up, qe.gate_up_scale, offsets,
                                                                 row_idx=src_token, K=H, zp_x=zp_x, wsum=gu_ws),
                                     args.reps, args.warmup),
                    "down": _time(lambda: ops.gemm_i8_grouped(hq, s_h, qe.down, qe.down_scale, offsets, K=I,
                                                              zp_x=zp_h, wsum=dn_ws), args.reps, args.warmup),
                    "combine": _time(lambda: ops.moe_combine(y, row_of, w), args.reps, args.warmup),
                    "separate": _time(separate, args.reps, args.warmup),
                    "experts": _time(lambda: qe(x, idx, w), args.reps, args.warmup),
                    "hf_bf16": _time(lambda: hf(x, idx, w), args.reps, args.warmup),
                }
            R = T * TOPK
            ops_n = 2.0 * R * (2 * I) * H + 2.0 * R * H * I
            row = {"scheme": scheme, "T": T, "rows_per_expert": [off[e + 1] - off[e] for e in range(E)],
                   "ms": {k: round(v, 4) for k, v in t.items()},
                   "grouped_over_separate": round((t["gate_up"] + t["down"]) / t["separate"], 3),
                   "gemm_tops": round(ops_n / ((t["gate_up"] + t["down"]) * 1e-3) / 1e12, 1),
                   "hf_bf16_over_experts": round(t["hf_bf16"] / t["experts"], 3)}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
            del x, Xq, hq, gu, y, per
            torch.cuda.empty_cache()
        del qe
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "Mixtral-8x7B MoE layer: grouped expert GEMM / GEMV vs E launches vs bf16 loop",
                      "E": E, "top_k": TOPK, "H": H, "I": I, "rows": rows}))


if __name__ == "__main__":
    main()
