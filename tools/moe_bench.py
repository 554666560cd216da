"""Routed-expert A8 path vs separate per-expert GEMMs vs transformers' bf16 loop at Mixtral-8x7B's shapes.

  python tools/moe_bench.py [--tokens 2048,8192] [--schemes W4A8,W8A8] [--reps 10] [--warmup 3]

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

and grouped / separate (the GEMM pair; <= 1.1 is the issue's bar).  Prints one JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="2048,8192")
    ap.add_argument("--schemes", default="W4A8,W8A8")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench needs a GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []

    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralExperts

    hf = MixtralExperts(MixtralConfig(hidden_size=H, intermediate_size=I, num_local_experts=E,
                                      num_experts_per_tok=TOPK)).to(dev).to(torch.bfloat16)
    with torch.no_grad():
        hf.gate_up_proj.normal_(0, 0.02, generator=g)
        hf.down_proj.normal_(0, 0.02, generator=g)
    for scheme in args.schemes.split(","):
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
    print(json.dumps({"metric": "Mixtral-8x7B MoE layer: grouped int8 expert GEMM vs E launches vs bf16 loop",
                      "E": E, "top_k": TOPK, "H": H, "I": I, "rows": rows}))


if __name__ == "__main__":
    main()
