"""The LM head and its cross-entropy, two ways, on one GPU: one JSON line.

Arm "logits" is ``nll_sum(F.linear(H, W), targets)``: what ``evaluate.perplexity`` runs behind the decoder by default
(a 16-bit GEMM that writes [M, V] logits, then log-softmax and gather over 1024 rows at a time).  Arm "fused" is
``ops.lm_head_nll(H, W, targets)`` and the fp64 sum of its ``nll``.  The arms alternate; each call is timed with HIP
events around the whole arm (both arms end in the host read of one fp64 scalar, inside the timed span), and the medians
over ``--repeats`` calls are reported with each arm's peak of allocated memory above the operands.

    python tools/lm_head_bench.py [--repeats 9] [--warmup 2] [--shapes 16384x4096x128256:bf16,...]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = "16384x4096x128256:bf16,3072x4096x128256:bf16,16384x4096x32000:bf16,8192x8192x128256:bf16,16384x4096x128256:fp16"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _arm_logits(H, W, tg):
    from quantool_amd.evaluate import nll_sum

    return nll_sum(F.linear(H, W), tg)


def _arm_fused(H, W, tg):
    from quantool_amd.hip import ops

    nll, _, _ = ops.lm_head_nll(H, W, tg)
    return float(nll.double().sum())


def _timed(fn, *a):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn(*a)                     # both arms end in a host read of one fp64 scalar
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def bench_shape(M, K, V, dtype, repeats, warmup, dev):
    g = torch.Generator(device=dev).manual_seed(M + K + V)
    H = torch.randn(M, K, generator=g, device=dev).to(dtype)
    W = (torch.randn(V, K, generator=g, device=dev) * (3.0 / K ** 0.5)).to(dtype)
    tg = torch.randint(0, V, (M,), generator=g, device=dev)
    arms = {"logits": _arm_logits, "fused": _arm_fused}
    times = {n: [] for n in arms}
    peak, value = {}, {}
    for it in range(warmup + repeats):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ms, out = _timed(fn, H, W, tg)
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
            value[name] = out
            if it >= warmup:
                times[name].append(ms)
    med = {n: statistics.median(t) for n, t in times.items()}
    flops = 2.0 * M * K * V
    return {"M": M, "K": K, "V": V, "dtype": str(dtype).replace("torch.", ""),
            "logits_ms": round(med["logits"], 3), "fused_ms": round(med["fused"], 3),
            "logits_ms_min_max": [round(min(times["logits"]), 3), round(max(times["logits"]), 3)],
            "fused_ms_min_max": [round(min(times["fused"]), 3), round(max(times["fused"]), 3)],
            "fused_over_logits": round(med["fused"] / med["logits"], 4),
            "fused_tflops": round(flops / med["fused"] / 1e9, 1), "logits_tflops": round(flops / med["logits"] / 1e9, 1),
            "logits_peak_bytes": int(peak["logits"]), "fused_peak_bytes": int(peak["fused"]),
            "mean_nll_logits": value["logits"] / M, "mean_nll_fused": value["fused"] / M}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=SHAPES, help="comma-separated MxKxV:dtype")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for spec in args.shapes.split(","):
        dims, dt = spec.split(":")
        M, K, V = (int(x) for x in dims.split("x"))
        rows.append(bench_shape(M, K, V, DTYPES[dt], args.repeats, args.warmup, dev))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "lm_head_bench", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
                      "warmup": args.warmup, "shapes": rows}))


if __name__ == "__main__":
    main()
