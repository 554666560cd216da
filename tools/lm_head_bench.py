"""The LM head and its cross-entropy, two ways, on one GPU: one JSON line.

Arm "logits" is ``nll_sum(F.linear(H, W), targets)``: what ``evaluate.perplexity`` runs behind the decoder by default
(a 16-bit GEMM that writes [M, V] logits, then log-softmax and gather over 1024 rows at a time).  Arm "fused" is
``ops.lm_head_nll(H, W, targets)`` and the fp64 sum of its ``nll``.  The arms alternate; each call is timed with HIP
events around the whole arm (both arms end in the host read of one fp64 scalar, inside the timed span), and the medians
over ``--repeats`` calls are reported with each arm's peak of allocated memory above the operands.

    python tools/lm_head_bench.py [--repeats 9] [--warmup 2] [--shapes 16384x4096x128256:bf16,...]

``--kl`` times the distance of two models that share the head instead, three arms interleaved: "logits" (two
``F.linear`` and an fp32 log-softmax KL over 1024 rows at a time: what a user writes without the kernel), "two_nll" (two
``ops.lm_head_nll`` launches: the price of the two perplexities alone, the same flops and W traffic per row) and "fused"
(``ops.lm_head_kl``).  Hq is the 16-bit rounding of Hp + 0.05 N(0, 1), the small KL of a real checkpoint.  Every arm
ends in the host read of its fp64 sums.
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


def _kl_arm_logits(Hp, Hq, W, tg, chunk_rows=1024):
    a, b = F.linear(Hp, W), F.linear(Hq, W)
    tot = torch.zeros(3, dtype=torch.float64, device=a.device)          # kl, nll_p, nll_q
    for r0 in range(0, a.shape[0], chunk_rows):
        lp = torch.log_softmax(a[r0:r0 + chunk_rows].float(), dim=-1)
        lq = torch.log_softmax(b[r0:r0 + chunk_rows].float(), dim=-1)
        t = tg[r0:r0 + chunk_rows].unsqueeze(1)
        tot += torch.stack([(lp.exp() * (lp - lq)).sum(-1).double().sum(), -lp.gather(1, t).double().sum(),
                            -lq.gather(1, t).double().sum()])
    return tot.tolist()


def _kl_arm_two_nll(Hp, Hq, W, tg):
    from quantool_amd.hip import ops

    np_, _, _ = ops.lm_head_nll(Hp, W, tg)
    nq, _, _ = ops.lm_head_nll(Hq, W, tg)
    return torch.stack([np_.double().sum() * 0, np_.double().sum(), nq.double().sum()]).tolist()


def _kl_arm_fused(Hp, Hq, W, tg):
    from quantool_amd.hip import ops

    r = ops.lm_head_kl(Hp, Hq, W, tg)
    return torch.stack([r.kl.double().sum(), r.nll_p.double().sum(), r.nll_q.double().sum()]).tolist()


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


def bench_kl_shape(M, K, V, dtype, repeats, warmup, dev):
    g = torch.Generator(device=dev).manual_seed(M + K + V)
    Hp = torch.randn(M, K, generator=g, device=dev).to(dtype)
    W = (torch.randn(V, K, generator=g, device=dev) * (3.0 / K ** 0.5)).to(dtype)
    Hq = (Hp.float() + 0.05 * torch.randn(M, K, generator=g, device=dev)).to(dtype)
    tg = torch.randint(0, V, (M,), generator=g, device=dev)
    arms = {"logits": _kl_arm_logits, "two_nll": _kl_arm_two_nll, "fused": _kl_arm_fused}
    times = {n: [] for n in arms}
    peak, value = {}, {}
    for it in range(warmup + repeats):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ms, out = _timed(fn, Hp, Hq, W, tg)
            peak[name] = max(peak.get(name, 0), torch.cuda.max_memory_allocated() - base)
            value[name] = out
            if it >= warmup:
                times[name].append(ms)
    med = {n: statistics.median(t) for n, t in times.items()}
    row = {"M": M, "K": K, "V": V, "dtype": str(dtype).replace("torch.", "")}
    for n in arms:
        row[n + "_ms"] = round(med[n], 3)
        row[n + "_ms_min_max"] = [round(min(times[n]), 3), round(max(times[n]), 3)]
        row[n + "_peak_bytes"] = int(peak[n])
    row.update({"fused_over_two_nll": round(med["fused"] / med["two_nll"], 4),
                "fused_over_logits": round(med["fused"] / med["logits"], 4),
                "fused_tflops": round(4.0 * M * K * V / med["fused"] / 1e9, 1),
                "mean_kl_logits": value["logits"][0] / M, "mean_kl_fused": value["fused"][0] / M,
                "mean_nll_p": {n: value[n][1] / M for n in arms}, "mean_nll_q": {n: value[n][2] / M for n in arms}})
    return row


KL_SHAPES = "16384x4096x128256:bf16,3072x4096x128256:bf16,16384x4096x128256:fp16"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=None, help="comma-separated MxKxV:dtype")
    ap.add_argument("--kl", action="store_true",
                    help="time ops.lm_head_kl against two logit matrices and against two NLL launches")
    args = ap.parse_args()
    bench = bench_kl_shape if args.kl else bench_shape
    dev = torch.device("cuda:0")
    rows = []
    for spec in (args.shapes or (KL_SHAPES if args.kl else SHAPES)).split(","):
        dims, dt = spec.split(":")
        M, K, V = (int(x) for x in dims.split("x"))
        rows.append(bench(M, K, V, DTYPES[dt], args.repeats, args.warmup, dev))
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "lm_head_bench", "mode": "kl" if args.kl else "nll",
                      "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
                      "shapes": rows}))


if __name__ == "__main__":
    main()
