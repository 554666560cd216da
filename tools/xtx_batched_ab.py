#!/usr/bin/env python3
"""In-process A/B of the batched Gram launch (qt_xtx_accumulate_batched) against the same problems as single launches
of qt_xtx_accumulate, one after the other on one stream.  The arms alternate pair by pair after a warm-up of every
shape; each timing is a pair of device events around work that ends in a synchronise.  Per case: the median and the
spread (min .. max) of each arm, the ratio of the medians, the batched plan (items, direct items, slab bytes) and the
largest |G_batched - G_single|_ij / sqrt(G_ii G_jj) over the lower triangle at the timed size (the Hessian bar: 1e-5).

usage: xtx_batched_ab.py [--pairs N] [--out FILE.json] [case ...]
cases: llama3_196608  3 x K = 4096 x 196 608 tokens (q/k/v, o and gate/up inputs of a Llama layer, full token count)
       llama3_65536   3 x K = 4096 x 65 536 tokens (what the staging buffer flushes)
       experts8       8 x K = 4096 x 49 152 +- 20 % tokens (Mixtral's experts)
       down8          8 x K = 14336 x ~36 000 tokens (for information: above one round of tiles per problem)"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from quantool_amd.hip import ops

dev = torch.device("cuda:0")
SPREAD8 = (0.8, 0.87, 0.93, 0.99, 1.04, 1.1, 1.15, 1.2)
CASES = {
    "llama3_196608": (4096, [196608] * 3),
    "llama3_65536": (4096, [65536] * 3),
    "experts8": (4096, [int(49152 * f) for f in SPREAD8]),
    "down8": (14336, [int(36000 * f) for f in SPREAD8]),
}


def inputs(n, K, seed):
    """N(0, 1) with 1 % of the channels x 10, as bench.py's activations"""
    g = torch.Generator(device=dev).manual_seed(seed)
    gain = torch.ones(K, device=dev)
    gain[torch.randperm(K, generator=g, device=dev)[:max(1, K // 100)]] = 10.0
    X = torch.empty((n, K), dtype=torch.bfloat16, device=dev)
    for t0 in range(0, n, 16384):
        t1 = min(n, t0 + 16384)
        X[t0:t1] = (torch.randn((t1 - t0, K), generator=g, device=dev) * gain).to(torch.bfloat16)
    return X


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_case(name, pairs):
    K, tokens = CASES[name]
    Xs = [inputs(n, K, seed=p) for p, n in enumerate(tokens)]
    Gb = [torch.zeros((K, K), device=dev) for _ in tokens]
    Gs = [torch.zeros((K, K), device=dev) for _ in tokens]

    def single():
        for X, G in zip(Xs, Gs):
            ops.xtx_accumulate(X, G)

    def batched():
        ops.xtx_accumulate_batched(Xs, Gb)

    # warm-up of both arms (also the outputs the accuracy figure is taken from: one launch into zeros each)
    single()
    batched()
    torch.cuda.synchronize()
    def rel(a, b, d):
        """max over the lower triangle of |a - b|_ij / (d_i d_j), in row blocks (fp64 temporaries)"""
        m = 0.0
        for r0 in range(0, K, 2048):
            diff = torch.tril((a[r0:r0 + 2048].double() - b[r0:r0 + 2048].double()), diagonal=r0).abs()
            m = max(m, float((diff / (d[r0:r0 + 2048, None] * d[None, :])).max()))
        return m

    worst = worst_b64 = worst_s64 = 0.0
    for X, a, b in zip(Xs, Gb, Gs):
        worst = max(worst, rel(a, b, torch.sqrt(torch.diagonal(b).double())))
        G64 = torch.zeros((K, K), dtype=torch.float64, device=dev)      # the fp64 Gram of the same rounded inputs
        for t0 in range(0, X.shape[0], 16384):
            x = X[t0:t0 + 16384].double()
            G64.addmm_(x.t(), x)
        d = torch.sqrt(torch.diagonal(G64))
        worst_b64, worst_s64 = max(worst_b64, rel(a, G64, d)), max(worst_s64, rel(b, G64, d))
        del G64, x
    res = {"single": [], "batched": []}
    for _ in range(pairs):
        res["single"].append(timed(single))
        res["batched"].append(timed(batched))
    items, n_slabs = ops.xtx_batched_plan(tokens, K)
    flop = 2.0 * sum(tokens) * K * (K + 256) / 2          # lower tiles incl. the diagonal ones, roughly
    out = {"case": name, "K": K, "tokens": tokens, "pairs": pairs, "items": len(items),
           "direct_items": sum(1 for it in items if it[5] < 0), "slab_bytes": n_slabs * 256 * 256 * 4,
           "max_rel_diff_vs_single": worst, "within_1e-5": worst <= 1e-5,
           "batched_max_rel_err_vs_f64": worst_b64, "single_max_rel_err_vs_f64": worst_s64}
    for arm, x in res.items():
        out[arm] = {"median_ms": statistics.median(x), "min_ms": min(x), "max_ms": max(x), "all_ms": x,
                    "tflops_at_median": flop / statistics.median(x) / 1e9}
    out["batched_over_single"] = out["batched"]["median_ms"] / out["single"]["median_ms"]
    for arm in ("single", "batched"):
        o = out[arm]
        print(f"{name:14s} {arm:8s} median {o['median_ms']:8.3f} ms  min {o['min_ms']:8.3f}  max {o['max_ms']:8.3f}  "
              f"n={pairs}  ~{o['tflops_at_median']:.0f} TFLOP/s", flush=True)
    print(f"{name:14s} batched / single = {out['batched_over_single']:.3f}; {out['items']} items, "
          f"{out['direct_items']} direct, {out['slab_bytes'] / 1e6:.0f} MB of slabs; max rel diff vs single "
          f"{worst:.2e}; vs the fp64 Gram: batched {worst_b64:.2e}, single {worst_s64:.2e}", flush=True)
    del Xs, Gb, Gs
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    assert args.pairs >= 5, "at least five pairs"
    results = [run_case(c, args.pairs) for c in (args.cases or list(CASES))]
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}, indent=1))
