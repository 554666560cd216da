#!/usr/bin/env python3
"""In-process A/B of the bound on fp32 chains inside a Gram launch (chain_tokens): per shape, in alternating
arms after a warm-up of every arm,
    plain        one launch, one fp32 chain per direct tile element over all tokens
    chain_F      the same launch with chain_tokens = F, F in 15 360, 30 720, 61 440
    split_F      launches of at most F tokens, one after the other (what QT_XTX_LAUNCH_TOKENS=F does)
Each timing is a pair of device events around work that ends in a synchronise; the order of the arms changes from round
to round.  Per arm: the median and the spread of
the times, the ratio to the plain arm's median, and the largest |G - G64|_ij / sqrt(G64_ii G64_jj) over the lower
triangle, G64 the torch-fp64 Gram of the same rounded inputs formed in row chunks.  Data: N(0, 1) bf16 with 1 % of the
channels x 10, as bench.py's activations.

usage: xtx_chain_ab.py [--rounds N] [--out FILE.json] [case ...]
cases: k4096      K = 4096  x 196 608 tokens
       k14336     K = 14336 x 196 608 tokens
       b3x65536   batched, 3 x K = 4096 x 65 536 tokens   (split arm: each problem's slices as single launches)
       b3x196608  batched, 3 x K = 4096 x 196 608 tokens"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from quantool_amd.hip import ops

dev = torch.device("cuda:0")
BOUNDS = (15360, 30720, 61440)
CASES = {
    "k4096": (4096, [196608], False),
    "k14336": (14336, [196608], False),
    "b3x65536": (4096, [65536] * 3, True),
    "b3x196608": (4096, [196608] * 3, True),
}


def inputs(n, K, seed):
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


def gram64(X):
    K = X.shape[1]
    G64 = torch.zeros((K, K), dtype=torch.float64, device=dev)
    for t0 in range(0, X.shape[0], 8192):
        x = X[t0:t0 + 8192].double()
        G64.addmm_(x.t(), x)
    return G64


def rel_err(G, G64):
    """max over the lower triangle of |G - G64|_ij / sqrt(G64_ii G64_jj), in row blocks"""
    K = G.shape[0]
    d = torch.sqrt(torch.diagonal(G64))
    worst = 0.0
    for r0 in range(0, K, 2048):
        diff = torch.tril(G[r0:r0 + 2048].double() - G64[r0:r0 + 2048], diagonal=r0).abs()
        worst = max(worst, float((diff / (d[r0:r0 + 2048, None] * d[None, :])).max()))
    return worst


def run_case(name, rounds):
    K, tokens, batched = CASES[name]
    Xs = [inputs(n, K, seed=p) for p, n in enumerate(tokens)]
    Gs = [torch.zeros((K, K), device=dev) for _ in tokens]

    def launch(chain):
        if batched:
            return lambda: ops.xtx_accumulate_batched(Xs, Gs, chain_tokens=chain)
        return lambda: ops.xtx_accumulate(Xs[0], Gs[0], chain_tokens=chain)

    def split(limit):
        def fn():
            for X, G in zip(Xs, Gs):
                for t0 in range(0, X.shape[0], limit):
                    ops.xtx_accumulate(X[t0:t0 + limit], G)
        return fn

    arms = {"plain": launch(0)}
    for F in BOUNDS:
        arms[f"chain_{F}"] = launch(F)
    for F in BOUNDS:
        arms[f"split_{F}"] = split(F)

    # warm-up of every arm into zeros: also the outputs the precision figure is taken from
    G64s = [gram64(X) for X in Xs]
    err = {}
    for arm, fn in arms.items():
        for G in Gs:
            G.zero_()
        fn()
        torch.cuda.synchronize()
        err[arm] = max(rel_err(G, G64) for G, G64 in zip(Gs, G64s))
    del G64s
    torch.cuda.empty_cache()
    times = {arm: [] for arm in arms}
    # the chip is power-limited in this kernel, so an arm is faster behind a light arm than behind a heavy one: every
    # round starts at another arm and every second round walks the arms backwards
    names = list(arms)
    for r in range(rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        for arm in (order[::-1] if r % 2 else order):
            times[arm].append(timed(arms[arm]))
    base = statistics.median(times["plain"])
    out = {"case": name, "K": K, "tokens": tokens, "batched": batched, "rounds": rounds, "arms": {}}
    for arm, x in times.items():
        med = statistics.median(x)
        out["arms"][arm] = {"median_ms": med, "min_ms": min(x), "max_ms": max(x), "all_ms": x,
                            "over_plain": med / base, "max_rel_err_vs_f64": err[arm]}
        print(f"{name:10s} {arm:12s} median {med:9.3f} ms  min {min(x):9.3f}  max {max(x):9.3f}  x{med / base:.4f} of plain  "
              f"max rel err vs fp64 {err[arm]:.2e}", flush=True)
    del Xs, Gs
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=14)
    ap.add_argument("--out", default=None)
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    assert args.rounds >= 5, "at least five rounds"
    results = [run_case(c, args.rounds) for c in (args.cases or list(CASES))]
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}, indent=1))
