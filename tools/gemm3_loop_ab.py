#!/usr/bin/env python3
"""In-process A/B of the two main loops of gemm3_kernel (csrc/gemm3_tn.hip; QT_G3_LOOP is read per launch), alternating
them round by round: the k = 14080, 256 x 14080 block-row product through the test face (wall time, plane split
included) and the factor chain at K = 14336, 3 x K = 4096 batched and K = 28672 (device events).
usage: gemm3_loop_ab.py [prod] [f14336] [b4096] [f28672]      (default: all four)"""
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from quantool_amd.hip import ops

dev = torch.device("cuda:0")
NAMES = ("chunk", "tri")
which = sys.argv[1:] or ["prod", "f14336", "b4096", "f28672"]


def setloop(name):
    if name == "chunk":
        os.environ["QT_G3_LOOP"] = "chunk"
    else:
        os.environ.pop("QT_G3_LOOP", None)


def ev(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def report(tag, res):
    for name in NAMES:
        x = sorted(res[name])
        print(f"{tag:28s} {name:5s} median {statistics.median(x):8.3f} ms  min {x[0]:8.3f}  max {x[-1]:8.3f}  n={len(x)}", flush=True)


if "prod" in which:
    k, M, N = 14080, 256, 14080
    A = torch.randn(k, M, device=dev)
    B = torch.randn(k, N, device=dev)
    C = torch.zeros(M, N, device=dev)
    res = {n: [] for n in NAMES}
    for r in range(7):
        for name in NAMES:
            setloop(name)
            ops.gemm3_tn(A, B, C, 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                ops.gemm3_tn(A, B, C, 1)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / 10 * 1e3)
    report("product k=14080 (face, +split)", res)
    del A, B, C


def gram(K, seed):
    torch.manual_seed(seed)
    X = torch.randn(2 * K, K, device=dev).to(torch.bfloat16)
    G = torch.zeros(K, K, device=dev)
    ops.xtx_accumulate(X, G)
    return G


for tag, K, nb, rounds in (("f14336", 14336, 1, 7), ("b4096", 4096, 3, 9), ("f28672", 28672, 1, 3)):
    if tag not in which:
        continue
    Gs = [gram(K, s) for s in range(nb)]
    res = {n: [] for n in NAMES}
    out = {}
    for r in range(rounds + 1):
        for name in NAMES:
            setloop(name)
            As = [ops.hessian_prepare(G, 8, 0.01, None)[0] for G in Gs]
            if nb == 1:
                U = torch.empty((K, K), dtype=torch.float32, device=dev) if name not in out else out[name]
                t = ev(lambda: ops.cholesky_inverse_upper(As[0], U))
            else:
                A3 = torch.stack(As)
                U = torch.empty((nb, K, K), dtype=torch.float32, device=dev) if name not in out else out[name]
                t = ev(lambda: ops.cholesky_inverse_upper_batched(A3, U))
                del A3
            out[name] = U
            del As
            if r > 0:
                res[name].append(t)
    report(f"factor K={K} x{nb}", res)
    d = (out["chunk"].double() - out["tri"].double()).abs().max().item() / out["chunk"].abs().max().item()
    print(f"  max |U_chunk - U_tri| / max|U| = {d:.3e}", flush=True)
    del out, Gs
    torch.cuda.empty_cache()
