#!/usr/bin/env python3
"""In-process A/B of the two plane modes of the factor chain's block-row products (csrc/gemm3_tn.hip: three bf16 planes
and six products against two fp16 planes and three; QT_CHOL_PLANES is read per call), alternating them round by round:
the k = 14080, 256 x 14080 block-row product through the test faces (wall time, plane split included) and the factor
chain at K = 14336, 3 x K = 4096 batched and K = 28672 (device events).  Both arms get the bound on lambda_min.
usage: chol_planes_ab.py [prod] [f14336] [b4096] [f28672]      (default: all four)"""
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from quantool_amd.hip import ops

dev = torch.device("cuda:0")
NAMES = ("bf16x3", "f16x2")
which = sys.argv[1:] or ["prod", "f14336", "b4096", "f28672"]


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
        print(f"{tag:28s} {name:6s} median {statistics.median(x):8.3f} ms  min {x[0]:8.3f}  max {x[-1]:8.3f}  n={len(x)}", flush=True)


if "prod" in which:
    k, M, N = 14080, 256, 14080
    A = torch.randn(k, M, device=dev)
    B = torch.randn(k, N, device=dev)
    C = torch.zeros(M, N, device=dev)
    ba, bb = float(A.abs().max()), float(B.abs().max())
    run = {"bf16x3": lambda: ops.gemm3_tn(A, B, C, 1), "f16x2": lambda: ops.gemm3_tn_f16x2(A, B, C, ba, bb, kind=1)}
    res = {n: [] for n in NAMES}
    for r in range(7):
        for name in NAMES:
            run[name]()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                run[name]()
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
    damps = torch.zeros(nb, dtype=torch.float32, device=dev)
    for r in range(rounds + 1):
        for name in NAMES:
            os.environ["QT_CHOL_PLANES"] = name
            As = [ops.hessian_prepare(G, 8, 0.01, None, damp_out=damps[b:b + 1])[0] for b, G in enumerate(Gs)]
            lb = damps * 0.5
            if nb == 1:
                U = torch.empty((K, K), dtype=torch.float32, device=dev) if name not in out else out[name]
                t = ev(lambda: ops.cholesky_inverse_upper(As[0], U, min_eig_lb=lb))
            else:
                A3 = torch.stack(As)
                U = torch.empty((nb, K, K), dtype=torch.float32, device=dev) if name not in out else out[name]
                t = ev(lambda: ops.cholesky_inverse_upper_batched(A3, U, min_eig_lb=lb))
                del A3
            out[name] = U
            del As
            if r > 0:
                res[name].append(t)
    report(f"factor K={K} x{nb}", res)
    d = (out["bf16x3"].double() - out["f16x2"].double()).abs().max().item() / out["bf16x3"].abs().max().item()
    print(f"  max |U_bf16x3 - U_f16x2| / max|U| = {d:.3e}", flush=True)
    del out, Gs
    torch.cuda.empty_cache()
