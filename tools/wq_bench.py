"""W4A16 / W4A16_ASYM / W8A16 linear on the packed weights vs bf16 F.linear at Llama-3-8B's shapes.

  python tools/wq_bench.py [--skinny-ms 1,2,4,8,16] [--large-ms 4096,8192] [--shapes-70b] [--reps 30]

Per shape (q/k/v fused N = 6144, K = 4096; gate/up N = 28672, K = 4096; down N = 4096, K = 14336; --shapes-70b adds
8192-wide ones) and scheme:
* decode (qt_gemm_wq_skinny, M in --skinny-ms) against bf16 F.linear on the same shape.  "cold" rotates over distinct
  weight copies totalling more than 512 MiB (twice the 256 MiB Infinity Cache), as decode reads each weight once per
  token; "warm" replays one copy back to back.  GB/s counts the packed weight, scale and zero-point bytes.
* large M (--large-ms): qt_dequantize_weight alone (GB/s over the bytes it reads plus the bf16 bytes it writes, cold)
  and the whole WeightOnlyLinear (dequantise + F.linear) against F.linear on the dense weight.
Prints one JSON line.  Device time from HIP events, mean over --reps after --warmup.

  python tools/wq_bench.py --stream [--stream-ms 17,32,48,64,96,128] [--reps 30] [--warmup 5]

The 17 - 128 row range: per shape (q/k/v, o, k/v, gate/up, gate or up alone, down, and K = 512 / 1024 /
2048 at N = 4096), scheme and M, ``ops.gemm_wq_stream`` against what a default WeightOnlyLinear does for those rows --
``ops.dequantize_weight`` into a fresh transient weight, then ``F.linear``, timed as a pair.  The two alternate call by
call in one loop, each call between its own HIP events, the weights rotating over more than 512 MiB of copies; median
us.  ``bits_equal_skinny`` says whether every 16-row slice of the kernel's output equals the skinny kernel's bits;
``skinny16_us`` is the skinny kernel at M = 16 on the same weights, so the step at row 17 shows.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantool_amd.engine.qlinear import WeightOnlyLinear, pack_int4  # noqa: E402
from quantool_amd.hip import ops  # noqa: E402

SHAPES = {"qkv": (6144, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}
SHAPES_70B = {"qkv_70b": (10240, 8192), "gate_up_70b": (57344, 8192), "down_70b": (8192, 28672)}
SCHEMES = {"W4A16": (4, False), "W4A16_ASYM": (4, True), "W8A16": (8, False)}
COLD_BYTES = 512 << 20


def _time(fn, reps, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(warmup + i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


def _copies(nbytes):
    return max(2, -(-int(COLD_BYTES * 1.1) // nbytes))


STREAM_SHAPES = {"qkv": (6144, 4096), "o": (4096, 4096), "kv": (1024, 4096), "gate_up": (28672, 4096),
                 "gate": (14336, 4096), "down": (4096, 14336), "k512": (4096, 512), "k1024": (4096, 1024),
                 "k2048": (4096, 2048)}


def _median_us(pairs):
    ts = sorted(a.elapsed_time(b) for a, b in pairs)
    return round(ts[len(ts) // 2] * 1e3, 2)


def _alternate(fns, reps, warmup):
    """Median device time (us) of each of ``fns``, called in turn in one loop, every call between its own events."""
    ev = [[] for _ in fns]
    for i in range(warmup + reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(i)
            b.record()
            if i >= warmup:
                ev[k].append((a, b))
    torch.cuda.synchronize()
    return [_median_us(e) for e in ev]


def stream_main(args):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    names = [k for k in args.shapes.split(",") if k] if args.shapes != ",".join(SHAPES) else list(STREAM_SHAPES)
    ms = [int(m) for m in args.stream_ms.split(",") if m]
    rows = []
    for shape in names:
        N, K = STREAM_SHAPES[shape]
        G = K // 128
        for scheme in args.schemes.split(","):
            bits, asym = SCHEMES[scheme]
            lo, hi = (-8, 8) if bits == 4 else (-128, 128)
            q = torch.randint(lo, hi, (N, K), device=dev, generator=g, dtype=torch.int8)
            Wq0 = pack_int4(q) if bits == 4 else q
            del q
            s0 = (torch.rand(N, G if bits == 4 else 1, device=dev, generator=g) * 0.01 + 1e-3)
            z0 = torch.randint(-8, 8, s0.shape, device=dev, generator=g, dtype=torch.int8) if asym else None
            qbytes = Wq0.numel() * Wq0.element_size() + s0.numel() * 4 + (z0.numel() if asym else 0)
            n_cp = _copies(qbytes)
            cps = [(Wq0.clone(), s0.clone(), None if z0 is None else z0.clone()) for _ in range(n_cp)]

            def pair(i, X):
                Wq, s, z = cps[i % n_cp]
                return F.linear(X, ops.dequantize_weight(Wq, s, K=K, zp_w=z, dtype=X.dtype))

            def stream(i, X):
                Wq, s, z = cps[i % n_cp]
                return ops.gemm_wq_stream(X, Wq, s, zp_w=z)

            X16 = torch.randn(16, K, device=dev, generator=g).to(torch.bfloat16)
            skinny16, = _alternate([lambda i: ops.gemm_wq_skinny(X16, cps[i % n_cp][0], cps[i % n_cp][1],
                                                                 zp_w=cps[i % n_cp][2])], args.reps, args.warmup)
            row = {"shape": shape, "N": N, "K": K, "scheme": scheme, "packed_mb": round(qbytes / 1e6, 2),
                   "cold_copies": n_cp, "skinny16_us": skinny16, "stream": {}}
            for M in ms:
                X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
                Y = stream(0, X)
                same = all(torch.equal(Y[i:i + 16].view(torch.int16),
                                       ops.gemm_wq_skinny(X[i:i + 16], Wq0, s0, zp_w=z0).view(torch.int16))
                           for i in range(0, M, 16))
                t_pair, t_stream = _alternate([lambda i: pair(i, X), lambda i: stream(i, X)], args.reps, args.warmup)
                row["stream"][M] = {"pair_us": t_pair, "stream_us": t_stream, "speedup": round(t_pair / t_stream, 2),
                                    "stream_tbs": round(qbytes / t_stream / 1e6, 3), "bits_equal_skinny": bool(same)}
            rows.append(row)
            del cps
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "wq_bench --stream", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "warmup": args.warmup, "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream", action="store_true", help="the 17 - 128 row range: qt_gemm_wq_stream against "
                    "dequantise + F.linear")
    ap.add_argument("--stream-ms", default="17,32,48,64,96,128")
    ap.add_argument("--skinny-ms", default="1,2,4,8,16")
    ap.add_argument("--large-ms", default="4096,8192")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--shapes-70b", action="store_true")
    ap.add_argument("--schemes", default=",".join(SCHEMES))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wq_bench needs a GPU")
    if args.stream:
        return stream_main(args)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = {k: SHAPES[k] for k in args.shapes.split(",") if k}
    if args.shapes_70b:
        shapes.update(SHAPES_70B)
    skinny_ms = [int(m) for m in args.skinny_ms.split(",") if m]
    large_ms = [int(m) for m in args.large_ms.split(",") if m]
    rows = []
    for shape, (N, K) in shapes.items():
        G = (K + 127) // 128
        dense_bytes = N * K * 2
        Wd = [torch.randn(N, K, device=dev, generator=g).to(torch.bfloat16) * 0.02 for _ in range(_copies(dense_bytes))]
        for scheme in args.schemes.split(","):
            bits, asym = SCHEMES[scheme]
            lo, hi = (-8, 8) if bits == 4 else (-128, 128)
            q = torch.randint(lo, hi, (N, K), device=dev, generator=g, dtype=torch.int8)
            Wq0 = pack_int4(q) if bits == 4 else q
            del q
            s0 = (torch.rand(N, G if bits == 4 else 1, device=dev, generator=g) * 0.01 + 1e-3)
            z0 = torch.randint(-8, 8, s0.shape, device=dev, generator=g, dtype=torch.int8) if asym else None
            qbytes = Wq0.numel() * Wq0.element_size() + s0.numel() * 4 + (z0.numel() if asym else 0)
            n_cp = _copies(qbytes)
            cps = [(Wq0.clone(), s0.clone(), None if z0 is None else z0.clone()) for _ in range(n_cp)]
            row = {"shape": shape, "N": N, "K": K, "scheme": scheme, "packed_mb": round(qbytes / 1e6, 2),
                   "cold_copies": n_cp, "skinny": {}, "large": {}}
            for M in skinny_ms:
                X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
                cold = _time(lambda i: ops.gemm_wq_skinny(X, cps[i % n_cp][0], cps[i % n_cp][1], zp_w=cps[i % n_cp][2]),
                             args.reps, args.warmup)
                warm = _time(lambda i: ops.gemm_wq_skinny(X, cps[0][0], cps[0][1], zp_w=cps[0][2]), args.reps,
                             args.warmup)
                nd = len(Wd)
                lin_cold = _time(lambda i: F.linear(X, Wd[i % nd]), args.reps, args.warmup)
                lin_warm = _time(lambda i: F.linear(X, Wd[0]), args.reps, args.warmup)
                row["skinny"][M] = {
                    "cold_us": round(cold * 1e6, 2), "warm_us": round(warm * 1e6, 2),
                    "cold_tbs": round(qbytes / cold / 1e12, 3), "warm_tbs": round(qbytes / warm / 1e12, 3),
                    "linear_cold_us": round(lin_cold * 1e6, 2), "linear_warm_us": round(lin_warm * 1e6, 2),
                    "speedup_cold": round(lin_cold / cold, 2), "speedup_warm": round(lin_warm / warm, 2)}
            out = torch.empty(N, K, dtype=torch.bfloat16, device=dev)
            dq = _time(lambda i: ops.dequantize_weight(cps[i % n_cp][0], cps[i % n_cp][1], K=K, zp_w=cps[i % n_cp][2],
                                                       out=out), args.reps, args.warmup)
            row["dequant"] = {"us": round(dq * 1e6, 2), "tbs": round((qbytes + dense_bytes) / dq / 1e12, 3)}
            m = WeightOnlyLinear(K, N, Wq0, s0, weight_zero_point=z0)
            for M in large_ms:
                X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
                with torch.no_grad():
                    t_mod = _time(lambda i: m(X), args.reps, args.warmup)
                    t_lin = _time(lambda i: F.linear(X, Wd[0]), args.reps, args.warmup)
                row["large"][M] = {"module_us": round(t_mod * 1e6, 1), "linear_us": round(t_lin * 1e6, 1),
                                   "overhead": round(t_mod / t_lin - 1.0, 4)}
            rows.append(row)
            del cps, m
            torch.cuda.empty_cache()
        del Wd
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "wq_bench", "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
