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

  python tools/wq_bench.py --panel [--panel-ms 48,64,96,128,192,256,384,512] [--reps 30] [--warmup 5]

The 33 - 512 row range, by the same method: per shape (q/k/v, o, k/v, gate/up, gate or up alone, down),
scheme and M, ``ops.gemm_wq_panel`` against the dequantise + ``F.linear`` pair and, up to 128 rows,
``ops.gemm_wq_stream``, all alternating in one loop.

  python tools/wq_bench.py --tile [--tile-ms 48,96,129,192,256,384,512,768,1024,2048,4096] [--reps 30] [--warmup 5]

48 rows and up, by the same method: ``ops.gemm_wq_tile`` against the dequantise + ``F.linear`` pair and,
on the shapes and rows a ``WeightOnlyLinear`` would give it, ``ops.gemm_wq_panel``; ``pair_peak_mb`` / ``tile_peak_mb``
are one call's peak allocation above the operands.

  python tools/wq_bench.py --gemv [--gemv-ms 1,2,3,4] [--reps 30] [--warmup 5]

1 - 4 rows, by the same method: ``ops.gemm_wq_gemv`` against ``ops.gemm_wq_skinny`` on q/k/v, o, k/v,
gate/up, gate or up alone and down, and ``ops.gemm_wq_gemv_act_mul`` against ``ops.gemm_wq_skinny_act_mul`` on gate and
up; TB/s of both over the packed bytes.
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


def _cold_weights(N, K, scheme, dev, g):
    """One random weight of ``scheme`` (levels, scales, zero-points), its packed bytes, and copies of it totalling more
    than 512 MiB for the calls to rotate over."""
    bits, asym = SCHEMES[scheme]
    lo, hi = (-8, 8) if bits == 4 else (-128, 128)
    q = torch.randint(lo, hi, (N, K), device=dev, generator=g, dtype=torch.int8)
    Wq0 = pack_int4(q) if bits == 4 else q
    del q
    s0 = (torch.rand(N, K // 128 if bits == 4 else 1, device=dev, generator=g) * 0.01 + 1e-3)
    z0 = torch.randint(-8, 8, s0.shape, device=dev, generator=g, dtype=torch.int8) if asym else None
    qbytes = Wq0.numel() * Wq0.element_size() + s0.numel() * 4 + (z0.numel() if asym else 0)
    cps = [(Wq0.clone(), s0.clone(), None if z0 is None else z0.clone()) for _ in range(_copies(qbytes))]
    return Wq0, s0, z0, qbytes, cps


PANEL_SHAPES = ("qkv", "o", "kv", "gate_up", "gate", "down")


def panel_main(args):
    """--panel: ``ops.gemm_wq_panel`` against the dequantise + ``F.linear`` pair (and ``ops.gemm_wq_stream`` up to its 128
    rows), --stream's method."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    names = [k for k in args.shapes.split(",") if k] if args.shapes != ",".join(SHAPES) else list(PANEL_SHAPES)
    ms = [int(m) for m in args.panel_ms.split(",") if m]
    rows = []
    for shape in names:
        N, K = STREAM_SHAPES[shape]
        for scheme in args.schemes.split(","):
            Wq0, s0, z0, qbytes, cps = _cold_weights(N, K, scheme, dev, g)
            n_cp = len(cps)

            def pair(i, X):
                Wq, s, z = cps[i % n_cp]
                return F.linear(X, ops.dequantize_weight(Wq, s, K=K, zp_w=z, dtype=X.dtype))

            def kernel(op, i, X):
                Wq, s, z = cps[i % n_cp]
                return op(X, Wq, s, zp_w=z)

            row = {"shape": shape, "N": N, "K": K, "scheme": scheme, "packed_mb": round(qbytes / 1e6, 2),
                   "cold_copies": n_cp, "panel": {}}
            for M in ms:
                X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
                Y = kernel(ops.gemm_wq_panel, 0, X)
                same = all(torch.equal(Y[i:i + 16].view(torch.int16),
                                       ops.gemm_wq_skinny(X[i:i + 16], Wq0, s0, zp_w=z0).view(torch.int16))
                           for i in range(0, M, 16))
                fns = [lambda i: pair(i, X), lambda i: kernel(ops.gemm_wq_panel, i, X)]
                if M <= ops.WQ_STREAM_MAX_M:
                    fns.append(lambda i: kernel(ops.gemm_wq_stream, i, X))
                ts = _alternate(fns, args.reps, args.warmup)
                cell = {"pair_us": ts[0], "panel_us": ts[1], "speedup": round(ts[0] / ts[1], 2),
                        "panel_tbs": round(qbytes / ts[1] / 1e6, 3), "bits_equal_skinny": bool(same)}
                if len(ts) > 2:
                    cell["stream_us"] = ts[2]
                row["panel"][M] = cell
            rows.append(row)
            del cps
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "wq_bench --panel", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "warmup": args.warmup, "rows": rows}))


def _peak_above(fn, X):
    """Peak allocated bytes of one call of ``fn`` above what is allocated before it (the operands)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn(0, X)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def tile_main(args):
    """--tile: ``ops.gemm_wq_tile`` against the dequantise + ``F.linear`` pair and, where ``WeightOnlyLinear``'s panel
    bounds hold (M <= 512, its N / K range), ``ops.gemm_wq_panel``: --stream's method, plus the peak allocation of pair
    and kernel above the operands."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    names = [k for k in args.shapes.split(",") if k] if args.shapes != ",".join(SHAPES) else list(PANEL_SHAPES)
    ms = [int(m) for m in args.tile_ms.split(",") if m]
    L = WeightOnlyLinear
    rows = []
    for shape in names:
        N, K = STREAM_SHAPES[shape]
        panel_shape = K >= L.panel_min_k and N >= L.panel_min_n and (L.panel_max_n == 0 or N <= L.panel_max_n)
        for scheme in args.schemes.split(","):
            Wq0, s0, z0, qbytes, cps = _cold_weights(N, K, scheme, dev, g)
            n_cp = len(cps)

            def pair(i, X):
                Wq, s, z = cps[i % n_cp]
                return F.linear(X, ops.dequantize_weight(Wq, s, K=K, zp_w=z, dtype=X.dtype))

            def kernel(op, i, X):
                Wq, s, z = cps[i % n_cp]
                return op(X, Wq, s, zp_w=z)

            row = {"shape": shape, "N": N, "K": K, "scheme": scheme, "packed_mb": round(qbytes / 1e6, 2),
                   "cold_copies": n_cp, "tile": {}}
            for M in ms:
                X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
                fns = [lambda i: pair(i, X), lambda i: kernel(ops.gemm_wq_tile, i, X)]
                if panel_shape and M <= ops.WQ_PANEL_MAX_M:
                    fns.append(lambda i: kernel(ops.gemm_wq_panel, i, X))
                ts = _alternate(fns, args.reps, args.warmup)
                cell = {"pair_us": ts[0], "tile_us": ts[1], "speedup": round(ts[0] / ts[1], 2),
                        "tile_tflops": round(2.0 * M * N * K / ts[1] / 1e6, 1),
                        "pair_peak_mb": round(_peak_above(pair, X) / 1e6, 2),
                        "tile_peak_mb": round(_peak_above(lambda i, x: kernel(ops.gemm_wq_tile, i, x), X) / 1e6, 2)}
                if len(ts) > 2:
                    cell["panel_us"] = ts[2]
                row["tile"][M] = cell
            rows.append(row)
            del cps
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "wq_bench --tile", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "warmup": args.warmup, "rows": rows}))


def fused_main(args):
    """--fused: the two fused decode forms against the launches they replace, --stream's method.  ``act_mul``:
    ``ops.gemm_wq_skinny_act_mul`` on gate and up [14336, 4096] against two ``ops.gemm_wq_skinny`` calls, ``F.silu`` and
    the multiply; ``qkv``: ``ops.gemm_wq_skinny_multi`` on q [4096, 4096], k and v [1024, 4096] against three
    ``ops.gemm_wq_skinny`` calls.  Cold weights, device time between events that enclose all launches of a form."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    K = 4096
    cells = {"act_mul": (14336, 14336), "qkv": (4096, 1024, 1024)}
    rows = []
    for scheme in args.schemes.split(","):
        for name, Ns in cells.items():
            ws = [_cold_weights(N, K, scheme, dev, g) for N in Ns]
            qbytes = sum(w[3] for w in ws)
            n_cp = min(len(w[4]) for w in ws)
            row = {"cell": name, "N": list(Ns), "K": K, "scheme": scheme, "packed_mb": round(qbytes / 1e6, 2),
                   "cold_copies": n_cp, "fused": {}}

            def unfused(i, X):
                ys = [ops.gemm_wq_skinny(X, *w[4][i % n_cp][:2], zp_w=w[4][i % n_cp][2]) for w in ws]
                return F.silu(ys[0]) * ys[1] if name == "act_mul" else ys

            def fused(i, X):
                cp = [w[4][i % n_cp] for w in ws]
                if name == "act_mul":
                    return ops.gemm_wq_skinny_act_mul(X, *cp)
                return ops.gemm_wq_skinny_multi(X, [(*c, None) for c in cp])

            for M in [int(m) for m in args.fused_ms.split(",") if m]:
                X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
                a, b = unfused(0, X), fused(0, X)
                same = all(torch.equal(x.view(torch.int16), y.view(torch.int16))
                           for x, y in zip(*(([a], [b]) if name == "act_mul" else (a, b))))
                ts = _alternate([lambda i: unfused(i, X), lambda i: fused(i, X)], args.reps, args.warmup)
                row["fused"][M] = {"unfused_us": ts[0], "fused_us": ts[1], "speedup": round(ts[0] / ts[1], 2),
                                   "fused_tbs": round(qbytes / ts[1] / 1e6, 3), "bits_equal": bool(same)}
            rows.append(row)
            del ws
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "wq_bench --fused", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "warmup": args.warmup, "rows": rows}))


def gemv_main(args):
    """--gemv: ``ops.gemm_wq_gemv`` against ``ops.gemm_wq_skinny`` at 1 - 4 rows, --stream's method (cold weights, the
    two alternating call by call), and ``ops.gemm_wq_gemv_act_mul`` against ``ops.gemm_wq_skinny_act_mul`` on gate and
    up [14336, 4096].  TB/s counts the packed weight, scale and zero-point bytes."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    names = [k for k in args.shapes.split(",") if k] if args.shapes != ",".join(SHAPES) else list(PANEL_SHAPES)
    ms = [int(m) for m in args.gemv_ms.split(",") if m]
    rows = []
    for scheme in args.schemes.split(","):
        for shape in names + ["act_mul"]:
            N, K = STREAM_SHAPES["gate" if shape == "act_mul" else shape]
            ws = [_cold_weights(N, K, scheme, dev, g) for _ in range(2 if shape == "act_mul" else 1)]
            qbytes = sum(w[3] for w in ws)
            n_cp = min(len(w[4]) for w in ws)

            def call(new, i, X):
                cp = [w[4][i % n_cp] for w in ws]
                if shape == "act_mul":
                    return (ops.gemm_wq_gemv_act_mul if new else ops.gemm_wq_skinny_act_mul)(X, *cp)
                return (ops.gemm_wq_gemv if new else ops.gemm_wq_skinny)(X, cp[0][0], cp[0][1], zp_w=cp[0][2])

            row = {"shape": shape, "N": N, "K": K, "scheme": scheme, "packed_mb": round(qbytes / 1e6, 2),
                   "cold_copies": n_cp, "gemv": {}}
            for M in ms:
                X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
                err = (call(True, 0, X).float() - call(False, 0, X).float()).abs().max().item()
                ts = _alternate([lambda i: call(False, i, X), lambda i: call(True, i, X)], args.reps, args.warmup)
                row["gemv"][M] = {"skinny_us": ts[0], "gemv_us": ts[1], "speedup": round(ts[0] / ts[1], 2),
                                  "skinny_tbs": round(qbytes / ts[0] / 1e6, 3), "gemv_tbs": round(qbytes / ts[1] / 1e6, 3),
                                  "max_abs_diff": err}
            rows.append(row)
            del ws
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "wq_bench --gemv", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "warmup": args.warmup, "rows": rows}))


def stream_main(args):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    names = [k for k in args.shapes.split(",") if k] if args.shapes != ",".join(SHAPES) else list(STREAM_SHAPES)
    ms = [int(m) for m in args.stream_ms.split(",") if m]
    rows = []
    for shape in names:
        N, K = STREAM_SHAPES[shape]
        for scheme in args.schemes.split(","):
            Wq0, s0, z0, qbytes, cps = _cold_weights(N, K, scheme, dev, g)
            n_cp = len(cps)

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
    ap.add_argument("--panel", action="store_true", help="the 33 - 512 row range: qt_gemm_wq_panel against "
                    "dequantise + F.linear and, up to 128 rows, qt_gemm_wq_stream")
    ap.add_argument("--panel-ms", default="48,64,96,128,192,256,384,512")
    ap.add_argument("--tile", action="store_true", help="48 rows and up: qt_gemm_wq_tile against dequantise + F.linear "
                    "and, where the module would take it, qt_gemm_wq_panel")
    ap.add_argument("--tile-ms", default="48,96,129,192,256,384,512,768,1024,2048,4096")
    ap.add_argument("--fused", action="store_true", help="the fused decode forms (qt_gemm_wq_skinny_act_mul, "
                    "qt_gemm_wq_skinny_multi) against the skinny launches and torch glue they replace")
    ap.add_argument("--fused-ms", default="1,8,16")
    ap.add_argument("--gemv", action="store_true", help="1 - 4 rows: qt_gemm_wq_gemv against qt_gemm_wq_skinny, and "
                    "qt_gemm_wq_gemv_act_mul against qt_gemm_wq_skinny_act_mul")
    ap.add_argument("--gemv-ms", default="1,2,3,4")
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
    if args.fused:
        return fused_main(args)
    if args.gemv:
        return gemv_main(args)
    if args.stream:
        return stream_main(args)
    if args.panel:
        return panel_main(args)
    if args.tile:
        return tile_main(args)
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
