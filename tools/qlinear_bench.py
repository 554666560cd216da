"""W8A8 / W4A8 linear on the int8 MFMA vs bf16 F.linear at Llama-3-8B's prefill shapes, and the decode GEMV against the
tiled GEMM at decode sizes.

  python tools/qlinear_bench.py [--ms 4096,8192] [--reps 20] [--warmup 5]
  python tools/qlinear_bench.py --ms 1,8,16            # decode: qt_gemm_i8 vs qt_gemm_i8_skinny
  python tools/qlinear_bench.py --mid [--reps 30]      # 17 .. 128 rows: qt_gemm_i8 vs qt_gemm_i8_mid
  python tools/qlinear_bench.py --ring-w4 [--ms 2048,4096,8192]   # W4A8 prefill: qt_gemm_i8 vs qt_gemm_i8_ring_w4
  python tools/qlinear_bench.py --splitk [--splits 4]  # 129 .. 2047 rows: qt_gemm_i8 vs qt_gemm_i8_ring vs qt_splitk_gemm_i8
  python tools/qlinear_bench.py --mlp [--ms 1,16,32,128,2048,8192]     # three Linears + glue vs QuantizedMLP
  python tools/qlinear_bench.py --norm [--ms 1,16,32,128,2048,8192]    # RMSNorm + 3 (2) quantisers vs one fused launch

Per shape (q/k/v fused N = 6144, K = 4096; gate/up N = 28672, K = 4096; down N = 4096, K = 14336) and M: device time
(HIP events, mean over --reps after --warmup) of the activation pass (qt_quantize_tokens_i8), the GEMM (qt_gemm_i8:
W8A8 = int8 channel-wise weights, symmetric activations; W4A8 = packed int4 g128 weights, asymmetric activations),
QuantizedLinear end to end, bf16 F.linear and torch._int_mm (when this torch build runs it; else the reason).
Prints one JSON line: TOPS (2 M N K / time), the share of the 5 PF int8 dense peak, the activation pass's GB/s and the
ratio of bf16 F.linear time to the W8A8 / W4A8 QuantizedLinear time (> 1: the quantized linear is faster).

Every M <= 16 in --ms is a decode size and gets a "decode" row instead: qt_gemm_i8 and qt_gemm_i8_skinny on the same
operands, alternating call by call in one loop, each call between its own pair of HIP events (so host gaps between
launches are not counted), the weights rotating over distinct copies totalling more than 512 MiB (twice the Infinity
Cache) so that every call reads them cold, as a decode step does.  Reported per kernel: median and mean microseconds,
weight + scale (+ wsum) bytes over the median, and that as a share of 8 TB/s.

Every M > 16 also gets a "ring" row (W8A8, symmetric activations): the tiled qt_gemm_i8 and the LDS-ring qt_gemm_i8_ring
on the same operands, with qt_quantize_tokens_i8, bf16 F.linear and torch._int_mm, all alternating in that one loop
under the same harness (per-call events, weights rotating over more than 512 MiB of copies, medians).  Reported:
median microseconds and TOPS per kernel, tiled / ring ("speedup"), and bf16 F.linear over quantize_tokens + ring
("bf16_over_act_plus_ring", > 1: the W8A8 linear on the ring is faster than bf16).

--mid prints only "mid" rows: the tiled qt_gemm_i8 (the yardstick) and qt_gemm_i8_mid on the same operands at M = 17, 24,
32, 48, 64, 96, 128, with M = 16 (where qt_gemm_i8_skinny joins the loop) and M = 256 (tiled alone) as neighbours, on the
three shapes above plus o_proj (4096 x 4096) and k/v (1024 x 4096), and on N = 4096 at K = 256 .. 2048 (the sweep that
sets ``QuantizedLinear.mid_min_k``; ``--mid-shapes`` picks among them, and knows ``gate_or_up`` = 14336 x 4096
besides), W8A8 (int8, G = 1, symmetric) and W4A8 (int4, G = K/128, asymmetric), under the
decode rows' harness (alternating call by call, per-call events, weights rotating over more than 512 MiB of copies,
medians), with ``bits_equal`` per cell.

--ring-w4 prints only "ring_w4" rows (W4A8: packed int4 g128 weights, asymmetric activations): the tiled qt_gemm_i8 and
the LDS-ring qt_gemm_i8_ring_w4 on the same operands, with qt_quantize_tokens_i8 and bf16 F.linear, under the "ring"
rows' harness, at --ms (default 2048,4096,8192) on the three shapes, with ``bits_equal`` per cell and tiled / ring as
"speedup".  ``QuantizedLinear.ring_w4_min_m`` is set from two such runs.

--splitk prints only "splitk" rows (W8A8, symmetric activations) at M = 129, 192, 256, 320, 384, 512, 640, 768, 1024, 1536,
2047 (``--ms`` picks others) on q/k/v, o (4096 x 4096), gate/up, down and Llama-3-70B's down (8192 x 28672; ``--shapes``
picks among them): the tiled qt_gemm_i8 (the yardstick), the whole-K ring qt_gemm_i8_ring, qt_splitk_gemm_i8 at the
rule's S (``--splits S`` forces another; a cell where S exceeds K / 128 is skipped), bf16 F.linear and torch._int_mm,
under the "ring" rows' harness (alternating call by call, per-call events, weights rotating over more than 512 MiB of
copies, medians), with ``bits_equal`` per cell, tiled / split-K as "speedup", and "reduce_share": the reduce kernel's
part of the two launches' device time, as torch's profiler reports them.  ``QuantizedLinear.splitk_min_m`` /
``splitk_min_k`` are set from two such runs.

--mlp prints only "mlp" rows: a Llama-3-8B MLP (hidden 4096, intermediate 14336) as W8A8 and W4A8, at --ms (default
1,16,32,128,2048,8192).  "glue": ``F.silu(g) * u`` followed by qt_quantize_tokens_i8 (three launches) against
qt_act_mul_quantize_i8 on the same gate / up outputs.  "mlp": ``down(silu(gate(x)) * up(x))`` on three
``QuantizedLinear``s (eight launches) against ``QuantizedMLP`` on the same three (five), under the decode rows' harness
(alternating call by call, per-call events, the Linears rotating over more than 512 MiB of copies, medians).  The unfused
form runs twice in each loop ("unfused", "unfused_again"): their ratio is the yardstick's own spread.  Bit equality of the
two forms is asserted before anything is timed.

--norm prints only "norm" rows: the glue in front of q/k/v and of gate/up alone, at K = 4096 and --ms (default
1,16,32,128,2048,8192), bf16, with symmetric and with asymmetric activations.  "qkv": the installed ``LlamaRMSNorm``
followed by three qt_quantize_tokens_i8 calls on its output against one qt_rmsnorm_quantize_i8 launch; "gate_up": the
same with two.  The --mlp rows' protocol: forms alternate call by call between their own events, the unfused form runs
twice in each loop and the ratio of its two medians is the spread.  Before anything is timed the fused Y is compared
with the norm's (``y_differ``: how many elements land on the other 16-bit neighbour -- the kernel's sum over K runs in its
own order) and its rows are asserted equal to qt_quantize_tokens_i8 of its own Y; ``torch_norm_kernels``
is the number of device kernels one call of the installed norm launches, as torch's profiler counts them.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantool_amd.engine.qlinear import QuantizedLinear, group_sums, pack_int4  # noqa: E402
from quantool_amd.hip import ops  # noqa: E402

SHAPES = {"qkv": (6144, 4096), "gate_up": (28672, 4096), "down": (4096, 14336)}
INT8_PEAK = 5.0e15     # MI355X dense int8 MFMA ops/s (MI355X_MICROARCH.md, Matrix cores: 2x the bf16 rate)
HBM_PEAK = 8.0e12      # bytes/s
COLD_BYTES = 512 << 20
DECODE_MAX_M = ops.I8_SKINNY_MAX_M


def time_pair(fns, reps, warmup):
    """{name: [seconds per call]}: the callables of ``fns`` run in turn, rep by rep (fn(i) with i the call's index), each
    call between its own pair of events."""
    names = list(fns)
    for i in range(warmup):
        for n in names:
            fns[n](i)
    torch.cuda.synchronize()
    ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
          for n in names}
    for i in range(reps):
        for n in names:
            a, b = ev[n][i]
            a.record()
            fns[n](warmup + i)
            b.record()
    torch.cuda.synchronize()
    return {n: [a.elapsed_time(b) * 1e-3 for a, b in ev[n]] for n in names}


def summarize(times, nbytes):
    t = sorted(times)
    med = t[len(t) // 2]
    return {"us": round(med * 1e6, 2), "mean_us": round(sum(t) / len(t) * 1e6, 2), "min_us": round(t[0] * 1e6, 2),
            "tbs": round(nbytes / med / 1e12, 3), "hbm_frac": round(nbytes / med / HBM_PEAK, 3)}


def decode_rows(shape, N, K, ms, reps, warmup, dev, g):
    """qt_gemm_i8 vs qt_gemm_i8_skinny at decode sizes, W8A8 (int8 channel-wise, symmetric activations) and W4A8
    (packed int4 g128, asymmetric activations), cold weights."""
    rows = []
    for scheme in ("W8A8", "W4A8"):
        int4 = scheme == "W4A8"
        G = K // 128 if int4 else 1
        q = torch.randint(-8 if int4 else -128, 8 if int4 else 128, (N, K), device=dev, generator=g, dtype=torch.int8)
        W0 = pack_int4(q) if int4 else q
        s0 = torch.rand(N, G, device=dev, generator=g) * 1e-2
        ws0 = group_sums(q, G) if int4 else None
        del q
        nbytes = W0.numel() * W0.element_size() + s0.numel() * 4 + (ws0.numel() * 4 if int4 else 0)
        n_cp = max(2, -(-int(COLD_BYTES * 1.1) // nbytes))
        cps = [(W0.clone(), s0.clone(), None if ws0 is None else ws0.clone()) for _ in range(n_cp)]
        for M in ms:
            X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not int4)

            def call(fn):
                return lambda i: fn(Xq, s_x, cps[i % n_cp][0], cps[i % n_cp][1], K=K, zp_x=zp_x, wsum=cps[i % n_cp][2])

            # the two kernels must read different copies in one rep, or the second finds the first's weights cached
            t = time_pair({"gemm_i8": call(ops.gemm_i8), "gemm_i8_skinny": lambda i: call(ops.gemm_i8_skinny)(i + 1)},
                          reps, warmup)
            same = torch.equal(call(ops.gemm_i8)(0).view(torch.int16), call(ops.gemm_i8_skinny)(0).view(torch.int16))
            row = {"shape": shape, "scheme": scheme, "M": M, "N": N, "K": K, "weight_mb": round(nbytes / 1e6, 2),
                   "cold_copies": n_cp, "bits_equal": same, "gemm_i8": summarize(t["gemm_i8"], nbytes),
                   "gemm_i8_skinny": summarize(t["gemm_i8_skinny"], nbytes)}
            row["speedup"] = round(row["gemm_i8"]["us"] / row["gemm_i8_skinny"]["us"], 2)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
        del cps
        torch.cuda.empty_cache()
    return rows


MID_MS = (16, 17, 24, 32, 48, 64, 96, 128, 256)
MID_SHAPES = {"o_proj": (4096, 4096), "kv": (1024, 4096), "qkv": (6144, 4096), "gate_up": (28672, 4096),
              "down": (4096, 14336), "n4096_k256": (4096, 256), "n4096_k512": (4096, 512),
              "n4096_k1024": (4096, 1024), "n4096_k2048": (4096, 2048)}
MID_EXTRA_SHAPES = {"gate_or_up": (14336, 4096)}       # one of gate / up alone (an unfused MLP): --mid-shapes gate_or_up


def mid_rows(shape, N, K, ms, reps, warmup, dev, g):
    """qt_gemm_i8 vs qt_gemm_i8_mid from 17 to 128 rows (and their neighbours), W8A8 and W4A8, cold weights."""
    rows = []
    for scheme in ("W8A8", "W4A8"):
        int4 = scheme == "W4A8"
        G = K // 128 if int4 else 1
        q = torch.randint(-8 if int4 else -128, 8 if int4 else 128, (N, K), device=dev, generator=g, dtype=torch.int8)
        W0 = pack_int4(q) if int4 else q
        s0 = torch.rand(N, G, device=dev, generator=g) * 1e-2
        ws0 = group_sums(q, G) if int4 else None
        del q
        nbytes = W0.numel() * W0.element_size() + s0.numel() * 4 + (ws0.numel() * 4 if int4 else 0)
        n_cp = max(3, -(-int(COLD_BYTES * 1.1) // nbytes))
        cps = [(W0.clone(), s0.clone(), None if ws0 is None else ws0.clone()) for _ in range(n_cp)]
        for M in ms:
            X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not int4)

            def call(fn, shift):
                # kernels that share a rep read different copies, or the second finds the first's weights cached
                def run(i):
                    W, s, ws = cps[(i + shift) % n_cp]
                    return fn(Xq, s_x, W, s, K=K, zp_x=zp_x, wsum=ws)
                return run

            fns = {"gemm_i8": call(ops.gemm_i8, 0)}
            if M <= ops.I8_MID_MAX_M:
                fns["gemm_i8_mid"] = call(ops.gemm_i8_mid, 1)
            if M <= ops.I8_SKINNY_MAX_M:
                fns["gemm_i8_skinny"] = call(ops.gemm_i8_skinny, 2)
            t = time_pair(fns, reps, warmup)
            want = fns["gemm_i8"](0).view(torch.int16)
            row = {"shape": shape, "scheme": scheme, "M": M, "N": N, "K": K, "weight_mb": round(nbytes / 1e6, 2),
                   "cold_copies": n_cp,
                   "bits_equal": all(torch.equal(want, fns[k](0).view(torch.int16)) for k in fns if k != "gemm_i8")}
            for k in fns:
                row[k] = summarize(t[k], nbytes)
            if "gemm_i8_mid" in fns:
                row["speedup"] = round(row["gemm_i8"]["us"] / row["gemm_i8_mid"]["us"], 2)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
        del cps
        torch.cuda.empty_cache()
    return rows


def ring_rows(shape, N, K, ms, reps, warmup, dev, g):
    """qt_gemm_i8 vs qt_gemm_i8_ring at prefill sizes, W8A8 (int8 channel-wise, symmetric activations), beside the
    activation pass, bf16 F.linear and torch._int_mm."""
    rows = []
    q = torch.randint(-128, 128, (N, K), device=dev, generator=g, dtype=torch.int8)
    s_w = torch.rand(N, 1, device=dev, generator=g) * 1e-3
    n_cp = max(2, -(-int(COLD_BYTES * 1.1) // q.numel()))
    cps = [q.clone() for _ in range(n_cp)]
    cps_t = [c.t() for c in cps]
    n_bf = max(2, -(-int(COLD_BYTES * 1.1) // (2 * q.numel())))
    bfs = [(torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16) for _ in range(n_bf)]
    del q
    for M in ms:
        X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        Xq, s_x, _ = ops.quantize_tokens_i8(X, symmetric=True)
        # kernels that share a rep read different copies, or the second finds the first's weights cached
        fns = {"gemm_i8": lambda i: ops.gemm_i8(Xq, s_x, cps[i % n_cp], s_w),
               "gemm_i8_ring": lambda i: ops.gemm_i8_ring(Xq, s_x, cps[(i + 1) % n_cp], s_w),
               "quantize_tokens": lambda i: ops.quantize_tokens_i8(X, symmetric=True),
               "bf16_linear": lambda i: F.linear(X, bfs[i % n_bf])}
        try:
            torch._int_mm(Xq, cps_t[0])
            fns["torch_int_mm"] = lambda i: torch._int_mm(Xq, cps_t[(i + 2) % n_cp])
        except Exception:  # noqa: BLE001  (the prefill rows report the reason)
            pass
        t = time_pair(fns, reps, warmup)
        same = torch.equal(fns["gemm_i8"](0).view(torch.int16), fns["gemm_i8_ring"](0).view(torch.int16))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        ops_n = 2.0 * M * N * K
        row = {"shape": shape, "scheme": "W8A8", "M": M, "N": N, "K": K, "cold_copies": n_cp, "bits_equal": same,
               "us": {k: round(v * 1e6, 2) for k, v in med.items()},
               "min_us": {k: round(min(v) * 1e6, 2) for k, v in t.items()},
               "tops": {k: round(ops_n / v / 1e12, 1) for k, v in med.items() if k != "quantize_tokens"},
               "int8_peak_frac": {k: round(ops_n / med[k] / INT8_PEAK, 3) for k in ("gemm_i8", "gemm_i8_ring")},
               "speedup": round(med["gemm_i8"] / med["gemm_i8_ring"], 3),
               "bf16_over_act_plus_tiled": round(med["bf16_linear"] / (med["quantize_tokens"] + med["gemm_i8"]), 3),
               "bf16_over_act_plus_ring": round(med["bf16_linear"] / (med["quantize_tokens"] + med["gemm_i8_ring"]), 3)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del X, Xq
    del cps, cps_t, bfs
    torch.cuda.empty_cache()
    return rows


def kernel_shares(fn, calls=5):
    """{kernel name: device microseconds per call} over ``calls`` calls of ``fn`` (torch's profiler), or the reason."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if e.device_type == DeviceType.CUDA and "memcpy" not in e.name.lower():
                out[e.name] = out.get(e.name, 0.0) + e.device_time / calls
        return out
    except Exception as e:  # noqa: BLE001
        return {"reason": f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"}


def splitk_rows(shape, N, K, ms, splits, reps, warmup, dev, g):
    """qt_gemm_i8 vs qt_gemm_i8_ring vs qt_splitk_gemm_i8 at short-prompt sizes, W8A8 (int8 channel-wise, symmetric
    activations), beside bf16 F.linear and torch._int_mm: the "ring" rows' harness."""
    rows = []
    q = torch.randint(-128, 128, (N, K), device=dev, generator=g, dtype=torch.int8)
    s_w = torch.rand(N, 1, device=dev, generator=g) * 1e-3
    n_cp = max(3, -(-int(COLD_BYTES * 1.1) // q.numel()))
    cps = [q.clone() for _ in range(n_cp)]
    cps_t = [c.t() for c in cps]
    n_bf = max(2, -(-int(COLD_BYTES * 1.1) // (2 * q.numel())))
    bfs = [(torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16) for _ in range(n_bf)]
    del q
    for M in ms:
        S, ws_bytes = ops.splitk_gemm_i8_plan(M, N, K)
        if splits:
            if splits > min(K // ops.SPLITK_I8_K_UNIT, ops.SPLITK_I8_MAX_SPLITS):
                continue
            S, ws_bytes = ops.splitk_gemm_i8_plan(M, N, K, splits=splits)
        X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        Xq, s_x, _ = ops.quantize_tokens_i8(X, symmetric=True)
        # kernels that share a rep read different copies, or the second finds the first's weights cached
        fns = {"gemm_i8": lambda i: ops.gemm_i8(Xq, s_x, cps[i % n_cp], s_w),
               "gemm_i8_ring": lambda i: ops.gemm_i8_ring(Xq, s_x, cps[(i + 1) % n_cp], s_w),
               "splitk_gemm_i8": lambda i: ops.splitk_gemm_i8(Xq, s_x, cps[(i + 2) % n_cp], s_w, splits=S),
               "bf16_linear": lambda i: F.linear(X, bfs[i % n_bf])}
        try:
            torch._int_mm(Xq, cps_t[0])
            fns["torch_int_mm"] = lambda i: torch._int_mm(Xq, cps_t[i % n_cp])
        except Exception:  # noqa: BLE001  (the prefill rows report the reason)
            pass
        t = time_pair(fns, reps, warmup)
        want = fns["gemm_i8"](0).view(torch.int16)
        same = torch.equal(want, fns["splitk_gemm_i8"](0).view(torch.int16))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        row = {"shape": shape, "scheme": "W8A8", "M": M, "N": N, "K": K, "splits": S, "workspace_bytes": ws_bytes,
               "cold_copies": n_cp, "bits_equal": same,
               "us": {k: round(v * 1e6, 2) for k, v in med.items()},
               "min_us": {k: round(min(v) * 1e6, 2) for k, v in t.items()},
               "speedup": round(med["gemm_i8"] / med["splitk_gemm_i8"], 3),
               "ring_over_splitk": round(med["gemm_i8_ring"] / med["splitk_gemm_i8"], 3),
               "bf16_over_splitk": round(med["bf16_linear"] / med["splitk_gemm_i8"], 3)}
        if "torch_int_mm" in med:
            row["splitk_over_int_mm"] = round(med["splitk_gemm_i8"] / med["torch_int_mm"], 3)
        if S > 1:
            k = kernel_shares(lambda: fns["splitk_gemm_i8"](0))
            red = [v for n, v in k.items() if "splitk_reduce" in n]
            par = [v for n, v in k.items() if "splitk_partial" in n]
            row["reduce_share"] = (round(red[0] / (red[0] + par[0]), 3) if red and par else k.get("reason", sorted(k)))
            if red and par:
                row["kernel_us"] = {"partial": round(par[0], 2), "reduce": round(red[0], 2)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del X, Xq
    del cps, cps_t, bfs
    torch.cuda.empty_cache()
    return rows


def ring_w4_rows(shape, N, K, ms, reps, warmup, dev, g):
    """qt_gemm_i8 vs qt_gemm_i8_ring_w4 at prefill sizes, W4A8 (packed int4 g128, asymmetric activations), beside the
    activation pass and bf16 F.linear."""
    rows = []
    G = K // 128
    q = torch.randint(-8, 8, (N, K), device=dev, generator=g, dtype=torch.int8)
    W0, s0, ws0 = pack_int4(q), torch.rand(N, G, device=dev, generator=g) * 1e-2, group_sums(q, G)
    del q
    nbytes = W0.numel() * 4 + s0.numel() * 4 + ws0.numel() * 4
    n_cp = max(3, -(-int(COLD_BYTES * 1.1) // nbytes))
    cps = [(W0.clone(), s0.clone(), ws0.clone()) for _ in range(n_cp)]
    n_bf = max(2, -(-int(COLD_BYTES * 1.1) // (2 * N * K)))
    bfs = [(torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16) for _ in range(n_bf)]
    for M in ms:
        X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=False)

        def call(fn, shift):
            # kernels that share a rep read different copies, or the second finds the first's weights cached
            def run(i):
                W, s, ws = cps[(i + shift) % n_cp]
                return fn(Xq, s_x, W, s, K=K, zp_x=zp_x, wsum=ws)
            return run

        fns = {"gemm_i8": call(ops.gemm_i8, 0), "gemm_i8_ring_w4": call(ops.gemm_i8_ring_w4, 1),
               "quantize_tokens": lambda i: ops.quantize_tokens_i8(X, symmetric=False),
               "bf16_linear": lambda i: F.linear(X, bfs[i % n_bf])}
        t = time_pair(fns, reps, warmup)
        same = torch.equal(fns["gemm_i8"](0).view(torch.int16), call(ops.gemm_i8_ring_w4, 0)(0).view(torch.int16))
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        ops_n = 2.0 * M * N * K
        row = {"shape": shape, "scheme": "W4A8", "M": M, "N": N, "K": K, "cold_copies": n_cp, "bits_equal": same,
               "us": {k: round(v * 1e6, 2) for k, v in med.items()},
               "min_us": {k: round(min(v) * 1e6, 2) for k, v in t.items()},
               "tops": {k: round(ops_n / v / 1e12, 1) for k, v in med.items() if k != "quantize_tokens"},
               "int8_peak_frac": {k: round(ops_n / med[k] / INT8_PEAK, 3) for k in ("gemm_i8", "gemm_i8_ring_w4")},
               "speedup": round(med["gemm_i8"] / med["gemm_i8_ring_w4"], 3),
               "bf16_over_act_plus_tiled": round(med["bf16_linear"] / (med["quantize_tokens"] + med["gemm_i8"]), 3),
               "bf16_over_act_plus_ring": round(med["bf16_linear"] / (med["quantize_tokens"] + med["gemm_i8_ring_w4"]),
                                                3)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del X, Xq
    del cps, bfs
    torch.cuda.empty_cache()
    return rows


SPLITK_MS = "129,192,256,320,384,512,640,768,1024,1536,2047"
SPLITK_SHAPES = {**SHAPES, "o": (4096, 4096), "down_70b": (8192, 28672)}
MLP_MS = "1,16,32,128,2048,8192"
MLP_HIDDEN, MLP_INTER = 4096, 14336


def mlp_rows(ms, reps, warmup, dev, g):
    """Three QuantizedLinears and torch's glue against QuantizedMLP, and the glue alone, W8A8 and W4A8, cold weights."""
    from quantool_amd.engine.qlinear import QuantizedMLP

    rows = []
    for scheme in ("W8A8", "W4A8"):
        int4 = scheme == "W4A8"

        def linear(K, N):
            q = torch.randint(-8 if int4 else -128, 8 if int4 else 128, (N, K), device=dev, generator=g,
                              dtype=torch.int8)
            s = torch.rand(N, K // 128 if int4 else 1, device=dev, generator=g) * (1e-2 if int4 else 1e-3)
            return QuantizedLinear(K, N, pack_int4(q) if int4 else q, s, act_symmetric=not int4)

        first = [linear(MLP_HIDDEN, MLP_INTER), linear(MLP_HIDDEN, MLP_INTER), linear(MLP_INTER, MLP_HIDDEN)]
        nbytes = sum(l.weight.numel() * l.weight.element_size() for l in first)
        n_cp = max(3, -(-int(COLD_BYTES * 1.1) // nbytes))
        sets = [first] + [[linear(l.in_features, l.out_features) for l in first] for _ in range(n_cp - 1)]
        fused_sets = [QuantizedMLP(*ls, torch.nn.SiLU()) for ls in sets]

        def ratios(t):
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            out = {k: {"us": round(med[k] * 1e6, 2), "min_us": round(min(v) * 1e6, 2)} for k, v in t.items()}
            out["speedup"] = round(med["unfused"] / med["fused"], 3)
            out["unfused_spread"] = round(abs(med["unfused"] / med["unfused_again"] - 1.0), 4)
            return out

        for M in ms:
            x = torch.randn(M, MLP_HIDDEN, device=dev, generator=g).to(torch.bfloat16)
            gate, up, down = first

            def unfused(i):
                ga, u, d = sets[i % n_cp]
                return d(F.silu(ga(x)) * u(x))

            def fused(i):
                return fused_sets[i % n_cp](x)

            with torch.no_grad():
                gv, uv = gate(x), up(x)

                def glue_unfused(i):
                    return ops.quantize_tokens_i8(F.silu(gv) * uv, symmetric=down.act_symmetric)

                def glue_fused(i):
                    return ops.act_mul_quantize_i8(gv, uv, symmetric=down.act_symmetric)

                for a, b in zip(glue_unfused(0), glue_fused(0)):
                    assert (a is None and b is None) or torch.equal(a, b), "the fused pass differs from the three passes"
                assert torch.equal(unfused(0).view(torch.int16), fused(0).view(torch.int16)), \
                    "QuantizedMLP differs from the three Linears"
                # forms that share a rep read different copies, or the later finds the earlier one's weights cached
                row = {"scheme": scheme, "M": M, "hidden": MLP_HIDDEN, "intermediate": MLP_INTER, "cold_copies": n_cp,
                       "bits_equal": True,
                       "glue": ratios(time_pair({"unfused": glue_unfused, "fused": glue_fused,
                                                 "unfused_again": glue_unfused}, reps, warmup)),
                       "mlp": ratios(time_pair({"unfused": unfused, "fused": lambda i: fused(i + 1),
                                                "unfused_again": lambda i: unfused(i + 2)}, reps, warmup))}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
            del x, gv, uv
        del sets, fused_sets, first
        torch.cuda.empty_cache()
    return rows


NORM_K = 4096
NORM_EPS = 1e-5


def count_kernels(fn):
    """How many device kernels one call of ``fn`` launches (torch's profiler), or the reason it could not be counted."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA and "memcpy" not in e.name.lower()]
        return {"count": len(names), "names": [n[:80] for n in names]}
    except Exception as e:  # noqa: BLE001
        return {"count": None, "reason": f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"}


def norm_rows(ms, reps, warmup, dev, g):
    """The installed RMSNorm + 3 (q/k/v) or 2 (gate/up) qt_quantize_tokens_i8 calls against one
    qt_rmsnorm_quantize_i8 launch, K = 4096, bf16."""
    from transformers.models.llama.modeling_llama import LlamaRMSNorm

    K = NORM_K
    norm = LlamaRMSNorm(K, NORM_EPS).to(dev, torch.bfloat16)
    norm.weight.data.copy_(torch.randn(K, device=dev, generator=g) * 0.5 + 1)
    w = norm.weight.detach()
    rows = []
    for M in ms:
        x = (torch.randn(M, K, device=dev, generator=g) * 3).to(torch.bfloat16)
        with torch.no_grad():
            kernels = count_kernels(lambda: norm(x))
            for symmetric in (True, False):
                want = norm(x)
                Y, Xq, s_x, zp_x = ops.rmsnorm_quantize_i8(x, w, NORM_EPS, symmetric=symmetric)
                for a, b in zip((Xq, s_x, zp_x), ops.quantize_tokens_i8(Y, symmetric=symmetric)):
                    assert (a is None and b is None) or torch.equal(a, b), "the fused rows are not the quantiser's"
                differ = int((Y.view(torch.int16) != want.view(torch.int16)).sum())
                row = {"M": M, "K": K, "symmetric": symmetric, "y_differ": differ, "y_elements": Y.numel(),
                       "torch_norm_kernels": kernels["count"]}
                for name, n in (("qkv", 3), ("gate_up", 2)):
                    def unfused(i, n=n):
                        y = norm(x)
                        return [ops.quantize_tokens_i8(y, symmetric=symmetric) for _ in range(n)]

                    def fused(i):
                        return ops.rmsnorm_quantize_i8(x, w, NORM_EPS, symmetric=symmetric)

                    t = time_pair({"unfused": unfused, "fused": fused, "unfused_again": unfused}, reps, warmup)
                    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
                    out = {k: {"us": round(med[k] * 1e6, 2), "min_us": round(min(v) * 1e6, 2)} for k, v in t.items()}
                    out["speedup"] = round(med["unfused"] / med["fused"], 3)
                    out["unfused_spread"] = round(abs(med["unfused"] / med["unfused_again"] - 1.0), 4)
                    out["launches"] = {"unfused": None if kernels["count"] is None else kernels["count"] + n, "fused": 1}
                    row[name] = out
                rows.append(row)
                print(json.dumps(row), file=sys.stderr)
        if M == ms[0]:
            print(json.dumps({"torch_norm_kernels": kernels}), file=sys.stderr)
        del x
    return rows, kernels


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
    return a.elapsed_time(b) / reps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="4096,8192")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-ring", action="store_true", help="leave out the tiled-vs-ring rows")
    ap.add_argument("--ring-only", action="store_true", help="only the tiled-vs-ring rows at M > 16")
    ap.add_argument("--mid", action="store_true", help="only the tiled-vs-mid rows (17 .. 128 rows and neighbours)")
    ap.add_argument("--mid-shapes", default=",".join(MID_SHAPES))
    ap.add_argument("--ring-w4", action="store_true", help="only the W4A8 tiled-vs-ring rows (qt_gemm_i8_ring_w4)")
    ap.add_argument("--splitk", action="store_true",
                    help="only the tiled-vs-ring-vs-split-K rows (qt_splitk_gemm_i8) at 129 .. 2047 rows")
    ap.add_argument("--splits", type=int, default=0, help="with --splitk: this S instead of the rule's")
    ap.add_argument("--mlp", action="store_true",
                    help="only the MLP rows: three QuantizedLinears + torch's glue vs QuantizedMLP (qt_act_mul_quantize_i8)")
    ap.add_argument("--norm", action="store_true",
                    help="only the norm rows: the installed RMSNorm + 3 (2) quantisers vs qt_rmsnorm_quantize_i8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qlinear_bench needs a GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    if args.norm:
        ms = [int(m) for m in (args.ms if args.ms != ap.get_default("ms") else MLP_MS).split(",") if m]
        rows, kernels = norm_rows(ms, args.reps, args.warmup, dev, g)
        print(json.dumps({"metric": "RMSNorm + per-token int8 quantisers (3: q/k/v, 2: gate/up) vs qt_rmsnorm_quantize_i8, "
                                    "K = 4096, bf16", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                          "torch_norm_kernels": kernels, "norm": rows}))
        return
    if args.mlp:
        ms = [int(m) for m in (args.ms if args.ms != ap.get_default("ms") else MLP_MS).split(",") if m]
        print(json.dumps({"metric": "Llama-3-8B MLP, A8: three QuantizedLinears + silu * up vs QuantizedMLP, cold weights",
                          "device": torch.cuda.get_device_name(0), "reps": args.reps,
                          "mlp": mlp_rows(ms, args.reps, args.warmup, dev, g)}))
        return
    if args.mid:
        mid = []
        for shape in args.mid_shapes.split(","):
            N, K = {**MID_SHAPES, **MID_EXTRA_SHAPES}[shape]
            mid += mid_rows(shape, N, K, MID_MS, args.reps, args.warmup, dev, g)
        print(json.dumps({"metric": "qt_gemm_i8 vs qt_gemm_i8_mid, 17 .. 128 rows, cold weights", "hbm_peak": HBM_PEAK,
                          "device": torch.cuda.get_device_name(0), "reps": args.reps, "mid": mid}))
        return
    if args.splitk:
        ms = [int(m) for m in (args.ms if args.ms != ap.get_default("ms") else SPLITK_MS).split(",") if m]
        shapes = args.shapes if args.shapes != ap.get_default("shapes") else "qkv,o,gate_up,down,down_70b"
        sk = []
        for shape in shapes.split(","):
            N, K = SPLITK_SHAPES[shape]
            sk += splitk_rows(shape, N, K, ms, args.splits, args.reps, args.warmup, dev, g)
        print(json.dumps({"metric": "qt_gemm_i8 vs qt_gemm_i8_ring vs qt_splitk_gemm_i8, W8A8, 129 .. 2047 rows, cold "
                                    "weights", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                          "cus": torch.cuda.get_device_properties(0).multi_processor_count,
                          "splits_forced": args.splits, "splitk": sk}))
        return
    if args.ring_w4:
        ms = [int(m) for m in (args.ms if args.ms != ap.get_default("ms") else "2048,4096,8192").split(",") if m]
        w4 = []
        for shape in args.shapes.split(","):
            N, K = SHAPES[shape]
            w4 += ring_w4_rows(shape, N, K, ms, args.reps, args.warmup, dev, g)
        print(json.dumps({"metric": "qt_gemm_i8 vs qt_gemm_i8_ring_w4, W4A8 prefill sizes, cold weights",
                          "int8_peak": INT8_PEAK, "device": torch.cuda.get_device_name(0), "reps": args.reps,
                          "ring_w4": w4}))
        return
    rows = []
    int_mm_note = None
    all_ms = [int(m) for m in args.ms.split(",") if m]
    decode_ms = [m for m in all_ms if m <= DECODE_MAX_M]
    large_ms = [m for m in all_ms if m > DECODE_MAX_M]
    decode = []
    ring = []
    for shape in args.shapes.split(","):
        N, K = SHAPES[shape]
        if decode_ms:
            decode += decode_rows(shape, N, K, decode_ms, args.reps, args.warmup, dev, g)
        if not large_ms:
            continue
        if not args.no_ring and K % ops.I8_RING_K_UNIT == 0:
            ring += ring_rows(shape, N, K, large_ms, args.reps, args.warmup, dev, g)
        if args.ring_only:
            continue
        q8 = torch.randint(-128, 128, (N, K), device=dev, generator=g, dtype=torch.int8)
        q4 = torch.randint(-8, 8, (N, K), device=dev, generator=g, dtype=torch.int8)
        w4 = pack_int4(q4)
        s_w1 = torch.rand(N, 1, device=dev, generator=g) * 1e-3
        s_wg = torch.rand(N, K // 128, device=dev, generator=g) * 1e-2
        wsum_g = group_sums(q4, K // 128)
        lin8 = QuantizedLinear(K, N, q8, s_w1, act_symmetric=True)
        lin4 = QuantizedLinear(K, N, w4, s_wg, act_symmetric=False)
        Wbf = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        for M in large_ms:
            X = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
            Xq, s_x, _ = ops.quantize_tokens_i8(X, symmetric=True)
            Xqa, s_xa, zp_xa = ops.quantize_tokens_i8(X, symmetric=False)
            t = {
                "act_sym": _time(lambda: ops.quantize_tokens_i8(X, symmetric=True), args.reps, args.warmup),
                "act_asym": _time(lambda: ops.quantize_tokens_i8(X, symmetric=False), args.reps, args.warmup),
                "gemm_w8a8": _time(lambda: ops.gemm_i8(Xq, s_x, q8, s_w1), args.reps, args.warmup),
                "gemm_w4a8": _time(lambda: ops.gemm_i8(Xqa, s_xa, w4, s_wg, K=K, zp_x=zp_xa, wsum=wsum_g),
                                   args.reps, args.warmup),
                "linear_w8a8": _time(lambda: lin8(X), args.reps, args.warmup),
                "linear_w4a8": _time(lambda: lin4(X), args.reps, args.warmup),
                "bf16_linear": _time(lambda: F.linear(X, Wbf), args.reps, args.warmup),
            }
            try:
                qt = q8.t()
                torch._int_mm(Xq, qt)
                t["torch_int_mm"] = _time(lambda: torch._int_mm(Xq, qt), args.reps, args.warmup)
            except Exception as e:  # noqa: BLE001
                int_mm_note = f"torch._int_mm does not run here: {type(e).__name__}: {str(e).splitlines()[0][:160]}"
            ops_n = 2.0 * M * N * K
            act_bytes = M * K * 2 + M * K + M * 8
            row = {"shape": shape, "M": M, "N": N, "K": K, "ms": {k: round(v * 1e3, 4) for k, v in t.items()},
                   "tops": {k: round(ops_n / t[k] / 1e12, 1) for k in t if not k.startswith("act")},
                   "int8_peak_frac": {k: round(ops_n / t[k] / INT8_PEAK, 3) for k in ("gemm_w8a8", "gemm_w4a8")},
                   "act_GBps": {k: round(act_bytes / t[k] / 1e9, 1) for k in ("act_sym", "act_asym")},
                   "bf16_over_w8a8": round(t["bf16_linear"] / t["linear_w8a8"], 3),
                   "bf16_over_w4a8": round(t["bf16_linear"] / t["linear_w4a8"], 3)}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr)
            del X, Xq, Xqa
        del q8, q4, w4, lin8, lin4, Wbf
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "W8A8 / W4A8 linear vs bf16 F.linear, Llama-3-8B prefill shapes", "int8_peak": INT8_PEAK,
                      "torch_int_mm": int_mm_note or "runs (timed as torch_int_mm)", "rows": rows,
                      "hbm_peak": HBM_PEAK, "device": torch.cuda.get_device_name(0), "decode": decode, "ring": ring}))


if __name__ == "__main__":
    main()
