"""W8A8 / W4A8 linear on the int8 MFMA vs bf16 F.linear at Llama-3-8B's prefill shapes.

  python tools/qlinear_bench.py [--ms 4096,8192] [--reps 20] [--warmup 5]

Per shape (q/k/v fused N = 6144, K = 4096; gate/up N = 28672, K = 4096; down N = 4096, K = 14336) and M: device time
(HIP events, mean over --reps after --warmup) of the activation pass (qt_quantize_tokens_i8), the GEMM (qt_gemm_i8:
W8A8 = int8 channel-wise weights, symmetric activations; W4A8 = packed int4 g128 weights, asymmetric activations),
QuantizedLinear end to end, bf16 F.linear and torch._int_mm (when this torch build runs it; else the reason).
Prints one JSON line: TOPS (2 M N K / time), the share of the 5 PF int8 dense peak, the activation pass's GB/s and the
ratio of bf16 F.linear time to the W8A8 / W4A8 QuantizedLinear time (> 1: the quantized linear is faster).
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qlinear_bench needs a GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []
    int_mm_note = None
    for shape in args.shapes.split(","):
        N, K = SHAPES[shape]
        q8 = torch.randint(-128, 128, (N, K), device=dev, generator=g, dtype=torch.int8)
        q4 = torch.randint(-8, 8, (N, K), device=dev, generator=g, dtype=torch.int8)
        w4 = pack_int4(q4)
        s_w1 = torch.rand(N, 1, device=dev, generator=g) * 1e-3
        s_wg = torch.rand(N, K // 128, device=dev, generator=g) * 1e-2
        wsum_g = group_sums(q4, K // 128)
        lin8 = QuantizedLinear(K, N, q8, s_w1, act_symmetric=True)
        lin4 = QuantizedLinear(K, N, w4, s_wg, act_symmetric=False)
        Wbf = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(torch.bfloat16)
        for M in (int(m) for m in args.ms.split(",")):
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
                      "torch_int_mm": int_mm_note or "runs (timed as torch_int_mm)", "rows": rows}))


if __name__ == "__main__":
    main()
