"""Perplexity of a saved checkpoint (any scheme this backend writes) on stored token ids.

  python tools/eval_checkpoint.py <checkpoint dir> --tokens ids.pt [--batch-size 8] [--dtype bfloat16]
                                  [--a16 dequantized|packed] [--a16-experts dequantized|packed]
                                  [--a16-stream-rows N] [--a16-experts-wide-tokens N] [--a8-fused-act]
                                  [--a8-fused-norm] [--head logits|fused] [--against REF]

``ids.pt`` holds a [B, T] integer tensor or a list of 1-d tensors (``torch.save``).  W8A8 / INT8 / W4A8 checkpoints run
on the int8 kernels (activations quantised per token), A16 checkpoints on their dequantised weights (``--a16 packed``:
on ``WeightOnlyLinear``s that keep the integer weights; ``--a16-experts packed`` with it: routed-expert banks on
``WeightOnlyExperts``; ``--a16-stream-rows N`` with it: inputs of 17 to N rows on ``qt_gemm_wq_stream``;
``--a16-experts-wide-tokens N`` with ``--a16-experts packed``: calls of 129 to N tokens on ``qt_moe_gemm_wq_wide``;
``--a8-fused-act`` on an A8 checkpoint: SiLU(gate) * up and the quantiser of the down product in one
``qt_act_mul_quantize_i8`` pass, the same perplexity to the bit; ``--a8-fused-norm`` on an A8 checkpoint: the RMSNorms in
front of q/k/v and gate/up and the quantiser their consumers share in one ``qt_rmsnorm_quantize_i8`` pass each, whose sum
over K runs in the kernel's own order, so the perplexity may move in its last digits).  ``--against REF`` (the original
model: a dense checkpoint directory, or a quantised one) adds ``"divergence"``: what ``evaluate.divergence(REF,
checkpoint)`` returns on the same tokens -- the mean and maximum per-token KL(REF || checkpoint), the top-1 agreement and
both perplexities through one ``qt_lm_head_kl`` pass per batch -- with its wall time and peak allocated memory.  Prints
one JSON line: perplexity, mean NLL, predicted tokens, the module counts, load and evaluation wall times.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from quantool_amd.engine.qlinear import (A16_MODES, QuantizedLinear, QuantizedMLP, QuantizingRMSNorm,  # noqa: E402
                                         WeightOnlyExperts, WeightOnlyLinear, load_quantized)
from quantool_amd.evaluate import divergence, load_side, perplexity  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--tokens", required=True)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--dtype", default=None, choices=[None, "bfloat16", "float16"])
    ap.add_argument("--a16", default="dequantized", choices=list(A16_MODES))
    ap.add_argument("--a16-experts", default="dequantized", choices=list(A16_MODES))
    ap.add_argument("--a16-stream-rows", type=int, default=0,
                    help="with --a16 packed: inputs of 17 to this many rows (at most 128) run qt_gemm_wq_stream")
    ap.add_argument("--a16-experts-wide-tokens", type=int, default=0,
                    help="with --a16-experts packed: calls of 129 to this many tokens route their rows and run "
                         "qt_moe_gemm_wq_wide instead of dequantising the banks")
    ap.add_argument("--a8-fused-act", action="store_true",
                    help="A8 checkpoints: run every MLP's and expert bank's glue as one qt_act_mul_quantize_i8 pass")
    ap.add_argument("--a8-fused-norm", action="store_true",
                    help="A8 checkpoints: run the RMSNorm in front of q/k/v and gate/up and their shared quantiser as one "
                         "qt_rmsnorm_quantize_i8 pass")
    ap.add_argument("--head", default="logits", choices=["logits", "fused"],
                    help="fused: the LM head and its cross-entropy run as one qt_lm_head_nll pass, no [B, T, V] logits")
    ap.add_argument("--against", default=None, metavar="REF",
                    help="the original model's directory: adds evaluate.divergence(REF, checkpoint) on the same tokens")
    args = ap.parse_args()
    ids = torch.load(args.tokens)
    t0 = time.perf_counter()
    model = load_quantized(args.checkpoint, device=args.device,
                           dtype=getattr(torch, args.dtype) if args.dtype else None, a16=args.a16,
                           a16_experts=args.a16_experts, a16_stream_rows=args.a16_stream_rows,
                           a16_experts_wide_tokens=args.a16_experts_wide_tokens, a8_fused_act=args.a8_fused_act,
                           a8_fused_norm=args.a8_fused_norm)
    if args.device.startswith("cuda"):
        torch.cuda.synchronize()
    t1 = time.perf_counter()
    if args.device.startswith("cuda"):
        torch.cuda.reset_peak_memory_stats()
    r = perplexity(model, ids, batch_size=args.batch_size, head=args.head)
    if args.device.startswith("cuda"):
        torch.cuda.synchronize()
        r["eval_peak_bytes"] = torch.cuda.max_memory_allocated()
    t2 = time.perf_counter()
    r.update({"checkpoint": str(args.checkpoint), "format": model._qt_checkpoint["format"],
              "quantized_linears": sum(isinstance(m, QuantizedLinear) for m in model.modules()),
              "quantized_mlps": sum(isinstance(m, QuantizedMLP) for m in model.modules()),
              "quantizing_norms": sum(isinstance(m, QuantizingRMSNorm) for m in model.modules()),
              "weight_only_linears": sum(isinstance(m, WeightOnlyLinear) for m in model.modules()),
              "weight_only_expert_banks": sum(isinstance(m, WeightOnlyExperts) for m in model.modules()),
              "head": args.head, "load_s": round(t1 - t0, 3), "eval_s": round(t2 - t1, 3)})
    if args.against:
        t3 = time.perf_counter()
        ref = load_side(args.against, args.device, getattr(torch, args.dtype) if args.dtype else None)
        if args.device.startswith("cuda"):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
        t4 = time.perf_counter()
        d = divergence(ref, model, ids, batch_size=args.batch_size)
        if args.device.startswith("cuda"):
            torch.cuda.synchronize()
            d["eval_peak_bytes"] = torch.cuda.max_memory_allocated()
        d.update({"against": str(args.against), "load_s": round(t4 - t3, 3),
                  "eval_s": round(time.perf_counter() - t4, 3)})
        r["divergence"] = d
    print(json.dumps(r))


if __name__ == "__main__":
    main()
