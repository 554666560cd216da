"""evaluate.perplexity on a W8A8 / W4A8 checkpoint with and without the LDS-ring GEMM (QuantizedLinear.ring_min_m,
or ring_w4_min_m for W4A8).

  python tools/ppl_bench.py <dir> [--layers 8] [--batch 8] [--seq 2048] [--scheme W8A8|W4A8] [--ring-min-m M]
  python tools/ppl_bench.py <dir> --layers 8 --batch 1 --seq 512 --splitk-min-m      # the split-K form at a short prompt

The checkpoint is the random-init Llama-3-8B-shaped RTN model of tools/decode_bench.py in that scheme (written to <dir>
when it is not there yet).  One loaded model runs ``perplexity`` over --batch x --seq random tokens as ``tiled`` (the
attribute at 0) and ``ring`` (the class default, or --ring-min-m: the way to time a ring that ships turned off), each
twice after one warm-up pass; wall seconds with the device synchronised.  With --splitk-min-m [M] the attribute that is
switched is ``splitk_min_m`` instead (W8A8; 0 against the class default or M; the second mode is still called "ring").  The Linears agree to the bit, so the perplexities must be equal as floats.  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from decode_bench import write_checkpoint  # noqa: E402

from quantool_amd.engine.qlinear import QuantizedLinear, load_quantized  # noqa: E402
from quantool_amd.evaluate import perplexity  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--scheme", default="W8A8", choices=["W8A8", "W4A8"])
    ap.add_argument("--ring-min-m", type=int, default=None, help="the 'ring' mode's attribute value (default: the class's)")
    ap.add_argument("--splitk-min-m", type=int, nargs="?", const=-1, default=None,
                    help="switch splitk_min_m (0 vs the class default, or vs M) instead of the ring's attribute")
    ap.add_argument("--splitk-min-k", type=int, default=None, help="with --splitk-min-m: splitk_min_k for both modes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppl_bench needs a GPU")
    dev = torch.device("cuda:0")
    path = Path(args.checkpoint)
    if not (path / "config.json").exists():
        write_checkpoint(path, args.layers, dev, args.scheme)
    model = load_quantized(path, device=dev)
    ids = torch.randint(0, model.config.vocab_size, (args.batch, args.seq), generator=torch.Generator().manual_seed(0))
    attr = "ring_min_m" if args.scheme == "W8A8" else "ring_w4_min_m"
    default = getattr(QuantizedLinear, attr)
    ring = default if args.ring_min_m is None else args.ring_min_m
    if args.splitk_min_m is not None:
        attr, default = "splitk_min_m", QuantizedLinear.splitk_min_m
        ring = default if args.splitk_min_m < 0 else args.splitk_min_m
        if args.splitk_min_k is not None:
            QuantizedLinear.splitk_min_k = args.splitk_min_k
    result = {"metric": f"evaluate.perplexity wall seconds, {args.scheme}, {attr} = 0 vs {ring}", "layers": args.layers,
              "tokens": args.batch * args.seq, "seq": args.seq, attr: ring, "class_default": default,
              "splitk_min_k": QuantizedLinear.splitk_min_k,
              "device": torch.cuda.get_device_name(0),
              "quantized_linears": sum(isinstance(m, QuantizedLinear) for m in model.modules()), "modes": {}}
    try:
        for rep in range(3):                                   # pass 0 warms up; both modes twice: the spread
            for mode, setting in (("tiled", 0), ("ring", ring)):
                setattr(QuantizedLinear, attr, setting)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ppl = perplexity(model, ids, batch_size=args.batch)["perplexity"]
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                m = result["modes"].setdefault(mode, {"seconds": [], "perplexity": ppl})
                assert m["perplexity"] == ppl, f"{mode}: two runs gave different perplexities"
                if rep:
                    m["seconds"].append(round(dt, 4))
    finally:
        setattr(QuantizedLinear, attr, default)
    t, r = (min(result["modes"][m]["seconds"]) for m in ("tiled", "ring"))
    result["perplexities_equal"] = result["modes"]["tiled"]["perplexity"] == result["modes"]["ring"]["perplexity"]
    result["speedup"] = round(t / r, 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
