"""evaluate.perplexity on a W8A8 checkpoint with and without the LDS-ring GEMM (QuantizedLinear.ring_min_m).

  python tools/ppl_bench.py <dir> [--layers 8] [--batch 8] [--seq 2048]

The checkpoint is the random-init Llama-3-8B-shaped RTN W8A8 model of tools/decode_bench.py (written to <dir> when it
is not there yet).  One loaded model runs ``perplexity`` over --batch x --seq random tokens as ``tiled``
(``ring_min_m = 0``) and ``ring`` (the class default), each twice after one warm-up pass; wall seconds with the device
synchronised.  The Linears agree to the bit, so the perplexities must be equal as floats.  Prints one JSON line.
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppl_bench needs a GPU")
    dev = torch.device("cuda:0")
    path = Path(args.checkpoint)
    if not (path / "config.json").exists():
        write_checkpoint(path, args.layers, dev, "W8A8")
    model = load_quantized(path, device=dev)
    ids = torch.randint(0, model.config.vocab_size, (args.batch, args.seq), generator=torch.Generator().manual_seed(0))
    default = QuantizedLinear.ring_min_m
    result = {"metric": "evaluate.perplexity wall seconds, W8A8, ring_min_m = 0 vs default", "layers": args.layers,
              "tokens": args.batch * args.seq, "ring_min_m": default, "device": torch.cuda.get_device_name(0),
              "quantized_linears": sum(isinstance(m, QuantizedLinear) for m in model.modules()), "modes": {}}
    try:
        for rep in range(3):                                   # pass 0 warms up; both modes twice: the spread
            for mode, setting in (("tiled", 0), ("ring", default)):
                QuantizedLinear.ring_min_m = setting
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
        QuantizedLinear.ring_min_m = default
    t, r = (min(result["modes"][m]["seconds"]) for m in ("tiled", "ring"))
    result["perplexities_equal"] = result["modes"]["tiled"]["perplexity"] == result["modes"]["ring"]["perplexity"]
    result["speedup"] = round(t / r, 3)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
