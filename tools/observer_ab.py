#!/usr/bin/env python3
"""The MSE weight observer next to the min/max one.  Two records, one JSON file:
  * launch time of ``qt_weight_gather_qparams_mse`` beside ``qt_weight_gather_qparams`` on the same inputs, interleaved,
    for the seven Linears of a Llama-3-8B layer (W4A16 g128, bf16) and one W8A16 channel-wise case;
  * the GPTQ sweep's summed loss on one 4096 x 4096 Linear (student-t weights, a well-conditioned random Hessian) with
    min/max tables and with MSE tables.
usage: observer_ab.py out.json [repeats]"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from quantool_amd.engine.gptq_linear import HessianAccumulator, gptq_quantize_shared
from quantool_amd.engine.schemes import QuantArgs
from quantool_amd.hip import ops

LINEARS = [("q", 4096, 4096), ("k", 1024, 4096), ("v", 1024, 4096), ("o", 4096, 4096), ("gate", 14336, 4096),
           ("up", 14336, 4096), ("down", 4096, 14336)]


def student_t(R, K, dev, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(R, K, generator=g)
    chi2 = torch.randn(3, R, K, generator=g).square().sum(0)
    return (z / (chi2 / 3.0).sqrt() * 0.02).to(torch.bfloat16).to(dev)


def time_pair(W, group_size, bits, repeats):
    R, K = W.shape
    dev = W.device
    G = 1 if group_size <= 0 else K // group_size
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K)).to(torch.int32).to(dev)
    dead = torch.zeros(K, dtype=torch.uint8, device=dev)
    out = torch.empty((R, K), dtype=torch.float32, device=dev)
    sc, zp = (torch.empty((R, G), dtype=torch.float32, device=dev) for _ in range(2))
    sct, zpt = (torch.empty((G, R), dtype=torch.float32, device=dev) for _ in range(2))
    ms = {"minmax": [], "mse": []}
    for rd in range(repeats + 2):                       # two warm-up rounds
        for name, fn in (("minmax", ops.weight_gather_qparams), ("mse", ops.weight_gather_qparams_mse)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(W, perm, dead, group_size, True, bits, out, sc, zp, sct, zpt)
            e1.record()
            torch.cuda.synchronize()
            if rd >= 2:
                ms[name].append(e0.elapsed_time(e1))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return {"R": R, "K": K, "group_size": group_size, "num_bits": bits, "minmax_ms": round(med["minmax"], 4),
            "mse_ms": round(med["mse"], 4), "minmax_ms_min": round(min(ms["minmax"]), 4), "mse_ms_min": round(min(ms["mse"]), 4)}


def main():
    out_path = Path(sys.argv[1])
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda:0")
    launches = []
    for name, R, K in LINEARS:
        launches.append(dict(time_pair(student_t(R, K, dev, R + K), 128, 4, repeats), linear=name, scheme="W4A16"))
        print(launches[-1], flush=True)
    launches.append(dict(time_pair(student_t(4096, 4096, dev, 1), -1, 8, repeats), linear="q", scheme="W8A16"))
    print(launches[-1], flush=True)

    K = 4096
    W = student_t(4096, K, dev, 7)
    acc = HessianAccumulator(K, dev)
    acc.add(torch.randn(4 * K, K, generator=torch.Generator().manual_seed(8)).to(torch.bfloat16).to(dev))
    loss = {}
    for observer in ("minmax", "mse"):
        res = gptq_quantize_shared([W], acc, QuantArgs(actorder="static", observer=observer))[0]
        loss[observer] = float(res.loss.double().sum().item())
    print(loss, flush=True)
    record = {"device": torch.cuda.get_device_name(0), "repeats": repeats, "timing": "device events, median (and minimum)",
              "launches": launches, "sweep_loss_4096x4096_W4A16_g128": dict(loss, ratio=loss["mse"] / loss["minmax"])}
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
