#!/usr/bin/env python3
"""The streamed placement against the resident one on a random-init model handed over on the HOST (no download):
GPTQ W4A16 g128 through the quantool plugin API, as tools/full_model.py runs it.

usage: stream_model.py shape layers mode [samples [seq]]
  shape   8b | 70b (Llama-3 dimensions) | 405b (Llama-3.1-405B) | mixtral-8x22b
  layers  decoder layers; "fit" = the fewest layers whose weights exceed the free device memory, "estimate" = the fewest
          whose weights plus the estimated resident working set do (either capped at half of the host's memory)
  mode    stream (the free-bytes probe says nothing fits) | resident (it says everything fits) | auto (the real probe)

The model is built on the meta device and filled layer by layer from device-side random numbers, so a model larger
than the device never has to exist there.  Prints quantize() wall time, the peak allocated device memory, the bytes
moved each way with the achieved rate against the 63 GB/s of PCIe Gen5 x16, and (QT_CALIB_TIMING=1) the exposed
onload / write-back phases; then reads one packed Linear back from the checkpoint.  Numbers: profiles/r05_streamed.txt."""
import json
import logging
import os
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
os.environ.setdefault("QT_CALIB_TIMING", "1")
import torch

import quantool_amd.methods  # noqa: F401
from quantool_amd.core import QuantizerRegistry
from quantool_amd.engine import placement

logging.basicConfig(level=logging.WARNING)
shape, layers_arg, mode = sys.argv[1], sys.argv[2], sys.argv[3]
n_samples = int(sys.argv[4]) if len(sys.argv) > 4 else 512
seq = int(sys.argv[5]) if len(sys.argv) > 5 else 384
dev = torch.device("cuda:0")
PCIE = 63e9


def mem_available() -> int:
    for line in Path("/proc/meminfo").read_text().splitlines():
        if line.startswith("MemAvailable:"):
            return int(line.split()[1]) * 1024
    return 0


def config(n_layers):
    if shape == "mixtral-8x22b":
        from transformers import MixtralConfig, MixtralForCausalLM

        return MixtralForCausalLM, MixtralConfig(
            hidden_size=6144, intermediate_size=16384, num_hidden_layers=n_layers, num_attention_heads=48,
            num_key_value_heads=8, num_local_experts=8, num_experts_per_tok=2, vocab_size=32768,
            max_position_embeddings=8192, rope_theta=1e6, rms_norm_eps=1e-5, tie_word_embeddings=False)
    from transformers import LlamaConfig, LlamaForCausalLM

    hidden, inter, heads = {"8b": (4096, 14336, 32), "70b": (8192, 28672, 64), "405b": (16384, 53248, 128)}[shape]
    return LlamaForCausalLM, LlamaConfig(
        hidden_size=hidden, intermediate_size=inter, num_hidden_layers=n_layers, num_attention_heads=heads,
        num_key_value_heads=8, vocab_size=128256, max_position_embeddings=8192, rope_theta=500000.0,
        rms_norm_eps=1e-5, tie_word_embeddings=False)


def build(n_layers):
    cls, cfg = config(n_layers)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device("meta"):
            model = cls(cfg)
    finally:
        torch.set_default_dtype(prev)
    model.to_empty(device="cpu")
    inner = model.model
    inner.rotary_emb = type(inner.rotary_emb)(config=cfg)          # non-persistent buffers: computed, not random
    g = torch.Generator(device=dev).manual_seed(0)
    for name, p in model.named_parameters():
        if p.dim() == 1:
            p.data.fill_(1.0)
            continue
        flat = p.data.view(-1)
        step = 1 << 28
        for a in range(0, flat.numel(), step):
            n = min(step, flat.numel() - a)
            flat[a:a + n].copy_((torch.randn(n, device=dev, generator=g) * 0.02).to(torch.bfloat16))
    torch.cuda.synchronize()
    return model.eval(), cfg


free = torch.cuda.mem_get_info(dev)[0]
host = mem_available()
if layers_arg in ("fit", "estimate"):
    # "fit": the weights alone exceed the free device memory; "estimate": the weights plus the resident working set
    # (placement.calibration_bytes) do -- what the decision compares.  Either under half of the host memory a command
    # may use (MemAvailable, or the cgroup's limit when lower)
    from quantool_amd.engine.schemes import QuantArgs

    cg = Path("/sys/fs/cgroup/memory.max")
    if cg.exists() and cg.read_text().strip().isdigit():
        host = min(host, int(cg.read_text()))
    cls, cfg = config(1)
    with torch.device("meta"):
        m1 = cls(cfg)
    per_layer = sum(p.numel() * 2 for p in m1.model.layers[0].parameters())
    rest = sum(p.numel() * 2 for n_, p in m1.named_parameters() if ".layers." not in n_)
    n_layers = 1
    while True:
        need = rest + n_layers * per_layer
        if layers_arg == "estimate":
            one = placement.layer_shape(list(m1.model.layers))
            need += placement.calibration_bytes(type(one)(one.name, n_layers, one.groups), cfg.hidden_size,
                                                n_samples * seq, QuantArgs())
        if need > free:
            break
        n_layers += 1
    cap = (host // 2 - rest) // per_layer
    print(f"free device memory {free / 1e9:.1f} GB, host memory {host / 1e9:.1f} GB: {n_layers} layers of "
          f"{per_layer / 1e9:.2f} GB exceed the device ({layers_arg}; host cap {cap} layers)", flush=True)
    if n_layers > cap:
        sys.exit(f"the host cannot hold {n_layers} layers under half of its memory")
else:
    n_layers = int(layers_arg)
t0 = time.perf_counter()
model, cfg = build(n_layers)
pbytes = sum(p.numel() * p.element_size() for p in model.parameters())
lbytes = sum(p.numel() * p.element_size() for p in model.model.layers.parameters())
print(f"model: {shape}-shaped, {n_layers} layers, {pbytes / 1e9:.1f} GB of bf16 parameters ({lbytes / 1e9:.1f} GB in "
      f"the decoder layers) on the host, built in {time.perf_counter() - t0:.1f} s; free device memory "
      f"{free / 1e9:.1f} GB, host MemAvailable {host / 1e9:.1f} GB", flush=True)
if mode != "auto":
    placement.free_device_bytes = (lambda d: 1) if mode == "stream" else (lambda d: 1 << 62)
if mode == "resident":      # handed over on the device, as tools/full_model.py does: the timed run moves nothing
    model.to(dev)

g = torch.Generator().manual_seed(0)
data = [{"input_ids": torch.randint(0, cfg.vocab_size, (seq,), generator=g)} for _ in range(n_samples)]
with tempfile.TemporaryDirectory(dir=os.environ.get("QT_FULL_MODEL_OUT")) as tmp:
    q = QuantizerRegistry.create("gptq", model_id=f"synthetic/{shape}-shaped")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    q.quantize(model=model, level="W4A16", dataset=data, num_calibration_samples=n_samples, max_seq_length=seq,
               oneshot_kwargs={"output_dir": tmp + "/work"})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = model._qt_placement
    print(f"gptq W4A16 {st['mode']}: quantize() {dt:.2f} s wall ({dt / n_layers:.3f} s per decoder layer), "
          f"{n_samples} samples x {seq} tokens", flush=True)
    print(f"peak GPU memory {torch.cuda.max_memory_allocated(dev) / 2**30:.1f} GiB allocated, "
          f"{torch.cuda.max_memory_reserved(dev) / 2**30:.1f} GiB reserved; one decoder layer "
          f"{lbytes / n_layers / 2**30:.2f} GiB", flush=True)
    if st["mode"] == "stream":
        for d, ms in (("h2d", st["ms_h2d"]), ("d2h", st["ms_d2h"])):
            b = st[f"bytes_{d}"]
            rate = b / (ms / 1e3) if ms else float("nan")
            print(f"{d}: {b / 1e9:.1f} GB in {ms / 1e3:.2f} s of copy-stream time = {rate / 1e9:.1f} GB/s "
                  f"({100 * rate / PCIE:.0f} % of {PCIE / 1e9:.0f} GB/s)", flush=True)
        print(f"pinned staging {st['pinned_bytes'] / 2**30:.2f} GiB", flush=True)
    name = f"model.layers.{n_layers - 1}.self_attn.o_proj"
    saved = Path(tmp) / "work"
    from safetensors import safe_open

    idx = saved / "model.safetensors.index.json"
    fname = json.loads(idx.read_text())["weight_map"][name + ".weight_packed"] if idx.exists() else "model.safetensors"
    with safe_open(str(saved / fname), framework="pt") as f:
        state = {k: f.get_tensor(k) for k in f.keys() if k.startswith(name + ".")}
    packed, scale = state[name + ".weight_packed"], state[name + ".weight_scale"].float()
    wshape = state[name + ".weight_shape"].tolist()
    nib = torch.stack([(packed >> (4 * j)) & 0xF for j in range(8)], dim=-1).reshape(packed.shape[0], -1)[:, :wshape[1]]
    w = (nib.to(torch.int32) - 8).float()
    gs = wshape[1] // scale.shape[1]
    w = (w.reshape(wshape[0], -1, gs) * scale[:, :, None]).reshape(wshape[0], wshape[1])
    ref = model.get_submodule(name).weight.detach().float()
    print(f"read-back of {name}: {tuple(wshape)}, weight on {ref.device}, max |dequant(packed) - written-back weight| "
          f"= {float((w - ref.cpu()).abs().max()):.3e} (bf16 rounding: <= {float(ref.abs().max()) * 2 ** -8:.1e})",
          flush=True)
