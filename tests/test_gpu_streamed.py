"""The streamed placement on the GPU: a model handed over on the host, forced to stream by a free-bytes probe that says
nothing fits, gives the checkpoint a resident run of the same seed gives, bit for bit, stays on the host with the same
dequantised weights, and keeps the device peak far below its decoder layers."""
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu


def _tiny_llama(layers=8, hidden=256, inter=512, heads=4, kv=2):
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads,
                      num_key_value_heads=kv, vocab_size=512, max_position_embeddings=128, tie_word_embeddings=False)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).eval()


def _tiny_mixtral(layers=8):
    from transformers import MixtralConfig, MixtralForCausalLM

    cfg = MixtralConfig(hidden_size=256, intermediate_size=256, num_hidden_layers=layers, num_attention_heads=4,
                        num_key_value_heads=2, num_local_experts=4, num_experts_per_tok=2, vocab_size=512,
                        max_position_embeddings=128, tie_word_embeddings=False)
    torch.manual_seed(0)
    return MixtralForCausalLM(cfg).to(torch.bfloat16).eval()


def _data(n=8, seq=48):
    g = torch.Generator().manual_seed(1)
    return [{"input_ids": torch.randint(0, 512, (seq,), generator=g)} for _ in range(n)]


def _checkpoint(path):
    from safetensors.torch import load_file

    state = {}
    for f in sorted(Path(path).glob("*.safetensors")):
        state.update(load_file(str(f)))
    return state, json.loads((Path(path) / "config.json").read_text())


def _force(monkeypatch, stream: bool):
    from quantool_amd.engine import placement

    monkeypatch.setattr(placement, "free_device_bytes", (lambda dev: 1) if stream else (lambda dev: 1 << 60))


def _oneshot(model, recipe, out, monkeypatch, stream):
    from quantool_amd.engine.oneshot import oneshot

    _force(monkeypatch, stream)
    res = oneshot(model=model, dataset=_data(), recipe=recipe, output_dir=str(out), num_calibration_samples=8,
                  max_seq_length=64, shuffle_calibration_samples=False)
    torch.cuda.synchronize()
    return res


def _recipe(kind):
    from quantool_amd.engine.modifiers import AWQModifier, GPTQModifier, SmoothQuantModifier

    return {"gptq-w4a16-group": lambda: GPTQModifier(scheme="W4A16", actorder="group"),
            "smoothquant-gptq-w8a8": lambda: [SmoothQuantModifier(smoothing_strength=0.5), GPTQModifier(scheme="W8A8")],
            "awq-w4a16-asym": lambda: AWQModifier(scheme="W4A16_ASYM"),
            "mixtral-gptq-w4a16": lambda: GPTQModifier(scheme="W4A16")}[kind]()


@pytest.mark.parametrize("kind", ["gptq-w4a16-group", "smoothquant-gptq-w8a8", "awq-w4a16-asym",
                                  "mixtral-gptq-w4a16"])
def test_streamed_run_equals_resident_run(dev, tmp_path, monkeypatch, kind):
    make = _tiny_mixtral if kind.startswith("mixtral") else _tiny_llama
    resident = _oneshot(make(), _recipe(kind), tmp_path / "resident", monkeypatch, stream=False)
    assert resident._qt_placement["mode"] == "resident"

    model = make()
    fused = model.model.layers[0].mlp.experts.gate_up_proj if kind.startswith("mixtral") else None
    streamed = _oneshot(model, _recipe(kind), tmp_path / "streamed", monkeypatch, stream=True)
    assert streamed is model and model._qt_placement["mode"] == "stream"
    stats = model._qt_placement
    layer_bytes = sum(p.numel() * p.element_size() for layer in model.model.layers for p in layer.parameters())
    assert stats["bytes_h2d"] == layer_bytes and stats["bytes_d2h"] > layer_bytes

    a, cfg_a = _checkpoint(tmp_path / "resident")
    b, cfg_b = _checkpoint(tmp_path / "streamed")
    assert cfg_a == cfg_b
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k

    pa, pb = dict(resident.named_parameters()), dict(model.named_parameters())
    assert sorted(pa) == sorted(pb)
    for n, p in pb.items():
        assert p.device.type == "cpu", n
        assert torch.equal(p.data, pa[n].data.cpu()), n
    for n, t in model.named_buffers():
        assert t.device.type == "cpu", n
    if fused is not None:       # the expert Linears still view the caller's fused parameter, which holds the result
        lin = model.model.layers[0].mlp.experts.experts[1].gate_up_proj.weight
        assert lin.untyped_storage().data_ptr() == fused.untyped_storage().data_ptr() and fused.device.type == "cpu"
    # the results live on the host; dequantized() still runs the device kernel and hands back a host tensor
    name = "model.layers.0.self_attn.q_proj"
    r = model._qt_results[name]
    assert r.weight_scale.device.type == "cpu"
    if r.Qt is not None:
        assert torch.equal(r.dequantized(torch.bfloat16), resident._qt_results[name].dequantized(torch.bfloat16).cpu())


def test_streamed_device_peak_stays_far_below_the_layers(dev, tmp_path, monkeypatch):
    from quantool_amd.engine.gptq_linear import HessianAccumulator

    # 48 layers of hidden 2048: 3.3 GB of decoder weights.  The working set has parts of a fixed size (the Cholesky
    # workspace is ~140 MB per problem of a batched chain) and the accumulators' token buffers (1 GiB worth of rows, at
    # least 4096 tokens); a small buffer and enough layers keep the working set at a real model's ratio
    monkeypatch.setattr(HessianAccumulator, "STAGE_BYTES", 4 << 20)
    model = _tiny_llama(layers=48, hidden=2048, inter=4096, heads=16, kv=4)
    layer_bytes = sum(p.numel() * p.element_size() for layer in model.model.layers for p in layer.parameters())
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    _oneshot(model, _recipe("gptq-w4a16-group"), tmp_path / "streamed", monkeypatch, stream=True)
    peak = torch.cuda.max_memory_allocated(dev) - base
    assert model._qt_placement["mode"] == "stream"
    assert all(p.device.type == "cpu" for p in model.parameters())
    assert peak < layer_bytes / 2, f"peak {peak / 2**20:.0f} MiB for {layer_bytes / 2**20:.0f} MiB of layers"


def test_plugin_streams_a_host_model(dev, tmp_path, monkeypatch):
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry

    outs = {}
    for stream in (False, True):
        monkeypatch.chdir(tmp_path)
        _force(monkeypatch, stream)
        model = _tiny_llama()
        q = QuantizerRegistry.create("gptq", model_id="synthetic/tiny-llama")
        out = q.quantize(model=model, level="W4A16", dataset=_data(), num_calibration_samples=8, max_seq_length=64,
                         shuffle_calibration_samples=False,
                         oneshot_kwargs={"output_dir": str(tmp_path / f"work-{stream}")})
        torch.cuda.synchronize()
        assert q.last_model is model
        assert model._qt_placement["mode"] == ("stream" if stream else "resident")
        outs[stream] = _checkpoint(out)
    (a, cfg_a), (b, cfg_b) = outs[False], outs[True]
    assert cfg_a == cfg_b and sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
