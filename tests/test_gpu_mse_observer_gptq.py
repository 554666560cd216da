"""``observer="mse"`` through the GPTQ chains and ``oneshot``: the sweep behind the new tables keeps its parity with the
oracle, the batched chain equals the single one, and a saved checkpoint says which observer made it."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
K = 384


def _case(dev, rows, seed):
    from quantool_amd.engine.gptq_linear import HessianAccumulator

    g = torch.Generator().manual_seed(seed)
    X = torch.randn(512, K, generator=g).to(torch.bfloat16).to(dev)
    W = (torch.distributions.StudentT(3.0).sample((rows, K)) * 0.02).to(torch.bfloat16).to(dev)
    acc = HessianAccumulator(K, dev)
    acc.add(X)
    return W, acc, X


def test_shared_chain_with_mse_tables_equals_the_oracle_sweep(dev, oracle):
    from quantool_amd.engine.gptq_linear import gptq_quantize_shared
    from quantool_amd.engine.schemes import QuantArgs

    torch.manual_seed(0)
    W, acc, _ = _case(dev, 24, 1)
    keep = {}
    res = gptq_quantize_shared([W], acc, QuantArgs(actorder="static", observer="mse"), keep=keep)[0]
    ref = gptq_quantize_shared([W], acc, QuantArgs(actorder="static"))[0]
    torch.cuda.synchronize()
    assert (res.scale_f32 != ref.scale_f32).float().mean().item() >= 0.5        # the route really was taken

    perm, dead = keep["perm"].cpu().numpy(), keep["dead"].cpu().numpy()
    Wn = np.where(dead[None] != 0, np.float32(0), W.float().cpu().numpy()[:, perm])
    scale, zp = res.scale_f32.cpu().numpy(), res.zp_f32.cpu().numpy()
    Q, Wdq, _ = oracle.gptq_sweep_c(Wn, keep["U"].cpu().numpy(), scale, zp, (perm // 128).astype(np.int32), 128, 4)
    q, wdq = np.empty_like(Q), np.empty_like(Wdq)
    q[:, perm], wdq[:, perm] = Q, Wdq
    assert np.array_equal(res.weight_packed.cpu().numpy(), oracle.pack_int4(q))
    assert np.array_equal(res.dequantized().cpu().numpy(), wdq)        # as values: the oracle's zeros carry a sign


def test_batched_chain_equals_the_single_runs(dev):
    """Rows 128 + 40: every group but the last of a batch must hold a multiple of 128 rows (``batchable``)."""
    from quantool_amd.engine.gptq_linear import gptq_quantize_batched, gptq_quantize_shared
    from quantool_amd.engine.schemes import QuantArgs

    torch.manual_seed(1)
    qargs = QuantArgs(actorder="static", observer="mse")
    groups = [([W], acc) for W, acc, _ in (_case(dev, 128, 2), _case(dev, 40, 3))]
    both = gptq_quantize_batched(groups, qargs)
    for (ws, acc), got in zip(groups, both):
        solo = gptq_quantize_shared(ws, acc, qargs)[0]
        for name in ("weight_packed", "scale_f32", "zp_f32", "loss"):
            assert torch.equal(getattr(got[0], name), getattr(solo, name)), name


def test_oneshot_saves_the_observer_and_reads_back(dev, tmp_path):
    from quantool_amd.engine.gptq_linear import gptq_quantize_shared
    from quantool_amd.engine.modifiers import GPTQModifier
    from quantool_amd.engine.oneshot import LinearCalibrationSet, LinearGroup, oneshot
    from quantool_amd.engine.qlinear import dequantized_weight, load_quantized
    from quantool_amd.engine.serialization import load_state
    from tests.test_gpu_qlinear import _tiny_llama

    torch.manual_seed(2)
    recipe = GPTQModifier(scheme="W4A16", observer="mse")
    W, acc, X = _case(dev, 24, 4)
    oneshot(model=LinearCalibrationSet([LinearGroup("g", X, {"lin": W})]), recipe=recipe, output_dir=str(tmp_path / "lin"))
    cfg = json.loads((tmp_path / "lin" / "config.json").read_text())["quantization_config"]
    assert cfg["config_groups"]["group_0"]["weights"]["observer"] == "mse"
    solo = gptq_quantize_shared([W], acc, recipe.weight_args())[0]
    leaves = {k.split(".", 1)[1]: v.to(dev) for k, v in load_state(tmp_path / "lin").items()}
    assert torch.equal(leaves["weight_packed"], solo.weight_packed)
    assert torch.equal(leaves["weight_scale"], solo.weight_scale)

    # a module: load_quantized rebuilds the Linears from what was stored
    data = [{"input_ids": torch.randint(0, 512, (48,))} for _ in range(8)]
    mem = oneshot(model=_tiny_llama(dev), dataset=data, recipe=recipe, output_dir=str(tmp_path / "llama"),
                  num_calibration_samples=8, max_seq_length=64, shuffle_calibration_samples=False)
    cfg = json.loads((tmp_path / "llama" / "config.json").read_text())["quantization_config"]
    assert cfg["config_groups"]["group_0"]["weights"]["observer"] == "mse"
    back = load_quantized(tmp_path / "llama", device=dev).state_dict()
    stored = load_state(tmp_path / "llama")
    name = "model.layers.1.mlp.down_proj"
    t = {k[len(name) + 1:]: v.to(dev) for k, v in stored.items() if k.startswith(name + ".")}
    assert torch.equal(back[name + ".weight"], dequantized_weight(name, t, torch.bfloat16))
    # in memory the fp32 scale dequantised; the stored scale is that rounded to bf16
    torch.testing.assert_close(back[name + ".weight"].float(), mem.state_dict()[name + ".weight"].float(), rtol=2.0 ** -7,
                               atol=0.0)
