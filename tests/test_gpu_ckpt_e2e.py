"""Checkpoints at odd widths, quantised through the plugins and written synthetically, loaded with ``load_quantized`` in
every mode and checked module by module against what the checkpoint files define (tests/ckpt_reference.py, which
decodes the files without the package).

The models: a Llama 200 wide with intermediate 328, 4 heads and 2 kv-heads (head_dim 50), and a Mixtral of the same
widths with 4 experts, top-2.  Every K is a multiple of 8 but not of 128 (the calibration kernels need K % 8 == 0), so
the plugins' channel-wise schemes (smoothquant W8A8 / INT8, GPTQ W8A16) run at these widths; the grouped schemes need
K % group_size == 0 there, so W4A16, W4A16_ASYM, W4A8 and W4A8 with a permuted weight_g_idx are written by the test
from a saved checkpoint, with the intermediate width changed to 330 (down_proj then has K % 8 != 0, a partial packed
word) except in the A16 Mixtral, whose dense transformers bank (torch._grouped_mm) needs 16-byte row strides.  Token
counts 1, 5, 16, 17 and 129 run the GEMV and the dequantise paths of ``WeightOnlyLinear`` and the grouped and dense
paths of ``WeightOnlyExperts``."""
import pytest
import torch
import torch.nn as nn

from tests import ckpt_reference as cr

pytestmark = pytest.mark.gpu

TOKENS = (1, 5, 16, 17, 129)


def _llama(dev):
    from transformers import LlamaConfig, LlamaForCausalLM

    cfg = LlamaConfig(hidden_size=200, intermediate_size=328, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=512, max_position_embeddings=256, tie_word_embeddings=False)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev).eval()


def _mixtral(dev):
    from transformers import MixtralConfig, MixtralForCausalLM

    cfg = MixtralConfig(hidden_size=200, intermediate_size=328, num_hidden_layers=2, num_attention_heads=4,
                        num_key_value_heads=2, num_local_experts=4, num_experts_per_tok=2, vocab_size=512,
                        max_position_embeddings=256, tie_word_embeddings=False)
    torch.manual_seed(0)
    return MixtralForCausalLM(cfg).to(torch.bfloat16).to(dev).eval()


def _plugin_checkpoint(dev, arch, method, level, out_dir):
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry

    model = _llama(dev) if arch == "llama" else _mixtral(dev)
    g = torch.Generator().manual_seed(2)
    data = [{"input_ids": torch.randint(0, 512, (48,), generator=g)} for _ in range(8)]
    q = QuantizerRegistry.create(method, model_id=f"synthetic/odd-{arch}")
    q.quantize(model=model, level=level, dataset=data, num_calibration_samples=8, max_seq_length=64,
               shuffle_calibration_samples=False)
    torch.cuda.synchronize()
    q.save_pretrained(str(out_dir))
    del q, model
    return out_dir


PLUGIN = {"W8A8": ("smoothquant", "W8A8"), "INT8": ("smoothquant", "INT8"), "W8A16": ("gptq", "W8A16")}
SYNTH = {"W4A16": dict(bits=4), "W4A16_ASYM": dict(bits=4, zero_point=True), "W4A8": dict(bits=4, act="asym"),
         "W4A8_gidx": dict(bits=4, act="asym", g_idx=True)}


@pytest.fixture(scope="module")
def checkpoints(dev, tmp_path_factory):
    """Checkpoints made once per module: {(arch, scheme): directory}; the plugins run in a scratch working dir."""
    import os

    made = {}
    root = tmp_path_factory.mktemp("odd_ckpts")
    cwd = os.getcwd()
    os.chdir(root)
    try:
        def get(arch, scheme):
            key = (arch, scheme)
            if key not in made:
                if scheme in PLUGIN:
                    made[key] = _plugin_checkpoint(dev, arch, *PLUGIN[scheme], root / f"{arch}_{scheme}")
                else:
                    cfg, dense, linears = cr.from_checkpoint(get(arch, "W8A16"))
                    # intermediate 330 where the model can carry it: transformers' dense Mixtral bank (grouped_mm)
                    # needs 16-byte row strides, so the A16 Mixtral keeps 328
                    wide = arch == "llama" or "act" in SYNTH[scheme]
                    cr.write_synthetic(root / f"{arch}_{scheme}", cfg, dense, linears, seed=len(scheme),
                                       resize={328: 330} if wide else None, **SYNTH[scheme])
                    made[key] = root / f"{arch}_{scheme}"
            return made[key]
        yield get
    finally:
        os.chdir(cwd)


# ---- the per-module check -------------------------------------------------------------------------------------------
def _is_bank(m):
    from quantool_amd.engine.qlinear import QuantizedExperts, WeightOnlyExperts

    return isinstance(m, (QuantizedExperts, WeightOnlyExperts)) or (
        isinstance(getattr(m, "gate_up_proj", None), nn.Parameter) and getattr(m, "gate_up_proj").dim() == 3)


def check_modules_against_files(model, ckpt, dev, tokens=TOKENS, vocab=512):
    """Run ``model`` on batches of ``tokens`` tokens, hook every Linear the checkpoint quantizes and every expert bank,
    and compare each output with tests/ckpt_reference.py on the module's own input.  Returns the number of checks."""
    from quantool_amd.hip import ops

    cfg, tensors = cr.read_checkpoint(ckpt)
    gs = cr.group_size(cfg)
    acts = cfg["quantization_config"]["config_groups"]["group_0"].get("input_activations")
    sym = None if acts is None else bool(acts.get("symmetric", True))
    quant = cr.quantized_modules(tensors)
    linears, banks = {}, {}
    for name, t in quant.items():
        ex = cr.expert_of(name)
        if ex is None:
            linears[name] = t
        else:
            banks.setdefault(ex[0], {}).setdefault(ex[1], {})[ex[2]] = t
    hooked = {}
    for n, m in model.named_modules():
        alt = n.replace(".mlp.", ".block_sparse_moe.")
        if n in linears or alt in linears:
            hooked[n] = ("linear", linears[n if n in linears else alt], m)
        elif _is_bank(m) and n.rpartition(".mlp.")[0] in banks:
            hooked[n] = ("bank", banks[n.rpartition(".mlp.")[0]], m)
    assert len(hooked) == len(linears) + len(banks), (sorted(hooked), sorted(linears), sorted(banks))
    seen = {}

    def hook(name):
        def f(mod, inp, out):
            seen.setdefault(name, []).append(([a.detach().clone() if torch.is_tensor(a) else a for a in inp],
                                              out.detach().clone()))
        return f

    handles = [m.register_forward_hook(hook(n)) for n, (_, _, m) in hooked.items()]
    n_checks = 0
    try:
        for T in tokens:
            seen.clear()
            ids = torch.randint(0, vocab, (1, T), generator=torch.Generator().manual_seed(T)).to(dev)
            with torch.no_grad():
                model(input_ids=ids)
            torch.cuda.synchronize()
            assert set(seen) == set(hooked)
            for name, calls in seen.items():
                kind, t, m = hooked[name]
                for inp, y in calls:
                    if kind == "linear":
                        N, K = cr.shape_of(t)
                        x = inp[0].reshape(-1, K)
                        Y = y.reshape(-1, N).cpu()
                        bias = getattr(m, "bias", None)
                        if sym is None:
                            y64, mag = cr.a16_linear(x, t, bias, gs)
                            tol = cr.gemv_tolerance(Y, mag, K)
                        else:
                            Xq, s_x, zp_x = ops.quantize_tokens_i8(x.contiguous(), symmetric=sym)
                            y64, mag = cr.a8_linear(Xq, s_x, zp_x, t, bias, gs)
                            tol = cr.gemm_i8_tolerance(Y, mag, t["weight_scale"].shape[1])
                    else:
                        x, idx, w = inp[0], inp[1], inp[2]
                        y64, tol = cr.expert_bank(x.reshape(-1, x.shape[-1]), idx, w, t, a8_symmetric=sym, gsize=gs)
                        Y = y.reshape(y64.shape).cpu()
                    cr.assert_within(Y, y64, tol, f"{name} at {T} tokens")
                    n_checks += 1
    finally:
        for h in handles:
            h.remove()
    return n_checks


# ---- the tests ------------------------------------------------------------------------------------------------------
A16_MODES = {"dequantized": dict(), "packed": dict(a16="packed"),
             "packed_experts": dict(a16="packed", a16_experts="packed")}


@pytest.mark.parametrize("arch", ["llama", "mixtral"])
@pytest.mark.parametrize("scheme", ["W8A8", "INT8", "W4A8", "W4A8_gidx"])
def test_a8_checkpoint_matches_its_files(dev, checkpoints, arch, scheme):
    from quantool_amd.engine.qlinear import QuantizedExperts, QuantizedLinear, load_quantized

    model = load_quantized(checkpoints(arch, scheme), device=dev)
    assert any(isinstance(m, QuantizedLinear) for m in model.modules())
    assert any(isinstance(m, QuantizedExperts) for m in model.modules()) == (arch == "mixtral")
    if scheme == "W4A8_gidx":
        assert any(getattr(m, "col_perm", None) is not None for m in model.modules())
    assert check_modules_against_files(model, checkpoints(arch, scheme), dev) > 0


@pytest.mark.parametrize("arch,mode", [("llama", "dequantized"), ("llama", "packed"), ("mixtral", "dequantized"),
                                       ("mixtral", "packed"), ("mixtral", "packed_experts")])
@pytest.mark.parametrize("scheme", ["W8A16", "W4A16", "W4A16_ASYM"])
def test_a16_checkpoint_matches_its_files(dev, checkpoints, arch, scheme, mode):
    from quantool_amd.engine.qlinear import WeightOnlyExperts, WeightOnlyLinear, load_quantized

    model = load_quantized(checkpoints(arch, scheme), device=dev, **A16_MODES[mode])
    assert any(isinstance(m, WeightOnlyLinear) for m in model.modules()) == (mode != "dequantized")
    assert any(isinstance(m, WeightOnlyExperts) for m in model.modules()) == (mode == "packed_experts")
    assert check_modules_against_files(model, checkpoints(arch, scheme), dev) > 0
