"""``method=awq`` on a sparse-MoE layer (the tiny random-init Mixtral of ``test_gpu_mixtral_module``: H = 256,
I = 256, E = 4, top-2, 2 KV heads, W4A16 g128): smoothing as an exact function-preserving rewrite (router and up
rows included), the bank search against an independent restatement, a per-expert search against the oracle, an
expert no token reaches, and the plugin end to end."""
import logging

import numpy as np
import pytest
import torch

from tests.util import bf16_tensor_to_bits

pytestmark = pytest.mark.gpu

H, I, E = 256, 256, 4
L0 = "model.layers.0"
BANK = f"{L0}.mlp.experts.experts"


def _tiny_mixtral(dev, dtype=torch.bfloat16):
    from transformers import MixtralConfig, MixtralForCausalLM

    from quantool_amd.engine.sequential import unfuse_expert_banks

    cfg = MixtralConfig(hidden_size=H, intermediate_size=I, num_hidden_layers=2, num_attention_heads=4,
                        num_key_value_heads=2, num_local_experts=E, num_experts_per_tok=2, vocab_size=512,
                        max_position_embeddings=128, tie_word_embeddings=False)
    torch.manual_seed(0)
    model = MixtralForCausalLM(cfg).to(dtype).to(dev).eval()
    assert unfuse_expert_banks(model) == 2
    return model


def _data(n=6, length=40, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [{"input_ids": torch.randint(0, 512, (length,), generator=g)} for _ in range(n)]


def _first(o):
    return o[0] if isinstance(o, (tuple, list)) else o


def _layer_inputs(model, data, dev):
    """(args, kwargs) of decoder layer 0 for every calibration row."""
    calls = []

    class Stop(Exception):
        pass

    def grab(_m, a, kw):
        calls.append((a, kw))
        raise Stop

    h = model.model.layers[0].register_forward_pre_hook(grab, with_kwargs=True)
    with torch.no_grad():
        for row in data:
            try:
                model(input_ids=row["input_ids"].reshape(1, -1).to(dev), use_cache=False)
            except Stop:
                pass
    h.remove()
    return calls


def _resolve(layer):
    from quantool_amd.engine.awq_module import normalise_mappings, resolve_mappings
    from quantool_amd.engine.modifiers import AWQModifier

    maps = resolve_mappings(layer, L0, normalise_mappings(None), AWQModifier().wants)
    assert len(maps) == 1 + 1 + E                    # GQA: no v -> o
    return maps


def _run_with_routing(layer, calls):
    """Layer outputs and the router's top-k indices per call."""
    idx = []
    h = layer.mlp.gate.register_forward_hook(lambda m, a, out: idx.append(out[2].clone()))
    with torch.no_grad():
        outs = [_first(layer(*a, **kw)).clone() for a, kw in calls]
    h.remove()
    return outs, idx


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_power_of_two_scales_preserve_the_layer_bit_for_bit(dev, dtype):
    """Derived, not measured: a power-of-two scale commutes with rounding, so norm / s with W * s (router columns
    included) and up rows / s with down columns * s give every product, hence every sum, the same bits."""
    from quantool_amd.engine.awq_module import _apply

    model = _tiny_mixtral(dev, dtype)
    calls = _layer_inputs(model, _data(2), dev)
    layer = model.model.layers[0]
    before, idx_before = _run_with_routing(layer, calls)
    assert sorted(torch.cat(idx_before).unique().tolist()) == list(range(E))      # all four experts hit
    g = torch.Generator().manual_seed(9)
    snapshot = {n: p.data.clone() for n, p in layer.named_parameters()}
    with torch.no_grad():
        for mp in _resolve(layer):
            K = mp.balance[0].in_features
            s = (2.0 ** torch.randint(-2, 3, (K,), generator=g).float()).to(dev)
            _apply(mp, s)
    changed = {n for n, p in layer.named_parameters() if not torch.equal(p.data, snapshot[n])}
    assert "mlp.gate.weight" in changed and "post_attention_layernorm.weight" in changed
    assert all(f"mlp.experts.experts.{e}.{w}.weight" in changed for e in range(E) for w in ("gate_up_proj", "down_proj"))
    after, idx_after = _run_with_routing(layer, calls)
    for a, b in zip(idx_before, idx_after):
        assert torch.equal(a, b)
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_random_scales_preserve_the_layer_to_bf16_rounding(dev):
    from quantool_amd.engine.awq_module import _apply

    model = _tiny_mixtral(dev)
    calls = _layer_inputs(model, _data(2), dev)
    layer = model.model.layers[0]
    before, _ = _run_with_routing(layer, calls)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for mp in _resolve(layer):
            K = mp.balance[0].in_features
            s = (0.5 + 1.5 * torch.rand(K, generator=g)).to(dev)
            w_before = mp.balance[0].weight.data.float().clone()
            _apply(mp, s)
            torch.testing.assert_close(mp.balance[0].weight.data.float(), (w_before * s).to(torch.bfloat16).float())
    after, _ = _run_with_routing(layer, calls)
    for b, a in zip(before, after):
        rel = (a.float() - b.float()).norm() / b.float().norm()
        print(f"rel = {float(rel):.3e}")
        assert rel < 2e-2, rel              # only bf16 re-rounding of the rescaled weights


@pytest.fixture(scope="module")
def searched(dev):
    """One ``awq_layer`` run on layer 0 and what an untouched twin model saw at the block and at every expert's
    down_proj on the same calibration rows; shared by the search tests and left unchanged."""
    from quantool_amd.engine.awq_module import awq_layer
    from quantool_amd.engine.modifiers import AWQModifier

    data = _data(6)
    model, ref = _tiny_mixtral(dev), _tiny_mixtral(dev)
    calls = _layer_inputs(ref, data, dev)
    layer = ref.model.layers[0]
    block = layer.mlp
    xs, parent_calls, down_in = [], [], {e: [] for e in range(E)}
    hooks = [block.register_forward_pre_hook(lambda m, a, kw: parent_calls.append((a, kw)), with_kwargs=True),
             block.register_forward_pre_hook(lambda m, a: xs.append(a[0].reshape(-1, a[0].shape[-1]).clone()))]
    for e in range(E):
        hooks.append(block.experts.experts[e].down_proj.register_forward_pre_hook(
            lambda m, a, e=e: down_in[e].append(a[0].reshape(-1, a[0].shape[-1]).clone())))
    with torch.no_grad():
        for a, kw in calls:
            layer(*a, **kw)
    for h in hooks:
        h.remove()
    router_before = model.model.layers[0].mlp.gate.weight.data.clone()
    with torch.no_grad():
        res = awq_layer(model.model.layers[0], L0, _layer_inputs(model, data, dev), AWQModifier(), dev)
    torch.cuda.synchronize()
    return dict(model=model, ref=ref, res=res, xs=xs, parent_calls=parent_calls, down_in=down_in,
                router_before=router_before)


def test_bank_search_matches_independent_restatement(dev, oracle, searched):
    """post_attention_layernorm -> every expert's gate_up_proj, parent = the MoE block, router untouched during the
    search.  Restated with the oracle's scale / pseudo-quant formulas over all block-input tokens and the E gate_up
    weights (no router), and torch's own forward of the block."""
    ref, res = searched["ref"], searched["res"]
    block = ref.model.layers[0].mlp
    parent_calls = searched["parent_calls"]
    X = torch.cat(searched["xs"]).float().cpu().numpy()
    assert X.shape == (6 * 40, H)
    x_mean = np.abs(X).astype(np.float64).mean(axis=0).astype(np.float32)
    lins = [block.experts.experts[e].gate_up_proj for e in range(E)]
    originals = [l.weight.data.clone() for l in lins]
    Ws = [w.float().cpu().numpy() for w in originals]
    w_mean = oracle.awq_weight_mean(Ws, 128)
    try:
        with torch.no_grad():
            fp = [_first(block(*a, **kw)).float() for a, kw in parent_calls]
            want_losses = []
            for gi in range(20):
                s = oracle.awq_scales_for_ratio(x_mean, w_mean, gi / 20)
                for l, W in zip(lins, Ws):
                    trial = (oracle.awq_pseudo_quantize((W * s[None, :]).astype(np.float32), 128, True, 4) / s[None, :])
                    l.weight.data.copy_(torch.from_numpy(trial.astype(np.float32)).to(dev).to(torch.bfloat16))
                sq = sum(float((r - _first(block(*a, **kw)).float()).pow(2).sum()) for (a, kw), r in zip(parent_calls, fp))
                want_losses.append(sq / sum(r.numel() for r in fp))
    finally:
        for l, w0 in zip(lins, originals):
            l.weight.data.copy_(w0)
    want_best = int(np.argmin(want_losses))

    r = res[f"{BANK}.0.gate_up_proj"]
    got_losses = r.losses.cpu().numpy()
    print("bank losses got", got_losses, "want", want_losses)
    # scales differ by powf rounding (1e-5), which can flip single roundings in the trial weights:
    # losses agree to a fraction of a percent, the argmin exactly unless two grid points tie that closely
    np.testing.assert_allclose(got_losses, np.array(want_losses, np.float32), rtol=2e-2)
    best = int(r.best_ratio_idx.item())
    assert best == want_best or abs(want_losses[best] - want_losses[want_best]) < 2e-2 * want_losses[want_best]
    np.testing.assert_allclose(r.smoothing_scales.cpu().numpy(),
                               oracle.awq_scales_for_ratio(x_mean, w_mean, best / 20), rtol=1e-4)
    # every expert's gate_up shares the one mapping: same scale vector object
    for e in range(1, E):
        assert res[f"{BANK}.{e}.gate_up_proj"].smoothing_scales is r.smoothing_scales
    # the router was rescaled with them (columns * s, bf16) and is not among the results
    s = r.smoothing_scales
    want_router = (searched["router_before"].float() * s[None, :]).to(torch.bfloat16)
    assert torch.equal(searched["model"].model.layers[0].mlp.gate.weight.data, want_router)
    assert f"{L0}.mlp.gate" not in res
    # every expert that received tokens carries smoothing scales on its down_proj too
    for e in range(E):
        assert sum(x.shape[0] for x in searched["down_in"][e]) > 0
        d = res[f"{BANK}.{e}.down_proj"]
        assert d.smoothing_scales is not None and d.losses.shape == (20,)


def test_per_expert_search_matches_oracle(dev, oracle, searched, e=1):
    """up rows of ``experts.e.gate_up_proj`` -> ``experts.e.down_proj``: a single balance Linear, so the Gram form;
    against ``awq_best_scale`` on the rows routed to that expert (tolerances of the single-balance search tests)."""
    ref, res = searched["ref"], searched["res"]
    Xb = torch.cat(searched["down_in"][e])
    assert 0 < Xb.shape[0] < 6 * 40 and Xb.shape[1] == I
    W = ref.model.layers[0].mlp.experts.experts[e].down_proj.weight.data.float().cpu().numpy()
    want = oracle.awq_best_scale(bf16_tensor_to_bits(Xb), [W], 128)
    r = res[f"{BANK}.{e}.down_proj"]
    print("expert losses got", r.losses.cpu().numpy(), "want", want["losses"])
    np.testing.assert_allclose(r.losses.cpu().numpy(), want["losses"], rtol=2e-3)
    assert int(r.best_ratio_idx.item()) == want["best_ratio_idx"]
    np.testing.assert_allclose(r.smoothing_scales.cpu().numpy(), want["best_scales"], rtol=1e-5)


class _MaskLastExpert(torch.nn.Module):
    """A router that never picks the last expert (its logit is -inf); the real router stays inside, so its weight is
    still the block's one 2-d ``weight [E, H]`` outside the bank."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, hidden_states):
        logits = torch.nn.functional.linear(hidden_states.reshape(-1, self.inner.hidden_dim), self.inner.weight)
        masked = logits.float().clone()
        masked[:, -1] = float("-inf")
        top, idx = torch.topk(torch.softmax(masked, dim=-1), self.inner.top_k, dim=-1)
        return logits, top / top.sum(dim=-1, keepdim=True), idx


def test_expert_without_tokens_is_skipped_and_still_quantised(dev, caplog):
    from quantool_amd.engine.awq_module import awq_layer
    from quantool_amd.engine.modifiers import AWQModifier

    model = _tiny_mixtral(dev)
    layer = model.model.layers[0]
    layer.mlp.gate = _MaskLastExpert(layer.mlp.gate)
    last = f"{BANK}.{E - 1}"
    with torch.no_grad(), caplog.at_level(logging.WARNING, logger="quantool_amd.engine.awq_module"):
        res = awq_layer(layer, L0, _layer_inputs(model, _data(4), dev), AWQModifier(), dev)
    torch.cuda.synchronize()
    skipped = [rec.getMessage() for rec in caplog.records if "skipped" in rec.getMessage()]
    assert len(skipped) == 1 and f"{last}.down_proj" in skipped[0] and "no calibration token" in skipped[0]
    assert len(res) == 4 + 2 * E
    d = res[f"{last}.down_proj"]
    assert d.smoothing_scales is None and d.losses is None and d.weight_packed is not None
    assert res[f"{last}.gate_up_proj"].smoothing_scales is not None          # the bank mapping covers it
    for e in range(E - 1):
        assert res[f"{BANK}.{e}.down_proj"].smoothing_scales is not None
    for name, r in res.items():
        lin = model.get_submodule(name)
        assert torch.isfinite(lin.weight.data.float()).all(), name
        assert torch.equal(lin.weight.data, r.dequantized(torch.bfloat16)), name
        assert torch.isfinite(r.weight_scale.float()).all(), name
        if r.smoothing_scales is not None:
            assert torch.isfinite(r.losses).all() and torch.isfinite(r.smoothing_scales).all(), name
    assert all(torch.isfinite(p.data.float()).all() for p in layer.parameters())


def test_non_finite_losses_raise(dev):
    """No 0/0 reaches an arg-min: a Gram sum that holds a NaN fails the search instead of picking a winner."""
    from quantool_amd.engine.awq_module import _Capture, _search
    from quantool_amd.engine.modifiers import AWQModifier

    model = _tiny_mixtral(dev)
    mp = _resolve(model.model.layers[0])[-1]
    assert mp.single
    cap = _Capture(mp, dev)
    cap._stats(torch.randn(8, I, device=dev, dtype=torch.bfloat16))
    cap.gram[0, 0] = float("nan")
    with pytest.raises(FloatingPointError, match="non-finite"):
        _search(mp, cap, AWQModifier().weight_args(), 20, True)


def test_awq_plugin_on_tiny_mixtral(dev, oracle, tmp_path, monkeypatch):
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry
    from safetensors.torch import load_file

    monkeypatch.chdir(tmp_path)
    x = torch.randint(0, 512, (1, 32), generator=torch.Generator().manual_seed(1)).to(dev)
    errs = {}
    for mode in ("rtn", "awq"):
        model = _tiny_mixtral(dev)
        with torch.no_grad():
            before = model(input_ids=x).logits.float()
        q = QuantizerRegistry.create("awq", model_id="synthetic/tiny-mixtral")
        # the yardstick: the same run with mappings that match nothing, i.e. round-to-nearest only
        kw = {"method_kwargs": {"mappings": [["re:.*matches_no_module$", ["re:.*matches_no_module$"]]]}} if mode == "rtn" else {}
        q.quantize(model=model, level="W4A16", dataset=_data(6), num_calibration_samples=6, max_seq_length=64, **kw)
        torch.cuda.synchronize()
        with torch.no_grad():
            after = model(input_ids=x).logits.float()
        errs[mode] = float((after - before).norm() / before.norm())
        res = model._qt_results
        assert len(res) == 2 * (4 + 2 * E)
        if mode == "rtn":
            assert all(r.smoothing_scales is None for r in res.values())
            continue
        q.save_pretrained(str(tmp_path / "saved"))
        sd = load_file(str(tmp_path / "saved" / "model.safetensors"))
        packed = sorted(k for k in sd if k.endswith("weight_packed"))
        assert len(packed) == 2 * (4 + 3 * E)
        for li in range(2):
            for e in range(E):
                for w in ("w1", "w2", "w3"):
                    assert f"model.layers.{li}.block_sparse_moe.experts.{e}.{w}.weight_packed" in sd
        with_scales = 0
        for name, r in res.items():
            lin = model.get_submodule(name)
            # module weight == dequantised levels, levels == unpacked words
            np.testing.assert_array_equal(
                lin.weight.data.float().cpu().numpy(),
                oracle.bf16_bits_to_f32(oracle.f32_to_bf16_bits(r.dequantized().cpu().numpy())))
            np.testing.assert_array_equal(oracle.unpack_int4(r.weight_packed.cpu().numpy(), lin.in_features),
                                          r.Qt.t().cpu().numpy())
            if r.smoothing_scales is not None:
                with_scales += 1
                assert int(torch.argmin(r.losses)) == int(r.best_ratio_idx)
                s = r.smoothing_scales
                assert torch.isfinite(s).all() and (s > 0).all()
        assert with_scales >= 2 * (3 + E)                 # q, k, v and every gate_up; down_proj where tokens arrived
    print(f"logit error: awq {errs['awq']:.4f} rtn {errs['rtn']:.4f}")
    # the search minimises block error on the calibration tokens, not logits on this probe, hence the margin; a
    # missed router or up half gives errors of order 1
    assert errs["awq"] <= 1.5 * errs["rtn"], errs
