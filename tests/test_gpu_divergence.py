"""``evaluate.divergence`` end to end on a small Llama: a model against itself (exactly zero, and both perplexities are
``perplexity(head="fused")``'s), against a copy with one Linear rounded to 4 bits (the means are held to the fp64
evaluation of the two models' own final hidden states within the bar of test_gpu_lm_head_kl.py), and a W8A8 checkpoint
written by ``oneshot`` against its original, both by path."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

VOCAB, HIDDEN, B, T = 515, 128, 3, 100


def _tiny_llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(1234)
    cfg = LlamaConfig(hidden_size=HIDDEN, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=VOCAB, max_position_embeddings=128, tie_word_embeddings=False)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).eval()


@pytest.fixture(scope="module")
def model(dev):
    return _tiny_llama().to(dev)


@pytest.fixture(scope="module")
def ids():
    return torch.randint(0, VOCAB, (B, T), generator=torch.Generator().manual_seed(5))


def test_a_model_against_itself(model, ids):
    from quantool_amd.evaluate import DIVERGENCE_KEYS, divergence, perplexity

    d = divergence(model, model, ids, batch_size=2)                    # two batches: the sums run across them
    assert set(d) == set(DIVERGENCE_KEYS)
    assert d["kl"] == 0.0 and d["kl_max"] == 0.0 and d["top1_agree"] == 1.0
    fused = perplexity(model, ids, head="fused", batch_size=2)
    assert d["perplexity"] == d["perplexity_ref"] == fused["perplexity"]
    assert d["nll"] == d["nll_ref"] == fused["nll"]
    assert d["top1"] == d["top1_ref"] == fused["top1"]
    assert d["tokens"] == fused["tokens"] == B * (T - 1)


def test_a_model_against_a_perturbed_copy(model, ids, dev, monkeypatch):
    from quantool_amd.evaluate import divergence

    other = copy.deepcopy(model)
    lin = other.model.layers[1].mlp.down_proj
    w = lin.weight.data.float()
    scale = w.abs().amax(dim=1, keepdim=True) / 7
    lin.weight.data = ((w / scale).round().clamp(-8, 7) * scale).to(torch.bfloat16)       # 4 bits per output row

    seen = {}
    hooks = [m.model.norm.register_forward_hook(lambda mod, inp, out, k=k: seen.setdefault(k, []).append(out.detach()))
             for k, m in (("p", model), ("q", other))]

    def no_logits(*a, **k):
        raise AssertionError("lm_head.forward was called: logits were formed")

    monkeypatch.setattr(model.lm_head, "forward", no_logits)
    monkeypatch.setattr(other.lm_head, "forward", no_logits)
    try:
        d = divergence(model, other, ids)
    finally:
        for h in hooks:
            h.remove()
        monkeypatch.undo()
    assert len(seen["p"]) == len(seen["q"]) == 1
    W = model.lm_head.weight.detach().cpu()
    hp = seen["p"][0][:, :-1].reshape(-1, HIDDEN).cpu()
    hq = seen["q"][0][:, :-1].reshape(-1, HIDDEN).cpu()
    tg = ids[:, 1:].reshape(-1, 1)

    def rows(cast):
        a, b = cast(hp) @ cast(W).T, cast(hq) @ cast(W).T
        lp, lq = torch.logsumexp(a, -1), torch.logsumexp(b, -1)
        kl = (torch.softmax(a, -1) * (a - b)).sum(-1) - lp + lq
        return kl.double(), (lp - a.gather(1, tg).squeeze(1)).double(), (lq - b.gather(1, tg).squeeze(1)).double(), a, b

    kl64, np64, nq64, a64, b64 = rows(torch.Tensor.double)
    kl32, np32, nq32, _, _ = rows(torch.Tensor.float)
    lse_max = float(torch.maximum(torch.logsumexp(a64, -1).abs(), torch.logsumexp(b64, -1).abs()).max())
    n = B * (T - 1)
    assert d["tokens"] == n
    # a mean's error is at most the rows' maximum error, which is what the bar is taken from
    for key, want, yard in (("kl", kl64, kl32), ("nll_ref", np64, np32), ("nll", nq64, nq32)):
        bar = max(4 * float((yard - want).abs().max()), 2.0 ** -22 * lse_max)
        err = abs(d[key] - float(want.mean()))
        print(f"{key}: {d[key]!r}, fp64 {float(want.mean())!r}, error {err:.3e}, bar {bar:.3e}")
        assert err <= bar, (key, err, bar)
    assert 0 < d["kl"] < 1 and d["kl_max"] >= d["kl"]
    assert abs(d["kl_max"] - float(kl64.max())) <= max(4 * float((kl32 - kl64).abs().max()), 2.0 ** -22 * lse_max)
    assert d["top1_agree"] == pytest.approx(float((a64.argmax(-1) == b64.argmax(-1)).double().mean()), abs=2 / n)


def test_differing_heads_are_refused(model, ids):
    from quantool_amd.evaluate import divergence

    other = copy.deepcopy(model)
    other.lm_head.weight.data[3, 5] += 1.0
    with pytest.raises(ValueError, match="the two models' LM heads differ: one head weight is what the kernel takes"):
        divergence(model, other, ids)


def test_a_w8a8_checkpoint_against_its_original_by_path(dev, tmp_path, ids):
    from quantool_amd.engine.modifiers import GPTQModifier, SmoothQuantModifier
    from quantool_amd.engine.oneshot import oneshot
    from quantool_amd.evaluate import divergence, perplexity

    m = _tiny_llama()
    m.save_pretrained(str(tmp_path / "orig"))
    g = torch.Generator().manual_seed(1)
    data = [{"input_ids": torch.randint(0, VOCAB, (48,), generator=g)} for _ in range(8)]
    recipe = [SmoothQuantModifier(smoothing_strength=0.5), GPTQModifier(scheme="W8A8")]
    oneshot(model=m.to(dev), dataset=data, recipe=recipe, output_dir=str(tmp_path / "w8a8"), num_calibration_samples=8, max_seq_length=64,
            shuffle_calibration_samples=False)
    torch.cuda.synchronize()
    del m
    d = divergence(str(tmp_path / "orig"), tmp_path / "w8a8", ids, device=dev)
    print(d)
    assert d["tokens"] == B * (T - 1)
    assert 0 < d["kl"] < 0.5 and d["kl"] <= d["kl_max"]
    assert 0 < d["top1_agree"] <= 1.0
    # each side's perplexity is that side's own
    assert d["perplexity"] == perplexity(tmp_path / "w8a8", ids, device=dev, head="fused")["perplexity"]
    assert d["perplexity_ref"] != d["perplexity"]
