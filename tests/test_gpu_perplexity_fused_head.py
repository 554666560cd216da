"""``evaluate.perplexity(..., head="fused")`` on a small Llama: the decoder runs alone, ``ops.lm_head_nll`` takes its
hidden states and the head weight, and ``lm_head.forward`` is never called -- no logits are formed.  The mean NLL is held
to the fp64 NLL of the hooked final hidden states and the head weight within bar (a) of test_gpu_lm_head_nll.py: 4x the
error of the fp32 CPU evaluation of the same quantity (the mean's error is at most the rows' maximum error, which is
what the bar is taken from)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

VOCAB, HIDDEN, B, T = 515, 128, 3, 100


@pytest.fixture(scope="module")
def model(dev):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(1234)
    cfg = LlamaConfig(hidden_size=HIDDEN, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, vocab_size=VOCAB, max_position_embeddings=128, tie_word_embeddings=False)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).to(dev).eval()


@pytest.fixture(scope="module")
def ids():
    return torch.randint(0, VOCAB, (B, T), generator=torch.Generator().manual_seed(5))


def test_fused_head_matches_fp64_and_forms_no_logits(model, ids, dev, monkeypatch):
    from quantool_amd.evaluate import perplexity

    default = perplexity(model, ids)

    seen = []
    hook = model.model.norm.register_forward_hook(lambda mod, inp, out: seen.append(out.detach()))

    def no_logits(*a, **k):
        raise AssertionError("lm_head.forward was called: logits were formed")

    monkeypatch.setattr(model.lm_head, "forward", no_logits)
    try:
        fused = perplexity(model, ids, head="fused")
    finally:
        hook.remove()
        monkeypatch.undo()
    assert len(seen) == 1 and seen[0].shape == (B, T, HIDDEN)

    assert fused["head"] == "fused" and fused["tokens"] == default["tokens"] == B * (T - 1)
    hs = seen[0][:, :-1].reshape(-1, HIDDEN).cpu()
    W = model.lm_head.weight.detach().cpu()
    tg = ids[:, 1:].reshape(-1)
    x64 = hs.double() @ W.double().T
    nll64 = torch.logsumexp(x64, -1) - x64.gather(1, tg.unsqueeze(1)).squeeze(1)
    x32 = hs.float() @ W.float().T
    nll32 = torch.logsumexp(x32, -1) - x32.gather(1, tg.unsqueeze(1)).squeeze(1)
    yard = float((nll32.double() - nll64).abs().max())
    err = abs(fused["nll"] - float(nll64.mean()))
    print(f"fused nll {fused['nll']!r}, fp64 {float(nll64.mean())!r}, error {err:.3e}, yardstick (rows' max) {yard:.3e}, "
          f"default path {default['nll']!r}")
    assert err <= 4 * yard, (err, yard)
    assert fused["perplexity"] == pytest.approx(float(torch.exp(nll64.mean())), rel=1e-5)
    hits = int((x64.argmax(-1) == tg).sum())
    assert fused["top1"] == hits / (B * (T - 1))
    # the default path rounds its logits to bf16: it lies far outside the fused path's error
    assert abs(default["nll"] - float(nll64.mean())) < 0.05


def test_the_default_head_is_the_logits_path(model, ids):
    from quantool_amd.evaluate import perplexity

    a = perplexity(model, ids)
    b = perplexity(model, ids, head="logits")
    assert a == b and set(a) == {"perplexity", "nll", "tokens"}


def test_a_head_with_a_bias_is_not_eligible(model, ids, dev, monkeypatch):
    from quantool_amd.evaluate import perplexity

    biased = torch.nn.Linear(HIDDEN, VOCAB, bias=True).to(torch.bfloat16).to(dev)
    monkeypatch.setattr(model, "lm_head", biased)
    with pytest.raises(ValueError, match=r'head="fused" is not available for this model: its head has a bias'):
        perplexity(model, ids, head="fused")
