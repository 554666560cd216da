"""The fused RMSNorm + quantise pass inside whole checkpoints, on the device.  A checkpoint loaded with
``a8_fused_norm=True`` is compared with the same checkpoint loaded without it whose eligible norms run the same kernel
and return its ``Y`` but hand nothing over, so every consumer quantises ``Y`` for itself: the logits must agree to the
bit.  That pins the hand-off -- which consumer gets which rows, zero points, staleness -- apart from the kernel's
arithmetic (test_gpu_rmsnorm_quant.py).  The launch counts are those of the dispatch test, on the real ``ops``."""
import pytest
import torch

from tests.norm_fake_ops import quantizing_norms, tag_linears

pytestmark = pytest.mark.gpu


class Calls:
    """Counts the real ``ops``' quantiser and fused-norm launches; ``quantised`` names the calling Linear."""

    def __init__(self, monkeypatch, ops):
        self.caller = None
        self.quantised, self.norms = [], []
        real_q, real_n = ops.quantize_tokens_i8, ops.rmsnorm_quantize_i8

        def quantize_tokens_i8(*a, **kw):
            self.quantised.append(self.caller)
            return real_q(*a, **kw)

        def rmsnorm_quantize_i8(*a, **kw):
            self.norms.append(tuple(a[0].shape))
            return real_n(*a, **kw)

        monkeypatch.setattr(ops, "quantize_tokens_i8", quantize_tokens_i8)
        monkeypatch.setattr(ops, "rmsnorm_quantize_i8", rmsnorm_quantize_i8)

    def clear(self):
        self.quantised.clear()
        self.norms.clear()


def _kernel_y_only(ops, model, names):
    """Every norm in ``names`` runs the fused kernel and returns its Y; nobody takes its rows."""
    for name in names:
        norm = model.get_submodule(name)
        assert type(norm).__name__.endswith("RMSNorm") and not hasattr(norm, "shared")

        def forward(x, norm=norm):
            K = norm.weight.numel()
            return ops.rmsnorm_quantize_i8(x.reshape(-1, K), norm.weight, norm.variance_epsilon)[0].reshape(x.shape)

        norm.forward = forward


def _both(ops, dev, path, calls, fused_act):
    from quantool_amd.engine.qlinear import load_quantized

    ids = torch.randint(0, 320, (2, 24), generator=torch.Generator().manual_seed(11)).to(dev)
    on = load_quantized(path, device=dev, a8_fused_act=fused_act, a8_fused_norm=True)
    names = sorted(quantizing_norms(on))
    off = load_quantized(path, device=dev, a8_fused_act=fused_act)
    assert quantizing_norms(off) == {} and list(on.state_dict()) == list(off.state_dict())
    _kernel_y_only(ops, off, names)
    out = {}
    for key, model in (("on", on), ("off", off)):
        tag_linears(model, calls)
        calls.clear()
        with torch.no_grad():
            out[key] = model(input_ids=ids).logits
        torch.cuda.synchronize()
        out[key + "_calls"] = (list(calls.quantised), list(calls.norms))
    assert not any(n.shared.holds_tensors for n in quantizing_norms(on).values())
    a, b = out["on"], out["off"]
    assert a.shape == b.shape == (2, 24, 320) and torch.isfinite(a.float()).all() and bool(a.any())
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ"
    return names, out


@pytest.mark.parametrize("fused_act", [False, True])
@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_dense_checkpoint_hand_off(ops, dev, tmp_path, monkeypatch, scheme, fused_act):
    from tests.a8_fused_ckpt import write_llama

    write_llama(tmp_path, scheme, layers=2, bias=True)
    calls = Calls(monkeypatch, ops)
    names, out = _both(ops, dev, tmp_path, calls, fused_act)
    assert names == sorted(f"model.layers.{i}.{n}" for i in range(2)
                           for n in ("input_layernorm", "post_attention_layernorm"))
    own = ("self_attn.o_proj",) if fused_act else ("self_attn.o_proj", "mlp.down_proj")
    quantised, norms = out["on_calls"]
    assert quantised == [f"model.layers.{i}.{n}" for i in range(2) for n in own]
    assert norms == [(48, 256)] * 4
    quantised, norms = out["off_calls"]
    assert len(quantised) == (10 if fused_act else 14) and norms == [(48, 256)] * 4


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_moe_checkpoint_hand_off(ops, dev, tmp_path, monkeypatch, scheme):
    from tests.a8_fused_ckpt import write_mixtral

    write_mixtral(tmp_path, scheme)
    calls = Calls(monkeypatch, ops)
    names, out = _both(ops, dev, tmp_path, calls, False)
    assert names == ["model.layers.0.input_layernorm"]
    quantised, norms = out["on_calls"]
    assert [c for c in quantised if c is not None] == ["model.layers.0.self_attn.o_proj"] and norms == [(48, 256)]
    assert len(quantised) == 3                               # o_proj and the bank's two
    assert len(out["off_calls"][0]) == 6


def test_decode_sized_input_and_a_second_forward(ops, dev, tmp_path, monkeypatch):
    """One row through the 16-byte path, twice: the second forward starts from an empty hand-off."""
    from quantool_amd.engine.qlinear import load_quantized
    from tests.a8_fused_ckpt import write_llama

    write_llama(tmp_path, "W8A8", layers=1)
    model = load_quantized(tmp_path, device=dev, a8_fused_norm=True)
    ids = torch.tensor([[5]], device=dev)
    with torch.no_grad():
        a = model(input_ids=ids).logits
        b = model(input_ids=ids).logits
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.isfinite(a.float()).all()
    assert not any(n.shared.holds_tensors for n in quantizing_norms(model).values())
