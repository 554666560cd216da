"""CPU side of the A16 runtime: ``load_quantized(..., a16="packed")`` on tiny Llama / Mixtral checkpoints gives
``WeightOnlyLinear``s whose integer buffers restate the default loader's dequantised weights bit for bit, whose CPU
forward equals the dequantised ``nn.Linear``'s, and which hold a fraction of the dense bytes.  No GPU call."""
import pytest
import torch
import torch.nn as nn

from tests.test_moe_loader import BANK, _write as _write_mixtral
from tests.test_qlinear_loader import _write as _write_llama

A16 = [("W4A16", False), ("W4A16", True), ("W4A16_ASYM", False), ("W4A16_ASYM", True), ("W8A16", False)]


def _buffer_bytes(m: nn.Module) -> int:
    return sum(b.numel() * b.element_size() for b in m.buffers())


@pytest.mark.parametrize("scheme,g_idx", A16)
def test_packed_linears_restate_the_dequantized_weights(tmp_path, scheme, g_idx):
    from quantool_amd.engine.qlinear import WeightOnlyLinear, dequantized_weight, load_quantized

    path, _, levels = _write_llama(tmp_path, scheme, g_idx=g_idx)
    dense = load_quantized(path, device="cpu")
    packed = load_quantized(path, device="cpu", a16="packed")
    assert packed._qt_checkpoint["a16"] == "packed" and packed._qt_checkpoint["dense_expert_banks"] == []
    assert "a16" not in dense._qt_checkpoint
    q_bytes = dense_bytes = 0
    for name, (q, t) in levels.items():
        lin, wol = dense.get_submodule(name), packed.get_submodule(name)
        assert type(lin) is nn.Linear and isinstance(wol, WeightOnlyLinear), name
        N, K = q.shape
        assert (wol.out_features, wol.in_features) == (N, K)
        assert wol.int4 == (scheme != "W8A16")
        assert wol.weight_scale.dtype == torch.float32 and torch.equal(wol.weight_scale, t["weight_scale"].float())
        assert (wol.weight_zero_point is not None) == ("weight_zero_point" in t)
        assert (wol.g_idx is not None) == g_idx
        if g_idx:
            assert wol.g_idx.dtype == torch.int32 and torch.equal(wol.g_idx, t["weight_g_idx"])
        w = dequantized_weight(name, wol.checkpoint_tensors(), torch.bfloat16)
        assert torch.equal(w.view(torch.int16), lin.weight.data.view(torch.int16)), name
        x = torch.randn(2, 3, K, generator=torch.Generator().manual_seed(len(name))).to(torch.bfloat16)
        with torch.no_grad():
            assert torch.equal(wol(x), lin(x)), name
        q_bytes += _buffer_bytes(wol)
        dense_bytes += lin.weight.numel() * lin.weight.element_size()
    ratio = q_bytes / dense_bytes
    assert ratio <= (0.55 if scheme == "W8A16" else 0.3), ratio
    ids = torch.tensor([[1, 2, 3, 4]])
    with torch.no_grad():
        assert torch.equal(packed(input_ids=ids).logits, dense(input_ids=ids).logits)


def test_extra_repr_names_the_format(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    path, _, _ = _write_llama(tmp_path, "W4A16_ASYM", g_idx=True)
    wol = load_quantized(path, device="cpu", a16="packed").model.layers[0].mlp.down_proj
    r = repr(wol)
    assert "WeightOnlyLinear" in r and "weights=int4" in r and "zero_point=True" in r and "g_idx=True" in r


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
@pytest.mark.parametrize("a16", ["dequantized", "packed"])
def test_a8_checkpoints_ignore_the_a16_mode(tmp_path, scheme, a16):
    from quantool_amd.engine.qlinear import QuantizedLinear, WeightOnlyLinear, load_quantized

    path, _, levels = _write_llama(tmp_path, scheme)
    model = load_quantized(path, device="cpu", a16=a16)
    for name in levels:
        assert isinstance(model.get_submodule(name), QuantizedLinear), name
    assert not any(isinstance(m, WeightOnlyLinear) for m in model.modules())
    assert "a16" not in model._qt_checkpoint


def test_bad_a16_mode_is_refused(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    path, _, _ = _write_llama(tmp_path, "W4A16")
    with pytest.raises(ValueError, match="a16"):
        load_quantized(path, device="cpu", a16="int4")


def test_packed_mode_keeps_a16_expert_banks_dense_and_records_them(tmp_path):
    from quantool_amd.engine.qlinear import QuantizedExperts, WeightOnlyLinear, load_quantized

    _write_mixtral(tmp_path, "W4A16")
    dense = load_quantized(tmp_path, device="cpu")
    packed = load_quantized(tmp_path, device="cpu", a16="packed")
    bank = packed.get_submodule(BANK)
    assert not isinstance(bank, QuantizedExperts)
    assert torch.equal(bank.gate_up_proj.data, dense.get_submodule(BANK).gate_up_proj.data)
    assert torch.equal(bank.down_proj.data, dense.get_submodule(BANK).down_proj.data)
    assert packed._qt_checkpoint["a16"] == "packed"
    assert packed._qt_checkpoint["dense_expert_banks"] == [BANK]
    attn = [n for n, m in packed.named_modules() if isinstance(m, WeightOnlyLinear)]
    assert len(attn) == 4 and all(".self_attn." in n for n in attn)
    ids = torch.tensor([[5, 6, 7]])
    with torch.no_grad():
        assert torch.equal(packed(input_ids=ids).logits, dense(input_ids=ids).logits)
