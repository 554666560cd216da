"""CPU side of packed A16 expert banks: ``load_quantized(..., a16="packed", a16_experts="packed")`` on tiny Mixtral
checkpoints gives ``WeightOnlyExperts`` whose integer buffers are the checkpoint's tensors stacked, which hold a
fraction of the dense bank's bytes and whose CPU forward equals the dense bank's; the refusals.  No GPU call."""
import pytest
import torch

from quantool_amd.engine.schemes import PRESET_SCHEMES
from tests.test_moe_loader import BANK, E, H, I, _ckpt_name, _write

A16 = [("W4A16", False), ("W4A16", True), ("W4A16_ASYM", False), ("W4A16_ASYM", True), ("W8A16", False)]


def _bytes(ts) -> int:
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


@pytest.mark.parametrize("scheme,g_idx", A16)
def test_packed_experts_hold_the_checkpoint_tensors(tmp_path, scheme, g_idx):
    from quantool_amd.engine.qlinear import WeightOnlyExperts, WeightOnlyLinear, load_quantized
    from quantool_amd.engine.serialization import load_state

    _write(tmp_path, scheme, g_idx=g_idx)
    dense = load_quantized(tmp_path, device="cpu")
    packed = load_quantized(tmp_path, device="cpu", a16="packed", a16_experts="packed")
    woe = packed.get_submodule(BANK)
    assert isinstance(woe, WeightOnlyExperts)
    assert (woe.num_experts, woe.hidden_dim, woe.intermediate_dim) == (E, H, I)
    int4 = PRESET_SCHEMES[scheme].weights.num_bits == 4
    assert woe.int4 == int4
    asym = not PRESET_SCHEMES[scheme].weights.symmetric
    state = load_state(tmp_path)
    leaf = "weight_packed" if int4 else "weight"
    for part, roles, K in (("gate_up", ("w1", "w3"), H), ("down", ("w2",), I)):
        w, s = getattr(woe, part), getattr(woe, f"{part}_scale")
        zp, gi = getattr(woe, f"{part}_zero_point"), getattr(woe, f"{part}_g_idx")
        assert w.dtype == (torch.int32 if int4 else torch.int8) and s.dtype == torch.float32
        assert (zp is not None) == asym and (gi is not None) == g_idx
        for e in range(E):
            names = [_ckpt_name(e, r) for r in roles]
            assert torch.equal(w[e], torch.cat([state[f"{n}.{leaf}"] for n in names]))
            assert torch.equal(s[e], torch.cat([state[f"{n}.weight_scale"].float() for n in names]))
            if asym:
                assert zp.dtype == torch.int8
                assert torch.equal(zp[e], torch.cat([state[f"{n}.weight_zero_point"] for n in names]))
            if g_idx:
                assert gi.dtype == torch.int32 and tuple(gi.shape) == (E, K)
                assert torch.equal(gi[e], state[f"{names[0]}.weight_g_idx"])
        # the dequantised view is the dense bank's parameter, to the bit
        ref = getattr(dense.get_submodule(BANK), f"{part}_proj").data
        assert torch.equal(woe.dense_weight(part, torch.bfloat16), ref)
    ratio = _bytes(woe.buffers()) / _bytes(dense.get_submodule(BANK).parameters())
    assert ratio <= (0.55 if scheme == "W8A16" else 0.3), ratio
    # the model no longer holds the bf16 bank: its parameters are the router's and the dense rest only
    assert not any(n.endswith(("gate_up_proj", "down_proj")) for n, _ in packed.named_parameters())
    assert len([m for m in packed.modules() if isinstance(m, WeightOnlyLinear)]) == 4
    ids = torch.tensor([[5, 6, 7, 8, 9]])
    with torch.no_grad():
        assert torch.equal(packed(input_ids=ids).logits, dense(input_ids=ids).logits)
    ck = packed._qt_checkpoint
    assert ck["a16"] == "packed" and ck["dense_expert_banks"] == [] and ck["packed_expert_banks"] == [BANK]
    assert "packed_expert_banks" not in load_quantized(tmp_path, device="cpu", a16="packed")._qt_checkpoint


def test_extra_repr_names_the_format(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    _write(tmp_path, "W4A16_ASYM", g_idx=True)
    r = repr(load_quantized(tmp_path, device="cpu", a16="packed", a16_experts="packed").get_submodule(BANK))
    assert "WeightOnlyExperts" in r and "weights=int4" in r and "zero_point=True" in r and "g_idx=True" in r


def test_bad_modes_are_refused(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    _write(tmp_path, "W4A16")
    with pytest.raises(ValueError, match="a16_experts"):
        load_quantized(tmp_path, device="cpu", a16_experts="packed")
    with pytest.raises(ValueError, match="a16_experts"):
        load_quantized(tmp_path, device="cpu", a16="packed", a16_experts="int4")


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_a8_checkpoints_ignore_the_argument(tmp_path, scheme):
    from quantool_amd.engine.qlinear import QuantizedExperts, WeightOnlyExperts, load_quantized

    _write(tmp_path, scheme)
    model = load_quantized(tmp_path, device="cpu", a16="packed", a16_experts="packed")
    assert isinstance(model.get_submodule(BANK), QuantizedExperts)
    assert not any(isinstance(m, WeightOnlyExperts) for m in model.modules())
    assert "a16" not in model._qt_checkpoint and "packed_expert_banks" not in model._qt_checkpoint


def _rewrite(path, edit):
    """Load the checkpoint's tensors, apply ``edit`` to the dict and save them back under the same config."""
    import json

    from quantool_amd.engine.serialization import load_state, save_state

    state = load_state(path)
    edit(state)
    cfg = json.loads((path / "config.json").read_text())
    qcfg = cfg.pop("quantization_config")
    save_state(state, qcfg, path, cfg)


def test_mixed_banks_are_refused(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized, unpack_int4

    kw = dict(device="cpu", a16="packed", a16_experts="packed")
    # expert 2's down weight as int8 while the rest are packed int4
    d = tmp_path / "format"
    _write(d, "W4A16")

    def to_int8(state):
        n = _ckpt_name(2, "w2")
        state[f"{n}.weight"] = unpack_int4(state.pop(f"{n}.weight_packed"), I)

    _rewrite(d, to_int8)
    with pytest.raises(ValueError, match="mix formats or group counts"):
        load_quantized(d, **kw)
    # expert 1's gate weight channel-wise while the rest have groups of 128
    d = tmp_path / "groups"
    _write(d, "W4A16")

    def channelwise(state):
        n = _ckpt_name(1, "w1")
        state[f"{n}.weight_scale"] = state[f"{n}.weight_scale"][:, :1].contiguous()

    _rewrite(d, channelwise)
    with pytest.raises(ValueError, match="mix formats or group counts"):
        load_quantized(d, **kw)
    # a zero-point on one expert only
    d = tmp_path / "zp"
    _write(d, "W4A16")

    def one_zero_point(state):
        n = _ckpt_name(3, "w2")
        state[f"{n}.weight_zero_point"] = torch.zeros(H, (I + 127) // 128, dtype=torch.int8)

    _rewrite(d, one_zero_point)
    with pytest.raises(ValueError, match="mix formats or group counts"):
        load_quantized(d, **kw)
    # gate and up of one expert grouped differently
    d = tmp_path / "gidx"
    _write(d, "W4A16", g_idx=True)

    def regroup(state):
        n = _ckpt_name(0, "w3")
        state[f"{n}.weight_g_idx"] = state[f"{n}.weight_g_idx"].flip(0).contiguous()

    _rewrite(d, regroup)
    with pytest.raises(ValueError, match="group their columns differently"):
        load_quantized(d, **kw)
    # every one of these still loads dequantised, as before
    for sub in ("format", "groups", "zp", "gidx"):
        load_quantized(tmp_path / sub, device="cpu", a16="packed")


@pytest.mark.parametrize("scheme", ["W4A16", "W8A16"])
def test_bank_refusals_stand_in_packed_mode(tmp_path, scheme):
    from quantool_amd.engine.qlinear import load_quantized

    kw = dict(device="cpu", a16="packed", a16_experts="packed")
    d = tmp_path / "missing"
    _write(d, scheme, drop=_ckpt_name(3, "w2") + ".")
    with pytest.raises(ValueError, match="missing from the checkpoint"):
        load_quantized(d, **kw)
    d = tmp_path / "partly"
    _write(d, scheme, dense_expert=(1, "down_proj"))
    with pytest.raises(ValueError, match="partly quantized"):
        load_quantized(d, **kw)
