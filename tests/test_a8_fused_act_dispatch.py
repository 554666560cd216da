"""The fused SiLU(gate) * up + quantise pass (``qt_act_mul_quantize_i8``) in the A8 modules and the loader, without a
GPU: ``quantool_amd.hip.ops`` is replaced by a recording fake.  ``QuantizedExperts.fused_act`` and ``QuantizedMLP``
change which passes run between the GEMMs and never which GEMM runs; with the switches off no new ``ops`` name is read;
``load_quantized(..., a8_fused_act=True)`` installs both without moving a state-dict key."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.a8_fused_ckpt import write_llama, write_mixtral
from tests.i8_fake_ops import Recorder, fake_ops  # noqa: F401

E, TOPK = 4, 2
WIDE = ("moe_gemm_i8_wide_supported", "moe_gemm_i8_wide"), ("moe_gemm_i8_ring_w4_supported", "moe_gemm_i8_ring_w4")


class FusedRecorder(Recorder):
    """``Recorder`` with the banks' later forms, a counting ``quantize_tokens_i8`` and a recording
    ``act_mul_quantize_i8``: ``fused`` lists (gate, up, symmetric, col_perm) of every call, ``quantised`` the shape of
    every ``quantize_tokens_i8`` input."""

    def __init__(self):
        super().__init__()
        for watch, gemm in WIDE:
            self.answers[watch] = True
            self.queries[watch] = []
            setattr(self, watch, self._supported(watch))
            setattr(self, gemm, self._grouped(gemm))
        self.fused = []
        self.quantised = []

    def quantize_tokens_i8(self, X, symmetric=True, col_perm=None):
        self.quantised.append(tuple(X.shape))
        return super().quantize_tokens_i8(X, symmetric=symmetric, col_perm=col_perm)

    def act_mul_quantize_i8(self, gate, up, symmetric=True, col_perm=None, act="silu", return_h=False):
        assert act == "silu" and not return_h
        self.fused.append((gate, up, symmetric, col_perm))
        M, K = gate.shape
        zp = None if symmetric else torch.zeros(M, dtype=torch.int32)
        return torch.zeros(M, K, dtype=torch.int8), torch.ones(M), zp

    def clear(self):
        self.calls.clear()
        self.fused.clear()
        self.quantised.clear()


@pytest.fixture
def rec(monkeypatch):
    import quantool_amd.hip as hip
    from quantool_amd.hip import ops as real   # noqa: F401  (the attribute the modules import must exist first)

    r = FusedRecorder()
    monkeypatch.setattr(hip, "ops", r)
    return r


# ---- what counts as SiLU --------------------------------------------------------------------------------------------
def test_silu_is_recognised():
    from transformers.activations import ACT2FN

    from quantool_amd.engine.qmodules import is_silu

    assert is_silu(nn.SiLU()) and is_silu(F.silu) and is_silu(ACT2FN["silu"]) and is_silu(ACT2FN["swish"])
    for other in (nn.GELU(), F.gelu, ACT2FN["gelu"], ACT2FN["relu"], nn.Identity(), torch.sigmoid, lambda x: x, None):
        assert not is_silu(other), other


def test_transformers_silu_is_torchs():
    """What the fused pass restates is ``F.silu``: the object transformers hands a model must compute exactly that."""
    from transformers.activations import ACT2FN

    x = torch.randn(64, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    assert torch.equal(ACT2FN["silu"](x), F.silu(x))


# ---- QuantizedExperts -----------------------------------------------------------------------------------------------
def _experts(H=512, I=640, int4=False, act_fn=None):
    from quantool_amd.engine.qmodules import QuantizedExperts

    if int4:
        gu, dn = torch.zeros(E, 2 * I, H // 8, dtype=torch.int32), torch.zeros(E, H, I // 8, dtype=torch.int32)
        s_gu, s_dn = torch.ones(E, 2 * I, H // 128), torch.ones(E, H, I // 128)
    else:
        gu, dn = torch.zeros(E, 2 * I, H, dtype=torch.int8), torch.zeros(E, H, I, dtype=torch.int8)
        s_gu, s_dn = torch.ones(E, 2 * I, 1), torch.ones(E, H, 1)
    return QuantizedExperts(H, I, gu, s_gu, dn, s_dn, nn.SiLU() if act_fn is None else act_fn, not int4)


def _forward(r, qe, T):
    r.clear()
    out = qe(torch.zeros(T, qe.hidden_dim, dtype=torch.bfloat16), torch.zeros(T, TOPK, dtype=torch.int64),
             torch.ones(T, TOPK))
    assert out.shape == (T, qe.hidden_dim)
    return list(r.calls)


def test_the_switch_is_off_by_default():
    from quantool_amd.engine.qmodules import QuantizedExperts

    assert QuantizedExperts.fused_act is False and "fused_act" not in vars(_experts())


@pytest.mark.parametrize("int4", [False, True])
def test_off_runs_the_three_passes_as_before(rec, int4):
    qe = _experts(int4=int4)
    for T in (1, 17, 300):
        _forward(rec, qe, T)
        assert rec.fused == []
        assert rec.quantised == [(T, 512), (T * TOPK, 640)]


def test_off_reads_no_new_name(fake_ops):
    """``fake_ops`` is the shared Recorder, which does not carry ``act_mul_quantize_i8``: reading it would raise."""
    assert not hasattr(fake_ops, "act_mul_quantize_i8")
    qe = _experts(H=256, I=384)
    fake_ops.calls.clear()
    qe(torch.zeros(5, 256, dtype=torch.bfloat16), torch.zeros(5, TOPK, dtype=torch.int64), torch.ones(5, TOPK))
    assert [c[0] for c in fake_ops.calls] == ["gemm_i8_skinny_grouped"] * 2
    qe.fused_act = True
    with pytest.raises(AttributeError, match="act_mul_quantize_i8"):
        qe(torch.zeros(5, 256, dtype=torch.bfloat16), torch.zeros(5, TOPK, dtype=torch.int64), torch.ones(5, TOPK))


@pytest.mark.parametrize("int4", [False, True])
@pytest.mark.parametrize("T", [1, 16, 17, 40, 300])
def test_on_fuses_the_glue_and_keeps_both_gemms(rec, int4, T):
    qe = _experts(int4=int4)
    off = _forward(rec, qe, T)
    qe.fused_act = True
    on = _forward(rec, qe, T)
    assert on == off and len(on) == 2 and all(rows == T * TOPK for _, rows in on)
    assert rec.quantised == [(T, 512)]
    assert len(rec.fused) == 1
    gate, up, symmetric, col_perm = rec.fused[0]
    R, I = T * TOPK, 640
    assert symmetric is qe.act_symmetric and col_perm is None
    # the two halves of the one [R, 2I] tensor the gate_up GEMM wrote: views, nothing copied
    for half, view in enumerate((gate, up)):
        assert tuple(view.shape) == (R, I) and view.stride() == (2 * I, 1)
        assert view.data_ptr() == gate.data_ptr() + half * I * gate.element_size()
        assert view.untyped_storage().data_ptr() == gate.untyped_storage().data_ptr()
        assert view.untyped_storage().nbytes() == R * 2 * I * gate.element_size()


def test_the_down_gemm_sees_more_than_one_form(rec):
    """The parametrised cases above are not all one GEMM: the down product of the int8 bank walks three forms."""
    qe = _experts()
    qe.fused_act = True
    assert [_forward(rec, qe, T)[1][0] for T in (16, 17, 300)] == ["gemm_i8_skinny_grouped", "moe_gemm_i8_wide",
                                                                   "gemm_i8_grouped"]


@pytest.mark.parametrize("act_fn", [nn.GELU(), F.gelu, nn.ReLU()])
def test_another_activation_keeps_the_three_passes(rec, act_fn):
    qe = _experts(act_fn=act_fn)
    qe.fused_act = True
    _forward(rec, qe, 17)
    assert rec.fused == [] and len(rec.quantised) == 2


# ---- QuantizedLinear / QuantizedMLP ---------------------------------------------------------------------------------
HID, INTER = 512, 640


def _linear(K, N, int4=False, sym=True, col_perm=None, bias=False):
    from quantool_amd.engine.qmodules import QuantizedLinear

    w = torch.zeros(N, K // 8, dtype=torch.int32) if int4 else torch.zeros(N, K, dtype=torch.int8)
    s = torch.ones(N, K // 128 if int4 else 1)
    return QuantizedLinear(K, N, w, s, sym, col_perm=col_perm,
                           bias=torch.zeros(N, dtype=torch.bfloat16) if bias else None)


def _three(int4=False, sym=True, down_perm=None):
    return (_linear(HID, INTER, int4, sym), _linear(HID, INTER, int4, sym),
            _linear(INTER, HID, int4, sym, col_perm=down_perm, bias=True))


@pytest.mark.parametrize("int4", [False, True])
@pytest.mark.parametrize("M", [1, 17, 200])
def test_mlp_shares_the_quantised_rows_and_keeps_the_three_gemms(rec, int4, M):
    from quantool_amd.engine.qmodules import QuantizedMLP

    perm = torch.randperm(INTER, generator=torch.Generator().manual_seed(1)).to(torch.int32)
    gate, up, down = _three(int4, sym=not int4, down_perm=perm)
    x = torch.zeros(2, M // 2, HID, dtype=torch.bfloat16) if M == 200 else torch.zeros(M, HID, dtype=torch.bfloat16)
    rows = x.numel() // HID
    rec.clear()
    y = down(F.silu(gate(x)) * up(x))
    alone = list(rec.calls)
    assert len(alone) == 3 and len(rec.quantised) == 3 and rec.fused == []
    mlp = QuantizedMLP(gate, up, down, nn.SiLU())
    rec.clear()
    out = mlp(x)
    assert out.shape == y.shape and out.dtype == y.dtype
    assert list(rec.calls) == alone
    assert rec.quantised == [(rows, HID)]
    assert len(rec.fused) == 1
    g, u, symmetric, col_perm = rec.fused[0]
    assert tuple(g.shape) == tuple(u.shape) == (rows, INTER)
    assert symmetric is down.act_symmetric and col_perm is down.col_perm and col_perm is not None


def test_mlp_gemm_names_walk_the_forms(rec):
    from quantool_amd.engine.qmodules import QuantizedMLP

    mlp = QuantizedMLP(*_three(), nn.SiLU())
    names = {}
    for M in (1, 17, 200):
        rec.clear()
        mlp(torch.zeros(M, HID, dtype=torch.bfloat16))
        names[M] = [c[0] for c in rec.calls]
    assert names[1] == ["gemm_i8_skinny"] * 3 and names[200] == ["gemm_i8"] * 3
    assert names[17] == ["gemm_i8_mid"] * 3


def test_mlp_keeps_its_childrens_names():
    from quantool_amd.engine.qmodules import QuantizedMLP

    mlp = QuantizedMLP(*_three(), nn.SiLU())
    assert [n for n, _ in mlp.named_children()] == ["gate_proj", "up_proj", "down_proj", "act_fn"]
    assert {k.split(".")[0] for k in mlp.state_dict()} == {"gate_proj", "up_proj", "down_proj"}


class LlamaMLP(nn.Module):
    """A stand-in with the name and the attributes of the transformers class."""

    def __init__(self, gate, up, down, act_fn):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj, self.act_fn = gate, up, down, act_fn


class GatedDeltaMLP(LlamaMLP):
    pass


def test_eligibility():
    from transformers.activations import ACT2FN

    from quantool_amd.engine.qmodules import QuantizedMLP

    perm = torch.randperm(HID, generator=torch.Generator().manual_seed(2)).to(torch.int32)
    ok = QuantizedMLP.eligible
    assert ok(LlamaMLP(*_three(), ACT2FN["silu"])) and ok(LlamaMLP(*_three(int4=True, sym=False), nn.SiLU()))
    # gate and up share a column permutation only when it is the same one
    g, u, d = _three()
    same = (_linear(HID, INTER, col_perm=perm), _linear(HID, INTER, col_perm=perm.clone()), d)
    assert ok(LlamaMLP(*same, nn.SiLU()))
    assert not ok(LlamaMLP(_linear(HID, INTER, col_perm=perm), u, d, nn.SiLU()))
    assert not ok(LlamaMLP(_linear(HID, INTER, col_perm=perm), _linear(HID, INTER, col_perm=perm.flip(0)), d, nn.SiLU()))
    assert not ok(LlamaMLP(_linear(HID, INTER, sym=False), u, d, nn.SiLU()))        # act_symmetric differs
    assert not ok(LlamaMLP(g, u, d, nn.GELU()))                                      # not SiLU
    assert not ok(LlamaMLP(g, nn.Linear(HID, INTER), d, nn.SiLU()))                  # not three QuantizedLinears
    assert not ok(LlamaMLP(g, u, _linear(INTER + 128, HID), nn.SiLU()))              # shapes do not chain
    assert not ok(GatedDeltaMLP(g, u, d, nn.SiLU()))                                 # a foreign forward
    assert not ok(nn.Sequential(g, u, d))
    with pytest.raises(ValueError, match="col_perm"):
        QuantizedMLP(_linear(HID, INTER, col_perm=perm), u, d, nn.SiLU())


def test_the_listed_parents_are_the_plain_forward():
    """Every class name ``QuantizedMLP`` accepts is, in the installed transformers, exactly
    ``down_proj(act_fn(gate_proj(x)) * up_proj(x))``."""
    import importlib
    import inspect

    from quantool_amd.engine.qmodules import QuantizedMLP

    for name in QuantizedMLP.PLAIN_MLPS:
        arch = name[:-3].lower()
        cls = getattr(importlib.import_module(f"transformers.models.{arch}.modeling_{arch}"), name)
        src = inspect.getsource(cls.forward)
        assert "self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))" in src, name


# ---- the loader -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_loader_wraps_dense_mlps(tmp_path, scheme):
    from quantool_amd.engine.qlinear import QuantizedLinear, QuantizedMLP, load_quantized

    write_llama(tmp_path, scheme, bias=True)
    plain = load_quantized(tmp_path, device="cpu")
    fused = load_quantized(tmp_path, device="cpu", a8_fused_act=True)
    assert plain._qt_checkpoint["a8_fused_act"] is False and fused._qt_checkpoint["a8_fused_act"] is True
    assert not any(isinstance(m, QuantizedMLP) for m in plain.modules())
    for layer, ref in zip(fused.model.layers, plain.model.layers):
        assert type(ref.mlp).__name__ == "LlamaMLP"
        assert isinstance(layer.mlp, QuantizedMLP)
        for n in ("gate_proj", "up_proj", "down_proj"):
            assert isinstance(getattr(layer.mlp, n), QuantizedLinear)
        assert layer.mlp.down_proj.bias is not None
        assert isinstance(layer.self_attn.q_proj, QuantizedLinear)
    a, b = plain.state_dict(), fused.state_dict()
    assert list(a) == list(b)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_loader_leaves_an_mlp_whose_halves_permute_differently(tmp_path):
    """actorder ``group`` gives gate_proj and up_proj a column permutation each: the rows cannot be shared."""
    from quantool_amd.engine.qlinear import QuantizedLinear, QuantizedMLP, load_quantized

    write_llama(tmp_path, "W4A8", g_idx=True)
    fused = load_quantized(tmp_path, device="cpu", a8_fused_act=True)
    assert fused._qt_checkpoint["a8_fused_act"] is True
    for layer in fused.model.layers:
        assert type(layer.mlp).__name__ == "LlamaMLP" and not isinstance(layer.mlp, QuantizedMLP)
        assert isinstance(layer.mlp.gate_proj, QuantizedLinear) and layer.mlp.gate_proj.col_perm is not None


@pytest.mark.parametrize("scheme", ["W8A8", "W4A8"])
def test_loader_sets_the_switch_on_every_bank(tmp_path, scheme):
    from quantool_amd.engine.qlinear import QuantizedExperts, load_quantized

    write_mixtral(tmp_path, scheme)
    plain = load_quantized(tmp_path, device="cpu")
    fused = load_quantized(tmp_path, device="cpu", a8_fused_act=True)
    banks = [m for m in fused.modules() if isinstance(m, QuantizedExperts)]
    assert len(banks) == 1 and all(b.fused_act is True for b in banks)
    assert all(m.fused_act is False for m in plain.modules() if isinstance(m, QuantizedExperts))
    assert QuantizedExperts.fused_act is False                 # the class default did not move
    assert plain._qt_checkpoint["a8_fused_act"] is False and fused._qt_checkpoint["a8_fused_act"] is True
    assert list(plain.state_dict()) == list(fused.state_dict())


def test_loader_rejects_a_value_that_is_no_bool(tmp_path):
    from quantool_amd.engine.qlinear import load_quantized

    write_llama(tmp_path, "W8A8", layers=1)
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="a8_fused_act"):
            load_quantized(tmp_path, device="cpu", a8_fused_act=bad)


def test_a16_checkpoints_ignore_it(tmp_path):
    from quantool_amd.engine.qlinear import QuantizedMLP, load_quantized

    write_llama(tmp_path, "W4A16", layers=1)
    for kw in (dict(), dict(a16="packed")):
        model = load_quantized(tmp_path, device="cpu", a8_fused_act=True, **kw)
        assert "a8_fused_act" not in model._qt_checkpoint
        assert not any(isinstance(m, QuantizedMLP) for m in model.modules())
