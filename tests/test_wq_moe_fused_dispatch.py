"""``qt_gemm_wq_grouped_act_mul`` / ``qt_moe_gemm_wq_wide_act_mul`` without a GPU: the header, the ctypes table and the
built library carry both with ``qt_moe_gemm_wq_wide``'s argument list; ``ops.moe_gemm_wq_act_mul_supported`` and the two
wrappers refuse before they touch the library; ``WeightOnlyExperts.fused_act`` routes the gate_up product of a routed
forward to the fused form and leaves everything else alone; ``load_quantized(..., a16_experts_fused_act=)`` sets it."""
import pytest
import torch
import torch.nn as nn

from tests.i8_fake_ops import check_surface
from tests.test_moe_loader import BANK, _write
from tests.test_wq_moe_wide_dispatch import _experts, _run, recorded  # noqa: F401  (recorded: a fixture)
from tests.test_wq_stream_dispatch import REFUSED, _no_library

NAMES = ("qt_gemm_wq_grouped_act_mul", "qt_moe_gemm_wq_wide_act_mul")
FUSED = ("gemm_wq_grouped_act_mul", "moe_gemm_wq_wide_act_mul", "moe_gemm_wq_act_mul_supported")


@pytest.mark.parametrize("name", NAMES)
def test_surface(name):
    from quantool_amd.hip import _lib

    check_surface("header", name)
    check_surface("ctypes", name, like="qt_moe_gemm_wq_wide")
    check_surface("library", name)
    assert len([n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")]) == 14


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    """The dense table's operands as a bank of one expert (a leading dimension of 1 keeps every address)."""
    ops = _no_library(monkeypatch)
    make, kw, reason = REFUSED[case]
    X, Wq, s_w = (t.unsqueeze(0) if i else t for i, t in enumerate(make()))
    assert ops.moe_gemm_wq_act_mul_supported(X, Wq, s_w, None, kw.get("g_idx")) is False
    for name in FUSED[:2]:
        with pytest.raises(ValueError, match=f"{name}: .*{reason}"):
            getattr(ops, name)(X, Wq, s_w, torch.zeros(2, dtype=torch.int32), **kw)


def test_supported_and_the_rules_of_its_own(monkeypatch):
    ops = _no_library(monkeypatch)
    X = torch.zeros(32, 256, dtype=torch.bfloat16)
    Wq, s_w = torch.zeros(2, 8, 256, dtype=torch.int8), torch.ones(2, 8, 2)
    assert ops.moe_gemm_wq_act_mul_supported(X, Wq, s_w) is True
    assert ops.moe_gemm_wq_act_mul_supported(X, Wq, s_w, torch.zeros(2, 8, 2, dtype=torch.int8), None,
                                             torch.zeros(64, dtype=torch.int32)) is True
    off = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="2 I rows per expert"):            # an odd bank has no halves
        ops.gemm_wq_grouped_act_mul(X, Wq[:, :7].contiguous(), s_w[:, :7].contiguous(), off)
    with pytest.raises(ValueError, match="act must be one of"):
        ops.moe_gemm_wq_wide_act_mul(X, Wq, s_w, off, act="gelu")
    # 16-row slots: the decode form's grid fills before the wide form's
    rows = torch.empty(16 * 65535, dtype=torch.int32, device="meta")
    assert ops.moe_gemm_wq_wide_supported(X, Wq, s_w, None, None, rows) is True
    assert ops.moe_gemm_wq_act_mul_supported(X, Wq, s_w, None, None, rows) is False


# ---- WeightOnlyExperts -----------------------------------------------------------------------------------------------
@pytest.fixture
def fused(recorded, monkeypatch):  # noqa: F811
    """``recorded`` plus recording fakes of the two fused forms and of the tile form."""
    ops, log = recorded

    def fake(name, halve):
        def f(X, Wq, s_w, offsets, *, row_idx=None, K=None, zp_w=None, g_idx=None):
            R = X.shape[0] if row_idx is None else row_idx.numel()
            log.append((name, "gate_up" if row_idx is not None else "down", R))
            return torch.zeros(R, Wq.shape[1] // (2 if halve else 1), dtype=X.dtype)
        return f

    monkeypatch.setattr(ops, "gemm_wq_grouped_act_mul", fake("grouped_act_mul", True))
    monkeypatch.setattr(ops, "moe_gemm_wq_wide_act_mul", fake("wide_act_mul", True))
    monkeypatch.setattr(ops, "moe_gemm_wq_tile", fake("tile", False))
    return ops, log


def test_off_by_default_and_no_fused_name_is_read(fused, monkeypatch):
    from quantool_amd.engine.qmodules import WeightOnlyExperts

    ops, log = fused
    assert WeightOnlyExperts.fused_act is False
    woe, bank = _experts()
    assert "fused_act=False" in repr(woe)
    for name in FUSED:
        monkeypatch.delattr(ops, name)
    woe.wide_min_tokens, woe.wide_max_tokens, woe.tile_max_tokens = 96, 300, 600
    for T in (1, 100, 200, 400, 700):
        _run(woe, T)
    assert [n for n, _, _ in log] == ["grouped"] * 2 + ["wide"] * 4 + ["tile"] * 2 and bank.calls == 1


def test_routes_with_fused_act(fused):
    _, log = fused
    woe, bank = _experts()
    woe.fused_act = True
    assert "fused_act=True" in repr(woe)
    woe.wide_min_tokens, woe.wide_max_tokens, woe.tile_max_tokens = 96, 300, 600
    for T in (1, 95, 96, 128, 129, 300, 301, 600, 601):
        _run(woe, T)
    assert log == [("grouped_act_mul", "gate_up", 2), ("grouped", "down", 2),
                   ("grouped_act_mul", "gate_up", 190), ("grouped", "down", 190),
                   ("wide_act_mul", "gate_up", 192), ("wide", "down", 192),
                   ("wide_act_mul", "gate_up", 256), ("wide", "down", 256),
                   ("wide_act_mul", "gate_up", 258), ("wide", "down", 258),        # the wide_max_tokens range
                   ("wide_act_mul", "gate_up", 600), ("wide", "down", 600),
                   ("tile", "gate_up", 602), ("tile", "down", 602),                # the tile range: unfused, unchanged
                   ("tile", "gate_up", 1200), ("tile", "down", 1200)]
    assert bank.calls == 1                                                          # 601: the dequantise path
    del log[:]
    woe.wide_min_tokens = 0
    _run(woe, 128)
    assert [n for n, _, _ in log] == ["grouped_act_mul", "grouped"]                 # 0: the decode form at every T <= 128
    del log[:]
    woe.act_fn = nn.GELU()                                                          # not SiLU: unfused
    _run(woe, 8)
    g_woe, _ = _experts(g_idx=True)                                                 # a bank the forms do not take: unfused
    g_woe.fused_act = True
    _run(g_woe, 8)
    assert [n for n, _, _ in log] == ["grouped"] * 4


# ---- load_quantized --------------------------------------------------------------------------------------------------
def test_loader_flag(tmp_path):
    from quantool_amd.engine.qlinear import WeightOnlyExperts, load_quantized

    _write(tmp_path, "W4A16")
    kw = dict(device="cpu", a16="packed", a16_experts="packed")
    model = load_quantized(tmp_path, **kw)
    assert model.get_submodule(BANK).fused_act is False and model._qt_checkpoint["a16_experts_fused_act"] is False
    model = load_quantized(tmp_path, a16_experts_fused_act=True, **kw)
    assert model.get_submodule(BANK).fused_act is True and model._qt_checkpoint["a16_experts_fused_act"] is True
    assert WeightOnlyExperts.fused_act is False                         # an instance attribute: the class keeps False
    model = load_quantized(tmp_path, a16_fused_act=True, **kw)          # the dense flag leaves the banks alone
    assert model.get_submodule(BANK).fused_act is False and model._qt_checkpoint["a16_fused_act"] is True
    for bad in (dict(device="cpu", a16="packed"), dict(device="cpu")):
        with pytest.raises(ValueError, match="needs a16='packed' and a16_experts='packed'"):
            load_quantized(tmp_path, a16_experts_fused_act=True, **bad)
        assert "a16_experts_fused_act" not in load_quantized(tmp_path, **bad)._qt_checkpoint
    with pytest.raises(ValueError, match="expected True or False"):
        load_quantized(tmp_path, a16_experts_fused_act=1, **kw)
    _write(tmp_path / "a8", "W4A8")                                     # A8 checkpoints ignore it
    model = load_quantized(tmp_path / "a8", a16_experts_fused_act=True, **kw)
    assert "a16_experts_fused_act" not in model._qt_checkpoint
    assert not any(isinstance(m, WeightOnlyExperts) for m in model.modules())
