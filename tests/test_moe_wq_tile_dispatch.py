"""``qt_moe_gemm_wq_tile``'s surface without a GPU: the header, the ctypes table, the built library and the resource
table carry it, ``ops.moe_gemm_wq_tile_supported`` / ``ops.moe_gemm_wq_tile`` refuse what the kernel does not take
before they touch the library, ``WeightOnlyExperts`` dispatches on ``tile_max_tokens`` above the grouped and wide ranges,
and ``load_quantized(..., a16_experts_tile_tokens=)`` switches the range on."""
import pytest
import torch

from tests.i8_fake_ops import check_surface, header_constants
from tests.test_moe_loader import BANK, _write
from tests.test_wq_moe_wide_dispatch import E0, _experts, _meta, _resources, _run, _s, _w4, _w8, recorded  # noqa: F401
from tests.test_wq_stream_dispatch import _no_library, _x

NAME = "qt_moe_gemm_wq_tile"


# ---- surface --------------------------------------------------------------------------------------------------------
def test_surface_header_signature_library_constants_and_build_tables():
    from quantool_amd.csrc import build
    from quantool_amd.hip import _lib, ops

    check_surface("header", NAME)
    check_surface("library", NAME)
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["qt_moe_gemm_wq_wide"]
    assert header_constants("QT_MOE_WQ_TILE_") == {"QT_MOE_WQ_TILE_K_UNIT": ops.MOE_WQ_TILE_K_UNIT,
                                                   "QT_MOE_WQ_TILE_MAX_E": ops.MOE_WQ_TILE_MAX_E,
                                                   "QT_MOE_WQ_TILE_MAX_TILES": ops.MOE_WQ_TILE_MAX_TILES}
    assert ops.MOE_WQ_TILE_K_UNIT == 128 and ops.MOE_WQ_TILE_ROWS == 128
    rows = [line for line in _resources("wq_moe_tile") if "moe_gemm_wq_tile_kernel" in line]
    assert len(rows) == 8                                       # int4 / int8 x bf16 / fp16 x zp / none
    for row in rows:
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row
        assert ("lds 97280" in row) == ("ILb1E" in row) and ("lds 109568" in row) == ("ILb0E" in row), row
    assert any(k in "moe_gemm_wq_tile_kernel" for k in build.NO_SPILL_KERNELS)
    assert "wq_moe_tile.hip" in build.SOURCE_FLAGS and build.SOURCE_FLAGS["wq_moe_tile.hip"] == \
        build.SOURCE_FLAGS["wq_tile.hip"]


# ---- refusals before the library ------------------------------------------------------------------------------------
REFUSED = {
    "g_idx given": (lambda: (_x(300, 1024), _w4(1024), _s(8)), dict(g_idx=torch.zeros(E0, 1024, dtype=torch.int32)),
                    "g_idx is not taken"),
    "K = 192": (lambda: (_x(300, 192), _w8(192), _s(1)), {}, "not a multiple of the k-unit 128"),
    "X shifted by 2 bytes": (lambda: (_x(300, 1024, shift=2), _w4(1024), _s(8)), {}, "16-byte aligned"),
    "G = 3 at K = 1024": (lambda: (_x(300, 1024), _w4(1024), _s(3)), {}, "G must be 1 or K / 128 = 8"),
    "fp32 X": (lambda: (_x(300, 1024, dtype=torch.float32), _w4(1024), _s(8)), {}, "bf16 or fp16"),
    "E past the limit": (lambda: (_x(300, 128), _meta(4097, 1, 16, dtype=torch.int32),
                                  _meta(4097, 1, 1, dtype=torch.float32)), {}, "E=4097 experts are more than 4096"),
    # (2^24 + 1) slots x 128 column tiles = 2^31 + 128
    "too many tiles": (lambda: (_x(300, 128), _meta(E0, 128 * 128, 16, dtype=torch.int32),
                                _meta(E0, 128 * 128, 1, dtype=torch.float32)),
                       dict(row_idx=_meta((128 << 24) - 128, dtype=torch.int32)), "16777217 row-tile slots"),
    "the 2^32 bound": (lambda: (_meta(1 << 21, 1024), _w4(1024), _s(8)), {}, "reaches 2\\^32 bytes"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    ops = _no_library(monkeypatch)
    make, kw, reason = REFUSED[case]
    X, Wq, s_w = make()
    assert ops.moe_gemm_wq_tile_supported(X, Wq, s_w, None, kw.get("g_idx"), kw.get("row_idx")) is False
    with pytest.raises(ValueError, match="moe_gemm_wq_tile: .*" + reason):
        ops.moe_gemm_wq_tile(X, Wq, s_w, torch.zeros(Wq.shape[0] + 1, dtype=torch.int32), **kw)


# ---- WeightOnlyExperts -----------------------------------------------------------------------------------------------
@pytest.fixture
def log(recorded, monkeypatch):     # noqa: F811
    ops, log = recorded

    def tile(X, Wq, s_w, offsets, *, row_idx=None, K=None, zp_w=None, g_idx=None):
        R = X.shape[0] if row_idx is None else row_idx.numel()
        log.append(("tile", "gate_up" if row_idx is not None else "down", R))
        return torch.zeros(R, Wq.shape[1], dtype=X.dtype)

    monkeypatch.setattr(ops, "moe_gemm_wq_tile", tile)
    return log


def test_tile_max_tokens_takes_the_calls_above_the_other_ranges(log):
    from quantool_amd.engine.qmodules import WeightOnlyExperts

    assert WeightOnlyExperts.tile_max_tokens == 0
    woe, bank = _experts()
    assert "tile_max_tokens=0" in repr(woe)
    woe.wide_min_tokens, woe.tile_max_tokens = 0, 300
    assert "tile_max_tokens=300" in repr(woe)
    for T in (128, 129, 300, 301):
        _run(woe, T)
    assert log == [("grouped", "gate_up", 256), ("grouped", "down", 256), ("tile", "gate_up", 258), ("tile", "down", 258),
                   ("tile", "gate_up", 600), ("tile", "down", 600)]
    assert bank.calls == 1                                              # 301
    del log[:]
    woe.wide_max_tokens, woe.tile_max_tokens = 200, 300                 # the wide range first, the tile range above it
    for T in (200, 201):
        _run(woe, T)
    assert log == [("wide", "gate_up", 400), ("wide", "down", 400), ("tile", "gate_up", 402), ("tile", "down", 402)]
    del log[:]
    for kw in (dict(g_idx=True), dict(K_ragged=True)):                  # a bank with an unsupported product: as before
        other, other_bank = _experts(**kw)
        other.tile_max_tokens = 300
        _run(other, 200)
        assert other_bank.calls == 1 and log == [], kw


def test_with_zero_no_tile_name_is_read(log, monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.delattr(ops, "moe_gemm_wq_tile")
    monkeypatch.delattr(ops, "moe_gemm_wq_tile_supported")
    woe, bank = _experts()
    woe.wide_max_tokens = 300
    for T in (64, 200, 301, 4096):
        _run(woe, T)
    assert [name for name, _, _ in log] == ["grouped"] * 2 + ["wide"] * 2 and bank.calls == 2


# ---- load_quantized -------------------------------------------------------------------------------------------------
def test_loader_sets_tile_tokens(tmp_path):
    from quantool_amd.engine.qlinear import A16_EXPERTS_TILE_MAX_TOKENS, WeightOnlyExperts, load_quantized

    _write(tmp_path, "W4A16")
    kw = dict(device="cpu", a16="packed", a16_experts="packed")
    model = load_quantized(tmp_path, **kw)
    assert model.get_submodule(BANK).tile_max_tokens == 0 and model._qt_checkpoint["a16_experts_tile_tokens"] == 0
    model = load_quantized(tmp_path, a16_experts_tile_tokens=2048, a16_experts_wide_tokens=384, **kw)
    woe = model.get_submodule(BANK)
    assert woe.tile_max_tokens == 2048 and "tile_max_tokens" in vars(woe) and woe.wide_max_tokens == 384
    assert WeightOnlyExperts.tile_max_tokens == 0                        # an instance attribute: the class keeps 0
    assert model._qt_checkpoint["a16_experts_tile_tokens"] == 2048 and "tile_max_tokens=2048" in repr(woe)
    for ok in (129, A16_EXPERTS_TILE_MAX_TOKENS):
        assert load_quantized(tmp_path, a16_experts_tile_tokens=ok, **kw).get_submodule(BANK).tile_max_tokens == ok
    for bad in (dict(a16_experts_tile_tokens=128), dict(a16_experts_tile_tokens=A16_EXPERTS_TILE_MAX_TOKENS + 1),
                dict(a16_experts_tile_tokens=-1), dict(a16_experts_tile_tokens=256.0),
                dict(a16_experts_tile_tokens=384, a16_experts_wide_tokens=384)):
        with pytest.raises(ValueError, match="a16_experts_tile_tokens"):
            load_quantized(tmp_path, **bad, **kw)
    with pytest.raises(ValueError, match="needs a16_experts='packed'"):
        load_quantized(tmp_path, device="cpu", a16="packed", a16_experts_tile_tokens=512)
    assert "a16_experts_tile_tokens" not in load_quantized(tmp_path, device="cpu", a16="packed")._qt_checkpoint
    _write(tmp_path / "a8", "W4A8")                                      # A8 checkpoints ignore it
    model = load_quantized(tmp_path / "a8", a16_experts_tile_tokens=512, **kw)
    assert "a16_experts_tile_tokens" not in model._qt_checkpoint
