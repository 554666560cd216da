"""``qt_gemm_wq_tile``'s surface without a GPU: the header, the ctypes table and the built library carry it,
``ops.gemm_wq_tile_supported`` / ``ops.gemm_wq_tile`` refuse what the kernel does not take before they touch the library,
``load_quantized(..., a16_tile_rows=)`` switches it on, and ``WeightOnlyLinear`` takes it last before dequantising."""
import pytest
import torch

from tests.i8_fake_ops import aligned_i8, check_surface, header_constants, header_text
from tests.test_qlinear_loader import _write as _write_llama
from tests.test_wq_panel_dispatch import _linear, _route, routed  # noqa: F401
from tests.test_wq_stream_dispatch import REFUSED, _no_library, _w4, _x

NAME = "qt_gemm_wq_tile"


def test_surface():
    from quantool_amd.hip import ops

    check_surface("header", NAME)
    check_surface("ctypes", NAME, "qt_gemm_wq_skinny")
    check_surface("library", NAME)
    assert header_constants("QT_WQ_TILE_") == {"QT_WQ_TILE_K_UNIT": ops.WQ_TILE_K_UNIT,
                                               "QT_WQ_TILE_MAX_LDX": ops.WQ_TILE_MAX_LDX}
    assert f"{NAME}:" in header_text()[0]                 # documented in the A16 block's comment


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    ops = _no_library(monkeypatch)
    make, kw, reason = REFUSED[case]
    X, Wq, s_w = make()
    assert ops.gemm_wq_tile_supported(X, Wq, s_w, **kw) is False
    with pytest.raises(ValueError, match=reason):
        ops.gemm_wq_tile(X, Wq, s_w, **kw)


def test_rows_and_pitch_out_of_range_and_supported_operands(monkeypatch):
    ops = _no_library(monkeypatch)
    with pytest.raises(ValueError, match="M >= 1"):
        ops.gemm_wq_tile(_x(0, 1024), _w4(8, 1024), torch.ones(8, 8))
    far = _x(2, 1024, pitch=(1 << 23) + 8)                  # a pitch the panel kernel takes and this one does not
    assert ops.gemm_wq_panel_supported(far, _w4(8, 1024), torch.ones(8, 8)) is True
    assert ops.gemm_wq_tile_supported(far, _w4(8, 1024), torch.ones(8, 8)) is False
    for M in (1, 129, 5000):
        assert ops.gemm_wq_tile_supported(_x(M, 1024, pitch=1032), aligned_i8(8, 1024), torch.ones(8, 1),
                                          torch.zeros(8, 1, dtype=torch.int8))


def test_loader_sets_tile_rows(tmp_path):
    from quantool_amd.engine.qlinear import WeightOnlyLinear, load_quantized

    path, _, levels = _write_llama(tmp_path, "W4A16")
    model = load_quantized(path, device="cpu", a16="packed")
    assert model._qt_checkpoint["a16_tile_rows"] == 0
    model = load_quantized(path, device="cpu", a16="packed", a16_stream_rows=32, a16_panel_rows=96, a16_tile_rows=2048)
    wols = [m for m in model.modules() if isinstance(m, WeightOnlyLinear)]
    assert len(wols) == len(levels) and all(vars(m)["tile_max_m"] == 2048 for m in wols)
    assert WeightOnlyLinear.tile_max_m == 0 and model._qt_checkpoint["a16_tile_rows"] == 2048
    with pytest.raises(ValueError, match="needs a16='packed'"):
        load_quantized(path, device="cpu", a16_tile_rows=2048)
    for kw in (dict(a16_tile_rows=16), dict(a16_tile_rows=-1), dict(a16_tile_rows=2.0),
               dict(a16_stream_rows=64, a16_tile_rows=64), dict(a16_panel_rows=512, a16_tile_rows=512)):
        with pytest.raises(ValueError, match="a16_tile_rows"):
            load_quantized(path, device="cpu", a16="packed", **kw)
    assert "a16_tile_rows" not in load_quantized(path, device="cpu")._qt_checkpoint


@pytest.fixture
def routed_tile(routed, monkeypatch):  # noqa: F811
    """``routed`` with a recording fake for the tile product, and a tripwire in place of the host check."""
    from quantool_amd.hip import ops

    def tile(X, Wq, s_w, zp_w=None, bias=None, out=None):
        routed.append("tile")
        return torch.zeros(X.shape[0], Wq.shape[0], dtype=X.dtype)

    monkeypatch.setattr(ops, "gemm_wq_tile", tile)
    return routed


def test_default_touches_no_tile_name(routed, monkeypatch):  # noqa: F811
    from quantool_amd.engine.qmodules import WeightOnlyLinear
    from quantool_amd.hip import ops

    monkeypatch.delattr(ops, "gemm_wq_tile")
    monkeypatch.delattr(ops, "gemm_wq_tile_supported")
    assert WeightOnlyLinear.tile_max_m == 0
    for name in ("tile_min_k", "tile_min_n", "tile_max_n"):
        assert type(getattr(WeightOnlyLinear, name)) is int and getattr(WeightOnlyLinear, name) >= 0
    m = _linear()
    assert "tile_max_m=0" in repr(m)
    assert [_route(m, routed, M) for M in (16, 17, 200, 5000)] == ["skinny"] + ["dequantize"] * 3


def test_branch_order_stream_panel_tile_dequantize(routed_tile, monkeypatch):
    from quantool_amd.engine.qmodules import WeightOnlyLinear

    for name in ("stream_max_n", "stream_min_k", "panel_min_k", "panel_min_n", "panel_max_n", "tile_min_k", "tile_min_n",
                 "tile_max_n"):
        monkeypatch.setattr(WeightOnlyLinear, name, 0)          # the rules under test, whatever the measured bounds
    m = _linear()
    m.tile_max_m = 1000
    assert [_route(m, routed_tile, M) for M in (16, 17, 1000, 1001)] == ["skinny", "tile", "tile", "dequantize"]
    m.stream_max_m, m.panel_max_m = 32, 200
    assert [_route(m, routed_tile, M) for M in (16, 17, 32, 33, 200, 201, 1000, 1001)] == [
        "skinny", "stream", "stream", "panel", "panel", "tile", "tile", "dequantize"]
    m.panel_max_m = 2000                                        # past the panel kernel's own 512 rows: the tile's
    assert [_route(m, routed_tile, M) for M in (512, 513)] == ["panel", "tile"]
    m.panel_min_n = 65                                          # a Linear outside the panel's bounds: the tile from row 33
    assert [_route(m, routed_tile, M) for M in (32, 33, 200)] == ["stream", "tile", "tile"]
    m.stream_max_m = 0
    assert _route(m, routed_tile, 17) == "tile"
    for attr, bad in (("tile_min_k", 1025), ("tile_min_n", 65), ("tile_max_n", 63)):      # the tile's own size bounds
        setattr(m, attr, bad)
        assert _route(m, routed_tile, 100) == "dequantize", attr
        setattr(m, attr, 0)
