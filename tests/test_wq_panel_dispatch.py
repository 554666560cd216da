"""``qt_gemm_wq_panel``'s surface without a GPU: the header, the ctypes table and the built library carry it,
``ops.gemm_wq_panel_supported`` / ``ops.gemm_wq_panel`` refuse what the kernel does not take before they
touch the library, and ``WeightOnlyLinear`` routes a call by its rows exactly at the attribute boundaries."""
import pytest
import torch

from tests.i8_fake_ops import aligned_i8, check_surface, header_constants, header_text
from tests.test_wq_moe_wide_dispatch import _OnDevice
from tests.test_wq_stream_dispatch import G_IDX, REFUSED, _no_library, _w4, _x

NAME = "qt_gemm_wq_panel"


def test_surface():
    from quantool_amd.hip import ops

    check_surface("header", NAME)
    check_surface("ctypes", NAME, "qt_gemm_wq_skinny")
    check_surface("library", NAME)
    assert header_constants("QT_WQ_PANEL_") == {"QT_WQ_PANEL_MAX_M": ops.WQ_PANEL_MAX_M,
                                                "QT_WQ_PANEL_K_UNIT": ops.WQ_PANEL_K_UNIT,
                                                "QT_WQ_PANEL_MAX_LDX": ops.WQ_PANEL_MAX_LDX}
    assert f"{NAME}:" in header_text()[0]                 # documented in the A16 block's comment


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    ops = _no_library(monkeypatch)
    make, kw, reason = REFUSED[case]
    X, Wq, s_w = make()
    assert ops.gemm_wq_panel_supported(X, Wq, s_w, **kw) is False
    with pytest.raises(ValueError, match=reason):
        ops.gemm_wq_panel(X, Wq, s_w, **kw)


def test_rows_and_pitch_out_of_range_and_supported_operands(monkeypatch):
    ops = _no_library(monkeypatch)
    for M in (0, 513):
        with pytest.raises(ValueError, match="1 <= M <= 512"):
            ops.gemm_wq_panel(_x(M, 1024), _w4(8, 1024), torch.ones(8, 8))
    far = _x(2, 1024, pitch=(1 << 24) + 8)                  # a pitch the stream kernel takes and this one does not
    assert ops.gemm_wq_stream_supported(far, _w4(8, 1024), torch.ones(8, 8)) is True
    assert ops.gemm_wq_panel_supported(far, _w4(8, 1024), torch.ones(8, 8)) is False
    zp = torch.zeros(8, 8, dtype=torch.int8)
    for M in (1, 33, 512):
        assert ops.gemm_wq_panel_supported(_x(M, 1024, dtype=torch.float16), _w4(8, 1024), torch.ones(8, 8)) is True
        assert ops.gemm_wq_panel_supported(_x(M, 1024, pitch=1032), aligned_i8(8, 1024), torch.ones(8, 1), zp[:, :1])


# ---- WeightOnlyLinear -----------------------------------------------------------------------------------------------
@pytest.fixture
def routed(monkeypatch):
    """``ops`` with every product of ``WeightOnlyLinear.forward`` replaced by a recording fake, and no library."""
    ops = _no_library(monkeypatch)
    log = []

    def product(name):
        def f(X, Wq, s_w, *, zp_w=None, g_idx=None, bias=None):
            log.append(name)
            return torch.zeros(X.shape[0], Wq.shape[0], dtype=X.dtype)
        return f

    def dequantize(Wq, s_w, *, K=None, zp_w=None, g_idx=None, dtype=torch.bfloat16):
        log.append("dequantize")
        return torch.zeros(Wq.shape[0], K, dtype=dtype)

    for name in ("skinny", "stream", "panel"):
        monkeypatch.setattr(ops, f"gemm_wq_{name}", product(name))
    monkeypatch.setattr(ops, "dequantize_weight", dequantize)
    return log


def _route(m, log, M):
    del log[:]
    y = m(torch.zeros(M, m.in_features, dtype=torch.bfloat16).as_subclass(_OnDevice))
    assert y.shape == (M, m.out_features) and len(log) == 1
    return log[0]


def _linear(N=64, K=1024, **kw):
    from quantool_amd.engine.qmodules import WeightOnlyLinear

    return WeightOnlyLinear(K, N, _w4(N, K), torch.ones(N, K // 128), **kw)


def test_defaults_call_nothing_new(routed):
    from quantool_amd.engine.qmodules import WeightOnlyLinear

    assert WeightOnlyLinear.panel_max_m == 0
    for name in ("panel_min_k", "panel_min_n", "panel_max_n"):
        assert type(getattr(WeightOnlyLinear, name)) is int and getattr(WeightOnlyLinear, name) >= 0
    m = _linear()
    assert "panel_max_m=0" in repr(m)
    assert [_route(m, routed, M) for M in (1, 16, 17, 64, 512, 513)] == ["skinny"] * 2 + ["dequantize"] * 4


def test_rows_pick_the_kernel_at_the_attribute_boundaries(routed, monkeypatch):
    from quantool_amd.engine.qmodules import WeightOnlyLinear

    for name in ("stream_max_n", "stream_min_k", "panel_min_k", "panel_min_n", "panel_max_n"):
        monkeypatch.setattr(WeightOnlyLinear, name, 0)          # the rules under test, whatever the measured bounds
    m = _linear()
    m.panel_max_m = 200
    assert [_route(m, routed, M) for M in (16, 17, 200, 201)] == ["skinny", "panel", "panel", "dequantize"]
    m.stream_max_m = 32
    assert [_route(m, routed, M) for M in (16, 17, 32, 33, 200, 201)] == [
        "skinny", "stream", "stream", "panel", "panel", "dequantize"]
    m.panel_max_m = 1024                                        # the kernel's own bound holds under a larger attribute
    assert [_route(m, routed, M) for M in (512, 513)] == ["panel", "dequantize"]
    m.panel_max_m, m.stream_max_m = 32, 32                      # nothing between the two
    assert _route(m, routed, 33) == "dequantize"
    # the size bounds: K from panel_min_k, N from panel_min_n and up to panel_max_n
    m.panel_max_m = 512
    for attr, ok, bad in (("panel_min_k", 1024, 1025), ("panel_min_n", 64, 65), ("panel_max_n", 64, 63)):
        setattr(m, attr, ok)
        assert _route(m, routed, 100) == "panel", attr
        setattr(m, attr, bad)
        assert _route(m, routed, 100) == "dequantize", attr
        setattr(m, attr, 0)
    # a Linear the kernel does not take stays on the dequantise path
    g = _linear(g_idx=G_IDX["g_idx"])
    g.panel_max_m = 512
    assert _route(g, routed, 100) == "dequantize"
