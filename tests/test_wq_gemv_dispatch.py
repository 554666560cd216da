"""``qt_gemm_wq_gemv`` / ``qt_gemm_wq_gemv_act_mul`` without a GPU: the header, the ctypes table and the built library
carry them, ``load_quantized(..., a16_gemv_rows=)`` switches the kernel on, and ``WeightOnlyLinear`` asks for it in
front of the skinny kernel only when told to."""
import pytest
import torch

from tests.i8_fake_ops import check_surface, header_constants, header_text
from tests.test_qlinear_loader import _write as _write_llama
from tests.test_wq_panel_dispatch import _linear, _route, routed  # noqa: F401


@pytest.mark.parametrize("name,like", [("qt_gemm_wq_gemv", "qt_gemm_wq_skinny"),
                                       ("qt_gemm_wq_gemv_act_mul", "qt_gemm_wq_skinny_act_mul")])
def test_surface(name, like):
    from quantool_amd.hip import _lib, ops

    check_surface("header", name)
    check_surface("ctypes", name, like)
    check_surface("library", name)
    assert header_constants("QT_WQ_GEMV_") == {"QT_WQ_GEMV_MAX_M": ops.WQ_GEMV_MAX_M, "QT_WQ_GEMV_K_UNIT": 128}
    assert f"{name}:" in header_text()[0]                 # documented in the A16 block's comment
    assert sum(n.endswith("_workspace_bytes") for n in _lib.SIGNATURES) == 14


def test_loader_sets_gemv_rows(tmp_path):
    from quantool_amd.engine.qlinear import WeightOnlyLinear, load_quantized

    path, _, levels = _write_llama(tmp_path, "W4A16")
    model = load_quantized(path, device="cpu", a16="packed")
    assert model._qt_checkpoint["a16_gemv_rows"] == 0 and not any("gemv_max_m" in vars(m) for m in model.modules())
    model = load_quantized(path, device="cpu", a16="packed", a16_gemv_rows=4)
    wols = [m for m in model.modules() if isinstance(m, WeightOnlyLinear)]
    assert len(wols) == len(levels) and all(vars(m)["gemv_max_m"] == 4 for m in wols)
    assert WeightOnlyLinear.gemv_max_m == 0 and model._qt_checkpoint["a16_gemv_rows"] == 4
    for kw in (dict(a16="packed", a16_gemv_rows=-1), dict(a16="packed", a16_gemv_rows=5),
               dict(a16="packed", a16_gemv_rows=2.0), dict(a16_gemv_rows=4)):
        with pytest.raises(ValueError, match="a16_gemv_rows"):
            load_quantized(path, device="cpu", **kw)
    assert "a16_gemv_rows" not in load_quantized(path, device="cpu")._qt_checkpoint


def test_default_touches_no_gemv_name(routed, monkeypatch):  # noqa: F811
    from quantool_amd.engine.qmodules import WeightOnlyLinear
    from quantool_amd.hip import ops

    for name in ("gemm_wq_gemv", "gemm_wq_gemv_supported", "gemm_wq_gemv_act_mul", "WQ_GEMV_MAX_M"):
        monkeypatch.delattr(ops, name)
    assert (WeightOnlyLinear.gemv_max_m, WeightOnlyLinear.gemv_min_k, WeightOnlyLinear.gemv_max_n) == (0, 0, 0)
    m = _linear()
    assert repr(m).endswith("gemv_max_m=0)")
    assert [_route(m, routed, M) for M in (1, 4, 5)] == ["skinny"] * 3


def test_rows_bounds_and_support_pick_the_gemv(routed, monkeypatch):  # noqa: F811
    from quantool_amd.hip import ops

    def gemv(X, Wq, s_w, zp_w=None, bias=None, out=None):
        routed.append("gemv")
        return torch.zeros(X.shape[0], Wq.shape[0], dtype=X.dtype)

    monkeypatch.setattr(ops, "gemm_wq_gemv", gemv)
    m = _linear()
    m.gemv_max_m = 4
    assert [_route(m, routed, M) for M in (1, 4, 5, 16)] == ["gemv", "gemv", "skinny", "skinny"]
    m.gemv_max_m = 16                                           # the kernel's own bound holds under a larger attribute
    assert [_route(m, routed, M) for M in (4, 5)] == ["gemv", "skinny"]
    for attr, bad in (("gemv_min_k", 1025), ("gemv_max_n", 63)):
        setattr(m, attr, bad)
        assert _route(m, routed, 1) == "skinny", attr
        setattr(m, attr, 0)
    monkeypatch.setattr(ops, "gemm_wq_gemv_supported", lambda *a: False)
    assert _route(m, routed, 1) == "skinny"
