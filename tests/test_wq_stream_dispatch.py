"""``qt_gemm_wq_stream``'s surface without a GPU: the header, the ctypes table and the built library carry it,
``ops.gemm_wq_stream_supported`` / ``ops.gemm_wq_stream`` refuse what the kernel does not take before they touch the
library, ``WeightOnlyLinear`` keeps it off by default, and ``load_quantized(..., a16_stream_rows=)`` switches it on."""
import re

import pytest
import torch

from tests.i8_fake_ops import aligned_i8, aligned_i32, check_surface, header_constants, header_text
from tests.test_qlinear_loader import _write as _write_llama

NAME = "qt_gemm_wq_stream"


# ---- surface --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_constants():
    from quantool_amd.hip import ops

    check_surface("header", NAME)
    assert header_constants("QT_WQ_STREAM_") == {"QT_WQ_STREAM_MAX_M": ops.WQ_STREAM_MAX_M,
                                                 "QT_WQ_STREAM_K_UNIT": ops.WQ_STREAM_K_UNIT,
                                                 "QT_WQ_STREAM_MAX_LDX": ops.WQ_STREAM_MAX_LDX}
    assert ops.WQ_STREAM_MAX_M == 128 and ops.WQ_STREAM_K_UNIT == 128
    assert f"{NAME}:" in header_text()[0]                 # documented in the A16 block's comment


def test_ctypes_table_holds_it_with_the_skinny_signature():
    check_surface("ctypes", NAME, "qt_gemm_wq_skinny")


def test_library_exports_it():
    check_surface("library", NAME)


def test_no_workspace_function_was_added():
    from quantool_amd.hip import _lib

    assert len([n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")]) == 14
    assert not [n for n in _lib.SIGNATURES if "stream" in n and n != NAME]


def test_every_instance_is_free_of_scratch():
    from quantool_amd.csrc import build

    res = build.OBJ_DIR / "wq.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    rows = [line for line in res.read_text().splitlines() if "wq_stream_kernel" in line]
    assert len(rows) == 64                                  # 1 ... 8 m-tiles x int4 / int8 x bf16 / fp16 x zp / none
    for row in rows:
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row
        assert int(re.search(r"lds (\d+)", row).group(1)) <= 65536, row


# ---- refusals before the library ------------------------------------------------------------------------------------
def _x(rows, K, shift=0, pitch=None, dtype=torch.bfloat16):
    """A zero 16-bit matrix whose first byte lies ``shift`` bytes behind a 16-byte boundary, rows ``pitch`` elements
    apart."""
    pitch = K if pitch is None else pitch
    buf = torch.zeros(max(rows, 1) * pitch + 32, dtype=dtype)
    off = ((-buf.data_ptr()) % 16) // 2 + shift // 2
    return buf[off:off + max(rows, 1) * pitch].view(max(rows, 1), pitch)[:rows, :K]


def _w4(N, K, shift=0):
    return aligned_i32(N, K // 8, shift // 4)


G_IDX = dict(g_idx=torch.zeros(1024, dtype=torch.int32))
REFUSED = {
    "g_idx given": (lambda: (_x(32, 1024), _w4(8, 1024), torch.ones(8, 8)), G_IDX, "actorder group runs on"),
    "K = 192": (lambda: (_x(32, 192), aligned_i8(8, 192), torch.ones(8, 1)), {}, "not a multiple of the k-unit 128"),
    "X shifted by 2 bytes": (lambda: (_x(32, 1024, shift=2), _w4(8, 1024), torch.ones(8, 8)), {}, "16-byte aligned"),
    "Wq shifted by 4 bytes": (lambda: (_x(32, 1024), _w4(8, 1024, shift=4), torch.ones(8, 8)), {}, "16-byte aligned"),
    "a pitch of K + 1": (lambda: (_x(32, 1024, pitch=1025), _w4(8, 1024), torch.ones(8, 8)), {}, "16-byte aligned"),
    "G = 3 at K = 1024": (lambda: (_x(32, 1024), _w4(8, 1024), torch.ones(8, 3)), {}, "G must be 1 or K / 128 = 8"),
    "fp32 X": (lambda: (_x(32, 1024, dtype=torch.float32), _w4(8, 1024), torch.ones(8, 8)), {}, "bf16 or fp16"),
    "float weights": (lambda: (_x(32, 1024), torch.zeros(8, 1024), torch.ones(8, 8)), {}, "weights only"),
}


def _no_library(monkeypatch):
    from quantool_amd.hip import _lib, ops

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(ops, "load", boom)
    return ops


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    ops = _no_library(monkeypatch)
    make, kw, reason = REFUSED[case]
    X, Wq, s_w = make()
    assert ops.gemm_wq_stream_supported(X, Wq, s_w, **kw) is False
    with pytest.raises(ValueError, match=reason):
        ops.gemm_wq_stream(X, Wq, s_w, **kw)


@pytest.mark.parametrize("M", [0, 129])
def test_rows_out_of_range_are_refused_before_the_library(monkeypatch, M):
    ops = _no_library(monkeypatch)
    with pytest.raises(ValueError, match="1 <= M <= 128"):
        ops.gemm_wq_stream(_x(M, 1024), _w4(8, 1024), torch.ones(8, 8))


def test_supported_operands(monkeypatch):
    ops = _no_library(monkeypatch)
    zp = torch.zeros(8, 8, dtype=torch.int8)
    for M in (1, 17, 128):
        for dtype in (torch.bfloat16, torch.float16):
            assert ops.gemm_wq_stream_supported(_x(M, 1024, dtype=dtype), _w4(8, 1024), torch.ones(8, 8)) is True
        assert ops.gemm_wq_stream_supported(_x(M, 1024), _w4(8, 1024), torch.ones(8, 1), zp[:, :1]) is True
        assert ops.gemm_wq_stream_supported(_x(M, 1024), aligned_i8(8, 1024), torch.ones(8, 8), zp, None) is True
        assert ops.gemm_wq_stream_supported(_x(M, 1024, pitch=1032), aligned_i8(8, 1024), torch.ones(8, 1)) is True


# ---- WeightOnlyLinear -----------------------------------------------------------------------------------------------
def test_the_kernel_is_off_by_default():
    from quantool_amd.engine.qmodules import WeightOnlyLinear

    assert WeightOnlyLinear.stream_max_m == 0
    for name in ("stream_max_n", "stream_min_k"):
        assert type(getattr(WeightOnlyLinear, name)) is int and getattr(WeightOnlyLinear, name) >= 0
    m = WeightOnlyLinear(1024, 8, _w4(8, 1024), torch.ones(8, 8))
    assert "stream_max_m=0" in repr(m)
    m.stream_max_m = 64
    assert "stream_max_m=64" in repr(m)


# ---- load_quantized -------------------------------------------------------------------------------------------------
def test_loader_sets_stream_rows(tmp_path):
    from quantool_amd.engine.qlinear import WeightOnlyLinear, load_quantized

    path, _, levels = _write_llama(tmp_path, "W4A16")
    model = load_quantized(path, device="cpu", a16="packed")
    wols = [m for m in model.modules() if isinstance(m, WeightOnlyLinear)]
    assert len(wols) == len(levels) and all(m.stream_max_m == 0 for m in wols)
    assert model._qt_checkpoint["a16_stream_rows"] == 0
    model = load_quantized(path, device="cpu", a16="packed", a16_stream_rows=64)
    wols = [m for m in model.modules() if isinstance(m, WeightOnlyLinear)]
    assert len(wols) == len(levels) and all(m.stream_max_m == 64 for m in wols)
    assert all("stream_max_m" in vars(m) for m in wols)                   # an instance attribute: the class keeps 0
    assert WeightOnlyLinear.stream_max_m == 0
    assert model._qt_checkpoint["a16_stream_rows"] == 64
    with pytest.raises(ValueError, match="needs a16='packed'"):
        load_quantized(path, device="cpu", a16_stream_rows=64)
    for bad in (16, 129, -1):
        with pytest.raises(ValueError, match="a16_stream_rows"):
            load_quantized(path, device="cpu", a16="packed", a16_stream_rows=bad)
    assert "a16_stream_rows" not in load_quantized(path, device="cpu")._qt_checkpoint


def test_a8_checkpoints_ignore_stream_rows(tmp_path):
    from quantool_amd.engine.qlinear import WeightOnlyLinear, load_quantized

    path, _, _ = _write_llama(tmp_path, "W8A8")
    model = load_quantized(path, device="cpu", a16="packed", a16_stream_rows=64)
    assert not any(isinstance(m, WeightOnlyLinear) for m in model.modules())
    assert "a16_stream_rows" not in model._qt_checkpoint
