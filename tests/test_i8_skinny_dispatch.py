"""The A8 decode GEMV's surface without a GPU: the header, the ctypes table and the built library carry the two entry
points, ``ops.gemm_i8_skinny`` refuses M outside 1..16 before it touches the library, and ``QuantizedLinear`` /
``QuantizedExperts`` pick the decode form by the row / token count (with ``quantool_amd.hip.ops`` replaced by recording
fakes, so nothing reaches a device)."""
import pytest
import torch
import torch.nn as nn

from tests.i8_fake_ops import check_surface, fake_ops  # noqa: F401

NAMES = ("qt_gemm_i8_skinny", "qt_gemm_i8_skinny_grouped")


def test_header_declares_both_entry_points():
    for n in NAMES:
        check_surface("header", n)


def test_ctypes_table_holds_both_with_the_tiled_signatures():
    from ctypes import c_int, c_int64

    from quantool_amd.hip import _lib

    for n in NAMES:
        assert n in _lib.SIGNATURES
    # the grouped form takes qt_gemm_i8_grouped's arguments; the GEMV qt_gemm_i8's, with M an int
    check_surface("ctypes", "qt_gemm_i8_skinny_grouped", "qt_gemm_i8_grouped")
    tiled, skinny = _lib.SIGNATURES["qt_gemm_i8"], _lib.SIGNATURES["qt_gemm_i8_skinny"]
    assert tiled[1][1] is c_int64 and skinny[1][1] is c_int
    assert skinny[0] is tiled[0] and skinny[1][:1] + skinny[1][2:] == tiled[1][:1] + tiled[1][2:]


def test_library_exports_both():
    for n in NAMES:
        check_surface("library", n)


def test_no_workspace_function_was_added():
    from quantool_amd.hip import _lib

    assert not [n for n in _lib.SIGNATURES if "skinny" in n and n.endswith("_workspace_bytes")]


@pytest.mark.parametrize("M", [0, 17])
def test_ops_refuses_m_out_of_range_before_the_library(monkeypatch, M):
    from quantool_amd.hip import ops

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(ops, "load", boom)
    assert ops.I8_SKINNY_MAX_M == 16
    Xq = torch.zeros(M, 128, dtype=torch.int8)
    with pytest.raises(ValueError, match="1 <= M <= 16"):
        ops.gemm_i8_skinny(Xq, torch.ones(M), torch.zeros(8, 128, dtype=torch.int8), torch.ones(8, 1))


# ---- dispatch -------------------------------------------------------------------------------------------------------
def _linear(K=256, N=24, int4=False):
    from quantool_amd.engine.qmodules import QuantizedLinear

    w = torch.zeros(N, K // 8, dtype=torch.int32) if int4 else torch.zeros(N, K, dtype=torch.int8)
    return QuantizedLinear(K, N, w, torch.ones(N, K // 128 if int4 else 1), act_symmetric=not int4)


@pytest.mark.parametrize("int4", [False, True])
def test_quantized_linear_sends_decode_sizes_to_the_skinny_gemm(fake_ops, int4):
    lin = _linear(int4=int4)
    assert type(lin).skinny_max_m >= 0
    lin.skinny_max_m = 16
    for shape, want in (((1, 256), ("gemm_i8_skinny", 1)), ((16, 256), ("gemm_i8_skinny", 16)),
                        ((17, 256), ("gemm_i8", 17)), ((2, 9, 256), ("gemm_i8", 18)),
                        ((2, 8, 256), ("gemm_i8_skinny", 16))):
        fake_ops.calls.clear()
        y = lin(torch.zeros(shape, dtype=torch.bfloat16))
        assert fake_ops.calls == [want]
        assert y.shape == (*shape[:-1], 24) and y.dtype == torch.bfloat16
    lin.skinny_max_m = 4                      # the attribute is the bound, capped by the kernel's own
    for M, name in ((4, "gemm_i8_skinny"), (5, "gemm_i8")):
        fake_ops.calls.clear()
        lin(torch.zeros(M, 256, dtype=torch.bfloat16))
        assert fake_ops.calls == [(name, M)]
    lin.skinny_max_m = 64
    fake_ops.calls.clear()
    lin(torch.zeros(17, 256, dtype=torch.bfloat16))
    assert fake_ops.calls == [("gemm_i8", 17)]


def test_quantized_linear_with_zero_keeps_the_tiled_gemm(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "skinny_max_m", 0)
    lin = _linear()
    for shape in ((1, 256), (16, 256), (17, 256), (2, 9, 256)):
        lin(torch.zeros(shape, dtype=torch.float16))
    assert [c[0] for c in fake_ops.calls] == ["gemm_i8"] * 4


def _experts(E=4, H=256, I=128):
    from quantool_amd.engine.qmodules import QuantizedExperts

    return QuantizedExperts(H, I, torch.zeros(E, 2 * I, H, dtype=torch.int8), torch.ones(E, 2 * I, 1),
                            torch.zeros(E, H, I, dtype=torch.int8), torch.ones(E, H, 1), nn.SiLU(), True)


def test_quantized_experts_dispatch_on_the_token_count(fake_ops):
    qe = _experts()
    assert type(qe).grouped_max_tokens >= 0
    qe.grouped_max_tokens = 16
    k = 2
    for T, name in ((1, "gemm_i8_skinny_grouped"), (16, "gemm_i8_skinny_grouped"), (17, "gemm_i8_grouped")):
        fake_ops.calls.clear()
        out = qe(torch.zeros(T, 256, dtype=torch.bfloat16), torch.zeros(T, k, dtype=torch.int64), torch.ones(T, k))
        # both products of one forward take the same form: T decides, not the routed-row count T k of the second
        assert fake_ops.calls == [(name, T * k), (name, T * k)]
        assert out.shape == (T, 256)
    qe.grouped_max_tokens = 0
    fake_ops.calls.clear()
    for T in (1, 16, 17):
        qe(torch.zeros(T, 256, dtype=torch.bfloat16), torch.zeros(T, k, dtype=torch.int64), torch.ones(T, k))
    assert {c[0] for c in fake_ops.calls} == {"gemm_i8_grouped"} and len(fake_ops.calls) == 6
