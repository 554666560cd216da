"""The grouped LDS-ring int8 GEMM's surface without a GPU: the header, the ctypes table and the built library carry
``qt_gemm_i8_ring_grouped``, ``ops.gemm_i8_ring_grouped_supported`` / ``ops.gemm_i8_ring_grouped`` refuse what the kernel
does not take before they touch the library, and ``QuantizedExperts`` picks the ring by ``ring_min_rows_per_expert``
(with ``quantool_amd.hip.ops`` replaced by a recording fake, so nothing reaches a device)."""
import re

import pytest
import torch
import torch.nn as nn

from tests.i8_fake_ops import Recorder, aligned_i8, check_surface, fake_ops, header_text  # noqa: F401

NAME = "qt_gemm_i8_ring_grouped"
WATCH = "gemm_i8_ring_grouped_supported"


# ---- surface --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point():
    check_surface("header", NAME)
    text = header_text()[1]
    decl = re.search(NAME + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert args[-2:] == ["int64_t x_rows", "qt_stream_t stream"]
    tiled = re.search(r"qt_gemm_i8_grouped\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert [a.strip() for a in tiled.split(",")] == args[:-2] + args[-1:]


def test_ctypes_table_holds_the_grouped_signature_plus_one_int64():
    from ctypes import c_int64

    from quantool_amd.hip import _lib

    res, args = _lib.SIGNATURES[NAME]
    tiled_res, tiled_args = _lib.SIGNATURES["qt_gemm_i8_grouped"]
    assert res is tiled_res
    assert args == tiled_args[:-1] + [c_int64] + tiled_args[-1:]       # x_rows, in front of the stream


def test_library_exports_it():
    check_surface("library", NAME)


def test_no_workspace_function_was_added():
    from quantool_amd.hip import _lib

    assert not [n for n in _lib.SIGNATURES if "ring" in n and n.endswith("_workspace_bytes")]


def test_build_audits_cover_the_grouped_kernel():
    from quantool_amd.csrc import build

    assert any(k in "gemm_i8_ring_moe_kernel" for k in build.NO_SPILL_KERNELS)
    src = (build.CSRC / "qlinear_ring.hip").read_text()
    assert "gemm_i8_ring_moe_kernel" in src and NAME in src
    res = build.OBJ_DIR / "qlinear_ring.resources.txt"
    if res.exists():                                                    # written by the build: no scratch, no spills
        rows = [line for line in res.read_text().splitlines() if "gemm_i8_ring" in line]
        assert len(rows) == 2
        for row in rows:                                                # both instances: 2 waves per SIMD
            assert "scratch 0\t" in row and "vgpr_spill 0\t" in row and row.endswith("waves_per_simd 2")


# ---- refusals before the library ------------------------------------------------------------------------------------
CASES = ["packed int4", "G = K/128 > 1", "ragged K", "K past the accumulator bound", "the 2^32 bound", "E > 4096",
         "too many tiles"]


def _refused(case):
    """(Xq, Wq, s_w, row_idx, reason).  The oversized operands are expanded views: their shape is all that is read."""
    from quantool_amd.hip import ops

    U = ops.I8_RING_K_UNIT
    i8 = lambda *s: torch.zeros(*s, dtype=torch.int8)   # noqa: E731
    idx = torch.zeros(4, dtype=torch.int32)
    if case == "packed int4":
        return i8(4, 256), torch.zeros(2, 8, 32, dtype=torch.int32), torch.ones(2, 8, 1), idx, "int8 weights only"
    if case == "G = K/128 > 1":
        return i8(4, 256), i8(2, 8, 256), torch.ones(2, 8, 2), idx, "one scale group"
    if case == "ragged K":
        return i8(4, U + 64), i8(2, 8, U + 64), torch.ones(2, 8, 1), idx, "not a multiple"
    if case == "K past the accumulator bound":
        return i8(1, 32768 + U), i8(2, 2, 32768 + U), torch.ones(2, 2, 1), idx, "32768"
    if case == "the 2^32 bound":
        K = 4096
        Xq = i8(1, K).expand(2 ** 32 // K + 1, K)
        return Xq, i8(2, 8, K), torch.ones(2, 8, 1), idx, r"2\^32"
    if case == "E > 4096":
        return i8(4, U), i8(1, 1, U).expand(4097, 1, U), torch.ones(4097, 1, 1), idx, "4096"
    if case == "too many tiles":
        R, N = 2 ** 31 - 1, 2 ** 20
        big_idx = torch.zeros(1, dtype=torch.int32).expand(R)
        return i8(4, U), i8(1, 1, U).expand(2, N, U), torch.ones(1, 1, 1).expand(2, N, 1), big_idx, "too many tiles"
    raise KeyError(case)


@pytest.mark.parametrize("case", CASES)
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    from quantool_amd.hip import ops

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(ops, "load", boom)
    Xq, Wq, s_w, row_idx, reason = _refused(case)
    assert ops.gemm_i8_ring_grouped_supported(Xq, Wq, s_w, row_idx) is False
    with pytest.raises(ValueError, match=reason):
        ops.gemm_i8_ring_grouped(Xq, torch.ones(Xq.shape[0]), Wq, s_w, torch.zeros(Wq.shape[0] + 1, dtype=torch.int32),
                                 row_idx=row_idx, K=Xq.shape[1])


def test_the_2_32_bound_is_about_gathered_rows_only(monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    K = 4096
    Wq, s_w = torch.zeros(2, 8, K, dtype=torch.int8), torch.ones(2, 8, 1)
    idx = torch.zeros(4, dtype=torch.int32)
    at = torch.zeros(1, K, dtype=torch.int8).expand(2 ** 32 // K, K)
    past = torch.zeros(1, K, dtype=torch.int8).expand(2 ** 32 // K + 1, K)
    assert ops.gemm_i8_ring_grouped_supported(at, Wq, s_w, idx) is True
    assert ops.gemm_i8_ring_grouped_supported(past, Wq, s_w, idx) is False
    assert ops.gemm_i8_ring_grouped_supported(past, Wq, s_w, None) is True     # contiguous rows: tile-relative offsets


def test_supported_operands_and_alignment(monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    U = ops.I8_RING_K_UNIT
    Wq, s_w = torch.zeros(2, 8, 4 * U, dtype=torch.int8), torch.ones(2, 8, 1)
    aligned, shifted = aligned_i8(4, 4 * U), aligned_i8(4, 4 * U, shift=1)
    assert aligned.data_ptr() % 16 == 0 and Wq.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 1
    assert ops.gemm_i8_ring_grouped_supported(aligned, Wq, s_w) is True
    assert ops.gemm_i8_ring_grouped_supported(aligned, Wq, s_w, torch.zeros(9, dtype=torch.int32)) is True
    assert ops.gemm_i8_ring_grouped_supported(shifted, Wq, s_w) is False
    assert ops.gemm_i8_ring_grouped_supported(aligned, shifted.view(1, 4, 4 * U), torch.ones(1, 4, 1)) is False
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.gemm_i8_ring_grouped(shifted, torch.ones(4), Wq, s_w, torch.zeros(3, dtype=torch.int32))


# ---- dispatch -------------------------------------------------------------------------------------------------------
E, TOPK = 4, 2


def _experts(H=256, I=128, int4=False):
    from quantool_amd.engine.qmodules import QuantizedExperts

    if int4:
        gu, dn = torch.zeros(E, 2 * I, H // 8, dtype=torch.int32), torch.zeros(E, H, I // 8, dtype=torch.int32)
        s_gu, s_dn = torch.ones(E, 2 * I, H // 128), torch.ones(E, H, I // 128)
    else:
        gu, dn = torch.zeros(E, 2 * I, H, dtype=torch.int8), torch.zeros(E, H, I, dtype=torch.int8)
        s_gu, s_dn = torch.ones(E, 2 * I, 1), torch.ones(E, H, 1)
    return QuantizedExperts(H, I, gu, s_gu, dn, s_dn, nn.SiLU(), not int4)


def _forward(fake_ops, qe, T):
    fake_ops.calls.clear()
    out = qe(torch.zeros(T, qe.hidden_dim, dtype=torch.bfloat16), torch.zeros(T, TOPK, dtype=torch.int64),
             torch.ones(T, TOPK))
    assert out.shape == (T, qe.hidden_dim)
    return fake_ops.calls


def test_the_attribute_is_a_non_negative_int():
    from quantool_amd.engine.qmodules import QuantizedExperts

    assert type(QuantizedExperts.ring_min_rows_per_expert) is int and QuantizedExperts.ring_min_rows_per_expert >= 0


def test_quantized_experts_send_enough_rows_per_expert_to_the_ring(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedExperts

    monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", 16)
    monkeypatch.setattr(QuantizedExperts, "ring_min_rows_per_expert", 32)
    qe = _experts()
    # R = T * TOPK routed rows over E = 4 experts: R / E = 32 at T = 64
    assert _forward(fake_ops, qe, 63) == [("gemm_i8_grouped", 126)] * 2
    assert fake_ops.asked == []                       # below the bound the new names are not touched
    assert _forward(fake_ops, qe, 64) == [("gemm_i8_ring_grouped", 128)] * 2
    # R is taken from row_idx for the gathered product and from x for the contiguous one
    assert fake_ops.asked == [128, None]
    assert _forward(fake_ops, qe, 500) == [("gemm_i8_ring_grouped", 1000)] * 2


def test_skinny_range_keeps_precedence(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedExperts

    monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", 16)
    monkeypatch.setattr(QuantizedExperts, "ring_min_rows_per_expert", 1)
    qe = _experts()
    for T in (1, 16):
        assert _forward(fake_ops, qe, T) == [("gemm_i8_skinny_grouped", T * TOPK)] * 2
    assert fake_ops.asked == []
    assert _forward(fake_ops, qe, 17) == [("gemm_i8_ring_grouped", 34)] * 2


def test_attribute_zero_never_uses_the_ring(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedExperts

    monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", 16)
    monkeypatch.setattr(QuantizedExperts, "ring_min_rows_per_expert", 0)
    qe = _experts()
    for T in (17, 64, 4096):
        assert _forward(fake_ops, qe, T) == [("gemm_i8_grouped", T * TOPK)] * 2
    assert fake_ops.asked == []


def test_int4_bank_stays_on_the_tiled_gemm(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedExperts

    monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", 16)
    monkeypatch.setattr(QuantizedExperts, "ring_min_rows_per_expert", 1)
    assert _forward(fake_ops, _experts(int4=True), 1024) == [("gemm_i8_grouped", 2048)] * 2
    assert fake_ops.asked == []                       # W4A8 never reaches the ring, nor its check


def test_a_ragged_k_falls_to_the_tiled_gemm(monkeypatch):
    """K = 192 with the real host-side check: the gate_up product (K = H = 192) is refused, the down product
    (K = I = 128) is taken."""
    import quantool_amd.hip as hip
    from quantool_amd.engine.qmodules import QuantizedExperts
    from quantool_amd.hip import ops as real

    rec = Recorder(WATCH)
    rec.gemm_i8_ring_grouped_supported = real.gemm_i8_ring_grouped_supported
    monkeypatch.setattr(real, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    monkeypatch.setattr(hip, "ops", rec)
    monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", 16)
    monkeypatch.setattr(QuantizedExperts, "ring_min_rows_per_expert", 1)
    qe = _experts(H=192, I=128)
    assert _forward(rec, qe, 64) == [("gemm_i8_grouped", 128), ("gemm_i8_ring_grouped", 128)]


def test_unsupported_operands_fall_to_the_tiled_gemm(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedExperts

    monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", 16)
    monkeypatch.setattr(QuantizedExperts, "ring_min_rows_per_expert", 1)
    fake_ops.supported = False
    assert _forward(fake_ops, _experts(), 64) == [("gemm_i8_grouped", 128)] * 2
    assert len(fake_ops.asked) == 2
