"""The W4A8 bank's LDS-ring GEMM without a GPU: the header, the ctypes table and the built library carry
``qt_moe_gemm_i8_ring_w4`` with ``qt_gemm_i8_ring_grouped``'s signature, ``ops.moe_gemm_i8_ring_w4_supported`` /
``ops.moe_gemm_i8_ring_w4`` refuse what the kernel does not take before they touch the library, and
``QuantizedExperts`` picks the ring by ``ring_w4_min_rows_per_expert`` (with ``quantool_amd.hip.ops`` replaced by a
recording fake that also carries the two new names, so nothing reaches a device)."""
import re

import pytest
import torch
import torch.nn as nn

from tests.i8_fake_ops import Recorder, aligned_i8, aligned_i32, check_surface, fake_ops, header_text  # noqa: F401

NAME = "qt_moe_gemm_i8_ring_w4"
GEMM = "moe_gemm_i8_ring_w4"
WATCH = "moe_gemm_i8_ring_w4_supported"
LIKE = "qt_gemm_i8_ring_grouped"
KERNEL = "gemm_i8_ring_w4_moe_kernel"


class W4Recorder(Recorder):
    """``Recorder`` with the W4A8 bank's two names: the GEMM records as the grouped ones do, ``asked`` lists the rows of
    row_idx (or None) of every ``moe_gemm_i8_ring_w4_supported`` call."""

    def __init__(self):
        super().__init__(WATCH)
        self.answers[WATCH] = True
        self.queries[WATCH] = []
        setattr(self, WATCH, self._supported(WATCH))
        setattr(self, GEMM, self._grouped(GEMM))

    @property
    def asked(self):
        return self.queries[WATCH]


@pytest.fixture
def w4_ops(monkeypatch):
    import quantool_amd.hip as hip
    from quantool_amd.hip import ops as real   # noqa: F401  (the attribute the modules import must exist first)

    rec = W4Recorder()
    monkeypatch.setattr(hip, "ops", rec)
    return rec


# ---- surface --------------------------------------------------------------------------------------------------------
def _declared_args(name, text):
    return [a.strip() for a in re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]


def test_header_declares_the_entry_point_with_the_grouped_rings_arguments():
    check_surface("header", NAME)
    text = header_text()[1]
    args = _declared_args(NAME, text)
    assert args == _declared_args(LIKE, text)
    assert args[-2:] == ["int64_t x_rows", "qt_stream_t stream"] and not [a for a in args if "bias" in a]


def test_header_states_the_contract():
    raw = re.sub(r"\s*\n\s*\*\s*", " ", header_text()[0])
    para = raw[raw.index(NAME + ":"):raw.index("qt_moe_combine:")]
    for must in ("bit-identical to qt_gemm_i8_grouped", "rows >= offsets[E] are not written", "clamped",
                 "No workspace, no atomics: deterministic"):
        assert must in para, must


def test_ctypes_table_holds_it_with_the_grouped_rings_signature():
    from quantool_amd.hip import _lib

    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES[LIKE]


def test_library_exports_it():
    check_surface("library", NAME)


def test_no_workspace_function_was_added():
    from quantool_amd.hip import _lib

    assert NAME + "_workspace_bytes" not in _lib.SIGNATURES
    assert not [n for n in _lib.SIGNATURES if "ring" in n and n.endswith("_workspace_bytes")]
    assert len([n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")]) == 14


def test_no_constant_was_added_to_the_header():
    from tests.i8_fake_ops import header_constants

    assert sorted(header_constants("QT_I8_RING_")) == ["QT_I8_RING_K_UNIT", "QT_I8_RING_LEAD", "QT_I8_RING_SLOTS"]
    assert sorted(header_constants("QT_I8_RING_W4_")) == ["QT_I8_RING_W4_K_UNIT", "QT_I8_RING_W4_LEAD",
                                                         "QT_I8_RING_W4_SLOTS"]


def test_the_form_stands_beside_the_table():
    from quantool_amd.hip import ops

    form = ops.I8_MOE_RING_W4_FORM
    dense = ops.I8_FORMS["qt_gemm_i8_ring_w4"]
    assert form.entry == NAME and NAME not in ops.I8_FORMS
    assert form.experts and form.max_e == 4096 and form.x_rows and form.dtypes == (torch.int32,)
    assert form.groups == "per_unit"
    assert (form.k_unit, form.aligned16, form.slots, form.lead) == (dense.k_unit, dense.aligned16, dense.slots, dense.lead)
    assert callable(getattr(ops, GEMM)) and callable(getattr(ops, WATCH))


def test_build_audits_cover_the_grouped_kernel():
    import inspect

    from quantool_amd.csrc import build

    assert KERNEL in build.NO_SPILL_KERNELS
    assert "gemm_i8_ring_w4_kernel" not in KERNEL
    assert '"qlinear_ring_w4.hip"' in inspect.getsource(build.build)    # audit_m0's list
    src = (build.CSRC / "qlinear_ring_w4.hip").read_text()
    assert KERNEL in src and NAME in src
    res = build.OBJ_DIR / "qlinear_ring_w4.resources.txt"
    if res.exists():                                                    # written by the build: no scratch, no spills
        lines = res.read_text().splitlines()
        rows = [line for line in lines if KERNEL in line]
        assert len(rows) == 2                                           # symmetric and asymmetric activations
        for row in rows:
            assert "scratch 0\t" in row and "vgpr_spill 0\t" in row and row.endswith("waves_per_simd 2")
        assert len([line for line in lines if "gemm_i8_ring_w4_kernel" in line]) == 2


# ---- refusals before the library ------------------------------------------------------------------------------------
CASES = ["int8 bank", "G = 1", "ragged K", "K past the accumulator bound", "misaligned Xq", "misaligned Wq",
         "the 2^32 bound", "E > 4096", "too many tiles"]


def _refused(case):
    """(Xq, Wq, s_w, row_idx, reason).  The oversized operands are expanded views: their shape is all that is read."""
    from quantool_amd.hip import ops

    U = ops.I8_RING_W4_K_UNIT
    i8 = lambda *s: torch.zeros(*s, dtype=torch.int8)    # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    idx = torch.zeros(4, dtype=torch.int32)
    if case == "int8 bank":
        return i8(4, 256), i8(2, 8, 256), torch.ones(2, 8, 2), idx, "int8 weights run on gemm_i8_ring_grouped"
    if case == "G = 1":
        return i8(4, 256), i32(2, 8, 32), torch.ones(2, 8, 1), idx, "scales run on gemm_i8_grouped"
    if case == "ragged K":
        K = 3 * U + 16
        return i8(4, K), i32(2, 8, K // 8), torch.ones(2, 8, 4), idx, "not a multiple"
    if case == "K past the accumulator bound":
        K = 32768 + U
        return i8(1, K), i32(2, 2, K // 8), torch.ones(2, 2, K // U), idx, "32768"
    if case == "misaligned Xq":
        return aligned_i8(4, 4 * U, shift=1), i32(2, 8, U // 2), torch.ones(2, 8, 4), idx, "16-byte aligned"
    if case == "misaligned Wq":
        Wq = aligned_i32(16, U // 2, shift=1).view(2, 8, U // 2)
        return aligned_i8(4, 4 * U), Wq, torch.ones(2, 8, 4), idx, "16-byte aligned"
    if case == "the 2^32 bound":
        K = 4096
        Xq = i8(1, K).expand(2 ** 32 // K + 1, K)
        return Xq, i32(2, 8, K // 8), torch.ones(2, 8, K // U), idx, r"2\^32"
    if case == "E > 4096":
        return i8(4, U), i32(1, 1, U // 8).expand(4097, 1, U // 8), torch.ones(4097, 1, 1), idx, "4096"
    if case == "too many tiles":
        R, N = 2 ** 31 - 1, 2 ** 20
        big_idx = torch.zeros(1, dtype=torch.int32).expand(R)
        return (i8(4, U), i32(1, 1, U // 8).expand(2, N, U // 8), torch.ones(1, 1, 1).expand(2, N, 1), big_idx,
                "too many tiles")
    raise KeyError(case)


@pytest.mark.parametrize("case", CASES)
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    from quantool_amd.hip import _lib, ops

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(ops, "load", boom)
    Xq, Wq, s_w, row_idx, reason = _refused(case)
    if case.startswith("misaligned"):
        assert (Xq if case.endswith("Xq") else Wq).data_ptr() % 16 != 0
    assert ops.moe_gemm_i8_ring_w4_supported(Xq, Wq, s_w, row_idx) is False
    with pytest.raises(ValueError, match=reason) as err:
        ops.moe_gemm_i8_ring_w4(Xq, torch.ones(Xq.shape[0]), Wq, s_w, torch.zeros(Wq.shape[0] + 1, dtype=torch.int32),
                                row_idx=row_idx, K=Xq.shape[1])
    assert str(err.value).startswith("moe_gemm_i8_ring_w4: ")


def test_the_dense_forms_hint_is_unchanged(monkeypatch):
    from quantool_amd.hip import ops

    why = ops._i8_refusal(ops.I8_FORMS["qt_gemm_i8_ring_w4"], torch.zeros(4, 256, dtype=torch.int8),
                          torch.zeros(8, 256, dtype=torch.int8), torch.ones(8, 2))
    assert why.endswith("(int8 weights run on gemm_i8_ring)")


def test_the_2_32_bound_is_about_gathered_rows_only(monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    K = 4096
    Wq, s_w = torch.zeros(2, 8, K // 8, dtype=torch.int32), torch.ones(2, 8, K // 128)
    idx = torch.zeros(4, dtype=torch.int32)
    at = torch.zeros(1, K, dtype=torch.int8).expand(2 ** 32 // K, K)
    past = torch.zeros(1, K, dtype=torch.int8).expand(2 ** 32 // K + 1, K)
    assert ops.moe_gemm_i8_ring_w4_supported(at, Wq, s_w, idx) is True
    assert ops.moe_gemm_i8_ring_w4_supported(past, Wq, s_w, idx) is False
    assert ops.moe_gemm_i8_ring_w4_supported(past, Wq, s_w, None) is True      # contiguous rows: tile-relative offsets


def test_supported_operands(monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    U = ops.I8_RING_W4_K_UNIT
    Wq, s_w = torch.zeros(2, 8, 4 * U // 8, dtype=torch.int32), torch.ones(2, 8, 4)
    aligned = aligned_i8(4, 4 * U)
    assert aligned.data_ptr() % 16 == 0 and Wq.data_ptr() % 16 == 0
    assert ops.moe_gemm_i8_ring_w4_supported(aligned, Wq, s_w) is True
    assert ops.moe_gemm_i8_ring_w4_supported(aligned, Wq, s_w, torch.zeros(9, dtype=torch.int32)) is True
    # one K-tile: the one group is the whole row, G = K / 128 = 1 is taken
    assert ops.moe_gemm_i8_ring_w4_supported(aligned.view(16, U), torch.zeros(2, 8, U // 8, dtype=torch.int32),
                                             torch.ones(2, 8, 1)) is True


# ---- dispatch -------------------------------------------------------------------------------------------------------
E, TOPK = 4, 2


def _experts(H=256, I=128, int4=True):
    from quantool_amd.engine.qmodules import QuantizedExperts

    if int4:
        gu, dn = torch.zeros(E, 2 * I, H // 8, dtype=torch.int32), torch.zeros(E, H, I // 8, dtype=torch.int32)
        s_gu, s_dn = torch.ones(E, 2 * I, (H + 127) // 128), torch.ones(E, H, (I + 127) // 128)
    else:
        gu, dn = torch.zeros(E, 2 * I, H, dtype=torch.int8), torch.zeros(E, H, I, dtype=torch.int8)
        s_gu, s_dn = torch.ones(E, 2 * I, 1), torch.ones(E, H, 1)
    return QuantizedExperts(H, I, gu, s_gu, dn, s_dn, nn.SiLU(), not int4)


def _forward(rec, qe, T):
    rec.calls.clear()
    out = qe(torch.zeros(T, qe.hidden_dim, dtype=torch.bfloat16), torch.zeros(T, TOPK, dtype=torch.int64),
             torch.ones(T, TOPK))
    assert out.shape == (T, qe.hidden_dim)
    return rec.calls


def _attrs(monkeypatch, ring_w4, ring=0):
    from quantool_amd.engine.qmodules import QuantizedExperts

    monkeypatch.setattr(QuantizedExperts, "grouped_max_tokens", 16)
    monkeypatch.setattr(QuantizedExperts, "ring_min_rows_per_expert", ring)
    monkeypatch.setattr(QuantizedExperts, "ring_w4_min_rows_per_expert", ring_w4)


def test_the_default_is_off_or_at_least_1024_rows_per_expert():
    from quantool_amd.engine.qmodules import QuantizedExperts

    d = QuantizedExperts.ring_w4_min_rows_per_expert
    assert type(d) is int and (d == 0 or d >= 1024)
    assert "ring_w4_min_rows_per_expert" in QuantizedExperts.__doc__


def test_int4_bank_takes_the_ring_from_the_attribute_on(w4_ops, monkeypatch):
    _attrs(monkeypatch, 32)
    qe = _experts()
    # R = T * TOPK routed rows over E = 4 experts: R / E = 32 at T = 64
    assert _forward(w4_ops, qe, 63) == [("gemm_i8_grouped", 126)] * 2
    assert w4_ops.asked == []                         # below the bound the new names are not touched
    assert _forward(w4_ops, qe, 64) == [(GEMM, 128)] * 2
    # R is taken from row_idx for the gathered product and from x for the contiguous one
    assert w4_ops.asked == [128, None]
    assert _forward(w4_ops, qe, 500) == [(GEMM, 1000)] * 2
    assert w4_ops.queries["gemm_i8_ring_grouped_supported"] == []      # an int4 bank never asks the int8 ring's name


def test_skinny_range_keeps_precedence(w4_ops, monkeypatch):
    _attrs(monkeypatch, 1)
    qe = _experts()
    for T in (1, 16):
        assert _forward(w4_ops, qe, T) == [("gemm_i8_skinny_grouped", T * TOPK)] * 2
    assert w4_ops.asked == []
    assert _forward(w4_ops, qe, 17) == [(GEMM, 34)] * 2


def test_attribute_zero_never_uses_the_ring(w4_ops, monkeypatch):
    _attrs(monkeypatch, 0, ring=1)
    qe = _experts()
    for T in (17, 64, 4096):
        assert _forward(w4_ops, qe, T) == [("gemm_i8_grouped", T * TOPK)] * 2
    assert w4_ops.asked == [] and w4_ops.queries["gemm_i8_ring_grouped_supported"] == []


def test_unsupported_operands_fall_to_the_tiled_gemm(w4_ops, monkeypatch):
    _attrs(monkeypatch, 1)
    w4_ops.answers[WATCH] = False
    assert _forward(w4_ops, _experts(), 64) == [("gemm_i8_grouped", 128)] * 2
    assert len(w4_ops.asked) == 2


def test_int8_bank_never_asks_the_new_name(w4_ops, monkeypatch):
    _attrs(monkeypatch, 1, ring=1)
    assert _forward(w4_ops, _experts(int4=False), 64) == [("gemm_i8_ring_grouped", 128)] * 2
    assert w4_ops.asked == []
    _attrs(monkeypatch, 1, ring=0)
    assert _forward(w4_ops, _experts(int4=False), 64) == [("gemm_i8_grouped", 128)] * 2
    assert w4_ops.asked == []


def test_below_the_bound_no_new_name_is_read(fake_ops, monkeypatch):
    """``fake_ops`` is the shared Recorder, which has neither of the two new names: reading one raises."""
    _attrs(monkeypatch, 1024, ring=1)
    assert not hasattr(fake_ops, GEMM) and not hasattr(fake_ops, WATCH)
    assert _forward(fake_ops, _experts(), 2047) == [("gemm_i8_grouped", 4094)] * 2       # R / E = 1023.5
    with pytest.raises(AttributeError):
        _forward(fake_ops, _experts(), 2048)
    _attrs(monkeypatch, 0, ring=1)
    assert _forward(fake_ops, _experts(), 4096) == [("gemm_i8_grouped", 8192)] * 2


def test_a_ragged_k_falls_to_the_tiled_gemm(monkeypatch):
    """H = 192 with the real host-side check: the gate_up product (K = H = 192: two groups, the second ragged) stays on
    the tiled kernel, the down product (K = I = 128: one K-tile) is taken."""
    import quantool_amd.hip as hip
    from quantool_amd.hip import ops as real

    rec = W4Recorder()
    setattr(rec, WATCH, real.moe_gemm_i8_ring_w4_supported)
    monkeypatch.setattr(real, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    monkeypatch.setattr(hip, "ops", rec)
    _attrs(monkeypatch, 1)
    qe = _experts(H=192, I=128)
    assert _forward(rec, qe, 64) == [("gemm_i8_grouped", 128), (GEMM, 128)]
