"""The A8 bank's form between the decode range and the rings without a GPU: the header, the ctypes table and the
built library carry ``qt_moe_gemm_i8_wide`` with ``qt_moe_gemm_i8_ring_w4``'s signature, ``ops.moe_gemm_i8_wide_supported``
/ ``ops.moe_gemm_i8_wide`` refuse what the kernel does not take before they touch the library, and ``QuantizedExperts``
picks the form by ``wide_max_rows_per_expert`` / ``wide_w4_max_rows_per_expert`` / ``wide_min_k`` / ``wide_max_n`` (with
``quantool_amd.hip.ops`` replaced by a recording fake that also carries the two new names, so nothing reaches a
device)."""
import re

import pytest
import torch
import torch.nn as nn

from tests.i8_fake_ops import Recorder, aligned_i8, aligned_i32, check_surface, fake_ops, header_constants  # noqa: F401
from tests.i8_fake_ops import header_text

NAME = "qt_moe_gemm_i8_wide"
GEMM = "moe_gemm_i8_wide"
WATCH = "moe_gemm_i8_wide_supported"
LIKE = "qt_moe_gemm_i8_ring_w4"
KERNEL = "moe_gemm_i8_wide_kernel"
STEM = "qlinear_moe_wide"


class WideRecorder(Recorder):
    """``Recorder`` with the form's two names: the GEMM records as the grouped ones do, ``asked`` lists the rows of
    row_idx (or None) of every ``moe_gemm_i8_wide_supported`` call.  The W4A8 ring's two names are carried as well."""

    def __init__(self):
        super().__init__(WATCH)
        for watch, gemm in ((WATCH, GEMM), ("moe_gemm_i8_ring_w4_supported", "moe_gemm_i8_ring_w4")):
            self.answers[watch] = True
            self.queries[watch] = []
            setattr(self, watch, self._supported(watch))
            setattr(self, gemm, self._grouped(gemm))

    @property
    def asked(self):
        return self.queries[WATCH]


@pytest.fixture
def wide_ops(monkeypatch):
    import quantool_amd.hip as hip
    from quantool_amd.hip import ops as real   # noqa: F401  (the attribute the modules import must exist first)

    rec = WideRecorder()
    monkeypatch.setattr(hip, "ops", rec)
    return rec


# ---- surface --------------------------------------------------------------------------------------------------------
def _declared_args(name, text):
    return [a.strip() for a in re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1).split(",")]


def test_header_declares_the_entry_point_with_the_w4_rings_arguments():
    check_surface("header", NAME)
    text = header_text()[1]
    args = _declared_args(NAME, text)
    assert args == _declared_args(LIKE, text)
    assert args[-2:] == ["int64_t x_rows", "qt_stream_t stream"] and not [a for a in args if "bias" in a]


def test_header_states_the_contract():
    raw = re.sub(r"\s*\n\s*\*\s*", " ", header_text()[0])
    para = raw[raw.index(NAME + ":"):raw.index("qt_moe_combine:")]
    for must in ("bit-identical to qt_gemm_i8_grouped", "rows >= offsets[E] are not written", "clamped into [0, x_rows)",
                 "65535", "No workspace, no atomics: deterministic", "QT_ERR_INVALID before any launch"):
        assert must in para, must


def test_ctypes_table_holds_it_with_the_w4_rings_signature():
    from quantool_amd.hip import _lib

    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES[LIKE]


def test_library_exports_it():
    check_surface("library", NAME)


def test_no_workspace_function_was_added():
    from quantool_amd.hip import _lib

    assert NAME in _lib.SIGNATURES and NAME + "_workspace_bytes" not in _lib.SIGNATURES
    assert len([n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")]) == 14


def test_constants_are_the_headers_and_the_forms():
    from quantool_amd.hip import ops

    form = ops.I8_MOE_WIDE_FORM
    assert header_constants("QT_MOE_I8_WIDE_") == {"QT_MOE_I8_WIDE_K_UNIT": 128, "QT_MOE_I8_WIDE_TILE_ROWS": 128,
                                                   "QT_MOE_I8_WIDE_MAX_E": 4096}
    assert (ops.MOE_I8_WIDE_K_UNIT, ops.MOE_I8_WIDE_TILE_ROWS, ops.MOE_I8_WIDE_MAX_E) == (128, 128, 4096)
    assert (form.k_unit, form.tile_rows, form.max_e) == (128, 128, 4096)
    assert ops.MOE_I8_WIDE_MAX_SLOTS == 65535


def test_the_form_stands_beside_the_table():
    from quantool_amd.hip import ops

    form = ops.I8_MOE_WIDE_FORM
    assert form.entry == NAME and NAME not in ops.I8_FORMS and len(ops.I8_FORMS) == 8
    assert form.experts and form.x_rows and form.aligned16 and form.groups == "one_or_per_unit"
    assert form.dtypes == (torch.int8, torch.int32) and form.max_m is None
    assert all(f.tile_rows is None for f in ops.I8_FORMS.values()) and ops.I8_MOE_RING_W4_FORM.tile_rows is None
    assert callable(getattr(ops, GEMM)) and callable(getattr(ops, WATCH))


def _resource_rows(stem, kernel):
    from quantool_amd.csrc import build

    res = build.OBJ_DIR / f"{stem}.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    return [line for line in res.read_text().splitlines() if kernel in line]


def test_the_new_files_instances_keep_their_registers():
    from quantool_amd.csrc import build

    assert build.CSRC / f"{STEM}.hip" in build.sources() and (build.CSRC / "i8_mid_tile.h").exists()
    assert KERNEL in build.NO_SPILL_KERNELS
    rows = _resource_rows(STEM, KERNEL)
    assert len(rows) == 12                                  # MT 2 / 4 / 8 x int8 / int4 x one group / K/128 groups
    for row in rows:
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row
        assert int(re.search(r"lds (\d+)", row).group(1)) <= 65536, row


def test_the_dense_file_keeps_its_twelve_instances():
    from quantool_amd.csrc import build

    src = (build.CSRC / "qlinear_mid.hip").read_text()
    assert '#include "i8_mid_tile.h"' in src and NAME not in src      # the tile is stated once, in the header
    rows = _resource_rows("qlinear_mid", "gemm_i8_mid_kernel")
    assert len(rows) == 12
    for row in rows:
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row
        assert int(re.search(r"lds (\d+)", row).group(1)) <= 65536, row


# ---- refusals before the library ------------------------------------------------------------------------------------
CASES = ["ragged K", "K past the accumulator bound", "G = 2 at K = 512", "misaligned Xq", "misaligned Wq", "E = 4097",
         "too many slots", "the 2^32 bound", "float weights"]


def _refused(case):
    """(Xq, Wq, s_w, row_idx, reason).  The oversized operands are expanded views: their shape is all that is read."""
    i8 = lambda *s: torch.zeros(*s, dtype=torch.int8)    # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)  # noqa: E731
    idx = torch.zeros(4, dtype=torch.int32)
    if case == "ragged K":
        return i8(4, 400), i32(2, 8, 50), torch.ones(2, 8, 1), idx, "not a multiple"
    if case == "K past the accumulator bound":
        K = 32768 + 128
        return i8(1, K), i8(2, 2, K), torch.ones(2, 2, 1), idx, "32768"
    if case == "G = 2 at K = 512":
        return i8(4, 512), i8(2, 8, 512), torch.ones(2, 8, 2), idx, "G must be 1 or"
    if case == "misaligned Xq":
        return aligned_i8(4, 512, shift=1), i32(2, 8, 64), torch.ones(2, 8, 4), idx, "16-byte aligned"
    if case == "misaligned Wq":
        return aligned_i8(4, 512), aligned_i32(16, 64, shift=1).view(2, 8, 64), torch.ones(2, 8, 4), idx, "16-byte aligned"
    if case == "E = 4097":
        return i8(4, 128), i8(1, 1, 128).expand(4097, 1, 128), torch.ones(4097, 1, 1), idx, "4096"
    if case == "too many slots":
        R = 128 * (65535 - 1) + 1                        # R // 128 + min(E, R) = 65534 + 2
        big_idx = torch.zeros(1, dtype=torch.int32).expand(R)
        return i8(4, 128), i8(2, 8, 128), torch.ones(2, 8, 1), big_idx, "row-tile slots"
    if case == "the 2^32 bound":
        K = 4096
        return i8(1, K).expand(2 ** 32 // K + 1, K), i32(2, 8, K // 8), torch.ones(2, 8, K // 128), idx, r"2\^32"
    if case == "float weights":
        return i8(4, 512), torch.zeros(2, 8, 512), torch.ones(2, 8, 1), idx, "weights only"
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
    why = ops._i8_refusal(ops.I8_MOE_WIDE_FORM, Xq, Wq, s_w, row_idx)
    assert why is not None and re.search(reason, why), why
    assert ops.moe_gemm_i8_wide_supported(Xq, Wq, s_w, row_idx) is False
    with pytest.raises(ValueError, match=reason) as err:
        ops.moe_gemm_i8_wide(Xq, torch.ones(Xq.shape[0]), Wq, s_w, torch.zeros(Wq.shape[0] + 1, dtype=torch.int32),
                             row_idx=row_idx, K=Xq.shape[1])
    assert str(err.value).startswith("moe_gemm_i8_wide: ")


def test_the_bounds_are_met_exactly(monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    i8 = lambda *s: torch.zeros(*s, dtype=torch.int8)    # noqa: E731
    W, s_w = i8(2, 8, 128), torch.ones(2, 8, 1)
    rows = lambda R: torch.zeros(1, dtype=torch.int32).expand(R)   # noqa: E731
    at = 128 * (65535 - 2) + 127                         # 65533 + 2 slots
    assert ops.moe_gemm_i8_wide_supported(i8(4, 128), W, s_w, rows(at)) is True
    assert ops.moe_gemm_i8_wide_supported(i8(4, 128), W, s_w, rows(at + 1)) is False
    # the rings' count of 256-row tiles is not this form's bound
    N = 2 ** 20
    assert ops.moe_gemm_i8_wide_supported(i8(4, 128), i8(1, 1, 128).expand(2, N, 128),
                                          torch.ones(1, 1, 1).expand(2, N, 1), rows(at)) is True
    K = 4096
    Wq, s4 = torch.zeros(2, 8, K // 8, dtype=torch.int32), torch.ones(2, 8, K // 128)
    idx = torch.zeros(4, dtype=torch.int32)
    at_x, past = i8(1, K).expand(2 ** 32 // K, K), i8(1, K).expand(2 ** 32 // K + 1, K)
    assert ops.moe_gemm_i8_wide_supported(at_x[:64], Wq, s4, idx) is True
    assert ops.moe_gemm_i8_wide_supported(at_x, Wq, s4, idx) is True
    assert ops.moe_gemm_i8_wide_supported(past, Wq, s4, idx) is False
    assert ops.moe_gemm_i8_wide_supported(i8(1, 128).expand(4, 128), i8(1, 1, 128).expand(4096, 1, 128),
                                          torch.ones(4096, 1, 1)) is True


def test_supported_operands(monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    Xq = aligned_i8(40, 512)
    idx = torch.zeros(9, dtype=torch.int32)
    for Wq, s_w in ((torch.zeros(2, 8, 512, dtype=torch.int8), torch.ones(2, 8, 1)),
                    (torch.zeros(2, 8, 512, dtype=torch.int8), torch.ones(2, 8, 4)),
                    (torch.zeros(2, 8, 64, dtype=torch.int32), torch.ones(2, 8, 1)),
                    (torch.zeros(2, 8, 64, dtype=torch.int32), torch.ones(2, 8, 4))):
        assert ops.moe_gemm_i8_wide_supported(Xq, Wq, s_w) is True
        assert ops.moe_gemm_i8_wide_supported(Xq, Wq, s_w, idx) is True


# ---- dispatch -------------------------------------------------------------------------------------------------------
E, TOPK = 4, 2


def _experts(H=512, I=512, int4=True):
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


def _attrs(monkeypatch, wide=0, wide_w4=0, ring=0, ring_w4=0, min_k=512, max_n=0):
    from quantool_amd.engine.qmodules import QuantizedExperts

    for name, value in (("grouped_max_tokens", 16), ("ring_min_rows_per_expert", ring),
                        ("ring_w4_min_rows_per_expert", ring_w4), ("wide_max_rows_per_expert", wide),
                        ("wide_w4_max_rows_per_expert", wide_w4), ("wide_min_k", min_k), ("wide_max_n", max_n)):
        monkeypatch.setattr(QuantizedExperts, name, value)


def test_class_defaults_are_sane():
    from quantool_amd.engine.qmodules import QuantizedExperts as QE

    for name in ("wide_max_rows_per_expert", "wide_w4_max_rows_per_expert", "wide_min_k", "wide_max_n"):
        assert type(getattr(QE, name)) is int and getattr(QE, name) >= 0
        assert name in QE.__doc__
    assert QE.wide_min_k >= 512                  # the existing dispatch tests' K <= 256 banks stay on the tiled kernel
    # the rings keep what they were measured to win
    for wide, ring in ((QE.wide_max_rows_per_expert, QE.ring_min_rows_per_expert),
                       (QE.wide_w4_max_rows_per_expert, QE.ring_w4_min_rows_per_expert)):
        assert wide == 0 or ring == 0 or wide < ring


def test_skinny_range_keeps_precedence(wide_ops, monkeypatch):
    _attrs(monkeypatch, wide=10 ** 6, wide_w4=10 ** 6)
    for int4 in (True, False):
        qe = _experts(int4=int4)
        for T in (1, 16):
            assert _forward(wide_ops, qe, T) == [("gemm_i8_skinny_grouped", T * TOPK)] * 2
        assert wide_ops.asked == []
        assert _forward(wide_ops, qe, 17) == [(GEMM, 34)] * 2
        wide_ops.asked.clear()


def test_both_rings_keep_precedence(wide_ops, monkeypatch):
    _attrs(monkeypatch, wide=10 ** 6, wide_w4=10 ** 6, ring=32, ring_w4=32)
    assert _forward(wide_ops, _experts(int4=False), 64) == [("gemm_i8_ring_grouped", 128)] * 2
    assert _forward(wide_ops, _experts(int4=True), 64) == [("moe_gemm_i8_ring_w4", 128)] * 2
    assert wide_ops.asked == []
    assert _forward(wide_ops, _experts(int4=False), 63) == [(GEMM, 126)] * 2
    assert _forward(wide_ops, _experts(int4=True), 63) == [(GEMM, 126)] * 2
    # R is taken from row_idx for the gathered product and from x for the contiguous one
    assert wide_ops.asked == [126, None, 126, None]


@pytest.mark.parametrize("int4", [True, False])
def test_both_edges_of_the_formats_attribute(wide_ops, monkeypatch, int4):
    """R = T * TOPK routed rows over E = 4 experts: R = 32 E at T = 64; R = 32 E + 2 at T = 65 is the next R a
    forward can make, R = 32 E + 1 goes through ``_product`` itself."""
    mine, other = ("wide_w4", "wide") if int4 else ("wide", "wide_w4")
    _attrs(monkeypatch, **{mine: 32, other: 0})
    qe = _experts(int4=int4)
    assert _forward(wide_ops, qe, 64) == [(GEMM, 128)] * 2
    assert wide_ops.asked == [128, None]
    assert _forward(wide_ops, qe, 65) == [("gemm_i8_grouped", 130)] * 2
    assert wide_ops.asked == [128, None]
    for R, want in ((32 * E, GEMM), (32 * E + 1, "gemm_i8_grouped")):
        wide_ops.calls.clear()
        qe._product("down", torch.zeros(R, qe.intermediate_dim, dtype=torch.bfloat16),
                    torch.zeros(E + 1, dtype=torch.int32), None, 100)
        qe._product("gate_up", torch.zeros(7, qe.hidden_dim, dtype=torch.bfloat16),
                    torch.zeros(E + 1, dtype=torch.int32), torch.zeros(R, dtype=torch.int32), 100)
        assert wide_ops.calls == [(want, R)] * 2
    # the other format's attribute is never read as this one's
    _attrs(monkeypatch, **{mine: 0, other: 10 ** 6})
    wide_ops.asked.clear()
    for T in (17, 64, 4096):
        assert _forward(wide_ops, qe, T) == [("gemm_i8_grouped", T * TOPK)] * 2
    assert wide_ops.asked == []


def test_attribute_zero_never_asks(wide_ops, monkeypatch):
    _attrs(monkeypatch)
    for int4 in (True, False):
        for T in (17, 64, 4096):
            assert _forward(wide_ops, _experts(int4=int4), T) == [("gemm_i8_grouped", T * TOPK)] * 2
    assert wide_ops.asked == []


def test_a_small_k_never_reads_the_new_names(fake_ops, monkeypatch):
    """``fake_ops`` is the shared Recorder, which has neither of the two new names: reading one raises."""
    _attrs(monkeypatch, wide=10 ** 6, wide_w4=10 ** 6)
    assert not hasattr(fake_ops, GEMM) and not hasattr(fake_ops, WATCH)
    for int4 in (True, False):
        small = _experts(H=256, I=128, int4=int4)
        for T in (17, 64, 4096):
            assert _forward(fake_ops, small, T) == [("gemm_i8_grouped", T * TOPK)] * 2
        with pytest.raises(AttributeError):
            _forward(fake_ops, _experts(H=512, I=512, int4=int4), 17)
    _attrs(monkeypatch)
    assert _forward(fake_ops, _experts(H=512, I=512), 17) == [("gemm_i8_grouped", 34)] * 2


def test_wide_min_k_is_per_product(wide_ops, monkeypatch):
    _attrs(monkeypatch, wide_w4=10 ** 6)
    assert _forward(wide_ops, _experts(H=512, I=384), 40) == [(GEMM, 80), ("gemm_i8_grouped", 80)]
    assert wide_ops.asked == [80]
    _attrs(monkeypatch, wide_w4=10 ** 6, min_k=384)
    assert _forward(wide_ops, _experts(H=512, I=384), 40) == [(GEMM, 80)] * 2


def test_wide_max_n_keeps_gate_up_on_the_tiled_form(wide_ops, monkeypatch):
    qe = _experts(H=512, I=640)                           # gate_up: N = 1280, down: N = 512
    _attrs(monkeypatch, wide_w4=10 ** 6, max_n=512)
    assert _forward(wide_ops, qe, 40) == [("gemm_i8_grouped", 80), (GEMM, 80)]
    assert wide_ops.asked == [None]
    _attrs(monkeypatch, wide_w4=10 ** 6, max_n=511)
    assert _forward(wide_ops, qe, 40) == [("gemm_i8_grouped", 80)] * 2
    _attrs(monkeypatch, wide_w4=10 ** 6, max_n=1280)
    assert _forward(wide_ops, qe, 40) == [(GEMM, 80)] * 2


def test_unsupported_operands_fall_to_the_tiled_gemm(wide_ops, monkeypatch):
    _attrs(monkeypatch, wide=10 ** 6, wide_w4=10 ** 6)
    wide_ops.answers[WATCH] = False
    for int4 in (True, False):
        assert _forward(wide_ops, _experts(int4=int4), 64) == [("gemm_i8_grouped", 128)] * 2
    assert len(wide_ops.asked) == 4


def test_a_ragged_k_falls_to_the_tiled_gemm(monkeypatch):
    """I = 576 with the real host-side check: the down product (K = 576, no multiple of 128) stays on the tiled kernel,
    the gate_up product (K = 512) is taken."""
    import quantool_amd.hip as hip
    from quantool_amd.hip import ops as real

    rec = WideRecorder()
    setattr(rec, WATCH, real.moe_gemm_i8_wide_supported)
    monkeypatch.setattr(real, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    monkeypatch.setattr(hip, "ops", rec)
    _attrs(monkeypatch, wide_w4=10 ** 6)
    assert _forward(rec, _experts(H=512, I=576), 64) == [(GEMM, 128), ("gemm_i8_grouped", 128)]
