"""The table of int8 GEMM forms (``ops.I8_FORMS``) without a GPU: every row's entry point is declared in the header and
held by the ctypes table with the dense or the grouped signature, its constants are the header's, and every refusal the
five dispatch test files list comes out of ``ops._i8_refusal`` with that row, before the library is touched.  A new
form's row is checked here."""
import re
from ctypes import c_int, c_int64

import pytest
import torch

from tests import test_i8_mid_dispatch as mid
from tests import test_i8_ring_dispatch as ring
from tests import test_i8_ring_grouped_dispatch as ring_grouped
from tests import test_i8_ring_w4_dispatch as ring_w4
from tests.i8_fake_ops import aligned_i8, aligned_i32, check_surface, header_constants

ENTRIES = ["qt_gemm_i8", "qt_gemm_i8_skinny", "qt_gemm_i8_mid", "qt_gemm_i8_ring", "qt_gemm_i8_ring_w4",
           "qt_gemm_i8_grouped", "qt_gemm_i8_skinny_grouped", "qt_gemm_i8_ring_grouped"]


def test_the_table_has_one_row_per_entry_point():
    from quantool_amd.hip import _lib, ops

    assert list(ops.I8_FORMS) == ENTRIES
    assert sorted(ENTRIES) == sorted(n for n in _lib.SIGNATURES if n.startswith("qt_gemm_i8"))
    for entry, form in ops.I8_FORMS.items():
        assert form.entry == entry and callable(getattr(ops, entry[3:]))
        assert form.experts == entry.endswith("_grouped")
        assert (form.k_unit is not None) == form.aligned16 == hasattr(ops, entry[3:] + "_supported")


@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_point_is_declared_with_the_dense_or_the_grouped_signature(entry):
    from quantool_amd.hip import _lib, ops

    form = ops.I8_FORMS[entry]
    check_surface("header", entry)
    res, args = _lib.SIGNATURES[entry]
    like_res, like = _lib.SIGNATURES["qt_gemm_i8_grouped" if form.experts else "qt_gemm_i8"]
    assert res is like_res
    if form.x_rows:                                   # x_rows, in front of the stream
        like = like[:-1] + [c_int64] + like[-1:]
    if entry == "qt_gemm_i8_skinny":                  # M is an int
        assert like[1] is c_int64
        like = like[:1] + [c_int] + like[2:]
    assert args == like


# where the header #defines an entry point's limits; the grouped ring runs the dense ring's instance
HEADER_PREFIX = {"qt_gemm_i8_mid": "QT_I8_MID_", "qt_gemm_i8_ring": "QT_I8_RING_", "qt_gemm_i8_ring_w4": "QT_I8_RING_W4_",
                 "qt_gemm_i8_ring_grouped": "QT_I8_RING_"}


@pytest.mark.parametrize("entry", ENTRIES)
def test_constants_are_the_headers(entry):
    from quantool_amd.hip import ops

    form = ops.I8_FORMS[entry]
    fields = {"MAX_M": form.max_m, "K_UNIT": form.k_unit, "SLOTS": form.slots, "LEAD": form.lead}
    if entry not in HEADER_PREFIX:                    # no #define: the skinny forms' 16 rows are the header's prose
        assert fields == {"MAX_M": 16 if entry == "qt_gemm_i8_skinny" else None, "K_UNIT": None, "SLOTS": None,
                          "LEAD": None}
        return
    prefix = HEADER_PREFIX[entry]
    defines = header_constants(prefix)
    assert defines and {k[len(prefix):]: v for k, v in defines.items()} == \
        {k: v for k, v in fields.items() if v is not None}
    for k, v in defines.items():                      # the public constants are the table's
        assert getattr(ops, k[len("QT_"):]) == v


def test_public_constants_without_a_define_are_the_tables():
    from quantool_amd.hip import ops

    assert ops.I8_SKINNY_MAX_M == ops.I8_FORMS["qt_gemm_i8_skinny"].max_m == 16
    assert ops.I8_RING_GROUPED_MAX_E == ops.I8_FORMS["qt_gemm_i8_ring_grouped"].max_e == 4096


def _skinny(M):
    return lambda: (torch.zeros(M, 128, dtype=torch.int8), torch.zeros(8, 128, dtype=torch.int8), torch.ones(8, 1),
                    None, "1 <= M <= 16")


def _misaligned(experts, int4, which):
    """One operand of an otherwise supported set one element off a 16-byte boundary."""
    def make():
        K = 512
        Xq = aligned_i8(4, K, shift=int(which == "Xq"))
        Wq = (aligned_i32(8, K // 8, shift=int(which == "Wq")) if int4 else aligned_i8(8, K, shift=int(which == "Wq")))
        s_w = torch.ones(8, K // 128 if int4 else 1)
        assert (Xq if which == "Xq" else Wq).data_ptr() % 16 != 0
        return (Xq, Wq[None], s_w[None], None, "16-byte aligned") if experts else (Xq, Wq, s_w, None, "16-byte aligned")

    return make


def _listed(table, case):
    return lambda: (*table()[case][:3], None, table()[case][3])


# every case the dispatch test files list, by entry point: name -> () -> (Xq, Wq, s_w, row_idx, reason)
REFUSED = {
    "qt_gemm_i8_skinny": {f"M = {M}": _skinny(M) for M in (0, 17)},
    "qt_gemm_i8_mid": {case: (lambda case=case: (*mid.REFUSED[case][0](), None, mid.REFUSED[case][1]))
                       for case in mid.REFUSED},
    "qt_gemm_i8_ring": {**{case: _listed(ring._refused_cases, case) for case in
                           ("packed int4", "G = K/128 > 1", "ragged K", "K past the accumulator bound")},
                        **{f"misaligned {w}": _misaligned(False, False, w) for w in ("Xq", "Wq")}},
    "qt_gemm_i8_ring_w4": {**{case: _listed(ring_w4._refused_cases, case) for case in
                              ("int8 weight", "G = 1", "ragged K", "K past the accumulator bound")},
                           **{f"misaligned {w}": _misaligned(False, True, w) for w in ("Xq", "Wq")}},
    "qt_gemm_i8_ring_grouped": {**{case: (lambda case=case: ring_grouped._refused(case))
                                   for case in ring_grouped.CASES},
                                **{f"misaligned {w}": _misaligned(True, False, w) for w in ("Xq", "Wq")}},
}


@pytest.mark.parametrize("entry,case", [(e, c) for e in ENTRIES for c in REFUSED.get(e, {})])
def test_refusal_comes_from_the_forms_row_before_the_library(monkeypatch, entry, case):
    from quantool_amd.hip import _lib, ops

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(ops, "load", boom)
    Xq, Wq, s_w, row_idx, reason = REFUSED[entry][case]()
    why = ops._i8_refusal(ops.I8_FORMS[entry], Xq, Wq, s_w, row_idx)
    assert why is not None and re.search(reason, why), why
    supported = getattr(ops, entry[3:] + "_supported", None)
    if supported is not None:
        assert supported(Xq, Wq, s_w, *((row_idx,) if ops.I8_FORMS[entry].experts else ())) is False
    s_x = torch.ones(Xq.shape[0])
    with pytest.raises(ValueError, match=reason):
        if ops.I8_FORMS[entry].experts:
            getattr(ops, entry[3:])(Xq, s_x, Wq, s_w, torch.zeros(Wq.shape[0] + 1, dtype=torch.int32),
                                    row_idx=row_idx, K=Xq.shape[1])
        else:
            getattr(ops, entry[3:])(Xq, s_x, Wq, s_w, K=Xq.shape[1])


@pytest.mark.parametrize("entry", ["qt_gemm_i8", "qt_gemm_i8_grouped", "qt_gemm_i8_skinny_grouped"])
def test_forms_without_limits_refuse_nothing_here(entry):
    """Their operands are checked by ``_i8_operands`` behind ``load()``, in its own words."""
    from quantool_amd.hip import ops

    for make in (*REFUSED["qt_gemm_i8_ring"].values(), *REFUSED["qt_gemm_i8_mid"].values()):
        Xq, Wq, s_w, row_idx, _ = make()
        assert ops._i8_refusal(ops.I8_FORMS[entry], Xq, Wq, s_w, row_idx) is None
