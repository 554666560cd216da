"""The split-K int8 GEMM's surface without a GPU: the header, the ctypes table and the built library carry
``qt_splitk_gemm_i8`` with its plan and range functions, the plan deals every K-tile to exactly one split,
``ops.splitk_gemm_i8_supported`` / ``ops.splitk_gemm_i8`` refuse what the kernel does not take before they touch the
library, and ``QuantizedLinear`` picks the form by ``splitk_min_m`` / ``splitk_min_k`` below ``ring_min_m`` (with
``quantool_amd.hip.ops`` replaced by a recording fake of this file's own, so nothing reaches a device)."""
import ctypes
import re

import pytest
import torch

from tests import i8_fake_ops
from tests.i8_fake_ops import aligned_i8, check_surface, header_constants, header_text

NAME = "qt_splitk_gemm_i8"
# the dispatch rules under test, whatever the measured class defaults are
LINEAR_ATTRS = {"skinny_max_m": 16, "ring_min_m": 2048, "ring_w4_min_m": 8192, "mid_max_m": 128, "mid_max_n": 6144,
                "mid_min_k": 512, "splitk_min_m": 256, "splitk_min_k": 1024}
GEMM_I8_NAMES = ["qt_gemm_i8", "qt_gemm_i8_grouped", "qt_gemm_i8_mid", "qt_gemm_i8_ring", "qt_gemm_i8_ring_grouped",
                 "qt_gemm_i8_ring_w4", "qt_gemm_i8_skinny", "qt_gemm_i8_skinny_grouped"]


# ---- surface --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_constants():
    from quantool_amd.hip import ops

    for name in (NAME, NAME + "_plan", NAME + "_range"):
        check_surface("header", name)
    assert header_constants("QT_SPLITK_I8_") == {"QT_SPLITK_I8_K_UNIT": ops.SPLITK_I8_K_UNIT,
                                                 "QT_SPLITK_I8_MAX_SPLITS": ops.SPLITK_I8_MAX_SPLITS,
                                                 "QT_SPLITK_I8_MIN_K_TILES": ops.SPLITK_I8_MIN_K_TILES}
    assert ops.SPLITK_I8_K_UNIT == ops.I8_RING_K_UNIT == 128            # the ring's K-tile
    assert ops.SPLITK_I8_MAX_SPLITS >= 17                               # one split per K-tile of a 17-tile reduction
    assert f"{NAME}:" in header_text()[0] and "(DESIGN.md 4.24)" in header_text()[0]


def test_ctypes_table_holds_it_with_the_tiled_arguments_and_three_more():
    from quantool_amd.hip import _lib

    res, args = _lib.SIGNATURES[NAME]
    tiled_res, tiled = _lib.SIGNATURES["qt_gemm_i8"]
    # qt_gemm_i8's arguments, then splits, workspace, workspace_size in front of the stream
    assert res is tiled_res
    assert args == tiled[:-1] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t] + tiled[-1:]
    assert _lib.SIGNATURES[NAME + "_plan"] == (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p])


def test_library_exports_them():
    for name in (NAME, NAME + "_plan", NAME + "_range"):
        check_surface("library", name)


def test_existing_names_are_unchanged():
    from quantool_amd.hip import _lib, ops

    assert len([n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")]) == 14
    assert not [n for n in _lib.SIGNATURES if "splitk" in n and n.endswith("_workspace_bytes")]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("qt_gemm_i8")) == GEMM_I8_NAMES
    assert sorted(ops.I8_FORMS) == GEMM_I8_NAMES and NAME not in ops.I8_FORMS
    assert ops.I8_SPLITK_FORM.entry == NAME
    ring = ops.I8_FORMS["qt_gemm_i8_ring"]                              # it takes what the dense ring takes
    assert (ops.I8_SPLITK_FORM.dtypes, ops.I8_SPLITK_FORM.k_unit, ops.I8_SPLITK_FORM.groups,
            ops.I8_SPLITK_FORM.aligned16) == (ring.dtypes, ring.k_unit, ring.groups, ring.aligned16)


def test_build_audits_cover_the_new_kernels():
    import inspect

    from quantool_amd.csrc import build

    for kernel in ("gemm_i8_splitk_partial_kernel", "gemm_i8_splitk_reduce_kernel"):
        assert kernel in build.NO_SPILL_KERNELS
    assert '"qlinear_ring.hip"' in inspect.getsource(build.build)       # audit_m0's list: the file the kernels live in
    assert build.SCRATCH_OK == ()
    res = build.OBJ_DIR / "qlinear_ring.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    for kernel, lds in (("gemm_i8_splitk_partial_kernel", 131072), ("gemm_i8_splitk_reduce_kernel", 0)):
        rows = [line for line in res.read_text().splitlines() if kernel in line]
        assert len(rows) == 1 and "scratch 0\t" in rows[0] and "vgpr_spill 0\t" in rows[0], rows
        assert f"lds {lds}\t" in rows[0], rows
    # the existing ring kernels keep the tile's budget
    ring = [line for line in res.read_text().splitlines() if "gemm_i8_ring_kernel" in line]
    part = [line for line in res.read_text().splitlines() if "gemm_i8_splitk_partial_kernel" in line]
    assert ring[0].split("\t")[1:] == part[0].split("\t")[1:]


# ---- the plan -------------------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


PLAN_GRID = [(M, N, K, cus) for M in (1, 129, 256, 257, 512, 1100, 2047) for N in (1, 264, 4096, 28672)
             for K in (128, 256, 896, 4096, 14336, 32768) for cus in (1, 64, 256, 304)]


def test_the_rule_is_clamp_cus_over_tiles_with_no_split_below_four_k_tiles():
    from quantool_amd.hip import ops

    for M, N, K, cus in PLAN_GRID:
        S, size = ops.splitk_gemm_i8_plan(M, N, K, cus=cus)
        tiles = _ceil(M, 256) * _ceil(N, 256)
        assert S == max(1, min(cus // tiles, K // 128 // ops.SPLITK_I8_MIN_K_TILES, ops.SPLITK_I8_MAX_SPLITS)), \
            (M, N, K, cus)
        assert S <= K // 128
        assert size == S * 256 * _ceil(M, 256) * 256 * _ceil(N, 256) * 4
    # the shapes the rule was made for: down at 512 and 1024 rows on 256 compute units
    assert ops.splitk_gemm_i8_plan(512, 4096, 14336, cus=256)[0] == 8
    assert ops.splitk_gemm_i8_plan(1024, 4096, 14336, cus=256)[0] == 4


@pytest.mark.parametrize("K", [128, 256, 384, 896, 1024, 1664, 2176, 4096, 14336, 32768])
def test_every_k_tile_belongs_to_exactly_one_split(K):
    from quantool_amd.hip import ops

    kt = K // 128
    for S in sorted({1, 2, 3, 5, 7, 8, 16, 17, kt, ops.SPLITK_I8_MAX_SPLITS}):
        if S > min(kt, ops.SPLITK_I8_MAX_SPLITS):
            with pytest.raises(ValueError, match=f"splits {S} > "):
                ops.splitk_gemm_i8_plan(300, 264, K, cus=256, splits=S)
            continue
        got, size = ops.splitk_gemm_i8_plan(300, 264, K, cus=256, splits=S)
        assert got == S and size == S * 512 * 512 * 4                 # requested S is honoured
        ranges = ops.splitk_ranges(K, S)
        assert len(ranges) == S and ranges[0][0] == 0 and ranges[-1][1] == kt
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))   # contiguous, in order: a partition of [0, kt)
        sizes = [t1 - t0 for t0, t1 in ranges]
        assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


def test_plan_refuses_what_the_kernel_does_not_take():
    from quantool_amd.hip import ops

    for (M, N, K, cus, S), reason in {(300, 264, 1000, 256, 0): "not a multiple of the k-unit",
                                      (300, 264, 32768 + 128, 256, 0): "32768",
                                      (0, 264, 1024, 256, 0): "bad arguments",
                                      (300, 264, 1024, 0, 0): "compute unit count",
                                      (300, 264, 1024, 256, 9): "splits 9 > K / 128 = 8"}.items():
        with pytest.raises(ValueError, match=reason):
            ops.splitk_gemm_i8_plan(M, N, K, cus=cus, splits=S)


# ---- refusals before the library ------------------------------------------------------------------------------------
def _refused_cases():
    i8 = lambda *s: torch.zeros(*s, dtype=torch.int8)   # noqa: E731
    return {
        "packed int4": (i8(300, 1024), torch.zeros(8, 128, dtype=torch.int32), torch.ones(8, 1), "int8 weights only"),
        "G = K/128 > 1": (i8(300, 1024), i8(8, 1024), torch.ones(8, 8), "one scale group"),
        "ragged K": (i8(300, 1040), i8(8, 1040), torch.ones(8, 1), "not a multiple"),
        "K past the accumulator bound": (i8(1, 32768 + 128), i8(2, 32768 + 128), torch.ones(2, 1), "32768"),
        "misaligned Xq": (aligned_i8(300, 1024, shift=1), aligned_i8(8, 1024), torch.ones(8, 1), "16-byte aligned"),
        "misaligned Wq": (aligned_i8(300, 1024), aligned_i8(8, 1024, shift=1), torch.ones(8, 1), "16-byte aligned"),
    }


@pytest.mark.parametrize("case", ["packed int4", "G = K/128 > 1", "ragged K", "K past the accumulator bound",
                                  "misaligned Xq", "misaligned Wq"])
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    from quantool_amd.hip import _lib, ops

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(ops, "load", boom)
    Xq, Wq, s_w, reason = _refused_cases()[case]
    why = ops._i8_refusal(ops.I8_SPLITK_FORM, Xq, Wq, s_w)
    assert why is not None and re.search(reason, why), why
    assert ops.splitk_gemm_i8_supported(Xq, Wq, s_w) is False
    with pytest.raises(ValueError, match=reason):
        ops.splitk_gemm_i8(Xq, torch.ones(Xq.shape[0]), Wq, s_w, K=Xq.shape[1])


def test_supported_operands(monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    assert ops.splitk_gemm_i8_supported(aligned_i8(300, 1024), aligned_i8(8, 1024), torch.ones(8, 1)) is True


# ---- dispatch -------------------------------------------------------------------------------------------------------
class Recorder(i8_fake_ops.Recorder):
    """tests/i8_fake_ops.py's stand-in plus the two names of this form; ``touched`` lists every read of either."""

    def __init__(self):
        super().__init__(watch=None)
        self.splitk_supported = True
        self.touched = []
        del self.I8_SPLITK_FORM                       # a constant the modules have no business reading

    def __getattr__(self, name):                      # only reached for names the instance does not carry
        if name == "splitk_gemm_i8":
            self.touched.append(name)
            return self._dense(name)
        if name == "splitk_gemm_i8_supported":
            self.touched.append(name)
            return lambda Xq, Wq, s_w: self.splitk_supported
        raise AttributeError(name)


@pytest.fixture
def fake_ops(monkeypatch):
    import quantool_amd.hip as hip
    from quantool_amd.engine.qmodules import QuantizedLinear
    from quantool_amd.hip import ops as real   # noqa: F401  (the attribute the modules import must exist first)

    rec = Recorder()
    monkeypatch.setattr(hip, "ops", rec)
    for name, value in LINEAR_ATTRS.items():
        monkeypatch.setattr(QuantizedLinear, name, value)
    return rec


def _linear(K=1024, N=24, int4=False, groups=None):
    from quantool_amd.engine.qmodules import QuantizedLinear

    w = torch.zeros(N, K // 8, dtype=torch.int32) if int4 else torch.zeros(N, K, dtype=torch.int8)
    G = groups if groups is not None else (K // 128 if int4 else 1)
    return QuantizedLinear(K, N, w, torch.ones(N, G), act_symmetric=not int4)


def _one(fake_ops, lin, shape):
    fake_ops.calls.clear()
    y = lin(torch.zeros(shape, dtype=torch.bfloat16))
    assert len(fake_ops.calls) == 1 and y.shape == (*shape[:-1], lin.out_features)
    return fake_ops.calls[0]


def test_class_attributes_are_ints_and_keep_short_reductions_on_the_tiled_kernel():
    from quantool_amd.engine.qmodules import QuantizedLinear

    assert type(QuantizedLinear.splitk_min_m) is int and QuantizedLinear.splitk_min_m >= 0
    assert type(QuantizedLinear.splitk_min_k) is int and QuantizedLinear.splitk_min_k >= 1024


def test_range_edges(fake_ops):
    lin = _linear()
    assert _one(fake_ops, lin, (255, 1024)) == ("gemm_i8", 255)             # splitk_min_m - 1
    assert fake_ops.touched == []                                           # below the bound no new name is read
    assert _one(fake_ops, lin, (256, 1024)) == ("splitk_gemm_i8", 256)      # splitk_min_m
    assert _one(fake_ops, lin, (2047, 1024)) == ("splitk_gemm_i8", 2047)    # ring_min_m - 1
    assert _one(fake_ops, lin, (2, 300, 1024)) == ("splitk_gemm_i8", 600)
    fake_ops.touched.clear()
    assert _one(fake_ops, lin, (2048, 1024)) == ("gemm_i8_ring", 2048)      # ring_min_m
    assert _one(fake_ops, lin, (128, 1024)) == ("gemm_i8_mid", 128)
    assert _one(fake_ops, lin, (16, 1024)) == ("gemm_i8_skinny", 16)
    assert fake_ops.touched == []


def test_without_a_ring_the_range_has_no_upper_edge(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_min_m", 0)
    assert _one(fake_ops, _linear(), (4096, 1024)) == ("splitk_gemm_i8", 4096)


def test_short_reductions_stay_on_the_tiled_kernel(fake_ops):
    assert _one(fake_ops, _linear(K=896), (600, 896)) == ("gemm_i8", 600)   # in_features < splitk_min_k
    assert _one(fake_ops, _linear(K=512), (600, 512)) == ("gemm_i8", 600)
    assert fake_ops.touched == []


def test_int4_and_grouped_scales_stay_on_the_tiled_kernel(fake_ops):
    assert _one(fake_ops, _linear(int4=True), (600, 1024)) == ("gemm_i8", 600)
    assert _one(fake_ops, _linear(groups=8), (600, 1024)) == ("gemm_i8", 600)     # int8 levels, G = K/128
    assert fake_ops.touched == []


def test_unsupported_operands_fall_to_the_tiled_kernel(fake_ops):
    fake_ops.splitk_supported = False
    assert _one(fake_ops, _linear(), (600, 1024)) == ("gemm_i8", 600)
    assert fake_ops.touched == ["splitk_gemm_i8_supported"]


def test_zero_never_uses_it_and_touches_no_new_name(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "splitk_min_m", 0)
    lin = _linear()
    for shape, name in (((1, 1024), "gemm_i8_skinny"), ((64, 1024), "gemm_i8_mid"), ((129, 1024), "gemm_i8"),
                        ((600, 1024), "gemm_i8"), ((2047, 1024), "gemm_i8"), ((2048, 1024), "gemm_i8_ring")):
        assert _one(fake_ops, lin, shape)[0] == name
    assert fake_ops.touched == []
