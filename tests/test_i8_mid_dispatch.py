"""The mid-M int8 GEMM's surface without a GPU: the header, the ctypes table and the built library carry
``qt_gemm_i8_mid``, ``ops.gemm_i8_mid_supported`` / ``ops.gemm_i8_mid`` refuse what the kernel does not take before they
touch the library, and ``QuantizedLinear`` picks the kernel by ``mid_max_m`` / ``mid_max_n`` / ``mid_min_k`` (with
``quantool_amd.hip.ops`` replaced by a recording fake, so nothing reaches a device)."""
import re

import pytest
import torch

from tests.i8_fake_ops import aligned_i8 as _aligned_i8
from tests.i8_fake_ops import check_surface, fake_ops, header_constants, header_text  # noqa: F401

NAME = "qt_gemm_i8_mid"
WATCH = "gemm_i8_mid_supported"
# the dispatch rules under test, whatever the measured class defaults are
LINEAR_ATTRS = {"skinny_max_m": 16, "ring_min_m": 2048, "mid_max_m": 96, "mid_max_n": 0, "mid_min_k": 512}


# ---- surface --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_constants():
    from quantool_amd.hip import ops

    check_surface("header", NAME)
    assert header_constants("QT_I8_MID_") == {"QT_I8_MID_MAX_M": ops.I8_MID_MAX_M,
                                              "QT_I8_MID_K_UNIT": ops.I8_MID_K_UNIT}
    assert ops.I8_MID_MAX_M == 128 and ops.I8_MID_K_UNIT == 128
    assert f"{NAME}:" in header_text()[0]                 # documented in the A8 block's comment


def test_ctypes_table_holds_it_with_the_tiled_signature():
    check_surface("ctypes", NAME, "qt_gemm_i8")


def test_library_exports_it():
    check_surface("library", NAME)


def test_no_workspace_function_was_added():
    from quantool_amd.hip import _lib

    assert len([n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")]) == 14
    assert not [n for n in _lib.SIGNATURES if "mid" in n and n != NAME]


def test_build_audits_cover_the_new_file():
    from quantool_amd.csrc import build

    assert "gemm_i8_mid_kernel" in build.NO_SPILL_KERNELS
    assert build.CSRC / "qlinear_mid.hip" in build.sources()
    assert "-ffp-contract=off" in build.HIPCC_FLAGS
    assert build.SCRATCH_OK == ()                          # any kernel with a private segment fails the build
    res = build.OBJ_DIR / "qlinear_mid.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    rows = [line for line in res.read_text().splitlines() if "gemm_i8_mid_kernel" in line]
    assert len(rows) == 12                                  # MT 2 / 4 / 8 x int8 / int4 x one group / K/128 groups
    for row in rows:
        assert "scratch 0\t" in row and "vgpr_spill 0\t" in row, row
        assert int(re.search(r"lds (\d+)", row).group(1)) <= 65536, row


# ---- refusals before the library ------------------------------------------------------------------------------------
REFUSED = {
    "M = 0": (lambda: (_aligned_i8(0, 256), _aligned_i8(8, 256), torch.ones(8, 1)), "1 <= M <= 128"),
    "M = 129": (lambda: (_aligned_i8(129, 256), _aligned_i8(8, 256), torch.ones(8, 1)), "1 <= M <= 128"),
    "ragged K": (lambda: (_aligned_i8(32, 192), _aligned_i8(8, 192), torch.ones(8, 1)), "not a multiple"),
    "K past the accumulator bound": (lambda: (_aligned_i8(17, 32768 + 128), _aligned_i8(2, 32768 + 128),
                                              torch.ones(2, 1)), "32768"),
    "G = 2 at K = 512": (lambda: (_aligned_i8(32, 512), _aligned_i8(8, 512), torch.ones(8, 2)), "G must be 1 or"),
    "misaligned Xq": (lambda: (_aligned_i8(32, 256, shift=1), _aligned_i8(8, 256), torch.ones(8, 1)), "16-byte aligned"),
    "misaligned Wq": (lambda: (_aligned_i8(32, 256), _aligned_i8(8, 256, shift=1), torch.ones(8, 1)), "16-byte aligned"),
    "float weights": (lambda: (_aligned_i8(32, 256), torch.zeros(8, 256), torch.ones(8, 1)), "weights only"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    from quantool_amd.hip import _lib, ops

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(ops, "load", boom)
    make, reason = REFUSED[case]
    Xq, Wq, s_w = make()
    assert ops.gemm_i8_mid_supported(Xq, Wq, s_w) is False
    assert reason in ops._i8_refusal(ops.I8_FORMS[NAME], Xq, Wq, s_w)
    with pytest.raises(ValueError, match=reason):
        ops.gemm_i8_mid(Xq, torch.ones(Xq.shape[0]), Wq, s_w, K=Xq.shape[1])


def test_supported_operands(monkeypatch):
    from quantool_amd.hip import _lib, ops

    boom = lambda: (_ for _ in ()).throw(AssertionError("the library was touched"))   # noqa: E731
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(ops, "load", boom)
    for M in (1, 17, 128):
        assert ops.gemm_i8_mid_supported(_aligned_i8(M, 512), _aligned_i8(8, 512), torch.ones(8, 1)) is True
        assert ops.gemm_i8_mid_supported(_aligned_i8(M, 512), _aligned_i8(8, 512), torch.ones(8, 4)) is True
        assert ops.gemm_i8_mid_supported(_aligned_i8(M, 512), torch.zeros(8, 64, dtype=torch.int32),
                                         torch.ones(8, 4)) is True


# ---- dispatch -------------------------------------------------------------------------------------------------------
def _linear(K=512, N=24, int4=False):
    from quantool_amd.engine.qmodules import QuantizedLinear

    w = torch.zeros(N, K // 8, dtype=torch.int32) if int4 else torch.zeros(N, K, dtype=torch.int8)
    return QuantizedLinear(K, N, w, torch.ones(N, K // 128 if int4 else 1), act_symmetric=not int4)


def _one(fake_ops, lin, shape):
    fake_ops.calls.clear()
    y = lin(torch.zeros(shape, dtype=torch.bfloat16))
    assert len(fake_ops.calls) == 1 and y.shape == (*shape[:-1], lin.out_features)
    return fake_ops.calls[0]


def test_class_defaults_are_sane():
    from quantool_amd.engine.qmodules import QuantizedLinear
    from quantool_amd.hip import ops

    for name in ("mid_max_m", "mid_max_n", "mid_min_k"):
        assert type(getattr(QuantizedLinear, name)) is int and getattr(QuantizedLinear, name) >= 0
    assert QuantizedLinear.mid_max_m <= ops.I8_MID_MAX_M
    assert QuantizedLinear.mid_min_k >= 512             # smaller Linears are launch-bound: they stay on the tiled kernel


def test_mid_range_goes_to_the_mid_kernel(fake_ops):
    lin = _linear()
    assert _one(fake_ops, lin, (16, 512)) == ("gemm_i8_skinny", 16)        # the skinny range keeps precedence
    assert _one(fake_ops, lin, (1, 512)) == ("gemm_i8_skinny", 1)
    assert fake_ops.asked == 0
    assert _one(fake_ops, lin, (17, 512)) == ("gemm_i8_mid", 17)
    assert _one(fake_ops, lin, (96, 512)) == ("gemm_i8_mid", 96)           # at mid_max_m
    assert _one(fake_ops, lin, (2, 48, 512)) == ("gemm_i8_mid", 96)
    assert fake_ops.asked == 3
    assert _one(fake_ops, lin, (97, 512)) == ("gemm_i8", 97)               # mid_max_m + 1
    assert fake_ops.asked == 3


def test_mid_max_m_is_capped_by_the_kernel(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "mid_max_m", 1000)
    lin = _linear()
    assert _one(fake_ops, lin, (128, 512)) == ("gemm_i8_mid", 128)
    assert _one(fake_ops, lin, (129, 512)) == ("gemm_i8", 129)
    assert fake_ops.asked == 1


def test_mid_max_m_zero_never_uses_it(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "mid_max_m", 0)
    lin = _linear()
    for M in (17, 64, 128, 129):
        assert _one(fake_ops, lin, (M, 512)) == ("gemm_i8", M)
    assert fake_ops.asked == 0


def test_small_k_stays_on_the_tiled_gemm(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    assert _one(fake_ops, _linear(K=384), (17, 384)) == ("gemm_i8", 17)
    assert fake_ops.asked == 0
    monkeypatch.setattr(QuantizedLinear, "mid_min_k", 384)
    assert _one(fake_ops, _linear(K=384), (17, 384)) == ("gemm_i8_mid", 17)


def test_large_n_stays_on_the_tiled_gemm(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "mid_max_n", 24)
    assert _one(fake_ops, _linear(N=24), (17, 512)) == ("gemm_i8_mid", 17)
    assert fake_ops.asked == 1
    assert _one(fake_ops, _linear(N=25), (17, 512)) == ("gemm_i8", 17)
    assert fake_ops.asked == 1


def test_unsupported_operands_fall_to_the_tiled_gemm(fake_ops):
    fake_ops.supported = False
    assert _one(fake_ops, _linear(), (17, 512)) == ("gemm_i8", 17)
    assert fake_ops.asked == 1


def test_int4_grouped_linear_goes_to_the_mid_kernel(fake_ops):
    lin = _linear(int4=True)
    assert lin.weight_scale.shape[1] == 512 // 128
    assert _one(fake_ops, lin, (32, 512)) == ("gemm_i8_mid", 32)
    assert _one(fake_ops, lin, (8, 512)) == ("gemm_i8_skinny", 8)


def test_ring_keeps_precedence(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_min_m", 17)
    lin = _linear()
    assert _one(fake_ops, lin, (17, 512)) == ("gemm_i8_ring", 17)
    assert _one(fake_ops, lin, (16, 512)) == ("gemm_i8_skinny", 16)
    assert fake_ops.asked == 0
    # an int4 Linear never takes the ring: the mid kernel is next in line
    assert _one(fake_ops, _linear(int4=True), (17, 512)) == ("gemm_i8_mid", 17)
    monkeypatch.setattr(QuantizedLinear, "ring_min_m", 2048)
    assert _one(fake_ops, lin, (2048, 512)) == ("gemm_i8_ring", 2048)
    assert _one(fake_ops, lin, (2047, 512)) == ("gemm_i8", 2047)
