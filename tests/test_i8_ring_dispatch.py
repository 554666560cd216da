"""The LDS-ring int8 GEMM's surface without a GPU: the header, the ctypes table and the built library carry
``qt_gemm_i8_ring``, ``ops.gemm_i8_ring_supported`` / ``ops.gemm_i8_ring`` refuse what the kernel does not take before
they touch the library, and ``QuantizedLinear`` picks the ring by ``ring_min_m`` (with ``quantool_amd.hip.ops`` replaced
by a recording fake, so nothing reaches a device)."""
import pytest
import torch

from tests.i8_fake_ops import aligned_i8, check_surface, fake_ops, header_constants  # noqa: F401

NAME = "qt_gemm_i8_ring"
WATCH = "gemm_i8_ring_supported"


# ---- surface --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_ring_constants():
    from quantool_amd.hip import ops

    check_surface("header", NAME)
    assert header_constants("QT_I8_RING_") == {"QT_I8_RING_K_UNIT": ops.I8_RING_K_UNIT,
                                               "QT_I8_RING_SLOTS": ops.I8_RING_SLOTS,
                                               "QT_I8_RING_LEAD": ops.I8_RING_LEAD}
    # the contract's limits: a unit of at most 128 that divides both Llama-3-8B reduction lengths, lead <= slots - 2
    U = ops.I8_RING_K_UNIT
    assert 0 < U <= 128 and 4096 % U == 0 and 14336 % U == 0
    assert 1 <= ops.I8_RING_LEAD <= ops.I8_RING_SLOTS - 2


def test_ctypes_table_holds_it_with_the_tiled_signature():
    check_surface("ctypes", NAME, "qt_gemm_i8")


def test_library_exports_it():
    check_surface("library", NAME)


def test_no_workspace_function_was_added():
    from quantool_amd.hip import _lib

    assert not [n for n in _lib.SIGNATURES if "ring" in n and n.endswith("_workspace_bytes")]


def test_build_audits_cover_the_new_file():
    import inspect

    from quantool_amd.csrc import build

    assert "gemm_i8_ring_kernel" in build.NO_SPILL_KERNELS
    assert '"qlinear_ring.hip"' in inspect.getsource(build.build)       # audit_m0's list
    assert build.CSRC / "qlinear_ring.hip" in build.sources()
    assert "-ffp-contract=off" in build.HIPCC_FLAGS
    res = build.OBJ_DIR / "qlinear_ring.resources.txt"
    if res.exists():                                                    # written by the build: no scratch, no spills
        row = [line for line in res.read_text().splitlines() if "gemm_i8_ring_kernel" in line]
        assert len(row) == 1 and "scratch 0\t" in row[0] and "vgpr_spill 0\t" in row[0]


# ---- refusals before the library ------------------------------------------------------------------------------------
def _refused_cases():
    from quantool_amd.hip import ops

    U = ops.I8_RING_K_UNIT
    i8 = lambda *s: torch.zeros(*s, dtype=torch.int8)   # noqa: E731
    return {
        "packed int4": (i8(4, 256), torch.zeros(8, 32, dtype=torch.int32), torch.ones(8, 1), "int8 weights only"),
        "G = K/128 > 1": (i8(4, 256), i8(8, 256), torch.ones(8, 2), "one scale group"),
        "ragged K": (i8(4, 3 * U + 16), i8(8, 3 * U + 16), torch.ones(8, 1), "not a multiple"),
        "K past the accumulator bound": (i8(1, 32768 + U), i8(2, 32768 + U), torch.ones(2, 1), "32768"),
    }


@pytest.mark.parametrize("case", ["packed int4", "G = K/128 > 1", "ragged K", "K past the accumulator bound"])
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    from quantool_amd.hip import ops

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(ops, "load", boom)
    Xq, Wq, s_w, reason = _refused_cases()[case]
    assert ops.gemm_i8_ring_supported(Xq, Wq, s_w) is False
    with pytest.raises(ValueError, match=reason):
        ops.gemm_i8_ring(Xq, torch.ones(Xq.shape[0]), Wq, s_w, K=Xq.shape[1])


def test_supported_operands_and_alignment(monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    U = ops.I8_RING_K_UNIT
    Wq, s_w = torch.zeros(8, 4 * U, dtype=torch.int8), torch.ones(8, 1)
    aligned, shifted = aligned_i8(4, 4 * U), aligned_i8(4, 4 * U, shift=1)
    assert aligned.data_ptr() % 16 == 0 and Wq.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 1
    assert ops.gemm_i8_ring_supported(aligned, Wq, s_w) is True
    assert ops.gemm_i8_ring_supported(shifted, Wq, s_w) is False
    assert ops.gemm_i8_ring_supported(Wq, shifted, torch.ones(4, 1)) is False
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.gemm_i8_ring(shifted, torch.ones(4), Wq, s_w)


# ---- dispatch -------------------------------------------------------------------------------------------------------
def _linear(K=256, N=24, int4=False):
    from quantool_amd.engine.qmodules import QuantizedLinear

    w = torch.zeros(N, K // 8, dtype=torch.int32) if int4 else torch.zeros(N, K, dtype=torch.int8)
    return QuantizedLinear(K, N, w, torch.ones(N, K // 128 if int4 else 1), act_symmetric=not int4)


def _one(fake_ops, lin, shape):
    fake_ops.calls.clear()
    y = lin(torch.zeros(shape, dtype=torch.bfloat16))
    assert len(fake_ops.calls) == 1 and y.shape == (*shape[:-1], lin.out_features)
    return fake_ops.calls[0]


def test_quantized_linear_sends_large_m_to_the_ring(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    assert type(QuantizedLinear.ring_min_m) is int and QuantizedLinear.ring_min_m >= 0
    monkeypatch.setattr(QuantizedLinear, "ring_min_m", 512)
    lin = _linear()
    assert _one(fake_ops, lin, (511, 256)) == ("gemm_i8", 511)
    assert fake_ops.asked == 0                        # below the bound the new names are not touched
    assert _one(fake_ops, lin, (512, 256)) == ("gemm_i8_ring", 512)
    assert _one(fake_ops, lin, (2, 300, 256)) == ("gemm_i8_ring", 600)
    assert _one(fake_ops, lin, (16, 256)) == ("gemm_i8_skinny", 16)


def test_int4_linear_stays_on_the_tiled_gemm(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_min_m", 512)
    assert _one(fake_ops, _linear(int4=True), (1024, 256)) == ("gemm_i8", 1024)


def test_ring_min_m_zero_never_uses_the_ring(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_min_m", 0)
    lin = _linear()
    for shape in ((1, 256), (17, 256), (512, 256), (4, 2048, 256)):
        name, _ = _one(fake_ops, lin, shape)
        assert name == ("gemm_i8_skinny" if shape == (1, 256) else "gemm_i8")
    assert fake_ops.asked == 0


def test_unsupported_operands_fall_to_the_tiled_gemm(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_min_m", 512)
    fake_ops.supported = False
    assert _one(fake_ops, _linear(), (1024, 256)) == ("gemm_i8", 1024)
    assert fake_ops.asked == 1


def test_skinny_range_keeps_precedence(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_min_m", 1)
    lin = _linear()
    assert _one(fake_ops, lin, (16, 256)) == ("gemm_i8_skinny", 16)
    assert _one(fake_ops, lin, (17, 256)) == ("gemm_i8_ring", 17)
