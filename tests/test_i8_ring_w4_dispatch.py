"""The packed-int4 LDS-ring GEMM's surface without a GPU: the header, the ctypes table and the built library carry
``qt_gemm_i8_ring_w4``, ``ops.gemm_i8_ring_w4_supported`` / ``ops.gemm_i8_ring_w4`` refuse what the kernel does not take
before they touch the library, and ``QuantizedLinear`` picks it by ``ring_w4_min_m`` (with ``quantool_amd.hip.ops``
replaced by a recording fake, so nothing reaches a device)."""
import pytest
import torch

from tests.i8_fake_ops import aligned_i8, aligned_i32, check_surface, fake_ops, header_constants  # noqa: F401

NAME = "qt_gemm_i8_ring_w4"
WATCH = "gemm_i8_ring_w4_supported"


# ---- surface --------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_instance_constants():
    from quantool_amd.hip import ops

    check_surface("header", NAME)
    assert header_constants("QT_I8_RING_W4_") == {"QT_I8_RING_W4_K_UNIT": ops.I8_RING_W4_K_UNIT,
                                                  "QT_I8_RING_W4_SLOTS": ops.I8_RING_W4_SLOTS,
                                                  "QT_I8_RING_W4_LEAD": ops.I8_RING_W4_LEAD}
    # a K-tile is one weight group, and the ring's WAR argument needs lead <= slots - 2
    assert ops.I8_RING_W4_K_UNIT == 128
    assert 1 <= ops.I8_RING_W4_LEAD <= ops.I8_RING_W4_SLOTS - 2
    assert callable(ops.gemm_i8_ring_w4) and callable(ops.gemm_i8_ring_w4_supported)


def test_ctypes_table_holds_it_with_the_tiled_signature():
    check_surface("ctypes", NAME, "qt_gemm_i8")


def test_library_exports_it():
    check_surface("library", NAME)


def test_build_audits_cover_the_new_file():
    import inspect

    from quantool_amd.csrc import build

    assert "gemm_i8_ring_w4_kernel" in build.NO_SPILL_KERNELS
    assert '"qlinear_ring_w4.hip"' in inspect.getsource(build.build)    # audit_m0's list
    assert build.CSRC / "qlinear_ring_w4.hip" in build.sources()
    res = build.OBJ_DIR / "qlinear_ring_w4.resources.txt"
    if res.exists():                                                    # written by the build: no scratch, no spills
        rows = [line for line in res.read_text().splitlines() if "gemm_i8_ring_w4_kernel" in line]
        assert len(rows) == 2                                           # symmetric and asymmetric activations
        assert all("scratch 0\t" in r and "vgpr_spill 0\t" in r for r in rows)


# ---- refusals before the library ------------------------------------------------------------------------------------
def _refused_cases():
    from quantool_amd.hip import ops

    U = ops.I8_RING_W4_K_UNIT
    i8 = lambda *s: torch.zeros(*s, dtype=torch.int8)          # noqa: E731
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)        # noqa: E731
    return {
        "int8 weight": (i8(4, 256), i8(8, 256), torch.ones(8, 2), "packed int4"),
        "G = 1": (i8(4, 256), i32(8, 32), torch.ones(8, 1), "one scale per group"),
        "ragged K": (i8(4, 3 * U + 16), i32(8, (3 * U + 16) // 8), torch.ones(8, 4), "not a multiple"),
        "K past the accumulator bound": (i8(1, 32768 + U), i32(2, (32768 + U) // 8), torch.ones(2, 257), "32768"),
    }


@pytest.mark.parametrize("case", ["int8 weight", "G = 1", "ragged K", "K past the accumulator bound"])
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    from quantool_amd.hip import ops

    def boom():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(ops, "load", boom)
    Xq, Wq, s_w, reason = _refused_cases()[case]
    assert ops.gemm_i8_ring_w4_supported(Xq, Wq, s_w) is False
    with pytest.raises(ValueError, match=reason):
        ops.gemm_i8_ring_w4(Xq, torch.ones(Xq.shape[0]), Wq, s_w, K=Xq.shape[1])


def test_supported_operands_and_alignment(monkeypatch):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    U = ops.I8_RING_W4_K_UNIT
    K = 4 * U
    Wq, s_w = torch.zeros(8, K // 8, dtype=torch.int32), torch.ones(8, 4)
    aligned, shifted = aligned_i8(4, K), aligned_i8(4, K, shift=1)
    w_shifted = aligned_i32(8, K // 8, shift=1)
    assert aligned.data_ptr() % 16 == 0 and Wq.data_ptr() % 16 == 0
    assert shifted.data_ptr() % 16 == 1 and w_shifted.data_ptr() % 16 == 4
    assert ops.gemm_i8_ring_w4_supported(aligned, Wq, s_w) is True
    assert ops.gemm_i8_ring_w4_supported(shifted, Wq, s_w) is False
    assert ops.gemm_i8_ring_w4_supported(aligned, w_shifted, s_w) is False
    # one K-tile: the one group is the whole row, G = K / 128 = 1 is taken
    assert ops.gemm_i8_ring_w4_supported(aligned.view(16, U), torch.zeros(8, U // 8, dtype=torch.int32),
                                         torch.ones(8, 1)) is True
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.gemm_i8_ring_w4(shifted, torch.ones(4), Wq, s_w, K=K)


# ---- dispatch -------------------------------------------------------------------------------------------------------
def _linear(K=512, N=24, int4=True, G=None):
    from quantool_amd.engine.qmodules import QuantizedLinear

    w = torch.zeros(N, K // 8, dtype=torch.int32) if int4 else torch.zeros(N, K, dtype=torch.int8)
    G = (K // 128 if int4 else 1) if G is None else G
    return QuantizedLinear(K, N, w, torch.ones(N, G), act_symmetric=False)


def _one(fake_ops, lin, shape):
    fake_ops.calls.clear()
    y = lin(torch.zeros(shape, dtype=torch.bfloat16))
    assert len(fake_ops.calls) == 1 and y.shape == (*shape[:-1], lin.out_features)
    return fake_ops.calls[0]


def test_default_is_off_or_a_prefill_size():
    from quantool_amd.engine.qmodules import QuantizedLinear

    d = QuantizedLinear.ring_w4_min_m
    assert type(d) is int and (d == 0 or d >= 2048)
    assert f"ring_w4_min_m={d}" in repr(_linear())


def test_int4_linear_takes_the_w4_ring_from_the_attribute_on(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_w4_min_m", 600)
    lin = _linear()
    assert _one(fake_ops, lin, (600, 512)) == ("gemm_i8_ring_w4", 600)
    assert _one(fake_ops, lin, (2, 300, 512)) == ("gemm_i8_ring_w4", 600)
    assert _one(fake_ops, lin, (4096, 512)) == ("gemm_i8_ring_w4", 4096)
    assert fake_ops.asked == 3


def test_below_the_attribute_nothing_changes(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_w4_min_m", 600)
    lin = _linear()
    assert _one(fake_ops, lin, (599, 512)) == ("gemm_i8", 599)
    assert _one(fake_ops, lin, (129, 512)) == ("gemm_i8", 129)
    assert _one(fake_ops, lin, (128, 512)) == ("gemm_i8_mid", 128)
    assert _one(fake_ops, lin, (17, 512)) == ("gemm_i8_mid", 17)
    assert _one(fake_ops, lin, (16, 512)) == ("gemm_i8_skinny", 16)
    assert _one(fake_ops, lin, (1, 512)) == ("gemm_i8_skinny", 1)
    assert fake_ops.asked == 0                         # below the bound the new names are not touched


def test_zero_never_uses_it_and_never_asks(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_w4_min_m", 0)
    lin = _linear()
    for shape, want in (((1, 512), "gemm_i8_skinny"), ((17, 512), "gemm_i8_mid"), ((2048, 512), "gemm_i8"),
                        ((4, 2048, 512), "gemm_i8")):
        assert _one(fake_ops, lin, shape)[0] == want
    assert fake_ops.asked == 0


def test_unsupported_operands_fall_to_the_tiled_gemm(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_w4_min_m", 600)
    fake_ops.supported = False
    assert _one(fake_ops, _linear(), (1024, 512)) == ("gemm_i8", 1024)
    assert fake_ops.asked == 1


def test_int8_and_channelwise_int4_linears_never_reach_it(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_w4_min_m", 600)
    monkeypatch.setattr(QuantizedLinear, "ring_min_m", 2048)
    assert _one(fake_ops, _linear(int4=False), (1024, 512)) == ("gemm_i8", 1024)
    assert _one(fake_ops, _linear(int4=False), (2048, 512)) == ("gemm_i8_ring", 2048)
    assert _one(fake_ops, _linear(int4=True, G=1), (2048, 512)) == ("gemm_i8", 2048)
    assert fake_ops.asked == 0


def test_skinny_range_keeps_precedence(fake_ops, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "ring_w4_min_m", 1)
    lin = _linear()
    assert _one(fake_ops, lin, (16, 512)) == ("gemm_i8_skinny", 16)
    assert _one(fake_ops, lin, (17, 512)) == ("gemm_i8_ring_w4", 17)
