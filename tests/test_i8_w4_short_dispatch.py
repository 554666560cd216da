"""qt_w4_short_gemm_i8 without a GPU: the refusals before the library is touched, and the route from
``QuantizedLinear`` by ``w4_short_min_m`` (``quantool_amd.hip.ops`` replaced by the recording fake)."""
import pytest
import torch

from tests.i8_fake_ops import aligned_i8, aligned_i32, fake_ops  # noqa: F401
from tests.test_i8_ring_w4_dispatch import _linear, _one

LINEAR_ATTRS = {"skinny_max_m": 16, "mid_max_m": 128, "ring_w4_min_m": 8192}
MARK = "gemm_i8_w4_short"


REFUSED = {
    "int8 weight": lambda: (aligned_i8(4, 256), aligned_i8(8, 256), torch.ones(8, 2), "packed int4"),
    "channel-wise scales": lambda: (aligned_i8(4, 256), aligned_i32(8, 32), torch.ones(8, 1), "one scale per group"),
    "ragged K": lambda: (aligned_i8(4, 400), aligned_i32(8, 50), torch.ones(8, 4), "not a multiple"),
    "K past the accumulator bound": lambda: (aligned_i8(1, 32896), aligned_i32(2, 4112), torch.ones(2, 257), "32768"),
    "misaligned Xq": lambda: (aligned_i8(4, 256, shift=1), aligned_i32(8, 32), torch.ones(8, 2), "16-byte aligned"),
    "misaligned Wq": lambda: (aligned_i8(4, 256), aligned_i32(8, 32, shift=1), torch.ones(8, 2), "16-byte aligned"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_unsupported_operands_are_refused_before_the_library(monkeypatch, case):
    from quantool_amd.hip import ops

    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    Xq, Wq, s_w, reason = REFUSED[case]()
    assert ops.gemm_i8_w4_short_supported(Xq, Wq, s_w) is False
    with pytest.raises(ValueError, match=reason):
        ops.gemm_i8_w4_short(Xq, torch.ones(Xq.shape[0]), Wq, s_w, K=Xq.shape[1])
    assert ops.gemm_i8_w4_short_supported(aligned_i8(4, 256), aligned_i32(8, 32), torch.ones(8, 2)) is True
    assert ops.gemm_i8_w4_short_supported(aligned_i8(4, 128), aligned_i32(8, 16), torch.ones(8, 1)) is True


def _route(fake_ops, monkeypatch, lin, M, min_m, supported=True, ring_w4=8192):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "w4_short_min_m", min_m)
    monkeypatch.setattr(QuantizedLinear, "ring_w4_min_m", ring_w4)
    if min_m:
        fake_ops.gemm_i8_w4_short = fake_ops._dense(MARK)
        fake_ops.gemm_i8_w4_short_supported = lambda Xq, Wq, s_w: supported
    return _one(fake_ops, lin, (M, lin.in_features))[0]


@pytest.mark.parametrize("M,min_m,want", [
    (129, 129, MARK), (200, 129, MARK), (8191, 129, MARK), (512, 512, MARK),
    (128, 129, "gemm_i8_mid"), (16, 129, "gemm_i8_skinny"), (511, 512, "gemm_i8"),
    (8192, 129, "gemm_i8_ring_w4"), (20000, 129, "gemm_i8_ring_w4"), (300, 0, "gemm_i8")])
def test_packed_g128_linear_takes_it_between_min_m_and_the_w4_ring(fake_ops, monkeypatch, M, min_m, want):
    from quantool_amd.engine.qmodules import QuantizedLinear

    assert QuantizedLinear.w4_short_min_m == 0 and "w4_short_min_m=0" in repr(_linear())    # the shipped default
    assert _route(fake_ops, monkeypatch, _linear(), M, min_m) == want
    if min_m == 0:                                    # the attribute at 0 reads no new name: the fake carries none
        assert not hasattr(fake_ops, "gemm_i8_w4_short") and not hasattr(fake_ops, "gemm_i8_w4_short_supported")
        return
    assert _route(fake_ops, monkeypatch, _linear(), 20000, 129, ring_w4=0) == MARK    # the w4 ring off: any M above


@pytest.mark.parametrize("what", ["int8 weight", "channel-wise int4", "below w4_short_min_k", "not supported"])
def test_other_linears_stay_where_they_were(fake_ops, monkeypatch, what):
    from quantool_amd.engine.qmodules import QuantizedLinear

    monkeypatch.setattr(QuantizedLinear, "splitk_min_m", 0)
    lin = {"int8 weight": lambda: _linear(int4=False), "channel-wise int4": lambda: _linear(G=1)}.get(what, _linear)()
    if what == "below w4_short_min_k":
        monkeypatch.setattr(QuantizedLinear, "w4_short_min_k", 1024)
    assert _route(fake_ops, monkeypatch, lin, 300, 129, supported=what != "not supported") == "gemm_i8"
