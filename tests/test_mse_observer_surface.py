"""The MSE weight observer without a GPU: the export, the modifier field, and the ``ops`` wrapper's refusals."""
import pytest
import torch

from tests.i8_fake_ops import check_surface


def test_the_entry_point_is_declared_bound_and_exported():
    from quantool_amd.hip import _lib

    check_surface("header", "qt_weight_gather_qparams_mse")
    check_surface("library", "qt_weight_gather_qparams_mse")
    assert len(_lib.SIGNATURES["qt_weight_gather_qparams_mse"][1]) == len(_lib.SIGNATURES["qt_weight_gather_qparams"][1]) + 4


def test_the_modifier_replaces_the_presets_observer():
    from quantool_amd.engine.modifiers import GPTQModifier

    assert GPTQModifier().weight_args().observer == "minmax"
    assert GPTQModifier(scheme="W8A16").weight_args().observer == "minmax"
    assert GPTQModifier(observer="mse").weight_args().observer == "mse"
    assert GPTQModifier(observer="mse").weight_args().to_config()["observer"] == "mse"


@pytest.mark.parametrize("over,match", [(dict(n_steps=0), "n_steps"), (dict(n_steps=33), "n_steps"),
                                        (dict(group_size=48), "multiple of 32"), (dict(shift=1), "16-byte aligned")])
def test_ops_refuses_before_the_library_is_touched(monkeypatch, over, match):
    """Host tensors that answer ``is_cuda`` with True, and a library that must not be reached."""
    from quantool_amd.hip import ops

    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    R, K, gs = 2, 96, over.get("group_size", 32)
    buf = torch.zeros(R * K + 8)
    off = ((-buf.data_ptr()) % 16) // 4 + over.get("shift", 0)
    out = buf[off:off + R * K].view(R, K)
    scale, zp = torch.zeros(R, K // gs), torch.zeros(R, K // gs)
    with pytest.raises(ValueError, match=match):
        ops.weight_gather_qparams_mse(torch.zeros(R, K, dtype=torch.bfloat16), None, None, gs, True, 4, out, scale, zp,
                                      n_steps=over.get("n_steps", 20))
