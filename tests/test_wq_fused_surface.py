"""The fused A16 decode forms without a GPU: the header, the ctypes table and the built library carry
the three entry points and no kernel of theirs uses scratch; ``WeightOnlyMLP`` on CPU tensors is its children
composed and names what it refuses; ``SharedOutputs`` hands an output over for the very tensor alone."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.i8_fake_ops import check_surface, header_constants, header_text
from tests.test_wq_stream_dispatch import _w4

NAMES = ("qt_gemm_wq_skinny_act_mul", "qt_gemm_wq_skinny_multi", "qt_rmsnorm")


@pytest.mark.parametrize("name", NAMES)
def test_surface(name):
    from quantool_amd.csrc import build
    from quantool_amd.hip import ops

    check_surface("header", name)
    check_surface("ctypes", name, name)                       # present in the table
    check_surface("library", name)
    assert f"{name}:" in header_text()[0]
    assert header_constants("QT_WQ_FUSED_") == {"QT_WQ_FUSED_MAX_M": ops.WQ_FUSED_MAX_M,
                                                "QT_WQ_FUSED_K_UNIT": ops.WQ_FUSED_K_UNIT}
    assert header_constants("QT_WQ_MULTI_") == {"QT_WQ_MULTI_MAX": ops.WQ_MULTI_MAX}
    res = build.OBJ_DIR / "wq_fused.resources.txt"
    if not res.exists():
        import __graft_entry__ as g

        g.build()
    rows = res.read_text().splitlines()
    assert len(rows) == 16 and all("scratch 0\t" in r and "vgpr_spill 0\t" in r for r in rows)


def _linear(N, K, seed, **kw):
    from quantool_amd.engine.qlinear import WeightOnlyLinear, pack_int4

    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-8, 8, (N, K), generator=g, dtype=torch.int8)
    return WeightOnlyLinear(K, N, pack_int4(q), torch.rand(N, K // 128, generator=g) * 0.01 + 1e-3, **kw)


def test_mlp_on_cpu_is_its_children_composed_and_refusals_are_named():
    from quantool_amd.engine.qlinear import WeightOnlyMLP

    gate, up, down = _linear(256, 128, 0), _linear(256, 128, 1), _linear(128, 256, 2)
    mlp = WeightOnlyMLP(gate, up, down, nn.SiLU())
    assert [n for n, _ in mlp.named_children()] == ["gate_proj", "up_proj", "down_proj", "act_fn"]
    x = torch.randn(2, 3, 128, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    assert torch.equal(mlp(x), down(F.silu(gate(x)) * up(x)))
    refused = {"must all be WeightOnlyLinears": (nn.Linear(128, 256), up, down, nn.SiLU()),
               "act_fn is not SiLU": (gate, up, down, nn.GELU()),
               "differ in features": (gate, _linear(128, 128, 4), down, nn.SiLU()),
               "outputs are not down_proj's inputs": (gate, up, _linear(128, 128, 5), nn.SiLU()),
               "has a bias": (_linear(256, 128, 6, bias=torch.zeros(256)), up, down, nn.SiLU()),
               "carries g_idx": (_linear(256, 128, 7, g_idx=torch.zeros(128, dtype=torch.int32)), up, down, nn.SiLU())}
    for reason, parts in refused.items():
        assert reason in WeightOnlyMLP.refusal(*parts)
        with pytest.raises(ValueError, match=reason):
            WeightOnlyMLP(*parts)


def test_predicate_reads_rows_alignment_and_the_weights_agreement():
    from quantool_amd.hip import ops

    x = lambda M, K=1024: torch.zeros(M, K, dtype=torch.bfloat16)   # noqa: E731
    w = (_w4(8, 1024), torch.ones(8, 8), None, None)
    assert ops.gemm_wq_fused_supported(x(1), [w, w]) and ops.gemm_wq_fused_supported(x(16), [w] * 4)
    for X, ws in ((x(17), [w]), (x(0), [w]), (x(4), [w] * 5), (x(4), []), (x(4, 1024)[:, :130], [w]),
                  (x(4), [w, (w[0], torch.ones(8, 1), None, None)]),
                  (x(4), [w, (w[0], w[1], torch.zeros(8, 8, dtype=torch.int8), None)]),
                  (x(4), [w, (torch.zeros(8, 1024, dtype=torch.int8), w[1], None, None)]),
                  (x(4), [(w[0], w[1], None, torch.zeros(1024, dtype=torch.int32))])):
        assert not ops.gemm_wq_fused_supported(X, ws)


def test_hand_off_is_for_the_very_tensor_unwritten(monkeypatch):
    from quantool_amd.engine.qlinear import SharedOutputs

    q, k, v = _linear(256, 128, 0), _linear(128, 128, 1), _linear(128, 128, 2)
    shared = SharedOutputs((q, k, v))
    assert q.outputs_from is k.outputs_from is v.outputs_from is shared
    runs = []

    def run(x):
        runs.append(x)
        return [torch.full((1,), float(10 * len(runs) + i)) for i in range(3)]

    monkeypatch.setattr(shared, "_run", run)
    x = torch.zeros(1, 128, dtype=torch.bfloat16)
    assert [shared.take(m, x).item() for m in (q, k, v)] == [10, 11, 12] and len(runs) == 1
    assert not shared.holds_tensors                           # after the last consumer nothing is pinned
    assert shared.take(q, x).item() == 20 and shared.take(k, x.clone()).item() == 31      # a different tensor
    x2 = runs[-1]
    x2.add_(1)                                                # the same tensor after an in-place write
    assert shared.take(v, x2).item() == 42 and len(runs) == 4
    monkeypatch.setattr(shared, "_run", lambda x: None)       # the launch does not apply: everyone computes for itself
    assert shared.take(q, x) is None and not shared.holds_tensors
    assert "two to four" in SharedOutputs.refusal((q,))
    assert "differ in" in SharedOutputs.refusal((q, _linear(128, 256, 3)))
