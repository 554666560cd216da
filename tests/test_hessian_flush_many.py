"""``HessianAccumulator.flush_many``: which accumulators go into one batched Gram launch and which are flushed alone
(host logic only: the Gram entry points are replaced by recorders, the accumulators live on the host)."""
import pytest
import torch

from quantool_amd.engine import gptq_linear as gl


@pytest.fixture
def calls(monkeypatch):
    """[("single" | "f32", K, dtype, rows)] and [("batched", [(K, dtype, rows), ...])] in call order"""
    log = []
    monkeypatch.setattr(gl.ops, "xtx_accumulate", lambda rows, G: log.append(("single", G.shape[0], rows.dtype, rows.shape[0])))
    monkeypatch.setattr(gl.ops, "xtx_accumulate_f32", lambda rows, G: log.append(("f32", G.shape[0], rows.dtype, rows.shape[0])))

    def batched(Xs, Gs):
        assert len(Xs) == len(Gs)
        log.append(("batched", [(G.shape[0], X.dtype, X.shape[0]) for X, G in zip(Xs, Gs)]))

    monkeypatch.setattr(gl.ops, "xtx_accumulate_batched", batched)
    monkeypatch.delenv("QT_XTX_LAUNCH_TOKENS", raising=False)
    monkeypatch.delenv("QT_FP32_ACTIVATIONS", raising=False)
    return log


def _acc(K, rows, dtype=torch.bfloat16, samples=1):
    acc = gl.HessianAccumulator(K, "cpu", stage_tokens=4096)
    if rows:
        acc.add(torch.ones(rows, K, dtype=dtype), num_samples=samples)
    return acc


def test_knob_off_is_the_loop(monkeypatch, calls):
    monkeypatch.delenv("QT_XTX_BATCHED", raising=False)
    accs = [_acc(512, 100), _acc(512, 200), _acc(1024, 70), _acc(512, 0)]
    gl.HessianAccumulator.flush_many(accs)
    assert calls == [("single", 512, torch.bfloat16, 100), ("single", 512, torch.bfloat16, 200),
                     ("single", 1024, torch.bfloat16, 70)]
    assert all(a._fill == 0 for a in accs)
    monkeypatch.setenv("QT_XTX_BATCHED", "0")
    accs = [_acc(512, 100), _acc(512, 200)]
    del calls[:]
    gl.HessianAccumulator.flush_many(accs)
    assert [c[0] for c in calls] == ["single", "single"]


def test_groups_by_k_and_dtype(monkeypatch, calls):
    monkeypatch.setenv("QT_XTX_BATCHED", "1")
    a = [_acc(512, 100), _acc(1024, 70), _acc(512, 200, torch.float16), _acc(512, 333), _acc(1024, 64),
         _acc(512, 50, torch.float16), _acc(512, 640)]
    gl.HessianAccumulator.flush_many(a)
    want = [("batched", [(512, torch.bfloat16, 100), (512, torch.bfloat16, 333), (512, torch.bfloat16, 640)]),
            ("batched", [(1024, torch.bfloat16, 70), (1024, torch.bfloat16, 64)]),
            ("batched", [(512, torch.float16, 200), (512, torch.float16, 50)])]
    assert len(calls) == 3 and all(w in calls for w in want)
    assert all(acc._fill == 0 and acc._staged_on is None for acc in a)


def test_singletons_fp32_and_empty_go_the_old_way(monkeypatch, calls):
    monkeypatch.setenv("QT_XTX_BATCHED", "1")
    lone = _acc(256, 90)                                    # the only member of its (K, dtype) group
    wide = [_acc(512, 100, torch.float32), _acc(512, 60, torch.float32)]        # fp32 accumulators: three-plane Gram
    empty = [_acc(512, 0), _acc(512, 0)]
    one_filled = _acc(512, 77)                              # its group's other members are empty: a singleton
    gl.HessianAccumulator.flush_many([lone, *wide, *empty, one_filled])
    assert calls == [("single", 256, torch.bfloat16, 90), ("f32", 512, torch.float32, 100),
                     ("f32", 512, torch.float32, 60), ("single", 512, torch.bfloat16, 77)]
    assert all(a._fill == 0 for a in [lone, *wide, *empty, one_filled])


def test_launch_token_limit_falls_back(monkeypatch, calls):
    """QT_XTX_LAUNCH_TOKENS would split a member's flush into several launches: the whole group is flushed alone, as
    today; a group it would not split is still batched."""
    monkeypatch.setenv("QT_XTX_BATCHED", "1")
    monkeypatch.setenv("QT_XTX_LAUNCH_TOKENS", "128")
    accs = [_acc(512, 100), _acc(512, 300), _acc(1024, 64), _acc(1024, 128)]
    gl.HessianAccumulator.flush_many(accs)
    assert calls == [("single", 512, torch.bfloat16, 100), ("single", 512, torch.bfloat16, 128),
                     ("single", 512, torch.bfloat16, 128), ("single", 512, torch.bfloat16, 44),
                     ("batched", [(1024, torch.bfloat16, 64), (1024, torch.bfloat16, 128)])]


def test_runs_of_at_most_16(monkeypatch, calls):
    monkeypatch.setenv("QT_XTX_BATCHED", "1")
    accs = [_acc(512, 64 + i) for i in range(35)]
    gl.HessianAccumulator.flush_many(accs)
    sizes = [len(c[1]) for c in calls if c[0] == "batched"]
    assert sizes == [16, 16, 3]
    accs = [_acc(512, 64 + i) for i in range(17)]
    del calls[:]
    gl.HessianAccumulator.flush_many(accs)
    assert [c[0] for c in calls] == ["batched", "single"] and len(calls[0][1]) == 16 and calls[1][3] == 64 + 16


@pytest.mark.parametrize("knob", ["0", "1"])
def test_n_and_fill_end_as_after_flush(monkeypatch, calls, knob):
    monkeypatch.setenv("QT_XTX_BATCHED", knob)
    shapes = [(512, 100, 3), (512, 200, 1), (1024, 70, 2), (512, 0, 0)]
    many = [_acc(K, rows, samples=s) for K, rows, s in shapes]
    alone = [_acc(K, rows, samples=s) for K, rows, s in shapes]
    gl.HessianAccumulator.flush_many(iter(many))           # any iterable, e.g. dict.values()
    for a in alone:
        a.flush()
    for m, a in zip(many, alone):
        assert (m.n, m._fill, m._staged_on, m.dtype) == (a.n, a._fill, a._staged_on, a.dtype)
    del calls[:]
    gl.HessianAccumulator.flush_many(many)                   # nothing staged: nothing launched
    assert calls == []
