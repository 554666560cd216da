"""The streamed placement of the sequential driver on the CPU: the resident / streamed decision against the shapes of
real models, the order of the copies against the per-layer stages (fakes of both), that tied weights and the views of an
unfused expert bank keep pointing at the caller's host storage, and the refusal under several ranks."""
import pytest
import torch
import torch.nn as nn

from quantool_amd.engine import placement, sequential
from quantool_amd.engine.model_shapes import LARGE_MODEL_SHAPES, MODEL_SHAPES
from quantool_amd.engine.schemes import QuantArgs

GB, GiB = 10 ** 9, 2 ** 30
W4 = QuantArgs()                                             # W4A16 g128, as tools/full_model.py runs it
TOKENS = 512 * 384

# (shape, hidden, vocab, measured peak of the resident run in GiB or None) -- profiles/r04_full_model.txt
MODELS = {
    "llama-3-8b": (MODEL_SHAPES["llama-3-8b"], 4096, 128256, 35.5),
    "llama-3-70b": (MODEL_SHAPES["llama-3-70b"], 8192, 128256, 204.4),
    "mixtral-8x7b": (MODEL_SHAPES["mixtral-8x7b"], 4096, 32000, 175.3),
    "mixtral-8x22b": (LARGE_MODEL_SHAPES["mixtral-8x22b"], 6144, 32768, None),
    "llama-3.1-405b": (LARGE_MODEL_SHAPES["llama-3.1-405b"], 16384, 128256, None),
}


def param_bytes(name):
    shape, hidden, vocab, _ = MODELS[name]
    norms = shape.n_layers * 2 * hidden + hidden
    return 2 * (shape.total_weights + 2 * vocab * hidden + norms)


def decide(name, free=288 * GB, on_host=True):
    shape, hidden, _, _ = MODELS[name]
    return placement.should_stream(shape, hidden, param_bytes(name), W4, TOKENS, free, on_host=on_host)


@pytest.mark.parametrize("name,streamed", [("llama-3-8b", False), ("llama-3-70b", False), ("mixtral-8x7b", False),
                                           ("mixtral-8x22b", True), ("llama-3.1-405b", True)])
def test_real_model_shapes_on_one_mi355x(name, streamed):
    assert decide(name) is streamed


@pytest.mark.parametrize("name", ["llama-3-8b", "llama-3-70b", "mixtral-8x7b"])
def test_estimate_is_not_below_the_measured_resident_peak(name):
    shape, hidden, _, peak = MODELS[name]
    est = param_bytes(name) + placement.calibration_bytes(shape, hidden, TOKENS, W4)
    assert est >= peak * GiB, f"{name}: estimate {est / GiB:.1f} GiB below the measured {peak} GiB"


def test_host_model_streams_only_when_it_does_not_fit():
    shape, hidden, _, _ = MODELS["llama-3-8b"]
    need = param_bytes("llama-3-8b") + placement.calibration_bytes(shape, hidden, TOKENS, W4)
    assert decide("llama-3-8b", free=need + 1) is False             # fits: resident
    assert decide("llama-3-8b", free=need - 1) is True              # does not: streamed
    assert decide("llama-3-8b", free=need // 4, on_host=False) is False    # a model on the device stays there
    assert decide("llama-3.1-405b", free=288 * GB, on_host=False) is False


def test_estimate_terms_scale_with_tokens_and_results():
    shape, hidden, _, _ = MODELS["llama-3-8b"]
    a = placement.calibration_bytes(shape, hidden, TOKENS, W4)
    b = placement.calibration_bytes(shape, hidden, 2 * TOKENS, W4)
    assert b - a == 2 * TOKENS * hidden * 2             # one more cache pair's worth; the forwards stay 32768 tokens
    streamed = placement.calibration_bytes(shape, hidden, TOKENS, W4, with_results=False)
    assert a - streamed == placement.result_bytes(shape.total_weights, W4)
    w8 = placement.result_bytes(shape.total_weights, QuantArgs(num_bits=8, strategy="channel", group_size=None))
    assert w8 > placement.result_bytes(shape.total_weights, W4)


class TinyBlock(nn.Module):
    def __init__(self, h=8):
        super().__init__()
        self.norm = nn.LayerNorm(h)
        self.lin = nn.Linear(h, h, bias=False)
        self.register_buffer("inv_freq", torch.arange(4.0))


class Tiny(nn.Module):
    def __init__(self, n=4, h=8, v=16):
        super().__init__()
        self.embed = nn.Embedding(v, h)
        self.layers = nn.ModuleList(TinyBlock(h) for _ in range(n))
        self.head = nn.Linear(h, v, bias=False)
        self.head.weight = self.embed.weight                      # tied
        self.register_buffer("rope", torch.ones(3))


def test_layer_shape_of_a_live_model_counts_linears_and_fused_experts():
    m = Tiny()
    s = placement.layer_shape(list(m.layers))
    assert s.n_layers == 4 and [(K, [R for _, R in lins]) for _, K, lins in s.groups] == [(8, [8])]

    class Fused(nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_up_proj = nn.Parameter(torch.zeros(3, 2 * 5, 8))
            self.down_proj = nn.Parameter(torch.zeros(3, 8, 5))
            self.act_fn = nn.SiLU()

    blk = nn.Module()
    blk.experts = Fused()
    s = placement.layer_shape([blk])
    assert sorted((K, lins[0][1]) for _, K, lins in s.groups) == sorted([(8, 10), (5, 8)] * 3)


def test_outside_modules_visit_and_leave_with_ties_kept():
    m = Tiny()
    emb_host, rope_host = m.embed.weight.data, m.rope
    lin_ptr = m.layers[0].lin.weight.data_ptr()
    with placement.outside_layers_on_device(m, list(m.layers), "cpu"):     # a copy stands in for the device's
        assert m.embed.weight.data_ptr() != emb_host.data_ptr() and m.head.weight is m.embed.weight
        assert m.rope is not rope_host and torch.equal(m.rope, rope_host)
        assert m.layers[0].lin.weight.data_ptr() == lin_ptr             # the layers stay where they are
    assert m.head.weight is m.embed.weight
    assert m.embed.weight.data.data_ptr() == emb_host.data_ptr() and m.rope is rope_host


class FakeMover:
    """LayerMover's interface on the CPU: a "device" copy is a clone, the write-back copies into the host tensors
    through ``_pieces`` over small chunks, as the real one does through its staging."""

    CHUNK = 96

    def __init__(self, layers, log):
        self.layers, self.log = layers, log
        self.slots, self.host, self.devt, self.resident, self.peak = {}, {}, {}, set(), 0

    def stage(self, i):
        self.log.append(("stage", i))
        self.slots[i] = placement._slots(self.layers[i])
        self.host[i] = [s[0].data if isinstance(s[0], nn.Parameter) else s[0] for s in self.slots[i]]

    def upload(self, i):
        self.log.append(("upload", i))
        self.devt[i] = [h.clone() for h in self.host[i]]
        self.resident.add(i)
        self.peak = max(self.peak, len(self.resident))

    def attach(self, i):
        self.log.append(("attach", i))
        for s, d in zip(self.slots[i], self.devt[i]):
            placement._point(s, d)

    def writeback(self, i, results=()):
        self.log.append(("writeback", i))
        src, dst = self.devt[i], self.host[i]
        sizes = [d.numel() * d.element_size() for d in dst]
        stage = [torch.empty(self.CHUNK, dtype=torch.uint8) for _ in range(placement._span(sizes, self.CHUNK)
                                                                             // self.CHUNK + 1)]
        fs, fd = [placement._flat(s) for s in src], [placement._flat(d) for d in dst]
        for t, off, c, co, k in placement._pieces(sizes, self.CHUNK):
            stage[c][co:co + k].copy_(fs[t][off:off + k])
        for t, off, c, co, k in placement._pieces(sizes, self.CHUNK):
            fd[t][off:off + k].copy_(stage[c][co:co + k])

    def release(self, i):
        self.log.append(("release", i))
        for s, h in zip(self.slots.pop(i), self.host.pop(i)):
            placement._point(s, h)
        del self.devt[i]
        self.resident.discard(i)

    def finish(self):
        self.log.append(("finish",))


def run_streamed(layers, quantize_body=lambda i, layer: None):
    log = []
    mover = FakeMover(layers, log)
    results = {}

    def quantize(i, between):
        log.append(("quantize-start", i))
        for s in placement._slots(layers[i]):
            assert s[0].data_ptr() in {d.data_ptr() for d in mover.devt[i]}, "layer not attached"
        between()
        quantize_body(i, layers[i])
        results[f"l{i}"] = object.__new__(type("R", (), {}))
        log.append(("quantize-end", i))

    def propagate(i):
        log.append(("propagate", i))

    sequential._stream_layers(len(layers), mover, quantize, propagate, results)
    return log, mover


def test_schedule_order_and_two_layers_at_most():
    m = Tiny(n=5)
    log, mover = run_streamed(list(m.layers))
    at = {e: k for k, e in enumerate(log)}
    n = len(m.layers)
    for i in range(n):
        if i + 1 < n:
            assert at[("upload", i + 1)] < at[("quantize-end", i)]          # next layer's onload before quantise ends
            assert at[("writeback", i)] > at[("propagate", i)]              # write-back behind the propagate
            assert at[("release", i)] < at[("attach", i + 1)] < at[("quantize-start", i + 1)]
        assert at[("quantize-start", i)] > at[("attach", i)]
        assert at[("release", i)] > at[("writeback", i)]
    assert ("propagate", n - 1) not in at
    assert mover.peak == 2 and log[-1] == ("finish",)


def test_round_trip_lands_in_the_callers_storage():
    from quantool_amd.engine.sequential import _UnfusedExperts

    class Fused(nn.Module):
        def __init__(self):
            super().__init__()
            self.gate_up_proj = nn.Parameter(torch.randn(3, 2 * 5, 8), requires_grad=False)
            self.down_proj = nn.Parameter(torch.randn(3, 8, 5), requires_grad=False)
            self.act_fn = nn.SiLU()

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.norm = nn.LayerNorm(8)
            self.experts = Fused()
            self.shared = nn.Linear(8, 8, bias=False)
            self.twin = nn.Linear(8, 8, bias=False)
            self.twin.weight = self.shared.weight                      # tied inside the layer

    layers = nn.ModuleList(Block() for _ in range(3))
    fused = [(b.experts.gate_up_proj, b.experts.down_proj) for b in layers]
    want = [(gu.data.clone(), dn.data.clone()) for gu, dn in fused]
    for b in layers:
        b.experts = _UnfusedExperts(b.experts)
    shared = [b.shared.weight for b in layers]
    ptrs = [b.shared.weight.data_ptr() for b in layers]

    def body(i, layer):                 # "quantise": every matrix changes on the device copy
        for e in layer.experts.experts:
            e.gate_up_proj.weight.data.add_(1.0)
            e.down_proj.weight.data.mul_(2.0)
        layer.shared.weight.data.fill_(float(i))
        layer.norm.weight.data.fill_(3.0)

    run_streamed(list(layers), body)
    for i, b in enumerate(layers):
        gu, dn = fused[i]
        assert torch.equal(gu.data, want[i][0] + 1.0) and torch.equal(dn.data, want[i][1] * 2.0)
        for e, ex in enumerate(b.experts.experts):          # still views of the caller's fused parameters
            assert ex.gate_up_proj.weight.data_ptr() == gu.data[e].data_ptr()
            assert ex.down_proj.weight.data_ptr() == dn.data[e].data_ptr()
        assert b.twin.weight is b.shared.weight is shared[i] and b.shared.weight.data_ptr() == ptrs[i]
        assert torch.equal(b.shared.weight.data, torch.full((8, 8), float(i)))
        assert torch.equal(b.norm.weight.data, torch.full((8,), 3.0))
        assert all(p.device.type == "cpu" for p in b.parameters())


def test_pieces_cover_every_byte_once_across_chunks():
    sizes = [5, 300, 0, 1, 97]
    seen = {i: [] for i in range(len(sizes))}
    for t, off, c, co, k in placement._pieces(sizes, 64):
        assert 0 < k <= 64 - co
        seen[t].append((off, k))
    for t, n in enumerate(sizes):
        covered = sorted(seen[t])
        assert sum(k for _, k in covered) == n
        assert all(a[0] + a[1] == b[0] for a, b in zip(covered, covered[1:]))


def test_several_ranks_refuse_to_stream_before_any_layer(monkeypatch):
    from quantool_amd.engine import sharding
    from quantool_amd.engine.modifiers import GPTQModifier

    m = Tiny()
    ran = []
    monkeypatch.setattr(sharding, "dist_world", lambda: (2, 0))
    monkeypatch.setattr(placement, "free_device_bytes", lambda dev: 1)             # nothing fits
    monkeypatch.setattr(sequential, "_first_layer_inputs", lambda *a, **k: ran.append("capture"))
    monkeypatch.setattr(sequential, "_calibrate_layer", lambda *a, **k: ran.append("calibrate"))
    monkeypatch.setattr(sequential, "awq_layer", lambda *a, **k: ran.append("awq"), raising=False)
    batches = [{"input_ids": torch.randint(0, 16, (1, 6))} for _ in range(4)]
    with pytest.raises(ValueError, match="streamed"):
        sequential.oneshot_module(m, None, GPTQModifier(targets="Linear", scheme="W4A16"), torch.device("cuda:0"),
                                  num_calibration_samples=4, max_seq_length=6, shuffle=False, dataloader=batches)
    assert ran == [] and m.embed.weight.device.type == "cpu"


def test_one_rank_and_a_model_that_fits_stays_resident(monkeypatch):
    from quantool_amd.engine.modifiers import GPTQModifier

    m = Tiny()
    monkeypatch.setattr(placement, "free_device_bytes", lambda dev: 1 << 50)
    qm = GPTQModifier(targets="Linear", scheme="W4A16")
    batches = [{"input_ids": torch.randint(0, 16, (1, 6))}]
    assert sequential._streams_layers(m, list(m.layers), qm, batches, "cpu") is False
    monkeypatch.setattr(placement, "free_device_bytes", lambda dev: 1)
    assert sequential._streams_layers(m, list(m.layers), qm, batches, "cpu") is True
