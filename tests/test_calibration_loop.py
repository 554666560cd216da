"""engine/sequential.py:_calibrate_layer on the CPU -- which Linears share an input, batch 0's replay or its second
forward, early stop, routed experts -- against upstream's calling pattern: one forward per sample, a plain pre-hook on
every targeted Linear.  A float64 Gram sum stands in for the HIP accumulator."""
import logging

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from quantool_amd.engine import sequential as sq

H, I, T = 16, 24, 4


class FakeAccumulator:
    """HessianAccumulator's contract: G = sum of X^T X (here float64), ``n`` counted as ``add`` counts it."""

    def __init__(self, K, device=None):
        self.K, self.n = K, 0
        self.G = torch.zeros(K, K, dtype=torch.float64)

    def add(self, X, num_samples=None):
        if num_samples is None:
            num_samples = X.shape[0] if X.dim() == 3 else 1
        X2 = X.reshape(-1, self.K).double()
        self.G += X2.T @ X2
        self.n += int(num_samples)

    def flush(self):
        pass


class Counter(nn.Module):
    """Identity that counts its calls: did a forward get past the last hooked Linear?"""

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, x):
        self.calls += 1
        return x


@pytest.fixture(autouse=True)
def cpu_accumulator(monkeypatch):
    monkeypatch.setattr(sq, "HessianAccumulator", FakeAccumulator)
    monkeypatch.setattr(sq, "_CALIB_CTX", {"samples": 1, "tokens_per_sample": None})


def samples_of(n, seed, **kwargs):
    """``n`` one-sample cache entries ``((x [1, T, H],), kwargs)``; ``kwargs``: name -> one [1, T] tensor per sample."""
    g = torch.Generator().manual_seed(seed)
    return [((torch.randn(1, T, H, generator=g, dtype=torch.float64),), {k: v[i] for k, v in kwargs.items()})
            for i in range(n)]


def stacked(samples, sizes):
    """The driver's cache: consecutive samples concatenated along the batch dimension, ``sizes`` per forward."""
    out, i = [], 0
    for b in sizes:
        run, i = samples[i:i + b], i + b
        out.append(((torch.cat([a[0] for a, _ in run]),), {k: torch.cat([kw[k] for _, kw in run]) for k in run[0][1]}))
    assert i == len(samples)
    return out


def linears_of(layer):
    return {f"layer.{n}": m for n, m in layer.named_modules() if isinstance(m, nn.Linear)}


def calibrate(layer, samples, sizes):
    with torch.no_grad():
        return sq._calibrate_layer(layer, linears_of(layer), stacked(samples, sizes), 1, "cpu")


def assert_upstream(layer, leaders, accs, samples):
    """Every Linear's Gram sum and sample count, one forward per sample with a plain pre-hook on each, equal the ones
    of its group's accumulator."""
    linears = linears_of(layer)
    want = {n: FakeAccumulator(m.in_features) for n, m in linears.items()}
    hooks = [m.register_forward_pre_hook(lambda _m, a, n=n: want[n].add(a[0])) for n, m in linears.items()]
    with torch.no_grad():
        for args, kwargs in samples:
            sq._CALIB_CTX.update(samples=1, tokens_per_sample=None)
            layer(*args, **kwargs)
    for hk in hooks:
        hk.remove()
    assert sorted(n for names in leaders.values() for n in names) == sorted(linears)
    for lead, names in leaders.items():
        assert lead == names[0]
        for n in names:
            assert accs[lead].n == want[n].n, n
            torch.testing.assert_close(accs[lead].G, want[n].G, rtol=1e-10, atol=1e-10, msg=n)


def _lin(k, r):
    return nn.Linear(k, r, bias=False).double()


class LlamaLike(nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.norm1, self.norm2 = nn.LayerNorm(H).double(), nn.LayerNorm(H).double()
        self.q, self.k, self.v, self.o = _lin(H, H), _lin(H, H), _lin(H, H), _lin(H, H)
        self.gate, self.up, self.down = _lin(H, I), _lin(H, I), _lin(I, H)
        self.post = Counter()

    def forward(self, x):
        h = self.norm1(x)
        att = torch.softmax(self.q(h) @ self.k(h).transpose(-1, -2) / 4, dim=-1) @ self.v(h)
        x = x + self.o(att)
        h = self.norm2(x)
        return (self.post(x + self.down(F.silu(self.gate(h)) * self.up(h))),)


def test_llama_like_layer_groups_shared_inputs_and_stops_early():
    layer = LlamaLike()
    samples = samples_of(7, seed=1)
    leaders, accs = calibrate(layer, samples, (3, 2, 2))
    assert leaders == {"layer.q": ["layer.q", "layer.k", "layer.v"], "layer.o": ["layer.o"],
                       "layer.gate": ["layer.gate", "layer.up"], "layer.down": ["layer.down"]}
    assert layer.post.calls == 1        # batch 0's discovery forward only: batches 1 and 2 stopped at down's input
    assert_upstream(layer, leaders, accs, samples)


class CalledTwice(nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a, self.b = _lin(H, H), _lin(H, H)
        self.post = Counter()

    def forward(self, x):
        y = self.a(torch.tanh(self.a(x)))        # one weight, two call sites
        return (self.post(self.b(y)),)


def test_a_linear_called_twice_counts_both_calls_and_turns_early_stop_off():
    layer = CalledTwice()
    samples = samples_of(6, seed=2)
    leaders, accs = calibrate(layer, samples, (2, 2, 2))
    assert leaders == {"layer.a": ["layer.a"], "layer.b": ["layer.b"]}
    assert accs["layer.a"].n == 2 * len(samples)
    assert layer.post.calls == 3        # every forward ran to its end
    assert_upstream(layer, leaders, accs, samples)


class WritesInPlace(nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a, self.b = _lin(H, H), _lin(H, H)
        self.post = Counter()

    def forward(self, x):
        h = x * 1.5
        y = self.a(h)
        h.add_(1)                                # what a read is gone once the forward is over
        return (self.post(self.b(y + h)),)


def test_an_input_written_in_place_forwards_batch_0_again(caplog):
    layer = WritesInPlace()
    samples = samples_of(6, seed=3)
    with caplog.at_level(logging.INFO, logger=sq.__name__):
        leaders, accs = calibrate(layer, samples, (3, 2, 1))
    assert "batch 0 is forwarded twice" in caplog.text
    assert leaders == {"layer.a": ["layer.a"], "layer.b": ["layer.b"]}
    assert layer.post.calls == 1        # discovery; the three hooked forwards (batch 0 again, 1, 2) stop at b
    assert_upstream(layer, leaders, accs, samples)


class FusedExperts(nn.Module):
    """A fused expert bank as transformers >= 5 keeps it: what ``_UnfusedExperts`` takes apart."""

    def __init__(self, E):
        super().__init__()
        self.gate_up_proj = nn.Parameter(torch.randn(E, 2 * I, H, dtype=torch.float64) * 0.3)
        self.down_proj = nn.Parameter(torch.randn(E, H, I, dtype=torch.float64) * 0.3)
        self.act_fn = F.silu


class RoutedExperts(nn.Module):
    """Top-1 routing over a fixed table: ``route [B, T]`` names each token's expert."""

    def __init__(self, E=4):
        super().__init__()
        torch.manual_seed(0)
        self.proj = _lin(H, H)
        self.experts = sq._UnfusedExperts(FusedExperts(E))
        self.post = Counter()

    def forward(self, x, route):
        B = x.shape[0]
        h = self.proj(x).reshape(B * T, H)
        out = self.experts(h, route.reshape(B * T, 1), torch.ones(B * T, 1, dtype=x.dtype))
        return (self.post(x + out.reshape(B, T, H)),)


def test_routed_experts_count_the_samples_that_reach_them():
    routes = [[0, 1, 2, 0], [0, 2, 2, 0], [1, 0, 2, 1],     # batch 0: sample 1 routes nothing to expert 1, none reach 3
              [0, 3, 1, 3], [1, 0, 0, 1],                   # batch 1: no token for expert 2
              [0, 1, 2, 3], [3, 2, 1, 0]]                   # batch 2
    route = torch.tensor(routes).reshape(len(routes), 1, T)
    layer = RoutedExperts()
    samples = samples_of(len(routes), seed=4, route=route)
    leaders, accs = calibrate(layer, samples, (3, 2, 2))
    e = "layer.experts.experts.{}.{}".format
    # one sample per forward counts expert 1 in six samples: two of batch 0, not three (its forward's B)
    assert accs[e(1, "gate_up_proj")].n == accs[e(1, "down_proj")].n == 6
    assert accs[e(3, "gate_up_proj")].n == 3 and leaders[e(3, "gate_up_proj")] == [e(3, "gate_up_proj")]   # solo
    assert accs[e(2, "down_proj")].n == 5
    assert layer.post.calls == 3        # expert 3 was not called in batch 0: no early stop
    assert_upstream(layer, leaders, accs, samples)
