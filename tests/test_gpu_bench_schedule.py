"""What `bench.quantize_layer` returns under the schedule `bench.py` times -- 2-3 decoder layers in flight on separate
stream sets ("lanes"), a Gram stream per lane, batched chains behind events, `record_stream` hand-offs, per-stream
workspaces and per-(lane, slot) accumulators -- against a one-stream reference, bit for bit.

Every kernel on the path is deterministic and a batched chain is bit-identical to a single one
(tests/test_gpu_batched_chains.py), so there is no tolerance to choose: `torch.equal`.

The benchmark itself feeds identical data to every step, so a kernel that reads a buffer one step too early, or an
allocator block recycled too soon, finds the previous step's bit-identical values there.  Here two DIFFERENT datasets A
and B alternate so that consecutive steps of one lane never get the same one: whatever a lane's streams, workspaces,
cached accumulators or recycled blocks still hold from its previous step is wrong data for this one.

The reference is formed without `quantize_layer`: per group a fresh `HessianAccumulator`, one `add`, then
`gptq_quantize_shared`, all on the current stream.  Widths are 1/16 of the models' (hidden 256, intermediate 896,
kv 128), which keeps every group's row count a multiple of 128; a race whose window only opens at full width is out of
this test's sight."""
import importlib.util
import os
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SCALE = 16

# name -> (model, samples, actorder, per_sample).  48 samples x 384 tokens = 18 432 >= DIRECT_TOKENS: one direct Gram launch
# per Llama group, as in the benchmark.  At 48 samples a Mixtral expert sees ~4 600 routed tokens, which the accumulator
# STAGES; at 192 samples ~18 400, a direct launch -- the route the benchmark's experts take (~49 000 tokens each).
WORKLOADS = {
    "llama-static": ("llama-3-8b", 48, "static", False),
    "llama-none": ("llama-3-8b", 48, "none", False),
    "llama-per-sample": ("llama-3-8b", 16, "static", True),
    "mixtral": ("mixtral-8x7b", 48, "static", False),
    "mixtral-direct": ("mixtral-8x7b", 192, "static", False),
}

# bench.py:175 evaluates `acc.G` -- a property that flushes staged tokens through the Gram kernel on the CURRENT stream --
# outside `with torch.cuda.stream(st)`, i.e. on the caller's stream, which has waited neither for the Gram stream's staging
# copies nor is waited for by the chain stream.  The benchmark's own sizes never stage on the Gram stream (every launch is
# direct), so its numbers are unaffected; at 48 samples the experts' ~4 600 tokens are staged.
MIXTRAL_STAGED_XFAIL = pytest.mark.xfail(strict=False, reason=(
    "bench.py:175 (`for t in [acc.G] + ...` in run_chains) reads the flushing property `acc.G` with the caller's stream "
    "current: with the Gram sums on the lane's Gram stream (`accumulate` only calls `acc.add`, no flush, bench.py:100) an "
    "expert's < DIRECT_TOKENS routed tokens are still staged, so their Gram launch is issued on the caller's stream, which "
    "never waited for the staging copies on the Gram stream, and the chain stream never waits for that launch: the case "
    "passes when the Gram stream happens to have drained by then (it did when this test was written) and nothing enforces "
    "that, e.g. when the Gram stream shares a hardware queue with another lane's chain. "
    "bench.py cannot change in this pull request; the benchmark's sizes (>= 16 384 tokens per expert) never stage there: "
    "test_concurrent_lanes_mixtral_direct_launches covers that route"))


def _load_bench(monkeypatch):
    """A fresh bench module (empty `_STREAMS` / `_ACCS`) with none of its environment knobs set."""
    for k in list(os.environ):
        if k.startswith("QT_BENCH_") or k in ("QT_BATCH_CHAINS", "QT_XTX_LAUNCH_TOKENS"):
            monkeypatch.delenv(k)
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert not mod._STREAMS and not mod._ACCS and mod.BATCH_CHAINS and not mod.SKIP
    return mod


def _shape(model):
    from quantool_amd.engine.model_shapes import MODEL_SHAPES, scaled

    return scaled(MODEL_SHAPES[model], SCALE)


def _qargs(actorder):
    from quantool_amd.engine.schemes import QuantArgs

    return QuantArgs(num_bits=4, symmetric=True, group_size=128, actorder=None if actorder == "none" else actorder)


def _dataset(bench, model, shape, samples, dev, which):
    """What `bench.main()` builds between "weights, acts, smooth = {}, {}, None" and its first synchronise, with
    `1000 * which` in the place of main's `1000 * rank` in every seed (and in the smoothing vector's, which main() does
    not vary): which = 0 / 1 are two different datasets of the same shapes."""
    off = 1000 * which
    n_tokens = samples * bench.SEQ_LEN
    weights, acts, smooth, route_counts = {}, {}, None, None
    if model == "mixtral-8x7b":
        g = torch.Generator(device=dev)
        g.manual_seed(7 + off)
        top2 = torch.randn((n_tokens, 8), generator=g, device=dev).topk(2, dim=1).indices
        route = [torch.nonzero((top2 == e).any(dim=1)).flatten() for e in range(8)]
        route_counts = [int(r.numel()) for r in route]
        x_moe = bench.synth_activations(n_tokens, shape.groups[0][1], seed=5 + off, device=dev)
    for gi, (gname, K, lins) in enumerate(shape.groups):
        if gname.startswith("expert"):
            e = int(gname[len("expert"):].split("_")[0])
            if gname.endswith("_in"):
                acts[gname] = x_moe[route[e]].contiguous()
            else:
                acts[gname] = bench.synth_activations(route_counts[e], K, seed=2 + 17 * gi + off, device=dev)
        else:
            acts[gname] = bench.synth_activations(n_tokens, K, seed=2 + 17 * gi + off, device=dev)
        for li, (lname, R) in enumerate(lins):
            weights[lname] = bench.synth_weight(R, K, seed=100 * gi + li + off, device=dev)
    if model == "mixtral-8x7b":
        g = torch.Generator(device=dev)
        g.manual_seed(11 + off)
        smooth = {"attn_in": (1.0 + 0.1 * torch.randn(shape.groups[0][1], generator=g, device=dev)).to(torch.bfloat16)}
    torch.cuda.synchronize()
    return SimpleNamespace(weights=weights, acts=acts, smooth=smooth, route_counts=route_counts)


def _reference(bench, shape, data, qargs, samples, dev):
    """Independent of `quantize_layer`: group by group on the current stream; CPU clones of every packed / scale tensor."""
    from quantool_amd.engine.gptq_linear import HessianAccumulator, gptq_quantize_shared

    ref = {}
    for gname, K, lins in shape.groups:
        X, wts = data.acts[gname], data.weights
        if data.smooth and gname in data.smooth:
            wts, X = bench.smooth_group(lins, data.weights, X, data.smooth[gname])
        acc = HessianAccumulator(K, dev)
        acc.add(X, num_samples=samples)
        for (lname, _), r in zip(lins, gptq_quantize_shared([wts[n] for n, _ in lins], acc, qargs)):
            ref[f"{lname}.weight_packed"] = r.weight_packed.cpu().clone()
            ref[f"{lname}.weight_scale"] = r.weight_scale.cpu().clone()
    torch.cuda.synchronize()
    return ref


@pytest.fixture(scope="module")
def workloads():
    """name -> (shape, qargs, samples, per_sample, [data A, data B], [reference A, reference B]); built once per name,
    never modified."""
    cache = {}

    def get(bench, name, dev):
        if name not in cache:
            model, samples, actorder, per_sample = WORKLOADS[name]
            shape, qargs = _shape(model), _qargs(actorder)
            data = [_dataset(bench, model, shape, samples, dev, which) for which in (0, 1)]
            refs = [_reference(bench, shape, d, qargs, samples, dev) for d in data]
            # preconditions: the two datasets must give different words for EVERY Linear, or a stale read of the other
            # dataset could pass
            assert set(refs[0]) == set(refs[1]) == {f"{n}.{s}" for _, _, lins in shape.groups for n, _ in lins
                                                    for s in ("weight_packed", "weight_scale")}
            for k in refs[0]:
                if k.endswith(".weight_packed"):
                    assert not torch.equal(refs[0][k], refs[1][k]), f"{name}: datasets A and B give the same {k}"
            cache[name] = (shape, qargs, samples, per_sample, data, refs)
        return cache[name]

    yield get
    cache.clear()


def _describe(got, want, other):
    """What the next engineer needs to localise a mismatch without another GPU run."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {tuple(got.shape)} {got.dtype}, expected {tuple(want.shape)} {want.dtype}"
    diff = got != want
    if got.dtype.is_floating_point:
        diff = diff & ~(torch.isnan(got) & torch.isnan(want))
        bad_pattern = f"{int(torch.isnan(got).sum())} NaN"
    else:
        bad_pattern = f"{int((got == -1).sum())} all-ones words"
    if not bool(diff.any()):
        return f"differs only where both hold NaN; contains {bad_pattern}"
    rows = torch.nonzero(diff.any(dim=1)).flatten()
    cols = torch.nonzero(diff.any(dim=0)).flatten()
    stale =other is not None and got.shape == other.shape and torch.equal(got, other)
    return (f"{int(diff.sum())} of {got.numel()} elements differ (rows {int(rows[0])}..{int(rows[-1])}, {rows.numel()} rows; "
            f"columns {int(cols[0])}..{int(cols[-1])}); equals the OTHER dataset's reference (stale read): {stale}; "
            f"contains {bad_pattern}")


def _mismatches(outs, ref, other, where):
    bad = []
    if set(outs) != set(ref):
        bad.append(f"{where}: key set differs: missing {sorted(set(ref) - set(outs))}, unexpected {sorted(set(outs) - set(ref))}")
    for k in sorted(set(outs) & set(ref)):
        got = outs[k].cpu()
        if not torch.equal(got, ref[k]):
            bad.append(f"{where}, {k}: {_describe(got, ref[k], other.get(k))}")
    return bad


def _report(bad):
    assert not bad, f"{len(bad)} tensors differ from the one-stream reference:\n" + "\n".join(bad[:60])


def _dataset_of(i, L):
    # consecutive steps of ONE lane (i, i + L, i + 2L, ...) must never get the same dataset.  With an odd number of lanes
    # i % 2 does that; with an even number i % 2 would tie every lane to one dataset, so the dataset changes once per round
    # of L steps instead.
    return i % 2 if L % 2 else (i // L) % 2


def _expected_streams(bench, dev, L, xmode, n_chain_streams):
    """Keys `_STREAMS` must hold after a concurrent run: the Gram stream(s) of the policy and the chain streams of every lane."""
    if xmode == "lane":
        gram = {(dev.index, "xtx", lane) for lane in range(L)}
    elif xmode == "shared":
        gram = {(dev.index, "xtx")}
    else:               # "group": by design no Gram stream exists; every Gram sum runs on its group's chain stream
        gram = set()
    return gram, {(dev.index, lane, slot) for lane in range(L) for slot in range(n_chain_streams)}


def _run_concurrent(bench, wl, dev, L, xmode="lane", n_chain_streams=1, drop=False):
    """The set-up steps and 2 L further steps as `main()` drives them: step i on lane i % L, no host synchronisation
    between steps, one join and one device synchronise at the end; then EVERY kept step against its dataset's reference."""
    shape, qargs, samples, per_sample, data, refs = wl
    n_steps = L + 2 * L
    for lane in range(L):
        seq = [_dataset_of(i, L) for i in range(lane, n_steps, L)]
        assert all(a != b for a, b in zip(seq, seq[1:])), (lane, seq)
    kept = {}
    for i in range(n_steps):
        d = data[_dataset_of(i, L)]
        kept[i] = bench.quantize_layer(shape, d.weights, d.acts, qargs, samples, overlap=True, lane=i % L,
                                       per_sample=per_sample, smooth=d.smooth)
        if drop and i - L in kept:
            # the outputs of the lane's previous step go back to its side streams' pools while later steps still run
            del kept[i - L]
    bench.join_streams(dev)
    torch.cuda.synchronize()
    if drop:
        assert sorted(kept) == list(range(n_steps - L, n_steps))
    # the run must have been a concurrent one: a Gram stream (where the policy has one) and chain streams on every lane
    gram, chains = _expected_streams(bench, dev, L, xmode, n_chain_streams)
    have = set(bench._STREAMS)
    assert gram <= have and chains <= have, f"streams {sorted(map(str, have))}"
    assert {k for k in have if "xtx" in k} == gram, f"Gram streams {sorted(map(str, have))} for policy {xmode!r}"
    assert len({st.cuda_stream for st in bench._STREAMS.values()} | {torch.cuda.current_stream(dev).cuda_stream}) == len(have) + 1
    bad = []
    for i, outs in sorted(kept.items()):
        d = _dataset_of(i, L)
        bad += _mismatches(outs, refs[d], refs[1 - d], f"step {i} (lane {i % L}, dataset {'AB'[d]})")
    _report(bad)


@pytest.mark.parametrize("name", list(WORKLOADS))
def test_serial_run_equals_reference(dev, monkeypatch, workloads, name):
    """`quantize_layer(overlap=False)` -- the benchmark's own code on one stream -- equals the independent reference:
    until it does, the concurrent comparisons mean nothing."""
    bench = _load_bench(monkeypatch)
    shape, qargs, samples, per_sample, data, refs = workloads(bench, name, dev)
    if not per_sample and not name.startswith("mixtral"):
        from quantool_amd.engine.gptq_linear import HessianAccumulator

        assert samples * bench.SEQ_LEN >= HessianAccumulator.DIRECT_TOKENS      # one direct Gram launch per group
    outs = bench.quantize_layer(shape, data[0].weights, data[0].acts, qargs, samples, overlap=False,
                                per_sample=per_sample, smooth=data[0].smooth)
    torch.cuda.synchronize()
    assert not bench._STREAMS
    _report(_mismatches(outs, refs[0], refs[1], "serial run (dataset A)"))


@pytest.mark.parametrize("name", ["llama-static", "llama-none"])
def test_concurrent_lanes_direct_default_routes(dev, monkeypatch, workloads, name):
    """Three lanes, the default policy: a Gram stream per lane, the layer's two batched chains (K = 256: three groups,
    K = 896: one) on two chain streams behind events."""
    bench = _load_bench(monkeypatch)
    _run_concurrent(bench, workloads(bench, name, dev), dev, L=3, n_chain_streams=2)


@pytest.mark.parametrize("xmode", ["shared", "group"])
def test_concurrent_lanes_gram_stream_policies(dev, monkeypatch, workloads, xmode):
    """QT_BENCH_XTX_STREAM=shared: ONE Gram stream for all three layers in flight; =group: the Gram sum on its group's
    chain stream, into the cached per-(lane, slot) accumulator, a chain per group."""
    bench = _load_bench(monkeypatch)
    monkeypatch.setenv("QT_BENCH_XTX_STREAM", xmode)         # read at call time
    _run_concurrent(bench, workloads(bench, "llama-static", dev), dev, L=3, xmode=xmode,
                    n_chain_streams=2 if xmode == "shared" else 4)
    if xmode == "group":
        assert len(bench._ACCS) == 3 * 4


def test_concurrent_lanes_chain_per_group(dev, monkeypatch, workloads):
    """BATCH_CHAINS off: every group's chain on its own stream right behind its Gram sum (four chain streams per lane)."""
    bench = _load_bench(monkeypatch)
    monkeypatch.setattr(bench, "BATCH_CHAINS", False)
    _run_concurrent(bench, workloads(bench, "llama-static", dev), dev, L=3, n_chain_streams=4)


def test_concurrent_lanes_per_sample(dev, monkeypatch, workloads):
    """per_sample=True: 16 calls of 384 tokens per group staged into the token buffer of the cached `_ACCS`
    accumulators, which every later step of the lane `reset()`s and refills with the other dataset."""
    bench = _load_bench(monkeypatch)
    _run_concurrent(bench, workloads(bench, "llama-per-sample", dev), dev, L=3, xmode="group", n_chain_streams=4)
    assert len(bench._ACCS) == 3 * 4 and all(a._stage is not None for a in bench._ACCS.values())


@MIXTRAL_STAGED_XFAIL
def test_concurrent_lanes_mixtral(dev, monkeypatch, workloads):
    """Two lanes of a Mixtral layer: SmoothQuant on attn_in (rescaled weights cross from the Gram stream to the chain's),
    ragged routed token counts per expert, two batches of chains (ten groups of K = 256, eight of K = 896)."""
    bench = _load_bench(monkeypatch)
    wl = workloads(bench, "mixtral", dev)
    for d in wl[4]:
        assert len(set(d.route_counts)) > 1                                   # ragged
    _run_concurrent(bench, wl, dev, L=2, n_chain_streams=2)


def test_concurrent_lanes_mixtral_direct_launches(dev, monkeypatch, workloads):
    """The same with 192 samples: every expert's routed tokens are a direct Gram launch (>= DIRECT_TOKENS), the route the
    benchmark's own Mixtral layer takes (~49 000 tokens per expert)."""
    from quantool_amd.engine.gptq_linear import HessianAccumulator

    bench = _load_bench(monkeypatch)
    wl = workloads(bench, "mixtral-direct", dev)
    for d in wl[4]:
        assert len(set(d.route_counts)) > 1 and min(d.route_counts) >= HessianAccumulator.DIRECT_TOKENS
    _run_concurrent(bench, wl, dev, L=2, n_chain_streams=2)


def test_concurrent_lanes_dropped_outputs(dev, monkeypatch, workloads):
    """Each step's outputs are dropped as soon as the step L later has been issued -- their blocks go back to the side
    streams' pools while later steps still run -- and the last L steps are compared."""
    bench = _load_bench(monkeypatch)
    _run_concurrent(bench, workloads(bench, "llama-static", dev), dev, L=3, n_chain_streams=2, drop=True)
