"""``HessianAccumulator.flush_many`` on the device: three accumulators of K = 512 and one of K = 1024, fed ragged batches
of exactly summable tokens on a side stream, flushed together on the caller's stream and read on a third.  With
``QT_XTX_BATCHED=1`` G and n must be bit-equal to per-accumulator ``flush()``: the inputs are integers whose every
partial sum is exact in fp32, so the different grouping of the batched launch cannot change a bit -- only a token that
is lost, doubled, added to another accumulator, or read before its staging copy has landed can."""
import pytest
import torch

from tests import exact_inputs as ex

pytestmark = pytest.mark.gpu

# (K, ragged batch lengths): each accumulator ends with a token count that is no multiple of 64
FEED = [(512, [100, 384, 37]), (512, [384, 384, 384, 90]), (512, [65]), (1024, [200, 129])]


def _batches(dev):
    out = []
    for a, (K, lens) in enumerate(FEED):
        xs = [torch.from_numpy(ex.dense_ints((n, K), seed=100 * a + i)).to(torch.bfloat16).to(dev)
              for i, n in enumerate(lens)]
        total = torch.cat(xs).double().abs()
        ex.assert_exactly_summable(total.t() @ total, 0, f"accumulator {a}")
        out.append(xs)
    return out


@pytest.mark.parametrize("knob", ["1", "0"])
def test_flush_many_equals_flushing_each(dev, monkeypatch, knob):
    from quantool_amd.engine.gptq_linear import HessianAccumulator

    monkeypatch.delenv("QT_XTX_LAUNCH_TOKENS", raising=False)
    batches = _batches(dev)
    monkeypatch.setenv("QT_XTX_BATCHED", "0")
    want = []
    for (K, _), xs in zip(FEED, batches):
        ref = HessianAccumulator(K, dev)
        for x in xs:
            ref.add(x, num_samples=1)
        ref.flush()
        want.append((ref.G.clone(), ref.n))
    torch.cuda.synchronize()

    monkeypatch.setenv("QT_XTX_BATCHED", knob)
    staging, reader = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    a = torch.ones(2048, 2048, dtype=torch.bfloat16, device=dev)
    accs = [HessianAccumulator(K, dev) for K, _ in FEED]
    torch.cuda.synchronize()
    with torch.cuda.stream(staging):
        for _ in range(50):
            keep = a @ a                                  # the staging copies queue behind these products
        for acc, xs in zip(accs, batches):
            for x in xs:
                acc.add(x, num_samples=1)
    assert all(acc._fill for acc in accs), "every batch is short enough to be staged"
    HessianAccumulator.flush_many(accs)                   # on the caller's stream
    assert all(acc._fill == 0 and acc._flushed is not None for acc in accs)
    if knob == "1":
        assert accs[0]._flushed[1] is accs[1]._flushed[1] is accs[2]._flushed[1], "one launch, one event"
        assert accs[3]._flushed[1] is not accs[0]._flushed[1], "K = 1024 is alone in its group"
    with torch.cuda.stream(reader):
        got = [acc.G.clone() for acc in accs]             # a third stream: must wait for the shared launch
    torch.cuda.synchronize()
    del keep
    for i, (acc, g, (w, n)) in enumerate(zip(accs, got, want)):
        assert acc.n == n
        lower, _ = ex.gram_masks(acc.K, dev)
        ex.assert_exact(g, w, region=lower, what=f"accumulator {i} (K = {acc.K}), QT_XTX_BATCHED={knob}", gram=True)
        x64 = torch.cat(batches[i]).double()
        ex.assert_exact(g, x64.t() @ x64, region=lower, what=f"accumulator {i} against the integer Gram", gram=True)
