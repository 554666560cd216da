"""``HessianAccumulator`` across streams: tokens staged on one stream, ``G`` first read (so the staged tokens flushed) on
a second, the sum consumed on a third, and more tokens staged while that flush may still be reading the buffer.  The
flush's Gram launch is the one launch a caller cannot order, because it does not see it; a stream is held busy with
large products so that nothing here comes out right by luck."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K, TOKENS = 256, 1000


def _tokens(dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(TOKENS, K, generator=g).to(torch.bfloat16).to(dev)


@pytest.fixture(scope="module")
def busy(dev):
    """busy(): some tens of milliseconds of products on the current stream (300 x 4096^3 in bf16 into one output).  The
    two 32 MiB buffers go back to the driver afterwards, so that later tests find the allocator's pool as it was."""
    a = torch.ones(4096, 4096, dtype=torch.bfloat16, device=dev)
    out = torch.empty_like(a)

    def run():
        for _ in range(300):
            torch.mm(a, a, out=out)
        return out

    yield run
    torch.cuda.synchronize()
    del a, out, run
    torch.cuda.empty_cache()


def test_a_flush_on_another_stream_sees_the_staged_tokens(dev, busy):
    from quantool_amd.engine.gptq_linear import HessianAccumulator

    X = _tokens(dev, 1)
    ref = HessianAccumulator(K, dev)
    ref.add(X, num_samples=1)
    want = ref.G.clone()
    torch.cuda.synchronize()
    assert bool(want.any())

    staging, consumer = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    with torch.cuda.stream(staging):
        keep = busy()                                    # the staging copy queues behind this
        acc = HessianAccumulator(K, dev)
        acc.add(X, num_samples=1)                        # short: staged, not launched
    acc.G                                                # flushes on the caller's stream, as a reader outside the block does
    with torch.cuda.stream(consumer):
        got = acc.G.clone()                              # a third stream: must wait for the flush's launch
    torch.cuda.synchronize()
    del keep
    assert acc.n == 1
    assert torch.equal(got, want)


def test_staging_again_waits_for_a_flush_that_still_reads_the_buffer(dev, busy):
    from quantool_amd.engine.gptq_linear import HessianAccumulator

    X1, X2 = _tokens(dev, 2), _tokens(dev, 3)
    ref = HessianAccumulator(K, dev)
    ref.add(X1, num_samples=1)
    ref.G
    ref.add(X2, num_samples=1)
    want = ref.G.clone()
    torch.cuda.synchronize()

    staging = torch.cuda.Stream(device=dev)
    acc = HessianAccumulator(K, dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(staging):
        acc.add(X1, num_samples=1)
    keep = busy()                                        # the flush below queues behind this, on the caller's stream
    acc.G
    with torch.cuda.stream(staging):
        acc.add(X2, num_samples=1)                       # the same rows of the buffer: not before the flush has read them
        got = acc.G.clone()
    torch.cuda.synchronize()
    del keep
    assert acc.n == 2
    assert torch.equal(got, want)
