"""``qt_xtx_accumulate_batched`` on exactly summable inputs: every problem's G must equal the integer reference bit for
bit.  A dropped, doubled or foreign token, a missed chunk, a slab added to the wrong problem or tile all change an
integer.  Inputs: ``dense_ints`` (+-{1, 2, 3}), one seed per problem, guarded by ``assert_exactly_summable``; every G
starts from non-zero integers with NaN in the tiles above the diagonal tile row, which must stay NaN.

One case per branch of the batched plan (tests/xtx_batched_cases.py); each checks its plan first."""
import pytest
import torch

from tests import exact_inputs as ex
from tests.xtx_batched_cases import CASES, check_branch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _start(K, dev, seed):
    g = torch.Generator().manual_seed(seed)
    G0 = torch.randint(1, 1001, (K, K), generator=g).float()
    G0 = (G0 * (torch.randint(0, 2, (K, K), generator=g).float() * 2 - 1)).to(dev)     # never zero
    lower, untouched = ex.gram_masks(K, dev)
    return G0, torch.where(untouched, torch.full_like(G0, float("nan")), G0), lower, untouched


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_problem_equals_the_integer_reference(ops, dev, name, dtype):
    tokens, K, branch = CASES[name]
    check_branch(name, *ops.xtx_batched_plan(tokens, K))
    Xs, Gs, want, masks = [], [], [], None
    for p, n in enumerate(tokens):
        X = torch.from_numpy(ex.dense_ints((n, K), seed=1000 * p + n + K)).to(dtype).to(dev)
        G0, G, lower, untouched = _start(K, dev, seed=p)
        x64 = X.double()
        ex.assert_exactly_summable(G0.double().abs() + x64.abs().t() @ x64.abs(), 0, f"{name} problem {p}")
        Xs.append(X)
        Gs.append(G)
        want.append(G0.double() + x64.t() @ x64)
        masks = (lower, untouched)
    ops.xtx_accumulate_batched(Xs, Gs)
    torch.cuda.synchronize()
    for p, (G, w) in enumerate(zip(Gs, want)):
        ex.assert_exact(G, w, region=masks[0], untouched=masks[1], gram=True,
                        what=f"{name} [{branch}] problem {p} ({tokens[p]} tokens) {dtype}")


def _random(n, K, dev, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, K, generator=g)
    X[:, ::97] *= 10
    return X.to(dtype).to(dev)


@pytest.mark.parametrize("tokens,K", [([200], 520), ([2117], 520), ([0, 4096, 0], 512)])
def test_a_batch_of_one_is_the_single_launch(ops, dev, tokens, K):
    """One problem with tokens, alone or beside empty ones: bit-identical to ops.xtx_accumulate on random data (direct
    items, and xtx_plan's slabs with a ragged last chunk)."""
    Xs = [_random(n, K, dev, seed=n + p) for p, n in enumerate(tokens)]
    Gb = [torch.full((K, K), float(p + 1), device=dev) for p in range(len(tokens))]
    Gs = [g.clone() for g in Gb]
    ops.xtx_accumulate_batched(Xs, Gb)
    for X, G in zip(Xs, Gs):
        ops.xtx_accumulate(X, G)
    torch.cuda.synchronize()
    for p, (a, b) in enumerate(zip(Gb, Gs)):
        assert torch.equal(a, b), f"problem {p}"
        assert tokens[p] or torch.equal(a, torch.full_like(a, float(p + 1))), "an empty problem's G was touched"


@pytest.mark.parametrize("name", ["mixed", "whole_rounds"])
def test_bits_repeat_and_depend_on_the_other_problems_sizes_only(ops, dev, name):
    """Random data: a second run of the same batch gives equal bits, and other values of the same shape in problem 1
    leave every other problem's G bit-identical."""
    tokens, K, _ = CASES[name]
    Xs = [_random(n, K, dev, seed=7 * p + n) for p, n in enumerate(tokens)]

    def run(inputs):
        Gs = [torch.zeros((K, K), device=dev) for _ in tokens]
        ops.xtx_accumulate_batched(inputs, Gs)
        torch.cuda.synchronize()
        return Gs

    first, second = run(Xs), run(Xs)
    for p in range(len(tokens)):
        assert torch.equal(first[p], second[p]), f"problem {p} differs between two runs"
    other = list(Xs)
    other[1] = _random(tokens[1], K, dev, seed=12345)
    third = run(other)
    for p in range(len(tokens)):
        if p != 1:
            assert torch.equal(first[p], third[p]), f"problem {p} moved with problem 1's data"
    assert not torch.equal(first[1], third[1])


def test_wrapper_checks_and_routes(ops, dev):
    """dtype / K / duplicate-G disagreement is refused; a strided ragged input goes through the single entry point and
    a list longer than 16 is split -- results as the single launches' (exact inputs: the order cannot matter)."""
    K = 264
    with pytest.raises(TypeError):
        ops.xtx_accumulate_batched([torch.zeros(64, K, dtype=torch.bfloat16, device=dev),
                                    torch.zeros(64, K, dtype=torch.float16, device=dev)],
                                   [torch.zeros(K, K, device=dev) for _ in range(2)])
    with pytest.raises(ValueError):
        ops.xtx_accumulate_batched([torch.zeros(64, K, dtype=torch.bfloat16, device=dev)] * 2,
                                   [torch.zeros(K, K, device=dev), torch.zeros(2 * K, 2 * K, device=dev)])
    G = torch.zeros(K, K, device=dev)
    with pytest.raises(ValueError):
        ops.xtx_accumulate_batched([torch.zeros(64, K, dtype=torch.bfloat16, device=dev)] * 2, [G, G])
    tokens = [70, 128] + [64 + 3 * i for i in range(17)]
    Xs = []
    for p, n in enumerate(tokens):
        X = torch.from_numpy(ex.dense_ints((n, K + 8), seed=p)).to(torch.bfloat16).to(dev)
        Xs.append(X[:, :K] if p < 2 else X[:, :K].contiguous())       # problems 0, 1: pitch K + 8; 0 is ragged too
    Gs = [torch.zeros(K, K, device=dev) for _ in tokens]
    ops.xtx_accumulate_batched(Xs, Gs)
    torch.cuda.synchronize()
    lower, _ = ex.gram_masks(K, dev)
    for p, (X, G) in enumerate(zip(Xs, Gs)):
        ex.assert_exact(G, X.double().t() @ X.double(), region=lower, what=f"problem {p}", gram=True)
