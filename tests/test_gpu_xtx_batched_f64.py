"""``qt_xtx_accumulate_batched`` against the fp64 Gram of the same rounded inputs, on inputs as the benchmark's:
N(0, 1) with 1 % of the channels x 10.  The bar is the project's Hessian bar, as in
tests/test_gpu_kernels.py::test_xtx_matches_f64_gram: |dG_ij| <= 1e-5 * sqrt(G_ii G_jj) over the lower triangle.
One case per branch of the batched plan (tests/xtx_batched_cases.py), both 16-bit dtypes."""
import pytest
import torch

from tests.xtx_batched_cases import CASES, check_branch

pytestmark = pytest.mark.gpu


def _inputs(n, K, dev, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, K, generator=g)
    cols = torch.randperm(K, generator=g)[:max(1, round(K * 0.01))]
    X[:, cols] *= 10.0
    return X.to(dtype).to(dev)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(CASES))
def test_every_problem_within_the_hessian_bar(ops, dev, name, dtype):
    tokens, K, branch = CASES[name]
    check_branch(name, *ops.xtx_batched_plan(tokens, K))
    Xs = [_inputs(n, K, dev, seed=31 * p + n + K, dtype=dtype) for p, n in enumerate(tokens)]
    Gs = [torch.zeros((K, K), dtype=torch.float32, device=dev) for _ in tokens]
    ops.xtx_accumulate_batched(Xs, Gs)
    ops.xtx_accumulate_batched(Xs, Gs)          # accumulate semantics: a second call adds
    torch.cuda.synchronize()
    for p, (X, G) in enumerate(zip(Xs, Gs)):
        if tokens[p] == 0:
            assert not G.any(), f"{name}: the empty problem {p} was written"
            continue
        x64 = X.double()
        want = 2 * (x64.t() @ x64)
        d = torch.sqrt(torch.outer(torch.diagonal(want), torch.diagonal(want)))
        err = float((torch.tril(G.double() - want).abs() / d).max())
        print(f"{name} [{branch}] problem {p} ({tokens[p]} tokens) {dtype}: max |dG| / sqrt(Gii Gjj) = {err:.3e}")
        assert err <= 1e-5, f"{name} problem {p}: {err:.3e}"
