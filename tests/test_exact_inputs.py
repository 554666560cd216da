"""CPU self-tests of tests/exact_inputs.py: the generators give what they promise, the guard refuses inputs whose
partial sums could round, and the comparator flags each mutation of a numpy Gram sum at the right tile; the exactly
factorable matrices keep their identities and their guard, and a numpy fp32 blocked Cholesky chain gives their reference
to the bit unless a k-chunk or a tile column's first block is left out."""
import numpy as np
import pytest
import torch

from tests import exact_inputs as ex


def test_dense_ints_are_nonzero_single_plane_values():
    x = ex.dense_ints((300, 264), seed=1)
    assert set(np.unique(np.abs(x))) == {1.0, 2.0, 3.0}
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(torch.from_numpy(x).to(dt).float(), torch.from_numpy(x))
    hi, mid, lo = ex.split_bf16x3(x)
    assert np.array_equal(hi, x) and not mid.any() and not lo.any()
    h, l, e = ex.split_f16x2(x, 4.0)
    assert e == 1 and np.array_equal(h, 2 * x) and not l.any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_one_hot_token_products_are_exact_in_fp32(dtype):
    X = ex.one_hot_token(70, 264, 64, dtype, seed=3)
    assert not X[:64].any() and not X[65:].any() and X[64].all()
    assert torch.equal(torch.from_numpy(X).to(dtype).float(), torch.from_numpy(X))
    row = X[64].astype(np.float64)
    prod = np.outer(row, row)
    p32 = prod.astype(np.float32)
    assert np.array_equal(p32.astype(np.float64), prod)
    assert np.isfinite(p32).all() and (np.abs(p32) >= np.finfo(np.float32).tiny).all()
    spread = np.log2(np.abs(row).max() / np.abs(row).min())
    assert spread >= (30 if dtype == torch.bfloat16 else 10)          # the exponents do spread


def test_multi_plane_columns_split_into_their_planes():
    """The restated splits (split3_kernel / split2h_kernel, round to nearest) give exactly the planes the generator
    meant, for every seed tried; the excluded pair (|a|, |b|) = (1, 2) does not (the reason it is excluded)."""
    for seed in range(40):
        col, want = ex.multi_plane_column(128, (0, 15, 127), seed, "bf16x3")
        got = ex.split_bf16x3(col)
        for p in range(3):
            assert np.array_equal(got[p].astype(np.float64), want[p]), (seed, p)
        col, want = ex.multi_plane_column(128, (16, 63, 64), seed, "f16x2")
        for bound in (4.0, 256.0):
            hi, lo, e = ex.split_f16x2(col, bound)
            assert np.array_equal(hi.astype(np.float64), want[0] * 2.0 ** e), (seed, bound)
            assert np.array_equal(lo.astype(np.float64), want[1] * 2.0 ** (e + 11)), (seed, bound)
    hi, _, _ = ex.split_bf16x3(np.float32(1 + 2 * 2.0 ** -9 + 2.0 ** -18))
    assert hi == np.float32(1 + 2.0 ** -7)


def test_kept_products_equal_the_full_product_against_a_single_plane_operand():
    k = 128
    A = ex.dense_ints((k, 8), seed=1)
    B = ex.dense_ints((k, 8), seed=2)
    A[:, 3], _ = ex.multi_plane_column(k, (0, 64, 127), 5, "bf16x3")
    full = A.astype(np.float64).T @ B.astype(np.float64)
    assert np.array_equal(ex.kept_products_bf16x3(A, B), full)
    assert np.array_equal(ex.kept_products_bf16x3(B, A), full.T)
    # two multi-plane columns against each other: mid*lo, lo*mid and lo*lo are dropped
    pair = ex.kept_products_bf16x3(A[:, 3:4], A[:, 3:4])[0, 0]
    assert pair != float(A[:, 3].astype(np.float64) @ A[:, 3].astype(np.float64))
    A[:, 3], _ = ex.multi_plane_column(k, (0, 64, 127), 5, "f16x2")
    full = A.astype(np.float64).T @ B.astype(np.float64)
    assert np.array_equal(ex.kept_products_f16x2(A, B, 4.0, 4.0), full)
    assert np.array_equal(ex.kept_products_f16x2(B, A, 256.0, 4.0), full.T)


def test_guard_accepts_exact_and_refuses_inexact_inputs():
    ex.assert_exactly_summable(2 ** 24 - 1, 0)
    ex.assert_exactly_summable(np.array([63.9, 1.0]), 18)
    ex.assert_exactly_summable(torch.tensor([[1000.0 + 9 * 2117]]), 0)
    with pytest.raises(AssertionError):
        ex.assert_exactly_summable(2 ** 24, 0)
    with pytest.raises(AssertionError):
        ex.assert_exactly_summable(np.array([1.0, 64.0]), 18)


def test_plan_restatement_matches_the_cases_the_gram_tests_name():
    assert ex.xtx_plan(63, 264)["s2"] == 1 and ex.xtx_plan(448, 1032)["s2"] == 1            # n_tt < 8: no slabs
    assert ex.xtx_plan(512, 264)["s2"] == 2 and ex.xtx_plan(2048, 256)["s2"] == 8
    assert ex.xtx_chunks(576, 264) == [(0, 320), (320, 576)]                                 # 5 and 4 token tiles
    assert ex.xtx_chunks(530, 264) == [(0, 320), (320, 530)]
    pl = ex.xtx_plan(529, 5640)
    assert (pl["n_tiles"], pl["n_direct"], pl["n_rem"], pl["s2"], pl["has_tail"]) == (276, 256, 20, 2, 1)
    assert ex.xtx_plan(2117, 520)["n_rem"] == 6 and ex.xtx_plan(2117, 520)["s2"] == 8
    assert ex.xtx_probe_tokens(530, 264) == [0, 15, 16, 63, 64, 319, 320, 512, 529]


def test_comparator_semantics():
    want = torch.tensor([[0.0, 1.0], [2.0, 3.0]], dtype=torch.float64)
    ex.assert_exact(torch.tensor([[-0.0, 1.0], [2.0, 3.0]]), want)                           # -0 == +0
    with pytest.raises(ex.ExactMismatch) as e:
        ex.assert_exact(torch.tensor([[0.0, 1.0], [float("nan"), 3.0]]), want)               # NaN equals nothing
    assert e.value.count == 1 and e.value.first == (1, 0)
    nan_want = torch.tensor([[0.0, 1.0], [float("nan"), 3.0]], dtype=torch.float64)
    with pytest.raises(ex.ExactMismatch):
        ex.assert_exact(torch.tensor([[0.0, 1.0], [float("nan"), 3.0]]), nan_want)           # not even another NaN
    unt = torch.tensor([[False, True], [False, False]])
    ex.assert_exact(torch.tensor([[0.0, float("nan")], [2.0, 3.0]]), want, untouched=unt)    # declared untouched: NaN stays
    with pytest.raises(ex.ExactMismatch) as e:
        ex.assert_exact(torch.tensor([[0.0, 1.0], [2.0, 3.0]]), want, untouched=unt)         # ... and was overwritten
    assert e.value.first == (0, 1)
    ex.assert_exact(torch.tensor([[0.0, 9.0], [2.0, 3.0]]), want, region=torch.tensor([[True, False], [True, True]]))
    with pytest.raises(ex.ExactMismatch) as e:
        ex.assert_exact(torch.tensor([[0.0, 1.0], [2.0, 3.0 + 2.0 ** -22]]), want)           # one ulp is a mismatch
    assert e.value.first == (1, 1) and e.value.delta == 2.0 ** -22


# ---- the four mutations of the numpy Gram sum ------------------------------------------------------------------------
N_TOK, K = 530, 520          # 6 lower tiles, a ragged last panel of 8 columns, two token chunks (5 + 4 tiles), a tail


@pytest.fixture(scope="module")
def gram_case():
    X = ex.dense_ints((N_TOK, K), seed=7)
    G0 = np.random.default_rng(8).integers(-1000, 1001, (K, K)).astype(np.float32)
    ex.assert_exactly_summable(np.abs(G0).astype(np.float64) + np.abs(X).astype(np.float64).T @ np.abs(X), 0)
    want = G0.astype(np.float64) + X.astype(np.float64).T @ X.astype(np.float64)
    lower, untouched = ex.gram_masks(K)
    return X, G0, want, lower, untouched


def _check(G, case):
    _, _, want, lower, untouched = case
    G = G.copy()
    G[untouched.numpy()] = np.nan                       # the fake leaves those tiles alone, as the kernels must
    ex.assert_exact(G, want, region=lower, untouched=untouched, what="fake Gram", gram=True)


def test_unmutated_fake_gram_passes(gram_case):
    X, G0 = gram_case[:2]
    assert ex.xtx_plan(N_TOK, K)["n_rem"] == 6 and len(ex.xtx_chunks(N_TOK, K)) == 2
    G, _ = ex.fake_xtx(X, G0)
    _check(G, gram_case)


def test_dropped_last_token_is_flagged_in_every_tile(gram_case):
    X, G0 = gram_case[:2]
    G, _ = ex.fake_xtx(X, G0, "drop_last_token")
    with pytest.raises(ex.ExactMismatch) as e:
        _check(G, gram_case)
    assert e.value.tiles == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]
    i, j = e.value.first
    assert e.value.tile == (0, 0) and e.value.delta == -float(X[-1, i] * X[-1, j])          # names the token's product
    assert e.value.count == K * (K + 1) // 2                                                # no zero factor hides one


def test_doubled_token_64_is_flagged_in_every_tile(gram_case):
    X, G0 = gram_case[:2]
    G, _ = ex.fake_xtx(X, G0, "double_token_64")
    with pytest.raises(ex.ExactMismatch) as e:
        _check(G, gram_case)
    i, j = e.value.first
    assert len(e.value.tiles) == 6 and e.value.delta == float(X[64, i] * X[64, j])
    assert "got - want" in str(e.value) and "tile (0, 0)" in str(e.value)


def test_shifted_column_panel_is_flagged_in_its_tile_only(gram_case):
    X, G0 = gram_case[:2]
    G, where = ex.fake_xtx(X, G0, "shift_column")
    with pytest.raises(ex.ExactMismatch) as e:
        _check(G, gram_case)
    assert where == (1, 0) and e.value.tiles == [(1, 0)] and e.value.tile == (1, 0)


def test_skipped_last_slab_chunk_is_flagged_in_its_tile_only(gram_case):
    X, G0 = gram_case[:2]
    G, where = ex.fake_xtx(X, G0, "skip_last_chunk")
    with pytest.raises(ex.ExactMismatch) as e:
        _check(G, gram_case)
    assert where == (2, 2) and e.value.tiles == [(2, 2)]
    assert e.value.first[0] >= 512 and e.value.first[1] >= 512


# ---- exactly factorable matrices (tests/test_gpu_chol_exact.py) ------------------------------------------------------
CHOL_SEEDS = [(K, K) for K in ex.CHOL_CASES] + [(K, K + b) for K in (640, 1536) for b in (1, 2)]     # the batches' seeds


@pytest.mark.parametrize("K,seed", CHOL_SEEDS)
def test_factorable_spd_identities_and_guard(K, seed):
    A, R, Y = ex.chol_case(K, seed)
    bounds = ex.assert_exactly_factorable(A, R, Y)
    print(f"\n[factorable] K={K} seed={seed}: " + ", ".join(f"{k} {v:.3g}" for k, v in bounds.items())
          + f" (limit {2.0 ** 24:.3g}); max|R| {np.abs(R).max()}, max|Y| {np.abs(Y).max()}, max|A| {np.abs(A).max()}")
    assert max(bounds.values()) * 4 < 2.0 ** 24                                    # headroom, not a near miss
    assert set(np.unique(np.diag(R))) <= {0.5, 1.0, 2.0} and len(np.unique(np.diag(R))) == 3
    assert np.array_equal(np.linalg.cholesky(A).T, R)                              # fp64 LAPACK agrees, exactly
    U = ex.chol_expected(Y)
    assert np.array_equal(U, np.triu(U)) and np.array_equal(U[0, 0], Y[K - 1, K - 1]) and np.array_equal(U[0, K - 1], Y[K - 1, 0])
    # no zero factor hides a dropped term: the triangle is well filled and every diagonal 128-block but a last block
    # of one row has off-diagonal entries
    assert np.count_nonzero(R) >= 0.1 * K * (K + 1) / 2 and np.count_nonzero(Y) >= 0.1 * K * (K + 1) / 2
    for b0 in range(0, K - 1, ex.CHOL_NB):
        assert np.count_nonzero(np.triu(R[b0:b0 + ex.CHOL_NB, b0:b0 + ex.CHOL_NB], 1)) > 0, b0
    lb = ex.min_eig_lb(A)
    assert 0 < lb < np.linalg.eigvalsh(A)[0]


def test_factorable_guard_trips_on_a_case_that_is_too_dense():
    A, R, Y = ex.factorable_spd(640, 1, 12, 0.2)
    assert np.array_equal(R @ Y.T, np.eye(640))                                    # still an exact inverse pair ...
    with pytest.raises(AssertionError):
        ex.assert_exactly_factorable(A, R, Y)                                      # ... whose sums no longer fit fp32
    A, R, Y = ex.chol_case(333)
    with pytest.raises(AssertionError, match="R Rinv"):
        ex.assert_exactly_factorable(A, R, np.tril(Y + np.eye(333)))
    R3 = R.copy()
    R3[0, 1] = 1.0 + 2.0 ** -9                                                     # two bf16 planes
    with pytest.raises(AssertionError):
        ex.assert_exactly_factorable(R3.T @ R3, R3, np.linalg.inv(R3).T)


@pytest.fixture(scope="module", params=[333, 640])
def chol_case(request):
    A, R, Y = ex.chol_case(request.param)
    ex.assert_exactly_factorable(A, R, Y)
    return A, R, ex.chol_expected(Y)


def test_fp32_blocked_chain_gives_the_reference_to_the_bit(chol_case):
    A, R, want = chol_case
    poisoned = A.copy()
    poisoned[np.tril_indices(A.shape[0], -1)] = np.nan
    U, info = ex.fake_chol_chain(poisoned)
    assert info == 0 and U.dtype == np.float32
    ex.assert_exact(U, want, what="fake chain")
    U64, _ = ex.fake_chol_chain(A, nb=64)                                          # ... whatever the blocking
    ex.assert_exact(U64, want, what="fake chain, 64-row blocks")


def test_chain_with_a_k_chunk_left_out_is_flagged(chol_case):
    """64 k-rows missing from the factor's product of the last block row: its rows of R, hence of Y, hence the FIRST rows
    of U are wrong, and nothing else."""
    A, R, want = chol_case
    K = A.shape[0]
    last = (K - 1) // ex.CHOL_NB * ex.CHOL_NB
    U, info = ex.fake_chol_chain(A, "drop_chunk")
    assert info == 0
    with pytest.raises(ex.ExactMismatch) as e:
        ex.assert_exact(U, want, what="fake chain, chunk dropped")
    bad_rows = np.flatnonzero((U.astype(np.float64) != want).any(axis=1))
    assert e.value.count > 0 and e.value.tile[0] == 0 and bad_rows.max() < K - last


def test_chain_with_a_tile_column_started_one_block_late_is_flagged(chol_case):
    """The inverse's product of the last block row skips the first 128 k-rows of tile column 0: Y[last rows, :128], i.e.
    the first rows and last 128 columns of U, and nothing else."""
    A, R, want = chol_case
    K = A.shape[0]
    last = (K - 1) // ex.CHOL_NB * ex.CHOL_NB
    U, info = ex.fake_chol_chain(A, "late_k")
    assert info == 0
    with pytest.raises(ex.ExactMismatch) as e:
        ex.assert_exact(U, want, what="fake chain, late k")
    bad = np.argwhere(U.astype(np.float64) != want)
    assert e.value.count == len(bad) > 0
    assert bad[:, 0].max() < K - last and bad[:, 1].min() >= K - ex.CHOL_NB
    assert e.value.tile[0] == 0 and e.value.tile[1] >= (K - ex.CHOL_NB) // ex.TILE


@pytest.mark.parametrize("factor", [1, 2])
def test_zero_and_negative_pivots_are_placed_exactly(chol_case, factor):
    A, R, _ = chol_case
    K = A.shape[0]
    for j in (0, 31, 32, 127, 128, K - 70, K - 1):
        B = ex.with_zero_pivot(A, R, j, factor)
        assert np.array_equal(np.delete(B.ravel(), j * K + j), np.delete(A.ravel(), j * K + j))
        U, info = ex.fake_chol_chain(B)
        assert info == j + 1 and np.array_equal(U, np.eye(K, dtype=np.float32))
        # the pivot itself: exactly 0 / -R[j][j]^2 in fp64, with the rows before it those of R
        piv = B[j, j] - R[:j, j] @ R[:j, j]
        assert piv == -(factor - 1) * R[j, j] ** 2
