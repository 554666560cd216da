"""Exactly summable inputs for the calibration side's MFMA sums (test infrastructure, no GPU needed).

bf16 x bf16 and fp16 x fp16 products are exact in the fp32 accumulator (include/quantool_amd.h, a7).  When every term of
an output is a multiple of 2^-q and sum |terms| * 2^q < 2^24, every partial sum in every order is a multiple of 2^-q of
magnitude below 2^24 * 2^-q, i.e. exactly representable in fp32: the result is then a pure function of WHICH products
were added, and a kernel must reproduce the integer reference bit for bit.  This module holds

* the generators: dense single-plane integers, one-hot-token matrices, sparse multi-plane columns;
* ``assert_exactly_summable``: the guard every case calls on its own inputs before it launches;
* ``assert_exact``: the comparator (elementwise equality, a report that names the first wrong entry and its tile);
* restatements of the two plane splits of csrc/gemm3_tn.hip and of the token plan of csrc/xtx.hip;
* ``fake_xtx``: a numpy Gram sum that walks that plan, with switchable mutations, for the comparator's self-tests;
* for the Cholesky chain (csrc/cholesky.hip): ``factorable_spd`` -- matrices whose factor, inverse factor and every
  intermediate are short dyadic numbers --, their guard ``assert_exactly_factorable``, ``with_zero_pivot``,
  ``min_eig_lb`` and ``fake_chol_chain``, a numpy fp32 blocked chain with switchable mutations.
"""
import numpy as np
import torch

TILE = 256            # output tile edge of every kernel here (BT in csrc/common.h)
TOKEN_TILE = 64       # tokens per token tile of the Gram kernel (BKT in csrc/xtx.hip)
NUM_CU = 256


# ----------------------------------------------------------------------------------------------------------- generators
def dense_ints(shape, seed, top=3):
    """float32 array of values in +-{1, 2, 3} (+-{1 .. top}): never zero (no dropped product hides behind a zero
    factor), exact in bf16 and fp16, and a single plane of either split."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, top + 1, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float32)


def one_hot_token(n_tokens, K, token, dtype, seed):
    """[n_tokens, K] float32, zero but for row `token`, which holds seeded values exact in `dtype`:
    bf16: +-(1 + m / 128) * 2^e, e in [-20, 20]; fp16: +-(1 + m / 1024) * 2^e, e in [-7, 7].  A product of two of them
    has at most 16 / 22 significant bits and an exponent inside +-41 / +-15: exact and normal in fp32."""
    rng = np.random.default_rng(seed)
    frac, emax = (128, 20) if dtype == torch.bfloat16 else (1024, 7)
    row = (1.0 + rng.integers(0, frac, K) / frac) * np.exp2(rng.integers(-emax, emax + 1, K)) * rng.choice([-1.0, 1.0], K)
    X = np.zeros((n_tokens, K), dtype=np.float32)
    X[token] = row.astype(np.float32)
    assert np.array_equal(X[token].astype(np.float64), row)
    return X


# (|a|, |b|) pairs of a multi-plane entry a + b 2^-9 + c 2^-18 whose round-to-nearest split (split3_kernel) gives the
# planes a, b 2^-9, c 2^-18 themselves.  (1, 2) is left out: its residual 2^-8 + c 2^-18 lies above half an ulp of the
# bf16 value 1 (2^-8), so round-to-nearest makes the hi plane 1 + 2^-7 where a truncating split keeps 1.
BF16X3_AB = ((1, 1), (2, 1), (2, 2))


def multi_plane_column(k, positions, seed, planes="bf16x3"):
    """float32 column of length k, zero except at `positions` (at most 3), where it holds
    bf16x3: s * (a + b 2^-9 + c 2^-18), (a, b) from BF16X3_AB, c in {1, 2};   f16x2: s * (a + b 2^-12), a, b in {1, 2}
    with one sign s per entry, so that hi, mid and lo pull the same way.  Returns (column, planes [n_planes, k] float64
    as the split must produce them)."""
    assert len(positions) <= 3 and len(set(positions)) == len(positions) and all(0 <= p < k for p in positions)
    rng = np.random.default_rng(seed)
    n_pl = 3 if planes == "bf16x3" else 2
    col = np.zeros(k, dtype=np.float64)
    want = np.zeros((n_pl, k), dtype=np.float64)
    for p in positions:
        s = float(rng.choice([-1, 1]))
        if planes == "bf16x3":
            a, b = BF16X3_AB[rng.integers(0, len(BF16X3_AB))]
            c = int(rng.integers(1, 3))
            want[:, p] = (s * a, s * b * 2.0 ** -9, s * c * 2.0 ** -18)
        else:
            a, b = int(rng.integers(1, 3)), int(rng.integers(1, 3))
            want[:, p] = (s * a, s * b * 2.0 ** -12)
        col[p] = want[:, p].sum()
    out = col.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), col)           # 19 / 14 significant bits: exact in fp32
    return out, want


# ----------------------------------------------------------------------------------------------------- the plane splits
def _bf16_rne(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def split_bf16x3(x):
    """split3_kernel of csrc/gemm3_tn.hip: h = bf16_rne(x); r1 = x - h; m = bf16_rne(r1); r2 = r1 - m; lo = bf16_rne(r2).
    -> (hi, mid, lo) float32 arrays."""
    x = np.asarray(x, dtype=np.float32)
    hi = _bf16_rne(x)
    r1 = x - hi
    mid = _bf16_rne(r1)
    r2 = r1 - mid
    return hi, mid, _bf16_rne(r2)


def kept_products_bf16x3(A, B):
    """fp64 sum of the six plane products gemm3_kernel keeps (PA_BITS / PB_BITS: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid,
    hi*hi); mid*lo, lo*mid and lo*lo are dropped.  A [k, M], B [k, N] float32 -> [M, N] float64."""
    pa = [p.astype(np.float64) for p in split_bf16x3(A)]
    pb = [p.astype(np.float64) for p in split_bf16x3(B)]
    out = np.zeros((A.shape[1], B.shape[1]), dtype=np.float64)
    for ia, ib in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
        _add_tn(out, pa[ia], pb[ib])
    return out


def _add_tn(out, a, b):
    """out += a^T b, over the columns of a and b that are not all zero (mid / lo planes are mostly empty)."""
    ca, cb = np.flatnonzero(a.any(axis=0)), np.flatnonzero(b.any(axis=0))
    if len(ca) and len(cb):
        out[np.ix_(ca, cb)] += a[:, ca].T @ b[:, cb]


def f16x2_scale_exponent(bound):
    """g3_scale_exponent: e = 3 - ceil(log2(bound))."""
    m, x = np.frexp(np.float32(bound))
    return int(3 - (x - 1 if m == 0.5 else x))


def split_f16x2(x, bound):
    """split2h_kernel: xs = x * 2^e; h = (_Float16)xs (nearest); lo' = (_Float16)((xs - h) * 2048).
    -> (hi, lo', e), the planes as float32 arrays of the SCALED values."""
    e = f16x2_scale_exponent(bound)
    xs = np.asarray(x, dtype=np.float32) * np.float32(2.0 ** e)
    hi = xs.astype(np.float16).astype(np.float32)
    lo = ((xs - hi) * np.float32(2048.0)).astype(np.float16).astype(np.float32)
    return hi, lo, e


def kept_products_f16x2(A, B, bound_a, bound_b):
    """fp64 value of the three products the duo loop keeps -- lo'_a hi_b + hi_a lo'_b + hi_a (2^11 hi_b), times
    2^-(11 + eA + eB); lo'_a lo'_b is dropped."""
    ha, la, ea = split_f16x2(A, bound_a)
    hb, lb, eb = split_f16x2(B, bound_b)
    ha, la, hb, lb = (p.astype(np.float64) for p in (ha, la, hb, lb))
    return (la.T @ hb + ha.T @ lb + ha.T @ (2048.0 * hb)) * 2.0 ** -(11 + ea + eb)


# ------------------------------------------------------------------------------------------------------------ the guard
def assert_exactly_summable(abs_sum, q, what=""):
    """The precondition of every exact case: all terms of an output are multiples of 2^-q and `abs_sum` is that
    output's sum |terms| (a start value included) -- computed in int64 / fp64 on the reference side.  Then
    abs_sum * 2^q < 2^24 makes every partial sum in every order exact in fp32.  A violation is a bug of the test."""
    worst = float(torch.as_tensor(abs_sum, dtype=torch.float64).max()) if not np.isscalar(abs_sum) else float(abs_sum)
    assert worst * 2.0 ** q < 2.0 ** 24, f"{what}: sum|terms| = {worst} in units of 2^-{q} is not below 2^24"


# ------------------------------------------------------------------------------------------------------- the comparator
class ExactMismatch(AssertionError):
    """Carries what the report says: count, first (i, j), tile of the first, all wrong tiles, got - want at the first."""

    def __init__(self, msg, count, first, tiles, delta):
        super().__init__(msg)
        self.count, self.first, self.tiles, self.delta = count, first, tiles, delta
        self.tile = (first[-2] // TILE, first[-1] // TILE)


def assert_exact(got, want, region=None, untouched=None, what="", gram=False):
    """got == want elementwise over `region` (bool mask, default everything): -0 equals +0, NaN equals nothing.  Entries
    of `untouched` (bool mask) are exempt from that and must instead still hold the NaN the case put there.
    Tensors or arrays, on any device (a large G stays on the GPU); compared in fp64.
    Raises ExactMismatch: number of wrong entries, the first (i, j), its 256-tile; for a Gram also got - want there."""
    got = torch.as_tensor(got)
    want = torch.as_tensor(want).to(got.device)
    assert got.shape == want.shape, (got.shape, want.shape)
    g64 = got.double()
    bad = g64 != want.double()                                   # NaN != x for every x, NaN included
    if region is not None:
        bad &= torch.as_tensor(region).to(got.device)
    if untouched is not None:
        u = torch.as_tensor(untouched).to(got.device)
        bad = torch.where(u, ~torch.isnan(g64), bad)
    count = int(bad.sum())
    if count == 0:
        return
    idx = torch.nonzero(bad)
    first = tuple(int(v) for v in idx[0])
    tiles = sorted({(int(a), int(b)) for a, b in torch.unique(idx[:, -2:] // TILE, dim=0).cpu().tolist()})
    delta = float(g64[first] - want.double()[first])
    msg = (f"{what}: {count} entries differ; first at {first} in tile {(first[-2] // TILE, first[-1] // TILE)}: "
           f"got {float(g64[first])!r}, want {float(want.double()[first])!r}; {len(tiles)} wrong tiles, first {tiles[:8]}")
    if gram:
        msg += f"; got - want = {delta!r} (the product x[t][i] * x[t][j] of the token that is missing or doubled)"
    raise ExactMismatch(msg, count, first, tiles, delta)


def gram_masks(K, device=None):
    """(lower, untouched): the lower triangle incl. the diagonal, and the 256 x 256 tiles strictly above the diagonal
    tile row, which no Gram entry point may write (quantool_amd.h: "lower triangle incl. diagonal tiles")."""
    i = torch.arange(K, device=device)
    lower = i[:, None] >= i[None, :]
    untouched = (i[None, :] // TILE) > (i[:, None] // TILE)
    return lower, untouched


# ------------------------------------------------------------------------------------- the Gram kernel's plan, restated
def xtx_plan(n_tokens, K):
    """xtx_plan of csrc/xtx.hip: -> dict(n_tiles, n_tt, has_tail, s2, n_direct, n_rem)."""
    nt = (K + TILE - 1) // TILE
    n_tiles = nt * (nt + 1) // 2
    n_tt = (n_tokens + TOKEN_TILE - 1) // TOKEN_TILE
    n_full = n_tiles // NUM_CU * NUM_CU
    rem = n_tiles - n_full
    best, best_cost = 1, 1.0
    if rem > 0:
        for S in range(2, 65):
            if n_tt // S < 4 or S * rem * TILE * TILE * 4 > 1 << 30:
                break
            cost = ((rem * S + NUM_CU - 1) // NUM_CU) / S
            if cost < best_cost * 0.97:
                best_cost, best = cost, S
    return dict(n_tiles=n_tiles, n_tt=n_tt, has_tail=int(n_tokens % TOKEN_TILE != 0), s2=best,
                n_direct=n_tiles if best == 1 else n_full, n_rem=0 if best == 1 else rem)


def xtx_chunks(n_tokens, K):
    """Token ranges [t0, t1) of the slab chunks, by the formula of xtx_item: chunk c takes base + (c < rem) token
    tiles.  One range over everything when the plan has no slabs."""
    pl = xtx_plan(n_tokens, K)
    base, rem = pl["n_tt"] // pl["s2"], pl["n_tt"] % pl["s2"]
    out = []
    for c in range(pl["s2"]):
        tt0 = c * base + min(c, rem)
        cnt = base + (1 if c < rem else 0)
        out.append((tt0 * TOKEN_TILE, min(n_tokens, (tt0 + cnt) * TOKEN_TILE)))
    return out


def xtx_probe_tokens(n_tokens, K):
    """Token positions a one-hot case visits: 0, 15, 16, 63, 64 (unit, double and token-tile edges), the first and last
    token of every slab chunk, the first tail token and the last token."""
    pos = {0, 15, 16, 63, 64, n_tokens - 1}
    for t0, t1 in xtx_chunks(n_tokens, K):
        pos.update((t0, t1 - 1))
    if n_tokens % TOKEN_TILE:
        pos.add(n_tokens // TOKEN_TILE * TOKEN_TILE)
    return sorted(p for p in pos if 0 <= p < n_tokens)


def fake_xtx(X, G0, mutation=None):
    """A numpy Gram sum G0 + X^T X that walks the kernel's plan -- lower tiles; the tiles of the plan's remainder (here:
    the last n_rem in row-major order) as token chunks summed slab by slab, the others over all tokens.  `mutation`
    breaks it the way an indexing bug would:
      "drop_last_token"   every tile leaves the last token out;
      "double_token_64"   every tile counts token 64 twice;
      "shift_column"      tile (1, 0) reads its column panel 8 channels to the right;
      "skip_last_chunk"   the last slabbed tile leaves its last token chunk out.
    -> (G float32 [K, K], tile the mutation is confined to or None for all tiles)."""
    X = np.asarray(X, dtype=np.float64)
    n, K = X.shape
    nt = (K + TILE - 1) // TILE
    tiles = [(ti, tj) for ti in range(nt) for tj in range(ti + 1)]
    pl = xtx_plan(n, K)
    chunks = xtx_chunks(n, K)
    G = np.array(G0, dtype=np.float64)
    where = None
    for idx, (ti, tj) in enumerate(tiles):
        r = slice(ti * TILE, min(K, (ti + 1) * TILE))
        c = slice(tj * TILE, min(K, (tj + 1) * TILE))
        Xa, Xb = X[:, r], X[:, c]
        if mutation == "shift_column" and (ti, tj) == (1, 0):
            Xb = X[:, np.minimum(np.arange(c.start, c.stop) + 8, K - 1)]
            where = (ti, tj)
        slabbed = idx >= pl["n_direct"]
        spans = chunks if slabbed else [(0, n)]
        if mutation == "skip_last_chunk" and idx == len(tiles) - 1:
            assert slabbed and len(spans) > 1, "the shape has no slabs"
            spans = spans[:-1]
            where = (ti, tj)
        acc = np.zeros((r.stop - r.start, c.stop - c.start))
        for t0, t1 in spans:
            t1 = t1 - 1 if mutation == "drop_last_token" and t1 == n else t1
            acc += Xa[t0:t1].T @ Xb[t0:t1]
            if mutation == "double_token_64" and t0 <= 64 < t1:
                acc += np.outer(Xa[64], Xb[64])
        G[r, c] += acc
    return G.astype(np.float32), where


# ------------------------------------------------------------------------- exactly factorable matrices (Cholesky chain)
# A symmetric positive definite matrix whose Cholesky factor, inverse factor and every intermediate of the blocked chain
# of csrc/cholesky.hip are short dyadic numbers: the chain then has ONE correct answer to the bit, whatever the block
# sizes, the order of a sum, the split of a k range or the arithmetic (fp32 fmaf chain, three bf16 planes, two fp16
# planes) -- a wrong output is a term that is missing, doubled or misplaced, never rounding.
CHOL_NB = 128         # panel block of the chain (NB in csrc/chol_layout.h)


def factorable_spd(K, seed, n_factors, density, exps=(-1, 0, 1)):
    """-> (A, R, Y) in fp64 with A = R^T R, R upper triangular, Y = R^-T (lower).
    R = D (I + N_1) ... (I + N_f): N_i is zero but for the block [:cut_i, cut_i:], which holds {-1, 0, +1} at `density`
    (distinct seeded cuts in [8, K - 8)), so N_i^2 = 0 and (I + N_i)^-1 = I - N_i; D = diag(2^e), e drawn from `exps`
    (the pivots of A are 4^e).  Rinv = (I - N_f) ... (I - N_1) D^-1 is formed by the same products: no solve.
    R[r][c], r < c, can be non-zero only where a cut lies in (r, c]: the cuts are therefore drawn one from each of
    n_factors equal strata of [8, K - 8) and applied in a seeded order, so that with a stratum of at most 128 every
    diagonal block of the chain has off-diagonal entries and every 128 k-rows of a product carry terms.
    The chain's contract (flat reversal of Y): U[i][j] = Y[K-1-i][K-1-j], strict lower triangle zero -- `chol_expected`."""
    assert K >= 18 and 1 <= n_factors <= K - 16
    rng = np.random.default_rng(seed)
    edges = np.linspace(8, K - 8, n_factors + 1).astype(np.int64)
    cuts = rng.permutation(np.array([rng.integers(edges[i], edges[i + 1]) for i in range(n_factors)]))
    d = np.exp2(rng.choice(np.asarray(exps, dtype=np.float64), size=K))
    R = np.diag(d)
    Rinv = np.diag(1.0 / d)
    for cut in cuts:
        blk = rng.choice([-1.0, 1.0], size=(cut, K - cut)) * (rng.random((cut, K - cut)) < density)
        R[:, cut:] += R[:, :cut] @ blk                       # R (I + N)
        Rinv[:cut, :] -= blk @ Rinv[cut:, :]                 # (I - N) Rinv
    return R.T @ R, R, np.ascontiguousarray(Rinv.T)


# K -> (n_factors, density) of the cases the tests use (seed = K; the batches also K + 1, K + 2): R is 11-25 % dense in
# its triangle, every diagonal 128-block has off-diagonal entries, and every bound of chol_exact_bounds keeps more
# than 4x headroom below 2^24 (tests/test_exact_inputs.py checks each)
CHOL_CASES = {129: (4, 0.1), 333: (8, 0.04), 640: (12, 0.015), 1000: (12, 0.012), 1536: (12, 0.008)}


def chol_case(K, seed=None, exps=(-1, 0, 1)):
    """factorable_spd at the parameters of CHOL_CASES, seed K unless given."""
    return factorable_spd(K, K if seed is None else seed, *CHOL_CASES[K], exps=exps)


def chol_expected(Y):
    """What ``qt_cholesky_inverse_upper`` must return for A = R^T R: U[i][j] = Y[K-1-i][K-1-j] (upper, zeros below)."""
    return np.ascontiguousarray(np.asarray(Y)[::-1, ::-1])


def min_eig_lb(A):
    """A valid ``min_eig_lb`` argument of the bounded entry points: half of fp64 eigvalsh(A)[0]."""
    return 0.5 * float(np.linalg.eigvalsh(np.asarray(A, dtype=np.float64))[0])


def with_zero_pivot(A, R, j, factor=1):
    """A - factor * R[j][j]^2 e_j e_j^T: pivot j of the factorisation is exactly 0 (factor 1) or -R[j][j]^2 (factor 2);
    every earlier pivot and every earlier row of R is unchanged."""
    B = np.array(A, dtype=np.float64)
    B[j, j] -= factor * R[j, j] ** 2
    return B


def chol_scale_exponent(bound):
    """The device's g3 scale exponent of a bound on |x|: 3 - ceil(log2(bound)) (chol_scales_kernel forms it from log2f)."""
    return int(3 - np.ceil(np.log2(float(bound))))


def _single_f16_plane(x, e):
    """x * 2^e is an fp16 value (split2h_kernel: hi == xs, lo' == 0) for every entry."""
    xs = np.asarray(x, dtype=np.float32) * np.float32(2.0 ** e)
    hi = xs.astype(np.float16).astype(np.float32)
    lo = ((xs - hi) * np.float32(2048.0)).astype(np.float16).astype(np.float32)
    return bool(np.array_equal(hi, xs)) and not lo.any()


def chol_exact_bounds(A, R, Y):
    """The largest sum |terms| of each family of sums the chain forms, in units of that family's least significant bit
    (R in halves, Rinv in quarters, A in quarters).  With P = |A| + |R|^T |R| (the factorisation's own sums):
      fac    4 max P                       A[i][j] - sum_p R[p][i] R[p][j]: potf2 (iii), trsm_rt's updates, the folds,
                                           both long products of the factor
      solve  16 max(|Rinv|^T P)            X^T B: potf2 (ii), trsm_rt's Z_b -- a 32-row inverse times a partial sum of A
      inv3   32 max(|Rinv| |R| |Rinv|)     Dinv^T T, Y_II T_I (the NEG products), trinv_mfma's X_b^T (I - R^T Z)
      inv2   8 max(|R|^T |Rinv|^T)         T = R^T Y (both recurrences, the long product of the inverse), potf2 (i)'s
                                           I - R^T Z, trinv_mfma's updates
      inv2r  8 max(|R| |Rinv|)             trinv_batched_kernel (QT_CHOL_TRINV=div): x_i -= R[i][p] x_p sums over R's rows
    -> dict name -> value; each must stay below 2^24."""
    aA, aR, aRi = np.abs(A), np.abs(R), np.abs(Y).T
    P = aA + aR.T @ aR
    return dict(fac=4.0 * P.max(), solve=16.0 * (aRi.T @ P).max(), inv3=32.0 * (aRi @ aR @ aRi).max(),
                inv2=8.0 * (aR.T @ aRi.T).max(), inv2r=8.0 * (aR @ aRi).max())


def assert_exactly_factorable(A, R, Y):
    """The precondition of every exact Cholesky case (a violation is a bug of the test, as with assert_exactly_summable):
    R Rinv == I exactly; A, R and Y survive fp32; every entry of R and Y is a single plane of both splits (bf16x3: mid
    = lo = 0; f16x2: lo' = 0 at the exponent the bound yields and at one less -- the device forms the exponent with
    log2f + ceilf and may land one lower at an exact power of four); every bound of chol_exact_bounds is below 2^24, so
    every partial sum of the factorisation, the panel solves and the inverse recurrences is exact in fp32 in any order.
    -> the bounds."""
    A, R, Y = (np.asarray(x, dtype=np.float64) for x in (A, R, Y))
    K = A.shape[0]
    assert np.array_equal(R, np.triu(R)) and np.array_equal(Y, np.tril(Y))
    assert np.array_equal(R @ Y.T, np.eye(K)), "R Rinv != I"
    assert np.array_equal(R.T @ R, A), "A != R^T R"
    for name, x in (("A", A), ("R", R), ("Y", Y)):
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x), f"{name} does not survive fp32"
    assert np.array_equal(R * 2, np.rint(R * 2)) and np.array_equal(Y * 4, np.rint(Y * 4)), "R in halves, Y in quarters"
    for name, x, bound in (("R", R, np.sqrt(np.diag(A).max())), ("Y", Y, 1.0 / np.sqrt(min_eig_lb(A)))):
        hi, mid, lo = split_bf16x3(x)
        assert np.array_equal(hi.astype(np.float64), x) and not mid.any() and not lo.any(), f"{name}: not one bf16 plane"
        assert np.abs(x).max() <= bound, f"{name}: the bound the scale exponent comes from does not hold"
        e = chol_scale_exponent(bound)
        assert _single_f16_plane(x, e) and _single_f16_plane(x, e - 1), f"{name}: not one fp16 plane at 2^{e} / 2^{e - 1}"
    bounds = chol_exact_bounds(A, R, Y)
    for name, v in bounds.items():
        assert v < 2.0 ** 24, f"{name}: sum|terms| = {v} lsb is not below 2^24"
    return bounds


def fake_chol_chain(A, mutation=None, nb=CHOL_NB):
    """A plain fp32 numpy restatement of the chain, left-looking by `nb`-row blocks: per block row j the product
    A[j, j:] -= R[:j0, j]^T R[:j0, j:], the diagonal block's factor, the panel solve with the block's inverse; then
    Y = R^-T block row by block row -- T = R[:i0, i]^T Y[:i0, :i0] with every `nb`-wide tile column's k range starting at
    its own first row (Y is lower triangular), Y[i, :i0] = -Dinv_i^T T -- and the flat reversal.  Only A's upper triangle
    is read.  `mutation` breaks it the way an indexing bug would:
      "drop_chunk"   the factor's product of the LAST block row leaves out the 64 k-rows [64, 128);
      "late_k"       tile column 0 of the inverse's product of the LAST block row starts its k range one block late.
    -> (U float32 [K, K], info)."""
    A = np.triu(np.asarray(A, dtype=np.float32))
    K = A.shape[0]
    R = np.zeros((K, K), dtype=np.float32)
    Dinv = {}
    starts = list(range(0, K, nb))
    for j0 in starts:
        j1 = min(K, j0 + nb)
        S = A[j0:j1, j0:].copy()
        if j0 > 0:
            keep = np.ones(j0, dtype=bool)
            if mutation == "drop_chunk" and j0 == starts[-1]:
                keep[64:128] = False
            S -= R[:j0, j0:j1][keep].T @ R[:j0, j0:][keep]
        n = j1 - j0
        Rjj = np.zeros((n, n), dtype=np.float32)
        D = S[:, :n].copy()
        for c in range(n):                                   # right-looking, one row per step (potf2's step c)
            piv = D[c, c]
            if not piv > 0:
                return np.eye(K, dtype=np.float32), j0 + c + 1
            Rjj[c, c:] = D[c, c:] / np.sqrt(piv)
            D[c + 1:, c + 1:] -= np.outer(Rjj[c, c + 1:], Rjj[c, c + 1:])
        X = np.eye(n, dtype=np.float32)                      # X = Rjj^-1 by back substitution, column by column
        for p in range(n - 1, -1, -1):
            X[p, :] /= Rjj[p, p]
            X[:p, :] -= np.outer(Rjj[:p, p], X[p, :])
        Dinv[j0] = X
        R[j0:j1, j0:j1] = Rjj
        R[j0:j1, j1:] = X.T @ S[:, n:]
    Y = np.zeros((K, K), dtype=np.float32)
    for i0 in starts:
        i1 = min(K, i0 + nb)
        Y[i0:i1, i0:i1] = Dinv[i0].T
        if i0 == 0:
            continue
        T = np.zeros((i1 - i0, i0), dtype=np.float32)
        for c0 in range(0, i0, nb):
            k0 = c0
            if mutation == "late_k" and i0 == starts[-1] and c0 == 0:
                k0 = nb
            T[:, c0:c0 + nb] = R[k0:i0, i0:i1].T @ Y[k0:i0, c0:c0 + nb]
        Y[i0:i1, :i0] = -(Dinv[i0].T @ T)
    return np.ascontiguousarray(Y[::-1, ::-1]), 0
