"""Exactly summable inputs for the calibration side's MFMA sums (test infrastructure, no GPU needed).

bf16 x bf16 and fp16 x fp16 products are exact in the fp32 accumulator (include/quantool_amd.h, a7).  When every term of
an output is a multiple of 2^-q and sum |terms| * 2^q < 2^24, every partial sum in every order is a multiple of 2^-q of
magnitude below 2^24 * 2^-q, i.e. exactly representable in fp32: the result is then a pure function of WHICH products
were added, and a kernel must reproduce the integer reference bit for bit.  This module holds

* the generators: dense single-plane integers, one-hot-token matrices, sparse multi-plane columns;
* ``assert_exactly_summable``: the guard every case calls on its own inputs before it launches;
* ``assert_exact``: the comparator (elementwise equality, a report that names the first wrong entry and its tile);
* restatements of the two plane splits of csrc/gemm3_tn.hip and of the token plan of csrc/xtx.hip;
* ``fake_xtx``: a numpy Gram sum that walks that plan, with switchable mutations, for the comparator's self-tests.
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
