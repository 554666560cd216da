"""The plane products (``qt_gemm3_tn_f32`` / ``_ex``: three bf16 planes; ``qt_gemm3_tn_f16x2``: two fp16 planes) and the
fp32 Gram (``qt_xtx_accumulate_f32``) on exactly summable inputs: the result must equal the reference bit for bit, so a
k-row, a chunk, a slab or one plane product that is missing, doubled or weighted wrongly fails -- the magnitude bars of
test_gpu_gemm3*.py / test_gpu_gemm_f16x2.py / test_gpu_fp32_activations.py cannot see a term that small.

Two kinds of input (tests/exact_inputs.py):

* dense single-plane integers +-{1, 2, 3}: the mid / lo planes are zero, the result is the integer product whatever the
  loop order -- pins WHICH (k-row, column) products are added;
* sparse multi-plane columns: a few columns of one operand are zero but for <= 3 entries a + b 2^-9 + c 2^-18 (f16x2:
  a + b 2^-12) at chosen k rows, against a dense single-plane other operand -- pins each kept plane product and its
  weight.  The reference is the fp64 sum of the KEPT plane products of the split restated from the kernel's own
  conversion, csrc/gemm3_tn.hip:

      split3_kernel:   const unsigned short h = bf16_bits_rne(x);
                       const float r1 = x - qt_bf16_to_f32(h);            // exact
                       const unsigned short m = bf16_bits_rne(r1);
                       const float r2 = r1 - qt_bf16_to_f32(m);           // exact
                       lo[e] = bf16_bits_rne(r2);
      kept (PA_BITS / PB_BITS):  A lo*B hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi   (mid*lo, lo*mid, lo*lo dropped)

      split2h_kernel:  float x = v[q] * scale;                             // scale = 2^e, e = 3 - ceil(log2(bound))
                       const _Float16 h = (_Float16)x;
                       const float r1 = x - (float)h;                      // exact
                       lo[q] = (_Float16)(r1 * 2048.0f)
      kept (duo loop): lo'_a * hi_b, hi_a * lo'_b, hi_a * (2^11 hi_b), all times 2^-(11 + eA + eB)   (lo'*lo' dropped)

  The split is round-to-nearest, so the entry (|a|, |b|) = (1, 2) is not generated: its hi plane is 1 + 2^-7, not 1
  (exact_inputs.BF16X3_AB; checked on the CPU in test_exact_inputs.py).  Against a single-plane operand every plane of
  the multi-plane column meets a kept product, so the reference equals the full product; an output where TWO multi-plane
  columns meet has nonzero dropped products and is held to 16 * 2^-24 * sum |a||b| instead of equality.

Guard (``assert_exactly_summable``, called by every case before it launches): integer outputs: |C0| + sum |a||b| < 2^24;
multi-plane outputs: terms are multiples of 2^-18 (2^-12) and |C0| + sum |a||b| < 2^6 (2^12), which is why there are at
most 3 entries of magnitude about 2 against |b| <= 3 and a start value of at most 20.
"""
import numpy as np
import pytest
import torch

from tests import exact_inputs as ex

from .test_gpu_gemm3_triunit import CASES
from .test_gpu_gemm_f16x2 import SHAPES as F16X2_SHAPES

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
LOOPS = ["triunit", "chunk"]
CHUNK_ROWS = 64
BATCH2 = [(256, 256, 520, 0, False, False), (256, 256, 520, 1, False, False)]        # the batch-of-two case, both kinds
F16X2_BATCH3 = [(0, 128, 264, 520), (1, 512, 256, 512)]                               # padded-stride batch of three
F32_GRAM_SHAPES = [(128, 256), (300, 512), (1000, 776), (9000, 1024), (20000, 260)]   # test_gpu_fp32_activations.py


def _set_loop(monkeypatch, loop):
    if loop == "chunk":
        monkeypatch.setenv("QT_G3_LOOP", "chunk")
    else:
        monkeypatch.delenv("QT_G3_LOOP", raising=False)


def _block_tri(B):
    """Exact zeros above the block diagonal: B[k][n] = 0 for k < 256 * (n / 256) (the contract of tri)."""
    k, N = B.shape[-2:]
    return B * (np.arange(k)[:, None] >= 256 * (np.arange(N)[None, :] // 256))


def slab_rows(k, M, N, tj, tri):
    """First k row of every piece of tile column tj under kind 1, by the formula of g3_test_run:
    pieces = min(n / 2, max(1, 512 / (Tm Tn))), piece s = chunks [lo + n s / pieces, lo + n (s + 1) / pieces)."""
    Tm, Tn, nch = (M + 255) // 256, (N + 255) // 256, k // CHUNK_ROWS
    lo = 4 * tj if tri else 0
    n = nch - lo
    pieces = min(n // 2, max(1, 512 // (Tm * Tn)))
    return [CHUNK_ROWS * (lo + n * s // pieces) for s in range(pieces)]


def _c0(shape, seed, top):
    return np.random.default_rng(seed).integers(-top, top + 1, shape).astype(np.float32)


def _launch(ops, dev, A, B, C0, kind, call):
    """C0 - A^T B (kind 0) or A^T B over a NaN C (kind 1) through `call(At, Bt, C)`; [batch, ...] numpy in, device out."""
    At, Bt = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev)
    C = torch.from_numpy(C0.copy()).to(dev) if kind == 0 else torch.full(C0.shape, float("nan"), dtype=torch.float32, device=dev)
    call(At, Bt, C)
    torch.cuda.synchronize()
    return C


def _want(prod, C0, kind):
    return C0.astype(np.float64) - prod if kind == 0 else prod


def _abs_sum(A, B, C0, kind):
    s = np.einsum("bkm,bkn->bmn", np.abs(A).astype(np.float64), np.abs(B).astype(np.float64))
    return s + np.abs(C0) if kind == 0 else s


# ---- dense single-plane integers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("k,M,N,kind,tri,tight", CASES + BATCH2)
def test_gemm3_dense_integers(ops, dev, monkeypatch, k, M, N, kind, tri, tight, loop):
    """Path: gemm3_kernel<MODE, LOOP_TRI> (default) and <MODE, LOOP_CHUNK> (QT_G3_LOOP=chunk) on the nine shapes of
    test_gpu_gemm3_triunit.py -- kind 0 (whole tiles, C -= A^T B from an integer C0) and kind 1 (k split into slabs, the
    ordered reduction, C = A^T B over NaN), tri (tile column 1's k range starts at row 256; exact zeros above the block
    diagonal of B), tight (plane pitch 520: edge tiles clamp their loads) -- plus the batch of two in one launch; the
    plain shapes also through qt_gemm3_tn_f32.  Pins: a 16-row tri-unit, a 64-row chunk or a slab missing or doubled in
    the prologue / body / tail of either loop, a batch member reading its neighbour's planes.  Both loops must equal the
    integer reference, hence each other.  Exact: mid = lo = 0, sum |terms| <= 1000 + 9 * 512 < 2^24 in integers."""
    batch = 2 if (k, M, N, kind, tri, tight) in BATCH2 else 1
    A = ex.dense_ints((batch, k, M), seed=k + M + N + kind)
    B = ex.dense_ints((batch, k, N), seed=k + M + N + kind + 1)
    if tri:
        B = _block_tri(B).astype(np.float32)
    for X in (A, B):
        hi, mid, lo = ex.split_bf16x3(X)
        assert np.array_equal(hi, X) and not mid.any() and not lo.any()
    C0 = _c0((batch, M, N), 1, 1000)
    ex.assert_exactly_summable(_abs_sum(A, B, C0, kind), 0, "gemm3 dense")
    want = _want(np.einsum("bkm,bkn->bmn", A.astype(np.float64), B.astype(np.float64)), C0, kind)
    _set_loop(monkeypatch, loop)
    what = f"gemm3 k={k} {M}x{N} kind={kind} tri={tri} tight={tight} batch={batch} loop={loop}"
    if batch == 1:
        C = _launch(ops, dev, A, B, C0, kind, lambda a, b, c: ops.gemm3_tn_ex(a[0], b[0], c[0], kind, tri=tri, tight=tight))
    else:
        C = _launch(ops, dev, A, B, C0, kind, lambda a, b, c: ops.gemm3_tn_ex(a, b, c, kind, tri=tri, tight=tight))
    ex.assert_exact(C, want, what=what)
    if batch == 1 and not tri and not tight:
        C = _launch(ops, dev, A, B, C0, kind, lambda a, b, c: ops.gemm3_tn(a[0], b[0], c[0], kind))
        ex.assert_exact(C, want, what=what + " (qt_gemm3_tn_f32)")


F16X2_BOUNDS = [(2.0, 2.0), (4.0, 4.0), (8.0, 4.0), (4.0, 256.0), (256.0, 256.0)]     # (2, 2): integers +-{1, 2}


@pytest.mark.parametrize("ba,bb", F16X2_BOUNDS)
@pytest.mark.parametrize("kind,k,M,N", F16X2_SHAPES)
def test_f16x2_dense_integers(ops, dev, kind, k, M, N, ba, bb):
    """Path: gemm3_kernel<MODE, LOOP_DUO> on the three shapes of test_gpu_gemm_f16x2.py (SUB on whole tiles; ragged edge
    tiles in both directions; split-k SET through slabs), bounds the powers of two AT the largest |x| (2, with integers
    +-{1, 2}: entries exactly at the declared bound) and above it (4, 8, 2^6 x 4 for |x| <= 3).  Pins: a duo-unit missing or doubled, the scale exponents and the final unscale 2^-(11 + eA + eB)
    -- a wrong exponent multiplies every output by a power of two.  Exact: x 2^e is a single fp16 plane for every one
    of these bounds (lo' = 0), sum |terms| <= 1000 + 9 * 1024 < 2^24 in integers, all scalings powers of two."""
    A = ex.dense_ints((1, k, M), seed=k + M + N, top=min(3, int(ba)))
    B = ex.dense_ints((1, k, N), seed=k + M + N + 1, top=min(3, int(bb)))
    for X, bound in ((A, ba), (B, bb)):
        assert np.abs(X).max() <= bound and not ex.split_f16x2(X, bound)[1].any()
    C0 = _c0((1, M, N), 2, 1000)
    ex.assert_exactly_summable(_abs_sum(A, B, C0, kind), 0, "f16x2 dense")
    want = _want(np.einsum("bkm,bkn->bmn", A.astype(np.float64), B.astype(np.float64)), C0, kind)
    C = _launch(ops, dev, A, B, C0, kind, lambda a, b, c: ops.gemm3_tn_f16x2(a[0], b[0], c[0], ba, bb, kind=kind))
    ex.assert_exact(C, want, what=f"f16x2 kind={kind} k={k} {M}x{N} bounds=({ba}, {bb})")


@pytest.mark.parametrize("kind,k,M,N", F16X2_BATCH3)
def test_f16x2_dense_integers_batch_of_three_at_padded_strides(ops, dev, kind, k, M, N):
    """Path: LOOP_DUO with three problems in one launch at padded batch strides (A rows k + 8, B rows k + 4, C rows
    M + 1), each with its own bounds, i.e. its own scale exponents.  Pins: a problem read at the unpadded stride or
    unscaled with its neighbour's exponents; the pad rows of C (NaN) must stay.  Exact: as the single problem."""
    n = 3
    ba, bb = [4.0, 8.0, 256.0], [4.0, 256.0, 4.0]
    A = ex.dense_ints((n, k, M), seed=31)
    B = ex.dense_ints((n, k, N), seed=32)
    C0 = _c0((n, M, N), 3, 1000)
    ex.assert_exactly_summable(_abs_sum(A, B, C0, kind), 0, "f16x2 batch")
    want = _want(np.einsum("bkm,bkn->bmn", A.astype(np.float64), B.astype(np.float64)), C0, kind)
    Ab = torch.full((n, k + 8, M), 3.0, dtype=torch.float32, device=dev)[:, :k]
    Bb = torch.full((n, k + 4, N), 3.0, dtype=torch.float32, device=dev)[:, :k]
    Cfull = torch.full((n, M + 1, N), float("nan"), dtype=torch.float32, device=dev)
    Cb = Cfull[:, :M]
    Ab.copy_(torch.from_numpy(A))
    Bb.copy_(torch.from_numpy(B))
    if kind == 0:
        Cb.copy_(torch.from_numpy(C0))
    assert Ab.stride(0) == (k + 8) * M and Cb.stride(0) == (M + 1) * N
    ops.gemm3_tn_f16x2(Ab, Bb, Cb, ba, bb, kind=kind)
    torch.cuda.synchronize()
    ex.assert_exact(Cb, want, what=f"f16x2 batch of three kind={kind}")
    assert bool(torch.isnan(Cfull[:, M]).all()), "the pad row behind a problem's C was written"


def _gram_start(K, dev, seed, top):
    g = torch.Generator().manual_seed(seed)
    G0 = torch.randint(-top, top + 1, (K, K), generator=g).float().to(dev)
    lower, untouched = ex.gram_masks(K, dev)
    return G0, lower, untouched


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("n,K", F32_GRAM_SHAPES)
def test_f32_gram_dense_integers(ops, dev, monkeypatch, n, K, loop):
    """Path: qt_xtx_accumulate_f32 (gemm3_kernel<G3_ADD, *>, both loops) on the five shapes of
    test_gpu_fp32_activations.py -- one token chunk, ragged tokens (rows zero-padded to a multiple of 128), K not a
    multiple of 256 (edge tiles, padded plane pitch) or of 8, two and three chunks of 8192 tokens (a full-chunk and a
    last-chunk item table) -- G0 integers |g| <= 1000 with NaN in the tiles above the diagonal tile row, called twice.
    Pins: a token chunk or its ragged end dropped or counted twice, stale plane rows behind a short last chunk, a tile
    outside the lower triangle written.  Exact: single-plane integers, sum |terms| <= 1000 + 2 * 9 * 20000 < 2^24."""
    _set_loop(monkeypatch, loop)
    X = torch.from_numpy(ex.dense_ints((n, K), seed=n + K)).to(dev)
    G0, lower, untouched = _gram_start(K, dev, n, 1000)
    ex.assert_exactly_summable(1000 + 2 * 9 * n, 0, "f32 Gram dense")
    ref = X.double().t() @ X.double()
    G = torch.where(untouched, torch.full_like(G0, float("nan")), G0)
    for calls in (1, 2):
        ops.xtx_accumulate_f32(X, G)
        torch.cuda.synchronize()
        ex.assert_exact(G, G0.double() + calls * ref, region=lower, untouched=untouched,
                        what=f"f32 Gram tokens={n} K={K} loop={loop}, call {calls}", gram=True)


# ---- sparse multi-plane columns --------------------------------------------------------------------------------------
def _sparse_problem(k, M, N, kind, tri, planes, seed):
    """A, B [k, *] dense single-plane integers with three multi-plane columns each, -> (A, B, rows of A's, columns of
    B's multi-plane columns).  k rows of the entries: the first and last row of a 16-row unit (0, 15, 16), a chunk
    boundary (63, 64), the last row, a slab boundary of kind 1 (its last row before and first row after) and, for tri,
    the first row of tile column 1's range (256) and the row before it."""
    A = ex.dense_ints((k, M), seed=seed)
    B = ex.dense_ints((k, N), seed=seed + 1)
    if tri:
        B = _block_tri(B).astype(np.float32)
    edge = slab_rows(k, M, N, 0, tri)[1] if kind == 1 else (256 if tri else 48)
    assert 48 <= edge < k
    sets_a = [(0, 15, 16), (63, 64, k - 1), (edge - 1, edge, 31)]
    cols_a = [1, min(M, 256) - 126, M - 1]
    cols_b = [2, min(N, 256) - 61, N - 3]
    for c, pos in zip(cols_a, sets_a):
        A[:, c], _ = ex.multi_plane_column(k, pos, seed + c, planes)
    for c in cols_b:
        base = 256 * (c // 256) if tri else 0        # a tri column is zero above its block
        edge_b = slab_rows(k, M, N, c // 256, tri)[1] if kind == 1 else base + 64
        pos = (base, base + 15, base + 16) if c != cols_b[1] else (edge_b - 1, edge_b, k - 1)
        B[:, c], _ = ex.multi_plane_column(k, pos, seed + 7 * c, planes)
    return A, B, cols_a, cols_b


def _check_sparse(C, A, B, C0, kind, kept, cols_a, cols_b, q, what):
    """Equality with the kept-product reference everywhere but where two multi-plane columns meet; there the bound
    16 * 2^-24 * sum |a||b| (C0 is zero there)."""
    M, N = C0.shape
    pair = np.zeros((M, N), dtype=bool)
    pair[np.ix_(cols_a, cols_b)] = True
    multi = np.zeros((M, N), dtype=bool)
    multi[cols_a, :] = True
    multi[:, cols_b] = True
    s = _abs_sum(A[None], B[None], C0[None], kind)[0]
    ex.assert_exactly_summable(s[multi & ~pair], q, what + ": multi-plane outputs")
    ex.assert_exactly_summable(s[~multi], 0, what + ": integer outputs")
    want = _want(kept, C0, kind)
    ex.assert_exact(C, want, region=~pair, what=what)
    got = C.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)[pair]
    assert np.isfinite(got[pair]).all() and (err <= 16 * EPS * s[pair]).all(), (what, float((err / s[pair]).max()) / EPS)


def _sparse_c0(M, N, cols_a, cols_b, seed):
    C0 = _c0((M, N), seed, 20)
    C0[np.ix_(cols_a, cols_b)] = 0
    return C0


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("k,M,N,kind,tri,tight", CASES)
def test_gemm3_sparse_multi_plane_columns(ops, dev, monkeypatch, k, M, N, kind, tri, tight, loop):
    """Path: both loops of gemm3_kernel on the nine triunit shapes (kind 0 / 1, tri, tight), three multi-plane columns in
    A (B's other columns single-plane) and three in B: A's pin lo*hi, mid*hi, hi*hi, B's pin hi*lo, hi*mid; their entries
    sit on the first / last k row of a tri-unit, a chunk boundary, the last k row, a slab boundary (kind 1) and the first
    row of tile column 1's range (tri).  Pins: one plane product skipped, run twice or taken from the wrong plane (its
    weight is 2^-9 or 2^-18 of the entry: invisible to a magnitude bar), a plane read one unit off.  Exact: terms are
    multiples of 2^-18 and |C0| + sum |a||b| <= 20 + 3 * 2.01 * 3 < 2^6, so every partial sum has < 24 bits; kind 0's
    final C0 - acc likewise.  The 9 outputs where two multi-plane columns meet: 16 * 2^-24 * sum |a||b|."""
    A, B, cols_a, cols_b = _sparse_problem(k, M, N, kind, tri, "bf16x3", seed=k + M + N)
    C0 = _sparse_c0(M, N, cols_a, cols_b, 5)
    kept = ex.kept_products_bf16x3(A, B)
    single = np.ones((M, N), dtype=bool)
    single[np.ix_(cols_a, cols_b)] = False
    full = A.astype(np.float64).T @ B.astype(np.float64)
    assert np.array_equal(kept[single], full[single])          # every plane of a lone multi-plane column is kept
    _set_loop(monkeypatch, loop)
    C = _launch(ops, dev, A[None], B[None], C0[None], kind,
                lambda a, b, c: ops.gemm3_tn_ex(a[0], b[0], c[0], kind, tri=tri, tight=tight))[0]
    _check_sparse(C, A, B, C0, kind, kept, cols_a, cols_b, 18,
                  f"gemm3 sparse k={k} {M}x{N} kind={kind} tri={tri} tight={tight} loop={loop}")


@pytest.mark.parametrize("ba,bb", [(4.0, 4.0), (256.0, 4.0)])
@pytest.mark.parametrize("kind,k,M,N", F16X2_SHAPES)
def test_f16x2_sparse_two_plane_columns(ops, dev, kind, k, M, N, ba, bb):
    """Path: LOOP_DUO on the three f16x2 shapes with entries a + b 2^-12 (planes hi = a 2^e and lo' = b 2^(e - 1)), at
    the tight bounds and with A's bound 2^6 too loose.  A's multi-plane columns pin lo'_a hi_b and hi_a hi_b, B's pin
    hi_a lo'_b.  Pins: one of the three products skipped or doubled, the 2^11 between the hi*hi product and the mixed
    ones, the unscale.  Exact: terms are multiples of 2^-12 and |C0| + sum |a||b| < 2^6 <= 2^12; the scalings are powers
    of two.  Where two multi-plane columns meet (lo'*lo' = 2^-24 of the term is dropped): 16 * 2^-24 * sum |a||b|."""
    A, B, cols_a, cols_b = _sparse_problem(k, M, N, kind, False, "f16x2", seed=k + M + N)
    assert np.abs(A).max() <= ba and np.abs(B).max() <= bb
    C0 = _sparse_c0(M, N, cols_a, cols_b, 6)
    kept = ex.kept_products_f16x2(A, B, ba, bb)
    single = np.ones((M, N), dtype=bool)
    single[np.ix_(cols_a, cols_b)] = False
    full = A.astype(np.float64).T @ B.astype(np.float64)
    assert np.array_equal(kept[single], full[single])
    C = _launch(ops, dev, A[None], B[None], C0[None], kind,
                lambda a, b, c: ops.gemm3_tn_f16x2(a[0], b[0], c[0], ba, bb, kind=kind))[0]
    _check_sparse(C, A, B, C0, kind, kept, cols_a, cols_b, 12, f"f16x2 sparse kind={kind} k={k} {M}x{N} bounds=({ba}, {bb})")


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("n,K", F32_GRAM_SHAPES)
def test_f32_gram_sparse_multi_plane_columns(ops, dev, monkeypatch, n, K, loop):
    """Path: qt_xtx_accumulate_f32 (gemm3_kernel<G3_ADD, *>, both loops, with A = B = the planes of X) on the five
    fp32-Gram shapes; three columns of X are multi-plane, the other columns play the single-plane operand: G[i][j] with exactly
    one multi-plane index pins lo*hi, mid*hi (i multi-plane) and hi*lo, hi*mid (j multi-plane).  Their entries sit at
    token 0, 15, 16, 63, 64, the last token and, past 8192 tokens, on both sides of the token-chunk boundary.  Pins: a
    plane product of the Gram skipped or doubled, a token chunk reading stale planes.  Exact: terms are multiples of
    2^-18, |G0| + sum |x_i x_j| <= 20 + 3 * 2.01 * 3 < 2^6.  Entries where two multi-plane columns meet (the diagonal
    ones included): 16 * 2^-24 * sum |x_i x_j|."""
    _set_loop(monkeypatch, loop)
    X = ex.dense_ints((n, K), seed=n + K)
    cols = [1, K // 2 + 3, K - 2]
    edge = 8192 if n > 8192 else 32
    for c, pos in zip(cols, [(0, 15, 16), (63, 64, n - 1), (edge - 1, edge, 48)]):
        X[:, c], _ = ex.multi_plane_column(n, pos, n + c, "bf16x3")
    kept = ex.kept_products_bf16x3(X, X)
    s = np.abs(X).astype(np.float64).T @ np.abs(X).astype(np.float64)
    pair = np.zeros((K, K), dtype=bool)
    pair[np.ix_(cols, cols)] = True
    multi = np.zeros((K, K), dtype=bool)
    multi[cols, :] = True
    multi[:, cols] = True
    G0, lower, untouched = _gram_start(K, dev, n + 1, 20)
    G0[torch.from_numpy(pair).to(dev)] = 0
    g0 = G0.cpu().numpy().astype(np.float64)
    ex.assert_exactly_summable((np.abs(g0) + s)[multi & ~pair], 18, "f32 Gram sparse: multi-plane outputs")
    ex.assert_exactly_summable((np.abs(g0) + s)[~multi], 0, "f32 Gram sparse: integer outputs")
    G = torch.where(untouched, torch.full_like(G0, float("nan")), G0)
    ops.xtx_accumulate_f32(torch.from_numpy(X).to(dev), G)
    torch.cuda.synchronize()
    want = g0 + kept
    ex.assert_exact(G, want, region=lower & ~torch.from_numpy(pair).to(dev), untouched=untouched,
                    what=f"f32 Gram sparse tokens={n} K={K} loop={loop}", gram=True)
    low_pair = pair & np.tril(np.ones((K, K), dtype=bool))
    got = G.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)[low_pair]
    assert (err <= 16 * EPS * s[low_pair]).all(), float((err / s[low_pair]).max()) / EPS
