"""``qt_xtx_accumulate`` and ``qt_xtx_dot`` on exactly summable inputs: the result must equal the integer reference bit
for bit, so one missing, doubled or misplaced product fails -- wherever it lands and however small it is beside the
sum (the magnitude bars of test_gpu_kernels.py / test_gpu_fp16.py cannot see such a term).

Inputs (tests/exact_inputs.py): activations in +-{1, 2, 3} (exact in bf16 and fp16, never zero), or one nonzero token
row of wide-exponent values.  Every case calls ``assert_exactly_summable`` on its own inputs before it launches:
sum |terms| < 2^24 per output, so every fp32 partial sum in every order is an integer below 2^24, i.e. exact.

Every Gram case starts G from random integers |g| <= 1000 (accumulate semantics), with NaN in every 256 x 256 tile
strictly above the diagonal tile row (quantool_amd.h: "lower triangle incl. diagonal tiles": those tiles must still hold
NaN afterwards); the upper half of the diagonal tiles is not asserted.  Reference: the fp64 product of the same
integers on the device (exact below 2^53).

Out of reach at these sizes: the throttled ``xtx_kernel<..., THROTTLE=true>`` instances need more than 1 GiB of X (and
four whole rounds of tiles); test_gpu_edges.py::test_llama3_70b_down_proj_hessian_size remains their only cover.
"""
import numpy as np
import pytest
import torch

from tests import exact_inputs as ex

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
SHAPES = ["16", "32"]


def _dev_x(x_np, dtype, dev, pad=0):
    """The activations on the device; pad > 0: a column range of a wider tensor whose other columns hold 3 (a read
    past K would show), row pitch K + pad."""
    X = torch.from_numpy(x_np).to(dtype).to(dev)
    if pad:
        wide = torch.full((X.shape[0], X.shape[1] + pad), 3.0, dtype=dtype, device=dev)
        wide[:, :X.shape[1]] = X
        X = wide[:, :X.shape[1]]
        assert X.stride(0) == X.shape[1] + pad or X.shape[0] == 1
    return X


def _start(K, dev, seed):
    """(G0 integers |g| <= 1000, G = G0 with NaN in the tiles above the diagonal tile row, lower, untouched)"""
    g = torch.Generator().manual_seed(seed)
    G0 = torch.randint(-1000, 1001, (K, K), generator=g).float().to(dev)
    lower, untouched = ex.gram_masks(K, dev)
    G = torch.where(untouched, torch.full_like(G0, float("nan")), G0)
    return G0, G, lower, untouched


def _twice_exact(ops, X, ref, dev, what, seed=0):
    """G0 + X^T X after one call and G0 + 2 X^T X after the second, exactly, with the NaN tiles untouched."""
    K = X.shape[-1]
    G0, G, lower, untouched = _start(K, dev, seed)
    x64 = X.reshape(-1, K).double().abs()
    ex.assert_exactly_summable(G0.double().abs() + 2 * (x64.t() @ x64), 0, what)
    for calls in (1, 2):
        ops.xtx_accumulate(X, G)
        torch.cuda.synchronize()
        ex.assert_exact(G, G0.double() + calls * ref, region=lower, untouched=untouched, what=f"{what}, call {calls}",
                        gram=True)
    return G


def _ref(X):
    x64 = X.reshape(-1, X.shape[-1]).double()
    return x64.t() @ x64


# (tokens, K, pitch pad): the smallest shapes that reach each path of xtx_plan / qt_xtx_accumulate
TAIL_ONLY = [(1, 8, 0), (17, 8, 0), (63, 264, 0)]
DIRECT = [(64, 256, 0), (200, 520, 0), (448, 1032, 0)]
SLABS_EQUAL = [(512, 264, 0), (2048, 256, 0)]
SLABS_RAGGED = [(576, 264, 0), (530, 264, 0), (2112 + 5, 520, 0)]
PITCHED_FULL = [(512, 264, 8)]
PITCHED_TAIL = [(70, 264, 8), (40, 264, 64), (530, 264, 8)]


def _case(ops, dev, monkeypatch, n, K, pad, dtype, shape):
    monkeypatch.setenv("QT_XTX_SHAPE", shape)
    X = _dev_x(ex.dense_ints((n, K), seed=n + K + pad), dtype, dev, pad)
    _twice_exact(ops, X, _ref(X), dev, f"tokens={n} K={K} pad={pad} {dtype} shape {shape}", seed=n + K)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,K,pad", TAIL_ONLY)
def test_tail_only(ops, dev, monkeypatch, n, K, pad, dtype, shape):
    """Path: n_tt = 1 with has_tail -- every unit of every item comes from the zero-padded staging (d_tail = 0), one
    direct launch; K = 8 clamps every panel load to column 0.  Pins: a tail row dropped or read twice, a staging row
    that is not zero, the clamp / store mask of the edge tile.  Exact: sum |terms| <= 1000 + 2 * 9 * 63 < 2^24."""
    assert ex.xtx_plan(n, K)["n_tt"] == 1 and ex.xtx_plan(n, K)["has_tail"] == 1
    _case(ops, dev, monkeypatch, n, K, pad, dtype, shape)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,K,pad", DIRECT)
def test_direct_items_without_slabs(ops, dev, monkeypatch, n, K, pad, dtype, shape):
    """Path: n_tt < 8, so xtx_plan keeps s2 = 1 -- every tile a direct item over all tokens, added into G from the
    epilogue; K = 520 and 1032 have a ragged last panel of 8 columns; (200, 520) ends in the tail staging.  Pins: a
    token or a 16-token unit missing or doubled in the ring's prologue / steady loop / drain, a product stored at
    the wrong (i, j), an edge tile's mask.  Exact: sum |terms| <= 1000 + 2 * 9 * 448 < 2^24."""
    assert ex.xtx_plan(n, K)["s2"] == 1 and ex.xtx_plan(n, K)["n_tt"] < 8
    _case(ops, dev, monkeypatch, n, K, pad, dtype, shape)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,K,pad", SLABS_EQUAL + SLABS_RAGGED)
def test_token_chunk_slabs(ops, dev, monkeypatch, n, K, pad, dtype, shape):
    """Path: fewer tiles than one round, n_tt >= 8 -- every tile is split over s2 token chunks into fp32 slabs that
    xtx_reduce_kernel sums in order: (512, 264) S = 2 and (2048, 256) S = 8 with equal chunks; (576, 264) chunks of 5 and
    4 token tiles; (530, 264) and (2117, 520) a ragged split whose last chunk ends in the tail staging.  Pins: a token
    tile lost or doubled at a chunk boundary (the base / remainder formula of xtx_item), a slab left out of or counted
    twice in the reduction, a slab written to another tile's slot.  Exact: sum |terms| <= 1000 + 2 * 9 * 2117 < 2^24."""
    pl = ex.xtx_plan(n, K)
    assert pl["s2"] > 1 and pl["n_direct"] == 0
    if (n, K) == (576, 264):
        assert [(b - a) // 64 for a, b in ex.xtx_chunks(n, K)] == [5, 4]
    _case(ops, dev, monkeypatch, n, K, pad, dtype, shape)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,K,pad", PITCHED_FULL + PITCHED_TAIL)
def test_pitched_rows(ops, dev, monkeypatch, n, K, pad, dtype, shape):
    """Path: ldx != K.  (512, 264, K + 8): full token tiles only, one launch at the caller's pitch.  (70, 264, K + 8):
    has_tail && ldx != K -- two launches, the 64 full rows at pitch ldx, then the staged tail at pitch K.  (40, 264,
    K + 64): full == 0, the second launch alone.  (530, 264, K + 8): the first launch runs the slab plan of the 512 full
    rows (S = 2) inside the slab area sized for the whole call.  The pad columns hold 3, so a row read at the wrong
    pitch changes the integers.  Pins: the pitch of either launch, the 2-D copy into the staging, tokens counted by both
    launches or by neither.  Exact: sum |terms| <= 1000 + 2 * 9 * 530 < 2^24."""
    _case(ops, dev, monkeypatch, n, K, pad, dtype, shape)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_d_input(ops, dev, monkeypatch, dtype, shape):
    """Path: X [4, 96, 256] flattened to 384 tokens by the wrapper: one tile, direct, no tail.  Pins: the leading
    dimensions' flattening (a sample dropped or its rows strided).  Exact: sum |terms| <= 1000 + 2 * 9 * 384 < 2^24."""
    monkeypatch.setenv("QT_XTX_SHAPE", shape)
    X = _dev_x(ex.dense_ints((4 * 96, 256), seed=4), dtype, dev).reshape(4, 96, 256)
    _twice_exact(ops, X, _ref(X), dev, f"[4, 96, 256] {dtype} shape {shape}")


# ---- whole rounds plus a slabbed remainder ---------------------------------------------------------------------------
BIG_N, BIG_K = 529, 5640


@pytest.fixture(scope="module")
def big(ops, dev):
    """X, its fp64 Gram and the result of the default settings (kept on the device; the only large G, 127 MB)."""
    pl = ex.xtx_plan(BIG_N, BIG_K)
    assert (pl["n_tiles"], pl["n_direct"], pl["n_rem"], pl["s2"], pl["has_tail"]) == (276, 256, 20, 2, 1)
    X = _dev_x(ex.dense_ints((BIG_N, BIG_K), seed=11), torch.bfloat16, dev)
    ref = _ref(X)
    with pytest.MonkeyPatch.context() as mp:
        for v in ("QT_XTX_SHAPE", "QT_XTX_ORDER", "QT_XTX_MAP"):
            mp.delenv(v, raising=False)
        G = _twice_exact(ops, X, ref, dev, "K=5640 default", seed=12)
    lower, _ = ex.gram_masks(BIG_K, dev)
    return X, ref, torch.where(lower, G, torch.zeros_like(G))


@pytest.mark.parametrize("env", [{}, {"QT_XTX_SHAPE": "16"}, {"QT_XTX_SHAPE": "32"}, {"QT_XTX_ORDER": "0"},
                                 {"QT_XTX_ORDER": "1"}, {"QT_XTX_ORDER": "2"}, {"QT_XTX_MAP": "1"}],
                         ids=lambda e: "-".join(f"{k[7:].lower()}{v}" for k, v in e.items()) or "default")
def test_whole_round_plus_slabbed_remainder(ops, dev, monkeypatch, big, env):
    """Path: K = 5640 is 23 panels = 276 tiles >= 256: one whole round of direct items (n_direct = 256) and 20 tiles
    split over S = 2 token chunks (5 + 4 token tiles, the last ending in the tail staging); the last panel is 8 columns
    wide.  Run with the defaults, with each MFMA shape, each tile-table walk (QT_XTX_ORDER 0 / 1 / 2) and the identity
    workgroup map (QT_XTX_MAP=1).  Pins: a tile missing from or listed twice in a table, xtx_logical's round / XCD
    arithmetic sending two workgroups to one item, the reduction reading tile_tab + n_direct.  All settings must give
    the integer reference, hence the default's bits.  Exact: sum |terms| <= 1000 + 2 * 9 * 529 < 2^24."""
    X, ref, G_default = big
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    G = _twice_exact(ops, X, ref, dev, f"K=5640 {env}", seed=12)
    lower, _ = ex.gram_masks(BIG_K, dev)
    assert torch.equal(torch.where(lower, G, torch.zeros_like(G)), G_default)


# ---- sweep -----------------------------------------------------------------------------------------------------------
SWEEP_TOKENS = (1, 15, 16, 17, 63, 64, 65, 127, 129, 257, 513)


def test_sweep_of_small_k_and_token_counts(ops, dev):
    """Path: every K in 8, 16, ..., 520 (one to three panels, every width of the last one) times the token counts
    around the unit (16), the double (32), the token tile (64) and the first slab split (513 = 8 full tiles + a tail):
    tail-only, direct and slabbed plans, bf16, default MFMA shape, one call each.  Pins: an edge-tile clamp or store
    mask that is wrong for one panel width only, a prologue / drain that is wrong for one short length only.  The fp64
    reference is computed once per K, as the running sum of the Grams of the token segments between two counts.
    Exact: sum |terms| <= 1000 + 9 * 513 < 2^24."""
    ex.assert_exactly_summable(1000 + 9 * max(SWEEP_TOKENS), 0, "sweep")
    for K in range(8, 521, 8):
        X = _dev_x(ex.dense_ints((max(SWEEP_TOKENS), K), seed=K), torch.bfloat16, dev)
        x64 = X.double()
        G0, Gnan, lower, untouched = _start(K, dev, K)
        ref = G0.double()
        prev = 0
        for n in SWEEP_TOKENS:
            ref = ref + x64[prev:n].t() @ x64[prev:n]
            prev = n
            G = Gnan.clone()
            ops.xtx_accumulate(X[:n], G)
            ex.assert_exact(G, ref, region=lower, untouched=untouched, what=f"sweep tokens={n} K={K}", gram=True)


# ---- one-hot tokens --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,K", [(530, 264), (2117, 520)])
def test_one_hot_token_at_every_boundary(ops, dev, monkeypatch, n, K, dtype, shape):
    """Path: the ragged slab plans of (530, 264) (S = 2) and (2117, 520) (S = 8), with ONE nonzero token row of seeded
    values (bf16: exponents over 2^+-20, fp16: over 2^+-7) placed at token 0, 15, 16, 63, 64, the first and last token
    of every slab chunk (xtx_item's formula, restated in exact_inputs.xtx_chunks), the first tail token and the last
    token.  G starts at zero (NaN in the tiles that must stay untouched), so every lower entry must be
    fp32(x_i) * fp32(x_j).  Pins: that token's row being skipped, read twice or read from a neighbour's address, and
    any rounding of the operands or the product on the way.  Exact: one nonzero term per output whose product has at
    most 16 / 22 significant bits and is normal in fp32 (checked on the reference); 0 + t is exact."""
    monkeypatch.setenv("QT_XTX_SHAPE", shape)
    lower, untouched = ex.gram_masks(K, dev)
    positions = ex.xtx_probe_tokens(n, K)
    chunks = ex.xtx_chunks(n, K)
    assert len(chunks) > 1 and all(t0 in positions and t1 - 1 in positions for t0, t1 in chunks)
    X = torch.zeros((n, K), dtype=dtype, device=dev)
    for t in positions:
        row = ex.one_hot_token(1, K, 0, dtype, seed=t + K)[0]
        prod = np.outer(row.astype(np.float64), row.astype(np.float64))
        p32 = prod.astype(np.float32)
        assert np.array_equal(p32.astype(np.float64), prod) and (np.abs(p32) >= np.finfo(np.float32).tiny).all()
        X.zero_()
        X[t] = torch.from_numpy(row).to(dtype).to(dev)
        G = torch.where(untouched, torch.full((K, K), float("nan"), device=dev), torch.zeros((K, K), device=dev))
        ops.xtx_accumulate(X, G)
        ex.assert_exact(G, torch.from_numpy(prod), region=lower, untouched=untouched,
                        what=f"one-hot token {t} of {n}, K={K} {dtype} shape {shape}", gram=True)


# ---- HessianAccumulator ----------------------------------------------------------------------------------------------
def test_accumulator_paths_are_exactly_equal(ops, dev):
    """Path: the calling pattern of test_per_sample_staging_matches_single_launch -- one launch over all 3840 tokens,
    the staged path (40 samples of 96 tokens through a 1024-token buffer: several flushes, the last on reading G) and
    the direct path behind two staged samples -- with integer activations.  Pins: a staged sample lost, flushed twice
    or flushed with rows of an earlier fill.  Exact: sum |terms| <= 9 * 3840 < 2^24, so all three must equal the
    integer reference, hence each other, on the lower triangle; n must be the sample count."""
    from quantool_amd.engine.gptq_linear import HessianAccumulator

    S, T, K = 40, 96, 520
    X = _dev_x(ex.dense_ints((S * T, K), seed=5), torch.bfloat16, dev).reshape(S, T, K)
    ref = _ref(X)
    ex.assert_exactly_summable(9 * S * T, 0, "accumulator")
    lower, _ = ex.gram_masks(K, dev)
    one = HessianAccumulator(K, dev, stage_tokens=0)
    one.add(X)
    staged = HessianAccumulator(K, dev, stage_tokens=1024)
    for i in range(S):
        staged.add(X[i:i + 1])
    assert staged._fill > 0
    big = HessianAccumulator(K, dev, stage_tokens=512)
    big.add(X[:2].reshape(-1, K), num_samples=2)
    big.add(X[2:].reshape(-1, K), num_samples=S - 2)
    results = [acc.G for acc in (one, staged, big)]
    assert staged._fill == 0 and one.n == staged.n == big.n == S
    for name, G in zip(("single launch", "staged", "direct behind staged"), results):
        ex.assert_exact(G, ref, region=lower, what=f"HessianAccumulator, {name}", gram=True)
    zero = torch.zeros_like(results[0])
    assert torch.equal(torch.where(lower, results[0], zero), torch.where(lower, results[1], zero))
    assert torch.equal(torch.where(lower, results[0], zero), torch.where(lower, results[2], zero))


# ---- qt_xtx_dot ------------------------------------------------------------------------------------------------------
def dot_case(n, K):
    """-> (X int64 [n, K], H int64 symmetric [K, K], the integer <H, X^T X>), with the guard of every stage:
    * the only fp32 step is the MFMA accumulator of an item (a tile, or a token chunk of one): sum |x_i x_j| <= 9 n
      < 2^24, exact;
    * the epilogue multiplies (double)H * (double)acc, doubles the off-diagonal entries and sums registers, lanes,
      waves and finally the items (sum_partials_kernel) in fp64: integers whose sum of magnitudes stays below 2^53,
      exact in any order -- so H can be DENSE (every entry of every tile is weighed, not a sample of them);
    * (float)(red[0] * scale) with scale a power of two is exact when |integer| < 2^24; with accumulate, out + v is
      exact when |out0| + |v| is below 2^24 in the same unit.  Both are asserted on the integers here."""
    X = ex.dense_ints((n, K), seed=n + K).astype(np.int64)
    H = ex.dense_ints((K, K), seed=n * K).astype(np.int64)
    H = np.tril(H) + np.tril(H, -1).T
    xf = X.astype(np.float64)                                        # BLAS products of integers below 2^53: exact
    G = (xf.T @ xf).astype(np.int64)
    ex.assert_exactly_summable(9 * n, 0, "xtx_dot: accumulator")
    assert 2 * int((np.abs(H) * (np.abs(xf).T @ np.abs(xf)).astype(np.int64)).sum()) < 2 ** 53
    total = int((H * G).sum())
    return X, H, total


DOT_OUT0 = 4097            # start value of the accumulate case, in units of the scale


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [256, 520, 1032])
@pytest.mark.parametrize("n", [64, 256, 1024])
def test_xtx_dot_equals_the_integer_contraction(ops, dev, n, K, dtype):
    """Path: xtx16_kernel<F16, DOT=true> over the usual plan (n = 64 / 256: whole tiles; n = 1024: every tile cut into
    token chunks, each item one fp64 partial) and sum_partials_kernel, accumulate off and on, scale = 2^-3.  Pins: an
    item's partial missing or doubled, the lower-triangle mask and the doubling of the off-diagonal entries (dense H),
    the ragged panel's mask, accumulate overwriting or a plain call adding.  Exact: see dot_case -- fp32 only inside the
    accumulator (9 n < 2^24), fp64 integers below 2^53 after it, |result| + |start| < 2^24 for the final conversion."""
    Xi, Hi, total = dot_case(n, K)
    ex.assert_exactly_summable(abs(total) + DOT_OUT0, 0, "xtx_dot: result")
    if n == 1024:
        assert ex.xtx_plan(n, K)["s2"] > 1
    scale = 2.0 ** -3
    X = torch.from_numpy(Xi.astype(np.float32)).to(dtype).to(dev)
    H = torch.from_numpy(Hi.astype(np.float32)).to(dev)
    out = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    ops.xtx_dot(X, H, scale=scale, out=out, accumulate=False)
    assert float(out.item()) == total * scale, (float(out.item()), total * scale)
    out.fill_(DOT_OUT0 * scale)
    ops.xtx_dot(X, H, scale=scale, out=out, accumulate=True)
    assert float(out.item()) == (DOT_OUT0 + total) * scale, (float(out.item()), (DOT_OUT0 + total) * scale)
    # the strictly upper triangle of H is never read: NaN there changes nothing
    Hn = torch.where(torch.triu(torch.ones_like(H, dtype=torch.bool), 1), torch.full_like(H, float("nan")), H)
    ops.xtx_dot(X, Hn, scale=scale, out=out, accumulate=False)
    assert float(out.item()) == total * scale
