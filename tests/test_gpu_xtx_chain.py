"""``chain_tokens``: the Gram kernels fold their accumulators into G (or their slab) every F tokens of a work item and
start again (``qt_xtx_accumulate_chained`` / ``qt_xtx_accumulate_batched_chained``).

* exact sums (tests/exact_inputs.py): a token dropped or counted twice at a cut, a flush that does not zero the
  accumulators, a slab's first flush adding into stale memory and the tail staging after a cut all change integers;
* the bit definition on random data: a tile with one owner equals the plain calls over the F-token slices in order,
  a split tile equals the fp32 fold of its spans and chunks;
* no cut inside the call: the plain call's bits;
* the batched form; the throttled kernel (the only large case); the workspace bound;
* precision, the point of it: against the fp64 Gram, at most half the plain launch's error and below 1e-5.
"""
import ctypes

import pytest
import torch

from tests import exact_inputs as ex

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
SHAPE_ENVS = [None, "16", "32"]
BIG_K, BIG_N = 5640, 2000 + 17
STEP = 640


def _shape_env(monkeypatch, shape):
    if shape is None:
        monkeypatch.delenv("QT_XTX_SHAPE", raising=False)
    else:
        monkeypatch.setenv("QT_XTX_SHAPE", shape)


def _start(K, dev, seed):
    """(G0 integers |g| <= 1000, G = G0 with NaN in the tiles above the diagonal tile row, lower, untouched)"""
    g = torch.Generator().manual_seed(seed)
    G0 = torch.randint(-1000, 1001, (K, K), generator=g).float().to(dev)
    lower, untouched = ex.gram_masks(K, dev)
    return G0, torch.where(untouched, torch.full_like(G0, float("nan")), G0), lower, untouched


def _ref(X):
    """fp64 Gram on the device, in row chunks (exact for integer inputs below 2^53)"""
    K = X.shape[1]
    out = torch.zeros((K, K), dtype=torch.float64, device=X.device)
    for t0 in range(0, X.shape[0], 8192):
        x64 = X[t0:t0 + 8192].double()
        out.addmm_(x64.t(), x64)
    return out


def _tile_mask(K, tiles, dev):
    """bool [K, K]: the entries of the listed (ti, tj) tiles that lie in the lower triangle"""
    nt = (K + ex.TILE - 1) // ex.TILE
    grid = torch.zeros((nt, nt), dtype=torch.bool)
    for ti, tj in tiles:
        grid[ti, tj] = True
    idx = torch.arange(K, device=dev) // ex.TILE
    lower, _ = ex.gram_masks(K, dev)
    return grid.to(dev)[idx[:, None], idx[None, :]] & lower


def _single_plan(ops, n, K):
    """(direct tiles, {slabbed tile: [(t0, t1) token ranges of its chunks, ascending]}) of the single launch"""
    items, _ = ops.xtx_batched_plan([n], K)
    direct = [(ti, tj) for _, ti, tj, _, _, slab in items if slab < 0]
    slabbed = {}
    for _, ti, tj, tt0, cnt, slab in items:
        if slab >= 0:
            slabbed.setdefault((ti, tj), []).append((tt0 * 64, min(n, (tt0 + cnt) * 64)))
    return direct, {k: sorted(v) for k, v in slabbed.items()}


# ---- 1. exact sums ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_exact(dev):
    """the integers of the big case (equal in bf16 and fp16), their fp64 Gram, and the start matrix"""
    pl = ex.xtx_plan(BIG_N, BIG_K)
    assert (pl["n_tiles"], pl["n_direct"], pl["n_rem"], pl["has_tail"]) == (276, 256, 20, 1) and pl["s2"] > 1
    X32 = torch.from_numpy(ex.dense_ints((BIG_N, BIG_K), seed=21)).to(dev)
    ref = _ref(X32)
    G0, Gnan, lower, untouched = _start(BIG_K, dev, 22)
    ex.assert_exactly_summable(1000 + 9 * BIG_N, 0, "K=5640 chained")        # 9 * 2017 < 2^24
    return X32, G0.double() + ref, Gnan, lower, untouched


@pytest.mark.parametrize("shape", SHAPE_ENVS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("chain", [640, 1280])
def test_exact_sums_whole_round_plus_slabs(ops, dev, monkeypatch, big_exact, chain, dtype, shape):
    """K = 5640 (276 tiles: 256 direct over all 2017 tokens -- 3 or 1 cuts --, 20 slabbed; the last panel 8 columns wide;
    the last 17 tokens in the tail staging, behind the last cut), G from nonzero integers.  Pins: a token dropped or
    counted twice at a cut, a flush that forgets to zero the accumulators (everything before the cut counted twice), a
    flush that writes another tile's entries or ignores the edge masks, the tail staging after a cut."""
    _shape_env(monkeypatch, shape)
    X32, want, Gnan, lower, untouched = big_exact
    G = Gnan.clone()
    ops.xtx_accumulate(X32.to(dtype), G, chain_tokens=chain)
    ex.assert_exact(G, want, region=lower, untouched=untouched, what=f"K=5640 chain={chain} {dtype} shape {shape}", gram=True)


def _cut_probes(n, chunks, chain):
    """token positions at each cut +- 1: the cuts of a whole-call item (k * chain) and of every slab chunk (t0 + k * chain)"""
    pos = set()
    for t0, t1 in [(0, n)] + list(chunks):
        for cut in range(t0 + chain, t1, chain):
            pos.update((cut - 1, cut, cut + 1))
        pos.update((t0, t1 - 1))
    return sorted(p for p in pos if 0 <= p < n)


# (tokens, K).  (2117, 264) is all slabbed, but xtx_plan cuts it into 8 chunks of at most 320 tokens, so no slab item
# reaches a cut there.  The other two are long enough for 63 chunks LONGER than 640 tokens: of 11 / 12 token tiles (one
# cut each: the slab's first flush is a store, the end an add) and of 21 / 22 token tiles (two cuts: a store, an add, the
# end an add), the last chunk ending in the tail staging
SLAB_CASES = [(2117, 264), (64 * 11 * 64, 264), (64 * 21 * 64 + 17, 264)]


@pytest.mark.parametrize("shape", SHAPE_ENVS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,K", SLAB_CASES)
def test_exact_sums_all_slabbed(ops, dev, monkeypatch, n, K, dtype, shape):
    """K = 264: 3 tiles, every one split over token chunks into slabs.  Dense integers from a nonzero G for chain_tokens
    640 and 1280, then one nonzero token row at every cut +- 1 and at both ends of every chunk (F = 640), G from zero.
    The slab area is filled with NaN in front of every call: a first flush that ADDS into its slab instead of storing
    turns the tile into NaN.  Pins, at the long-chunk shapes: the slab's store-then-add sequence, a cut counted from the
    call's first token instead of the item's, a token lost or doubled at a cut.  Exact: 1000 + 9 * 86033 < 2^24."""
    _shape_env(monkeypatch, shape)
    pl, chunks = ex.xtx_plan(n, K), ex.xtx_chunks(n, K)
    assert pl["n_direct"] == 0 and pl["s2"] > 1
    shortest = min(t1 - t0 for t0, t1 in chunks)
    if n > 2117:                    # every chunk crosses one cut (two cuts) of F = 640
        assert shortest > (STEP if n < 64 * 21 * 64 else 2 * STEP)
    ex.assert_exactly_summable(1000 + 9 * n, 0, f"tokens={n} K={K}")
    X = torch.from_numpy(ex.dense_ints((n, K), seed=n + K)).to(dtype).to(dev)
    want = _ref(X)
    G0, Gnan, lower, untouched = _start(K, dev, n)
    for chain in (640, 1280):
        ops.workspace(ops.load().qt_xtx_workspace_bytes(n, K), dev, "xtx").fill_(0xFF)      # NaN slabs
        G = Gnan.clone()
        ops.xtx_accumulate(X, G, chain_tokens=chain)
        ex.assert_exact(G, G0.double() + want, region=lower, untouched=untouched,
                        what=f"tokens={n} K={K} chain={chain} {dtype} shape {shape}", gram=True)
    probes = _cut_probes(n, chunks, STEP)
    if n > 2117:                    # 64 chunks: the cuts of the first, a middle and the last chunk
        keep = [chunks[0], chunks[len(chunks) // 2], chunks[-1]]
        probes = [p for p in probes if any(t0 <= p < t1 for t0, t1 in keep)]
        assert any(p - t0 == STEP for p in probes for t0, _ in keep)
    X.zero_()
    for t in probes:
        row = torch.from_numpy(ex.one_hot_token(1, K, 0, dtype, seed=t + K)[0]).to(dev)
        X[t] = row.to(dtype)
        G = torch.where(untouched, torch.full((K, K), float("nan"), device=dev), torch.zeros((K, K), device=dev))
        ops.xtx_accumulate(X, G, chain_tokens=STEP)
        ex.assert_exact(G, torch.outer(row.double(), row.double()), region=lower, untouched=untouched,
                        what=f"one-hot token {t} of {n}, K={K} {dtype} shape {shape}", gram=True)
        X[t] = 0


# ---- 2. the bit definition on random data ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_random(dev):
    g = torch.Generator().manual_seed(31)
    X = torch.randn((BIG_N, BIG_K), generator=g).to(torch.bfloat16).to(dev)
    G0 = torch.randn((BIG_K, BIG_K), generator=g).to(dev)
    return X, G0


def test_bits_are_those_of_plain_launches_over_the_slices(ops, dev, monkeypatch, big_random):
    """F = 640 on N(0, 1) bf16 data, K = 5640, 2017 tokens.  A tile that is direct in the whole launch and in every slice
    launch (the first 256 of the table) must equal, to the bit, the plain calls over X[0:640], X[640:1280], ... in order:
    (((G + p1) + p2) + ...).  A slabbed tile must equal the fp32 restatement: per chunk the fold of its spans' partial
    sums in span order (the partial sums from plain launches into a zero G), the chunks summed in ascending order
    starting from the first (xtx_reduce_kernel), that sum added to G."""
    monkeypatch.delenv("QT_XTX_SHAPE", raising=False)
    X, G0 = big_random
    F = STEP
    pl = ex.xtx_plan(BIG_N, BIG_K)
    assert (pl["n_tiles"], pl["n_direct"], pl["n_rem"]) == (276, 256, 20)
    direct, slabbed = _single_plan(ops, BIG_N, BIG_K)
    assert len(direct) == 256 and len(slabbed) == 20
    for t0 in range(0, BIG_N, F):
        d_slice, _ = _single_plan(ops, min(F, BIG_N - t0), BIG_K)
        assert set(direct) <= set(d_slice), "a tile of the first round is not direct in a slice launch"
    G = G0.clone()
    ops.xtx_accumulate(X, G, chain_tokens=F)
    Gs = G0.clone()
    for t0 in range(0, BIG_N, F):
        ops.xtx_accumulate(X[t0:t0 + F], Gs)
    m = _tile_mask(BIG_K, direct, dev)
    assert torch.equal(G[m], Gs[m]), f"{int((G[m] != Gs[m]).sum())} entries of the direct tiles differ from the slice launches"

    # slabbed tiles: one plain launch into a zero G per span (a span lies inside one chunk; every such launch is short
    # enough to be all direct)
    ranges = sorted({r for v in slabbed.values() for r in v})
    assert all(ranges == v for v in slabbed.values())
    ms = _tile_mask(BIG_K, slabbed, dev)
    total = None
    for t0, t1 in ranges:
        chunk = None
        for s0 in range(t0, t1, F):
            s1 = min(t1, s0 + F)
            assert ex.xtx_plan(s1 - s0, BIG_K)["s2"] == 1
            P = torch.zeros((BIG_K, BIG_K), device=dev)
            ops.xtx_accumulate(X[s0:s1], P)
            chunk = P[ms] if chunk is None else chunk + P[ms]
        total = chunk if total is None else total + chunk
    want = G0[ms] + total
    assert torch.equal(G[ms], want), f"{int((G[ms] != want).sum())} entries of the slabbed tiles differ from the restatement"


# ---- 3. no cut -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPE_ENVS)
def test_a_bound_no_shorter_than_the_call_gives_the_plain_bits(ops, dev, monkeypatch, big_random, shape):
    """chain_tokens = 2560 >= 2017 tokens: no item reaches a cut, the CHAIN kernels' end-of-item code alone runs.  The
    lower triangle must be the plain call's, bit for bit."""
    _shape_env(monkeypatch, shape)
    X, G0 = big_random
    chain = (BIG_N + STEP - 1) // STEP * STEP
    G, Gp = G0.clone(), G0.clone()
    ops.xtx_accumulate(X, G, chain_tokens=chain)
    ops.xtx_accumulate(X, Gp)
    lower, _ = ex.gram_masks(BIG_K, dev)
    assert torch.equal(G[lower], Gp[lower])


# ---- 4. batched ------------------------------------------------------------------------------------------------------
# (K, tokens).  The first: three problems as short as a test can make them; the batched planner cuts all of their 18
# (problem, tile) pairs into slabbed chunks of 6 token tiles, so nothing there reaches a cut.  The second is the
# smallest batch with a whole round of 256 direct pairs -- 13 problems of 21 tiles -- whose direct items (11 and 12
# token tiles) cross the cut at 640 tokens, one of them into a ragged tail, and whose last 17 pairs are slabbed.
BATCHED = [(520, [2000, 1411, 700]), (1536, [768] * 12 + [700])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,tokens", BATCHED, ids=["k520x3", "k1536x13"])
def test_batched_exact(ops, dev, K, tokens, dtype):
    """Several problems of one K in one launch, F = 640, integers from a nonzero G, the slab area NaN beforehand.  Pins
    the batched form's cuts (counted from each item's own first token), its per-problem G pointer in the flush and its
    ragged tail behind a cut."""
    F = STEP
    items, n_slabs = ops.xtx_batched_plan(tokens, K)
    assert n_slabs > 0 and any(slab >= 0 for *_, slab in items), "no slabbed item"
    if K == 1536:
        assert any(slab < 0 and cnt * 64 > F for _, _, _, _, cnt, slab in items), "no direct item crosses a cut"
        assert any(slab < 0 and cnt * 64 > F and tokens[p] % 64 for p, _, _, _, cnt, slab in items)
    ex.assert_exactly_summable(1000 + 9 * max(tokens), 0, "batched chained")
    Xs = [torch.from_numpy(ex.dense_ints((n, K), seed=n + p)).to(dtype).to(dev) for p, n in enumerate(tokens)]
    starts = [_start(K, dev, n + p) for p, n in enumerate(tokens)]
    Gs = [s[1].clone() for s in starts]
    ops.workspace(ops.xtx_batched_workspace_bytes(tokens, K), dev, "xtx_batched").fill_(0xFF)
    ops.xtx_accumulate_batched(Xs, Gs, chain_tokens=F)
    for p, (X, G, (G0, _, lower, untouched)) in enumerate(zip(Xs, Gs, starts)):
        ex.assert_exact(G, G0.double() + _ref(X), region=lower, untouched=untouched, what=f"problem {p} {dtype}", gram=True)


# ---- 5. precision ----------------------------------------------------------------------------------------------------
def test_precision_against_fp64(ops, dev, monkeypatch):
    """K = 5888 (276 tiles, 256 of them direct), 65 536 tokens of N(0, 1) bf16 with 1 % of the channels times 10,
    F = 3840 (4096 rounded down to a multiple of 640).  e = max |dG| / sqrt(Gii Gjj) over the 256 direct tiles against
    the fp64 Gram of the same rounded inputs.  A random walk of fp32 roundings predicts e(chained) / e(plain) =
    sqrt(3840 / 65 536) = 0.24; the bars: at most 0.5, and e(chained) <= 1e-5.  The plain error must be at least 2e-6
    for the case to discriminate.
    Measured: e(plain) = 4.32e-6, e(chained) = 3.9e-7 (ratio 0.09)."""
    monkeypatch.delenv("QT_XTX_SHAPE", raising=False)
    K, n, F = 5888, 65536, 4096 // STEP * STEP
    assert F == 3840
    pl = ex.xtx_plan(n, K)
    assert (pl["n_tiles"], pl["n_direct"]) == (276, 256)
    direct, _ = _single_plan(ops, n, K)
    g = torch.Generator(device=dev).manual_seed(5)
    X = torch.randn((n, K), generator=g, device=dev)
    hot = torch.randperm(K, generator=g, device=dev)[:K // 100]
    X[:, hot] *= 10
    X = X.to(torch.bfloat16)
    ref = _ref(X)
    d = ref.diagonal().sqrt()
    m = _tile_mask(K, direct, dev)

    def err(chain):
        G = torch.zeros((K, K), device=dev)
        ops.xtx_accumulate(X, G, chain_tokens=chain)
        rel = (G.double() - ref).abs_() / (d[:, None] * d[None, :])
        return float(rel[m].max())

    e_plain, e_chained = err(0), err(F)
    print(f"precision K={K} tokens={n}: e(plain) = {e_plain:.3e}, e(chained, F={F}) = {e_chained:.3e}, "
          f"ratio {e_chained / e_plain:.3f}")
    assert e_plain >= 2e-6, f"the plain error {e_plain:.3e} is too small for this case to discriminate"
    assert e_chained <= 0.5 * e_plain, (e_chained, e_plain)
    assert e_chained <= 1e-5, e_chained


# ---- 6. the throttled kernel, once -----------------------------------------------------------------------------------
def test_throttled_kernel_exact(ops, dev, monkeypatch):
    """K = 11 776 (1081 tiles: 1024 direct in four rounds), 46 080 tokens (X > 1 GiB, 720 token tiles), QT_XTX_SHAPE=32:
    the launch takes xtx_kernel with the throttle, here with two cuts (F = 15 360) per direct item.  Integers from a
    nonzero G; the fp64 reference is formed on the device.  Exact: 1000 + 9 * 46 080 < 2^24.  The only large case."""
    monkeypatch.setenv("QT_XTX_SHAPE", "32")
    monkeypatch.delenv("QT_XTX_THROTTLE", raising=False)
    K, n, F = 11776, 46080, 15360
    pl = ex.xtx_plan(n, K)
    assert pl["n_tiles"] == 1081 and pl["n_direct"] >= 4 * ex.NUM_CU and pl["n_tt"] >= 512 and n * K * 2 > 1 << 30
    ex.assert_exactly_summable(1000 + 9 * n, 0, "throttled chained")
    g = torch.Generator(device=dev).manual_seed(6)
    X = torch.randint(1, 4, (n, K), generator=g, device=dev, dtype=torch.int8)
    X = (X * (torch.randint(0, 2, (n, K), generator=g, device=dev, dtype=torch.int8) * 2 - 1)).to(torch.bfloat16)
    want = _ref(X)
    G0, G, lower, untouched = _start(K, dev, 7)
    want += G0
    del G0
    ops.xtx_accumulate(X, G, chain_tokens=F)
    ex.assert_exact(G, want, region=lower, untouched=untouched, what="K=11776 throttled, chain=15360", gram=True)


# ---- 7. the workspace bound ------------------------------------------------------------------------------------------
PATTERN = 0xA5


def _guarded(dev, need, offset):
    guard = (max(1 << 20, need) + 255) // 256 * 256
    start = guard + offset
    buf = torch.full((start + need + guard,), PATTERN, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    return buf, start


def _bad(region):
    bad = (region != PATTERN).nonzero()
    return None if bad.numel() == 0 else (int(bad[0]), int(bad[-1]), int(bad.numel()))


@pytest.mark.parametrize("offset", [0, 16])
def test_chained_calls_stay_inside_the_workspace_they_ask_for(ops, dev, offset):
    """The chained calls use the unchained calls' workspace sizes: run with exactly those bytes between two guards, they
    write nothing outside, refuse one byte less, and give the bits of the call through ``ops``.  Single: (2117, 520),
    slabs + tail + table; batched: [2000, 1411, 700] x 520."""
    from quantool_amd.hip._lib import QT_BF16, QT_ERR_WORKSPACE, QT_OK

    lib, K, F = ops.load(), 520, STEP
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(offset)
    tokens = [2000, 1411, 700]
    host = [(torch.randn(t, K, generator=g) * 0.5).to(torch.bfloat16) for t in [2117] + tokens]
    Xs = [h.to(dev) for h in host]

    # single
    need = int(lib.qt_xtx_workspace_bytes(2117, K))
    buf, start = _guarded(dev, need, offset)
    G = torch.full((K, K), 0.25, device=dev)
    args = (Xs[0].data_ptr(), QT_BF16, 2117, K, K, G.data_ptr(), F)
    assert lib.qt_xtx_accumulate_chained(*args, buf.data_ptr() + start, need - 1, stream) == QT_ERR_WORKSPACE
    rc = lib.qt_xtx_accumulate_chained(*args, buf.data_ptr() + start, need, stream)
    assert rc == QT_OK, lib.qt_last_error()
    torch.cuda.synchronize()
    assert _bad(buf[:start]) is None and _bad(buf[start + need:]) is None, "single: wrote outside its workspace"
    G2 = torch.full((K, K), 0.25, device=dev)
    ops.xtx_accumulate(Xs[0], G2, chain_tokens=F)
    assert torch.equal(G, G2)

    # batched
    need = ops.xtx_batched_workspace_bytes(tokens, K)
    buf, start = _guarded(dev, need, offset)
    Gs = [torch.full((K, K), 0.25, device=dev) for _ in tokens]
    m = len(tokens)
    counts = (ctypes.c_int64 * m)(*tokens)
    ldx = (ctypes.c_int64 * m)(*[K] * m)
    xp = (ctypes.c_void_p * m)(*[x.data_ptr() for x in Xs[1:]])
    gp = (ctypes.c_void_p * m)(*[x.data_ptr() for x in Gs])
    args = (xp, QT_BF16, counts, ldx, K, gp, m, F)
    assert lib.qt_xtx_accumulate_batched_chained(*args, buf.data_ptr() + start, need - 1, stream) == QT_ERR_WORKSPACE
    rc = lib.qt_xtx_accumulate_batched_chained(*args, buf.data_ptr() + start, need, stream)
    assert rc == QT_OK, lib.qt_last_error()
    torch.cuda.synchronize()
    assert _bad(buf[:start]) is None and _bad(buf[start + need:]) is None, "batched: wrote outside its workspace"
    G2s = [torch.full((K, K), 0.25, device=dev) for _ in tokens]
    ops.xtx_accumulate_batched(Xs[1:], G2s, chain_tokens=F)
    assert all(torch.equal(a, b) for a, b in zip(Gs, G2s))
