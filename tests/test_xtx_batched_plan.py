"""The item table of ``qt_xtx_accumulate_batched``, read through ``qt_xtx_batched_plan`` (host only: no device needed).
The launch goes through the same planner, so what holds here holds for what runs."""
import ctypes

import numpy as np
import pytest

from tests.exact_inputs import NUM_CU, TILE, TOKEN_TILE, xtx_chunks, xtx_plan

KS = (512, 520, 1024, 4096, 14336)
_rng = np.random.default_rng(11)
TOKENS = {
    "one": [64],
    "zero_in_the_middle": [200, 0, 1000, 64],
    "ragged3": [4096, 4160, 130],
    "ragged8": [int(v) for v in _rng.integers(500, 3001, 8)],
    "llama3": [196608] * 3,
    "experts8": [int(49152 * f) for f in (0.8, 0.87, 0.93, 0.99, 1.04, 1.1, 1.15, 1.2)],
}
MIN_CHUNK = 4
SLAB_BYTES = TILE * TILE * 4


@pytest.fixture(scope="module")
def lib():
    from quantool_amd.hip import _lib

    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as g

        g.build()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))          # loading needs no GPU
    for name in ("qt_xtx_batched_plan", "qt_xtx_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def plan(lib, tokens, K):
    n = len(tokens)
    counts = (ctypes.c_int64 * n)(*tokens)
    n_items, n_slabs, need = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_size_t(0)
    assert lib.qt_xtx_batched_plan(counts, n, K, None, 0, ctypes.byref(n_items), ctypes.byref(n_slabs), None) == 0
    rows = (ctypes.c_int32 * (6 * max(1, n_items.value)))()
    assert lib.qt_xtx_batched_plan(counts, n, K, rows, n_items.value, ctypes.byref(n_items), ctypes.byref(n_slabs),
                                   ctypes.byref(need)) == 0
    items = np.frombuffer(rows, dtype=np.int32)[:6 * n_items.value].reshape(-1, 6).copy()
    return items, n_slabs.value, int(need.value)


@pytest.mark.parametrize("name", list(TOKENS))
@pytest.mark.parametrize("K", KS)
def test_plan_covers_every_token_tile_exactly_once(lib, K, name):
    tokens = TOKENS[name]
    items, n_slabs, need = plan(lib, tokens, K)
    nt = (K + TILE - 1) // TILE
    n_tiles = nt * (nt + 1) // 2
    n_tt = [(t + TOKEN_TILE - 1) // TOKEN_TILE for t in tokens]
    prob, ti, tj, tt0, cnt, slab = items.T
    assert len(items) > 0
    assert (cnt > 0).all(), "an empty item"
    assert ((0 <= prob) & (prob < len(tokens))).all()
    assert all(tokens[p] > 0 for p in set(prob.tolist())), "an item of a zero-token problem"
    assert ((0 <= tj) & (tj <= ti) & (ti < nt)).all(), "an item outside the lower triangle"
    assert (tt0 >= 0).all() and all(a + c <= n_tt[p] for p, a, c in zip(prob, tt0, cnt))
    # every (problem, lower tile, token tile) exactly once: per (problem, tile) the spans tile [0, n_tt) without overlap
    spans = {}
    for p, i, j, a, c in zip(prob.tolist(), ti.tolist(), tj.tolist(), tt0.tolist(), cnt.tolist()):
        spans.setdefault((p, i, j), []).append((a, c))
    assert len(spans) == n_tiles * sum(t > 0 for t in tokens)
    for (p, i, j), sp in spans.items():
        at = 0
        for a, c in sorted(sp):
            assert a == at, f"problem {p} tile ({i}, {j}): token tiles {at}..{a} missed or doubled"
            at = a + c
        assert at == n_tt[p]
    # a pair with one item is direct, a pair with several is slabbed throughout
    for key, sp in spans.items():
        sl = slab[(prob == key[0]) & (ti == key[1]) & (tj == key[2])]
        assert (sl < 0).all() if len(sp) == 1 else (sl >= 0).all(), key
    # no chunk below 4 token tiles unless the problem itself is shorter
    assert all(c >= min(MIN_CHUNK, n_tt[p]) for p, c in zip(prob, cnt))
    # slabs: distinct, dense, capped at 1 GiB; the workspace covers slabs, tails and tables
    used = slab[slab >= 0]
    assert len(set(used.tolist())) == len(used) == n_slabs
    assert n_slabs == 0 or (used.min() == 0 and used.max() == n_slabs - 1)
    assert n_slabs * SLAB_BYTES <= 1 << 30
    if sum(t > 0 for t in tokens) > 1:
        ragged = sum(t % TOKEN_TILE != 0 for t in tokens)
        n_red = sum(len(sp) > 1 for sp in spans.values())
        tables = len(items) * 32 + len(tokens) * 64 + n_red * 32
        assert need >= n_slabs * SLAB_BYTES + ragged * TOKEN_TILE * K * 2 + tables
    # a pure function of (tokens, K): equal on a second call
    again, n_slabs2, need2 = plan(lib, tokens, K)
    assert np.array_equal(items, again) and (n_slabs2, need2) == (n_slabs, need)


@pytest.mark.parametrize("n", [64, 200, 777, 4096, 65536, 196608])
@pytest.mark.parametrize("K", KS)
def test_a_batch_of_one_is_the_single_plan(lib, K, n):
    """One problem with tokens (alone, or beside empty ones): xtx_plan's items, chunk for chunk, and
    qt_xtx_accumulate's workspace, since the launch hands the problem to it."""
    pl, chunks = xtx_plan(n, K), xtx_chunks(n, K)
    for tokens, p in (([n], 0), ([0, n, 0], 1)):
        items, n_slabs, need = plan(lib, tokens, K)
        assert (items[:, 0] == p).all()
        direct = items[items[:, 5] < 0]
        assert len(direct) == pl["n_direct"] and (direct[:, 3] == 0).all() and (direct[:, 4] == pl["n_tt"]).all()
        assert np.array_equal(items[:pl["n_direct"]], direct), "direct items come first, as xtx_item numbers them"
        slabbed = items[pl["n_direct"]:]
        assert len(slabbed) == pl["n_rem"] * (pl["s2"] if pl["n_rem"] else 0) == n_slabs
        assert np.array_equal(slabbed[:, 5], np.arange(len(slabbed))), "slab index = logical - n_direct"
        for c in range(pl["s2"] if pl["n_rem"] else 0):
            part = slabbed[c * pl["n_rem"]:(c + 1) * pl["n_rem"]]
            t0, t1 = chunks[c]
            assert (part[:, 3] * TOKEN_TILE == t0).all()
            assert (np.minimum((part[:, 3] + part[:, 4]) * TOKEN_TILE, n) == t1).all()
        assert need == lib.qt_xtx_workspace_bytes(n, K)


def test_three_k4096_problems_run_mostly_direct(lib):
    """What the batch exists for: alone, a K = 4096 problem has 136 tiles, fewer than the 256 CUs, and xtx_plan splits
    every one of them into slabs; three of them together are 408 tiles, of which whole rounds need none."""
    assert xtx_plan(196608, 4096)["n_direct"] == 0
    items, n_slabs, _ = plan(lib, [196608] * 3, 4096)
    direct = items[items[:, 5] < 0]
    assert len(direct) >= NUM_CU, f"{len(direct)} of 408 tiles direct"
    assert (direct[:, 4] == 196608 // TOKEN_TILE).all()
    assert n_slabs * SLAB_BYTES < 3 * 535e6 / 2, "fewer slab bytes than half of the three single launches'"


@pytest.mark.parametrize("name", ["ragged8", "experts8", "llama3", "ragged3"])
@pytest.mark.parametrize("K", [1024, 4096, 14336])
def test_ragged_batches_stay_balanced(lib, K, name):
    """Workgroups are dealt to 256 CUs in item order, each CU taking the next item when it is free.  List scheduling
    bounds that walk's makespan by work / 256 + the longest item; from one whole round of (problem, tile) pairs up the
    planner lets no item be longer than ceil(work / 256), so the walk ends within twice the ideal whatever the mix."""
    import heapq

    items, _, _ = plan(lib, TOKENS[name], K)
    cnt = items[:, 4].tolist()
    free = [0] * NUM_CU
    for c in cnt:
        heapq.heappush(free, heapq.heappop(free) + c)
    makespan = max(free)
    ideal = -(-sum(cnt) // NUM_CU)
    assert makespan <= sum(cnt) / NUM_CU + max(cnt)
    if len({tuple(r) for r in items[:, :3].tolist()}) >= NUM_CU:
        assert max(cnt) <= ideal and makespan <= 2 * ideal, (max(cnt), makespan, ideal)


def test_consecutive_items_share_a_problem(lib):
    """The 32 consecutive items an XCD takes: at most two problems among them (a chunk may straddle one boundary)."""
    for name in ("ragged8", "experts8", "llama3"):
        items, _, _ = plan(lib, TOKENS[name], 4096)
        for c0 in range(0, len(items), 32):
            assert len(set(items[c0:c0 + 32, 0].tolist())) <= 2


def test_arguments_are_checked(lib):
    counts = (ctypes.c_int64 * 17)(*([64] * 17))
    n, need = ctypes.c_int(7), ctypes.c_size_t(7)
    for n_problems, K in ((17, 512), (0, 512), (2, 516)):
        assert lib.qt_xtx_batched_plan(counts, n_problems, K, None, 0, ctypes.byref(n), None, ctypes.byref(need)) == -1
        assert (n.value, need.value) == (0, 0), "a refused call leaves no stale count or size"
        n.value = need.value = 7
    zeros = (ctypes.c_int64 * 3)(0, 0, 0)
    assert lib.qt_xtx_batched_plan(zeros, 3, 512, None, 0, ctypes.byref(n), None, ctypes.byref(need)) == 0
    assert (n.value, need.value) == (0, 0), "a batch without tokens: no item, no workspace"
