"""``qt_moe_gemm_wq_wide`` on the GPU: every row bit for bit against ``qt_gemm_wq_grouped`` and against per-expert
``qt_gemm_wq_skinny`` at ragged expert sizes, k-block counts and column tiles; one-hot rows that pin expert, m-tile and
row against the dequantised weight; exact inputs against the fp64 sum; random inputs inside the header's bound; a
caller-owned Y with sentinels and clamped ``row_idx``; the raw ABI's refusals; ``WeightOnlyExperts`` with
``wide_min_tokens`` / ``wide_max_tokens``; and ``load_quantized(..., a16_experts_wide_tokens=)`` end to end."""
import itertools
import math

import pytest
import torch

from tests.test_gpu_moe import _random_routing
from tests.test_gpu_wq_experts import _acts, _experts, _per_expert, _quantize_mixtral, _restated
from tests.test_gpu_wq_linear import _bits_equal, _check_bound, _ref_w, _weight

pytestmark = pytest.mark.gpu

N0, K0 = 33, 5 * 128        # three column tiles, the last partial; five k-blocks: waves with two and with one

# (E, rows per expert) and the m-tiles the host rule must pick from R = sum and E
RAGGED = [
    (8, [0, 0, 5, 17, 0, 0, 1, 0], 1),          # empty experts first, adjacent and last; one row; two slots of 16
    (4, [15, 16, 17, 0], 1),                    # a tile less one, a tile, a tile and a row at 16 rows per tile
    (4, [31, 32, 33, 0], 2),                    # the same at 32 rows
    (4, [63, 64, 65, 0], 4),                    # at 64
    (4, [127, 128, 129, 0], 8),                 # at 128
    (4, [70, 40, 0, 1], 2),                     # an expert of three slots and one of two
    (3, [28, 0, 20], 1),                        # ceil(R / E) = 16: the last R of the 1-tile instance
    (3, [29, 0, 20], 2),                        # 17: the first of the 2-tile instance
    (3, [76, 0, 20], 2),                        # 32
    (3, [77, 0, 20], 4),                        # 33
    (3, [150, 22, 20], 4),                      # 64
    (3, [151, 22, 20], 8),                      # 65
    (1, [1], 1),
    (1, [150], 8),                              # E = 1: one expert of two slots
    (64, [(7 * e) % 5 for e in range(64)], 1),  # E = 64, a fifth of the experts empty
    (64, [40 if e % 3 == 0 else 5 for e in range(64)], 2),   # E = 64 past 16 rows per expert on average
]
FACTORS = list(itertools.product((4, 8), (False, True), (False, True), (torch.bfloat16, torch.float16), (True, False)))


def test_ragged_cases_pick_the_instances_they_name(ops):
    seen = set()
    for E, counts, mt in RAGGED:
        assert len(counts) == E and ops.moe_wq_wide_mtiles(sum(counts), E) == mt, (E, counts)
        seen.add(mt)
    assert seen == {1, 2, 4, 8}


def _bank(dev, E, N, K, bits, zp, grouped, seed):
    """(Wq [E, N, .], s_w [E, N, G], zp_w or None, the checkpoint leaves per expert), experts all different."""
    ts = [_weight(N, K, bits, zp=zp, grouped=grouped, seed=seed + 7 * e)[0] for e in range(E)]
    Wq = torch.stack([t["weight_packed" if bits == 4 else "weight"] for t in ts]).to(dev)
    s = torch.stack([t["weight_scale"] for t in ts]).to(dev)
    z = torch.stack([t["weight_zero_point"] for t in ts]).to(dev) if zp else None
    return Wq, s, z, ts


def _offsets(counts, dev):
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    return off, torch.tensor(off, dtype=torch.int32, device=dev)


def _operands(dev, counts, K, dtype, gather, seed):
    """(X, row_idx or None, the source row of every routed row) for sum(counts) routed rows."""
    R = sum(counts)
    if gather:
        T = max(R // 2, 3)
        X = _acts(T, K, dtype, dev, seed)
        row_idx = torch.randint(0, T, (R,), generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(dev)
        return X, row_idx, row_idx.long()
    return _acts(R, K, dtype, dev, seed), None, torch.arange(R, device=dev)


def _check_case(ops, dev, E, counts, N, K, combos, skinny_every):
    """The wide form against the grouped GEMV on every combination of ``combos``, and against per-expert skinny
    launches on every ``skinny_every``-th of them."""
    off_l, off = _offsets(counts, dev)
    banks = {}
    for n, (bits, zp, grouped, dtype, gather) in enumerate(combos):
        key = (bits, zp, grouped)
        if key not in banks:
            banks[key] = _bank(dev, E, N, K, bits, zp, grouped, seed=len(counts) + K + bits)
        Wq, s, z, _ = banks[key]
        X, row_idx, src = _operands(dev, counts, K, dtype, gather, seed=N + K)
        Y = ops.moe_gemm_wq_wide(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z)
        assert Y.shape == (off_l[-1], N) and Y.dtype == dtype
        what = (E, counts[:8], N, K, bits, zp, grouped, dtype, gather)
        want = ops.gemm_wq_grouped(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z)
        assert torch.equal(Y.view(torch.int16), want.view(torch.int16)), what
        if n % skinny_every == 0:
            for lo, hi, rows in _per_expert(ops, X, src, off_l, Wq, s, z, None):
                assert torch.equal(Y[lo:hi].view(torch.int16), rows.view(torch.int16)), (what, lo, hi)


# ---- bits against the grouped GEMV and the skinny kernel -----------------------------------------------------------
@pytest.mark.parametrize("case", range(len(RAGGED)), ids=[f"E{e}-R{sum(c)}-mt{m}" for e, c, m in RAGGED])
def test_ragged_experts_equal_grouped_and_skinny(ops, dev, case):
    """All 32 combinations of weight format, zero-point, group count, dtype and gathered / contiguous rows against the
    grouped GEMV; every eighth of them, a different eighth per case, against the skinny kernel on 16-row slices."""
    E, counts, _ = RAGGED[case]
    combos = FACTORS[case % 8:] + FACTORS[:case % 8]
    _check_case(ops, dev, E, counts, N0, K0, combos, skinny_every=8)


def _cycled(values):
    """One (value, combination) per value, the combinations walking FACTORS so that every pair of factor values meets
    over the k-block and the column-tile tests (test_cycled_cases_cover_every_pair)."""
    return [(v, FACTORS[(11 * i + 3) % 32]) for i, v in enumerate(values)]


KBS = (1, 3, 4, 5, 16, 17, 32, 33)      # around the four waves and around a batch of either format (8 / 4 k-blocks)
NS = (1, 15, 16, 17, 33)


def test_cycled_cases_cover_every_pair():
    combos = [c for _, c in _cycled(KBS)] + [c for _, c in _cycled(NS)] + [FACTORS[(5 * i) % 32] for i in range(8)]
    for a, b in itertools.combinations(range(5), 2):
        seen = {(c[a], c[b]) for c in combos}
        assert len(seen) == 4, (a, b, seen)


@pytest.mark.parametrize("kbs,combo", _cycled(KBS), ids=[f"kb{k}" for k in KBS])
def test_k_blocks(ops, dev, kbs, combo):
    extra = [FACTORS[(5 * i) % 32] for i in range(8)] if kbs == 5 else []
    _check_case(ops, dev, 3, [17, 0, 40], N0, 128 * kbs, [combo] + extra, skinny_every=1)


@pytest.mark.parametrize("N,combo", _cycled(NS), ids=[f"N{n}" for n in NS])
def test_column_tiles(ops, dev, N, combo):
    _check_case(ops, dev, 3, [17, 0, 40], N, K0, [combo], skinny_every=1)


# ---- one-hot rows: which expert, which m-tile, which row -------------------------------------------------------------
@pytest.mark.parametrize("E,counts", [(4, [33, 0, 70, 5]), (2, [130, 3])], ids=["mt2", "mt8"])
@pytest.mark.parametrize("bits,zp,dtype", [(4, False, torch.bfloat16), (4, True, torch.float16),
                                           (8, False, torch.float16)])
def test_one_hot_rows_read_their_experts_weight(ops, dev, E, counts, bits, zp, dtype):
    N, K = N0, K0
    Wq, s, z, ts = _bank(dev, E, N, K, bits, zp, True, seed=bits + E)
    Wt = [_ref_w(t, dtype).to(dev).t().contiguous().view(torch.int16) for t in ts]      # per expert [K, N]
    off_l, off = _offsets(counts, dev)
    R = off_l[-1]
    owner = torch.cat([torch.full((c,), e) for e, c in enumerate(counts)]).tolist()
    rows = torch.arange(R, device=dev)
    for shift in (0, 1, 127, 129, 300):
        cols = (rows + shift) % K
        X = torch.zeros(R, K, dtype=dtype, device=dev)
        X[rows, cols] = 1
        want = torch.stack([Wt[owner[m]][c] for m, c in enumerate(cols.tolist())])
        Y = ops.moe_gemm_wq_wide(X, Wq, s, off, K=K, zp_w=z)
        assert torch.equal(Y.view(torch.int16), want), ("contiguous", shift)
        # gathered: routed row m reads X row perm[m]
        perm = torch.randperm(R, generator=torch.Generator().manual_seed(shift)).to(dev)
        inv = torch.empty_like(perm)
        inv[perm] = rows
        Y = ops.moe_gemm_wq_wide(X[inv].contiguous(), Wq, s, off, row_idx=perm.to(torch.int32), K=K, zp_w=z)
        assert torch.equal(Y.view(torch.int16), want), ("gathered", shift)


# ---- exact and random inputs against fp64 -----------------------------------------------------------------------------
# |x| <= 4, |q - zp| <= 16 (int4) or 136 (int8), scales 2^0 .. 2^-4, K = 1024: every partial sum is a multiple of 2^-4
# below 2^20, so exact in fp32 (test_gpu_wq_stream.test_exact_inputs_bit_exact's argument)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("bits,zp", [(4, False), (4, True), (8, False), (8, True)])
def test_exact_inputs_equal_the_fp64_sum_rounded_once(ops, dev, dtype, bits, zp):
    E, counts, N, K = 3, [40, 0, 17], 33, 1024
    ts = [_weight(N, K, bits, zp=zp, seed=3 * e + bits, pow2_scales=True)[0] for e in range(E)]
    Wq = torch.stack([t["weight_packed" if bits == 4 else "weight"] for t in ts]).to(dev)
    s = torch.stack([t["weight_scale"] for t in ts]).to(dev)
    z = torch.stack([t["weight_zero_point"] for t in ts]).to(dev) if zp else None
    off_l, off = _offsets(counts, dev)
    X = torch.randint(-4, 5, (off_l[-1], K), generator=torch.Generator().manual_seed(K)).to(dtype)
    Y = ops.moe_gemm_wq_wide(X.to(dev), Wq, s, off, K=K, zp_w=z)
    for e in range(E):
        lo, hi = off_l[e], off_l[e + 1]
        ref = X[lo:hi].double() @ _ref_w(ts[e], dtype).double().T
        _bits_equal(Y[lo:hi], (ref + 0.0).to(dtype))    # the kernel sums from +0: an exactly zero output is +0


@pytest.mark.parametrize("counts,N,kbs,bits,zp,dtype,gather", [([17, 0, 40], 33, 5, 4, True, torch.bfloat16, True),
                                                               ([70, 3], 17, 17, 8, False, torch.float16, False),
                                                               ([130, 20], 33, 33, 4, False, torch.bfloat16, True)])
def test_random_inputs_within_the_fp64_bound(ops, dev, counts, N, kbs, bits, zp, dtype, gather):
    """|y - y_fp64| <= ulp(y) / 2 + K 2^-24 sum |x w| (the header's bound for qt_gemm_wq_skinny), fp64 on the CPU."""
    E, K = len(counts), 128 * kbs
    Wq, s, z, ts = _bank(dev, E, N, K, bits, zp, True, seed=N + kbs)
    off_l, off = _offsets(counts, dev)
    X, row_idx, src = _operands(dev, counts, K, dtype, gather, seed=5)
    Y = ops.moe_gemm_wq_wide(X, Wq, s, off, row_idx=row_idx, K=K, zp_w=z)
    for e in range(E):
        lo, hi = off_l[e], off_l[e + 1]
        if hi > lo:
            _check_bound(Y[lo:hi], X[src[lo:hi]], _ref_w(ts[e], dtype))


# ---- a caller-owned Y, clamped row_idx, the raw ABI -------------------------------------------------------------------
def _raw(X, code, K, ldx, row_idx, R, off, E, Wq, fmt, N, s, G, zp, g_idx, Y, ldy, x_rows):
    from quantool_amd.hip import _lib

    p = lambda v: None if v is None else (v if isinstance(v, int) else v.data_ptr())   # noqa: E731
    _lib.check("qt_moe_gemm_wq_wide", _lib.load().qt_moe_gemm_wq_wide(
        p(X), code, K, ldx, p(row_idx), R, p(off), E, p(Wq), fmt, N, p(s), G, p(zp), p(g_idx), p(Y), ldy, x_rows,
        torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("bits", [4, 8])
def test_caller_owned_output_keeps_its_sentinels_and_row_idx_is_clamped(ops, dev, bits):
    from quantool_amd.hip import _lib

    E, N, K, T = 4, N0, K0, 24
    Wq, s, z, _ = _bank(dev, E, N, K, bits, True, True, seed=4)
    # operands as exact-size allocations: each ends with its storage
    Wq, s, z = Wq.clone(), s.clone(), z.clone()
    counts = [3, 0, 37, 1]                                  # R = 41 routed rows of 50: rows [41, 50) belong to no expert
    off_l, off = _offsets(counts, dev)
    R, routed = 50, off_l[-1]
    # X sits between NaN rows the test owns: an index that is followed, not clamped, reads NaN
    xbuf = torch.full((T + 16, K), float("nan"), dtype=torch.bfloat16, device=dev)
    xbuf[8:8 + T] = _acts(T, K, torch.bfloat16, dev, seed=3)
    X = xbuf[8:8 + T]
    row_idx = torch.randint(0, T, (R,), generator=torch.Generator().manual_seed(7)).to(torch.int32)
    row_idx[[0, 5, 20, 40]] = torch.tensor([-1, T, -7, T + 6], dtype=torch.int32)
    clamped = row_idx.clamp(0, T - 1).to(dev)
    row_idx = row_idx.to(dev)
    ldy, rows = N + 17, R + 3
    fmt = _lib.QT_W_INT4_PACKED if bits == 4 else _lib.QT_W_INT8
    runs = []
    for _ in range(2):
        buf = torch.full((rows * ldy + 64,), 7.0, dtype=torch.bfloat16, device=dev)
        _raw(X, _lib.QT_BF16, K, K, row_idx, R, off, E, Wq, fmt, N, s, s.shape[2], z, None, buf, ldy, T)
        runs.append(buf)
    torch.cuda.synchronize()
    _bits_equal(runs[0], runs[1])                                                       # two runs, the same bits
    grid = runs[0][:rows * ldy].view(rows, ldy)
    want = ops.gemm_wq_grouped(X, Wq, s, off, row_idx=clamped, K=K, zp_w=z)
    assert torch.isfinite(grid[:routed, :N].float()).all()
    _bits_equal(grid[:routed, :N].contiguous(), want[:routed])
    assert (grid[:routed, N:] == 7).all() and (grid[routed:] == 7).all() and (runs[0][rows * ldy:] == 7).all()


def test_raw_abi_refusals_launch_nothing(ops, dev):
    from quantool_amd.hip._lib import QT_BF16, QT_ERR_INVALID, QT_F32, QT_W_INT8, HipBackendError

    E, N, K, R = 2, 32, 1024, 40
    wbuf = torch.zeros(E * N * K + 16, dtype=torch.int8, device=dev)
    Wq, Wq_off = wbuf[:E * N * K].view(E, N, K), wbuf[4:4 + E * N * K].view(E, N, K)
    xbuf = torch.zeros(R * (K + 8) + 8, dtype=torch.bfloat16, device=dev)
    X, X_off = xbuf[:R * K].view(R, K), xbuf[1:1 + R * K].view(R, K)
    s = torch.ones(E, N, 8, device=dev)
    gi = torch.zeros(E, K, dtype=torch.int32, device=dev)
    off = torch.tensor([0, 17, R], dtype=torch.int32, device=dev)
    Y = torch.full((R, N), 7.0, dtype=torch.bfloat16, device=dev)
    i8, bf = QT_W_INT8, QT_BF16
    big = (1 << 32) // (2 * K)          # x_rows ldx 2 = 2^32
    #        X, code, K, ldx, row_idx, R, offsets, E, Wq, fmt, N, s_w, G, zp, g_idx, Y, ldy, x_rows
    cases = {
        "g_idx": ((X, bf, K, K, None, R, off, E, Wq, i8, N, s, 8, None, gi, Y, N, R), "g_idx is not taken"),
        "ragged K": ((X, bf, 192, K, None, R, off, E, Wq, i8, N, s, 1, None, None, Y, N, R),
                     "not a multiple of the k-unit"),
        "X shifted": ((X_off, bf, K, K, None, R, off, E, Wq, i8, N, s, 1, None, None, Y, N, R), "16-byte aligned"),
        "Wq shifted": ((X, bf, K, K, None, R, off, E, Wq_off, i8, N, s, 1, None, None, Y, N, R), "16-byte aligned"),
        "pitch K + 1": ((X, bf, K, K + 1, None, R, off, E, Wq, i8, N, s, 1, None, None, Y, N, R), "16-byte aligned"),
        "pitch below K": ((X, bf, K, K - 8, None, R, off, E, Wq, i8, N, s, 1, None, None, Y, N, R), "ldx >= K"),
        "ldy below N": ((X, bf, K, K, None, R, off, E, Wq, i8, N, s, 1, None, None, Y, N - 1, R), "ldy >= N"),
        "null X": ((None, bf, K, K, None, R, off, E, Wq, i8, N, s, 1, None, None, Y, N, R), "null pointer"),
        "null offsets": ((X, bf, K, K, None, R, None, E, Wq, i8, N, s, 1, None, None, Y, N, R), "null pointer"),
        "null Wq": ((X, bf, K, K, None, R, off, E, None, i8, N, s, 1, None, None, Y, N, R), "null pointer"),
        "null s_w": ((X, bf, K, K, None, R, off, E, Wq, i8, N, None, 1, None, None, Y, N, R), "null pointer"),
        "null Y": ((X, bf, K, K, None, R, off, E, Wq, i8, N, s, 1, None, None, None, N, R), "null pointer"),
        "G = 3": ((X, bf, K, K, None, R, off, E, Wq, i8, N, s, 3, None, None, Y, N, R), "G must be 1 or K / 128 = 8"),
        "fp32 X": ((X, QT_F32, K, K, None, R, off, E, Wq, i8, N, s, 1, None, None, Y, N, R), "must be bf16 or fp16"),
        "w_format": ((X, bf, K, K, None, R, off, E, Wq, 99, N, s, 1, None, None, Y, N, R), "w_format 99"),
        "R = 0": ((X, bf, K, K, None, 0, off, E, Wq, i8, N, s, 1, None, None, Y, N, R), "bad sizes"),
        "E past the limit": ((X, bf, K, K, None, R, off, ops.MOE_WQ_WIDE_MAX_E + 1, Wq, i8, N, s, 1, None, None, Y, N,
                              R), "bad sizes"),
        # 8 m-tiles: floor(R / 128) + E = 65536 + 2 slots (a row_idx pointer that is never read: refused first)
        "too many slots": ((X, bf, K, K, off, 128 * 65536, off, E, Wq, i8, N, s, 1, None, None, Y, N, R),
                           "row-tile slots"),
        "2^32 bytes": ((X, bf, K, K, off, R, off, E, Wq, i8, N, s, 1, None, None, Y, N, big), "2\\^32"),
        "x_rows below R": ((X, bf, K, K, None, R, off, E, Wq, i8, N, s, 1, None, None, Y, N, R - 1),
                           "without row_idx"),
    }
    for what, (args, reason) in cases.items():
        with pytest.raises(HipBackendError, match=reason) as e:
            _raw(*args)
        assert e.value.status == QT_ERR_INVALID, what
    torch.cuda.synchronize()
    assert (Y == 7).all()
    _raw(X, bf, K, K, None, R, off, E, Wq, i8, N, s, 8, None, None, Y, N, R)             # and the same call, accepted
    torch.cuda.synchronize()
    assert (Y == 0).all()


# ---- WeightOnlyExperts -----------------------------------------------------------------------------------------------
def _call(dev, woe, T, k=2):
    x = _acts(T, woe.hidden_dim, torch.bfloat16, dev, seed=T)
    idx = _random_routing(T, k, woe.num_experts, seed=T + 1).to(dev)
    w = torch.softmax(torch.randn(T, k, generator=torch.Generator().manual_seed(T)), -1).to(torch.bfloat16).to(dev)
    return x, idx, w


@pytest.mark.parametrize("bits,zp", [(4, False), (4, True), (8, False)])
def test_module_wide_form_inside_the_routed_forward(ops, dev, monkeypatch, bits, zp):
    woe, _ = _experts(dev, 8, 256, 384, bits, zp, False, seed=bits)
    calls = {"wide": 0}
    real = ops.moe_gemm_wq_wide

    def wide(*a, **kw):
        calls["wide"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "moe_gemm_wq_wide", wide)
    with torch.no_grad():
        for T in (17, 40, 128):
            x, idx, w = _call(dev, woe, T)
            woe.wide_min_tokens = 0
            want = woe(x, idx, w)
            assert calls["wide"] == 0
            woe.wide_min_tokens = 17
            got = woe(x, idx, w)
            assert calls["wide"] == 2
            calls["wide"] = 0
            _bits_equal(got, want)


@pytest.mark.parametrize("bits,zp", [(4, False), (4, True), (8, False)])
def test_module_extended_range(ops, dev, bits, zp):
    woe, ref = _experts(dev, 4, 256, 384, bits, zp, False, seed=bits + 1)
    woe.wide_max_tokens = 300
    with torch.no_grad():
        for T in (129, 300):
            x, idx, w = _call(dev, woe, T)
            got = woe(x, idx, w)
            _bits_equal(got, _restated(ops, woe, x, idx, w))
            # a row of the fused kernels is within a rounding and the summation-order bound of the
            # dense bank's; 2^-4 of the output scale is the bound the end-to-end tests hold the logits to
            dense = ref(x, idx, w)
            diff, scale = (got.float() - dense.float()).abs().max().item(), dense.float().abs().max().item()
            assert diff <= 2.0 ** -4 * scale, (T, diff, scale)
        x, idx, w = _call(dev, woe, 301)
        assert torch.equal(woe(x, idx, w), ref(x, idx, w))                  # past wide_max_tokens: the dense bank again
    g_bank, g_ref = _experts(dev, 4, 256, 384, 4, False, True, seed=9)      # g_idx: never the kernel
    g_bank.wide_max_tokens = 300
    with torch.no_grad():
        x, idx, w = _call(dev, g_bank, 200)
        assert torch.equal(g_bank(x, idx, w), g_ref(x, idx, w))


def test_module_routed_path_makes_no_host_sync(ops, dev, monkeypatch):
    """test_gpu_wq_experts.test_module_decode_path_makes_no_host_sync's patching, on both ranges of the wide form."""
    woe, _ = _experts(dev, 8, 256, 384, 4, False, False, seed=3)
    woe.wide_min_tokens, woe.wide_max_tokens = 17, 300
    calls = {"route": 0, "wide": 0}
    real_route, real_wide = ops.moe_route, ops.moe_gemm_wq_wide

    def route(*a, **kw):
        calls["route"] += 1
        return real_route(*a, **kw)

    def wide(*a, **kw):
        calls["wide"] += 1
        return real_wide(*a, **kw)

    def host_read(*a, **kw):
        raise AssertionError("host read on the routed path")

    inputs = [_call(dev, woe, T) for T in (40, 200)]
    with torch.no_grad():
        want = [woe(*a) for a in inputs]
        torch.cuda.synchronize()
        monkeypatch.setattr(ops, "moe_route", route)
        monkeypatch.setattr(ops, "moe_gemm_wq_wide", wide)
        for name in ("nonzero", "item", "tolist", "cpu"):
            monkeypatch.setattr(torch.Tensor, name, host_read)
        monkeypatch.setattr(torch, "nonzero", host_read)
        got = [woe(*a) for a in inputs]
        monkeypatch.undo()
    assert calls == {"route": 2, "wide": 4}
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        _bits_equal(a, b)


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_end_to_end_wide_tokens(dev, tmp_path, monkeypatch):
    from quantool_amd.engine.qlinear import WeightOnlyExperts, load_quantized
    from quantool_amd.evaluate import perplexity
    from quantool_amd.hip import ops
    from tests.test_gpu_qlinear import _eval_ids

    monkeypatch.chdir(tmp_path)
    ckpt = tmp_path / "ckpt"
    _quantize_mixtral(dev, "W4A16", ckpt)
    dense_bank = load_quantized(ckpt, device=dev, a16="packed")
    packed = load_quantized(ckpt, device=dev, a16="packed", a16_experts="packed", a16_experts_wide_tokens=512)
    banks = [m for m in packed.modules() if isinstance(m, WeightOnlyExperts)]
    assert len(banks) == 2 and all(b.wide_max_tokens == 512 for b in banks)
    assert packed._qt_checkpoint["a16_experts_wide_tokens"] == 512
    calls = {"wide": 0, "dequant": 0}

    def counting(name, real):
        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return f

    ids = _eval_ids()
    batch = ids[:4].to(dev)                                             # 4 x 96 tokens: past grouped_max_tokens
    assert banks[0].grouped_max_tokens < batch.numel() <= 512
    with torch.no_grad():
        ref = dense_bank(input_ids=batch).logits.float()
        monkeypatch.setattr(ops, "moe_gemm_wq_wide", counting("wide", ops.moe_gemm_wq_wide))
        monkeypatch.setattr(ops, "dequantize_weight", counting("dequant", ops.dequantize_weight))
        got = packed(input_ids=batch).logits.float()
        # both banks on the wide form; the Linears of 384 rows still dequantise
        assert calls["wide"] == 2 * len(banks)
        monkeypatch.undo()
    # test_end_to_end_packed_experts' bound and argument: every routed row is within one rounding plus the
    # summation-order bound of the dense bank's row
    scale = ref.abs().max().item()
    delta = 2.0 ** -4 * scale
    assert (got - ref).abs().max().item() <= delta
    p_dense = perplexity(dense_bank, ids, batch_size=4)["perplexity"]
    p_wide = perplexity(packed, ids, batch_size=4)["perplexity"]
    # logits within delta move every token's log-probability by at most 2 delta, and so the mean of them
    assert math.isfinite(p_wide) and abs(math.log(p_wide) - math.log(p_dense)) <= 2 * delta, (p_wide, p_dense, delta)
