"""qt_moe_gemm_i8_ring_w4: the 256 x 256 LDS-ring int8 GEMM over a packed int4 expert bank (W4A8 prefill).

Its contract is bit equality with the tiled qt_gemm_i8_grouped on the same arguments, so every comparison here is on bit
patterns (``.view(torch.int16)`` + ``torch.equal``), against two yardsticks: ``ops.gemm_i8_grouped`` on the same bank and
one dense ``ops.gemm_i8_ring_w4`` per expert on that expert's gathered rows.  Those would pass kernels wrong in the same
way, so the same cases also go against the fp64 reference of tests/ckpt_reference.py within the project's own bound for
this sequence (``gemm_i8_tolerance`` with G groups); an identity test pins the expert, the group's scale and the nibble
every routed row reads, and a test whose inputs are shown on the CPU to be sensitive to the order of the fp32 group fold
pins that order without a bias.  Shapes are in the kernel's own constants: U = the K-tile = one weight group, R = the
ring's slots, L = its lead."""
import numpy as np
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_i8_ring_grouped import _Counter, _acts, _offsets, _twice
from tests.test_gpu_i8_ring_w4 import _fold32, _url
from tests.test_gpu_i8_skinny import _same_bits, _sentinel, _untouched
from tests.test_gpu_runtime_edges import _leaves, _levels, cr_wsum

pytestmark = pytest.mark.gpu

NAME = "qt_moe_gemm_i8_ring_w4"


def _bank(q4, seed, s_w=None):
    """Checkpoint leaves per expert, and the stacked device operands, of the levels q4 int8 [E, N, K]: every expert
    has its own weights, scales and wsum."""
    E, N, K = q4.shape
    G = K // 128
    leaves = [_leaves(q4[e], 4, G, seed=seed + e) for e in range(E)]
    if s_w is not None:
        for e in range(E):
            leaves[e]["weight_scale"] = s_w[e]
    Wq = torch.stack([t["weight_packed"] for t in leaves])
    scales = torch.stack([t["weight_scale"] for t in leaves]).contiguous()
    wsum = torch.stack([cr_wsum(q4[e], G) for e in range(E)]).contiguous()
    assert Wq.shape == (E, N, K // 8) and Wq.dtype == torch.int32 and scales.shape == wsum.shape == (E, N, G)
    return leaves, Wq, scales, wsum


def _case(ops, dev, counts, N, K, seed):
    """A packed int4 bank, a routing with ``counts`` rows per expert and both quantisations of the source rows, with the
    fp64 reference of every routed row (computed once per case)."""
    E, n_rows = len(counts), sum(counts)
    q4 = _levels((E, N, K), 4, seed=seed)
    leaves, Wq, s_w, wsum = _bank(q4, seed + 100)
    assert E == 1 or not torch.equal(s_w[0], s_w[-1])
    T, src = _twice(n_rows, seed + 2)
    X = _acts(T, K, dev, seed + 3)
    out = {"E": E, "rows": n_rows, "N": N, "K": K, "G": K // 128, "counts": counts, "Wq": Wq.to(dev), "s_w": s_w.to(dev),
           "wsum": wsum.to(dev), "offsets": _offsets(counts, dev), "src": src.to(dev)}
    off = [0] + torch.tensor(counts).cumsum(0).tolist()
    for asym in (False, True):
        Xq, s_x, zp_x = ops.quantize_tokens_i8(X, symmetric=not asym)
        y64, mag = torch.zeros(n_rows, N, dtype=torch.float64), torch.zeros(n_rows, N, dtype=torch.float64)
        for e in range(E):
            lo, hi = off[e], off[e + 1]
            if hi > lo:
                rows = src[lo:hi].long()
                y64[lo:hi], mag[lo:hi] = cr.a8_linear(Xq.cpu()[rows], s_x.cpu()[rows],
                                                      None if zp_x is None else zp_x.cpu()[rows], leaves[e])
        out[asym] = (Xq, s_x, zp_x, y64, mag)
    return out


def _check(ops, c, asym, dt, gather, what):
    Xq, s_x, zp_x, y64, mag = c[asym]
    src = c["src"].long()
    if gather:
        A, sa, za, ri = Xq, s_x, zp_x, c["src"]
    else:
        A, sa, ri = Xq[src].contiguous(), s_x[src].contiguous(), None
        za = None if zp_x is None else zp_x[src].contiguous()
    ws = c["wsum"] if asym else None
    kw = dict(row_idx=ri, K=c["K"], zp_x=za, wsum=ws, out_dtype=dt)
    want = ops.gemm_i8_grouped(A, sa, c["Wq"], c["s_w"], c["offsets"], **kw)
    got = ops.moe_gemm_i8_ring_w4(A, sa, c["Wq"], c["s_w"], c["offsets"], **kw)
    torch.cuda.synchronize()
    assert got.shape == (c["rows"], c["N"])
    _same_bits(got, want, f"{what} vs gemm_i8_grouped")
    off = c["offsets"].cpu().tolist()
    for e in range(c["E"]):                      # the second yardstick: the dense W4 ring per expert on its gathered rows
        lo, hi = off[e], off[e + 1]
        if hi > lo:
            r = src[lo:hi]
            one = ops.gemm_i8_ring_w4(Xq[r].contiguous(), s_x[r].contiguous(), c["Wq"][e], c["s_w"][e], K=c["K"],
                                      zp_x=None if zp_x is None else zp_x[r].contiguous(),
                                      wsum=None if ws is None else ws[e], out_dtype=dt)
            _same_bits(got[lo:hi], one, f"{what} expert {e} vs gemm_i8_ring_w4")
    cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, c["G"]), f"{what} vs fp64")
    return got


def _all_forms(ops, c, what):
    for asym in (False, True):
        for dt in (torch.bfloat16, torch.float16):
            for gather in (True, False):
                _check(ops, c, asym, dt, gather, f"{what} asym={asym} {dt} gather={gather}")


# ---- 1: ragged experts ----------------------------------------------------------------------------------------------
def test_ragged_experts(ops, dev):
    """Empty experts first, in the middle and last; one row; exactly one tile; a tile and one row; a tile and 44 rows."""
    U, R, L = _url()
    c = _case(ops, dev, (0, 1, 256, 257, 0, 300, 0), 384, (R + 1) * U, seed=1)
    _all_forms(ops, c, "ragged")


# ---- 2: the ring's depth --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("units", ["1", "2", "L", "R+1", "2R+3"])
def test_ring_depth(ops, dev, units):
    """K-tiles (= weight groups): the prologue alone, exactly one trip round the ring, the lead, the first wrap, two
    trips with an odd K-tile left over."""
    U, R, L = _url()
    K = U * {"1": 1, "2": 2, "L": L, "R+1": R + 1, "2R+3": 2 * R + 3}[units]
    c = _case(ops, dev, (130, 0, 300), 300, K, seed=K)
    _all_forms(ops, c, f"K={K}")


# ---- 3: the tile walk -----------------------------------------------------------------------------------------------
def test_many_small_experts(ops, dev):
    """E = 64 with 3 rows each: every tile clamps 253 of its rows to its own expert's last row, and the B and scale
    bases move by e N K/2 and e N G from tile to tile."""
    U, R, L = _url()
    c = _case(ops, dev, (3,) * 64, 130, (R + 1) * U, seed=3)
    _all_forms(ops, c, "E=64")


def test_one_expert_owns_all_rows(ops, dev):
    """700 rows on expert 5 of 8: 3 of the 3 + 8 m-tile slots work, the other 8 exit."""
    U, R, L = _url()
    c = _case(ops, dev, (0, 0, 0, 0, 0, 700, 0, 0), 200, (R + 1) * U, seed=4)
    _all_forms(ops, c, "one expert")


def test_more_than_group_m_tile_slots(ops, dev):
    """16 + 0 + 18 tiles in 34 + 3 = 37 slots: more than the 32 that walk the n-tiles together, over 2 n-tiles."""
    U, R, L = _url()
    c = _case(ops, dev, (4000, 0, 4500), 300, U, seed=5)
    for asym, dt, gather in ((True, torch.bfloat16, True), (False, torch.float16, False)):
        _check(ops, c, asym, dt, gather, f"37 slots asym={asym} gather={gather}")


def _raw(ops, name, Xq_ptr, K, row_idx, n_rows, offsets, E, Wq_ptr, fmt, N, s_x, zp_x, s_w, G, wsum, Y, ldy, x_rows):
    from quantool_amd.hip import _lib

    extra = (x_rows,) if name == NAME else ()
    _lib.check(name, getattr(_lib.load(), name)(
        Xq_ptr, K, ops._ptr(row_idx), n_rows, offsets.data_ptr(), E, Wq_ptr, fmt, N, s_x.data_ptr(), ops._ptr(zp_x),
        s_w.data_ptr(), G, ops._ptr(wsum), Y.data_ptr(), ops._dtype_code(Y), ldy, *extra, ops._stream()))


def test_an_all_empty_table_writes_nothing(ops, dev):
    from quantool_amd.hip import _lib

    U, R, L = _url()
    E, n_rows, N, K = 5, 300, 260, 2 * U
    G = K // U
    Xq = torch.ones(n_rows, K, dtype=torch.int8, device=dev)
    Wq = torch.full((E, N, K // 8), 0x11111111, dtype=torch.int32, device=dev)
    s_x, s_w = torch.ones(n_rows, device=dev), torch.ones(E, N, G, device=dev)
    zp_x = torch.ones(n_rows, dtype=torch.int32, device=dev)
    wsum = torch.full((E, N, G), 128, dtype=torch.int32, device=dev)
    for table in ([0] * (E + 1), [7] * (E + 1), [9, 5, 5, 2, 0, 0]):       # empty, empty at 7, descending: clamped empty
        for zp, ws in ((None, None), (zp_x, wsum)):
            Y = _sentinel((n_rows, N), torch.bfloat16, dev)
            offsets = torch.tensor(table, dtype=torch.int32, device=dev)
            _raw(ops, NAME, Xq.data_ptr(), K, None, n_rows, offsets, E, Wq.data_ptr(), _lib.QT_W_INT4_PACKED, N, s_x, zp,
                 s_w, G, ws, Y, N, n_rows)
            torch.cuda.synchronize()
            assert _untouched(Y), table


# ---- 4: lane, slot, expert, group and nibble maps -------------------------------------------------------------------
@pytest.mark.parametrize("scales", ["unit", "eG+g+1"])
def test_identity_activations_read_the_expert_the_group_and_the_nibble(ops, dev, scales):
    """Xq = the K x K identity, unit s_x, no zero-point: routed row r of expert e, gathered from source row k, is
    s_w[e, n, k // 128] (float)W[e][n, k] exactly.  With unit scales that pins the expert, the gathered row and the
    nibble; with s_w[e, n, g] = e G + g + 1, different for every (expert, group), also whose scale was folded."""
    U, R, L = _url()
    K, N, counts = (R + 1) * U, 96, (300, 0, 515, 1)
    E, n_rows, G = len(counts), sum(counts), K // U
    W = _levels((E, N, K), 4, seed=77)
    assert len({tuple(r) for r in W.reshape(E * N, K).tolist()}) == E * N and not torch.equal(W[0], W[2])
    assert not torch.equal(W, W.flip(2))
    if scales == "unit":
        s_w = torch.ones(E, N, G)
    else:
        s_w = (torch.arange(E)[:, None, None] * G + torch.arange(G)[None, None, :] + 1).float().expand(E, N, G).contiguous()
        assert s_w.unique().numel() == E * G
    _, Wq, s_w, _ = _bank(W, 1, s_w=s_w)
    src = torch.randperm(K, generator=torch.Generator().manual_seed(6))[:n_rows].to(torch.int32)
    assert n_rows < K and not torch.equal(src, src.sort().values)
    expert = torch.repeat_interleave(torch.arange(E), torch.tensor(counts))
    want = W[expert, :, src.long()].float() * s_w[expert, :, src.long() // U]          # [rows, N]
    assert float(want.abs().max()) <= 2048                                            # exact in fp16
    Xq = torch.eye(K, dtype=torch.int8, device=dev)
    Y = ops.moe_gemm_i8_ring_w4(Xq, torch.ones(K, device=dev), Wq.to(dev), s_w.to(dev), _offsets(counts, dev),
                                row_idx=src.to(dev), K=K, out_dtype=torch.float16)
    torch.cuda.synchronize()
    _same_bits(Y.cpu(), want.to(torch.float16).contiguous(), f"identity, {scales} scales")


def test_row_indices_are_clamped_into_xq(ops, dev):
    """An index below 0 reads row 0, one past the end reads the last row (the tiled kernel leaves this to the caller)."""
    U, R, L = _url()
    c = _case(ops, dev, (40, 270), 64, 2 * U, seed=8)
    Xq, s_x, zp_x, _, _ = c[True]
    T = Xq.shape[0]
    wild = c["src"].clone()
    tame = c["src"].clone()
    wild[::3], tame[::3] = -5, 0
    wild[1::3], tame[1::3] = 2 ** 31 - 1, T - 1
    kw = dict(K=c["K"], zp_x=zp_x, wsum=c["wsum"])
    got = ops.moe_gemm_i8_ring_w4(Xq, s_x, c["Wq"], c["s_w"], c["offsets"], row_idx=wild, **kw)
    want = ops.gemm_i8_grouped(Xq, s_x, c["Wq"], c["s_w"], c["offsets"], row_idx=tame, **kw)
    torch.cuda.synchronize()
    _same_bits(got, want, "clamped row_idx")


def test_gathered_rows_past_2_31_bytes(ops, dev):
    """Xq of exactly 2^32 bytes: a gathered row's 32-bit byte offset is unsigned, so rows on both sides of 2^31 and the
    very last row are read where the tiled kernel's 64-bit addresses read them."""
    K, N, counts = 4096, 48, (19, 21)
    G = K // 128
    x_rows = 2 ** 32 // K
    picks = torch.tensor([0, 1, x_rows // 2 - 1, x_rows // 2, x_rows // 2 + 5, x_rows - 2, x_rows - 1])
    Xq = torch.zeros(x_rows, K, dtype=torch.int8, device=dev)
    Xq[picks.to(dev)] = _levels((len(picks), K), 8, seed=9).to(dev)
    g = torch.Generator().manual_seed(10)
    src = picks[torch.randint(0, len(picks), (sum(counts),), generator=g)].to(torch.int32)
    s_x = (torch.rand(x_rows, generator=g) * 1e-2 + 1e-3).to(dev)
    zp_x = torch.randint(-20, 21, (x_rows,), generator=g, dtype=torch.int32).to(dev)
    leaves, Wq, s_w, wsum = _bank(_levels((2, N, K), 4, seed=11), 12)
    Wq, s_w, wsum = Wq.to(dev), s_w.to(dev), wsum.to(dev)
    offsets = _offsets(counts, dev)
    assert ops.moe_gemm_i8_ring_w4_supported(Xq, Wq, s_w, src.to(dev))
    kw = dict(row_idx=src.to(dev), K=K, zp_x=zp_x, wsum=wsum)
    got = ops.moe_gemm_i8_ring_w4(Xq, s_x, Wq, s_w, offsets, **kw)
    want = ops.gemm_i8_grouped(Xq, s_x, Wq, s_w, offsets, **kw)
    torch.cuda.synchronize()
    _same_bits(got, want, "2^32-byte Xq")
    rows = Xq[src.long().to(dev)].cpu()
    for e, (lo, hi) in enumerate(((0, counts[0]), (counts[0], sum(counts)))):
        sel = src.long()[lo:hi]
        y64, mag = cr.a8_linear(rows[lo:hi], s_x.cpu()[sel], zp_x.cpu()[sel], leaves[e])
        cr.assert_within(got[lo:hi], y64, cr.gemm_i8_tolerance(got[lo:hi].cpu(), mag, G), f"expert {e} vs fp64")


# ---- 5: the order of the group fold ---------------------------------------------------------------------------------
def _to16(y32, dt):
    return torch.from_numpy(y32).to(dt)


def test_groups_are_folded_in_ascending_order(ops, dev):
    """No bias to cancel against, so the inputs cancel themselves: groups g and g + G/2 hold negated weights, equal scales
    and equal activations, hence t_{g+G/2} = -t_g exactly and the exact sum is 0.  What the 16-bit output shows is
    then the rounding residue of the fp32 fold, which depends on its order: the ascending and the descending fold,
    re-derived here with one rounding per product and sum, differ in at least half of the outputs (asserted below, on
    the CPU; a pairwise-interleaved order would give all zeros).  The kernel has to match the ascending fold -- and the
    tiled grouped kernel -- to the bit, for two experts with different data."""
    G, N, M, E = 8, 384, 4, 2
    K, Hf = G * 128, G // 2
    gen = torch.Generator().manual_seed(1)
    q_half = torch.randint(-7, 8, (E, N, Hf * 128), generator=gen, dtype=torch.int8)    # -(-8) is no int4 level
    q = torch.cat([q_half, -q_half], 2).contiguous()
    x_blk = torch.randint(-128, 128, (E * M, Hf * 128), generator=gen, dtype=torch.int8)
    Xq = torch.cat([x_blk, x_blk], 1).contiguous()
    u = torch.rand(E, N, Hf, generator=gen) * 0.02 + 1e-4
    s_w = torch.cat([u, u], 2).contiguous()
    zp_x = torch.full((E * M,), 37, dtype=torch.int32)
    s_x = torch.full((E * M,), 0.0123, dtype=torch.float32)
    leaves, Wq, s_w, wsum = _bank(q, 0, s_w=s_w)
    asc, desc = [], []
    for e in range(E):
        xi, qi = Xq[e * M:(e + 1) * M].numpy().astype(np.int64), q[e].numpy().astype(np.int64)
        t = np.stack([xi[:, j * 128:(j + 1) * 128] @ qi[:, j * 128:(j + 1) * 128].T
                      - 37 * wsum[e][:, j].numpy().astype(np.int64)[None, :] for j in range(G)], 2)
        assert (t[:, :, :Hf] == -t[:, :, Hf:]).all()
        zero, sx = np.zeros(N, np.float32), s_x[:M].numpy()
        asc.append(_fold32(t, s_w[e].numpy(), sx, zero, range(G)))
        desc.append(_fold32(t, s_w[e].numpy(), sx, zero, range(G - 1, -1, -1)))
        inter = _fold32(t, s_w[e].numpy(), sx, zero, [g for p in range(Hf) for g in (p, p + Hf)])
        assert not inter.any()
    asc, desc = np.concatenate(asc), np.concatenate(desc)
    assert not np.array_equal(asc[:M], asc[M:])
    offsets = _offsets((M, M), dev)
    for dt in (torch.float16, torch.bfloat16):
        a16, d16 = _to16(asc, dt), _to16(desc, dt)
        differ = (a16.view(torch.int16) != d16.view(torch.int16)).float().mean().item()
        print(f"{dt} outputs that differ between the ascending and the descending fold: {differ:.4f}")
        assert differ >= 0.5
        kw = dict(K=K, zp_x=zp_x.to(dev), wsum=wsum.to(dev), out_dtype=dt)
        want = ops.gemm_i8_grouped(Xq.to(dev), s_x.to(dev), Wq.to(dev), s_w.to(dev), offsets, **kw)
        got = ops.moe_gemm_i8_ring_w4(Xq.to(dev), s_x.to(dev), Wq.to(dev), s_w.to(dev), offsets, **kw)
        torch.cuda.synchronize()
        _same_bits(got, want, f"group order vs the tiled grouped kernel, {dt}")
        _same_bits(got.cpu(), a16.contiguous(), f"group order vs the ascending CPU fold, {dt}")


# ---- 6: raw C ABI calls ---------------------------------------------------------------------------------------------
def test_caller_owned_y_keeps_its_padding(ops, dev):
    """ldy = N + 17, offsets[E] < R and rows behind R: everything outside Y[r < offsets[E], n < N] keeps its sentinel."""
    from quantool_amd.hip import _lib

    U, R, L = _url()
    counts, N, K = (257, 0, 130), 200, (R + 1) * U
    c = _case(ops, dev, counts, N, K, seed=12)
    Xq, s_x, zp_x, _, _ = c[True]
    live, ldy = sum(counts), N + 17
    n_rows = live + 40                                           # 40 dropped routing slots
    row_idx = torch.cat([c["src"], torch.zeros(40, dtype=torch.int32, device=dev)])
    Ys = {}
    for name in ("qt_gemm_i8_grouped", NAME):
        Ys[name] = _sentinel((n_rows + 3, ldy), torch.bfloat16, dev)
        _raw(ops, name, Xq.data_ptr(), K, row_idx, n_rows, c["offsets"], c["E"], c["Wq"].data_ptr(),
             _lib.QT_W_INT4_PACKED, N, s_x, zp_x, c["s_w"], c["G"], c["wsum"], Ys[name], ldy, Xq.shape[0])
    torch.cuda.synchronize()
    Y = Ys[NAME]
    assert _untouched(Y[:, N:]) and _untouched(Y[live:]) and not _untouched(Y[:live, :N])
    _same_bits(Y[:live, :N].contiguous(), Ys["qt_gemm_i8_grouped"][:live, :N].contiguous(), "ldy > N")
    _same_bits(Y, Ys["qt_gemm_i8_grouped"], "the whole buffer")


def test_refusals_write_nothing_and_name_the_reason(ops, dev):
    from quantool_amd.hip import _lib
    from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

    U, R, L = _url()
    E, M, N, K = 2, 20, 32, 4 * 128
    Kbig = 32768 + U
    G = K // U
    # every pointer below lies inside one of these buffers with room for the whole operand behind it; the cases whose
    # sizes are numbers only (2^32, E, tiles) come with an all-zero offsets table and row_idx
    xbuf = torch.ones(M * Kbig + 32, dtype=torch.int8, device=dev)
    wbuf = torch.zeros(E * N * Kbig + 32, dtype=torch.int8, device=dev)
    assert xbuf.data_ptr() % 16 == 0 and wbuf.data_ptr() % 16 == 0
    s_x = torch.ones(M, device=dev)
    s_w = torch.ones(E * N * (Kbig // 128), device=dev)
    zp = torch.zeros(M, dtype=torch.int32, device=dev)
    offsets = torch.tensor([0, 8, M], dtype=torch.int32, device=dev)
    zeros = torch.zeros(4098, dtype=torch.int32, device=dev)
    row_idx = torch.zeros(M, dtype=torch.int32, device=dev)
    Y = _sentinel((M, N), torch.bfloat16, dev)
    X, W, I8, I4 = xbuf.data_ptr(), wbuf.data_ptr(), _lib.QT_W_INT8, _lib.QT_W_INT4_PACKED
    cases = {     # (Xq, K, row_idx, R, offsets, E, Wq, format, N, zp_x, G, x_rows), reason
        "int8 format": ((X, K, None, M, offsets, E, W, I8, N, None, G, M), "run on qt_gemm_i8_ring_grouped"),
        "G == 1": ((X, K, None, M, offsets, E, W, I4, N, None, 1, M), "run on qt_gemm_i8_grouped"),
        "K % U != 0": ((X, K + 16, None, M, offsets, E, W, I4, N, None, G, M), "not a multiple of the k-unit"),
        "K > 32768": ((X, Kbig, None, M, offsets, E, W, I4, N, None, Kbig // U, M), "32768"),
        "Xq misaligned": ((X + 1, K, None, M, offsets, E, W, I4, N, None, G, M), "Xq is not 16-byte aligned"),
        "Wq misaligned": ((X, K, None, M, offsets, E, W + 4, I4, N, None, G, M), "Wq is not 16-byte aligned"),
        "x_rows K > 2^32": ((X, K, row_idx, M, zeros, E, W, I4, N, None, G, 2 ** 32 // K + 1), "2^32"),
        "E > 4096": ((X, K, None, M, zeros, 4097, W, I4, N, None, G, M), "4096"),
        "R > 2^31 - 1": ((X, K, None, 2 ** 31, zeros, E, W, I4, N, None, G, 2 ** 31), "too large"),
        "too many tiles": ((X, K, None, 2 ** 31 - 1, zeros, E, W, I4, 2 ** 20, None, G, 2 ** 31 - 1), "too many tiles"),
        "x_rows < R": ((X, K, None, M, offsets, E, W, I4, N, None, G, M - 1), "without row_idx"),
        "zp_x without wsum": ((X, K, None, M, offsets, E, W, I4, N, zp, G, M), "zp_x needs wsum"),
    }
    for what, ((xq, k, ri, n_rows, off, e, wq, fmt, n, z, g, x_rows), reason) in cases.items():
        with pytest.raises(HipBackendError) as err:
            _raw(ops, NAME, xq, k, ri, n_rows, off, e, wq, fmt, n, s_x, z, s_w, g, None, Y, max(n, N), x_rows)
        assert err.value.status == QT_ERR_INVALID, what
        assert reason in str(err.value), (what, str(err.value))
    torch.cuda.synchronize()
    assert _untouched(Y)
    # the same operands, legal: the call goes through (so the refusals above were about what they name)
    _raw(ops, NAME, X, K, row_idx, M, offsets, E, W, I4, N, s_x, None, s_w, G, None, Y, N, 2 ** 32 // K)
    torch.cuda.synchronize()
    assert not _untouched(Y)


# ---- 7: the module, end to end --------------------------------------------------------------------------------------
def test_tiny_mixtral_is_the_same_with_and_without_the_w4_ring(ops, dev, tmp_path, monkeypatch):
    """The tiny Mixtral W4A8 checkpoint on a prompt past the skinny range: logits and perplexity with both banks' products
    on the ring equal those with none on it, to the bit."""
    import quantool_amd.methods  # noqa: F401
    from quantool_amd.core import QuantizerRegistry
    from quantool_amd.engine.qlinear import QuantizedExperts, load_quantized
    from quantool_amd.evaluate import perplexity
    from tests.test_gpu_moe import _tiny_mixtral

    monkeypatch.chdir(tmp_path)
    model = _tiny_mixtral(dev)
    g = torch.Generator().manual_seed(2)
    data = [{"input_ids": torch.randint(0, 512, (48,), generator=g)} for _ in range(8)]
    q = QuantizerRegistry.create("smoothquant", model_id="synthetic/tiny-mixtral")
    q.quantize(model=model, level="W4A8", dataset=data, num_calibration_samples=8, max_seq_length=64,
               shuffle_calibration_samples=False)
    torch.cuda.synchronize()
    q.save_pretrained(str(tmp_path / "ckpt"))
    del q, model
    model = load_quantized(tmp_path / "ckpt", device=dev)
    banks = [m for m in model.modules() if isinstance(m, QuantizedExperts)]
    assert len(banks) == 2 and all(b.int4 and b.gate_up_scale.shape[2] * 128 == b.hidden_dim
                                   and b.down_scale.shape[2] * 128 == b.intermediate_dim for b in banks)
    ids = torch.randint(0, 512, (6, 96), generator=torch.Generator().manual_seed(11))
    assert ids[:2].numel() > QuantizedExperts.grouped_max_tokens
    counter = _Counter(monkeypatch, ops, "moe_gemm_i8_ring_w4")
    logits, ppl, calls = {}, {}, {}
    for setting in (0, 1):
        monkeypatch.setattr(QuantizedExperts, "ring_w4_min_rows_per_expert", setting)
        before = counter.n
        with torch.no_grad():
            logits[setting] = model(input_ids=ids[:2].to(dev)).logits
        ppl[setting] = perplexity(model, ids, batch_size=4)["perplexity"]
        torch.cuda.synchronize()
        calls[setting] = counter.n - before
    assert calls[0] == 0
    assert calls[1] >= 2 * len(banks) * 3              # both products of both banks, in the forward and both batches
    assert torch.isfinite(logits[1].float()).all()
    _same_bits(logits[1], logits[0], "W4A8 logits, ring_w4_min_rows_per_expert 1 vs 0")
    assert ppl[1] == ppl[0]
