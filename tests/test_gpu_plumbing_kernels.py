"""The plumbing kernels every calibrated Linear goes through (csrc/quant.hip, csrc/stats.hip, csrc/hessian.hip) one by one
against plain numpy or the CPU oracle, evaluated on the values the device actually holds (a 16-bit tensor widened to
fp32): the min/max observer and its fused form, the column gather, pack / dequantise, the activation statistics and the
one-pass Hessian prepare.  The reference is never another device kernel.

The shared grid: 1, 3, 4, 63, 64, 65 and 300 rows; bf16, fp16 and fp32; W contiguous, a row-strided view (the pad holds
a sentinel), a view that starts one element into its buffer (not 16-byte aligned) and, for the 16-bit dtypes, a view of
pitch K + 4 (every other row starts 8 bytes off a 16-byte boundary, so both load paths of the fused kernel run in one
launch).  Every case draws from its own seed.

"Equal" means equal as numbers (``np.array_equal`` on finite values): every rounding is pinned, the sign of a zero is
not.  Pinned exactly: the observer's four tables, the gather, the packed words, the dequantised weight in all three
output dtypes, channel min / max, ``dead`` / ``diag`` / the off-diagonal of the prepared Hessian.  Pinned by a bound:
the |x| sums ((n + 3) 2^-24, derived at the test) and the damped diagonal (1 ulp: the mean is an fp64 sum whose order
differs).  Each planted edge is asserted on the reference side, so no test passes by missing its edge.
"""
import numpy as np
import pytest
import torch

from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError
from tests.util import synth_weight

pytestmark = pytest.mark.gpu

f32 = np.float32
ROWS = (1, 3, 4, 63, 64, 65, 300)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
# (group_size, K): groups shorter than a wave, lane-uneven (40, 192, channel-wise 200 / 264), longer than 64 (the lane loop)
PAIRS = ((32, 96), (40, 200), (64, 192), (128, 256), (128, 1152), (192, 576), (512, 1024), (1024, 2048), (-1, 200),
         (-1, 264), (-1, 1152))
EPS = 2.0 ** -24            # unit roundoff of fp32
SCALE_FLOOR = f32(2.0 ** -23)   # the observer's clamp (torch.finfo(float32).eps)
SENTINEL = 7.0


# ------------------------------------------------------------------------------------------------------ helpers
def _rng(*key):
    return np.random.default_rng([int(k) % 65536 for k in key])


def _weights(R, K, *key, std=0.05):
    return synth_weight(R, K, seed=[int(k) % 65536 for k in key], std=std)


def _host(t):
    t = t.detach().cpu()
    return t.float().numpy() if t.is_floating_point() else t.numpy()


def _round_to(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dtype).float().numpy()


def _layouts(w, dtype, dev):
    """(name, device view, fp32 values): the same values contiguous, row-strided (ldw = K + 24, the pad holds a
    sentinel), starting one element into a buffer and, 16-bit only, at pitch K + 4."""
    R, K = w.shape
    base = torch.from_numpy(w).to(dtype)
    vals = base.float().numpy()
    pad = torch.full((R, K + 24), SENTINEL, dtype=dtype)
    pad[:, :K] = base
    flat = torch.full((R * K + 1,), SENTINEL, dtype=dtype)
    flat[1:] = base.reshape(-1)
    off = flat.to(dev)[1:].view(R, K)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()              # a misaligned row is in play
    out = [("contiguous", base.to(dev), vals), ("strided", pad.to(dev)[:, :K], vals), ("offset", off, vals)]
    if dtype != torch.float32:
        p4 = torch.full((R, K + 4), SENTINEL, dtype=dtype)
        p4[:, :K] = base
        v = p4.to(dev)[:, :K]
        if R > 1 and K % 8 == 0:
            # rows 0, 2, .. aligned (vector loads), rows 1, 3, .. 8 bytes off (scalar loads)
            assert v.data_ptr() % 16 == 0 and (v.data_ptr() + v.stride(0) * v.element_size()) % 16 == 8
        out.append(("pitch4", v, vals))
    return out


EDGES = ("zero", "positive", "negative", "negzero", "largest")


def _plant(w, gs, dtype, rot):
    """Plants the five edge groups in ``w`` (in place) and returns {edge: (row, group)}.  With fewer than five groups in
    the whole matrix (few rows, channel-wise) as many as fit, starting at edge ``rot``."""
    R, K = w.shape
    g = K if gs <= 0 else gs
    G = K // g
    n = R * G
    if n >= 5:
        flat, names = (0, n - 1, n // 2, n // 4, 3 * n // 4), EDGES
    else:
        flat, names = tuple(range(n)), tuple(EDGES[(rot + i) % 5] for i in range(n))
    assert len(set(flat)) == len(flat)
    where = {}
    for name, f in zip(names, flat):
        r, gi = divmod(f, G)
        sl = w[r, gi * g:(gi + 1) * g]
        if name == "zero":
            sl[:] = 0
        elif name == "positive":
            sl[:] = np.abs(sl) + f32(0.01)
        elif name == "negative":
            sl[:] = -np.abs(sl) - f32(0.01)
        elif name == "negzero":
            sl[:] = 0
            sl[::2] = f32(-0.0)
        else:
            sl[g // 2] = f32(torch.finfo(dtype).max)
        where[name] = (r, gi)
    return where


def _check_planted(where, vals, gs, symmetric, bits, dtype, s, z):
    """On the REFERENCE: every planted edge does what it was planted for."""
    K = vals.shape[1]
    g = K if gs <= 0 else gs
    qmin, qmax = f32(-(2 ** (bits - 1))), f32(2 ** (bits - 1) - 1)
    for name, (r, gi) in where.items():
        grp = vals[r, gi * g:(gi + 1) * g]
        if name in ("zero", "negzero"):
            assert np.all(grp == 0) and (name == "zero" or np.signbit(grp).any())
            # the clamp at eps; the zero point is 0 symmetric and qmin - 0 / scale = qmin asymmetric
            assert s[r, gi] == SCALE_FLOOR and z[r, gi] == (0 if symmetric else qmin)
        elif name == "positive":
            assert grp.min() > 0
            if not symmetric:                                            # min clamps to 0: zero point at qmin
                assert z[r, gi] == qmin and s[r, gi] == grp.max() / f32(qmax - qmin)
        elif name == "negative":
            assert grp.max() < 0
            if not symmetric:                                            # max clamps to 0: zero point at qmax
                assert z[r, gi] == qmax and s[r, gi] == -grp.min() / f32(qmax - qmin)
        else:
            big = f32(torch.finfo(dtype).max)
            assert grp.max() == big and np.isfinite(s[r, gi])
            if symmetric:
                assert s[r, gi] == big / f32((qmax - qmin) / 2)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(z))


def _perm_dead(K, rng):
    perm = rng.permutation(K).astype(np.int32)
    dead = (rng.random(K) < 0.03).astype(np.uint8)
    dead[0] = dead[K - 1] = 1
    return perm, dead


def _gathered(vals, perm, dead):
    want = vals[:, perm] if perm is not None else vals.copy()
    if dead is not None:
        want[:, dead.astype(bool)] = 0
    return np.ascontiguousarray(want)


def _dev(a, dev):
    return None if a is None else torch.from_numpy(a).to(dev)


# ----------------------------------------------------------------------------------------- qt_group_minmax_qparams
@pytest.mark.parametrize("gs,K", PAIRS)
def test_observer_equals_the_oracle(ops, dev, oracle, gs, K):
    """rows x dtype x layout x symmetric / asymmetric x 2 / 3 / 4 / 8 bits: scale, zp and the two group-major tables
    EQUAL ``oracle.minmax_qparams`` (upstream's calculate_qparams in fp32; its 2- and 3-bit ranges are checked against
    upstream's formula in tests/test_oracle_kat.py).  Planted in every matrix: an all-zero group (scale at the 2^-23
    clamp; zero point 0 symmetric, qmin = qmin - 0 / scale asymmetric), an all-positive one (min clamps to 0, asymmetric
    zero point qmin), an all-negative one (qmax), one whose only non-zeros are -0.0 and one holding the dtype's largest
    finite value."""
    for R in ROWS:
        base = _weights(R, K, 1, R, K, gs)
        for dtype in DTYPES:
            w = base.copy()
            where = _plant(w, gs, dtype, R)
            lay = _layouts(w, dtype, dev)
            vals = lay[0][2]
            for symmetric in (True, False):
                for bits in (2, 3, 4, 8):
                    s, z = oracle.minmax_qparams(vals, gs, symmetric, bits)
                    _check_planted(where, vals, gs, symmetric, bits, dtype, s, z)
                    for name, W, _ in lay:
                        got = ops.group_minmax_qparams(W, gs, symmetric, bits)
                        for what, t, want in zip(("scale", "zp", "scale_t", "zp_t"), got, (s, z, s.T, z.T)):
                            assert np.array_equal(_host(t), want), (R, dtype, name, symmetric, bits, what)


def test_observer_and_gather_above_32768_rows(ops, dev, oracle):
    """Beyond 32768 rows both entry points chunk the rows and offset their pointers; with G = 3 the group-major tables
    (pitch R, not the chunk's row count) differ from the row-major ones.  fp16, row-strided, asymmetric, 8 bits."""
    R, K, gs = 32768 + 65, 96, 32
    w = _weights(R, K, 2, R, K)
    where = _plant(w, gs, torch.float16, 0)
    _, W, vals = _layouts(w, torch.float16, dev)[1]
    assert W.stride(0) > K
    s, z = oracle.minmax_qparams(vals, gs, False, 8)
    _check_planted(where, vals, gs, False, 8, torch.float16, s, z)
    assert not np.array_equal(s.T.reshape(R, 3), s)
    got = ops.group_minmax_qparams(W, gs, False, 8)
    for what, t, want in zip(("scale", "zp", "scale_t", "zp_t"), got, (s, z, s.T, z.T)):
        assert np.array_equal(_host(t), want), what
    perm, dead = _perm_dead(K, _rng(2, 1))
    out = ops.weight_gather_f32(W, _dev(perm, dev), _dev(dead, dev))
    assert np.array_equal(_host(out), _gathered(vals, perm, dead))


# -------------------------------------------------------------------------------------------- qt_weight_gather_f32
@pytest.mark.parametrize("K", [136, 200, 256, 264, 1000])
def test_weight_gather_equals_numpy_indexing(ops, dev, K):
    """out[r][s] = dead[s] ? 0 : float(W[r][perm[s]]): exact, with and without ``perm`` and ``dead`` (positions 0 and
    K - 1 among the dead)."""
    perm, dead = _perm_dead(K, _rng(3, K))
    assert dead[0] and dead[K - 1]
    for R in ROWS:
        w = _weights(R, K, 3, R, K, std=1.0)
        for dtype in DTYPES:
            for name, W, vals in _layouts(w, dtype, dev):
                for pm in (perm, None):
                    for dd in (dead, None):
                        got = ops.weight_gather_f32(W, _dev(pm, dev), _dev(dd, dev))
                        assert np.array_equal(_host(got), _gathered(vals, pm, dd)), (R, dtype, name, pm is None, dd is None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_gather_into_a_row_slice_leaves_its_neighbours(ops, dev, dtype):
    R, K = 65, 264
    perm, dead = _perm_dead(K, _rng(4, K))
    w = _weights(R, K, 4, R, K, std=1.0)
    for name, W, vals in _layouts(w, dtype, dev):
        big = torch.full((R + 10, K), SENTINEL, dtype=torch.float32, device=dev)
        got = ops.weight_gather_f32(W, _dev(perm, dev), _dev(dead, dev), out=big[3:3 + R])
        assert got.data_ptr() == big[3:3 + R].data_ptr()
        host = _host(big)
        assert np.array_equal(host[3:3 + R], _gathered(vals, perm, dead)), name
        assert np.all(host[:3] == SENTINEL) and np.all(host[3 + R:] == SENTINEL), name


# ---------------------------------------------------------------------------------------- qt_weight_gather_qparams
# G = 1, 2, 5, 9 at group 64 (the four waves of a workgroup take uneven numbers of groups) and K with K % V != 0 (scalar
# loads; V = 8 16-bit / 4 fp32 elements per 16 bytes) and K % 4 != 0 (scalar stores)
FUSED_EXTRA = ((64, 64), (64, 128), (64, 320), (64, 576), (-1, 100), (-1, 50))


def _fused_case(ops, dev, oracle, gs, K, rows, dtypes):
    g = K if gs <= 0 else gs
    G = K // g
    perm, dead = _perm_dead(K, _rng(5, K, gs))
    for R in rows:
        base = _weights(R, K, 5, R, K, gs)
        for dtype in dtypes:
            w = base.copy()
            where = _plant(w, gs, dtype, R + 1)
            lay = _layouts(w, dtype, dev)
            vals = lay[0][2]
            for pm, dd in ((perm, dead), (None, None)):
                want_out = _dev(_gathered(vals, pm, dd), dev)
                pm_d, dd_d = _dev(pm, dev), _dev(dd, dev)
                for symmetric in (True, False):
                    for bits in (4, 8):
                        s, z = oracle.minmax_qparams(vals, gs, symmetric, bits)
                        _check_planted(where, vals, gs, symmetric, bits, dtype, s, z)
                        for name, W, _ in lay:
                            out = torch.full((R, K), SENTINEL, dtype=torch.float32, device=dev)
                            sc = torch.full((R, G), SENTINEL, dtype=torch.float32, device=dev)
                            zp = torch.full((R, G), SENTINEL, dtype=torch.float32, device=dev)
                            wide_s = torch.full((G, R + 56), -1.0, dtype=torch.float32, device=dev)
                            wide_z = torch.full((G, R + 56), -1.0, dtype=torch.float32, device=dev)
                            ops.weight_gather_qparams(W, pm_d, dd_d, gs, symmetric, bits, out=out, scale=sc, zp=zp,
                                                      scale_t=wide_s[:, 24:24 + R], zp_t=wide_z[:, 24:24 + R])
                            tag = (R, dtype, name, pm is None, symmetric, bits)
                            assert torch.equal(out, want_out), tag       # the numpy gather, uploaded; -0.0 == 0.0
                            assert np.array_equal(_host(sc), s) and np.array_equal(_host(zp), z), tag
                            ws, wz = _host(wide_s), _host(wide_z)
                            assert np.array_equal(ws[:, 24:24 + R], s.T) and np.array_equal(wz[:, 24:24 + R], z.T), tag
                            for wt in (ws, wz):
                                assert np.all(wt[:, :24] == -1) and np.all(wt[:, 24 + R:] == -1), tag


@pytest.mark.parametrize("gs,K", PAIRS + FUSED_EXTRA)
def test_fused_gather_qparams_equals_the_oracle_and_numpy(ops, dev, oracle, gs, K):
    """One read of W for the observer and the sweep's working copy, against the oracle's tables and numpy's gather
    directly (not against the two-pass kernels, which share the scale arithmetic line for line).  Aligned rows with
    K % V == 0 take 16-byte loads, everything else scalar loads: the offset view and every other row of the pitch K + 4
    view take the scalar path at a K where the contiguous tensor takes the vector one.  The group-major tables are a
    column range of wider sentinel-filled ones."""
    _fused_case(ops, dev, oracle, gs, K, ROWS, DTYPES)
    if K == 100:
        assert K % 8 and K % 4 == 0                                      # scalar loads (16-bit), vector stores
    if K == 50:
        assert K % 8 and K % 4                                           # scalar loads (16-bit and fp32), scalar stores


@pytest.mark.parametrize("dtype,K", [(torch.bfloat16, 81920), (torch.float32, 40960)])
def test_fused_gather_qparams_at_the_lds_limit(ops, dev, oracle, dtype, K):
    """A row of exactly 160 KiB still fits the LDS: it must work and equal the reference."""
    R = 2
    assert K * torch.empty(0, dtype=dtype).element_size() == 160 * 1024
    w = _weights(R, K, 6, K)
    W = torch.from_numpy(w).to(dtype)
    vals = W.float().numpy()
    perm, dead = _perm_dead(K, _rng(6, K, 1))
    for symmetric, bits in ((False, 8), (True, 4)):
        s, z = oracle.minmax_qparams(vals, -1, symmetric, bits)
        out = torch.full((R, K), SENTINEL, dtype=torch.float32, device=dev)
        sc = torch.full((R, 1), SENTINEL, dtype=torch.float32, device=dev)
        zp = torch.full((R, 1), SENTINEL, dtype=torch.float32, device=dev)
        st, zt = torch.empty((1, R), dtype=torch.float32, device=dev), torch.empty((1, R), dtype=torch.float32, device=dev)
        ops.weight_gather_qparams(W.to(dev), _dev(perm, dev), _dev(dead, dev), -1, symmetric, bits, out=out, scale=sc,
                                  zp=zp, scale_t=st, zp_t=zt)
        assert np.array_equal(_host(out), _gathered(vals, perm, dead))
        assert np.array_equal(_host(sc), s) and np.array_equal(_host(zp), z)
        assert np.array_equal(_host(st), s.T) and np.array_equal(_host(zt), z.T)


@pytest.mark.parametrize("dtype,K", [(torch.bfloat16, 81928), (torch.float32, 40964)])
def test_fused_gather_qparams_refuses_a_row_beyond_the_lds(ops, dev, dtype, K):
    """One vector past 160 KiB: QT_ERR_INVALID (engine/gptq_linear.py chooses the two-pass fallback by the same limit),
    and nothing is written."""
    R = 2
    W = torch.from_numpy(_weights(R, K, 7, K)).to(dtype).to(dev)
    out = torch.full((R, K), SENTINEL, dtype=torch.float32, device=dev)
    sc = torch.full((R, 1), SENTINEL, dtype=torch.float32, device=dev)
    zp = torch.full((R, 1), SENTINEL, dtype=torch.float32, device=dev)
    with pytest.raises(HipBackendError) as e:
        ops.weight_gather_qparams(W, None, None, -1, True, 4, out=out, scale=sc, zp=zp)
    assert e.value.status == QT_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((sc == SENTINEL).all()) and bool((zp == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- qt_pack_int4
PACK_ROWS = (1, 3, 4, 5, 64, 252, 256, 260, 516)


@pytest.mark.parametrize("K", [8, 20, 36, 256, 264, 2056])
def test_pack_int4_equals_the_oracle_on_both_kernels(ops, dev, oracle, K):
    """``oracle.pack_int4`` exactly, with and without ``col_src``, whole columns of -8 and of 7 among the levels.  For
    R % 4 == 0 the aligned call runs the four-rows-per-lane kernel; the same levels from a Qt that starts one byte into
    its buffer run the generic kernel and must give the same words.  K = 20 and 36 end in a partial word whose unused
    high nibbles are 0; K = 2056 is 257 words, one into a second column block."""
    Kw = (K + 7) // 8
    for R in PACK_ROWS:
        rng = _rng(8, R, K)
        Q = rng.integers(-8, 8, size=(R, K)).astype(np.int8)            # levels in ORIGINAL column order
        Q[:, 0], Q[:, K - 1] = -8, 7
        want = oracle.pack_int4(Q)
        assert want.shape == (R, Kw)
        for col_src in (rng.permutation(K).astype(np.int32), None):
            # sweep-position-major storage: position col_src[c] holds original column c
            Qpos = np.empty((K, R), np.int8)
            Qpos[col_src if col_src is not None else np.arange(K)] = Q.T
            Qt = torch.from_numpy(Qpos).to(dev)
            assert Qt.data_ptr() % 4 == 0
            packed = ops.pack_int4(Qt, _dev(col_src, dev))
            got = _host(packed)
            assert np.array_equal(got, want), (R, col_src is None)
            if K % 8:                                                    # a partial last word is in play
                assert np.all(got[:, -1].view(np.uint32) >> np.uint32(4 * (K % 8)) == 0)
            if R % 4 == 0:
                buf = torch.zeros(K * R + 1, dtype=torch.int8, device=dev)
                buf[1:] = Qt.reshape(-1)
                Qoff = buf[1:].view(K, R)
                assert Qoff.data_ptr() % 4 != 0 and Qoff.is_contiguous()
                assert torch.equal(ops.pack_int4(Qoff, _dev(col_src, dev)), packed), (R, col_src is None)


# --------------------------------------------------------------------------------------------------- qt_dequantize
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_dequantize_equals_fp32_numpy_rounded_once(ops, dev, out_dtype):
    """(q - z) * s in fp32, rounded once to the output dtype (checkpoints are written in bf16 / fp16): exact.  Levels
    over the 4-bit and the full int8 range (W8 schemes go down to -128), zero points including -128 and 127, G = 1, 3
    and K, ``g_of_col`` permuted as under activation ordering, with and without ``col_src``."""
    sizes = (1, 63, 64, 65, 130)
    for R in sizes:
        for K in sizes:
            for G in sorted({1, min(3, K), K}):
                for lo, hi in ((-8, 8), (-128, 128)):
                    rng = _rng(9, R, K, G, hi)
                    Q = rng.integers(lo, hi, size=(R, K)).astype(np.int8)
                    Q[0, 0], Q[R - 1, K - 1] = lo, hi - 1
                    scale = ((0.05 + rng.random((R, G))) / hi).astype(f32)
                    zp = rng.integers(lo, hi, size=(R, G)).astype(f32)
                    zp[0, 0], zp[R - 1, G - 1] = (-128, 127) if hi == 128 else (lo, hi - 1)
                    g_of_col = rng.permutation((np.arange(K) * G // K).astype(np.int32))
                    want = _round_to((Q.astype(f32) - zp[:, g_of_col]) * scale[:, g_of_col], out_dtype)
                    assert np.all(np.isfinite(want))
                    for col_src in (rng.permutation(K).astype(np.int32), None):
                        Qpos = np.empty((K, R), np.int8)
                        Qpos[col_src if col_src is not None else np.arange(K)] = Q.T
                        got = ops.dequantize(_dev(Qpos, dev), _dev(scale, dev), _dev(zp, dev), _dev(g_of_col, dev),
                                             _dev(col_src, dev), out_dtype)
                        assert got.dtype == out_dtype
                        assert np.array_equal(_host(got), want), (R, K, G, hi, col_src is None)


# ----------------------------------------------------------------------------------------- qt_act_stats_accumulate
def _stats_plan(n, K):
    """csrc/stats.hip's chunk plan: (strips, chunks, tokens per chunk)."""
    strips = (K + 2047) // 2048
    want = max(1, min(max(1, 2048 // strips), (n + 15) // 16))
    per = (n + want - 1) // want
    return strips, (n + per - 1) // per, per


def _acts(n, K, dtype, *key):
    """16-bit activations with outlier channels, channel 0 all zero and channel 1 all negative; returns (cpu tensor,
    fp32 values)."""
    rng = _rng(*key)
    x = rng.standard_normal((n, K)).astype(f32)
    x[:, 2::37] *= 10
    x[:, 0] = 0
    x[:, 1] = -np.abs(x[:, 1]) - f32(0.25)
    t = torch.from_numpy(x).to(dtype)
    return t, t.float().numpy()


@pytest.mark.parametrize("K", [8, 264, 2048, 2056, 4104])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 100, 1000, 4099])
def test_act_stats_running_min_max_and_abs_sum(ops, dev, n, K):
    """bf16 and fp16, X contiguous and at pitch K + 8 (sentinel in the pad), two calls on different data, each of: all
    three outputs, ``abs_sum`` alone, ``cmin`` / ``cmax`` alone.

    Min / max have no rounding: exact against numpy, and from +-inf the second call leaves the elementwise min / max of
    both batches (the running statistics SmoothQuant keeps).

    ``abs_sum`` against fp64 sum |x| per channel within (n + 3) 2^-24 of it: every term is an exact widening, and the
    result is a chain of non-negative fp32 additions.  A partial sum starts at 0 (the first addition is exact), so a
    chunk of L tokens costs L - 1 roundings, the ordered sum of C chunk sums C - 1 and the final ``+=`` one: L + C - 1
    with C = ceil(n / L), at most n for every 1 <= L <= n.  The second call adds n2 + 1 more.  The chunk plan depends on
    (n, K) only, so the strided and contiguous runs, every output combination and a repeated run agree to the bit."""
    strips, chunks, per = _stats_plan(n, K)
    if n in (17, 100, 1000, 4099):
        assert chunks > 1 and n % per != 0                               # a short last chunk is in play
    if K == 2056:
        assert strips == 2 and (K - 2048) // 8 == 1                      # one live lane in the second strip
    for dtype in (torch.bfloat16, torch.float16):
        (t1, v1), (t2, v2) = _acts(n, K, dtype, 10, n, K, 1), _acts(n, K, dtype, 10, n, K, 2)
        a1, a2 = np.abs(v1.astype(np.float64)).sum(axis=0), np.abs(v2.astype(np.float64)).sum(axis=0)
        mn1, mx1 = v1.min(axis=0), v1.max(axis=0)
        mn12, mx12 = np.minimum(mn1, v2.min(axis=0)), np.maximum(mx1, v2.max(axis=0))
        assert not np.array_equal(mn12, mn1) and not np.array_equal(mx12, mx1)    # the running min / max moves
        assert mn12[0] == 0 and mx12[0] == 0 and mx12[1] < 0 and a1[0] == 0
        first = []
        for layout in ("contiguous", "strided", "contiguous"):
            Xs = []
            for t in (t1, t2):
                if layout == "strided":
                    wide = torch.full((n, K + 8), 3.0e4, dtype=dtype)
                    wide[:, :K] = t
                    Xs.append(wide.to(dev)[:, :K])
                else:
                    Xs.append(t.to(dev))
            for with_sum, with_minmax in ((True, True), (True, False), (False, True)):
                s = torch.zeros(K, dtype=torch.float32, device=dev) if with_sum else None
                mn = torch.full((K,), float("inf"), dtype=torch.float32, device=dev) if with_minmax else None
                mx = torch.full((K,), float("-inf"), dtype=torch.float32, device=dev) if with_minmax else None
                tag = (dtype, layout, with_sum, with_minmax)
                ops.act_stats_accumulate(Xs[0], s, mn, mx)
                if with_minmax:
                    assert np.array_equal(_host(mn), mn1) and np.array_equal(_host(mx), mx1), tag
                if with_sum:
                    one = _host(s)
                    first.append(one)
                    err = np.abs(one.astype(np.float64) - a1)
                    print(f"n={n} K={K} {tag}: abs_sum err / (2^-24 ref) max {np.max(err / (EPS * a1 + 1e-300)):.2f}"
                          f" (bound {n + 3})")
                    assert np.all(err <= (n + 3) * EPS * a1), tag
                    assert one[0] == 0
                ops.act_stats_accumulate(Xs[1], s, mn, mx)
                if with_minmax:
                    assert np.array_equal(_host(mn), mn12) and np.array_equal(_host(mx), mx12), tag
                if with_sum:
                    two = _host(s)
                    assert np.all(np.abs(two.astype(np.float64) - (a1 + a2)) <= (2 * n + 4) * EPS * (a1 + a2)), tag
                    assert two[0] == 0
        assert len(first) == 6 and all(np.array_equal(first[0], f) for f in first[1:])


@pytest.mark.parametrize("pitch_extra", [16, 12])
def test_act_stats_and_gram_take_a_view_the_entry_point_rejects(ops, dev, pitch_extra):
    """X = wide[:, 4:4 + K] starts 8 bytes off a 16-byte boundary (and at ``pitch_extra`` = 12 its pitch is no multiple
    of 8): the C entry points refuse such rows, so the wrappers copy them to a contiguous tensor first, as
    ``xtx_accumulate_f32`` does -- the numbers are those of the contiguous copy, which are checked against numpy here."""
    n, K = 100, 264
    t, v = _acts(n, K, torch.bfloat16, 11, pitch_extra)
    wide = torch.full((n, K + pitch_extra), 3.0e4, dtype=torch.bfloat16)
    wide[:, 4:4 + K] = t
    X = wide.to(dev)[:, 4:4 + K]
    assert X.data_ptr() % 16 != 0 and X.stride(0) == K + pitch_extra
    outs = []
    for x in (X, t.to(dev)):
        s = torch.zeros(K, dtype=torch.float32, device=dev)
        mn = torch.full((K,), float("inf"), dtype=torch.float32, device=dev)
        mx = torch.full((K,), float("-inf"), dtype=torch.float32, device=dev)
        ops.act_stats_accumulate(x, s, mn, mx)
        G = torch.zeros((K, K), dtype=torch.float32, device=dev)
        ops.xtx_accumulate(x, G)
        outs.append((s, mn, mx, G))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    s, mn, mx, G = outs[0]
    assert np.array_equal(_host(mn), v.min(axis=0)) and np.array_equal(_host(mx), v.max(axis=0))
    ref = np.abs(v.astype(np.float64)).sum(axis=0)
    assert np.all(np.abs(_host(s) - ref) <= (n + 3) * EPS * ref)
    Gt = v.astype(np.float64).T @ v.astype(np.float64)
    d = np.sqrt(np.diag(Gt))
    # the bound tests/util.py's oracle_group holds the Gram sum to
    assert np.all(np.abs(np.tril(_host(G)) - np.tril(Gt)) <= 1e-5 * np.tril(np.outer(d, d)) + 1e-30)


# ------------------------------------------------------------------- qt_hessian_prepare / qt_hessian_diag (one pass)
A_SENTINEL = -777.0


def _prepare_and_check(ops, dev, oracle, g_lower, n_samples, percdamp, perm):
    """``g_lower``: fp32 [K, K], lower triangle valid.  The device sees NaN in the strict upper triangle."""
    K = g_lower.shape[0]
    Gl = np.tril(g_lower).astype(f32)
    Gfull = Gl + np.tril(Gl, -1).T
    Gdev = torch.from_numpy(Gl + np.triu(np.full((K, K), np.nan, f32), 1)).to(dev)
    A_out = torch.full((K, K), A_SENTINEL, dtype=torch.float32, device=dev)
    A, dead, diag = ops.hessian_prepare(Gdev, n_samples, percdamp, _dev(perm, dev), A_out=A_out)
    assert A.data_ptr() == A_out.data_ptr()
    H = Gfull * f32(2.0 / n_samples)                                     # one fp32 multiply per element, as the kernel
    assert H.dtype == f32
    assert np.array_equal(_host(diag), np.diag(H))
    assert torch.equal(ops.hessian_diag(Gdev, n_samples), diag)          # bit for bit
    Hp = H[perm][:, perm] if perm is not None else H
    Hd, odead, damp = oracle.hessian_dead_and_damp(Hp, percdamp)
    assert np.array_equal(_host(dead).astype(bool), odead)
    want, got = Hd[::-1, ::-1], _host(A)
    iu = np.triu_indices(K, 1)
    assert np.array_equal(got[iu], want[iu])                             # off-diagonal: exact
    # diagonal: + damp, whose mean is an fp64 sum in a different order -> 1 ulp
    np.testing.assert_allclose(np.diag(got), np.diag(want), rtol=2.4e-7, atol=0)
    il = np.tril_indices(K, -1)
    assert np.all(got[il] == A_SENTINEL)                                 # the strict lower triangle is the caller's
    return odead, damp, got


@pytest.mark.parametrize("K", [8, 200, 1000, 1024, 1032, 1536])
def test_hessian_prepare_one_pass_against_the_oracle(ops, dev, oracle, K):
    """Below the two-pass threshold, at and around the 1024-thread reduction width of the diagonal statistics:
    n_samples 1, 3 and 7 (2 / n inexact for 3 and 7), percdamp 0.01 and 0, with and without ``perm``, dead columns at 0,
    K - 1 and one on each half of the sweep order.  Reference: ``oracle.hessian_dead_and_damp`` on Gfull * fp32(2 / n)."""
    rng = _rng(12, K)
    perm = rng.permutation(K).astype(np.int32)
    X = rng.standard_normal((64, K)).astype(f32)
    X[:, 2::37] *= 10
    dead_cols = sorted({0, K - 1, int(perm[K // 4]), int(perm[3 * K // 4])})
    X[:, dead_cols] = 0
    g = X.T @ X
    for n_samples in (1, 3, 7):
        if n_samples > 1:
            assert float(f32(2.0 / n_samples)) != 2.0 / n_samples
        for percdamp in (0.01, 0.0):
            for pm in (perm, None):
                odead, damp, _ = _prepare_and_check(ops, dev, oracle, g, n_samples, percdamp, pm)
                where = np.flatnonzero(odead)
                if pm is None:
                    assert where.tolist() == dead_cols
                else:                                                    # sweep positions, one on each half among them
                    assert K // 4 in where and 3 * K // 4 in where and sorted(int(perm[i]) for i in where) == dead_cols
                assert (damp == 0) == (percdamp == 0)


@pytest.mark.parametrize("K", [8, 1000, 1032])
def test_hessian_prepare_all_dead_and_single_live_column(ops, dev, oracle, K):
    """No calibration signal at all: every column dead, the mean of the repaired diagonal is 1, damp = percdamp and
    A = (1 + damp) I.  One live column: the mean is (K - 1 + h) / K."""
    perm = _rng(13, K).permutation(K).astype(np.int32)
    for pm in (perm, None):
        odead, damp, got = _prepare_and_check(ops, dev, oracle, np.zeros((K, K), f32), 3, 0.01, pm)
        assert odead.all() and damp == f32(0.01)
        assert np.array_equal(np.triu(got), np.diag(np.full(K, f32(1) + f32(0.01), f32)))
        g = np.zeros((K, K), f32)
        live = K // 3
        g[live, live] = 12.5
        odead, damp, got = _prepare_and_check(ops, dev, oracle, g, 3, 0.01, pm)
        assert odead.sum() == K - 1
        assert not odead[live if pm is None else int(np.flatnonzero(perm == live)[0])]
