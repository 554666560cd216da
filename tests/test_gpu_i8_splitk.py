"""qt_splitk_gemm_i8: the ring's 256 x 256 tile over S k-ranges plus an int32 reduce pass, for W8A8 / INT8 Linears at
129-2047 rows.

Its contract is bit equality with the tiled qt_gemm_i8 on the same arguments, so every comparison here is on bit
patterns, and -- because that alone would pass two kernels wrong in the same way -- the same cases also go against the
fp64 reference of tests/ckpt_reference.py within the project's own bound for this sequence (``gemm_i8_tolerance``), as
in test_gpu_i8_ring.py, whose ``_case`` (one weight, both quantisations, their fp64 references, computed once per
shape) is reused.  Shapes are in K-tiles of U = ``ops.SPLITK_I8_K_UNIT`` k-bytes."""
import pytest
import torch

from tests import ckpt_reference as cr
from tests.test_gpu_i8_ring import _case, _Counter
from tests.test_gpu_i8_skinny import _bias, _same_bits, _sentinel, _untouched

pytestmark = pytest.mark.gpu


def _check(ops, c, asym, dt, bias, splits, what):
    Xq, s_x, zp_x, y64, mag = c[asym]
    kw = dict(zp_x=zp_x, wsum=c["wsum"] if asym else None, bias=bias, out_dtype=dt)
    want = ops.gemm_i8(Xq, s_x, c["Wq"], c["s_w"], **kw)
    got = ops.splitk_gemm_i8(Xq, s_x, c["Wq"], c["s_w"], splits=splits, **kw)
    torch.cuda.synchronize()
    _same_bits(got, want, what)
    if bias is not None:
        b = bias.cpu().double()
        y64, mag = y64 + b, mag + b.abs()
    cr.assert_within(got, y64, cr.gemm_i8_tolerance(got.cpu(), mag, 1), f"{what} vs fp64")


# ---- 1: split geometry ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_tiles", [2, 3, 7, 8, 13, 17])
def test_split_geometry(ops, dev, k_tiles):
    """2 x 2 ragged tiles over S = 2, 3 and one split per K-tile: splits of one K-tile (four units, below the lead of
    six), uneven splits (7 = 3 + 2 + 2, 17 = 6 + 6 + 5), splits of an odd number of K-tiles (a trailing half trip round
    the ring), and k-ranges that start in either half of the ring."""
    U = ops.SPLITK_I8_K_UNIT
    M, N, K = 257, 264, k_tiles * U
    c = _case(ops, dev, M, N, K, seed=K)
    for S in sorted(s for s in {2, 3, k_tiles} if s <= k_tiles):
        sizes = [t1 - t0 for t0, t1 in ops.splitk_ranges(K, S)]
        assert sum(sizes) == k_tiles and max(sizes) - min(sizes) <= 1 and min(sizes) >= 1
        for asym in (False, True):
            for dt in (torch.bfloat16, torch.float16):
                for with_bias in (False, True):
                    bias = _bias(N, dt, dev, seed=N) if with_bias else None
                    _check(ops, c, asym, dt, bias, S, f"K={K} S={S} asym={asym} {dt} bias={with_bias}")


# ---- 2: tile edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(129, 256), (255, 257), (300, 24), (513, 1), (1100, 520)])
def test_tile_edges(ops, dev, M, N):
    """One short of a tile and one over in either direction, a sliver of columns, one column (the reduce pass's
    element-wise last quad), and 5 x 3 tiles x 2 splits."""
    K = 1024
    c = _case(ops, dev, M, N, K, seed=M + N)
    _check(ops, c, True, torch.bfloat16, _bias(N, torch.bfloat16, dev, seed=M), 2, f"M={M} N={N}")
    _check(ops, c, False, torch.float16, None, 2, f"M={M} N={N} sym")


# ---- 3: the slabs are added as integers -----------------------------------------------------------------------------
@pytest.mark.parametrize("level", [127, -128])
def test_partials_are_summed_in_int32(ops, dev, level):
    """K = 2048, S = 4, every level 127 (or -128): acc = 2048 * 127^2 = 33 032 192 > 2^24, every partial 8 258 048 >
    2^22, so neither fits a 24-bit multiply-add or a partial narrowed below int32.  With s_w = 2^-12 and s_x = 2^-13 the
    epilogue's two products are exact and y = fp32(acc) * 2^-25: the expected bits follow from the exact integer alone,
    also for the asymmetric difference acc - zp * wsum, which must be taken on the complete sum."""
    M, N, K, S = 130, 40, 2048, 4
    acc = K * level * level
    assert acc > 2 ** 24 and acc // S > 2 ** 22
    Xq = torch.full((M, K), level, dtype=torch.int8, device=dev)
    Wq = torch.full((N, K), level, dtype=torch.int8, device=dev)
    s_x = torch.full((M,), 2.0 ** -13, device=dev)
    s_w = torch.full((N, 1), 2.0 ** -12, device=dev)
    got = ops.splitk_gemm_i8(Xq, s_x, Wq, s_w, out_dtype=torch.float16, splits=S)
    want = ops.gemm_i8(Xq, s_x, Wq, s_w, out_dtype=torch.float16)
    torch.cuda.synchronize()
    _same_bits(got, want, f"level {level}")
    exact = torch.tensor(float(acc), dtype=torch.float32) * 2.0 ** -25      # one rounding of the int, exact scaling
    _same_bits(got.cpu(), exact.to(torch.float16).expand(M, N).contiguous(), f"level {level} vs the exact integer")
    # asymmetric: the int32 difference acc - zp * wsum is taken on the complete sum
    zp = torch.full((M,), 3, dtype=torch.int32, device=dev)
    wsum = torch.full((N, 1), K * level, dtype=torch.int32, device=dev)
    got = ops.splitk_gemm_i8(Xq, s_x, Wq, s_w, zp_x=zp, wsum=wsum, out_dtype=torch.float16, splits=S)
    want = ops.gemm_i8(Xq, s_x, Wq, s_w, zp_x=zp, wsum=wsum, out_dtype=torch.float16)
    torch.cuda.synchronize()
    _same_bits(got, want, f"level {level} asym")
    exact = torch.tensor(float(acc - 3 * K * level), dtype=torch.float32) * 2.0 ** -25
    _same_bits(got.cpu(), exact.to(torch.float16).expand(M, N).contiguous(), f"level {level} asym vs the exact integer")


def _row_with_sum(n, total):
    """n int8 levels that add up to ``total``: all 127, the first few lowered."""
    row = torch.full((n,), 127, dtype=torch.int64)
    short = 127 * n - total
    assert 0 <= short <= 255 * n
    row[: short // 255] = -128
    row[short // 255] -= short % 255
    assert int(row.sum()) == total and row.min() >= -128
    return row.to(torch.int8)


def test_an_fp32_partial_would_change_the_bits(ops, dev):
    """The all-127 case above has partials that fp32 holds exactly, so it cannot tell a reduce that converts each slab
    before adding.  This one can.  K = 2304, S = 2, W all 127, every row of Xq with level sums s0, s1 over the two
    k-ranges such that both partials 127 s0, 127 s1 are above 2^24 and = 3 (mod 4) -- each rounds UP to fp32 -- and
    acc = 127 (s0 + s1) = m 2^15 + 2^14 + 2 above 2^25 with m even: the exact int32 rounds once to m 2^15 + 2^14, a
    tie of the fp16 grid at y = acc 2^-25 that goes down to even, while the sum of two rounded partials is acc + 2,
    just above the tie, and goes up.  The test first shows that with fp32 arithmetic on the host."""
    import numpy as np

    M, N, K, S = 130, 40, 2304, 2
    half = K // S
    t = next(t for t in range(2 * half * 127, 0, -2) if (127 * t) % 65536 == 16386)
    s0 = t // 2 - (t // 2 - 1) % 4
    s1 = t - s0
    p0, p1, acc = 127 * s0, 127 * s1, 127 * t
    assert acc > 2 ** 25 and min(p0, p1) > 2 ** 24 and p0 % 4 == p1 % 4 == 3 and (acc >> 15) % 2 == 0
    scale = np.float32(2.0 ** -25)
    exact = np.float16(np.float32(acc) * scale)
    through_fp32 = np.float16((np.float32(p0) + np.float32(p1)) * scale)
    assert exact != through_fp32                                        # the inputs tell the two reduces apart
    assert ops.splitk_ranges(K, S) == [(0, half // 128), (half // 128, K // 128)]
    row = torch.cat([_row_with_sum(half, s0), _row_with_sum(half, s1)])
    Xq = row.expand(M, K).contiguous().to(dev)
    Wq = torch.full((N, K), 127, dtype=torch.int8, device=dev)
    s_x = torch.full((M,), 2.0 ** -13, device=dev)
    s_w = torch.full((N, 1), 2.0 ** -12, device=dev)
    got = ops.splitk_gemm_i8(Xq, s_x, Wq, s_w, out_dtype=torch.float16, splits=S)
    want = ops.gemm_i8(Xq, s_x, Wq, s_w, out_dtype=torch.float16)
    torch.cuda.synchronize()
    _same_bits(got, want, "odd partials above 2^24")
    assert got.unique().tolist() == [float(exact)]


# ---- 4 + 5: raw C ABI calls: the workspace, Y, refusals -------------------------------------------------------------
def _raw(ops, Xq_ptr, M, K, Wq_ptr, fmt, N, s_x, zp_x, s_w, G, wsum, bias, Y, ldy, splits, ws_ptr, ws_size):
    from quantool_amd.hip import _lib

    _lib.check("qt_splitk_gemm_i8", _lib.load().qt_splitk_gemm_i8(
        Xq_ptr, M, K, Wq_ptr, fmt, N, s_x.data_ptr(), ops._ptr(zp_x), s_w.data_ptr(), G, ops._ptr(wsum),
        ops._ptr(bias), Y.data_ptr(), ops._dtype_code(Y), ldy, splits, ws_ptr, ws_size, ops._stream()))


GUARD = 4096


def test_workspace_needs_no_zeroes_and_is_not_overrun(ops, dev):
    """Two poison bytes in the whole workspace before the call give the same Y (nothing relies on zeroes, no padded
    element reaches Y: M = 300, N = 264 pad to 512 x 512), the guard behind the plan's size keeps its bytes, and a
    workspace one byte short is refused with the needed size named and Y untouched."""
    from quantool_amd.hip import _lib
    from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

    M, N, K, S = 300, 264, 1024, 3
    c = _case(ops, dev, M, N, K, seed=11)
    Xq, s_x, zp_x, _, _ = c[True]
    bias = _bias(N, torch.bfloat16, dev, seed=12)
    want = ops.gemm_i8(Xq, s_x, c["Wq"], c["s_w"], zp_x=zp_x, wsum=c["wsum"], bias=bias, out_dtype=torch.bfloat16)
    S_plan, size = ops.splitk_gemm_i8_plan(M, N, K, cus=256, splits=S)
    assert S_plan == S and size == S * 512 * 512 * 4
    args = (Xq.data_ptr(), M, K, c["Wq"].data_ptr(), _lib.QT_W_INT8, N, s_x, zp_x, c["s_w"], 1, c["wsum"], bias)
    for poison in (0x7F, 0xA5):
        buf = torch.full((size + GUARD,), poison, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 16 == 0
        Y = _sentinel((M, N), torch.bfloat16, dev)
        _raw(ops, *args, Y, N, S, buf.data_ptr(), size)
        torch.cuda.synchronize()
        _same_bits(Y, want, f"poison {poison:#x}")
        assert bool((buf[size:] == poison).all()), "the guard behind the workspace was written"
    Y = _sentinel((M, N), torch.bfloat16, dev)
    with pytest.raises(HipBackendError) as e:
        _raw(ops, *args, Y, N, S, buf.data_ptr(), size - 1)
    assert e.value.status == QT_ERR_INVALID and str(size) in str(e.value) and "workspace_size" in str(e.value)
    torch.cuda.synchronize()
    assert _untouched(Y)


def test_caller_owned_y_keeps_its_padding(ops, dev):
    from quantool_amd.hip import _lib

    M, N, K, S = 257, 200, 1152, 2
    ldy = N + 17
    c = _case(ops, dev, M, N, K, seed=4)
    Xq, s_x, zp_x, _, _ = c[True]
    bias = _bias(N, torch.bfloat16, dev, seed=5)
    want = ops.gemm_i8(Xq, s_x, c["Wq"], c["s_w"], zp_x=zp_x, wsum=c["wsum"], bias=bias, out_dtype=torch.bfloat16)
    _, size = ops.splitk_gemm_i8_plan(M, N, K, cus=256, splits=S)
    ws = torch.empty(size, dtype=torch.uint8, device=dev)
    Y = _sentinel((M + 3, ldy), torch.bfloat16, dev)
    _raw(ops, Xq.data_ptr(), M, K, c["Wq"].data_ptr(), _lib.QT_W_INT8, N, s_x, zp_x, c["s_w"], 1, c["wsum"], bias, Y, ldy,
         S, ws.data_ptr(), size)
    torch.cuda.synchronize()
    assert _untouched(Y[:, N:]) and _untouched(Y[M:]) and not _untouched(Y[:M, :N])
    _same_bits(Y[:M, :N].contiguous(), want, "ldy > N")


def test_refusals_write_nothing_and_name_the_reason(ops, dev):
    from quantool_amd.hip import _lib
    from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

    M, N, K = 130, 32, 4 * 128
    xbuf = torch.ones(M * K + 32, dtype=torch.int8, device=dev)
    wbuf = torch.zeros(N * K + 32, dtype=torch.int8, device=dev)
    s_x = torch.ones(M, device=dev)
    s_w = torch.ones(N, K // 128, device=dev)
    _, size = ops.splitk_gemm_i8_plan(M, N, K, cus=256, splits=4)
    ws = torch.full((size,), 0x5A, dtype=torch.uint8, device=dev)
    Y = _sentinel((M, N), torch.bfloat16, dev)
    X, W, P = xbuf.data_ptr(), wbuf.data_ptr(), ws.data_ptr()
    i8, i4 = _lib.QT_W_INT8, _lib.QT_W_INT4_PACKED
    cases = {
        "S = 1": ((X, M, K, W, i8, N, s_x, None, s_w, 1), (1, P, size), "splits 1 is qt_gemm_i8_ring"),
        "S > K/128": ((X, M, K, W, i8, N, s_x, None, s_w, 1), (5, P, 2 * size), "splits 5 > K / 128 = 4"),
        "null workspace": ((X, M, K, W, i8, N, s_x, None, s_w, 1), (2, None, size), "workspace is null"),
        "int4 format": ((X, M, K, W, i4, N, s_x, None, s_w, 1), (2, P, size), "int8 weights only"),
        "G > 1": ((X, M, K, W, i8, N, s_x, None, s_w, K // 128), (2, P, size), "one scale group"),
        "K % U != 0": ((X, M, K + 16, W, i8, N, s_x, None, s_w, 1), (2, P, size), "not a multiple of the k-unit"),
        "Xq misaligned": ((X + 1, M, K, W, i8, N, s_x, None, s_w, 1), (2, P, size), "Xq is not 16-byte aligned"),
        "workspace misaligned": ((X, M, K, W, i8, N, s_x, None, s_w, 1), (2, P + 4, size - 4),
                                 "workspace is not 16-byte aligned"),
    }
    for what, (args, tail, reason) in cases.items():
        with pytest.raises(HipBackendError) as e:
            _raw(ops, *args, None, None, Y, N, *tail)
        assert e.value.status == QT_ERR_INVALID, what
        assert reason in str(e.value), (what, str(e.value))
    torch.cuda.synchronize()
    assert _untouched(Y) and bool((ws == 0x5A).all())


def test_wrapper_takes_the_plans_split_and_the_ring_at_one(ops, dev, monkeypatch):
    """``splits`` = 0 is the plan's S for this device; a plan of S = 1 (more tiles than compute units) is the ring."""
    M, N, K = 300, 264, 1024
    c = _case(ops, dev, M, N, K, seed=21)
    S, _ = ops.splitk_gemm_i8_plan(M, N, K)
    assert S == 2 == K // ops.SPLITK_I8_K_UNIT // ops.SPLITK_I8_MIN_K_TILES
    _check(ops, c, True, torch.bfloat16, None, 0, "the plan's S")
    ring = _Counter(monkeypatch, ops, "gemm_i8_ring")
    _check(ops, c, False, torch.bfloat16, None, 1, "S = 1")
    assert ring.n == 1
    with pytest.raises(ValueError, match="splits 9 > K / 128 = 8"):
        ops.splitk_gemm_i8(c[False][0], c[False][1], c["Wq"], c["s_w"], splits=9)


# ---- 6: the module --------------------------------------------------------------------------------------------------
def test_module_is_the_same_with_and_without_the_split(ops, dev, monkeypatch):
    from quantool_amd.engine.qmodules import QuantizedLinear

    M, N, K = 300, 264, 1024
    g = torch.Generator().manual_seed(31)
    w = torch.randint(-128, 128, (N, K), generator=g, dtype=torch.int8)
    lin = QuantizedLinear(K, N, w, torch.rand(N, 1, generator=g) * 0.01 + 0.001, act_symmetric=False,
                          bias=_bias(N, torch.bfloat16, "cpu", seed=32)).to(dev)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    split = _Counter(monkeypatch, ops, "splitk_gemm_i8")
    tiled = _Counter(monkeypatch, ops, "gemm_i8")
    monkeypatch.setattr(QuantizedLinear, "splitk_min_m", 0)
    with torch.no_grad():
        off = lin(x)
    assert (split.n, tiled.n) == (0, 1)
    monkeypatch.setattr(QuantizedLinear, "splitk_min_m", 129)
    monkeypatch.setattr(QuantizedLinear, "splitk_min_k", 1024)
    with torch.no_grad():
        on = lin(x)
    torch.cuda.synchronize()
    assert (split.n, tiled.n) == (1, 1)
    assert torch.isfinite(on.float()).all() and on.abs().max() > 0
    assert torch.equal(on, off)
