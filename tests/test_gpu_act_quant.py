"""``qt_act_mul_quantize_i8`` on the device, against what it replaces: torch's SiLU kernel, torch's multiply and
``qt_quantize_tokens_i8``.

The activation is pinned over every 16-bit pattern of both dtypes (``H`` from the kernel equals ``F.silu(gate) * up`` to
the bit); the quantiser is pinned against ``quantize_tokens_i8`` on that ``H`` and on torch's product, at shapes that
take the 16-byte path, the element path, every tail, several strides of the workgroup and the largest row; and nothing
outside the four outputs is written."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
FLT_EPSILON = 2.0 ** -23


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_where_not_nan(got, want, what):
    """Equal to the bit, infinities included; NaNs (inf * 0, silu(-inf)) at the same places."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), f"{what}: NaN positions differ"
    diff = (_bits(got) != _bits(want)) & ~wn
    n = int(diff.sum())
    if n:
        i = diff.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n} elements differ, first at {i}: {got[tuple(i)].item()} != "
                             f"{want[tuple(i)].item()}")


def _perm(K, dev, seed=5):
    return torch.randperm(K, generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(dev)


def _triple_equal(got, want, what, rows=None):
    for name, a, b in zip(("Xq", "s_x", "zp_x"), got, want):
        assert (a is None) == (b is None), f"{what}: {name}"
        if a is None:
            continue
        if rows is not None:
            a, b = a[rows], b[rows]
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a, b), f"{what}: {name} differs in {int((a != b).sum())} places"


# ---- the activation, exhaustively -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def patterns(dev):
    """dtype -> gate [32, 2048]: all 65536 bit patterns, NaNs replaced by 0."""
    out = {}
    for dt in DTYPES:
        g = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt).to(dev)
        out[dt] = torch.where(torch.isnan(g), torch.zeros_like(g), g).reshape(32, 2048).contiguous()
    return out


@pytest.mark.parametrize("up_kind", ["ones", "normal"])
@pytest.mark.parametrize("dt", DTYPES)
def test_every_pattern_equals_torch(ops, dev, patterns, dt, up_kind):
    gate = patterns[dt]
    assert int(torch.isinf(gate).sum()) == 2 and not bool(torch.isnan(gate).any())
    assert len(torch.unique(gate.view(torch.int16))) == 65536 - (2 ** 8 - 2 if dt == torch.bfloat16 else 2 ** 11 - 2)
    if up_kind == "ones":
        up = torch.ones_like(gate)
    else:
        up = torch.randn(gate.shape, generator=torch.Generator().manual_seed(7)).to(dt).to(dev)
    want = F.silu(gate) * up
    perm = _perm(gate.shape[1], dev)
    finite_rows = torch.isfinite(want).all(dim=1)
    assert int(finite_rows.sum()) >= 24                     # the quantiser comparison below is not vacuous
    for symmetric in (True, False):
        for col_perm in (None, perm):
            Xq, s_x, zp_x, H = ops.act_mul_quantize_i8(gate, up, symmetric=symmetric, col_perm=col_perm, return_h=True)
            torch.cuda.synchronize()
            _same_where_not_nan(H, want, f"{dt} up={up_kind}")
            ref = ops.quantize_tokens_i8(H, symmetric=symmetric, col_perm=col_perm)
            _triple_equal((Xq, s_x, zp_x), ref, f"{dt} up={up_kind} sym={symmetric} perm={col_perm is not None}",
                          rows=finite_rows)


# ---- shapes and layouts ---------------------------------------------------------------------------------------------
SHAPES = [(1, 8), (3, 1000), (5, 1031), (17, 4096), (2, 14336), (1, 32768)]
LAYOUTS = ["separate", "halves", "pitch+3", "shifted"]


def _rows(M, K, dt, seed):
    """(gate, up) values [M, K] on the CPU: row 0 carries one x1000 outlier, the last row of M >= 2 is all zero."""
    g = torch.Generator().manual_seed(seed)
    gate, up = torch.randn(M, K, generator=g) * 2, torch.randn(M, K, generator=g)
    up[0, K // 3] = 1000.0
    gate[0, K // 3] = 3.0
    if M >= 2:
        gate[M - 1] = 0.0
    return gate.to(dt), up.to(dt)


def _layout(gate, up, layout, dev):
    """The same values as device views of the given layout (unit column stride throughout)."""
    M, K = gate.shape
    if layout == "separate":
        return gate.to(dev), up.to(dev)
    if layout == "halves":
        Y = torch.cat([gate, up], 1).to(dev)
        return Y[:, :K], Y[:, K:]
    if layout == "pitch+3":
        G = torch.zeros(M, K + 3, dtype=gate.dtype, device=dev)
        U = torch.zeros(M, K + 3, dtype=gate.dtype, device=dev)
        G[:, :K], U[:, :K] = gate.to(dev), up.to(dev)
        return G[:, :K], U[:, :K]
    if layout == "shifted":                                  # one element behind a 16-byte boundary, K as it is
        G = torch.zeros(M * K + 8, dtype=gate.dtype, device=dev)
        U = torch.zeros(M * K + 8, dtype=gate.dtype, device=dev)
        gv, uv = G[1:1 + M * K].view(M, K), U[1:1 + M * K].view(M, K)
        gv.copy_(gate)
        uv.copy_(up)
        return gv, uv
    raise KeyError(layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,K", SHAPES)
def test_shapes_and_layouts(ops, dev, M, K, layout):
    perm = _perm(K, dev, seed=K)
    for dt in DTYPES:
        gate, up = _layout(*_rows(M, K, dt, seed=M * 100003 + K), layout, dev)
        assert gate.stride(1) == 1 and up.stride(1) == 1
        if layout == "halves":
            assert up.data_ptr() == gate.data_ptr() + 2 * K and gate.stride(0) == 2 * K
            assert (up.data_ptr() % 16 != 0) == (K % 8 != 0)
        if layout == "shifted":
            assert gate.data_ptr() % 16 == 2
        prod = F.silu(gate) * up
        assert torch.isfinite(prod).all()
        for symmetric in (True, False):
            for col_perm in (None, perm):
                what = f"{M}x{K} {layout} {dt} sym={symmetric} perm={col_perm is not None}"
                want = ops.quantize_tokens_i8(prod, symmetric=symmetric, col_perm=col_perm)
                got = ops.act_mul_quantize_i8(gate, up, symmetric=symmetric, col_perm=col_perm, return_h=True)
                torch.cuda.synchronize()
                assert torch.equal(_bits(got[3]), _bits(prod)), what
                _triple_equal(got[:3], want, what)
                again = ops.act_mul_quantize_i8(gate, up, symmetric=symmetric, col_perm=col_perm)
                assert len(again) == 3
                _triple_equal(again, want, what + " (no H)")
                if M >= 2:
                    assert float(got[1][M - 1]) == FLT_EPSILON
                    assert bool((got[0][M - 1] == (0 if symmetric else -128)).all())
                    if not symmetric:
                        assert int(got[2][M - 1]) == -128
                # the outlier row: h = silu(3) * 1000 = 2858 takes the edge (s >= 2858 / 127.5, or / 255), every other
                # |h| < 45 lands within 2 (4) levels of the zero-point
                off = got[0][0].to(torch.int32) - (0 if symmetric else int(got[2][0]))
                assert int((off.abs() > (2 if symmetric else 4)).sum()) == 1 and int(off.abs().max()) >= 127, what


def test_a_rows_result_does_not_depend_on_the_grid(ops, dev):
    """Row m of a 40-row call is the one-row call on row m."""
    gate, up = _rows(40, 1000, torch.bfloat16, seed=9)
    gate, up = gate.to(dev), up.to(dev)
    Xq, s_x, zp_x = ops.act_mul_quantize_i8(gate, up, symmetric=False)
    for m in (0, 17, 39):
        one = ops.act_mul_quantize_i8(gate[m:m + 1], up[m:m + 1], symmetric=False)
        _triple_equal(one, (Xq[m:m + 1], s_x[m:m + 1], zp_x[m:m + 1]), f"row {m}")


def test_col_perm_is_clamped_into_the_row(ops, dev):
    """An index outside [0, K) reads the row's first or last element: never anything outside the row."""
    gate, up = (t.to(dev) for t in _rows(3, 100, torch.bfloat16, seed=4))
    perm = torch.arange(100, dtype=torch.int32)
    perm[5], perm[50], perm[99] = -7, 100000, 100
    got = ops.act_mul_quantize_i8(gate, up, symmetric=False, col_perm=perm.to(dev))
    want = ops.act_mul_quantize_i8(gate, up, symmetric=False, col_perm=perm.clamp(0, 99).to(dev))
    _triple_equal(got, want, "clamped col_perm")


# ---- nothing else is written ----------------------------------------------------------------------------------------
PAD = 64


@pytest.mark.parametrize("M,K", [(3, 1000), (5, 1031), (1, 32768)])
@pytest.mark.parametrize("symmetric", [True, False])
def test_only_the_outputs_are_written(ops, dev, M, K, symmetric):
    from quantool_amd.hip import _lib

    lib = _lib.load()
    dt = torch.bfloat16
    gate, up = (t.to(dev) for t in _rows(M, K, dt, seed=21))
    ldh = K + 5
    xq = torch.full((PAD + M * K + PAD,), 0x5A, dtype=torch.int8, device=dev)
    sx = torch.full((PAD + M + PAD,), -7.5, dtype=torch.float32, device=dev)
    zp = torch.full((PAD + M + PAD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    hb = torch.full((PAD + M * ldh + PAD,), 0x5A5A, dtype=torch.int16, device=dev)
    st = lib.qt_act_mul_quantize_i8(
        gate.data_ptr(), gate.stride(0), up.data_ptr(), up.stride(0), _lib.QT_BF16, M, K, 0, None, int(symmetric),
        xq.data_ptr() + PAD, sx.data_ptr() + 4 * PAD, zp.data_ptr() + 4 * PAD, hb.data_ptr() + 2 * PAD, ldh,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, lib.qt_last_error()
    for name, buf, n in (("Xq", xq, M * K), ("s_x", sx, M), ("zp_x", zp, M), ("H", hb, M * ldh)):
        poison = buf[0].item()
        assert bool((buf[:PAD] == poison).all()) and bool((buf[PAD + n:] == poison).all()), name
    h = hb[PAD:PAD + M * ldh].view(M, ldh)
    assert bool((h[:, K:] == 0x5A5A).all())                  # the pitch gap of H
    prod = F.silu(gate) * up
    assert torch.equal(h[:, :K], _bits(prod))
    want = ops.quantize_tokens_i8(prod, symmetric=symmetric)
    assert torch.equal(xq[PAD:PAD + M * K].view(M, K), want[0])
    assert torch.equal(sx[PAD:PAD + M], want[1])
    if symmetric:
        assert bool((zp == 0x5A5A5A5A).all())                # never written when symmetric
    else:
        assert torch.equal(zp[PAD:PAD + M], want[2])


def test_refusals_through_ops(ops, dev):
    g = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="agree"):
        ops.act_mul_quantize_i8(g, g.to(torch.float16))
    with pytest.raises(ValueError, match="agree"):
        ops.act_mul_quantize_i8(g, g[:, :32])
    with pytest.raises(ValueError, match="unit column stride"):
        ops.act_mul_quantize_i8(g[:, ::2], g[:, ::2])
    with pytest.raises(TypeError, match="bf16 or fp16"):
        ops.act_mul_quantize_i8(g.float(), g.float())
    with pytest.raises(ValueError, match="act must be"):
        ops.act_mul_quantize_i8(g, g, act="gelu")
    with pytest.raises(ValueError, match="col_perm"):
        ops.act_mul_quantize_i8(g, g, col_perm=torch.zeros(63, dtype=torch.int32, device=dev))
    big = torch.zeros(1, 32768 + 8, dtype=torch.bfloat16, device=dev)
    with pytest.raises(Exception, match="32768"):
        ops.act_mul_quantize_i8(big, big)
