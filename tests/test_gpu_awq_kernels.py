"""The a12 / a13 kernels (csrc/awq.hip) one by one against plain numpy: an fp32 restatement where include/quantool_amd.h
fixes the operation sequence (then the device result must EQUAL it), fp64 elsewhere.

The grid: group sizes 32, 40 (K = 200), 64, 128, 192, 512, 1024 and channel-wise; 1, 63, 64, 65, 100 and 300 rows; K a
multiple of 128 and not (K = 200, 264 and 1152 among them); bf16, fp16 and fp32 weights; W contiguous, a row-strided
view (ldw > K) and a view that starts one element into its buffer (not 16-byte aligned: the generic kernels).

"Equal" for floating outputs means equal as numbers (``np.array_equal`` on finite values): every rounding is pinned, the
sign of a zero is not (``fmaxf(-0.0f, 0.0f)`` may return either).
"""
import numpy as np
import pytest
import torch

from quantool_amd.hip._lib import QT_ERR_INVALID, HipBackendError

pytestmark = pytest.mark.gpu

f32 = np.float32
ROWS = (1, 63, 64, 65, 100, 300)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
# (group_size, K): every group size with a K that is a multiple of 128 and one that is not, where one exists
GROUPS = ((32, 1152), (32, 96), (40, 200), (64, 1152), (64, 192), (128, 1152), (128, 256), (192, 1152), (192, 576),
          (512, 1024), (512, 1536), (1024, 2048), (1024, 1024), (-1, 200), (-1, 264), (-1, 1152))
EPS = 2.0 ** -24            # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------------ helpers
def _weights(R, K, seed, std=0.05):
    """fp32 weights; row 0's first 32 columns are zero (an all-zero group at the smallest group size, a zero stretch in
    wider ones)."""
    w = (np.random.default_rng(seed).standard_normal((R, K)) * std).astype(f32)
    w[0, :32] = 0
    return w


def _layouts(w, dtype, dev):
    """(name, device view, fp32 values): the same values contiguous, row-strided (ldw = K + 24, the pad holds a
    sentinel) and starting one element into a buffer."""
    R, K = w.shape
    base = torch.from_numpy(w).to(dtype)
    vals = base.float().numpy()
    pad = torch.full((R, K + 24), 7.0, dtype=dtype)
    pad[:, :K] = base
    flat = torch.full((R * K + 1,), 7.0, dtype=dtype)
    flat[1:] = base.reshape(-1)
    off = flat.to(dev)[1:].view(R, K)
    assert off.data_ptr() % 16 != 0 and off.is_contiguous()
    return (("contiguous", base.to(dev), vals), ("strided", pad.to(dev)[:, :K], vals), ("offset", off, vals))


def _round_to(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dtype).float().numpy()


def _host(t):
    return t.detach().cpu().float().numpy()


def _pq(Wf, s, gs, symmetric, bits):
    """fp32 restatement of awq_pseudo_quant_kernel, operation by operation: returns (pseudo_quant(W s) / s, D = W - that,
    zero points or None), all fp32 and before any rounding to a 16-bit output."""
    R, K = Wf.shape
    g = K if gs <= 0 else gs
    v = (Wf * s[None, :]).reshape(R, K // g, g)
    assert v.dtype == f32
    if symmetric:
        amax = np.abs(v).max(axis=2, keepdims=True)
        max_int, min_int = f32(2 ** (bits - 1) - 1), f32(-(2 ** (bits - 1)))
        sc = np.maximum(amax, f32(1e-5)) / max_int
        q = np.minimum(np.maximum(np.rint(v / sc), min_int), max_int) * sc
        z = None
    else:
        mx, mn = v.max(axis=2, keepdims=True), v.min(axis=2, keepdims=True)
        max_int = f32(2 ** bits - 1)
        sc = np.maximum(mx - mn, f32(1e-5)) / max_int
        z = np.minimum(np.maximum(-np.rint(mn / sc), f32(0)), max_int)
        q = (np.minimum(np.maximum(np.rint(v / sc) + z, f32(0)), max_int) - z) * sc
    out = q.reshape(R, K) / s[None, :]
    D = Wf - out
    assert out.dtype == f32 and D.dtype == f32
    return out, D, z


def _scales(K, seed):
    return (0.5 + np.random.default_rng(seed).random(K)).astype(f32)


# ------------------------------------------------------------------------------------------- qt_awq_pseudo_quantize
@pytest.mark.parametrize("gs,K", GROUPS)
def test_pseudo_quantize_equals_the_fp32_restatement(ops, dev, gs, K):
    """Every grid point: rows x dtype x layout x symmetric / asymmetric x 4 / 8 bits.  The three device paths (the
    16-lane g128 vector kernel, the wave-per-group register kernel, the two-pass long / odd-group kernel) are each held
    to the same restatement, so they agree with one another to the bit wherever two of them can take the same input;
    at group 128 that is asserted directly on the raw bits (aligned call = vector kernel, offset view = generic)."""
    s_host = _scales(K, K + gs)
    s = torch.from_numpy(s_host).to(dev)
    for R in ROWS:
        w = _weights(R, K, 1000 * R + K)
        g = K if gs <= 0 else gs
        w[R - 1, K - g:] = np.abs(w[R - 1, K - g:]) + f32(0.01)          # all-positive group: zero point clamps at 0
        for dtype in DTYPES:
            lay = _layouts(w, dtype, dev)
            for symmetric in (True, False):
                for bits in (4, 8):
                    want, _, z = _pq(lay[0][2], s_host, gs, symmetric, bits)
                    want = _round_to(want, dtype)
                    assert np.all(np.isfinite(want))
                    if not symmetric:
                        assert z[R - 1, -1, 0] == 0                      # the clamp is in play
                    raw = {}
                    for name, W, _ in lay:
                        got = ops.awq_pseudo_quantize(W, s, gs, symmetric, bits)
                        assert np.array_equal(_host(got), want), (R, dtype, name, symmetric, bits)
                        raw[name] = got
                    if gs == 128 and dtype != torch.float32:
                        assert torch.equal(raw["contiguous"].view(torch.int16), raw["offset"].view(torch.int16))
                        assert torch.equal(raw["contiguous"].view(torch.int16), raw["strided"].view(torch.int16))


def test_pseudo_quantize_agrees_with_the_oracle(ops, dev, oracle):
    """The restatement above is the oracle's ``awq_pseudo_quantize`` (upstream's ``_pseudo_quantize_tensor``)."""
    w = _weights(65, 264, 3)
    s = _scales(264, 4)
    for gs, symmetric, bits in ((-1, True, 8), (88, False, 4), (24, True, 4)):
        mine, _, _ = _pq(w, s, gs, symmetric, bits)
        theirs = oracle.awq_pseudo_quantize((w * s[None, :]).astype(f32), gs, symmetric, bits) / s[None, :]
        assert np.array_equal(mine, theirs.astype(f32))


@pytest.mark.parametrize("gs,K", [(128, 256), (64, 192), (40, 200), (-1, 1152)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pseudo_quantize_out_may_alias_w(ops, dev, gs, K, dtype):
    s = torch.from_numpy(_scales(K, 9)).to(dev)
    W = torch.from_numpy(_weights(100, K, 5)).to(dtype).to(dev)
    for symmetric in (True, False):
        want = ops.awq_pseudo_quantize(W, s, gs, symmetric, 4)
        Wa = W.clone()
        got = ops.awq_pseudo_quantize(Wa, s, gs, symmetric, 4, out=Wa)
        assert got.data_ptr() == Wa.data_ptr() and torch.equal(Wa, want)


@pytest.mark.parametrize("gs,K", [(32, 96), (128, 256), (192, 576), (-1, 200)])
def test_pseudo_quantize_edges_all_zero_and_all_positive_groups(ops, dev, gs, K):
    """An all-zero group: amax (or max - min) clamps at 1e-5, every level is 0, the output is exactly 0.  A group whose
    scaled values are all positive, asymmetric: -rint(min / scale) is negative and the zero point clamps at 0, so the
    group is quantised on [0, max_int] * scale and its smallest values are NOT mapped to level 0 -- the restatement says
    by how much."""
    g = K if gs <= 0 else gs
    s_host = _scales(K, 2)
    s = torch.from_numpy(s_host).to(dev)
    w = _weights(4, K, 8)
    w[1, :g] = 0
    w[2, :g] = np.abs(w[2, :g]) + f32(0.5)
    for dtype in DTYPES:
        Wt = torch.from_numpy(w).to(dtype)
        for symmetric in (True, False):
            got = _host(ops.awq_pseudo_quantize(Wt.to(dev), s, gs, symmetric, 4))
            want, _, z = _pq(Wt.float().numpy(), s_host, gs, symmetric, 4)
            assert np.array_equal(got, _round_to(want, dtype))
            assert np.all(got[1, :g] == 0)
            if not symmetric:
                assert z[2, 0, 0] == 0 and z[1, 0, 0] == 0
                assert np.all(got[2, :g] > 0)


# ------------------------------------------------------------------------------------ qt_awq_weight_mean_accumulate
def _wmean_f64(vals, gs):
    R, K = vals.shape
    g = K if gs <= 0 else gs
    a = np.abs(vals.astype(np.float64)).reshape(R, K // g, g)
    return (a / (a.max(axis=2, keepdims=True) + np.float64(f32(1e-6)))).reshape(R, K).sum(axis=0)


def _wmean_f32(vals, gs, start=None):
    """The device's own sequence in fp32: per 64-row chunk an ascending-row chain of |w| / (group max + 1e-6), the chunk
    sums added in ascending order from 0, the result added to what w_sum held."""
    R, K = vals.shape
    g = K if gs <= 0 else gs
    a = np.abs(vals).reshape(R, K // g, g)
    term = (a / (a.max(axis=2, keepdims=True) + f32(1e-6))).reshape(R, K)
    assert term.dtype == f32
    total = np.zeros(K, f32)
    for r0 in range(0, R, 64):
        acc = np.zeros(K, f32)
        for r in range(r0, min(R, r0 + 64)):
            acc = acc + term[r]
        total = total + acc
    return (np.zeros(K, f32) if start is None else start) + total


@pytest.mark.parametrize("gs,K", GROUPS)
def test_weight_mean_against_fp64_and_the_fp32_sequence(ops, dev, gs, K):
    """fp64 reference sum_r |w| / (group absmax + 1e-6) per column, tolerance (R + 3) * 2^-24 * ref: every term carries two
    roundings (the sum with 1e-6 and the quotient), then a chain of R non-negative fp32 sums (64-row chunks, the chunk
    sums, the running total) whose error is bounded by its length times the unit roundoff of the result.  The second
    call accumulates (2 R terms).  Beyond the tolerance, all three paths (register kernel, long-group table, short-group
    kernel) must EQUAL the fp32 restatement of that sequence."""
    for R in ROWS:
        w = _weights(R, K, 77 * R + K)
        w[:, 5] = 0                                                       # a zero column: the sum stays exactly 0
        for dtype in DTYPES:
            for name, W, vals in _layouts(w, dtype, dev):
                ref = _wmean_f64(vals, gs)
                out = torch.zeros(K, dtype=torch.float32, device=dev)
                ops.awq_weight_mean_accumulate(W, gs, out)
                one = _host(out)
                ops.awq_weight_mean_accumulate(W, gs, out)
                two = _host(out)
                assert np.all(np.abs(one - ref) <= (R + 3) * EPS * ref), (R, dtype, name)
                assert np.all(np.abs(two - 2 * ref) <= (2 * R + 3) * EPS * 2 * ref), (R, dtype, name)
                first = _wmean_f32(vals, gs)
                assert np.array_equal(one, first), (R, dtype, name)
                assert np.array_equal(two, _wmean_f32(vals, gs, first)), (R, dtype, name)
                assert one[5] == 0


def test_weight_mean_70000_rows_on_the_register_path_and_the_long_path_refusal(ops, dev):
    """The register path has no row limit (1094 chunks in gridDim.y); the long-group path launches one workgroup per
    (group, row) and documents R <= 65535 per call: that call is refused and w_sum is left alone."""
    R, K = 70000, 128
    w = _weights(R, K, 12)
    W = torch.from_numpy(w).to(torch.bfloat16)
    vals = W.float().numpy()
    out = torch.zeros(K, dtype=torch.float32, device=dev)
    ops.awq_weight_mean_accumulate(W.to(dev), 128, out)
    got, ref = _host(out), _wmean_f64(vals, 128)
    assert np.all(np.abs(got - ref) <= (R + 3) * EPS * ref)
    assert np.array_equal(got, _wmean_f32(vals, 128))
    # K = 72: one group per row that is neither a multiple of 64 nor shorter than 64 -- the long-group path
    W72 = torch.from_numpy(_weights(R, 72, 13)).to(torch.bfloat16).to(dev)
    out72 = torch.full((72,), 3.0, dtype=torch.float32, device=dev)
    with pytest.raises(HipBackendError) as e:
        ops.awq_weight_mean_accumulate(W72, -1, out72)
    assert e.value.status == QT_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out72 == 3.0).all())
    # the same rows in two calls are taken
    ops.awq_weight_mean_accumulate(W72[:40000], -1, out72)
    ops.awq_weight_mean_accumulate(W72[40000:], -1, out72)
    ref = 3.0 + _wmean_f64(W72.float().cpu().numpy(), -1)
    assert np.all(np.abs(_host(out72) - ref) <= (40000 + 3) * EPS * ref)


# ----------------------------------------------------------------------------------------------------- qt_awq_scales
@pytest.mark.parametrize("K", [8, 1000, 1024, 4104])
@pytest.mark.parametrize("n_grid", [1, 7, 20])
@pytest.mark.parametrize("duo", [True, False])
def test_awq_scales_against_fp64(ops, dev, K, n_grid, duo):
    """fp64 evaluation of s = clamp(x_mean^r / (w_mean^(1-r) + 1e-4), 1e-4) / sqrt(max s * min s) at the rtol the suite
    already holds the scales to (2e-5, test_awq_channelwise_w8a16: powf is good to a few ulp, not exact).  A channel with
    x_mean = 0 gives pow(0, 0) = 1 at ratio 0 and 0 -> the 1e-4 clamp at every later ratio; one with w_mean = 0 leaves
    the bare 1e-4 in the denominator.  The normalisation: sqrt(max * min) of what comes back is 1 within 1e-6 (two
    fp32 roundings of the quotients: 1.2e-7)."""
    rng = np.random.default_rng(K + n_grid)
    n_tok, n_rows = 1234, 77
    xs = (rng.random(K) * 3 * n_tok).astype(f32)
    wsum = (rng.random(K) * 0.8 * n_rows + 0.01).astype(f32)
    xs[3], wsum[5] = 0, 0
    got = _host(ops.awq_scales(torch.from_numpy(xs).to(dev), n_tok, torch.from_numpy(wsum).to(dev), n_rows, n_grid, duo))
    xm, wm = xs.astype(np.float64) / n_tok, wsum.astype(np.float64) / n_rows
    for gi in range(n_grid):
        r = gi / n_grid
        sref = np.power(xm, r) / (np.power(wm, 1 - r) + 1e-4) if duo else np.power(xm, r)
        sref = np.maximum(sref, 1e-4)
        if gi == 0:
            assert sref[3] == (1 / (wm[3] + 1e-4) if duo else 1.0)
        else:
            assert sref[3] == 1e-4
        sref = sref / np.sqrt(sref.max() * sref.min())
        np.testing.assert_allclose(got[gi], sref, rtol=2e-5, atol=0)
        g64 = got[gi].astype(np.float64)
        assert abs(np.sqrt(g64.max() * g64.min()) - 1.0) <= 1e-6


# ------------------------------------------------------------------------------------- qt_awq_loss / qt_awq_losses
LOSS_GROUPS = ((32, 256), (40, 200), (64, 192), (128, 256), (128, 1152), (192, 576), (512, 1024), (1024, 1024), (-1, 264),
               (-1, 200))
# the tolerances the suite already states (test_gpu_awq_smoothquant.py): exact 1e-5 at 4 bits, 5e-4 at 8 bits
# (test_awq_exact_rescoring..., test_awq_channelwise_w8a16); fast 3e-3 at 4 bits, 1e-2 at 8 bits (test_awq_two_balance_layers...,
# test_awq_channelwise_w8a16)
LOSS_RTOL = {(1, 4): 1e-5, (1, 8): 5e-4, (0, 4): 3e-3, (0, 8): 1e-2}


def _gram(K, n_tok, seed):
    X = np.random.default_rng(seed).standard_normal((n_tok, K))
    X[:, ::37] *= 8
    G = (X.T @ X).astype(f32)
    return np.ascontiguousarray(np.tril(G) + np.tril(G, -1).T)


def _loss_f64(G, D, n_tok):
    D = D.astype(np.float64)
    return float(np.sum((D @ G.astype(np.float64)) * D) / (n_tok * D.shape[0]))


@pytest.mark.parametrize("gs,K", LOSS_GROUPS)
def test_awq_loss_against_fp64_from_the_restated_difference(ops, dev, gs, K):
    """D = W - pseudo_quant(W s) / s from the fp32 restatement (equal to the device's, shown above), then
    <G, D^T D>_F / (n R) in fp64: the product alone is under test, not rounding flips of the quantiser.  R % 64 == 0 takes
    the fused Frobenius epilogue (the path real jobs run), other R the materialised D^T D; exact = 1 the f32 GEMM.
    ``weight`` scales the loss and ``accumulate`` adds it to what loss_out held (one fp32 rounding of the sum more)."""
    n_tok = 2 * K
    Gh = _gram(K, n_tok, K)
    G = torch.from_numpy(Gh).to(dev)
    s_host = _scales(K, K + 1)
    s = torch.from_numpy(s_host).to(dev)
    for R, dtype in ((64, torch.bfloat16), (100, torch.bfloat16), (128, torch.float16), (65, torch.float32)):
        Wt = torch.from_numpy(_weights(R, K, R + K, 0.05)).to(dtype)
        W = Wt.to(dev)
        for symmetric in (True, False):
            for bits in (4, 8):
                _, D, _ = _pq(Wt.float().numpy(), s_host, gs, symmetric, bits)
                ref = _loss_f64(Gh, D, n_tok)
                assert ref > 0
                for exact in (0, 1):
                    rtol = LOSS_RTOL[(exact, bits)]
                    out = torch.full((1,), 123.0, dtype=torch.float32, device=dev)
                    ops.awq_loss(W, s, gs, symmetric, bits, G, n_tok, out, exact=bool(exact))
                    got = float(out.item())
                    print(f"gs={gs} K={K} R={R} {dtype} sym={symmetric} bits={bits} exact={exact}: rel err "
                          f"{abs(got - ref) / ref:.2e} (rtol {rtol:.0e})")
                    assert abs(got - ref) <= rtol * ref, (R, dtype, symmetric, bits, exact, got, ref)
                    out.fill_(0.5)
                    ops.awq_loss(W, s, gs, symmetric, bits, G, n_tok, out, exact=bool(exact), weight=0.25, accumulate=True)
                    acc = float(out.item())
                    assert abs(acc - (0.5 + 0.25 * ref)) <= rtol * 0.25 * ref + EPS * (0.5 + 0.25 * ref)


@pytest.mark.parametrize("R,gs,K", [(128, 128, 256), (100, 128, 256), (128, 64, 192), (64, 128, 1152)])
def test_awq_losses_against_the_same_fp64_numbers(ops, dev, R, gs, K):
    """qt_awq_losses, batched (R % 64 == 0, 16-bit, g128) and the per-point fallback (R % 64 != 0; a group size other
    than 128), against the fp64 losses above at the fast form's tolerance (3e-3, 4 bits); accumulate adds."""
    n_tok, n_grid = 2 * K, 5
    Gh = _gram(K, n_tok, K + 3)
    G = torch.from_numpy(Gh).to(dev)
    sc = np.stack([_scales(K, 50 + i) for i in range(n_grid)])
    Wt = torch.from_numpy(_weights(R, K, R)).to(torch.bfloat16)
    ref = np.array([_loss_f64(Gh, _pq(Wt.float().numpy(), sc[i], gs, True, 4)[1], n_tok) for i in range(n_grid)])
    out = torch.full((n_grid,), 9.0, dtype=torch.float32, device=dev)
    ops.awq_losses(Wt.to(dev), torch.from_numpy(sc).to(dev), gs, True, 4, G, n_tok, out)
    got = _host(out).astype(np.float64)
    print(f"R={R} gs={gs} K={K}: rel err {np.abs(got - ref) / ref}")
    assert np.all(np.abs(got - ref) <= 3e-3 * ref)
    ops.awq_losses(Wt.to(dev), torch.from_numpy(sc).to(dev), gs, True, 4, G, n_tok, out, weight=0.5, accumulate=True)
    assert np.all(np.abs(_host(out) - 1.5 * ref) <= 3e-3 * 1.5 * ref)


# ------------------------------------------------------------ qt_rtn_quantize, qt_scale_columns, qt_col_absmax_accumulate
SMALL = ((40, 200), (-1, 264), (128, 1152), (64, 256))


@pytest.mark.parametrize("gs,K", SMALL)
def test_rtn_quantize_equals_numpy_fp32(ops, dev, gs, K):
    """x = w / scale; x = x + zp; clamp to [qmin, qmax]; rint -- in that order, in fp32; Qt is [K, R]."""
    g = K if gs <= 0 else gs
    G = K // g
    gcol = np.arange(K) // g
    for R in ROWS:
        rng = np.random.default_rng(R + K)
        w = _weights(R, K, R * 3 + K)
        for bits in (4, 8):
            qmin, qmax = f32(-(2 ** (bits - 1))), f32(2 ** (bits - 1) - 1)
            scale = ((0.5 + rng.random((R, G))) * 0.2 / 2 ** bits).astype(f32)
            zp = rng.integers(int(qmin), int(qmax) + 1, (R, G)).astype(f32)
            for dtype in DTYPES:
                for name, W, vals in _layouts(w, dtype, dev):
                    x = vals / scale[:, gcol]
                    x = x + zp[:, gcol]
                    want = np.rint(np.minimum(np.maximum(x, qmin), qmax)).astype(np.int8).T
                    got = ops.rtn_quantize(W, torch.from_numpy(scale).to(dev), torch.from_numpy(zp).to(dev), gs, bits)
                    assert np.array_equal(got.cpu().numpy(), want), (R, bits, dtype, name)


@pytest.mark.parametrize("K", [200, 264, 1152, 256])
def test_scale_columns_equals_numpy_fp32(ops, dev, K):
    """The fp32 product (quotient) rounded once to the weight's dtype."""
    s_host = _scales(K, K)
    s = torch.from_numpy(s_host).to(dev)
    for R in ROWS:
        w = _weights(R, K, R + 11 * K)
        for dtype in DTYPES:
            for name, W, vals in _layouts(w, dtype, dev):
                assert np.array_equal(_host(ops.scale_columns(W, s)), _round_to(vals * s_host[None, :], dtype)), (R, dtype, name)
                assert np.array_equal(_host(ops.scale_columns(W, s, divide=True)), _round_to(vals / s_host[None, :], dtype)), (
                    R, dtype, name)


@pytest.mark.parametrize("K", [200, 264, 1152, 256])
def test_col_absmax_running_maximum_equals_numpy(ops, dev, K):
    """A maximum has no rounding: exact.  Two calls keep the running maximum; an all-zero column stays 0."""
    for R in (1, 127, 128, 129, 300):
        w1, w2 = _weights(R, K, R + K, 1.0), _weights(R, K, R + K + 1, 1.0)
        w1[:, 9], w2[:, 9] = 0, 0
        for dtype in DTYPES:
            for (name, W1, v1), (_, W2, v2) in zip(_layouts(w1, dtype, dev), _layouts(w2, dtype, dev)):
                out = torch.zeros(K, dtype=torch.float32, device=dev)
                ops.col_absmax_accumulate(W1, out)
                assert np.array_equal(_host(out), np.abs(v1).max(axis=0)), (R, dtype, name)
                ops.col_absmax_accumulate(W2, out)
                assert np.array_equal(_host(out), np.maximum(np.abs(v1).max(axis=0), np.abs(v2).max(axis=0))), (R, dtype, name)
                assert float(out[9]) == 0


# ---------------------------------------------------------------------------------------------- qt_smoothquant_scales
@pytest.mark.parametrize("K", [8, 264, 1000])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_smoothquant_scales_against_fp64(ops, dev, K, alpha):
    """s = (cmax - cmin)^alpha / wmax^(1 - alpha), s = cmax - cmin where wmax == 0, in fp64 at the rtol the suite already
    uses for it (1e-5, test_smoothquant_scales_and_apply).  A constant channel has a = 0: pow(0, alpha) is 1 at
    alpha = 0 and 0 otherwise."""
    rng = np.random.default_rng(K)
    cmin = (-rng.random(K) * 4).astype(f32)
    cmax = (rng.random(K) * 6).astype(f32)
    wmax = (rng.random(K) + 0.01).astype(f32)
    cmin[2] = cmax[2] = f32(1.25)
    wmax[4] = 0
    got = _host(ops.smoothquant_scales(*(torch.from_numpy(a).to(dev) for a in (cmin, cmax, wmax)), alpha))
    a = cmax.astype(np.float64) - cmin.astype(np.float64)
    with np.errstate(divide="ignore"):
        ref = np.where(wmax > 0, np.power(a, alpha) / np.power(wmax.astype(np.float64), 1 - alpha), a)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=0)
    assert got[2] == (pytest.approx(1 / float(wmax[2]), rel=1e-6) if alpha == 0 else 0)
    assert got[4] == f32(cmax[4] - cmin[4])


# ------------------------------------------------------------------------------------- qt_argmin_f32, qt_symmetrize_lower
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024])
def test_argmin_first_minimum_ties_and_nan(ops, dev, n):
    rng = np.random.default_rng(n)
    v = rng.standard_normal(n).astype(f32)
    assert int(ops.argmin_first(torch.from_numpy(v).to(dev)).item()) == int(np.argmin(v))
    if n > 1:
        # ties keep the first index: the minimum again in the same lane's next element, in a neighbouring lane, and last
        for first, second in ((n // 3, min(n - 1, n // 3 + 64)), (n // 2, n // 2 + 1 if n // 2 + 1 < n else 0), (0, n - 1)):
            t = v.copy()
            t[first] = t[second] = f32(-10)
            assert int(ops.argmin_first(torch.from_numpy(t).to(dev)).item()) == min(first, second)
        # a NaN never wins, wherever it sits
        t = v.copy()
        t[0] = np.nan
        t[n - 1] = np.nan
        if n > 2:
            assert int(ops.argmin_first(torch.from_numpy(t).to(dev)).item()) == int(np.nanargmin(t))
        t = np.full(n, np.nan, f32)
        t[n - 1] = 2.0
        assert int(ops.argmin_first(torch.from_numpy(t).to(dev)).item()) == n - 1


def test_argmin_refuses_more_than_1024_values(ops, dev):
    with pytest.raises(HipBackendError) as e:
        ops.argmin_first(torch.zeros(1025, dtype=torch.float32, device=dev))
    assert e.value.status == QT_ERR_INVALID


@pytest.mark.parametrize("K", [200, 1032])
def test_symmetrize_lower_mirrors_and_keeps_the_lower_triangle(ops, dev, K):
    g = np.random.default_rng(K).standard_normal((K, K)).astype(f32)
    G = torch.from_numpy(g).to(dev)
    ops.symmetrize_lower(G)
    got = _host(G)
    assert np.array_equal(np.tril(got), np.tril(g))                      # lower triangle and diagonal unchanged
    assert np.array_equal(got, got.T)                                      # upper == lower
