"""``qt_weight_gather_qparams_mse`` against an fp64 restatement of its definition.

The bar on a group's relative excess ``err64[idx] / min_i err64[i] - 1`` is twice the relative error ``eps`` the kernel's
fp32 error sum can have against the fp64 one (if both candidates' sums are off by ``eps`` the kernel can prefer one that
is worse by ``(1 + eps) / (1 - eps) - 1``).  ``eps`` from the stated arithmetic, u = 2^-24, per element with
``e = (q - z) s - w`` and ``x = clamp(w / s + z)``:
  * e: one rounding of the product, one of the difference, ``u (|(q - z) s| + |e|)``, and where the fp32 ``x`` rounds to
    the other neighbour than the fp64 one (division and sum within ``2 u |x|`` of a tie) ``|e|`` moves by at most
    ``2 s 2 u |x|``; to first order ``|e|^norm`` moves by ``norm |e|^(norm - 1)`` times their sum;
  * the power: ``log2`` within 1 ulp (``2 u`` relative) and the rounded product with norm (``u``) put
    ``3 u norm |log2 e|`` on the exponent, so ``ln 2`` times that on ``exp2`` relatively, plus its own 1 ulp, ``2 u``;
  * the group sum of n terms: ``(n - 1) u``.
A group's ``eps`` is the largest over its candidates, evaluated on the fp64 reference (never on the kernel's output).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F, U, NORM, STEPS = np.float32, 2.0 ** -24, 2.4, 20
SHRINK = np.array([1.0 - i / 100.0 for i in range(STEPS)]).astype(F)


def qparams_f32(mn, mx, sym, bits):
    """calculate_qparams, fp32 operation by operation."""
    qmin, qmax = F(-(1 << (bits - 1))), F((1 << (bits - 1)) - 1)
    mn, mx = np.minimum(mn, F(0)), np.maximum(mx, F(0))
    if sym:
        s = np.maximum(np.maximum(np.abs(mn), np.abs(mx)) / ((qmax - qmin) / F(2)), F(2.0 ** -23))
        return s, np.zeros_like(s)
    s = np.maximum((mx - mn) / (qmax - qmin), F(2.0 ** -23))
    return s, np.clip(np.rint(qmin - mn / s), qmin, qmax)


def reference(Wf, gs, sym, bits):
    """Per (candidate, row, group): scale, zero point (fp32), the fp64 error and the bound ``eps`` on the kernel's."""
    R, K = Wf.shape
    Wg = Wf.reshape(R, K // gs, gs)
    p = SHRINK[:, None, None]
    s, z = qparams_f32(p * Wg.min(2), p * Wg.max(2), sym, bits)
    w, s64, z64 = Wg.astype(np.float64)[None], s.astype(np.float64)[..., None], z.astype(np.float64)[..., None]
    x = np.clip(w / s64 + z64, -(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    dq = (np.rint(x) - z64) * s64
    e = np.abs(dq - w)
    err = (e ** NORM).sum(-1)
    de = U * (np.abs(dq) + e) + 4 * U * s64 * np.abs(x)
    lg = np.abs(np.log2(np.maximum(e, 1e-300)))
    eps = (NORM * e ** (NORM - 1) * de + e ** NORM * (3 * np.log(2) * U * NORM * lg + 2 * U)).sum(-1) / err + (gs - 1) * U
    return s, z, err, eps


BF, HF, FP = torch.bfloat16, torch.float16, torch.float32
CASES = [  # R, K, dtype, symmetric, bits, group_size, perm + dead; 8 bits only where the fp64 choice still varies
    (5, 384, BF, True, 4, 128, True), (3, 2176, BF, True, 4, 128, False), (3, 2176, HF, False, 4, 128, True),
    (5, 384, HF, True, 4, 128, False), (3, 2176, FP, False, 4, 128, False), (5, 384, FP, True, 4, 128, True),
    (5, 384, BF, True, 4, 32, False), (5, 384, HF, False, 4, 32, True), (3, 2176, FP, False, 4, 32, False),
    (3, 2176, BF, True, 8, 32, True), (5, 384, FP, True, 8, 32, False),
    (5, 384, HF, True, 8, -1, True), (5, 384, HF, False, 4, -1, False), (5, 384, FP, True, 4, -1, True),
    (3, 2176, BF, False, 8, -1, False), (3, 2176, HF, True, 8, -1, True),
    (5, 384, BF, True, 4, 192, False),      # two wide groups: the workgroup-wide path more than once per row
]


@pytest.mark.parametrize("R,K,dtype,sym,bits,group_size,permuted", CASES)
def test_mse_observer_against_fp64(ops, dev, R, K, dtype, sym, bits, group_size, permuted):
    rng = np.random.default_rng(0)
    W = torch.from_numpy((rng.standard_t(3, (R, K)) * 0.02).astype(F)).to(dtype)
    Wf = W.float().numpy()
    gs = K if group_size <= 0 else group_size
    G = K // gs
    s, z, err, eps = reference(Wf, gs, sym, bits)
    first = err.argmin(0)
    assert len(np.unique(first)) >= (8 if gs == 128 else 2)          # a constant answer cannot pass

    perm = rng.permutation(K).astype(np.int32) if permuted else None
    dead = (rng.random(K) < 0.05).astype(np.uint8) if permuted else None
    out, sc, zp = (torch.empty(shape, dtype=FP, device=dev) for shape in ((R, K), (R, G), (R, G)))
    sc_t, zp_t = (torch.full((G, R + 3), -7.0, dtype=FP, device=dev) for _ in range(2))
    idx = torch.full((R, G), -1, dtype=torch.int8, device=dev)
    on = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    ops.weight_gather_qparams_mse(W.to(dev), on(perm), on(dead), group_size, sym, bits, out, sc, zp, sc_t[:, :R],
                                  zp_t[:, :R], idx=idx)
    alone = ops.group_mse_qparams(W.to(dev), group_size, sym, bits)
    torch.cuda.synchronize()

    i = idx.cpu().numpy().astype(np.int64)
    assert i.min() >= 0 and i.max() < STEPS
    pick = lambda a: np.take_along_axis(a, i[None], 0)[0]              # noqa: E731
    for got, got_t, want in ((sc, sc_t, pick(s)), (zp, zp_t, pick(z))):
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got_t.cpu().numpy()[:, :R], got.cpu().numpy().T)
        assert (got_t.cpu().numpy()[:, R:] == -7.0).all()
    for a, b in zip(alone, (sc, zp, sc_t[:, :R], zp_t[:, :R])):
        assert torch.equal(a, b)
    want = Wf if perm is None else np.where(dead[None] != 0, F(0), Wf[:, perm])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))

    excess = pick(err) / err.min(0) - 1.0
    bar = 2.0 * eps.max(0)
    print(f"max excess {excess.max():.3e}, bar {bar.min():.3e} .. {bar.max():.3e}, "
          f"{(i != first).sum()} of {i.size} groups off the fp64 choice, {len(np.unique(first))} distinct choices")
    assert (excess <= bar).all()
    assert (i[excess == 0.0] == first[excess == 0.0]).all()
