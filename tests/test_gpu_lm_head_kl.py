"""``qt_lm_head_kl`` on the GPU.

1. Each side is the NLL kernel's, to the bit: ``lse``, ``argmax`` and ``nll`` of the P and the Q side equal
   ``ops.lm_head_nll`` on (Hp, W) and (Hq, W), with int32 and int64 targets, the ignore index and targets >= V, on random
   inputs and on the exactly summable +-{1, 2, 3} inputs of ``tests/exact_inputs.py`` with planted columns and a tie.
2. Equal rows give exactly zero: ``kl == 0.0`` and bit-equal ``lse_p`` / ``lse_q`` wherever ``Hq[m] == Hp[m]``.
3. A row depends on the row alone: one (Hp, Hq) row pair at index 0, 127, 128, M - 1, alone, and in strided views of
   different pitches 16 bytes off a 256-byte boundary gives seven bit-equal outputs.
4. The numeric bar on random inputs, against the fp64 KL of the same 16-bit inputs: the kernel's maximum absolute error
   is at most max(4 x the maximum error of the same formula evaluated in fp32 on the CPU, 2^-22 max|lse|).  The factor 4
   is the convention of test_gpu_lm_head_nll.py; the floor is one fp32 ulp for each of the two ``lse`` terms that cancel
   in ``t / s - lse_p + lse_q``.
5. The workspace contract by the guard-pattern method of test_gpu_lm_head_workspace.py.

128 is the row-tile edge of this kernel (256 is the NLL kernel's), so M walks {1, 127, 128, 129, 300}.
"""
import math

import numpy as np
import pytest
import torch

from quantool_amd.hip import _lib
from tests.exact_inputs import assert_exactly_summable, dense_ints

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
MARGIN = 4.0
FIELDS = ("kl", "nll_p", "nll_q", "lse_p", "lse_q", "argmax_p", "argmax_q")

CASES = [  # (M, V, K, dtype): a cross of the edges, not the full product
    (1, 256, 128, BF), (1, 2049, 1024, FP), (1, 513, 256, BF),
    (127, 513, 256, FP), (127, 1000, 128, BF),
    (128, 256, 1024, BF), (128, 2049, 256, FP),
    (129, 513, 128, BF), (129, 1000, 1024, FP),
    (300, 2049, 128, FP), (300, 256, 256, BF), (300, 1000, 256, BF),
]
IDS = [f"{m}x{v}x{k}-{str(d).replace('torch.', '')}" for m, v, k, d in CASES]


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _random(M, V, K, dtype, seed, kind="near"):
    g = torch.Generator().manual_seed(seed)
    Hp = torch.randn(M, K, generator=g).to(dtype)
    W = (torch.randn(V, K, generator=g) * (3.0 / math.sqrt(K))).to(dtype)
    if kind == "near":
        Hq = (Hp.float() + 0.05 * torch.randn(M, K, generator=g)).to(dtype)
    else:
        Hq = torch.randn(M, K, generator=g).to(dtype)
    tg = torch.randint(0, V, (M,), generator=g)
    return Hp, Hq, W, tg


def _assert_sides_are_the_nll_kernels(ops, Hp, Hq, W, tg, what):
    r = ops.lm_head_kl(Hp, Hq, W, tg)
    for side, H in (("p", Hp), ("q", Hq)):
        nll, lse, argmax = ops.lm_head_nll(H, W, tg)
        for name, got, want in (("nll", getattr(r, "nll_" + side), nll), ("lse", getattr(r, "lse_" + side), lse),
                                ("argmax", getattr(r, "argmax_" + side), argmax)):
            assert torch.equal(bits(got), bits(want)), f"{what}: {name}_{side} is not ops.lm_head_nll's"
    return r


@pytest.mark.parametrize("M,V,K,dtype", CASES, ids=IDS)
def test_each_side_is_the_nll_kernels_to_the_bit(ops, dev, M, V, K, dtype):
    Hp, Hq, W, tg = _random(M, V, K, dtype, 31 * M + V + K)
    if M > 2:
        tg[1], tg[M - 2] = -100, V                   # the ignore index, a target past V
    if M > 140:
        tg[130], tg[131] = V + 7, -1
    Hp, Hq, W = Hp.to(dev), Hq.to(dev), W.to(dev)
    for tdt in (torch.int64, torch.int32):
        r = _assert_sides_are_the_nll_kernels(ops, Hp, Hq, W, tg.to(dev, tdt), f"random, {tdt}")
        if M > 2:
            assert float(r.nll_p[1]) == 0.0 and float(r.nll_q[1]) == 0.0
            assert math.isnan(float(r.nll_p[M - 2])) and math.isnan(float(r.nll_q[M - 2]))
            assert bool(torch.isfinite(r.kl).all()) and bool(torch.isfinite(r.lse_p).all())
    none = ops.lm_head_kl(Hp, Hq, W)                  # targets=None: every row carries the ignore index
    for n in ("kl", "lse_p", "lse_q", "argmax_p", "argmax_q"):
        assert torch.equal(bits(getattr(none, n)), bits(getattr(r, n))), n
    assert not bool(none.nll_p.any()) and not bool(none.nll_q.any())


@pytest.mark.parametrize("M,V,K,dtype", CASES, ids=IDS)
def test_exactly_summable_inputs(ops, dev, M, V, K, dtype):
    """+-{1, 2, 3} operands: every logit of either side is an integer below 2^24, so the target logits and the argmax
    are exact on both sides (planted dominant columns at the edges of the lane, wave and tile maps, and a tie), and
    a - b is an exact integer."""
    from tests.test_gpu_lm_head_nll import _exact_inputs

    seed = 7 * M + V + K
    Hp, W, tg, probes, tie = _exact_inputs(M, V, K, seed)
    Hq = dense_ints((M, K), seed + 5)
    for j, (m, v) in enumerate(probes):
        if j % 2:                                      # every second planted row: the Q side sees the planted column too
            Hq[m] = Hp[m]
    assert_exactly_summable(9 * K, 0, "logits of +-{1,2,3} operands")
    a64 = torch.from_numpy(Hp.astype(np.float64)) @ torch.from_numpy(W.astype(np.float64)).T
    b64 = torch.from_numpy(Hq.astype(np.float64)) @ torch.from_numpy(W.astype(np.float64)).T
    Hpd, Hqd, Wd = (torch.from_numpy(x).to(dev, dtype) for x in (Hp, Hq, W))
    for tdt in (torch.int64, torch.int32):
        tgd = torch.from_numpy(tg).to(dev, tdt)
        r = _assert_sides_are_the_nll_kernels(ops, Hpd, Hqd, Wd, tgd, f"exact, {tdt}")
        assert torch.equal(r.argmax_p.cpu().long(), torch.from_numpy(np.argmax(a64.numpy(), axis=1)))
        assert torch.equal(r.argmax_q.cpu().long(), torch.from_numpy(np.argmax(b64.numpy(), axis=1)))
        for m, v in probes:
            assert int(r.argmax_p[m]) == v
        if tie is not None:
            assert int(r.argmax_p[tie]) == 1
        # the target logits, exact: lse - nll is one fp32 subtraction away from the integer
        idx = torch.from_numpy(tg).unsqueeze(1)
        for lse, nll, x64 in ((r.lse_p, r.nll_p, a64), (r.lse_q, r.nll_q, b64)):
            want = (lse.cpu() - x64.gather(1, idx).squeeze(1).float())
            assert torch.equal(bits(nll.cpu()), bits(want))
    # KL against fp64.  The logits are exact here, so what is left is the arithmetic of the record: kl is the sum of
    # three fp32 terms of magnitude D = max_v |a - b|, |lse_p| and |lse_q|; t passes at most 1 + 5 + 3 + 9 = 18 merges
    # of two products, a sum and an expf (2 ulp) each, so 2^-17 (D + |lse_p| + |lse_q|) bounds the error per row, and a
    # dropped, doubled or misplaced a - b moves kl by whole units
    kl64, lp64, lq64 = _kl64(a64, b64)
    err = (r.kl.cpu().double() - kl64).abs()
    bar = 2.0 ** -17 * ((a64 - b64).abs().max(dim=1).values + lp64.abs() + lq64.abs())
    print(f"exact M={M} V={V} K={K}: kl max {float(kl64.max()):.3e}, max err {float(err.max()):.3e}, "
          f"max err / bar {float((err / bar).max()):.3f}")
    assert bool((err <= bar).all()), (float((err / bar).max()), int((err / bar).argmax()))
    same = torch.from_numpy((Hp == Hq).all(axis=1))
    assert bool((r.kl.cpu()[same] == 0).all())


# -------------------------------------------------------------------------------------------------- equal rows: zero
@pytest.mark.parametrize("M,V,K,dtype", [(300, 1000, 256, BF), (129, 2049, 128, FP), (1, 513, 1024, BF)],
                         ids=["300x1000x256-bf16", "129x2049x128-fp16", "1x513x1024-bf16"])
def test_equal_rows_give_exactly_zero(ops, dev, M, V, K, dtype):
    Hp, other, W, tg = _random(M, V, K, dtype, 99 + M, kind="far")
    Hq = Hp.clone()
    changed = [m for m in (0, 5, 127, 128, 200, M - 1) if 0 < m < M]
    for m in changed:
        Hq[m] = other[m]
    r = ops.lm_head_kl(Hp.to(dev), Hq.to(dev), W.to(dev), tg.to(dev))
    keep = torch.ones(M, dtype=torch.bool)
    keep[changed] = False
    kl = r.kl.cpu()
    assert bool((bits(kl[keep]) == 0).all()), kl[keep].abs().max()       # +0.0, not -0.0, not 1e-9
    assert torch.equal(bits(r.lse_p.cpu())[keep], bits(r.lse_q.cpu())[keep])
    assert torch.equal(bits(r.nll_p.cpu())[keep], bits(r.nll_q.cpu())[keep])
    assert torch.equal(r.argmax_p.cpu()[keep], r.argmax_q.cpu()[keep])
    if changed:
        assert bool((kl[changed] > 1e-3).all()), kl[changed]


# ------------------------------------------------------------------------------------------- a row depends on the row
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_a_row_depends_on_the_row_alone(ops, dev, dtype):
    M, K, V = 300, 256, 1000
    Hp, Hq, W, tg = _random(M, V, K, dtype, 11)
    places = (0, 127, 128, M - 1)
    for p in places:
        Hp[p], Hq[p], tg[p] = Hp[0], Hq[0], tg[0]
    W = W.to(dev)
    base = ops.lm_head_kl(Hp.to(dev), Hq.to(dev), W, tg.to(dev))
    alone = ops.lm_head_kl(Hp[:1].to(dev), Hq[:1].to(dev), W, tg[:1].to(dev))

    def strided(X, ld):                               # a view of pitch ld whose base lies 16 bytes behind a 256-byte edge
        flat = torch.zeros(M * ld + 256, dtype=dtype, device=dev)
        off = ((-flat.data_ptr()) % 256 + 16) // 2
        v = flat[off:off + M * ld].view(M, ld)[:, :K]
        v.copy_(X)
        assert v.data_ptr() % 256 == 16 and v.stride(0) == ld
        return v

    views = ops.lm_head_kl(strided(Hp, K + 72), strided(Hq, K + 8), W, tg.to(dev))
    for name, a, b, c in zip(FIELDS, base, views, alone):
        assert torch.equal(bits(a), bits(b)), f"{name}: the strided, shifted views differ from the contiguous call"
        row = bits(a)[list(places)]
        assert bool((row == row[0]).all()), f"{name}: the same row at {places} gives {a[list(places)].tolist()}"
        assert torch.equal(bits(a)[:1], bits(c)), f"{name}: the row alone (M = 1) differs from the row among {M}"
    again = ops.lm_head_kl(Hp.to(dev), Hq.to(dev), W, tg.to(dev))
    for a, b in zip(base, again):
        assert torch.equal(bits(a), bits(b))


def test_outputs_past_m_and_m_zero(dev):
    lib = _lib.load()
    M, K, V, extra = 129, 128, 513, 64
    Hp, Hq, W, tg = (x.to(dev) for x in _random(M, V, K, BF, 3))
    outs = [torch.full((M + extra,), -12345.5, dtype=torch.float32, device=dev) for _ in range(5)]
    outs += [torch.full((M + extra,), -77, dtype=torch.int32, device=dev) for _ in range(2)]
    ws = torch.empty(lib.qt_lm_head_kl_workspace_size(M, V), dtype=torch.uint8, device=dev)

    def call(m):
        return lib.qt_lm_head_kl(Hp.data_ptr(), K, Hq.data_ptr(), K, W.data_ptr(), K, _lib.QT_BF16, m, K, V,
                                 tg.data_ptr(), 8, *(o.data_ptr() for o in outs), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream)

    before = [o.clone() for o in outs]
    assert lib.qt_lm_head_kl_workspace_size(0, V) == 0
    assert call(0) == _lib.QT_OK
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, before)), "M = 0 wrote an output"
    assert call(M) == _lib.QT_OK, lib.qt_last_error()
    torch.cuda.synchronize()
    for name, o, b in zip(FIELDS, outs, before):
        assert torch.equal(o[M:], b[M:]), f"{name}: memory past M was written"
        assert not bool((o[:M] == b[:M]).any()), f"{name}: a row was not written"


# -------------------------------------------------------------------------------------------------- the numeric bar
def _kl64(a, b):
    lp, lq = torch.logsumexp(a, -1), torch.logsumexp(b, -1)
    P = torch.exp(a - lp.unsqueeze(1))
    return (P * (a - b)).sum(-1) - lp + lq, lp, lq


def _kl_fp32(Hp, Hq, W):
    """The yardstick: the kernel's formula evaluated in fp32 on the CPU."""
    f = lambda x: torch.as_tensor(x).float()           # noqa: E731
    a, b = f(Hp) @ f(W).T, f(Hq) @ f(W).T
    lp, lq = torch.logsumexp(a, -1), torch.logsumexp(b, -1)
    P = torch.softmax(a, -1)
    return ((P * (a - b)).sum(-1) - lp + lq).double()


RANDOM = [(300, 128, 513), (129, 256, 1000), (128, 1024, 2049), (127, 256, 256)]


@pytest.mark.parametrize("kind", ["near", "far"])
@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,K,V", RANDOM)
def test_numeric_bar_on_random_inputs(ops, dev, M, K, V, dtype, kind):
    """``near``: Hq = the 16-bit rounding of Hp + 0.05 N(0, 1), the small KL of a real checkpoint; ``far``: an
    independent Hq, a KL of several nats.  Measured on an MI355X (DESIGN.md 4.23 has the table per shape): the worst
    ratio of the kernel's maximum error to the yardstick's was 1.72 (fp16, 128 x 1024 x 2049, far)."""
    Hp, Hq, W, tg = _random(M, V, K, dtype, 1000 * M + K + V, kind)
    a64, b64 = Hp.double() @ W.double().T, Hq.double() @ W.double().T
    kl64, lp64, lq64 = _kl64(a64, b64)
    yard = (_kl_fp32(Hp, Hq, W) - kl64).abs()
    Hpd, Hqd, Wd = Hp.to(dev), Hq.to(dev), W.to(dev)
    r = ops.lm_head_kl(Hpd, Hqd, Wd, tg.to(dev))
    err = (r.kl.cpu().double() - kl64).abs()

    # what a user writes today: two 16-bit logit matrices, an fp32 log-softmax of each
    lp = torch.log_softmax(torch.nn.functional.linear(Hpd, Wd).float(), -1)
    lq = torch.log_softmax(torch.nn.functional.linear(Hqd, Wd).float(), -1)
    arm_err = ((lp.exp() * (lp - lq)).sum(-1).cpu().double() - kl64).abs()

    floor = 2.0 ** -22 * float(torch.maximum(lp64.abs(), lq64.abs()).max())
    bar = max(MARGIN * float(yard.max()), floor)
    ratio = float(err.max()) / float(yard.max())
    print(f"random {kind} M={M} K={K} V={V} {dtype}: kl mean {float(kl64.mean()):.3e}; kernel max {float(err.max()):.3e} "
          f"(row {int(err.argmax())}) mean {float(err.mean()):.3e}; yardstick max {float(yard.max()):.3e} mean "
          f"{float(yard.mean()):.3e}; ratio {ratio:.2f}; floor {floor:.3e}; logits arm mean {float(arm_err.mean()):.3e}")
    assert float(err.max()) <= bar, (int(err.argmax()), ratio)
    assert float(r.kl.min()) >= -floor                # not clamped, and never further below 0 than the floor
    assert (float((r.lse_p.cpu().double() - lp64).abs().max()) <= 1e-4 and
            float((r.lse_q.cpu().double() - lq64).abs().max()) <= 1e-4)


# ------------------------------------------------------------------------------------------- the workspace contract
PATTERN = 0xA5
WS_CASES = [  # (M, V, K, dtype, branch)
    (129, 513, 128, BF, "two row tiles, three vocabulary tiles, the last one column wide"),
    (100, 256, 256, FP, "one vocabulary tile: one record per row and side"),
]


def _first_bad(region):
    bad = (region != PATTERN).nonzero()
    return None if bad.numel() == 0 else (int(bad[0]), int(bad[-1]), int(bad.numel()))


@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("M,V,K,dtype,branch", WS_CASES, ids=[c[4].split(":")[0].split(",")[0] for c in WS_CASES])
def test_no_write_outside_the_workspace(ops, dev, M, V, K, dtype, branch, offset):
    lib = _lib.load()
    Hp, Hq, W, tg = (x.to(dev) for x in _random(M, V, K, dtype, M + V + K))
    outs = [torch.full((M,), -3.5, dtype=torch.float32, device=dev) for _ in range(5)]
    outs += [torch.full((M,), -9, dtype=torch.int32, device=dev) for _ in range(2)]
    need = int(lib.qt_lm_head_kl_workspace_size(M, V))
    tiles_n = (V + 255) // 256
    assert need == 32 * M * tiles_n + 8 * M and need > 0
    guard = (max(1 << 20, need) + 255) // 256 * 256
    start = guard + offset
    buf = torch.full((start + need + guard,), PATTERN, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    ws = buf.data_ptr() + start
    before = [o.clone() for o in outs]
    torch.cuda.synchronize()

    def call(wsp, nbytes):
        return lib.qt_lm_head_kl(Hp.data_ptr(), K, Hq.data_ptr(), K, W.data_ptr(), K,
                                 _lib.QT_BF16 if dtype == BF else _lib.QT_F16, M, K, V, tg.data_ptr(), 8,
                                 *(o.data_ptr() for o in outs), wsp, nbytes, torch.cuda.current_stream().cuda_stream)

    assert call(ws, need - 1) == _lib.QT_ERR_WORKSPACE
    assert call(None, need) == _lib.QT_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert _first_bad(buf) is None, "a refused call wrote to the workspace buffer"
    for n, o, b in zip(FIELDS, outs, before):
        assert torch.equal(o, b), f"a refused call wrote to {n}"

    rc = call(ws, need)
    assert rc == _lib.QT_OK, lib.qt_last_error()
    torch.cuda.synchronize()
    lo, hi = _first_bad(buf[:start]), _first_bad(buf[start + need:])
    assert hi is None, f"[{branch}] wrote past the {need} bytes it asked for: {hi}"
    assert lo is None, f"[{branch}] wrote in front of the workspace: {lo}"
    # every record has a writer (P: four words, Q: three and a zero), and so has every target logit (targets in [0, V))
    mid = buf[start:start + need]
    recs = mid[:32 * M * tiles_n].view(-1, 16)
    assert not bool((recs[:, :12] == PATTERN).all(dim=1).any()), "a record was never written"
    assert not bool((recs[:M * tiles_n, 12:] == PATTERN).all(dim=1).any()), "a P record's t was never written"
    tgts = mid[32 * M * tiles_n:].view(-1, 4)
    assert tgts.shape[0] == 2 * M and not bool((tgts == PATTERN).all(dim=1).any()), "a target logit was never written"

    got = ops.lm_head_kl(Hp, Hq, W, tg)
    for n, a, b in zip(FIELDS, outs, got):
        assert torch.equal(bits(a), bits(b)), f"{n} differs from the call through ops"
