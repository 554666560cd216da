"""``qt_lm_head_nll`` on the GPU: exactly summable inputs pin which products each logit adds and which columns each
row's softmax sees; row independence and determinism; the ignore index, an out-of-range target and the memory past M;
and the numeric bar on random inputs against fp64, with the fp32 CPU evaluation of the same quantity as the yardstick.

Exact cases.  H and W hold +-{1, 2, 3}, so every logit is an integer of magnitude <= 9 K < 2^24 that fp32 holds exactly
in any summation order: ``tgt`` must equal the integer reference bit for bit, ``argmax`` its lowest maximal index.  In
every shape probe rows get a dominant column v* (W[v*] = 3 sign(H[m]): the logit 3 sum |H[m]| >= 3 K) at the edges of
the lane, wave and tile maps; a dropped, doubled or shifted column moves ``lse`` by whole units and moves ``argmax``.
``lse`` itself involves exp and log, so it is held to the bar of the random cases: 4x the error of the fp32 CPU
evaluation, and never less than 2^-23 |lse| (one unit in the last place of the result at most: with exact logits, the
rounding of the result is the error the format itself imposes).
"""
import math

import numpy as np
import pytest
import torch

from tests.exact_inputs import assert_exact, assert_exactly_summable, dense_ints

pytestmark = pytest.mark.gpu

MIN_K = 128
BF, FP = torch.bfloat16, torch.float16
MARGIN = 4.0            # bar (a): the kernel's maximum error over the yardstick's (DESIGN.md 4.22 records the measured)


def _fp64_rows(H, W, tg):
    """fp64 (logits, lse, nll) of 16-bit inputs given as float64 arrays."""
    x = torch.from_numpy(H) @ torch.from_numpy(W).T
    lse = torch.logsumexp(x, dim=-1)
    ok = (tg >= 0) & (tg < W.shape[0])
    t = x.gather(1, torch.from_numpy(np.where(ok, tg, 0)).unsqueeze(1)).squeeze(1)
    return x, lse, lse - t


def _fp32_rows(H, W, tg):
    """The yardstick: the same quantity evaluated in fp32 on the CPU."""
    x = torch.from_numpy(H).float() @ torch.from_numpy(W).float().T
    lse = torch.logsumexp(x, dim=-1)
    t = x.gather(1, torch.from_numpy(tg).unsqueeze(1)).squeeze(1)
    return lse, lse - t


# ------------------------------------------------------------------------------------------------------ exact cases
EXACT = [  # (M, V, K, dtype): a cross of the edges, not the full product
    (1, 256, MIN_K, BF), (1, 1000, MIN_K + 128, BF), (1, 2049, 1024, FP),
    (255, 513, MIN_K, FP), (255, 2049, MIN_K + 128, FP), (255, 640, 1024, BF),
    (256, 640, MIN_K + 128, BF), (256, 256, 1024, FP), (256, 1000, MIN_K, BF),
    (257, 1000, MIN_K + 128, FP), (257, 2049, 1024, BF), (257, 513, MIN_K, BF),
    (600, 2049, MIN_K, BF), (600, 513, 1024, FP), (600, 640, MIN_K + 128, BF), (600, 1000, MIN_K, FP),
    (600, 256, MIN_K + 128, FP), (1, 513, MIN_K, FP), (1, 640, 1024, BF),
]


def _probe_columns(V):
    last_tile = (V - 1) // 256 * 256
    return sorted({v for v in (0, 31, 32, 63, 64, 255, 256, last_tile, V - 1) if v < V})


def _exact_inputs(M, V, K, seed):
    H = dense_ints((M, K), seed)
    W = dense_ints((V, K), seed + 1)
    rng = np.random.default_rng(seed + 2)
    tg = rng.integers(0, V, size=M).astype(np.int64)
    cols = _probe_columns(V)
    if M == 1:
        cols = [cols[seed % len(cols)]]               # one row, one planted column: the seed walks the list
    rows = [(j * M) // len(cols) for j in range(len(cols))] if M >= len(cols) else [0]
    probes = list(zip(rows, cols))
    for m, v in probes:
        W[v] = 3 * np.sign(H[m])
        tg[m] = v
    tie = None
    if M > 1 and V >= 4:
        # two equal columns in different lanes (and, where V allows, different tiles) dominate one more row: a tie
        m = (M // 2) | 1
        if m not in rows and m < M:
            W[1] = W[V - 2] = 3 * np.sign(H[m])
            tie = m
            tg[m] = V - 2
    return H, W, tg, probes, tie


@pytest.mark.parametrize("M,V,K,dtype", EXACT, ids=lambda v: str(v).replace("torch.", ""))
def test_exact_logits_targets_and_argmax(ops, dev, M, V, K, dtype):
    H, W, tg, probes, tie = _exact_inputs(M, V, K, 7 * M + V + K)
    assert_exactly_summable(9 * K, 0, "logits of +-{1,2,3} operands")
    x64, lse64, _ = _fp64_rows(H.astype(np.float64), W.astype(np.float64), tg)
    assert float(x64.abs().max()) <= 9 * K
    want_tgt = x64.gather(1, torch.from_numpy(tg).unsqueeze(1)).squeeze(1)
    want_arg = torch.from_numpy(np.argmax(x64.numpy(), axis=1))         # numpy: the first of equal maxima
    for m, v in probes:
        assert int(want_arg[m]) == v and float(x64[m, v]) >= 3 * K      # the planted column dominates its row
    if tie is not None:
        assert int(want_arg[tie]) == 1                                   # the lower of the two equal columns
    lse32, _ = _fp32_rows(H.astype(np.float64), W.astype(np.float64), tg)

    Hd = torch.from_numpy(H).to(dev, dtype)
    Wd = torch.from_numpy(W).to(dev, dtype)
    for tdt in (torch.int64, torch.int32):
        nll, lse, argmax, tgt = ops.lm_head_nll(Hd, Wd, torch.from_numpy(tg).to(dev, tdt), return_target_logit=True)
        torch.cuda.synchronize()
        assert_exact(tgt.cpu().view(1, -1), want_tgt.view(1, -1), what=f"tgt ({tdt})")
        assert_exact(argmax.cpu().view(1, -1), want_arg.view(1, -1), what=f"argmax ({tdt})")
        err = (lse.cpu().double() - lse64).abs()
        yard = (lse32.double() - lse64).abs()
        bar = max(MARGIN * float(yard.max()), 2.0 ** -23 * float(lse64.abs().max()))
        print(f"exact M={M} V={V} K={K}: lse max err {float(err.max()):.3e}, yardstick {float(yard.max()):.3e}")
        assert float(err.max()) <= bar, (float(err.max()), bar, int(err.argmax()))
        # nll is lse - tgt, one fp32 subtraction of the two outputs
        assert torch.equal(nll, lse - tgt)


# ---------------------------------------------------------------------------- row independence, determinism, targets
def _raw_call(lib, H, ldh, W, tg, M, outs, ws):
    from quantool_amd.hip import _lib

    K, V = W.shape[1], W.shape[0]
    code = _lib.QT_BF16 if W.dtype == BF else _lib.QT_F16
    return lib.qt_lm_head_nll(H.data_ptr(), ldh, W.data_ptr(), W.stride(0), code, M, K, V, tg.data_ptr(),
                              tg.element_size(), outs["nll"].data_ptr(), outs["lse"].data_ptr(), outs["tgt"].data_ptr(),
                              outs["argmax"].data_ptr(), ws.data_ptr(), ws.numel(),
                              torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
def test_a_row_depends_on_the_row_alone(ops, dev, dtype):
    from quantool_amd.hip import _lib

    lib = _lib.load()
    M, K, V, pad, extra = 600, MIN_K + 128, 1000, 72, 64
    g = torch.Generator().manual_seed(11)
    Hc = torch.randn(M, K, generator=g).to(dtype)
    W = (torch.randn(V, K, generator=g) * (3.0 / math.sqrt(K))).to(dtype).to(dev)
    tg = torch.randint(0, V, (M,), generator=g)
    places = (0, 255, 256, M - 1)
    for p in places:
        Hc[p] = Hc[0]
        tg[p] = tg[0]
    ignored, beyond = 3, 300
    tg[ignored], tg[beyond] = -100, V

    # the contiguous, aligned call through ops
    base = ops.lm_head_nll(Hc.to(dev), W, tg.to(dev), return_target_logit=True)
    # the row alone
    alone = ops.lm_head_nll(Hc[:1].to(dev), W, tg[:1].to(dev), return_target_logit=True)
    # a strided view (ldh > K) whose base lies 16 bytes behind a 256-byte boundary, outputs longer than M
    ldh = K + pad
    flat = torch.zeros(M * ldh + 256, dtype=dtype, device=dev)
    off = ((-flat.data_ptr()) % 256 + 16) // 2
    Hs = flat[off:off + M * ldh].view(M, ldh)[:, :K]
    Hs.copy_(Hc)
    assert Hs.data_ptr() % 256 == 16 and Hs.stride(0) == ldh
    sent_f, sent_i = -12345.5, -77
    outs = {n: torch.full((M + extra,), sent_f, dtype=torch.float32, device=dev) for n in ("nll", "lse", "tgt")}
    outs["argmax"] = torch.full((M + extra,), sent_i, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.qt_lm_head_nll_workspace_size(M, V), dtype=torch.uint8, device=dev)
    tgd = tg.to(dev)
    assert _raw_call(lib, Hs, ldh, W, tgd, M, outs, ws) == _lib.QT_OK, lib.qt_last_error()
    torch.cuda.synchronize()
    strided = (outs["nll"][:M], outs["lse"][:M], outs["argmax"][:M], outs["tgt"][:M])
    for n in ("nll", "lse", "tgt"):
        assert bool((outs[n][M:] == sent_f).all()), f"{n}: memory past M was written"
    assert bool((outs["argmax"][M:] == sent_i).all()), "argmax: memory past M was written"

    def bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t

    normal = torch.ones(M, dtype=torch.bool, device=dev)
    normal[beyond] = False                                               # NaN there: compared by bit pattern below
    for a, b, name in zip(base, strided, ("nll", "lse", "argmax", "tgt")):
        assert torch.equal(bits(a), bits(b)), f"{name}: the strided, shifted view differs from the contiguous call"
        row = bits(a)[list(places)]
        assert bool((row == row[0]).all()), f"{name}: the same row at {places} gives {a[list(places)].tolist()}"
        assert torch.equal(bits(a)[:1], bits(alone[["nll", "lse", "argmax", "tgt"].index(name)])), \
            f"{name}: the row alone (M = 1) differs from the row among {M}"
    # determinism: a second call
    again = ops.lm_head_nll(Hc.to(dev), W, tgd, return_target_logit=True)
    for a, b in zip(base, again):
        assert torch.equal(bits(a), bits(b))
    # the ignore index and a target past V
    nll, lse, argmax, tgt = base
    assert float(nll[ignored]) == 0.0 and float(tgt[ignored]) == 0.0
    assert math.isnan(float(nll[beyond])) and math.isnan(float(tgt[beyond]))
    x = Hc.double() @ W.cpu().double().T
    for m in (ignored, beyond):
        assert abs(float(lse[m]) - float(torch.logsumexp(x[m], 0))) < 1e-4
        assert int(argmax[m]) == int(np.argmax(x[m].numpy()))
    assert not bool(torch.isnan(nll[normal]).any())


def test_m_zero_touches_nothing(dev):
    from quantool_amd.hip import _lib

    lib = _lib.load()
    W = torch.zeros(256, MIN_K, dtype=BF, device=dev)
    H = torch.zeros(1, MIN_K, dtype=BF, device=dev)
    tg = torch.zeros(1, dtype=torch.int64, device=dev)
    outs = {n: torch.full((4,), 3.0, dtype=torch.float32, device=dev) for n in ("nll", "lse", "tgt")}
    outs["argmax"] = torch.full((4,), 3, dtype=torch.int32, device=dev)
    ws = torch.empty(16, dtype=torch.uint8, device=dev)
    assert lib.qt_lm_head_nll_workspace_size(0, 256) == 0
    assert _raw_call(lib, H, MIN_K, W, tg, 0, outs, ws) == _lib.QT_OK
    torch.cuda.synchronize()
    assert all(bool((t == 3).all()) for t in outs.values())


# -------------------------------------------------------------------------------------------------- the numeric bar
RANDOM = [(300, MIN_K, 513), (257, 384, 1000), (64, 1024, 2049)]


@pytest.mark.parametrize("dtype", [BF, FP], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,K,V", RANDOM)
def test_numeric_bar_on_random_inputs(ops, dev, M, K, V, dtype):
    """(a) max error <= 4x the fp32 CPU yardstick's; (b) max error <= 2 gamma_K max_v sum_k |h_k w_vk| + |lse| 2^-23;
    (c) mean error <= 1/16 of the mean error of nll_sum(F.linear(H, W), targets) on the GPU."""
    from quantool_amd.evaluate import nll_sum

    g = torch.Generator().manual_seed(1000 * M + K + V)
    H = torch.randn(M, K, generator=g).to(dtype)
    W = (torch.randn(V, K, generator=g) * (3.0 / math.sqrt(K))).to(dtype)
    tg = torch.randint(0, V, (M,), generator=g)
    Hn, Wn = H.double().numpy(), W.double().numpy()
    _, lse64, nll64 = _fp64_rows(Hn, Wn, tg.numpy())
    _, nll32 = _fp32_rows(Hn, Wn, tg.numpy())
    yard = (nll32.double() - nll64).abs()

    Hd, Wd, tgd = H.to(dev), W.to(dev), tg.to(dev)
    nll, lse, argmax = ops.lm_head_nll(Hd, Wd, tgd)
    err = (nll.cpu().double() - nll64).abs()

    # the "logits" arm, row by row: the body of nll_sum, whose sum it must reproduce
    logits = torch.nn.functional.linear(Hd, Wd)
    arm = -torch.log_softmax(logits.float(), dim=-1).gather(1, tgd.unsqueeze(1)).squeeze(1)
    assert abs(float(arm.double().sum()) - nll_sum(logits, tgd)) <= 1e-9 * M * 20
    arm_err = (arm.cpu().double() - nll64).abs()

    u = 2.0 ** -24
    gamma = K * u / (1 - K * u)
    cap = 2 * gamma * float((H.double().abs() @ W.double().abs().T).max()) + float(lse64.abs().max()) * 2.0 ** -23
    ratio = float(err.max()) / float(yard.max())
    print(f"random M={M} K={K} V={V} {dtype}: kernel max {float(err.max()):.3e} mean {float(err.mean()):.3e}; "
          f"yardstick max {float(yard.max()):.3e} mean {float(yard.mean()):.3e}; ratio {ratio:.2f}; cap {cap:.3e}; "
          f"logits arm mean {float(arm_err.mean()):.3e}")
    assert float(err.max()) <= MARGIN * float(yard.max()), ratio                        # (a)
    assert float(err.max()) <= cap                                                      # (b)
    assert float(err.mean()) <= float(arm_err.mean()) / 16                              # (c)
    x64 = torch.from_numpy(Hn) @ torch.from_numpy(Wn).T
    top = x64.gather(1, argmax.cpu().long().unsqueeze(1)).squeeze(1)
    # the fp32 maximum may sit on another column than the fp64 one only where the two logits are closer than the cap
    assert float((x64.max(dim=1).values - top).max()) <= cap
