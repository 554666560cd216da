"""The fused sweep (``sweep_fused_kernel``: a batch's block steps and near updates in one launch, beside the far
update of the batch before it) against the chain of launches it replaces (``QT_SWEEP_FUSED=0``): the levels, the
updated ``W`` and the loss must be equal bit for bit -- no tolerance, no excluded elements.

Shapes are the smallest that reach each seam: two batches with an empty ``far_rest``; a ``far_rest`` beside a batch
and an odd last batch; a full 8-block batch; and the shapes that must take the chain of launches either way (a ragged
last block, rows off the 128-row tiles).  Both lane counts of the row workgroups are run where the fused form applies.

The two forms give equal bits by contract, so equal bits do not say which form ran: a sweep that fell back to the chain
would be compared with itself.  ``sweep_launches`` is the witness: the library's profiling marks count one pair per
block-kernel launch, ``ceil(K / (128 batch))`` fused and ``ceil(K / 128)`` as a chain, and every case with two or more
blocks per batch asserts the count of the form it names.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SWEEP_ENV = ("QT_SWEEP_FUSED", "QT_SWEEP_LANES", "QT_SWEEP_BLOCK", "QT_SWEEP_BATCH", "QT_SWEEP_FAR", "QT_SGEMM_RING",
             "QT_SGEMM_RING_MIN_TILES")


@pytest.fixture(autouse=True)
def _default_sweep_form(monkeypatch):
    for name in SWEEP_ENV:
        monkeypatch.delenv(name, raising=False)


QT_PROF_SWEEP_BLOCK = 1      # include/quantool_amd.h, enum qt_prof_kernel


def sweep_launches(run):
    """``run()`` with the library's profiling marks on: (what it returned, block-kernel launches it made).  ``sweep_run``
    marks one pair per launch of a block kernel: ``fused_launches`` of them in the fused form, ``chain_launches`` as a
    chain of launches.  The two differ whenever a batch has two or more blocks and K > 128."""
    from quantool_amd.hip._lib import QT_OK, load

    lib = load()
    ms, n = ctypes.c_double(), ctypes.c_int64(-1)
    assert lib.qt_profile_enable(1) == QT_OK
    try:
        out = run()
        torch.cuda.synchronize()
        assert lib.qt_profile_read(QT_PROF_SWEEP_BLOCK, ctypes.byref(ms), ctypes.byref(n)) == QT_OK
    finally:
        lib.qt_profile_enable(0)
    return out, int(n.value)


def default_batch(K):
    return 8 if K >= 8192 else 4      # sweep_batch_blocks (sweep.hip) with QT_SWEEP_BATCH unset


def fused_launches(K, batch):
    return -(-K // (128 * batch))


def chain_launches(K):
    return -(-K // 128)


def expected_launches(form, K, batch):
    """``form``: "fused" or "chain".  None where one block per batch makes the two counts equal."""
    if batch < 2 or K <= 128:
        return None
    return {"fused": fused_launches(K, batch), "chain": chain_launches(K)}[form]


_FACTORS = {}


def _factor(K, seed):
    """Upper U with U^T U = (X^T X / n + damp)^-1 for a small random X: well conditioned, computed in fp64."""
    if (K, seed) not in _FACTORS:
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((2 * K, K))
        H = X.T @ X / (2 * K)
        H += 0.05 * np.mean(np.diag(H)) * np.eye(K)
        L = np.linalg.cholesky(np.linalg.inv(H))
        _FACTORS[(K, seed)] = np.ascontiguousarray(L.T).astype(np.float32)
    return _FACTORS[(K, seed)]


def _inputs(R, K, bits, sym, seed, n_factors=1):
    rng = np.random.default_rng(seed)
    W = rng.standard_normal((R, K)).astype(np.float32)
    gs = 64 if K % 64 == 0 else K
    G = K // gs
    g_idx = np.stack([(np.arange(K) // gs).astype(np.int32)[rng.permutation(K)] for _ in range(n_factors)])
    U = np.stack([_factor(K, seed + 7 * (g + 1)) for g in range(n_factors)])
    # min-max parameters per (row, group) over arbitrary columns: any positive scale and in-range zero point do
    lo, hi = W.min(axis=1, keepdims=True) * rng.uniform(0.5, 1.0, (R, G)), W.max(axis=1, keepdims=True) * rng.uniform(0.5, 1.0, (R, G))
    qmin, qmax = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    if sym:
        scale = (np.maximum(-lo, hi) / qmax).astype(np.float32)
        zp = np.zeros_like(scale)
    else:
        scale = ((hi - lo) / (qmax - qmin)).astype(np.float32)
        zp = np.clip(np.rint(qmin - lo / scale), qmin, qmax).astype(np.float32)
        assert np.any(zp != 0)
    return dict(W=W, U=U, g_idx=g_idx, scale_t=np.ascontiguousarray(scale.T), zp_t=np.ascontiguousarray(zp.T), bits=bits)


def _run(ops, dev, c, row_end=None):
    W = torch.from_numpy(c["W"].copy()).to(dev)
    U = torch.from_numpy(c["U"]).to(dev)
    s, z = torch.from_numpy(c["scale_t"]).to(dev), torch.from_numpy(c["zp_t"]).to(dev)
    g = torch.from_numpy(c["g_idx"]).to(dev)
    if row_end is None:
        Qt, loss = ops.gptq_sweep(W, U[0], s, z, g[0].contiguous(), 128, c["bits"])
    else:
        Qt, loss = ops.gptq_sweep_grouped(W, U, row_end, s, z, g, 128, c["bits"])
    torch.cuda.synchronize()
    return Qt.cpu().numpy(), W.cpu().numpy(), loss.cpu().numpy()


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _both_forms(ops, dev, monkeypatch, cases, batch, lanes, row_end=None, fused=None, form="fused"):
    """Every case of ``cases`` in order under each form, on one stream; the outputs must agree bit for bit.  ``form``:
    what the second run must be, "fused" or (a shape off whole tiles) "chain"; the first is the chain.  Both are held to
    their launch counts wherever the counts can tell them apart (``expected_launches``)."""
    K = cases[0]["W"].shape[1]
    monkeypatch.setenv("QT_SWEEP_BATCH", str(batch))
    monkeypatch.setenv("QT_SWEEP_FUSED", "0")
    want, n_want = sweep_launches(lambda: [_run(ops, dev, c, row_end) for c in cases])
    monkeypatch.delenv("QT_SWEEP_FUSED")
    if fused is not None:
        monkeypatch.setenv("QT_SWEEP_FUSED", fused)
    if lanes is not None:
        monkeypatch.setenv("QT_SWEEP_LANES", str(lanes))
    got, n_got = sweep_launches(lambda: [_run(ops, dev, c, row_end) for c in cases])
    assert n_want == len(cases) * chain_launches(K), (n_want, "QT_SWEEP_FUSED=0 did not run the chain of launches")
    if expected_launches(form, K, batch) is not None:
        assert n_got == len(cases) * expected_launches(form, K, batch), (n_got, f"the second run was not the {form} form")
    for (q0, w0, l0), (q1, w1, l1) in zip(want, got):
        assert _bits_equal(q0, q1), f"{(q0 != q1).sum()} of {q0.size} levels differ"
        assert _bits_equal(w0, w1), f"{(w0.view(np.uint32) != w1.view(np.uint32)).sum()} of {w0.size} weights differ"
        assert _bits_equal(l0, l1), f"{(l0.view(np.uint32) != l1.view(np.uint32)).sum()} of {l0.size} losses differ"
        assert np.isfinite(w1).all() and np.isfinite(l1).all() and np.any(q1 != 0)


# R, K, QT_SWEEP_BATCH, bits, symmetric
SEAMS = [
    (128, 256, 1, 4, True),       # two batches; far_near with k = 128; empty far_rest
    (256, 768, 2, 4, False),      # non-empty far_rest beside a batch; an odd number of blocks in the last batch
    (128, 1152, 8, 8, False),     # a full 8-block batch plus a 1-block batch; near updates 896 columns wide
    (128, 1100, 4, 4, True),      # ragged last block of 76 columns
    (200, 512, 2, 4, False),      # rows not a multiple of 128
    (32, 512, 2, 4, True),        # fewer rows than one 128-row tile
]
# the last three are off whole tiles: the chain of launches either way.  (128, 256) has one block per batch, as many
# launches fused as chained: the launch count cannot witness its form.
OFF_WHOLE_TILES = {(128, 1100), (200, 512), (32, 512)}


@pytest.mark.parametrize("lanes", [None, 8, 16])
@pytest.mark.parametrize("R,K,batch,bits,sym", SEAMS)
def test_fused_equals_the_chain_of_launches(ops, dev, monkeypatch, R, K, batch, bits, sym, lanes):
    _both_forms(ops, dev, monkeypatch, [_inputs(R, K, bits, sym, seed=R + K + bits)], batch, lanes,
                form="chain" if (R, K) in OFF_WHOLE_TILES else "fused")


# K of each stack, by its rows.  K = 768 with two blocks per batch is three batches: far_rest(0), beside batch 1, is 256
# columns wide and takes each tile's B operand from its row group's factor (set_groups -> group_bsB in the shared launch)
STACK_K = {448: 512, 512: 512, 384: 768, 896: 768}


@pytest.mark.parametrize("lanes", [None, 8, 16])
@pytest.mark.parametrize("R,row_end", [(448, [128, 384, 448]), (512, [128, 384, 512]), (384, [128, 384]),
                                       (896, [128, 384, 512, 768, 896])])
def test_stacked_sweep(ops, dev, monkeypatch, R, row_end, lanes):
    """Factors stacked; (128, 384, 448) ends in a group of 64 rows (the chain of launches either way), (128, 384, 512)
    is the same stack on whole 128-row tiles (fused; two batches, so no far update shares a launch); two and five
    factors at K = 768 are fused with a non-empty ``far_rest``."""
    K = STACK_K[R]
    _both_forms(ops, dev, monkeypatch, [_inputs(R, K, 4, False, seed=R, n_factors=len(row_end))], 2, lanes, row_end,
                form="chain" if R % 128 else "fused")


@pytest.mark.parametrize("lanes", [8, 16])
def test_two_datasets_back_to_back(ops, dev, monkeypatch, lanes):
    """A second sweep on the same stream and workspace right behind the first: a far update that read the wrong one
    of the two error buffers, or one left over from the first sweep, changes the second's bits."""
    cases = [_inputs(256, 768, 4, False, seed=11), _inputs(256, 768, 4, True, seed=12)]
    _both_forms(ops, dev, monkeypatch, cases, 2, lanes)


@pytest.mark.parametrize("fused", [None, "1"])
def test_above_the_height_threshold(ops, dev, monkeypatch, fused):
    """Above 6144 rows the default is the chain of launches; ``QT_SWEEP_FUSED=1`` takes the fused form there, with
    more row workgroups (260) than a far update is ever given.  (One block per batch: the launch count is three either
    way and cannot witness the form; ``test_gpu_sweep_fused_oracle.py`` runs this height with two blocks per batch.)"""
    _both_forms(ops, dev, monkeypatch, [_inputs(8320, 384, 4, False, seed=5)], 1, None, fused=fused)
