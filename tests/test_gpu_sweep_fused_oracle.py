"""The fused sweep (``sweep_fused_kernel``, csrc/sweep.hip) against ``oracle/gptq_oracle.c``: its own quantise step
(``col_step`` on ``TriLayout``, 8 or 16 lanes per row), its own near update and the far update that shares its launch
(``sgemm_ring_body<true>``), over what the entry points accept on whole 128-tiles -- the shapes the default takes the
fused form at.  ``test_gpu_sweep_matrix.py`` sits off whole tiles and holds the chain of launches to the same oracle.

Bars (those of ``test_gpu_sweep_matrix.py``, whose ``_case`` / ``_check`` are used): levels and
dequantised W bit-exact, loss to 1e-6.  Every GPU case runs with ``QT_SWEEP_LANES`` unset, 8 and 16, has two or more
blocks per batch, and asserts by its count of block-kernel launches that the fused form ran
(``test_gpu_sweep_fused.py::sweep_launches``).

What the oracle's side of a case must hold -- both clamp ends reached at 2 and 8 bits, the ``F32_EPS`` scale, the dead
flags, more far tiles than far workgroups -- needs no GPU and is asserted by the tests without the ``gpu`` mark, on the
same cached cases.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_sweep_fused import SWEEP_ENV, _bits_equal, chain_launches, default_batch, fused_launches, sweep_launches
from tests.test_gpu_sweep_matrix import (WIDTH_SCHEME, _assert_oracle_hits_the_clamp, _case, _check, _check_grouped, _factor,
                                         _grouped_case, _permuted_g_idx)
from tests.util import synth_weight

gpu = pytest.mark.gpu
LANES = [None, 8, 16]


@pytest.fixture(autouse=True)
def _default_sweep_form(monkeypatch):
    for name in SWEEP_ENV:
        monkeypatch.delenv(name, raising=False)


def _check_fused(ops, dev, monkeypatch, c, lanes, batch=None):
    """``_check`` on the case with ``lanes`` lanes per row and ``batch`` blocks per batch (None: the defaults); the
    launch count must be the fused form's."""
    if lanes is not None:
        monkeypatch.setenv("QT_SWEEP_LANES", str(lanes))
    if batch is not None:
        monkeypatch.setenv("QT_SWEEP_BATCH", str(batch))
    out, launches = sweep_launches(lambda: _check(ops, dev, c))
    batch = default_batch(c["K"]) if batch is None else batch
    assert batch >= 2 and launches == fused_launches(c["K"], batch) != chain_launches(c["K"]), launches
    return out


def _has_far_rest(K, batch):
    """Whether a far update shares a launch: columns are left right of batch 1."""
    return K > 2 * 128 * (batch or default_batch(K))


# ------------------------------------------------------------------------------------ a. width x scheme
# R = 128, K = 1152: nine blocks, three batches at the default batch of 4, so batch 1 has a far_rest beside it.  The
# default seed (R + K + bits) reaches both ends of the range at 2 and 8 bits in every scheme (the test below).
@functools.lru_cache(maxsize=None)
def _width_case(oracle, bits, sym, gs):
    return _case(oracle, 128, 1152, gs, sym, bits)


@pytest.mark.parametrize("bits,sym,gs", WIDTH_SCHEME)
def test_width_and_scheme_cases_reach_the_clamp(oracle, bits, sym, gs):
    c = _width_case(oracle, bits, sym, gs)
    assert c["R"] % 128 == 0 and c["K"] % 128 == 0 and _has_far_rest(c["K"], None)
    if bits in (2, 8):
        _assert_oracle_hits_the_clamp(c)


@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("bits,sym,gs", WIDTH_SCHEME)
def test_width_and_scheme(ops, oracle, dev, monkeypatch, bits, sym, gs, lanes):
    _check_fused(ops, dev, monkeypatch, _width_case(oracle, bits, sym, gs), lanes)


# ------------------------------------------------------------------------------------ b. batch length
BATCH_K = [1152, 2304]
BATCH_SCHEME = [(4, True), (8, False)]


@functools.lru_cache(maxsize=None)
def _batch_case(oracle, K, bits, sym):
    return _case(oracle, 256, K, 128, sym, bits)


@pytest.mark.parametrize("bits,sym", BATCH_SCHEME)
@pytest.mark.parametrize("K", BATCH_K)
def test_batch_length_cases_reach_the_clamp(oracle, K, bits, sym):
    c = _batch_case(oracle, K, bits, sym)
    if bits == 8:
        _assert_oracle_hits_the_clamp(c)
    assert [_has_far_rest(K, b) for b in (2, 3, 8)] == [True, True, K == 2304]


@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("batch", [2, 3, 8])
@pytest.mark.parametrize("bits,sym", BATCH_SCHEME)
@pytest.mark.parametrize("K", BATCH_K)
def test_batch_length(ops, oracle, dev, monkeypatch, K, bits, sym, batch, lanes):
    """``QT_SWEEP_BATCH`` 2, 3 and 8 at nine and eighteen blocks: last batches of one, two, three and full length; with
    8 the two error buffers lie beyond the room the chain of launches asks for, and at K = 2304 the far update of an
    8-block batch (eight chains per tile) shares the launch of the next."""
    _check_fused(ops, dev, monkeypatch, _batch_case(oracle, K, bits, sym), lanes, batch)


# ------------------------------------------------------------------------------------ c. dead columns
DEAD = (300, 1100)            # 1100: in the last block
ZERO_ROWS, ZERO_GROUP = 9, 7
DEAD_SCHEME = [(4, True), (8, False), (4, False)]


@functools.lru_cache(maxsize=None)
def _dead_case(oracle, bits, sym):
    # (_case asserts the factor's dead flags and the F32_EPS scales of the zeroed group)
    return _case(oracle, 128, 1152, 64, sym, bits, dead=DEAD, zero_group=(np.arange(ZERO_ROWS), ZERO_GROUP))


@pytest.mark.parametrize("bits,sym", DEAD_SCHEME)
def test_dead_column_cases_hold_their_preconditions(oracle, bits, sym):
    c = _dead_case(oracle, bits, sym)
    assert np.all(c["scale"][:ZERO_ROWS, ZERO_GROUP] == oracle.F32_EPS) and np.all(c["scale"][ZERO_ROWS:] > oracle.F32_EPS)
    assert np.all(c["W"][:, list(DEAD)] == 0) and np.all(c["U"][list(DEAD), list(DEAD)] != 0)
    for d in DEAD:      # the oracle itself answers with the level of 0.0
        np.testing.assert_array_equal(c["Qo"][:, d].astype(np.float32), c["zp"][:, c["g_idx"][d]])
    if bits == 8:
        _assert_oracle_hits_the_clamp(c)


@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("bits,sym", DEAD_SCHEME)
def test_dead_columns_and_an_all_zero_group(ops, oracle, dev, monkeypatch, bits, sym, lanes):
    """``test_gpu_sweep_matrix.py``'s case of the same name on whole tiles: two activation columns that never fire (one
    in the last block), W zeroed there, and one group of the first rows all zero (scale at the ``F32_EPS`` floor)."""
    c = _dead_case(oracle, bits, sym)
    q, w = _check_fused(ops, dev, monkeypatch, c, lanes)
    for d in DEAD:
        g = c["g_idx"][d]
        np.testing.assert_array_equal(q[:, d].astype(np.float32), c["zp"][:, g])
        np.testing.assert_array_equal(w[:, d], (q[:, d].astype(np.float32) - c["zp"][:, g]) * c["scale"][:, g])
        assert np.all(w[:, d] == 0)


# ------------------------------------------------------------------------------------ d. the grouped entry point
def _fused_rows(n):
    return tuple(np.cumsum([128 if g % 2 == 0 else 256 for g in range(n)]).tolist())      # ends 128, 384, 512, 768, ...


# K, QT_SWEEP_BATCH.  768 in batches of two blocks: three batches, far_rest(0) is 256 columns wide and every one of its
# tiles takes its B operand from its row group's factor (set_groups -> group_bsB inside the shared launch).
# 640 at the default batch of 4: a batch of one block behind a full one, no far_rest.
GROUPED_K = [(768, 2), (640, None)]
GROUPED_FAR_REST = {768: True, 640: False}
GROUPED_N = [2, 5, 16]          # 16: SG_MAX_GROUPS
GROUPED_SCHEME = [(4, True), (8, False)]


@pytest.mark.parametrize("bits,sym", GROUPED_SCHEME)
@pytest.mark.parametrize("K,batch", GROUPED_K)
@pytest.mark.parametrize("n", GROUPED_N)
def test_grouped_cases_reach_the_clamp(oracle, n, K, batch, bits, sym):
    c = _grouped_case(oracle, _fused_rows(n), K, bits, sym)      # asserts every group's clamp ends at 8 bits
    assert all(r % 128 == 0 for r in c["row_end"]) and K % 128 == 0
    assert _has_far_rest(K, batch) == GROUPED_FAR_REST[K]


@gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("bits,sym", GROUPED_SCHEME)
@pytest.mark.parametrize("K,batch", GROUPED_K)
@pytest.mark.parametrize("n", GROUPED_N)
def test_grouped_sweep_each_group_against_the_oracle(ops, oracle, dev, monkeypatch, n, K, batch, bits, sym, lanes):
    """``qt_gptq_sweep_grouped`` in the fused form: every ``row_end`` a multiple of 128 (groups of 128 and 256 rows in
    turn), per-group factors in a NaN-filled buffer of stride K * K + 256, per-group permuted ``g_idx``; each group's
    rows against ``gptq_sweep_c`` on that group alone, the gaps still NaN."""
    if lanes is not None:
        monkeypatch.setenv("QT_SWEEP_LANES", str(lanes))
    if batch is not None:
        monkeypatch.setenv("QT_SWEEP_BATCH", str(batch))
    c = _grouped_case(oracle, _fused_rows(n), K, bits, sym)
    _, launches = sweep_launches(lambda: _check_grouped(ops, dev, c))
    assert launches == fused_launches(K, batch or default_batch(K)) != chain_launches(K), launches


# ------------------------------------------------------------------------------------ e. far workgroups with two tiles
# R, K, QT_SWEEP_BATCH, QT_SWEEP_FUSED
FAR_WALKS = [
    (6144, 1408, 2, None),       # 192 row workgroups leave room for 320 far ones; far_rest(0) has 48 x 7 = 336 tiles
    (8320, 1024, 2, "1"),        # 260 row workgroups (> 256): room is 256; far_rest(0) has 65 x 4 = 260 tiles
]


def _far_walk(R, K, batch, lanes=16):
    """The launch of batch 1 as ``sweep_run`` shapes it: row workgroups, the far workgroups it may add (two workgroups
    on each of 256 CUs, less the row workgroups, at least one per CU) and the 128 x 128 tiles of far_rest(0)."""
    span = 128 * batch
    n_row_wgs = R // (512 // lanes)
    room = max(512 - n_row_wgs, 256)
    tiles_m, tiles_n = R // 128, (K - 2 * span) // 128
    return dict(n_row_wgs=n_row_wgs, room=room, tiles_m=tiles_m, tiles_n=tiles_n, n_tiles=tiles_m * tiles_n)


def _assert_second_tiles(geo):
    """More tiles than far workgroups, so workgroup w also walks tile w + room; tile t is (t / tiles_n, t % tiles_n),
    so the second tiles are the bottom rows of W, and the last 128 rows hold nothing else."""
    assert geo["tiles_n"] > 0 and geo["room"] < geo["n_tiles"] <= 2 * geo["room"], geo
    assert (geo["tiles_m"] - 1) * geo["tiles_n"] >= geo["room"], geo


@pytest.mark.parametrize("R,K,batch,fused", FAR_WALKS)
def test_far_walk_shapes_have_more_tiles_than_workgroups(R, K, batch, fused):
    geo = _far_walk(R, K, batch)
    _assert_second_tiles(geo)
    assert (R > 6144) == (fused == "1") and R % 128 == 0 and K % 128 == 0      # the default above 6144 rows is the chain
    assert (geo["n_row_wgs"] > 256) == (R == 8320)                            # both branches of room


def _sweep(ops, dev, c):
    W = torch.from_numpy(c["W"].copy()).to(dev)
    Qt, loss = ops.gptq_sweep(W, torch.from_numpy(c["U"]).to(dev), torch.from_numpy(np.ascontiguousarray(c["scale"].T)).to(dev),
                              torch.from_numpy(np.ascontiguousarray(c["zp"].T)).to(dev), torch.from_numpy(c["g_idx"]).to(dev),
                              128, c["bits"])
    torch.cuda.synchronize()
    return Qt.cpu().numpy().T, W.cpu().numpy(), loss.cpu().numpy()


@gpu
@pytest.mark.parametrize("R,K,batch,fused", FAR_WALKS)
def test_far_workgroups_walk_a_second_tile(ops, oracle, dev, monkeypatch, R, K, batch, fused):
    """All rows bit for bit against the chain of launches; the first, a middle and the last 128 rows (rows are
    independent given U) against the oracle.  The last 128 rows are tiles that a far workgroup walks second."""
    _assert_second_tiles(_far_walk(R, K, batch))
    bits, sym, gs, seed = 4, False, 128, R + K
    c = dict(W=synth_weight(R, K, seed=seed), U=_factor(oracle, K, seed + 1)[0], g_idx=_permuted_g_idx(K, gs, seed), bits=bits)
    c["scale"], c["zp"] = oracle.minmax_qparams(c["W"], gs, sym, bits)
    monkeypatch.setenv("QT_SWEEP_BATCH", str(batch))
    monkeypatch.setenv("QT_SWEEP_FUSED", "0")
    (q0, w0, l0), launches = sweep_launches(lambda: _sweep(ops, dev, c))
    assert launches == chain_launches(K)
    monkeypatch.delenv("QT_SWEEP_FUSED")
    if fused is not None:
        monkeypatch.setenv("QT_SWEEP_FUSED", fused)
    (q1, w1, l1), launches = sweep_launches(lambda: _sweep(ops, dev, c))
    assert launches == fused_launches(K, batch)
    assert _bits_equal(q0, q1), f"{(q0 != q1).sum()} of {q0.size} levels differ; rows {np.flatnonzero((q0 != q1).any(axis=1))}"
    assert _bits_equal(w0, w1), f"rows {np.flatnonzero((w0.view(np.uint32) != w1.view(np.uint32)).any(axis=1))} of W differ"
    assert _bits_equal(l0, l1)
    mid = R // 256 * 128
    for r0 in (0, mid, R - 128):
        rows = slice(r0, r0 + 128)
        Qo, Wo, lo = oracle.gptq_sweep_c(c["W"][rows], c["U"], c["scale"][rows], c["zp"][rows], c["g_idx"], 128, bits)
        assert np.array_equal(q1[rows], Qo), f"rows {r0}..: {(q1[rows] != Qo).sum()} of {Qo.size} levels differ"
        np.testing.assert_array_equal(w1[rows], Wo, err_msg=f"rows {r0}..")
        np.testing.assert_allclose(l1[rows], lo, rtol=1e-6, err_msg=f"rows {r0}..")
