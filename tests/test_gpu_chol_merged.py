"""The factor chain walked block row by row (``QT_CHOL_MERGE``; csrc/cholesky.hip ``chol_merge_mode``): ``order`` runs
the row walk with the separate long products and tables of ``0`` and must give its bits; ``1`` runs the two long
products of a row as the two segments of one gemm3 launch with one item table, which changes the cut of a tile's k
range and so the factor's low bits, not its accuracy.

K = 640 (512 + a ragged 128-row block: a one-tile segment 0 beside a two-tile triangular segment 1) and K = 1536 (three
block rows), the graded matrices of ``test_gpu_chol_f16x2`` from ``ops.hessian_prepare``, products forced on for every
step that has one, both plane modes (bounded: two fp16 planes; unbounded: three bf16 planes).

Bars: ``order`` equals ``0`` bit for bit; merged, max|U - U64| / max|U64| <= 2 x that of ``0`` on the same input and
<= max(4 x fp32 LAPACK three-step's, 5e-6) (``test_gpu_chol_f16x2``)."""
import numpy as np
import pytest
import torch

from .test_gpu_chol_f16x2 import _err, _force_products, case  # noqa: F401  (case: the module-scoped fixture)

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("bounded", [True, False], ids=["f16x2", "bf16x3"])


def _env(monkeypatch, merge):
    _force_products(monkeypatch)
    monkeypatch.setenv("QT_CHOL_MERGE", merge)


def _single(ops, A, lb):
    U, info = ops.cholesky_inverse_upper(A.clone(), min_eig_lb=lb)
    torch.cuda.synchronize()
    return U, int(info.item())


def _batch(ops, dev, mats, lbs):
    """Problems at padded strides in one chain of launches -> (U [n, K, K], info)."""
    n, K = len(mats), mats[0].shape[0]
    Abuf = torch.zeros((n, K * K + 256), dtype=torch.float32, device=dev)
    Ubuf = torch.zeros((n, K * K + 512), dtype=torch.float32, device=dev)
    A = Abuf[:, :K * K].view(n, K, K)
    U = Ubuf[:, :K * K].view(n, K, K)
    for b, m in enumerate(mats):
        A[b].copy_(m)
    info = ops.cholesky_inverse_upper_batched(A, U, min_eig_lb=None if lbs is None else torch.cat(lbs).contiguous())
    torch.cuda.synchronize()
    return U, info.cpu().numpy()


@MODES
def test_order_is_bit_identical_to_two_phases(case, ops, monkeypatch, bounded):
    lb = case["lb"] if bounded else None
    _env(monkeypatch, "0")
    U0, i0 = _single(ops, case["A"], lb)
    _env(monkeypatch, "order")
    U1, i1 = _single(ops, case["A"], lb)
    assert i0 == 0 and i1 == 0
    assert torch.equal(U0, U1)
    # a failed pivot is found at the same place and ends the same way
    bad = case["A"].clone()
    j = case["K"] - 70
    bad[j, j] = -1.0
    _env(monkeypatch, "0")
    Ub0, ib0 = _single(ops, bad, lb)
    _env(monkeypatch, "order")
    Ub1, ib1 = _single(ops, bad, lb)
    assert ib0 == j + 1 and ib1 == ib0 and torch.equal(Ub0, Ub1)


@MODES
def test_merged_factor_vs_fp64(case, ops, monkeypatch, bounded):
    lb = case["lb"] if bounded else None
    _env(monkeypatch, "0")
    U0, i0 = _single(ops, case["A"], lb)
    _env(monkeypatch, "1")
    U1, i1 = _single(ops, case["A"], lb)
    U2, i2 = _single(ops, case["A"], lb)
    assert i0 == 0 and i1 == 0 and i2 == 0
    assert torch.equal(U1, U2), "a rerun must give the same bits"
    assert bool((torch.tril(U1, -1) == 0).all())
    assert not torch.equal(U0, U1), "the merged products were not taken"
    e0, e1 = _err(U0.cpu().numpy(), case["truth"]), _err(U1.cpu().numpy(), case["truth"])
    e_lap = _err(case["U_lapack"], case["truth"])
    print(f"\n[merged] K={case['K']} {'f16x2' if bounded else 'bf16x3'}: max err / max|U| vs fp64: two phases {e0:.3e}, "
          f"merged {e1:.3e}, fp32 LAPACK three-step {e_lap:.3e}")
    assert e1 <= 2 * e0, (e1, e0)
    assert e1 <= max(4 * e_lap, 5e-6), (e1, e_lap)


@MODES
def test_merged_batch_equals_singles_bit_for_bit(case, ops, dev, monkeypatch, bounded):
    """Three problems with different scale exponents (A, 64 A, A / 1024)."""
    _env(monkeypatch, "1")
    fac = [1.0, 64.0, 1.0 / 1024.0]
    mats = [case["A"] * f for f in fac]
    lbs = [case["lb"] * f for f in fac] if bounded else None
    U, info = _batch(ops, dev, mats, lbs)
    assert (info == 0).all()
    for b in range(3):
        Us, i_s = _single(ops, mats[b], lbs[b] if bounded else None)
        assert i_s == 0 and torch.equal(U[b], Us), f"problem {b}"


@MODES
def test_merged_non_pd_problem_in_a_batch(case, ops, dev, monkeypatch, bounded):
    _env(monkeypatch, "1")
    K = case["K"]
    bad = case["A"].clone()
    j = K // 3
    bad[j, j] = -1.0
    mats = [case["A"], bad, case["A"] * 4.0]
    lbs = [case["lb"], case["lb"], case["lb"] * 4.0] if bounded else None
    U, info = _batch(ops, dev, mats, lbs)
    assert info[0] == 0 and info[2] == 0 and info[1] == j + 1
    assert torch.equal(U[1], torch.eye(K, dtype=torch.float32, device=dev))
    for b in (0, 2):
        Us, _ = _single(ops, mats[b], lbs[b] if bounded else None)
        assert torch.equal(U[b], Us), f"neighbour {b}"
        assert bool(torch.isfinite(U[b]).all())


@MODES
def test_merged_ignores_a_nan_poisoned_strict_lower_triangle(case, ops, monkeypatch, bounded):
    _env(monkeypatch, "1")
    lb = case["lb"] if bounded else None
    U0, info0 = _single(ops, case["A"], lb)
    poison = torch.full_like(case["A"], float("nan"))
    poison[::3] = float("inf")
    U1, info1 = _single(ops, torch.triu(case["A"]) + torch.tril(poison, -1), lb)
    assert info0 == 0 and info1 == 0
    assert torch.equal(U0, U1)


@MODES
@pytest.mark.parametrize("n", [1, 2])
def test_merged_stays_inside_the_workspace(case, ops, dev, monkeypatch, bounded, n):
    """Exactly ``*_workspace_bytes()`` between two guards: the merged chain writes nothing outside it, refuses a
    workspace one byte short, and gives the bits of the call through ``ops`` (``test_gpu_workspace_contract``).  The
    size does not depend on the switch."""
    from quantool_amd.hip import _lib

    from .test_gpu_workspace_contract import BF16X3_CHAIN, Case, _run, _stream

    K = case["K"]
    fac = [1.0, 16.0][:n]
    _force_products(monkeypatch)
    sizes = []
    for merge in ("0", "order", "1"):
        monkeypatch.setenv("QT_CHOL_MERGE", merge)
        sizes.append(int(_lib.load().qt_cholesky_inverse_upper_batched_workspace_bytes(K, n)))
    assert sizes[0] == sizes[1] == sizes[2]

    def make(dev_):
        return dict(A=torch.stack([case["A"] * f for f in fac]), U=torch.zeros((n, K, K), dtype=torch.float32, device=dev_),
                    info=torch.full((n,), 7, dtype=torch.int32, device=dev_),
                    lb=torch.cat([case["lb"] * f for f in fac]).contiguous())

    def via_ops(ops_, t):
        t["info"] = ops_.cholesky_inverse_upper_batched(t["A"], t["U"], min_eig_lb=t["lb"] if bounded else None)

    def call(lib, t, ws, nb):
        if bounded:
            return lib.qt_cholesky_inverse_upper_batched_bounded(
                t["A"].data_ptr(), K * K, K, t["U"].data_ptr(), K * K, t["info"].data_ptr(), n, t["lb"].data_ptr(), ws, nb,
                _stream())
        return lib.qt_cholesky_inverse_upper_batched(
            t["A"].data_ptr(), K * K, K, t["U"].data_ptr(), K * K, t["info"].data_ptr(), n, ws, nb, _stream())

    entry = Case(f"merged qt_cholesky_inverse_upper_batched K={K} n={n}", "row walk, one launch per row", make,
                 lambda lib, t: lib.qt_cholesky_inverse_upper_batched_workspace_bytes(K, n), call, via_ops, ["U", "info"],
                 dict(BF16X3_CHAIN, QT_CHOL_MERGE="1"))
    _run(entry, dev, ops, monkeypatch, 0)
