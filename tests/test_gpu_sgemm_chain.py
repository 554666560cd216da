"""qt_sgemm_tn_f32 against the CPU fmaf chain over EVERY output element, on every path of qt_sgemm_tn.

The reference is oracle/gptq_oracle.c: orc_sgemm_tn_chain (tests/test_sgemm_oracle.py holds it to libm's fmaf and shows
that the inputs below tell an ascending chain from a wrong order) -- never another device kernel.  Every case of
tests/sgemm_cases.py runs in each of its modes, once on randn operands and once on exact integers whose fp64 product
pins WHICH products are added independently of that function.  The whole output must equal the reference as numbers
(np.array_equal: the sign of a zero is not pinned); there is no tolerance anywhere.  Cin and out are column slices of
wider NaN-filled matrices (ldc > N) whose NaNs must survive; mode 0 also runs twice in place (out = Cin), and so does
the reference.  Before it launches, a case asserts on the reference side that its call lands on the path it is listed
for (Case.check_plan): kernel, tile count, k-steps, operand alignment, chunk list."""
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import sgemm_cases as sc
from tests.exact_inputs import assert_exactly_summable

pytestmark = pytest.mark.gpu

LEFT, RIGHT = 3, 2          # sentinel columns around a C slice: ldc = N + 5, the slice starts 12 bytes into a row


@pytest.fixture(scope="module")
def ops(dev):
    from quantool_amd.hip import ops as _ops

    return _ops


def wide(dev, M, N, values=None):
    """-> (W, S): W [M, LEFT + N + RIGHT] on the device, all NaN; S = W[:, LEFT:LEFT + N], holding `values` if given."""
    W = torch.full((M, LEFT + N + RIGHT), float("nan"), dtype=torch.float32, device=dev)
    S = W[:, LEFT:LEFT + N]
    if values is not None:
        S.copy_(torch.from_numpy(np.ascontiguousarray(values)))
    return W, S


def place(case, A, B, dev):
    """A and B on the device in the layout the case asks for: A `a_offset` floats into its allocation, B the first N
    columns of a [k, N + b_pad] matrix."""
    k, M = A.shape
    N = B.shape[1]
    abuf = torch.empty(k * M + case.a_offset, dtype=torch.float32, device=dev)
    dA = abuf[case.a_offset:].view(k, M)
    dA.copy_(torch.from_numpy(A))
    Bw = torch.full((k, N + case.b_pad), float("nan"), dtype=torch.float32, device=dev)
    dB = Bw[:, :N]
    dB.copy_(torch.from_numpy(B))
    return dA, dB


def assert_whole_output(W, want, tile, what):
    """The slice of W equals `want` in every element, and every sentinel column still holds its NaNs."""
    h = W.cpu().numpy()
    N = want.shape[1]
    assert np.isnan(h[:, :LEFT]).all() and np.isnan(h[:, LEFT + N:]).all(), f"{what}: a sentinel beside the slice was written"
    got = h[:, LEFT:LEFT + N].astype(np.float64)
    bad = got != np.asarray(want, dtype=np.float64)               # NaN (never written, or a sentinel read) != anything
    if bad.any():
        idx = np.argwhere(bad)
        m, n = (int(v) for v in idx[0])
        tiles = sorted({(int(a), int(b)) for a, b in idx // tile})
        raise AssertionError(f"{what}: {len(idx)} of {bad.size} outputs differ; first at ({m}, {n}), {tile}-tile "
                             f"{(m // tile, n // tile)}: got {float(got[m, n])!r}, want {float(want[m, n])!r}; "
                             f"{len(tiles)} wrong tiles, first {tiles[:8]}")


def set_knobs(monkeypatch, env):
    for key, val in env.items():
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)


@pytest.mark.parametrize("name,mode", sc.CASE_MODES)
def test_whole_output_is_the_cpu_chain(ops, dev, oracle, monkeypatch, name, mode):
    case = sc.BY_NAME[name]
    p = case.check_plan(mode)                     # the path this call takes, asserted on the reference side
    M, N, k = case.M, case.N, case.k
    chunks = p["chunks"]
    env = case.env_for(mode)

    def launch(dA, dB, Cin, out):
        ops.sgemm_tn(dA, dB, Cin, mode, skip_zero_k=case.skip_zero_k, allow_split_k=case.allow_split_k, out=out)

    for kind in ("randn", "ints"):
        what = f"{name} mode {mode} {kind} ({p['kernel']})"
        A, B, C = sc.randn_inputs(case) if kind == "randn" else sc.int_inputs(case)
        if kind == "randn":
            first = oracle.sgemm_tn_chain(A, B, C if mode == 0 else None, mode, chunks=chunks)
            third = oracle.sgemm_tn_chain(A, B, first, 0, chunks=chunks) if mode == 0 else None
        else:
            P = A.astype(np.float64).T @ B.astype(np.float64)
            absP = np.abs(A).astype(np.float64).T @ np.abs(B).astype(np.float64)
            assert_exactly_summable(np.abs(C).astype(np.float64) + 2.0 * absP, 0, what)
            first = {0: C - P, 1: P, 2: -P}[mode]
            third = C - 2.0 * P
        dA, dB = place(case, A, B, dev)
        if k > 0:
            assert (dA.data_ptr() % 16 == 0 and dA.stride(0) % 4 == 0) == p["a_vec"], what
            assert (dB.data_ptr() % 16 == 0 and dB.stride(0) % 4 == 0) == p["b_vec"], what
        set_knobs(monkeypatch, env)
        Wo, out = wide(dev, M, N)
        if mode != 0:
            launch(dA, dB, None, out)
            assert_whole_output(Wo, first, p["tile"], what)
            continue
        Wc, Cin = wide(dev, M, N, C)
        launch(dA, dB, Cin, out)
        assert_whole_output(Wo, first, p["tile"], what)
        assert_whole_output(Wc, C, p["tile"], what + ": Cin after the call")
        for _ in range(2):                        # in place, twice: the second pass reads what the first wrote
            launch(dA, dB, Cin, Cin)
        assert_whole_output(Wc, third, p["tile"], what + ", twice in place")
        if p["kernel"] == "ring":                 # the same calls through the register-staged kernel: the same bits
            set_knobs(monkeypatch, dict(env, QT_SGEMM_RING="0"))
            assert case.plan(mode, ring=False)["kernel"] in ("64x64", "128x128")
            Wr, Cr = wide(dev, M, N, C)
            for _ in range(2):
                launch(dA, dB, Cr, Cr)
            assert torch.equal(Cr.contiguous().view(torch.int32), Cin.contiguous().view(torch.int32)), what + " vs QT_SGEMM_RING=0"
            assert_whole_output(Wr, third, p["tile"], what + ", QT_SGEMM_RING=0")


def test_knobs_are_the_ones_the_library_reads(dev):
    """The two per-call knobs the cases set are spelled as csrc/sgemm_tn.hip reads them, and the once-per-process ones
    (QT_SGEMM_SUB_WAVES, QT_SGEMM_INTERIOR, QT_SGEMM_SPLIT_*) are at their defaults in this process: a case that ran
    with one of them set would not be on the path its plan names."""
    src = (Path(__file__).resolve().parent.parent / "quantool_amd" / "csrc" / "sgemm_tn.hip").read_text()
    for knob in ("QT_SGEMM_RING", "QT_SGEMM_RING_MIN_TILES"):
        assert f'getenv("{knob}")' in src
    for knob in ("QT_SGEMM_SUB_WAVES", "QT_SGEMM_INTERIOR", "QT_SGEMM_SPLIT_TARGET", "QT_SGEMM_SPLIT_MIN_CHUNK"):
        assert f'getenv("{knob}")' in src and knob not in os.environ
