"""orc_sgemm_tn_chain (oracle/gptq_oracle.c): the CPU restatement of qt_sgemm_tn_f32 that tests/test_gpu_sgemm_chain.py
compares whole device outputs with.  No GPU: the function against libm's fmaf element by element, against the exact
integer product, the cases of tests/sgemm_cases.py against the paths they are listed for, and the cases' random inputs
against two wrong summation orders (an equality test on inputs that cannot tell the orders apart would prove nothing)."""
import ctypes

import numpy as np
import pytest

from tests import sgemm_cases as sc
from tests.exact_inputs import assert_exactly_summable, dense_ints

SENTINEL = np.float32(-777.0)


@pytest.fixture(scope="module")
def fmaf():
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    return libm.fmaf


def libm_reference(fmaf, A, B, Cin, mode, chunks):
    """The definition, one libm call per product: a chain from 0 per chunk, chunk sums added by fp32 '+' in ascending
    order from 0.0, then the mode as one fp32 operation."""
    k, M = A.shape
    N = B.shape[1]
    out = np.empty((M, N), np.float32)
    spans = [(0, k)] if chunks is None else list(zip(chunks, chunks[1:]))
    for m in range(M):
        for n in range(N):
            total = np.float32(0.0)
            for k0, k1 in spans:
                acc = 0.0
                for kk in range(k0, k1):
                    acc = fmaf(float(A[kk, m]), float(B[kk, n]), acc)
                total = np.float32(acc) if chunks is None else np.float32(total + np.float32(acc))
            out[m, n] = {0: lambda: np.float32(Cin[m, n] - total), 1: lambda: total, 2: lambda: np.float32(-total)}[mode]()
    return out


def pitched(x, left, right, fill=SENTINEL):
    """x as a column slice of a wider sentinel-filled matrix -> (wide, view)."""
    wide = np.full((x.shape[0], x.shape[1] + left + right), fill, np.float32)
    wide[:, left:left + x.shape[1]] = x
    return wide, wide[:, left:left + x.shape[1]]


@pytest.mark.parametrize("M,N,k,chunks", [
    (40, 24, 70, None), (40, 24, 70, [0, 16, 33, 70]), (1, 5, 3, None), (1, 5, 3, [0, 1, 3]),
    (33, 17, 37, None), (33, 17, 37, [0, 37]), (13, 24, 64, [0, 8, 16, 24, 32, 40, 48, 56, 63, 64]), (7, 3, 0, None),
])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_chain_is_libm_fmaf_for_every_element(oracle, fmaf, M, N, k, chunks, mode):
    """Every operand at a pitch of its own (column slices of wider matrices), every element against libm."""
    rng = np.random.default_rng([M, N, k, mode])
    A = pitched(rng.standard_normal((k, M), dtype=np.float32), 1, 2)[1]
    B = pitched(rng.standard_normal((k, N), dtype=np.float32), 3, 0)[1]
    Cw, C = pitched(rng.standard_normal((M, N), dtype=np.float32), 2, 3)
    Ow, O = pitched(np.zeros((M, N), np.float32), 1, 1)
    want = libm_reference(fmaf, A, B, C, mode, chunks)
    Cw0 = Cw.copy()
    got = oracle.sgemm_tn_chain(A, B, C if mode == 0 else None, mode, chunks=chunks, out=O)
    assert got is O and np.array_equal(O, want)
    assert (Ow[:, 0] == SENTINEL).all() and (Ow[:, -1] == SENTINEL).all() and np.array_equal(Cw, Cw0)
    assert np.array_equal(oracle.sgemm_tn_chain(np.ascontiguousarray(A), np.ascontiguousarray(B),
                                                np.ascontiguousarray(C) if mode == 0 else None, mode, chunks=chunks), want)
    if mode == 0:       # in place, twice: Cin is Cout
        for _ in range(2):
            oracle.sgemm_tn_chain(A, B, C, 0, chunks=chunks, out=C)
        assert np.array_equal(C, libm_reference(fmaf, A, B, want, 0, chunks))
        assert (Cw[:, :2] == SENTINEL).all() and (Cw[:, -3:] == SENTINEL).all()


@pytest.mark.parametrize("M,N,k,chunks", [(40, 24, 70, None), (130, 70, 37, [0, 16, 37]), (100, 72, 1100, "rule"),
                                          (64, 64, 0, None)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_chain_is_the_integer_product_on_exact_inputs(oracle, M, N, k, chunks, mode):
    """Integers in +-{1, 2, 3}: every partial sum in every order is exact, so the chain IS the fp64 product."""
    if chunks == "rule":
        chunks = sc.split_chunks(M, N, k)
        assert len(chunks) == 10
    A, B = dense_ints((k, M), 1), dense_ints((k, N), 2)
    C = np.random.default_rng(3).integers(-1000, 1001, size=(M, N)).astype(np.float32)
    P = A.astype(np.float64).T @ B.astype(np.float64)
    assert_exactly_summable(np.abs(C.astype(np.float64)) + np.abs(A).astype(np.float64).T @ np.abs(B).astype(np.float64), 0)
    got = oracle.sgemm_tn_chain(A, B, C if mode == 0 else None, mode, chunks=chunks)
    assert np.array_equal(got.astype(np.float64), {0: C - P, 1: P, 2: -P}[mode])


@pytest.mark.parametrize("name,mode", sc.CASE_MODES)
def test_every_case_lands_on_the_path_it_is_listed_for(name, mode):
    case = sc.BY_NAME[name]
    p = case.check_plan(mode)
    if p["kernel"] == "ring":     # the same call under QT_SGEMM_RING=0 takes a register-staged kernel
        assert case.plan(mode, ring=False)["kernel"] == ("128x128" if p["t128"] >= sc.BIG_TILE_MIN else "64x64")


def test_split_rule_restated():
    """The figures of the rule (csrc/sgemm_tn.hip: qt_sgemm_tn) at its corners."""
    assert sc.split_chunks(128, 128, 511) is None                       # k below 512
    assert sc.split_chunks(2048, 3072, 4096) is None                    # 384 tiles: never split
    assert sc.split_chunks(128, 128, 512) == [0, 128, 256, 384, 512]    # chunk floor of 128
    assert sc.split_chunks(1280, 1280, 1024) == [0, 512, 1024]          # 256 // 100 = 2 splits
    assert sc.split_chunks(1280, 1408, 1024) == [0, 512, 1024]          # 110 tiles: still 2
    assert sc.split_chunks(1664, 1280, 1024) is None                    # 130 tiles: 256 // 130 = 1 split
    assert sc.split_chunks(128, 128, 8192) == [256 * z for z in range(33)]          # at most 32 chunks
    assert sc.split_chunks(128, 128, 8200) == [320 * z for z in range(26)] + [8200]  # ceil(8200 / 32) = 257 -> 320


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_random_inputs_tell_the_orders_apart(oracle, name, capsys):
    """On the randn operands the GPU test uses, the ascending fmaf chain differs from a descending-k chain and from an
    unfused acc + a * b in at least one element of every case (k = 0 has no product and no order: all three agree).
    Shares of differing elements of the accumulators (mode 1; the operands are the same in every mode), as printed:

      case                                       descending   unfused
      s64_scalar_one_partial_step                    0.2000    0.4000      (5 outputs, k = 3)
      s64_interior_fast_loop                         0.7922    0.6304
      s64_interior_odd_nsteps                        0.8364    0.6727
      s64_interior_ragged_k                          0.8149    0.6487
      s64_every_edge                                 0.8166    0.6453
      s64_k0                                         0.0000    0.0000      (no product)
      s64_a_unaligned                                0.8643    0.6991
      s64_b_pitch_unaligned                          0.8625    0.7049
      s64_aligned_control                            0.8606    0.7055
      s128_ragged_384_tiles                          0.8264    0.6575
      s128_interior_384_tiles                        0.8070    0.6346
      ring_32_tiles_shortest_k                       0.8634    0.7007
      ring_three_stage_pairs                         0.8875    0.7333
      ring_one_tile                                  0.8574    0.7061
      ring_two_tiles_per_workgroup                   0.8624    0.7002
      split_4_chunks                                 0.8858    0.7592
      split_8_chunks_ragged_last_scalar_reduce       0.8966    0.7829
      split_9_chunks_vector_reduce                   0.9031    0.7908
      split_32_chunks                                0.9094    0.8340
      split_100_tiles_2_chunks                       0.9415    0.8242
      split_below_threshold                          0.9532    0.8318
      skip_s64                                       0.8546    0.7028
      skip_s64_interior_fast_loop                    0.8708    0.7227
      skip_split_clamped_per_chunk                   0.8777    0.7544
    """
    case = sc.BY_NAME[name]
    A, B, _ = sc.randn_inputs(case)
    chunks = case.plan(1)["chunks"]
    asc = oracle.sgemm_tn_chain(A, B, None, 1, chunks=chunks)
    desc = oracle.sgemm_tn_chain(A, B, None, 1, chunks=chunks, variant=1)
    unfused = oracle.sgemm_tn_chain(A, B, None, 1, chunks=chunks, variant=2)
    s_desc, s_unf = float((asc != desc).mean()), float((asc != unfused).mean())
    with capsys.disabled():
        print(f"\n      {name:42s} {s_desc:10.4f} {s_unf:9.4f}", end="")
    if case.k == 0:
        assert s_desc == 0 and s_unf == 0 and not asc.any()
        return
    assert s_desc > 0, "a descending-k chain gives the same bits: these inputs cannot pin the order"
    assert s_unf > 0, "acc + a * b gives the same bits: these inputs cannot pin the fused multiply-add"
