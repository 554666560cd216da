"""The cases of the fp32 TN GEMM's whole-matrix chain tests (test infrastructure, no GPU needed).

tests/test_gpu_sgemm_chain.py runs every case on the device and compares all M x N outputs with the CPU chain
(oracle/gptq_oracle.c: orc_sgemm_tn_chain); tests/test_sgemm_oracle.py checks, without a GPU, that every case lands on
the path it is listed for and that its random inputs tell an ascending fmaf chain from a wrong order.  This module holds

* ``plan``: the dispatch of ``qt_sgemm_tn`` (csrc/sgemm_tn.hip) restated -- which kernel a call takes, with how many
  tiles, k-steps and chunks, and whether its loads are the vector or the scalar ones.  The split rule is part of the
  bits (a chunk is a chain of its own), so the tests restate it instead of asking the library;
* ``CASES``: shape, modes, operand layout and environment of every case, each with ``want``: the fields of its plan
  that make it the case it is listed as.  ``check_plan`` compares them, so no case passes by missing its path;
* ``randn_inputs`` / ``int_inputs``: the operands, from a seed per case, the same for every mode of the case.
"""
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests.exact_inputs import dense_ints

BK = 16                 # k rows per k-step of every kernel (BK in csrc/sgemm_tn.hip, RBK in csrc/sgemm_ring.h)
BIG_TILE_MIN = 384      # from this many 128 x 128 tiles on: the 128 x 128 kernels, below: 64 x 64 tiles
RING_MIN_TILES = 32     # default of QT_SGEMM_RING_MIN_TILES
RING_MAX_WGS = 512      # persistent workgroups of the ring kernel: two per CU
SPLIT_TARGET_WGS = 256  # defaults of QT_SGEMM_SPLIT_TARGET / QT_SGEMM_SPLIT_MIN_CHUNK
SPLIT_MIN_CHUNK = 128
SPLIT_MIN_K = 512
SPLIT_MAX = 32


def _cdiv(a, b):
    return -(-a // b)


def split_chunks(M, N, k):
    """The split rule of qt_sgemm_tn for a call that passes the split workspace: -> chunk boundaries [0, ..., k], or
    None where k is not split (one chain)."""
    t128 = _cdiv(M, 128) * _cdiv(N, 128)
    if not (t128 < BIG_TILE_MIN and k >= SPLIT_MIN_K):
        return None
    splits = max(1, min(SPLIT_MAX, SPLIT_TARGET_WGS // t128))
    chunk = _cdiv(_cdiv(k, splits), 64) * 64
    chunk = max(chunk, SPLIT_MIN_CHUNK)
    splits = _cdiv(k, chunk)
    if splits < 2:
        return None
    return [min(k, z * chunk) for z in range(splits + 1)]


def plan(M, N, k, mode, *, allow_split_k=False, skip_zero_k=False, ring=True, ring_min_tiles=RING_MIN_TILES,
         lda=None, ldb=None, a_aligned=True, b_aligned=True):
    """What qt_sgemm_tn does with this call.  lda / ldb: pitches in elements (default: M, N); a_aligned / b_aligned:
    whether the operand starts on a 16-byte boundary.  -> dict:
      kernel      "split" (128 x 128 SET instances over k chunks + splitk_reduce_kernel), "ring", "128x128", "64x64"
      tile        edge of the kernel's output tile;  tiles: how many;  whole_tiles: those that lie inside M x N
      waves       waves per workgroup of the instance (8: the MODE_SUB 128 x 128 kernel and the ring)
      a_vec, b_vec  16-byte loads legal for the operand;  interior_tiles: whole tiles that load with them unguarded
      nsteps      k-steps of 16 per chain (of the longest chunk when split);  ragged_k: the last k-step is partial
      fast_loop   the 64 x 64 kernel's branch-free two-steps-in-flight loop (interior tiles, an even number of whole
                  k-steps from the tile's first k row on)
      chunks      chunk boundaries or None;  reduce_vector: the reducer's float4 path (N % 4 == 0)
      ring_pairs, ring_wgs, ring_tiles_per_wg  stage pairs per tile, workgroups, most tiles one workgroup streams
      k_begins    skip_zero_k: the first k row each tile column reads (before a chunk clamps it)"""
    lda = M if lda is None else lda
    ldb = N if ldb is None else ldb
    t128 = _cdiv(M, 128) * _cdiv(N, 128)
    a_vec = lda % 4 == 0 and a_aligned
    b_vec = ldb % 4 == 0 and b_aligned
    p = dict(t128=t128, a_vec=a_vec, b_vec=b_vec, chunks=None, ragged_k=k % BK != 0)
    chunks = split_chunks(M, N, k) if allow_split_k else None
    ring_applies = (mode == 0 and not skip_zero_k and k >= 4 * BK and k % (2 * BK) == 0 and M % 128 == 0 and
                    N % 128 == 0 and a_vec and b_vec)
    if chunks is not None:
        longest = max(b - a for a, b in zip(chunks, chunks[1:]))
        p.update(kernel="split", tile=128, waves=4, chunks=chunks, nsteps=_cdiv(longest, BK),
                 ragged_k=any((b - a) % BK for a, b in zip(chunks, chunks[1:])), reduce_vector=N % 4 == 0)
    elif ring and ring_applies and t128 >= ring_min_tiles:
        wgs = min(RING_MAX_WGS, t128)
        p.update(kernel="ring", tile=128, waves=8, nsteps=k // BK, ring_pairs=k // (2 * BK), ring_wgs=wgs,
                 ring_tiles_per_wg=_cdiv(t128, wgs))
    elif t128 >= BIG_TILE_MIN:
        p.update(kernel="128x128", tile=128, waves=8 if mode == 0 else 4, nsteps=_cdiv(k, BK))
    else:
        p.update(kernel="64x64", tile=64, waves=4, nsteps=_cdiv(k, BK))
    t = p["tile"]
    p["tiles"] = _cdiv(M, t) * _cdiv(N, t)
    p["whole_tiles"] = (M // t) * (N // t)
    p["interior_tiles"] = p["whole_tiles"] if a_vec and b_vec else 0
    k_begins = [n0 // BK * BK for n0 in range(0, N, t)] if skip_zero_k else [0]
    p["fast_loop"] = p["kernel"] == "64x64" and p["interior_tiles"] > 0 and any(
        (k - kb) > 0 and (k - kb) % (2 * BK) == 0 for kb in k_begins)
    if skip_zero_k:
        p["k_begins"] = k_begins
    return p


@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    k: int
    modes: tuple
    want: dict                      # mode-independent plan fields; `want_mode` adds per-mode ones
    want_mode: dict = field(default_factory=dict)
    allow_split_k: bool = False
    skip_zero_k: bool = False
    a_offset: int = 0               # A starts this many floats into its allocation
    b_pad: int = 0                  # B is the first N columns of a [k, N + b_pad] matrix
    env: dict = field(default_factory=dict)   # QT_SGEMM_RING / QT_SGEMM_RING_MIN_TILES; per mode: {mode: {...}}

    @property
    def seed(self):
        return zlib.crc32(self.name.encode())

    def env_for(self, mode):
        """The two per-call knobs for this mode: None means unset (the default)."""
        e = {"QT_SGEMM_RING": None, "QT_SGEMM_RING_MIN_TILES": None}
        e.update(self.env.get(mode, {}))
        return e

    def plan(self, mode, ring=None):
        e = self.env_for(mode)
        use_ring = e["QT_SGEMM_RING"] != "0" if ring is None else ring
        min_tiles = int(e["QT_SGEMM_RING_MIN_TILES"] or RING_MIN_TILES)
        return plan(self.M, self.N, self.k, mode, allow_split_k=self.allow_split_k, skip_zero_k=self.skip_zero_k,
                    ring=use_ring, ring_min_tiles=min_tiles, lda=self.M, ldb=self.N + self.b_pad,
                    a_aligned=self.a_offset % 4 == 0)

    def check_plan(self, mode):
        """The reference-side assertion: the call of this case and mode lands where the case says.  -> the plan."""
        p = self.plan(mode)
        for key, val in {**self.want, **self.want_mode.get(mode, {})}.items():
            assert p[key] == val, f"{self.name} mode {mode}: plan[{key!r}] = {p[key]!r}, the case needs {val!r}"
        return p


ALL = (0, 1, 2)
_S64 = dict(kernel="64x64", chunks=None)
_RING_OFF = {0: {"QT_SGEMM_RING": "0"}}

CASES = [
    # ---- the 64 x 64 register-staged kernel (fewer than 384 tiles of 128 x 128)
    Case("s64_scalar_one_partial_step", 1, 5, 3, ALL,
         dict(_S64, tiles=1, whole_tiles=0, nsteps=1, ragged_k=True, a_vec=False, b_vec=False)),
    Case("s64_interior_fast_loop", 64, 64, 32, ALL,
         dict(_S64, tiles=1, interior_tiles=1, nsteps=2, ragged_k=False, fast_loop=True)),
    Case("s64_interior_odd_nsteps", 64, 128, 48, ALL,
         dict(_S64, tiles=2, interior_tiles=2, nsteps=3, ragged_k=False, fast_loop=False)),
    Case("s64_interior_ragged_k", 128, 192, 37, ALL,
         dict(_S64, tiles=6, interior_tiles=6, nsteps=3, ragged_k=True, fast_loop=False)),
    Case("s64_every_edge", 130, 70, 37, ALL,
         dict(_S64, tiles=6, whole_tiles=2, interior_tiles=0, nsteps=3, ragged_k=True, a_vec=False, b_vec=False)),
    Case("s64_k0", 64, 64, 0, ALL,
         dict(_S64, tiles=1, nsteps=0)),
    Case("s64_a_unaligned", 192, 128, 64, ALL,
         dict(_S64, tiles=6, whole_tiles=6, interior_tiles=0, nsteps=4, a_vec=False, b_vec=True), a_offset=1),
    Case("s64_b_pitch_unaligned", 192, 128, 64, ALL,
         dict(_S64, tiles=6, whole_tiles=6, interior_tiles=0, nsteps=4, a_vec=True, b_vec=False), b_pad=2),
    Case("s64_aligned_control", 192, 128, 64, ALL,
         dict(_S64, tiles=6, interior_tiles=6, nsteps=4, a_vec=True, b_vec=True, fast_loop=True)),
    # ---- the 128 x 128 kernels (384 tiles or more): 8 waves in mode 0, the 4-wave SET / NEG instances otherwise
    Case("s128_ragged_384_tiles", 1930, 3000, 40, ALL,
         dict(kernel="128x128", t128=384, tiles=384, whole_tiles=15 * 23, a_vec=False, b_vec=True, nsteps=3, ragged_k=True,
              chunks=None),
         {0: dict(waves=8), 1: dict(waves=4), 2: dict(waves=4)}),
    Case("s128_interior_384_tiles", 2048, 3072, 32, ALL,
         dict(kernel="128x128", t128=384, tiles=384, interior_tiles=384, nsteps=2, ragged_k=False, chunks=None),
         {0: dict(waves=8), 1: dict(waves=4), 2: dict(waves=4)}, env=_RING_OFF),
    # ---- the ring kernel (mode 0, whole tiles, default QT_SGEMM_RING)
    Case("ring_32_tiles_shortest_k", 512, 1024, 64, (0,),
         dict(kernel="ring", tiles=32, ring_pairs=2, ring_wgs=32, ring_tiles_per_wg=1)),
    Case("ring_three_stage_pairs", 512, 1024, 96, (0,),
         dict(kernel="ring", tiles=32, ring_pairs=3, ring_wgs=32, ring_tiles_per_wg=1)),
    Case("ring_one_tile", 128, 128, 64, (0,),
         dict(kernel="ring", tiles=1, ring_pairs=2, ring_wgs=1, ring_tiles_per_wg=1),
         env={0: {"QT_SGEMM_RING_MIN_TILES": "1"}}),
    Case("ring_two_tiles_per_workgroup", 2048, 4224, 64, (0,),
         dict(kernel="ring", tiles=528, ring_pairs=2, ring_wgs=512, ring_tiles_per_wg=2)),
    # ---- split-K: each chunk a chain from 0, the chunk sums added in ascending order
    Case("split_4_chunks", 128, 128, 512, ALL,
         dict(kernel="split", chunks=[0, 128, 256, 384, 512], reduce_vector=True, ragged_k=False), allow_split_k=True),
    Case("split_8_chunks_ragged_last_scalar_reduce", 100, 70, 1000, ALL,
         dict(kernel="split", chunks=list(range(0, 1000, 128)) + [1000], reduce_vector=False, ragged_k=True),
         allow_split_k=True),
    Case("split_9_chunks_vector_reduce", 100, 72, 1100, ALL,
         dict(kernel="split", chunks=list(range(0, 1100, 128)) + [1100], reduce_vector=True), allow_split_k=True),
    Case("split_32_chunks", 128, 1024, 4096, ALL,
         dict(kernel="split", chunks=list(range(0, 4097, 128)), reduce_vector=True), allow_split_k=True),
    Case("split_100_tiles_2_chunks", 1280, 1280, 1024, ALL,
         dict(kernel="split", t128=100, chunks=[0, 512, 1024], reduce_vector=True), allow_split_k=True),
    Case("split_below_threshold", 128, 128, 511, ALL,
         dict(_S64, tiles=4, nsteps=32, ragged_k=True), allow_split_k=True),
    # ---- skip_zero_k: B[kk][n] == 0 for kk < n; a tile column starts at its n0 rounded down to a k-step
    Case("skip_s64", 70, 200, 200, ALL,
         dict(_S64, tiles=8, k_begins=[0, 64, 128, 192], ragged_k=True), skip_zero_k=True),
    Case("skip_s64_interior_fast_loop", 64, 256, 256, ALL,
         dict(_S64, tiles=4, interior_tiles=4, k_begins=[0, 64, 128, 192], ragged_k=False, fast_loop=True),
         skip_zero_k=True),
    Case("skip_split_clamped_per_chunk", 128, 1024, 1024, ALL,
         dict(kernel="split", chunks=list(range(0, 1025, 128)), k_begins=list(range(0, 1024, 128))),
         allow_split_k=True, skip_zero_k=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CASE_MODES = [(c.name, m) for c in CASES for m in c.modes]


def skip_mask(k, N):
    """[k, N] bool: where a skip_zero_k case's B is nonzero -- kk >= n, so the diagonal and row n0 of every tile column
    are among the nonzeros and a kernel that skips one k row too many loses a product."""
    return np.arange(k)[:, None] >= np.arange(N)[None, :]


def randn_inputs(case):
    """-> (A [k, M], B [k, N], C [M, N]) float32 standard normal from the case's seed (far from subnormals)."""
    rng = np.random.default_rng(case.seed)
    A = rng.standard_normal((case.k, case.M), dtype=np.float32)
    B = rng.standard_normal((case.k, case.N), dtype=np.float32)
    C = rng.standard_normal((case.M, case.N), dtype=np.float32)
    if case.skip_zero_k:
        keep = skip_mask(case.k, case.N)
        B = np.where(keep, B, np.float32(0))
        assert (B != 0)[keep].all()
    return A, B, C


def int_inputs(case):
    """-> (A, B, C) float32 integers: A, B in +-{1, 2, 3} (never zero where B is not structurally zero), |C| <= 1000."""
    s = case.seed
    A = dense_ints((case.k, case.M), s + 1)
    B = dense_ints((case.k, case.N), s + 2)
    C = np.random.default_rng(s + 3).integers(-1000, 1001, size=(case.M, case.N)).astype(np.float32)
    if case.skip_zero_k:
        B = np.where(skip_mask(case.k, case.N), B, np.float32(0))
    return A, B, C
