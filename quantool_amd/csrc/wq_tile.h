// The 128 x 128 A16 tile on packed weights, stated once for its two kernels: wq_tile_kernel (wq_tile.hip, a dense
// Linear of any M) and moe_gemm_wq_tile_kernel (wq_moe_tile.hip, the same tile over E weight matrices and routed,
// gathered rows).  wq_tile.hip's head comment states the tile, its units, its hazards and its numerics; this header
// holds the constants and helpers, and wq_tile_body.h the statements, which each kernel includes as its body behind
// its own choice of tile.  Text, not a function template, for wq_stream_tile.h's reason: an inlined template moved
// wq.hip's register allocation both ways, and the dense kernel is to stay what was measured.  As text its eight
// instances keep their register counts and LDS, and their ISA from the first LDS-DMA to the last store instruction for
// instruction; the scalar address arithmetic in front of it is scheduled in another order under other SGPR names.
// Everything sits in an unnamed namespace: each translation unit gets its own copy.
#pragma once
#include "common.h"
#include "i8_ring_tile.h"
#include "wq_stream_tile.h"

namespace {

constexpr int TT = 128;                      // output tile edge
constexpr int TKU = 64;                      // columns per K-tile: half a weight group
constexpr int TSLOTS = 3;                    // units resident in LDS
constexpr int TLEAD = 2;                     // unit t + TLEAD is issued in phase t
constexpr int TTHREADS = 256;                // 4 waves: 2 (M) x 2 (N), 64 x 64 outputs per wave
constexpr int TX_BYTES = TT * TKU * 2;       // 16 KiB: the X tile, and one weight image
constexpr int TS_BYTES = 2 * TT * 4;         // 128 scales, 128 zero-points as dwords
static_assert(2 * TKU == WQ_KB, "two K-tiles per weight group");
static_assert(TLEAD <= TSLOTS - 1, "WAR: see wq_tile.hip's head comment");

// One sign-extended byte per lane into a dword of LDS (64 x 4 B per wave-instruction): the gather of a column of the
// int8 zero-point table, whose entries no dword load can address.  ring_pipe.h's glds4_one with the byte opcode;
// counted in vmcnt like every other LDS-DMA.
__device__ __forceinline__ void glds1_one(unsigned voff, const void* sbase, unsigned lds_dst) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_sbyte %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}

template <int DT>
__device__ __forceinline__ f32x16 tile_mfma(const u32x4 a, const u32x4 b, f32x16 c) {
    if constexpr (DT == QT_F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0,
                                                      0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                       0, 0, 0);
}

// byte offset of the 16-byte chunk c of row r in the X tile / weight image
__device__ __forceinline__ int tile_img(int r, int c) {
    return (r >> 3) * 1024 + (r & 7) * 128 + 16 * (c ^ ((r >> 1) & 7));
}

}  // namespace
