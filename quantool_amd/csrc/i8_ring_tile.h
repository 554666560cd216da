// What the two int8 instances of ring_pipe.h's pipeline share -- gemm_i8_ring_kernel / gemm_i8_ring_moe_kernel
// (qlinear_ring.hip) and gemm_i8_ring_w4_kernel / gemm_i8_ring_w4_moe_kernel (qlinear_ring_w4.hip): the 256 x 256 tile
// over K-contiguous operands, the grouped forms' expert walk,
// K-tile t = units 4t .. 4t+3 = A0, B0, B1, A1 (half panels of 128 rows x 128 k), R 8, L 6.  Each file's head comment
// keeps the hazard argument of its own instance.  As with ring_pipe.h, an edit here edits hand-scheduled kernels:
// tools/isa_compare.py says whether one meant to be neutral was (profiles/i8_ring_tile_isa_parent_vs_refactor.txt
// lists the pieces that stayed in the two files and why).
#pragma once
#include "ring_pipe.h"

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

constexpr int RING = 8;                      // slots of 16 KiB resident in LDS (128 KiB): a unit lives in slot unit % 8
constexpr int LEAD = 6;                      // unit u + LEAD is issued in phase u (LEAD <= RING - 2)
constexpr int KU = 128;                      // k per K-tile: one cache line per row of Xq and fetch
constexpr int HP = 128;                      // rows of a half panel
constexpr int GROUP_M = 32;                  // m-tiles that walk the n-tiles together: workgroups are dealt round-robin
                                             // over 8 XCDs of 32 CUs, so the 32 tiles resident on one XCD are
                                             // 4 m-tiles x 8 n-tiles = 12 panels
static_assert(HP * KU == UNIT_BYTES, "an A unit is a half panel of 128 rows x 128 k-bytes");
static_assert(LEAD <= RING - 2, "ring_pipe.h, WAR");

// tile order: GROUP_M m-tiles walk the n-tiles together (as gemm_i8_kernel); workgroup pid -> its m-tile and n-tile
__device__ __forceinline__ void i8_ring_tile_of(int pid, int tiles_m, int tiles_n, int& m_tile, int& n_tile) {
    const int per_group = GROUP_M * tiles_n;
    const int first_m = pid / per_group * GROUP_M;
    const int gsize = (tiles_m - first_m) < GROUP_M ? (tiles_m - first_m) : GROUP_M;
    const int in_g = pid % per_group;
    m_tile = first_m + in_g % gsize;
    n_tile = in_g / gsize;
}

// The grouped (MOE) forms -- gemm_i8_ring_moe_kernel and gemm_i8_ring_w4_moe_kernel: expert e owns rows
// [offsets[e], offsets[e + 1]) of Y and the e-th weight matrix; R routed rows in all; A row m (and s_x / zp_x) is read
// at row_idx[m], clamped into [0, x_rows), when row_idx is given, else at m
struct RingMoe {
    const int32_t* offsets;
    const int32_t* row_idx;
    int64_t x_rows;
    int E;
};

// m-tile slot -> (expert, first row of the tile, end of the expert's rows); offsets clamped to [0, R] and made
// ascending, so a bad table cannot move a write out of Y (as gemm_i8_kernel).  False for a surplus slot.  The grid
// holds ceil(R/256) + E slots, an upper bound on sum_e ceil(rows_e / 256).  Uniform over the workgroup: scalar work
__device__ __forceinline__ bool i8_ring_moe_walk(const RingMoe& g, int R, int slot, int& e, int& m0, int& m_end) {
    int start = 0;
    for (int j = 0; j < g.E; ++j) {
        const int lo = min(max(g.offsets[j], 0), R);
        const int hi = min(max(g.offsets[j + 1], lo), R);
        const int nt = (int)(((int64_t)hi - lo + BT - 1) / BT);
        if (slot < start + nt) {
            e = j;
            m0 = lo + (slot - start) * BT;
            m_end = hi;
            return true;
        }
        start += nt;
    }
    return false;
}

// the Xq / s_x / zp_x row of output row m
__device__ __forceinline__ int64_t i8_ring_moe_src_row(const RingMoe& g, int64_t m) {
    if (g.row_idx) return min(max((int64_t)g.row_idx[m], (int64_t)0), g.x_rows - 1);
    return m;
}

// LDS image of an A unit (and of an int8 B unit): 16 pieces of 1 KiB, piece = 8 rows x 128 B; the 16-byte chunk c of row
// r (of the half panel) sits at chunk c ^ ((r >> 1) & 7) of its row.  A wave-instruction of the DMA fills one piece
// lane-linear, two per wave and unit (pieces 2 wave, 2 wave + 1): the XOR is on the source address.
// Instruction i of a thread: row 16 wave + 8 i + (lane >> 3) of the half panel, physical chunk lane & 7.  Its source byte
// offsets in the A0 and A1 units, relative to k-byte 0 of row row(0): a tile row past a_last (the panel's last valid
// row, relative to the tile) is fetched from a_last -- clamped, computed and never stored
template <class Row>
__device__ __forceinline__ void i8_ring_a_voff(int wave, int lane, int i, int64_t a_last, int K, Row&& row, unsigned& a0,
                                               unsigned& a1) {
    const int r = 16 * wave + 8 * i + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    const int64_t ra0 = r < a_last ? r : a_last, ra1 = HP + r < a_last ? HP + r : a_last;
    a0 = (unsigned)((size_t)row(ra0) * K + 16 * c);                      // < 256 * 32768 from the tile's first row
    a1 = (unsigned)((size_t)row(ra1) * K + 16 * c);
}

// C/D map of the 32x32 MFMA: column = lane & 31; row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  The output row of
// accumulator element r in lane half lh = lane >> 5 of the MFMA tile whose first row is `first`
__device__ __forceinline__ int64_t i8_ring_cd_row(int64_t first, int r, int lh) {
    return first + (r & 3) + 8 * (r >> 2) + 4 * lh;
}
