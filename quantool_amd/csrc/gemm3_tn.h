// fp32-accurate "TN" product on the bf16 MFMA:  acc[m][n] = sum_k A[k][m] * B[k][n]  with every fp32
// operand split into three bf16 planes  x = hi + mid + lo  (each the round-to-nearest bf16 of what the
// previous ones left: the residual after three planes is <= 2^-27 |x|) and the six plane products whose
// weight is >= 2^-16 of hi*hi summed in one fp32 MFMA accumulator, smallest first:
//     lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi              (dropped: mid*lo, lo*mid, lo*lo <= 2^-24)
// -- 6 bf16-MFMA flops per fp32 flop at 16x the f32-MFMA rate.  The kernel is xtx.hip's LDS-ring pipeline
// (ring_pipe.h) on "tri-units": 16 k-rows of all three planes of both operands (48 KiB) per ring slot, three
// slots, so each plane panel of a k-slab is staged into LDS once and its fragments are read once for all six
// products (48 MFMAs per wave between barrier pairs).  Summation order inside a tile: 16-row slab -> product
// (smallest first).  QT_G3_LOOP=chunk selects the earlier loop (one plane pair per 16 KiB unit, 64-row chunk ->
// product -> 16-row unit: every product stages its own two panels, 12 stagings per chunk for 6 distinct
// panels) for A/B runs; the two loops sum the same products in a different order, so their bits differ.
// The kernel serves the two products that carry the K^3 of qt_cholesky_inverse_upper (cholesky.hip), which
// are not bit-pinned by the oracle (the factor U is compared through the sweep's outputs, not bit
// for bit), the opt-in QT_SWEEP_FAR=bf16x3 and the fp32-activation Gram sum (qt_xtx_accumulate_f32).  NOT used
// by the GPTQ sweep's default trailing update, whose ascending-k fmaf order is part of the parity contract
// (sgemm_tn.h).
#pragma once
#include <vector>

#include "common.h"

constexpr int G3_CHUNK_ROWS = 64;   // granularity of an item's k range

// One workgroup = one item: a 256x256 output tile over k rows [64*c_lo, 64*c_hi) of the planes (>= 2 chunks).
struct G3Item {
    int tile;   // (ti << 16) | (segment << 15) | tj : output rows 256*ti.., columns 256*tj.. of the segment's C
    int c_lo;   // k range in chunks of G3_CHUNK_ROWS rows, relative to row0 of the call
    int c_hi;
    int slab;   // < 0: the item covers the tile's whole k range and applies it to C itself (C -= acc / C = acc);
                // >= 0: partial product -> slab[slab] (256x256 fp32), reduced in table order afterwards
};
// One output tile assembled from `count` consecutive slabs starting at `first`.
struct G3Red {
    int tile;
    int first;
    int count;
    int seg;    // segment (0 / 1) whose C the tile belongs to
};
constexpr int G3_SEG_BIT = 1 << 15;   // in G3Item::tile (G3Red::tile carries ti and tj only)
constexpr int G3_TJ_MASK = G3_SEG_BIT - 1;

enum { G3_SUB = 0, G3_SET = 1, G3_ADD = 2 };   // C -= product  /  C = product  /  C += product

// Plane mode.  G3_BF16X3: the three bf16 planes and six products above.  G3_F16X2: two fp16 planes per operand,
//     hi = fp16(x * 2^e),  lo' = fp16((x * 2^e - hi) * 2^11)          (both differences exact; residual <= 2^-24 |x|)
// and three products in the one accumulator, smallest first:  lo'_a * hi_b,  hi_a * lo'_b,  hi_a * (2^11 hi_b)  (the
// last factor made in registers, exactly), scaled by 2^-(11 + eA + eB) in the epilogue (exact): half the MFMAs and two
// thirds of the staged bytes.  fp16 has 5 exponent bits, so the caller must know a bound on each operand and give the
// per-problem exponents e with |x| * 2^e < 2^4: elements down to 2^-18 of that keep 22 significant bits, smaller ones
// keep an absolute error of 2^-25 * 2^-e (fp16 subnormals), nothing overflows.  Dropped: lo_a * lo_b <= 2^-24.
enum { G3_BF16X3 = 0, G3_F16X2 = 1 };
constexpr int G3_E_MAX = 40;   // |e| of a scale exponent (the epilogue's 2^-(11 + eA + eB) stays a normal float)

struct G3Args {
    const unsigned short* Apl;   // plane 0 of the A operand, [rows][ld] bf16; plane q at + q * plane_stride
    const unsigned short* Bpl;
    int64_t plane_stride;        // elements between planes (same for A and B)
    int64_t ld;                  // row pitch in elements (same for A and B; a multiple of 8)
    int64_t rowA0, rowB0;        // plane row of k = 0
    int colA0, colB0;            // plane column of output row 0 / output column 0
    int colmax;                  // planes have colmax columns (loads are clamped to colmax - 8)
    int M, N;                    // output extent
    float* C;
    int64_t ldc;
    // B-side layout when it differs from A's (0 = same as A): pitch, plane stride, column count
    int64_t ldB = 0, plane_strideB = 0;
    int colmaxB = 0;
    int mode;                    // G3_SUB / G3_SET: what direct items and the slab reduction do to C
    float* slabs;                // [n_slabs][256*256]
    const G3Item* items;         // device
    int n_items;
    const G3Red* red;            // device
    int n_red;
    // batch > 1: `batch` problems of identical shape in one launch (one item / reduction table for all): problem b
    // reads planes at Apl + b * bsApl, Bpl + b * bsBpl (elements), writes C + b * bsC and uses slabs + b * bsSlabs.
    int batch = 1;
    int64_t bsApl = 0, bsBpl = 0, bsC = 0, bsSlabs = 0;
    // G3_F16X2: the planes are the two fp16 planes of qt_split2h_launch (plane 1 at + plane_stride) and eA / eB
    // (device, int32[batch], |e| <= G3_E_MAX) the exponents they were split with.
    int planes = G3_BF16X3;
    const int32_t* eA = nullptr;
    const int32_t* eB = nullptr;
    // Second segment (Bpl1 != nullptr): the same launch also forms  A^T B1  into C1.  Items and reductions whose tile
    // carries G3_SEG_BIT read B1's planes (layout, pitch and batch stride as B's) from column colB01 on and apply to
    // C1 [M][N1] with mode1; everything on the A side, the slabs and the tables are shared.
    const unsigned short* Bpl1 = nullptr;
    int colB01 = 0;
    const int32_t* eB1 = nullptr;
    float* C1 = nullptr;
    int64_t ldc1 = 0, bsC1 = 0;
    int mode1 = G3_SET;
    int N1 = 0;
};

// Enqueue the product (and the slab reduction when n_red > 0).  Returns qt_status.
int qt_gemm3_launch(const G3Args& a, hipStream_t stream);

// fp32 [rows][ld_src] -> three bf16 planes at planes + q * plane_stride (pitch ld_pl).  cols % 4 == 0.
// mask_upper != 0: elements with (col_g0 + c) > (row_g0 + r) are written as zeros (a lower-triangular
// source whose upper part is not initialised).
// batch > 1: problem b reads src + b * bs_src and writes planes + b * bs_planes (elements).
int qt_split3_launch(const float* src, int64_t ld_src, int rows, int cols, unsigned short* planes, int64_t ld_pl,
                     int64_t plane_stride, int mask_upper, int row_g0, int col_g0, hipStream_t stream, int batch = 1,
                     int64_t bs_src = 0, int64_t bs_planes = 0);

// The two-plane sibling (G3_F16X2): fp16 planes hi, lo' of src * 2^e[problem] at planes, planes + plane_stride; e: device
// int32[batch].  Same call pattern, strides and masking.
int qt_split2h_launch(const float* src, int64_t ld_src, int rows, int cols, unsigned short* planes, int64_t ld_pl,
                      int64_t plane_stride, int mask_upper, int row_g0, int col_g0, const int32_t* e, hipStream_t stream,
                      int batch = 1, int64_t bs_src = 0, int64_t bs_planes = 0);

// Host: the scale exponent e = 3 - ceil(log2(bound)) for an operand with |x| <= bound, clamped to +-G3_E_MAX.
int g3_scale_exponent(float bound);

// Host-side item table of a block-row product: Tm x Tn tiles over k chunks [lo, c_end) (chunks of
// G3_CHUNK_ROWS rows), lo = 0, or with tri != 0 lo = first chunk of row 256 * tj (B is lower-triangular in
// 256-blocks: B[k][n] == 0 for k < 256 * tj); split along k into <= 256 items of near-equal length (one round
// of the 256 CUs), longest first.
long g3_row_chunks(int Tm, int Tn, int c_end, int tri);
void g3_plan_row(int Tm, int Tn, int c_end, int tri, std::vector<G3Item>& items, std::vector<G3Red>& red, int target_items = 0);
// One table for the two products of a block row that share the A operand and the k range: segment 0 = Tm x Tn0 tiles
// over chunks [0, c_end), segment 1 = Tm x Tn1 tiles with the triangular start (G3_SEG_BIT set in their tile).  Same
// rule as g3_plan_row over the union of the tiles; slab ids run across both segments.  max_slabs > 0: pieces grow
// until the table needs no more slabs than that.
void g3_plan_row2(int Tm, int Tn0, int Tn1, int c_end, std::vector<G3Item>& items, std::vector<G3Red>& red,
                  int target_items = 0, int max_slabs = 0);
