// The weight-streaming 16-column A16 tile, stated once for its two kernels: wq_stream_kernel (wq.hip, a dense Linear of
// 1 .. 128 rows) and moe_gemm_wq_wide_kernel (wq_moe_wide.hip, the same tile over E weight matrices), together with the
// weight description and the fragment helpers the skinny kernel shares with them.  include/quantool_amd.h, "A16
// runtime"; DESIGN.md 4.16 and 4.19.
//
// The skinny tile over MT m-tiles of 16 activation rows: the same workgroup shape (256 threads own 16 output columns n
// = weight rows and split K over 4 waves, k-block kb of 128 columns to wave kb % 4), the same statements for the weight
// chunk, the group parameters and the A fragment, so accumulator t of wave w runs the chain the skinny kernel's wave w
// runs on rows [16 t, 16 t + 16).  The A fragments of a k-block are formed once and kept for every m-tile.  The B
// fragments (activation rows) come from L2 in fragment shape, WQ_XB - 1 (k-block, m-tile) steps ahead of the MFMAs that
// use them.  A wave takes its k-blocks in batches of WQ_SB (then 4, 2, 1 for the rest), so nothing in a batch is
// conditional: no dead k-block, no dead m-tile.  (The skinny kernel pads its last batch with all-zero products
// instead, which leave a sum that started at +0 unchanged; the batch length is no part of the summation order.)
// Instances for 2 / 4 / 8 tiles with uniform branches around the dead tiles' loads and MFMAs were tried first: every
// branch made the compiler merge the whole accumulator array, and the 8-tile instance needed 256 VGPRs and 200 AGPRs of
// copies.
//
// Activations come through buffer loads, and a row that does not exist is a lane out of the descriptor's range: it
// gets zeros and no memory access is made for it.
//   MOE = false  one instance per tile count MT = ceil(M / 16).  m-tile t's descriptor starts at row 16 t and ends with
//                the last column of row min(M, 16 t + 16) - 1, so a lane whose row is >= M is out of range (ldx >= K).
//                The host bounds ldx, so the byte offsets fit 32 bits.
//   MOE = true   p is one expert's weight and p.M <= 16 MT of its rows, first output row m0 (the kernel walks offsets
//                before the tile's statements).  One descriptor covers X [x_rows, ldx]; row m of the tile is X[row_idx[m0 +
//                m] clamped into [0, x_rows)] or X[m0 + m], one 32-bit byte offset per m-tile and lane; a row >= p.M
//                has the descriptor's size as its offset.  MT may exceed ceil(p.M / 16): a dead m-tile multiplies
//                zeros that came from no memory access, and is not stored.  The host keeps x_rows ldx 2 + 2 K below
//                2^32, so no sum of offsets wraps.
// A row of the MFMA's output reads its own B column only, so neither the dead rows nor the other rows of a tile change
// a row's bits.
//
// This header holds the weight description and the helpers; the tile's statements are wq_stream_tile_body.h, which
// each of the two kernels includes as its body (it reads the kernel's INT4 / DT / ZP / MT, a constexpr bool MOE, p, m0
// and x_rows).  A function template around the same statements was tried first: inlined into wq_stream_kernel it moved
// the int8 instances' register allocation both ways (8 m-tiles 186 -> 132 VGPRs, 6 m-tiles with a zero-point 132 ->
// 202), and wq.hip's kernels are to stay what was measured.  As text in the kernel's body every wq.hip kernel compiles
// to the ISA it had, line for line (profiles/wq_moe_wide_isa_wq_parent_vs_new.txt).
// Everything sits in an unnamed namespace: each translation unit gets its own copy, and wq.hip's kernels keep the
// symbol names they had while these definitions stood in that file.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own unless written as __builtin_fmaf.
#pragma once
#include "common.h"

namespace {

constexpr int WQ_THREADS = 256;
constexpr int WQ_WAVES = WQ_THREADS / 64;
constexpr int WQ_KB = 128;      // columns per k-block (= the weight group)
constexpr int WQ_UNROLL = 4;    // k-blocks in flight per wave

struct WqArgs {
    const unsigned short* X;
    int64_t ldx;
    int M;
    const void* Wq;
    int N, K, Kw;               // Kw: int32 words per packed row (int4)
    const float* s_w;
    int G;
    const int8_t* zp_w;
    const int32_t* g_idx;
    const unsigned short* bias;
    unsigned short* Y;          // Y (GEMV) or W (dequantise)
    int64_t ldy;
    int vec;                    // 16-byte weight / activation / output accesses are aligned and in bounds
    // grouped forms only (qt_gemm_wq_grouped, qt_moe_gemm_wq_wide): M is the routed-row count R; expert e owns output
    // rows [offsets[e], offsets[e + 1]) and weight matrix e; X row of output row m is row_idx[m] (or m when NULL)
    const int32_t* offsets;
    const int32_t* row_idx;
    int E;
};

template <int DT>
__device__ __forceinline__ unsigned pack2(float a, float b) {
    if constexpr (DT == QT_F16) {
        const unsigned lo = __builtin_bit_cast(unsigned short, (_Float16)a);
        const unsigned hi = __builtin_bit_cast(unsigned short, (_Float16)b);
        return lo | (hi << 16);
    } else {
        const unsigned lo = __builtin_bit_cast(unsigned short, (__bf16)a);
        const unsigned hi = __builtin_bit_cast(unsigned short, (__bf16)b);
        return lo | (hi << 16);
    }
}

template <int DT>
__device__ __forceinline__ float h2f(unsigned short h) {
    return DT == QT_F16 ? qt_f16_to_f32(h) : qt_bf16_to_f32(h);
}

// The group of column c and its scale / zero-point offset.  cz = OFF + zp: the stored level plus OFF is the unsigned
// value u the kernels convert (u - cz = q - zp exactly).  g_idx values are clamped to [0, G).
template <bool INT4, bool ZP, bool GIDX>
__device__ __forceinline__ void group_params(const WqArgs& p, int64_t n, int c, float& s, float& cz) {
    int g;
    if constexpr (GIDX) {
        g = p.g_idx[c];
        g = min(max(g, 0), p.G - 1);
    } else {
        g = p.G == 1 ? 0 : c / WQ_KB;
    }
    s = p.s_w[n * p.G + g];
    cz = INT4 ? 8.0f : 128.0f;
    if constexpr (ZP) cz = cz + (float)p.zp_w[n * p.G + g];
}

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// a once-read 16-byte weight chunk: non-temporal load (MI355X_MICROARCH nt-weights)
__device__ __forceinline__ uint4 ld_nt16(const void* p) {
    const u32x4 v = __builtin_nontemporal_load((const u32x4*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

template <int DT>
__device__ __forceinline__ f32x4 mfma16(const u32x4 a, const u32x4 b, f32x4 c) {
    if constexpr (DT == QT_F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0,
                                                      0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                       0, 0, 0);
}

// The A fragment of one MFMA step: 8 consecutive weight columns, w = round_to_dtype(dequantised value).
// Without a zero-point the value is fma(u, s, -OFF s): -OFF s is exact (OFF a power of two), so this is one rounding
// of q s, the same value as (u - OFF) * s.  With a zero-point: (u - cz) * s, the difference exact.
template <int DT, bool ZP>
__device__ __forceinline__ u32x4 frag_from_u(const float (&u)[8], float s, float cz, float noff) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if constexpr (ZP) {
            const float t = u[j] - cz;
            f[j] = t * s;
        } else {
            f[j] = __builtin_fmaf(u[j], s, noff);
        }
    }
    return (u32x4){pack2<DT>(f[0], f[1]), pack2<DT>(f[2], f[3]), pack2<DT>(f[4], f[5]), pack2<DT>(f[6], f[7])};
}

// one packed word (8 int4 columns) -> u values in column order (nibble j = column j)
__device__ __forceinline__ void u_int4(unsigned w, float (&u)[8]) {
    const unsigned lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u[2 * i] = (float)((lo >> (8 * i)) & 0xffu);       // v_cvt_f32_ubyte{i}
        u[2 * i + 1] = (float)((hi >> (8 * i)) & 0xffu);
    }
}

// two dwords (8 int8 columns) -> u = level + 128
__device__ __forceinline__ void u_int8(unsigned a, unsigned b, float (&u)[8]) {
    a ^= 0x80808080u;
    b ^= 0x80808080u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u[i] = (float)((a >> (8 * i)) & 0xffu);
        u[4 + i] = (float)((b >> (8 * i)) & 0xffu);
    }
}

constexpr int WQ_XB = 4;        // activation fragment sets resident per wave: the one in use and WQ_XB - 1 in flight

template <int V>
struct WqInt {
    static constexpr int value = V;
};

}  // namespace
