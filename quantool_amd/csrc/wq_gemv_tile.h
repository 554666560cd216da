// The row-stream A16 GEMV body, stated once for its two kernels: wq_gemv_kernel (one weight) and
// wq_gemv_act_mul_kernel (gate and up of a gated MLP against one x), both in wq_gemv.hip, whose head comment gives the
// layout, the summation order and the bounds.  include/quantool_amd.h, "A16 runtime"; DESIGN.md 4.32.
//
// The weight values are formed by wq_stream_tile.h's statements (group_params, u_int4 / u_int8, frag_from_u): eight
// consecutive columns become four dwords of 16-bit pairs w = round_to_dtype((q - zp) s), in column order, which is the
// order of x in memory, so a dword of weights meets a dword of activations in one v_dot2_f32_{bf16,f16}.
// Everything sits in an unnamed namespace, as wq_stream_tile.h's definitions do.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own unless written as __builtin_fmaf.
#pragma once
#include "common.h"
#include "wq_fused_tile.h"

namespace {

constexpr int GV_ROWS = 4;                      // weight rows per workgroup: R
constexpr int GV_WAVES = 4;                     // K is split over the waves of a workgroup
constexpr int GV_THREADS = 64 * GV_WAVES;
static_assert(QT_WQ_GEMV_K_UNIT == WQ_KB, "a wave's K-range is a whole number of weight groups");

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// c + w.lo x.lo + w.hi x.hi on two 16-bit pairs: the products are exact in fp32, the sum is the instruction's own
template <int DT>
__device__ __forceinline__ float gv_dot2(unsigned w2, unsigned x2, float c) {
    if constexpr (DT == QT_F16)
        return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, w2), __builtin_bit_cast(f16x2, x2), c, false);
    else
        return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w2), __builtin_bit_cast(bf16x2, x2), c, false);
}

// a lane's once-read piece of a weight row: WD dwords, non-temporal
template <int WD>
__device__ __forceinline__ void gv_ld_piece(const void* src, unsigned (&d)[WD]) {
    static_assert(WD == 1 || WD == 2 || WD == 4, "4-, 8- or 16-byte pieces");
    if constexpr (WD == 4) {
        const uint4 v = ld_nt16(src);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    } else if constexpr (WD == 2) {
        const u32x2 v = __builtin_nontemporal_load((const u32x2*)src);
        d[0] = v.x, d[1] = v.y;
    } else {
        d[0] = __builtin_nontemporal_load((const unsigned*)src);
    }
}

// How wide a lane's piece is, in units of 8 columns, for a weight of K columns: the widest (16 bytes) whose slab of
// 64 pieces still fits the K-range of a wave, so that no wave is half idle at K = 4096 split four ways.
static inline int gv_units(bool int4, int K) {
    const int range = ((K / WQ_KB + GV_WAVES - 1) / GV_WAVES) * WQ_KB;
    int U = int4 ? 4 : 2;
    while (U > 1 && 64 * 8 * U > range) U >>= 1;
    return U;
}

// This wave's partial sums of M activation rows (M <= 4, rows of X, pitch ldx) times rows [n0, n0 + GV_ROWS) of each
// of NW weights of one format and G.  Wave v walks the k-blocks [nkb v / 4, nkb (v + 1) / 4) in slabs of 64 pieces of
// 8 U columns; lane l's piece of a slab starts at column slab + 8 U l and lies inside one weight group.  acc[i][r][m]
// is one fp32 chain per lane: slabs ascending, the piece's columns ascending in pairs.  A lane whose piece starts
// past the range loads nothing and adds nothing; a weight row n >= N re-reads row N - 1 (never stored).
template <bool INT4, int DT, bool ZP, int M, int U, int NW>
__device__ __forceinline__ void gv_rows(const unsigned short* X, int64_t ldx, int K, int G, int N,
                                        const FusedW (&w)[NW], int64_t n0, float (&acc)[NW][GV_ROWS][M]) {
    static_assert(M >= 1 && M <= QT_WQ_GEMV_MAX_M && (U == 1 || U == 2 || (U == 4 && INT4)), "piece of at most 16 bytes");
    constexpr int PC = 8 * U;                   // columns per piece
    constexpr int SLAB = 64 * PC;
    constexpr int WD = INT4 ? U : 2 * U;        // dwords per piece
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nkb = K / WQ_KB;
    const int cbeg = (int)((int64_t)nkb * wave / GV_WAVES) * WQ_KB;
    const int cend = (int)((int64_t)nkb * (wave + 1) / GV_WAVES) * WQ_KB;
    const float off = INT4 ? 8.0f : 128.0f;

    WqArgs p[NW];                               // group_params' view of each weight
    const char* row[NW][GV_ROWS];
    int64_t nrow[GV_ROWS];
#pragma unroll
    for (int r = 0; r < GV_ROWS; ++r) nrow[r] = n0 + r < N ? n0 + r : (int64_t)N - 1;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        p[i] = WqArgs{};
        p[i].s_w = w[i].s_w;
        p[i].zp_w = w[i].zp_w;
        p[i].G = G;
#pragma unroll
        for (int r = 0; r < GV_ROWS; ++r) {
            row[i][r] = (const char*)w[i].Wq + nrow[r] * (INT4 ? K / 2 : K);
#pragma unroll
            for (int m = 0; m < M; ++m) acc[i][r][m] = 0.0f;
        }
    }

    unsigned cur[NW][GV_ROWS][WD] = {};
    if (cbeg + lane * PC < cend) {
#pragma unroll
        for (int i = 0; i < NW; ++i)
#pragma unroll
            for (int r = 0; r < GV_ROWS; ++r) gv_ld_piece<WD>(row[i][r] + (cbeg + lane * PC) / (INT4 ? 2 : 1), cur[i][r]);
    }
    for (int cs = cbeg; cs < cend; cs += SLAB) {
        const int c = cs + lane * PC;
        unsigned nxt[NW][GV_ROWS][WD] = {};
        if (c < cend - SLAB) {                  // the next slab's pieces are in flight under this slab's arithmetic
#pragma unroll
            for (int i = 0; i < NW; ++i)
#pragma unroll
                for (int r = 0; r < GV_ROWS; ++r) gv_ld_piece<WD>(row[i][r] + (c + SLAB) / (INT4 ? 2 : 1), nxt[i][r]);
        }
        if (c < cend) {
            float s[NW][GV_ROWS], cz[NW][GV_ROWS];
#pragma unroll
            for (int i = 0; i < NW; ++i)
#pragma unroll
                for (int r = 0; r < GV_ROWS; ++r) group_params<INT4, ZP, false>(p[i], nrow[r], c, s[i][r], cz[i][r]);
#pragma unroll
            for (int j = 0; j < U; ++j) {
                uint4 xv[M];                    // 8 columns of every activation row, shared by the NW x R weight rows
#pragma unroll
                for (int m = 0; m < M; ++m) xv[m] = *(const uint4*)(X + (int64_t)m * ldx + c + 8 * j);
#pragma unroll
                for (int i = 0; i < NW; ++i) {
#pragma unroll
                    for (int r = 0; r < GV_ROWS; ++r) {
                        float uu[8];
                        if constexpr (INT4) u_int4(cur[i][r][j], uu);
                        else u_int8(cur[i][r][2 * j], cur[i][r][2 * j + 1], uu);
                        const u32x4 a = frag_from_u<DT, ZP>(uu, s[i][r], cz[i][r], -(off * s[i][r]));
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            float v = acc[i][r][m];
                            v = gv_dot2<DT>(a.x, xv[m].x, v);
                            v = gv_dot2<DT>(a.y, xv[m].y, v);
                            v = gv_dot2<DT>(a.z, xv[m].z, v);
                            v = gv_dot2<DT>(a.w, xv[m].w, v);
                            acc[i][r][m] = v;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NW; ++i)
#pragma unroll
            for (int r = 0; r < GV_ROWS; ++r)
#pragma unroll
                for (int d = 0; d < WD; ++d) cur[i][r][d] = nxt[i][r][d];
    }
}

// Lane partials by a fixed xor tree (32, 16, ..., 1), then the wave's sums into red[wave][(i R + r) M + m]; the
// barrier is inside.  gv_sum adds the waves' sums in wave order.
template <int M, int NW>
__device__ __forceinline__ void gv_reduce(const float (&acc)[NW][GV_ROWS][M], float (*red)[NW * GV_ROWS * M]) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NW; ++i)
#pragma unroll
        for (int r = 0; r < GV_ROWS; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float v = acc[i][r][m];
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
                if (lane == 0) red[wave][(i * GV_ROWS + r) * M + m] = v;
            }
    __syncthreads();
}
template <int W>
__device__ __forceinline__ float gv_sum(const float (*red)[W], int t) {
    float v = red[0][t];
#pragma unroll
    for (int wv = 1; wv < GV_WAVES; ++wv) v = v + red[wv][t];
    return v;
}

}  // namespace
