// The weight-streaming 16-column A16 tile over a gate / up pair of one expert: wq_stream_tile_body.h's MOE tile with two
// weights that share every activation fragment (wq_moe_fused.hip, qt_moe_gemm_wq_wide_act_mul).
//
// The workgroup shape, the k-block split (k-block kb of 128 columns to wave kb % 4, ascending), the statements for the
// weight chunk, the group parameters and the A fragment, and the activation descriptor over X [x_rows, ldx] with one
// 32-bit byte offset per m-tile and lane are those of wq_stream_tile_body.h, so accumulator (i, t) of wave w runs the
// chain qt_moe_gemm_wq_wide's wave w runs on weight i and rows [16 t, 16 t + 16).  Per k-block the two A fragment sets
// are formed once and kept for every m-tile; an m-tile's B fragments are loaded once and feed both chains.  A wave
// takes its k-blocks in batches of WQ_PB (then 2, 1 for the rest): half of the single tile's batch, so the weight
// chunks in flight stay at 32 VGPRs for the pair.  The batch length is no part of the summation order.
//
// Unlike the single tile this is a function template: it has one kernel, and no earlier ISA to keep.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own unless written as __builtin_fmaf.
#pragma once
#include "common.h"
#include "wq_fused_tile.h"

namespace {

// acc[i][t]: this wave's partial of weight i (0 gate, 1 up; each [N, K], rows >= N never read: level 0) on rows
// [m0 + 16 t, m0 + 16 t + 16) of the routed order, M <= 16 MT of them live, D[row 4 kq + j][col r] = column n0 + 4 kq + j
// of row 16 t + r.
template <bool INT4, int DT, bool ZP, int MT>
__device__ __forceinline__ void wq_stream_pair_tile(const unsigned short* X, int64_t ldx, int64_t x_rows,
                                                    const int32_t* row_idx, int64_t m0, int M, int K, int G, int N,
                                                    const FusedW (&w)[2], int64_t n0, f32x4 (&acc)[2][MT]) {
    constexpr int WQ_PB = INT4 ? WQ_UNROLL : WQ_UNROLL / 2;   // k-blocks in flight per wave, both weights
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // in an SGPR: the k-block offsets are scalar
    const int r = lane & 15;            // A row (weight row n0 + r) and B column (activation row 16 t + r)
    const int kq = lane >> 4;           // which 32 columns of the k-block
    const int64_t n = n0 + r;
    const bool n_ok = n < N;
    const int64_t nrow = n_ok ? n : 0;
    const int nfull = K / WQ_KB;        // K is a multiple of WQ_KB
    const int Kw = K / 8;
    const float off = INT4 ? 8.0f : 128.0f;
    constexpr int WV = INT4 ? 1 : 2;    // 16-byte weight chunks per lane per k-block
    constexpr unsigned FILL = INT4 ? 0x88888888u : 0x80808080u;   // level 0 of a row past N
    // the lane's byte offset in the one descriptor over X, per m-tile; the descriptor's size for a dead row.  A dead
    // lane reads row_idx at the tile's first row (in bounds) and drops the value.
    const unsigned xsize = (unsigned)((uint64_t)((x_rows - 1) * ldx + K) * 2);
    unsigned xo[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = 16 * t + r;
        const bool m_ok = m < M;
        const int64_t mm = m0 + (m_ok ? m : 0);
        int64_t row = mm;
        if (row_idx) row = min(max((int64_t)row_idx[mm], (int64_t)0), x_rows - 1);
        xo[t] = m_ok ? (unsigned)((uint64_t)(row * ldx + 32 * kq) * 2) : xsize;
    }

    WqArgs p[2];                        // group_params' view of each weight
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        p[i] = WqArgs{};
        p[i].s_w = w[i].s_w;
        p[i].zp_w = w[i].zp_w;
        p[i].G = G;
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[i][t] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    }

    // UC k-blocks kb, kb + 4, ... of this wave: every weight load issued before the first MFMA
    auto batch = [&](const int kb, auto uc) {
        constexpr int UC = decltype(uc)::value;
        constexpr int STEPS = UC * MT;
        uint4 wv[2][UC][WV];
        u32x4 xv[WQ_XB][4];
        float sc[2][UC], cz[2][UC];
        // step j = (k-block u = j / MT, m-tile t = j % MT): its four 16-byte activation loads
        auto load_x = [&](int j, u32x4 (&dst)[4]) {
            const int u = j / MT, t = j % MT;
            const int soff = (kb + u * WQ_WAVES) * (WQ_KB * 2);
            const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)X, 0, (int)xsize, 0x00020000);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                dst[s] = __builtin_bit_cast(u32x4,
                                            __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(xo[t] + 16 * s), soff, 0));
        };
#pragma unroll
        for (int j = 0; j < WQ_XB - 1 && j < STEPS; ++j) load_x(j, xv[j]);
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            const int c0 = (kb + u * WQ_WAVES) * WQ_KB + 32 * kq;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint4* src = INT4 ? (const uint4*)((const int32_t*)w[i].Wq + nrow * Kw + c0 / 8)
                                        : (const uint4*)((const int8_t*)w[i].Wq + nrow * K + c0);
#pragma unroll
                for (int v = 0; v < WV; ++v) wv[i][u][v] = n_ok ? ld_nt16(src + v) : make_uint4(FILL, FILL, FILL, FILL);
                float sv = 0.0f, czv = off;
                if (n_ok) group_params<INT4, ZP, false>(p[i], nrow, c0, sv, czv);
                sc[i][u] = sv;
                cz[i][u] = czv;
            }
        }
#pragma unroll
        for (int u = 0; u < UC; ++u) {
            u32x4 a[2][4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float s = sc[i][u];
                const float noff = -(off * s);
                const unsigned wd[8] = {wv[i][u][0].x, wv[i][u][0].y, wv[i][u][0].z, wv[i][u][0].w,
                                        wv[i][u][WV - 1].x, wv[i][u][WV - 1].y, wv[i][u][WV - 1].z,
                                        wv[i][u][WV - 1].w};
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    float uu[8];
                    if constexpr (INT4) u_int4(wd[s4], uu);
                    else u_int8(wd[2 * s4], wd[2 * s4 + 1], uu);
                    a[i][s4] = frag_from_u<DT, ZP>(uu, s, cz[i][u], noff);
                }
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const int j = u * MT + t;
                if (j + WQ_XB - 1 < STEPS) load_x(j + WQ_XB - 1, xv[(j + WQ_XB - 1) % WQ_XB]);
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    acc[0][t] = mfma16<DT>(a[0][s4], xv[j % WQ_XB][s4], acc[0][t]);
                    acc[1][t] = mfma16<DT>(a[1][s4], xv[j % WQ_XB][s4], acc[1][t]);
                }
            }
        }
    };
    int kb = wave;
    int left = nfull > wave ? (nfull - wave + WQ_WAVES - 1) / WQ_WAVES : 0;   // this wave's k-blocks: kb, kb + 4, ...
    for (; left >= WQ_PB; left -= WQ_PB, kb += WQ_PB * WQ_WAVES) batch(kb, WqInt<WQ_PB>{});
    if constexpr (WQ_PB > 2) {
        if (left & 2) {
            batch(kb, WqInt<2>{});
            kb += 2 * WQ_WAVES;
        }
    }
    if (left & 1) batch(kb, WqInt<1>{});
}

}  // namespace
