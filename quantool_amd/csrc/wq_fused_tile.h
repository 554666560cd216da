// The skinny kernel's 16-byte loop over NW weights that share the B fragment, stated once for wq_fused.hip (the q/k/v
// multi GEMV and the dense SiLU(gate) * up pair) and wq_moe_fused.hip (the pair over a routed-expert bank).
// DESIGN.md 4.27 and 4.31.
//
// The weight fragments are formed by wq_stream_tile.h's statements (group_params, u_int4 / u_int8, frag_from_u),
// batches of WQ_UNROLL k-blocks per wave with every load issued before the first MFMA, a k-block past the end
// re-reading k-block `wave` and multiplying zeros -- so chain w of weight i is the chain wq_skinny_kernel's wave w
// runs on it.  Everything sits in an unnamed namespace, as wq_stream_tile.h's definitions do.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own unless written as __builtin_fmaf.
#pragma once
#include "common.h"
#include "wq_stream_tile.h"

namespace {

// One weight of a launch: what group_params and the loads read of it.
struct FusedW {
    const void* Wq;
    const float* s_w;
    const int8_t* zp_w;
};

// Accumulates M <= 16 activation rows times rows [n0, n0 + 16) of each of the NW weights (all [N, K] of one format
// and G): acc[i] is this wave's partial of weight i, D[row 4 kq + j][col r] = column n0 + 4 kq + j of activation row
// r.  xrow is the lane's activation row r = lane & 15 (any readable row where r >= M: it is replaced by zeros).  A
// weight row n >= N is never read: its lanes hold level 0, whatever lies behind the weight's N-th row.
template <bool INT4, int DT, bool ZP, int NW>
__device__ __forceinline__ void wq_tile(const unsigned short* xrow, int M, int K, int G, int N, const FusedW (&w)[NW],
                                        int64_t n0, f32x4 (&acc)[NW]) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int r = lane & 15;            // A row (weight row n0 + r) and B column (activation row m = r)
    const int kq = lane >> 4;           // which 32 columns of the k-block
    const int64_t n = n0 + r;
    const bool n_ok = n < N;
    const bool m_ok = r < M;
    const int64_t nrow = n_ok ? n : 0;
    const int nkb = K / WQ_KB;
    const int Kw = K / 8;
    const float off = INT4 ? 8.0f : 128.0f;
    constexpr int WV = INT4 ? 1 : 2;    // 16-byte weight chunks per lane per k-block
    constexpr unsigned FILL = INT4 ? 0x88888888u : 0x80808080u;   // level 0 of a row past N

    WqArgs p[NW];                       // group_params' view of each weight
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        p[i] = WqArgs{};
        p[i].s_w = w[i].s_w;
        p[i].zp_w = w[i].zp_w;
        p[i].G = G;
        acc[i] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    }

    for (int kb = wave; kb < nkb; kb += WQ_UNROLL * WQ_WAVES) {
        uint4 wv[NW][WQ_UNROLL][WV];
        uint4 xv[WQ_UNROLL][4];
        float sc[NW][WQ_UNROLL], cz[NW][WQ_UNROLL];
#pragma unroll
        for (int u = 0; u < WQ_UNROLL; ++u) {
            const int kbu = kb + u * WQ_WAVES < nkb ? kb + u * WQ_WAVES : wave;
            const int c0 = kbu * WQ_KB + 32 * kq;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const uint4* src = INT4 ? (const uint4*)((const int32_t*)w[i].Wq + nrow * Kw + c0 / 8)
                                        : (const uint4*)((const int8_t*)w[i].Wq + nrow * K + c0);
#pragma unroll
                for (int v = 0; v < WV; ++v) wv[i][u][v] = n_ok ? ld_nt16(src + v) : make_uint4(FILL, FILL, FILL, FILL);
                float sv = 0.0f, czv = off;
                if (n_ok) group_params<INT4, ZP, false>(p[i], nrow, c0, sv, czv);
                sc[i][u] = sv;
                cz[i][u] = czv;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
                xv[u][s] = m_ok ? *(const uint4*)(xrow + c0 + 8 * s) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < WQ_UNROLL; ++u) {
            const bool live = kb + u * WQ_WAVES < nkb;   // uniform
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                const uint4 x4 = xv[u][s4];
                const u32x4 b = live ? (u32x4){x4.x, x4.y, x4.z, x4.w} : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const float s = live ? sc[i][u] : 0.0f;
                    const float noff = -(off * s);
                    const unsigned wd[8] = {wv[i][u][0].x, wv[i][u][0].y, wv[i][u][0].z, wv[i][u][0].w,
                                            wv[i][u][WV - 1].x, wv[i][u][WV - 1].y, wv[i][u][WV - 1].z,
                                            wv[i][u][WV - 1].w};
                    float uu[8];
                    if constexpr (INT4) u_int4(wd[s4], uu);
                    else u_int8(wd[2 * s4], wd[2 * s4 + 1], uu);
                    const u32x4 a = frag_from_u<DT, ZP>(uu, s, cz[i][u], noff);
                    acc[i] = mfma16<DT>(a, b, acc[i]);
                }
            }
        }
    }
}

// waves 1 .. 3 leave their partial in red; after the barrier wave 0 holds ((c0 + c1) + c2) + c3
__device__ __forceinline__ void wq_reduce_store(f32x4 (*red)[64], const f32x4& acc) {
    const int wave = threadIdx.x >> 6;
    if (wave > 0) red[wave - 1][threadIdx.x & 63] = acc;
}
__device__ __forceinline__ f32x4 wq_reduce_sum(f32x4 (*red)[64], f32x4 acc) {
#pragma unroll
    for (int w = 0; w < WQ_WAVES - 1; ++w) {
        const f32x4 o = red[w][threadIdx.x & 63];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = acc[i] + o[i];
    }
    return acc;
}

}  // namespace
