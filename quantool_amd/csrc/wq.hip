// W4A16 / W8A16 weight-only runtime: the integer weights of an A16 checkpoint stay on the device and are dequantised on
// chip (include/quantool_amd.h, "A16 runtime").
//
// qt_dequantize_weight   one thread per 8 columns of a row: one packed word (int4) or 8 bytes (int8) in, one 16-byte
//                        store out; four such chunks per thread, 256 threads per row piece.  HBM-bound.
// qt_gemm_wq_skinny      the decode GEMV (1 <= M <= 16).  A workgroup owns 16 output columns n (weight rows) and splits
//                        K over its 4 waves (k-block kb of 128 columns goes to wave kb % 4).  Per k-block a lane loads
//                        one 16-byte chunk of its weight row straight into VGPRs (non-temporal: the weights are read
//                        once), dequantises it and feeds v_mfma_f32_16x16x32_{bf16,f16} with M padded to 16 (the
//                        activations are the B operand).  Four k-blocks are in flight per wave before the first MFMA.
//                        The 4 waves' fp32 partials are summed through LDS in wave order: no atomics.
// qt_gemm_wq_stream      the skinny tile over up to 8 m-tiles of 16 rows (M <= 128; the tile is stated in
//                        wq_stream_tile.h and shared with wq_moe_wide.hip): a k-block's weight
//                        chunk is loaded and dequantised once and multiplied with every live m-tile; each m-tile's
//                        accumulator runs the skinny kernel's chain, so every row equals the skinny kernel's to the bit.
// qt_gemm_wq_grouped     the same kernel over E weight matrices (MOE = true): grid (column tiles, slots), one slot per
//                        16-row tile of one expert's rows.  The slot count floor(R/16) + min(E, R) bounds the tiles of
//                        any routing without reading the counts; a workgroup finds its (expert, tile) by walking
//                        offsets and a surplus one returns before its first weight load and its barrier.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own unless written as __builtin_fmaf.
#include "common.h"
#include "wq_stream_tile.h"

namespace {

// unsigned value u = level + OFF of column c of row n (any alignment)
template <bool INT4>
__device__ __forceinline__ float level_u(const WqArgs& p, int64_t n, int c) {
    if constexpr (INT4) {
        const unsigned w = (unsigned)((const int32_t*)p.Wq)[n * p.Kw + (c >> 3)];
        return (float)((w >> (4 * (c & 7))) & 0xfu);
    } else {
        return (float)(((unsigned)(uint8_t)((const int8_t*)p.Wq)[n * p.K + c]) ^ 0x80u);
    }
}

// ---- qt_dequantize_weight -------------------------------------------------------------------------------------------
constexpr int DQ_CHUNKS = 4;    // 8-column chunks per thread

template <bool INT4, int DT, bool ZP, bool GIDX>
__global__ void __launch_bounds__(WQ_THREADS) dequant_kernel(const WqArgs p, int chunks_per_row, int blocks_per_row) {
    const int64_t n = blockIdx.x / blocks_per_row;
    const int base = (blockIdx.x % blocks_per_row) * (WQ_THREADS * DQ_CHUNKS);
    unsigned short* out = p.Y + n * p.ldy;
#pragma unroll
    for (int u = 0; u < DQ_CHUNKS; ++u) {
        const int ch = base + u * WQ_THREADS + threadIdx.x;
        if (ch >= chunks_per_row) break;
        const int c0 = ch * 8;
        if (p.vec && c0 + 8 <= p.K) {
            unsigned v[8];
            if constexpr (INT4) {
                const unsigned w = (unsigned)((const int32_t*)p.Wq)[n * p.Kw + ch];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = (w >> (4 * j)) & 0xfu;
            } else {
                const uint2 b = *(const uint2*)((const int8_t*)p.Wq + n * p.K + c0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = ((b.x >> (8 * j)) & 0xffu) ^ 0x80u;
                    v[4 + j] = ((b.y >> (8 * j)) & 0xffu) ^ 0x80u;
                }
            }
            float s, cz;
            if constexpr (!GIDX) group_params<INT4, ZP, GIDX>(p, n, c0, s, cz);
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (GIDX) group_params<INT4, ZP, GIDX>(p, n, c0 + j, s, cz);
                const float t = (float)v[j] - cz;   // q - zp, exact
                f[j] = t * s;
            }
            *(uint4*)(out + c0) = make_uint4(pack2<DT>(f[0], f[1]), pack2<DT>(f[2], f[3]), pack2<DT>(f[4], f[5]),
                                             pack2<DT>(f[6], f[7]));
        } else {
            for (int c = c0; c < c0 + 8 && c < p.K; ++c) {
                float s, cz;
                group_params<INT4, ZP, GIDX>(p, n, c, s, cz);
                const float t = level_u<INT4>(p, n, c) - cz;
                const float f = t * s;
                out[c] = (unsigned short)(pack2<DT>(f, 0.0f) & 0xffffu);
            }
        }
    }
}

// ---- qt_gemm_wq_skinny ----------------------------------------------------------------------------------------------
// MOE: the grouped form.  blockIdx.y is a slot: the walk over offsets (clamped to [0, R], so a bad table cannot move a
// write out of Y) maps it to expert e and rows [m0, m0 + M) of that expert, M <= 16; the expert's weight, scale,
// zero-point and g_idx rows are then the arguments of the same tile code.  Rows are independent through the MFMA (row m
// of D reads B column m only), so each row equals the skinny kernel's on that expert alone.
template <bool INT4, int DT, bool ZP, bool GIDX, bool MOE = false>
__global__ void __launch_bounds__(WQ_THREADS) wq_skinny_kernel(const WqArgs args) {
    __shared__ f32x4 red[WQ_WAVES - 1][64];
    WqArgs p = args;
    int64_t m0 = 0;                     // output row of activation row 0 of the tile
    if constexpr (MOE) {
        const int64_t slot = blockIdx.y;
        int64_t start = 0;
        int e = -1;
        int64_t hi = 0;
        for (int j = 0; j < p.E; ++j) {
            const int64_t lo = min(max((int64_t)p.offsets[j], (int64_t)0), (int64_t)p.M);
            hi = min(max((int64_t)p.offsets[j + 1], lo), (int64_t)p.M);
            const int64_t nt = (hi - lo + 15) / 16;
            if (slot < start + nt) {
                e = j;
                m0 = lo + (slot - start) * 16;
                break;
            }
            start += nt;
        }
        if (e < 0) return;              // surplus slot (uniform: before any load of the weights and the barrier)
        p.M = (int)min(hi - m0, (int64_t)16);
        const int64_t wrow = INT4 ? (int64_t)p.Kw : (int64_t)p.K;
        p.Wq = INT4 ? (const void*)((const int32_t*)p.Wq + (int64_t)e * p.N * wrow)
                    : (const void*)((const int8_t*)p.Wq + (int64_t)e * p.N * wrow);
        p.s_w += (int64_t)e * p.N * p.G;
        if constexpr (ZP) p.zp_w += (int64_t)e * p.N * p.G;
        if constexpr (GIDX) p.g_idx += (int64_t)e * p.K;
    }
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int r = lane & 15;            // A row (weight row n0 + r) and B column (activation row m = r)
    const int kq = lane >> 4;           // which 32 columns of the k-block
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    const int64_t n = n0 + r;
    const bool n_ok = n < p.N;
    const bool m_ok = r < p.M;
    const int64_t nrow = n_ok ? n : 0;
    int64_t xr = m_ok ? r : 0;
    if constexpr (MOE) xr = p.row_idx ? (int64_t)p.row_idx[m0 + xr] : m0 + xr;
    const unsigned short* xrow = p.X + xr * p.ldx;
    const int nkb = (p.K + WQ_KB - 1) / WQ_KB;
    const int nfull = (GIDX || !p.vec) ? 0 : p.K / WQ_KB;   // k-blocks on the 16-byte path
    const float off = INT4 ? 8.0f : 128.0f;

    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int WV = INT4 ? 1 : 2;    // 16-byte weight chunks per lane per k-block

    // 16-byte path: batches of WQ_UNROLL k-blocks, every load issued before the first MFMA.  A k-block past nfull in
    // the last batch re-reads k-block `wave` (in bounds) and is zeroed before use.
    for (int kb = wave; kb < nfull; kb += WQ_UNROLL * WQ_WAVES) {
        uint4 wv[WQ_UNROLL][WV];
        uint4 xv[WQ_UNROLL][4];
        float sc[WQ_UNROLL], cz[WQ_UNROLL];
#pragma unroll
        for (int u = 0; u < WQ_UNROLL; ++u) {
            const int kbu = kb + u * WQ_WAVES < nfull ? kb + u * WQ_WAVES : wave;
            const int c0 = kbu * WQ_KB + 32 * kq;
            if constexpr (INT4) {
                const uint4* src = (const uint4*)((const int32_t*)p.Wq + nrow * p.Kw + c0 / 8);
                wv[u][0] = n_ok ? ld_nt16(src) : make_uint4(0x88888888u, 0x88888888u, 0x88888888u,
                                                                                 0x88888888u);
            } else {
                const uint4* src = (const uint4*)((const int8_t*)p.Wq + nrow * p.K + c0);
                wv[u][0] = n_ok ? ld_nt16(src) : make_uint4(0x80808080u, 0x80808080u, 0x80808080u,
                                                                                 0x80808080u);
                wv[u][1] = n_ok ? ld_nt16(src + 1)
                                : make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
                xv[u][s] = m_ok ? *(const uint4*)(xrow + c0 + 8 * s) : make_uint4(0u, 0u, 0u, 0u);
            float sv = 0.0f, czv = off;
            if (n_ok) group_params<INT4, ZP, false>(p, nrow, c0, sv, czv);
            sc[u] = sv;
            cz[u] = czv;
        }
#pragma unroll
        for (int u = 0; u < WQ_UNROLL; ++u) {
            const bool live = kb + u * WQ_WAVES < nfull;   // uniform
            const float s = live ? sc[u] : 0.0f;
            const float noff = -(off * s);
            const unsigned wd[8] = {wv[u][0].x, wv[u][0].y, wv[u][0].z, wv[u][0].w, wv[u][WV - 1].x,
                                    wv[u][WV - 1].y, wv[u][WV - 1].z, wv[u][WV - 1].w};
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                float uu[8];
                if constexpr (INT4) u_int4(wd[s4], uu);
                else u_int8(wd[2 * s4], wd[2 * s4 + 1], uu);
                const u32x4 a = frag_from_u<DT, ZP>(uu, s, cz[u], noff);
                const uint4 x4 = xv[u][s4];
                const u32x4 b = live ? (u32x4){x4.x, x4.y, x4.z, x4.w} : (u32x4){0u, 0u, 0u, 0u};
                acc = mfma16<DT>(a, b, acc);
            }
        }
    }
    // element-wise path: the partial last k-block, unaligned operands, or g_idx (a scale per column)
    for (int kb = (nfull > wave ? wave + ((nfull - wave + WQ_WAVES - 1) / WQ_WAVES) * WQ_WAVES : wave); kb < nkb;
         kb += WQ_WAVES) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            float f[8], x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = kb * WQ_KB + 32 * kq + 8 * s4 + j;
                f[j] = 0.0f;
                x[j] = 0.0f;
                if (c < p.K) {
                    if (n_ok) {
                        float s, czv;
                        group_params<INT4, ZP, GIDX>(p, nrow, c, s, czv);
                        const float t = level_u<INT4>(p, nrow, c) - czv;
                        f[j] = t * s;
                    }
                    if (m_ok) x[j] = h2f<DT>(xrow[c]);
                }
            }
            const u32x4 a = {pack2<DT>(f[0], f[1]), pack2<DT>(f[2], f[3]), pack2<DT>(f[4], f[5]), pack2<DT>(f[6], f[7])};
            const u32x4 b = {pack2<DT>(x[0], x[1]), pack2<DT>(x[2], x[3]), pack2<DT>(x[4], x[5]), pack2<DT>(x[6], x[7])};
            acc = mfma16<DT>(a, b, acc);
        }
    }

    // D[row 4 kq + i][col r]: output column n0 + 4 kq + i of activation row r.  y = ((w0 + w1) + w2) + w3 (+ bias)
    if (wave > 0) red[wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0 && m_ok) {
#pragma unroll
        for (int w = 0; w < WQ_WAVES - 1; ++w) {
            const f32x4 o = red[w][lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = acc[i] + o[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t nn = n0 + 4 * kq + i;
            if (nn >= p.N) continue;
            float y = acc[i];
            if (p.bias) y = y + h2f<DT>(p.bias[nn]);
            p.Y[(m0 + r) * p.ldy + nn] = (unsigned short)(pack2<DT>(y, 0.0f) & 0xffffu);
        }
    }
}

// ---- qt_gemm_wq_stream ----------------------------------------------------------------------------------------------
// wq_stream_tile.h's tile on rows [0, M) of X: one instance per tile count MT = ceil(M / 16).
template <bool INT4, int DT, bool ZP, int MT>
__global__ void __launch_bounds__(WQ_THREADS) wq_stream_kernel(const WqArgs p) {
    constexpr bool MOE = false;
    constexpr int64_t m0 = 0, x_rows = 0;
#include "wq_stream_tile_body.h"
}

template <bool I4, int D, bool Z>
void launch_stream(int mtiles, dim3 grid, hipStream_t stream, const WqArgs& a) {
#define QT_WQ_STREAM_MT(T) \
    case T: hipLaunchKernelGGL((wq_stream_kernel<I4, D, Z, T>), grid, dim3(WQ_THREADS), 0, stream, a); break;
    switch (mtiles) {
        QT_WQ_STREAM_MT(1) QT_WQ_STREAM_MT(2) QT_WQ_STREAM_MT(3) QT_WQ_STREAM_MT(4) QT_WQ_STREAM_MT(5)
        QT_WQ_STREAM_MT(6) QT_WQ_STREAM_MT(7) QT_WQ_STREAM_MT(8)
    }
#undef QT_WQ_STREAM_MT
}

template <template <bool, int, bool, bool> class L, typename... A>
void dispatch(bool int4, int dtype, bool zp, bool gidx, A&&... a) {
#define QT_WQ_CASE(I4, D, Z, GI) \
    if (int4 == I4 && dtype == D && zp == Z && gidx == GI) return L<I4, D, Z, GI>::run(a...);
#define QT_WQ_CASES(I4, D) QT_WQ_CASE(I4, D, false, false) QT_WQ_CASE(I4, D, false, true) \
    QT_WQ_CASE(I4, D, true, false) QT_WQ_CASE(I4, D, true, true)
    QT_WQ_CASES(true, QT_BF16) QT_WQ_CASES(true, QT_F16) QT_WQ_CASES(false, QT_BF16) QT_WQ_CASES(false, QT_F16)
#undef QT_WQ_CASES
#undef QT_WQ_CASE
}

template <bool I4, int D, bool Z, bool GI>
struct LaunchDequant {
    static void run(dim3 grid, hipStream_t stream, const WqArgs& a, int chunks, int bpr) {
        hipLaunchKernelGGL((dequant_kernel<I4, D, Z, GI>), grid, dim3(WQ_THREADS), 0, stream, a, chunks, bpr);
    }
};
template <bool I4, int D, bool Z, bool GI>
struct LaunchSkinny {
    static void run(dim3 grid, hipStream_t stream, const WqArgs& a) {
        hipLaunchKernelGGL((wq_skinny_kernel<I4, D, Z, GI>), grid, dim3(WQ_THREADS), 0, stream, a);
    }
};
template <bool I4, int D, bool Z, bool GI>
struct LaunchGrouped {
    static void run(dim3 grid, hipStream_t stream, const WqArgs& a) {
        hipLaunchKernelGGL((wq_skinny_kernel<I4, D, Z, GI, true>), grid, dim3(WQ_THREADS), 0, stream, a);
    }
};

int check_weight(const char* fn, const void* Wq, int w_format, int N, int K, const float* s_w, int G) {
    QT_CHECK_ARG(Wq && s_w && N > 0 && K > 0, "%s: bad weight arguments", fn);
    QT_CHECK_ARG(w_format == QT_W_INT8 || w_format == QT_W_INT4_PACKED, "%s: w_format %d unsupported", fn, w_format);
    QT_CHECK_ARG(G == 1 || G == (K + 127) / 128, "%s: G %d must be 1 or ceil(K / 128) = %d", fn, G, (K + 127) / 128);
    return QT_OK;
}

}  // namespace

extern "C" int qt_dequantize_weight(const void* Wq, int w_format, int N, int K, const float* s_w, int G,
                                    const int8_t* zp_w, const int32_t* g_idx, void* W, int dtype, int64_t ldw,
                                    qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int e = check_weight("qt_dequantize_weight", Wq, w_format, N, K, s_w, G)) return e;
    QT_CHECK_ARG(W && ldw >= K, "qt_dequantize_weight: bad output arguments");
    QT_CHECK_ARG(qt_dtype_is16(dtype), "qt_dequantize_weight: dtype %d must be bf16 or fp16", dtype);
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const int chunks = (K + 7) / 8;
    const int bpr = (chunks + WQ_THREADS * DQ_CHUNKS - 1) / (WQ_THREADS * DQ_CHUNKS);
    QT_CHECK_ARG((int64_t)N * bpr <= 0x7fffffffLL, "qt_dequantize_weight: too many rows");
    const bool vec = ((uintptr_t)W & 15) == 0 && ldw % 8 == 0 && (int4 || (((uintptr_t)Wq & 7) == 0 && K % 8 == 0));
    WqArgs a{nullptr, 0, 0, Wq, N, K, (K + 7) / 8, s_w, G, zp_w, g_idx, nullptr, (unsigned short*)W, ldw, (int)vec,
             nullptr, nullptr, 0};
    dispatch<LaunchDequant>(int4, dtype, zp_w != nullptr, g_idx != nullptr, dim3((unsigned)((int64_t)N * bpr)), stream,
                            a, chunks, bpr);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_gemm_wq_skinny(const void* X, int x_dtype, int M, int K, int64_t ldx, const void* Wq, int w_format,
                                 int N, const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx,
                                 const void* bias, void* Y, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int e = check_weight("qt_gemm_wq_skinny", Wq, w_format, N, K, s_w, G)) return e;
    QT_CHECK_ARG(X && Y && M >= 1 && M <= 16 && ldx >= K && ldy >= N,
                 "qt_gemm_wq_skinny: bad arguments (1 <= M <= 16, ldx >= K, ldy >= N)");
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "qt_gemm_wq_skinny: x_dtype %d must be bf16 or fp16", x_dtype);
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const bool vec = (((uintptr_t)X | (uintptr_t)Wq) & 15) == 0 && ldx % 8 == 0 &&
                     (int4 ? ((K + 7) / 8) % 4 == 0 : K % 16 == 0);
    WqArgs a{(const unsigned short*)X, ldx, M, Wq, N, K, (K + 7) / 8, s_w, G, zp_w, g_idx,
             (const unsigned short*)bias, (unsigned short*)Y, ldy, (int)vec, nullptr, nullptr, 0};
    dispatch<LaunchSkinny>(int4, x_dtype, zp_w != nullptr, g_idx != nullptr, dim3((unsigned)((N + 15) / 16)), stream,
                           a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_gemm_wq_stream(const void* X, int x_dtype, int M, int K, int64_t ldx, const void* Wq, int w_format,
                                 int N, const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx,
                                 const void* bias, void* Y, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(X && Wq && s_w && Y, "qt_gemm_wq_stream: null pointer (X, Wq, s_w and Y are required)");
    QT_CHECK_ARG(g_idx == nullptr,
                 "qt_gemm_wq_stream: g_idx is not taken (actorder group runs on qt_dequantize_weight + a dense GEMM)");
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "qt_gemm_wq_stream: x_dtype %d must be bf16 or fp16", x_dtype);
    QT_CHECK_ARG(w_format == QT_W_INT8 || w_format == QT_W_INT4_PACKED, "qt_gemm_wq_stream: w_format %d unsupported",
                 w_format);
    QT_CHECK_ARG(M >= 1 && M <= QT_WQ_STREAM_MAX_M, "qt_gemm_wq_stream: 1 <= M <= %d rows only, got M = %d",
                 QT_WQ_STREAM_MAX_M, M);
    QT_CHECK_ARG(N >= 1 && K >= 1, "qt_gemm_wq_stream: empty weight (N = %d, K = %d)", N, K);
    QT_CHECK_ARG(K % QT_WQ_STREAM_K_UNIT == 0, "qt_gemm_wq_stream: K = %d is not a multiple of the k-unit %d", K,
                 QT_WQ_STREAM_K_UNIT);
    QT_CHECK_ARG(G == 1 || G == K / QT_WQ_STREAM_K_UNIT, "qt_gemm_wq_stream: G must be 1 or K / %d = %d, got %d",
                 QT_WQ_STREAM_K_UNIT, K / QT_WQ_STREAM_K_UNIT, G);
    QT_CHECK_ARG(ldx >= K && ldy >= N && ldx <= QT_WQ_STREAM_MAX_LDX,
                 "qt_gemm_wq_stream: bad pitch (ldx >= K, ldy >= N, ldx <= %d)", QT_WQ_STREAM_MAX_LDX);
    QT_CHECK_ARG((((uintptr_t)X | (uintptr_t)Wq) & 15) == 0 && ldx % 8 == 0,
                 "qt_gemm_wq_stream: X, Wq and the row pitch of X must be 16-byte aligned");
    const bool int4 = w_format == QT_W_INT4_PACKED;
    WqArgs a{(const unsigned short*)X, ldx, M, Wq, N, K, K / 8, s_w, G, zp_w, nullptr,
             (const unsigned short*)bias, (unsigned short*)Y, ldy, 1, nullptr, nullptr, 0};
    const dim3 grid((unsigned)(((int64_t)N + 15) / 16));
    const int mtiles = (M + 15) / 16;
#define QT_WQ_STREAM_CASE(I4, D, Z) \
    if (int4 == I4 && x_dtype == D && (zp_w != nullptr) == Z) launch_stream<I4, D, Z>(mtiles, grid, stream, a);
    QT_WQ_STREAM_CASE(true, QT_BF16, false) QT_WQ_STREAM_CASE(true, QT_BF16, true)
    QT_WQ_STREAM_CASE(true, QT_F16, false) QT_WQ_STREAM_CASE(true, QT_F16, true)
    QT_WQ_STREAM_CASE(false, QT_BF16, false) QT_WQ_STREAM_CASE(false, QT_BF16, true)
    QT_WQ_STREAM_CASE(false, QT_F16, false) QT_WQ_STREAM_CASE(false, QT_F16, true)
#undef QT_WQ_STREAM_CASE
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_gemm_wq_grouped(const void* X, int x_dtype, int K, int64_t ldx, const int32_t* row_idx, int64_t R,
                                  const int32_t* offsets, int E, const void* Wq, int w_format, int N,
                                  const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx, void* Y,
                                  int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int e = check_weight("qt_gemm_wq_grouped", Wq, w_format, N, K, s_w, G)) return e;
    QT_CHECK_ARG(X && Y && offsets && R > 0 && E > 0 && ldx >= K && ldy >= N,
                 "qt_gemm_wq_grouped: bad arguments (R, E > 0, ldx >= K, ldy >= N)");
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "qt_gemm_wq_grouped: x_dtype %d must be bf16 or fp16", x_dtype);
    QT_CHECK_ARG(R <= 0x7fffffffLL && E <= 4096, "qt_gemm_wq_grouped: R %lld or E %d too large", (long long)R, E);
    const int64_t slots = R / 16 + (E < R ? E : R);
    QT_CHECK_ARG(slots <= 65535, "qt_gemm_wq_grouped: %lld row-tile slots (R = %lld) exceed the grid", (long long)slots,
                 (long long)R);
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const int64_t wrow_bytes = int4 ? (int64_t)((K + 7) / 8) * 4 : (int64_t)K;
    // as qt_gemm_wq_skinny, and every expert's matrix 16-byte aligned as well as the base
    const bool vec = (((uintptr_t)X | (uintptr_t)Wq) & 15) == 0 && ldx % 8 == 0 &&
                     (int4 ? ((K + 7) / 8) % 4 == 0 : K % 16 == 0) && ((int64_t)N * wrow_bytes) % 16 == 0;
    WqArgs a{(const unsigned short*)X, ldx, (int)R, Wq, N, K, (K + 7) / 8, s_w, G, zp_w, g_idx, nullptr,
             (unsigned short*)Y, ldy, (int)vec, offsets, row_idx, E};
    dispatch<LaunchGrouped>(int4, x_dtype, zp_w != nullptr, g_idx != nullptr,
                            dim3((unsigned)((N + 15) / 16), (unsigned)slots), stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
