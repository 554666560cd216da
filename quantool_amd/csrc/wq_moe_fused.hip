// SiLU(gate) * up straight from a packed A16 expert bank gate_up [E, 2 I, .] (rows [0, I) of an expert gate, [I, 2 I)
// up): H [R, I] in the activation dtype, the one output (include/quantool_amd.h, "A16 runtime").
//
// qt_gemm_wq_grouped_act_mul   the decode form, the pair form of wq_skinny_kernel<..., MOE>: grid (column tiles of I,
//                              slots), one slot per 16 rows of one expert.  A workgroup walks offsets as the grouped
//                              kernel does (clamped, a surplus slot returning before its first weight load and its
//                              barrier), gathers its rows through row_idx and runs wq_fused_tile.h's wq_tile<NW = 2> on
//                              rows e 2 I + n and e 2 I + I + n of the bank: one activation fragment per k-block, two
//                              MFMA chains, one fp32 accumulator each.
// qt_moe_gemm_wq_wide_act_mul  the batched-decode form, the pair form of moe_gemm_wq_wide_kernel: MT m-tiles of 16 rows
//                              of one expert per workgroup on wq_stream_pair_tile.h's tile, 2 MT accumulators per wave;
//                              MT from R and E alone, as qt_moe_gemm_wq_wide chooses it.
//
// Both epilogues: every accumulator goes through LDS, ((c0 + c1) + c2) + c3; g and u are rounded once to the
// activation dtype and h16_act.h's silu_mul makes h.  Chain w of each half is the chain qt_gemm_wq_grouped runs on
// that row and expert, and silu_mul is torch's SiLU and multiply on 16-bit values, so H is what act_fn(gate) * up
// leaves of qt_gemm_wq_grouped's output, to the bit.
//
// The column bound of both halves is I, not 2 I: each half is handed to the tile as a weight of I rows of its own, so
// a gate row past I is level-0 fill and never the first up rows, and an up row past I never expert e + 1's gate rows.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own unless written as __builtin_fmaf.
#include "common.h"
#include "h16_act.h"
#include "wq_fused_tile.h"
#include "wq_stream_pair_tile.h"

static_assert(QT_MOE_WQ_WIDE_K_UNIT == WQ_KB, "the tile's k-block is the form's k-unit");

namespace {

// By value in the kernel arguments, never modified and never indexed at run time (csrc/build.py on scratch).
struct PairArgs {
    const unsigned short* X;
    int64_t ldx, x_rows;
    const int32_t* row_idx;
    const int32_t* offsets;
    int R, E;
    const void* Wq;             // gate_up [E, 2 I, K / 8 words or K bytes]
    const float* s_w;           // [E, 2 I, G]
    const int8_t* zp_w;         // [E, 2 I, G] or null
    int I, K, G;
    unsigned short* H;
    int64_t ldh;
};

// slot -> (expert e, first row m0, live rows <= TILE); offsets clamped to [0, R] so a bad table cannot move a write
// out of H.  False for a surplus slot (uniform over the workgroup).
template <int TILE>
__device__ __forceinline__ bool slot_walk(const PairArgs& a, int& e, int64_t& m0, int& rows) {
    const int64_t slot = blockIdx.y;
    int64_t start = 0;
    for (int j = 0; j < a.E; ++j) {
        const int64_t lo = min(max((int64_t)a.offsets[j], (int64_t)0), (int64_t)a.R);
        const int64_t hi = min(max((int64_t)a.offsets[j + 1], lo), (int64_t)a.R);
        const int64_t nt = (hi - lo + TILE - 1) / TILE;
        if (slot < start + nt) {
            e = j;
            m0 = lo + (slot - start) * TILE;
            rows = (int)min(hi - m0, (int64_t)TILE);
            return true;
        }
        start += nt;
    }
    return false;
}

// the two halves of expert e: each a weight [I, K] of its own
template <bool INT4, bool ZP>
__device__ __forceinline__ void expert_pair(const PairArgs& a, int e, FusedW (&w)[2]) {
    const int64_t wrow = INT4 ? (int64_t)(a.K / 8) * 4 : (int64_t)a.K;   // bytes per weight row
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t row0 = ((int64_t)e * 2 + i) * a.I;
        w[i].Wq = (const void*)((const char*)a.Wq + row0 * wrow);
        w[i].s_w = a.s_w + row0 * a.G;
        w[i].zp_w = ZP ? a.zp_w + row0 * a.G : nullptr;
    }
}

// ---- qt_gemm_wq_grouped_act_mul -------------------------------------------------------------------------------------
template <bool INT4, int DT, bool ZP>
__global__ void __launch_bounds__(WQ_THREADS) wq_grouped_act_mul_kernel(const PairArgs a) {
    __shared__ f32x4 red[2][WQ_WAVES - 1][64];
    int e = 0, M = 0;
    int64_t m0 = 0;
    if (!slot_walk<16>(a, e, m0, M)) return;    // surplus slot: before any load of the weights and the barrier
    FusedW w[2];
    expert_pair<INT4, ZP>(a, e, w);
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    // the lane's gathered row; a lane past M reads the tile's first row and wq_tile drops it
    const int64_t mm = m0 + (r < M ? r : 0);
    const int64_t row = a.row_idx ? min(max((int64_t)a.row_idx[mm], (int64_t)0), a.x_rows - 1) : mm;
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    f32x4 acc[2];
    wq_tile<INT4, DT, ZP, 2>(a.X + row * a.ldx, M, a.K, a.G, a.I, w, n0, acc);

    wq_reduce_store(red[0], acc[0]);
    wq_reduce_store(red[1], acc[1]);
    __syncthreads();
    if (threadIdx.x < 64 && r < M) {
        const f32x4 g = wq_reduce_sum(red[0], acc[0]);
        const f32x4 u = wq_reduce_sum(red[1], acc[1]);
        constexpr bool F16 = DT == QT_F16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t nn = n0 + 4 * kq + i;
            if (nn >= a.I) continue;
            a.H[(m0 + r) * a.ldh + nn] = silu_mul<F16>(to_h16<F16>(g[i]), to_h16<F16>(u[i]));
        }
    }
}

// ---- qt_moe_gemm_wq_wide_act_mul ------------------------------------------------------------------------------------
template <bool INT4, int DT, bool ZP, int MT>
__global__ void __launch_bounds__(WQ_THREADS) moe_wq_wide_act_mul_kernel(const PairArgs a) {
    __shared__ f32x4 red[WQ_WAVES - 1][2][MT][64];
    int e = 0, M = 0;
    int64_t m0 = 0;
    if (!slot_walk<16 * MT>(a, e, m0, M)) return;   // surplus slot: before any load of the weights and the barrier
    FusedW w[2];
    expert_pair<INT4, ZP>(a, e, w);
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    f32x4 acc[2][MT];
    wq_stream_pair_tile<INT4, DT, ZP, MT>(a.X, a.ldx, a.x_rows, a.row_idx, m0, M, a.K, a.G, a.I, w, n0, acc);

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < MT; ++t) red[wave - 1][i][t][lane] = acc[i][t];
    }
    __syncthreads();
    if (wave == 0) {
        constexpr bool F16 = DT == QT_F16;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int64_t m = 16 * t + r;
            f32x4 g = acc[0][t], u = acc[1][t];
#pragma unroll
            for (int wv = 0; wv < WQ_WAVES - 1; ++wv) {
                const f32x4 og = red[wv][0][t][lane], ou = red[wv][1][t][lane];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    g[i] = g[i] + og[i];
                    u[i] = u[i] + ou[i];
                }
            }
            if (m >= M) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t nn = n0 + 4 * kq + i;
                if (nn >= a.I) continue;
                a.H[(m0 + m) * a.ldh + nn] = silu_mul<F16>(to_h16<F16>(g[i]), to_h16<F16>(u[i]));
            }
        }
    }
}

// The m-tiles a workgroup of the wide pair form holds: qt_moe_gemm_wq_wide's choice from R and E alone.
int wide_mtiles(int64_t R, int E) {
    const int64_t per = (R + E - 1) / E;
    return per <= 16 ? 1 : per <= 32 ? 2 : per <= 64 ? 4 : 8;
}

// Operand rules of both entry points (qt_moe_gemm_wq_wide's), then the launch of the grouped or the wide form.
int run(const char* fn, bool wide, const void* X, int x_dtype, int K, int64_t ldx, const int32_t* row_idx, int64_t R,
        const int32_t* offsets, int E, const void* Wq, int w_format, int N, const float* s_w, int G, const int8_t* zp_w,
        const int32_t* g_idx, void* H, int64_t ldh, int64_t x_rows, hipStream_t stream) {
    QT_CHECK_ARG(X && Wq && s_w && offsets && H, "%s: null pointer (X, offsets, Wq, s_w and H are required)", fn);
    QT_CHECK_ARG(g_idx == nullptr, "%s: g_idx is not taken (an actorder-group bank runs on qt_gemm_wq_grouped and the "
                 "activation in a pass of its own)", fn);
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "%s: x_dtype %d must be bf16 or fp16", fn, x_dtype);
    QT_CHECK_ARG(w_format == QT_W_INT8 || w_format == QT_W_INT4_PACKED, "%s: w_format %d unsupported", fn, w_format);
    QT_CHECK_ARG(N >= 1 && N <= 0x3fffffff && K >= 1, "%s: empty or oversized weight (I = %d, K = %d)", fn, N, K);
    QT_CHECK_ARG(K % QT_MOE_WQ_WIDE_K_UNIT == 0, "%s: K = %d is not a multiple of the k-unit %d", fn, K,
                 QT_MOE_WQ_WIDE_K_UNIT);
    QT_CHECK_ARG(G == 1 || G == K / QT_MOE_WQ_WIDE_K_UNIT, "%s: G must be 1 or K / %d = %d, got %d", fn,
                 QT_MOE_WQ_WIDE_K_UNIT, K / QT_MOE_WQ_WIDE_K_UNIT, G);
    QT_CHECK_ARG(R >= 1 && R <= 0x7fffffffLL && E >= 1 && E <= QT_MOE_WQ_WIDE_MAX_E && x_rows >= 1,
                 "%s: bad sizes (1 <= R < 2^31, 1 <= E <= %d, x_rows >= 1; R = %lld, E = %d, x_rows = %lld)", fn,
                 QT_MOE_WQ_WIDE_MAX_E, (long long)R, E, (long long)x_rows);
    QT_CHECK_ARG(ldx >= K && ldh >= N, "%s: bad pitch (ldx >= K, ldh >= I)", fn);
    QT_CHECK_ARG((((uintptr_t)X | (uintptr_t)Wq) & 15) == 0 && ldx % 8 == 0,
                 "%s: X, Wq and the row pitch of X must be 16-byte aligned", fn);
    QT_CHECK_ARG(x_rows <= (1LL << 32) / (2 * ldx) && x_rows * ldx * 2 + 2 * (int64_t)K < (1LL << 32),
                 "%s: x_rows %lld x ldx %lld x 2 + 2 K reaches 2^32 bytes: a row of X is addressed by a 32-bit offset",
                 fn, (long long)x_rows, (long long)ldx);
    QT_CHECK_ARG(row_idx || x_rows >= R, "%s: x_rows %lld < R %lld without row_idx", fn, (long long)x_rows,
                 (long long)R);
    const int mt = wide ? wide_mtiles(R, E) : 1;
    const int64_t slots = R / (16 * mt) + (E < R ? E : R);
    QT_CHECK_ARG(slots <= QT_MOE_WQ_WIDE_MAX_SLOTS, "%s: %lld row-tile slots (R = %lld, E = %d) exceed the grid's %d", fn,
                 (long long)slots, (long long)R, E, QT_MOE_WQ_WIDE_MAX_SLOTS);
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const bool zp = zp_w != nullptr;
    const PairArgs a{(const unsigned short*)X, ldx, x_rows, row_idx, offsets, (int)R, E, Wq, s_w, zp_w, N, K, G,
                     (unsigned short*)H, ldh};
    const dim3 grid((unsigned)(((int64_t)N + 15) / 16), (unsigned)slots), block(WQ_THREADS);
#define QT_WQ_PAIR_MT(I4, D, Z, T) \
    case T: hipLaunchKernelGGL((moe_wq_wide_act_mul_kernel<I4, D, Z, T>), grid, block, 0, stream, a); break;
#define QT_WQ_PAIR_CASE(I4, D, Z)                                                                              \
    if (int4 == I4 && x_dtype == D && zp == Z) {                                                               \
        if (!wide) hipLaunchKernelGGL((wq_grouped_act_mul_kernel<I4, D, Z>), grid, block, 0, stream, a);       \
        else switch (mt) { QT_WQ_PAIR_MT(I4, D, Z, 1) QT_WQ_PAIR_MT(I4, D, Z, 2) QT_WQ_PAIR_MT(I4, D, Z, 4)   \
                           QT_WQ_PAIR_MT(I4, D, Z, 8) }                                                        \
    }
    QT_WQ_PAIR_CASE(true, QT_BF16, false) QT_WQ_PAIR_CASE(true, QT_BF16, true)
    QT_WQ_PAIR_CASE(true, QT_F16, false) QT_WQ_PAIR_CASE(true, QT_F16, true)
    QT_WQ_PAIR_CASE(false, QT_BF16, false) QT_WQ_PAIR_CASE(false, QT_BF16, true)
    QT_WQ_PAIR_CASE(false, QT_F16, false) QT_WQ_PAIR_CASE(false, QT_F16, true)
#undef QT_WQ_PAIR_CASE
#undef QT_WQ_PAIR_MT
    QT_LAUNCH_CHECK();
    return QT_OK;
}

}  // namespace

extern "C" int qt_gemm_wq_grouped_act_mul(const void* X, int x_dtype, int K, int64_t ldx, const int32_t* row_idx,
                                          int64_t R, const int32_t* offsets, int E, const void* Wq, int w_format, int N,
                                          const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx, void* H,
                                          int64_t ldh, int64_t x_rows, qt_stream_t stream) {
    return run("qt_gemm_wq_grouped_act_mul", false, X, x_dtype, K, ldx, row_idx, R, offsets, E, Wq, w_format, N, s_w, G,
               zp_w, g_idx, H, ldh, x_rows, (hipStream_t)stream);
}

extern "C" int qt_moe_gemm_wq_wide_act_mul(const void* X, int x_dtype, int K, int64_t ldx, const int32_t* row_idx,
                                           int64_t R, const int32_t* offsets, int E, const void* Wq, int w_format,
                                           int N, const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx,
                                           void* H, int64_t ldh, int64_t x_rows, qt_stream_t stream) {
    return run("qt_moe_gemm_wq_wide_act_mul", true, X, x_dtype, K, ldx, row_idx, R, offsets, E, Wq, w_format, N, s_w, G,
               zp_w, g_idx, H, ldh, x_rows, (hipStream_t)stream);
}
