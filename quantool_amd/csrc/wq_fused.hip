// The A16 decode GEMV over more than one weight that reads one input (include/quantool_amd.h, "A16 runtime";
// DESIGN.md 4.27).  1 <= M <= 16, K a multiple of 128, the skinny kernel's 16-byte path only.
//
// qt_gemm_wq_skinny_act_mul  H = SiLU(x Wg^T) * (x Wu^T).  A workgroup owns 16 columns n of the gate weight and the same
//                            16 columns of the up weight; its 4 waves split the 128-column k-blocks as wq_skinny_kernel
//                            does (k-block kb to wave kb % 4, ascending).  A wave loads its activation fragment once per
//                            k-block and feeds it to two v_mfma_f32_16x16x32_{bf16,f16} chains, one fp32 accumulator
//                            each.  Both accumulators go through LDS, ((c0 + c1) + c2) + c3 each; g and u are rounded
//                            once to the activation dtype and h16_act.h's silu_mul makes h: what torch's SiLU and
//                            multiply leave of the two skinny GEMVs' outputs, to the bit.
// qt_gemm_wq_skinny_multi    up to QT_WQ_MULTI_MAX weights (q/k/v) in one launch: the grid's x dimension is the sum of
//                            the weights' column tiles, and a workgroup finds its weight in a by-value table of tile
//                            starts.  One accumulator; output i equals qt_gemm_wq_skinny on weight i to the bit.
//
// Both run one tile: wq_fused_tile.h's wq_tile<NW>, the skinny kernel's 16-byte loop over NW weights that share the B
// fragment, so chain w of weight i is the chain wq_skinny_kernel's wave w runs on it.
// No bias in the paired form, no workspace, no atomics.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own unless written as __builtin_fmaf.
#include "common.h"
#include "h16_act.h"
#include "wq_fused_tile.h"

namespace {

// the lane's activation row of a dense X: row lane & 15, row 0 for a lane past M (wq_tile drops what it reads)
__device__ __forceinline__ const unsigned short* dense_xrow(const unsigned short* X, int64_t ldx, int M) {
    const int r = threadIdx.x & 15;
    return X + (int64_t)(r < M ? r : 0) * ldx;
}

// ---- qt_gemm_wq_skinny_act_mul --------------------------------------------------------------------------------------
template <bool INT4, int DT, bool ZP>
__global__ void __launch_bounds__(WQ_THREADS) wq_act_mul_kernel(const unsigned short* X, int64_t ldx, int M, int K,
                                                                int G, int N, const FusedW gate, const FusedW up,
                                                                unsigned short* H, int64_t ldh) {
    __shared__ f32x4 red[2][WQ_WAVES - 1][64];
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    const FusedW w[2] = {gate, up};
    f32x4 acc[2];
    wq_tile<INT4, DT, ZP, 2>(dense_xrow(X, ldx, M), M, K, G, N, w, n0, acc);

    wq_reduce_store(red[0], acc[0]);
    wq_reduce_store(red[1], acc[1]);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    if (threadIdx.x < 64 && r < M) {
        const f32x4 g = wq_reduce_sum(red[0], acc[0]);
        const f32x4 u = wq_reduce_sum(red[1], acc[1]);
        constexpr bool F16 = DT == QT_F16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t nn = n0 + 4 * kq + i;
            if (nn >= N) continue;
            H[(int64_t)r * ldh + nn] = silu_mul<F16>(to_h16<F16>(g[i]), to_h16<F16>(u[i]));
        }
    }
}

// ---- qt_gemm_wq_skinny_multi ----------------------------------------------------------------------------------------
constexpr int MULTI_MAX = QT_WQ_MULTI_MAX;

// By value in the kernel arguments; read through compile-time indices only (a run-time index into a by-value struct
// puts it in scratch, csrc/build.py).
struct MultiTable {
    FusedW w[MULTI_MAX];
    const unsigned short* bias[MULTI_MAX];
    unsigned short* Y[MULTI_MAX];
    int64_t ldy[MULTI_MAX];
    int N[MULTI_MAX];
    int tile0[MULTI_MAX];               // first column tile of weight i; unused entries hold the grid size
};

template <bool INT4, int DT, bool ZP>
__global__ void __launch_bounds__(WQ_THREADS) wq_multi_kernel(const unsigned short* X, int64_t ldx, int M, int K, int G,
                                                              const MultiTable t) {
    __shared__ f32x4 red[WQ_WAVES - 1][64];
    const int tile = blockIdx.x;
    FusedW w[1] = {t.w[0]};
    const unsigned short* bias = t.bias[0];
    unsigned short* Y = t.Y[0];
    int64_t ldy = t.ldy[0];
    int N = t.N[0];
    int first = 0;
#pragma unroll
    for (int i = 1; i < MULTI_MAX; ++i) {
        if (tile >= t.tile0[i]) {       // uniform; tile0 ascends
            w[0] = t.w[i];
            bias = t.bias[i];
            Y = t.Y[i];
            ldy = t.ldy[i];
            N = t.N[i];
            first = t.tile0[i];
        }
    }
    const int64_t n0 = (int64_t)(tile - first) * 16;
    f32x4 acc[1];
    wq_tile<INT4, DT, ZP, 1>(dense_xrow(X, ldx, M), M, K, G, N, w, n0, acc);

    wq_reduce_store(red, acc[0]);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    if (threadIdx.x < 64 && r < M) {
        const f32x4 c = wq_reduce_sum(red, acc[0]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t nn = n0 + 4 * kq + i;
            if (nn >= N) continue;
            float y = c[i];
            if (bias) y = y + h2f<DT>(bias[nn]);
            Y[(int64_t)r * ldy + nn] = (unsigned short)(pack2<DT>(y, 0.0f) & 0xffffu);
        }
    }
}

// The conditions both entry points share, on X and on one weight; `what` names the weight in the message.
int check_x(const char* fn, const void* X, int x_dtype, int M, int K, int64_t ldx) {
    QT_CHECK_ARG(X, "%s: X is null", fn);
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "%s: x_dtype %d must be bf16 or fp16", fn, x_dtype);
    QT_CHECK_ARG(M >= 1 && M <= QT_WQ_FUSED_MAX_M, "%s: 1 <= M <= %d rows only, got M = %d", fn, QT_WQ_FUSED_MAX_M, M);
    QT_CHECK_ARG(K >= 1 && K % QT_WQ_FUSED_K_UNIT == 0, "%s: K = %d is not a multiple of the k-unit %d", fn, K,
                 QT_WQ_FUSED_K_UNIT);
    QT_CHECK_ARG(ldx >= K, "%s: ldx %lld is below K %d", fn, (long long)ldx, K);
    QT_CHECK_ARG(((uintptr_t)X & 15) == 0 && ldx % 8 == 0, "%s: X and its row pitch must be 16-byte aligned", fn);
    return QT_OK;
}

int check_w(const char* fn, const char* what, const void* Wq, int w_format, int N, int K, const float* s_w, int G,
            const int32_t* g_idx) {
    QT_CHECK_ARG(Wq && s_w, "%s: %s: null pointer (Wq and s_w are required)", fn, what);
    QT_CHECK_ARG(g_idx == nullptr, "%s: %s: g_idx is not taken (actorder group runs on qt_gemm_wq_skinny)", fn, what);
    QT_CHECK_ARG(w_format == QT_W_INT8 || w_format == QT_W_INT4_PACKED, "%s: %s: w_format %d unsupported", fn, what,
                 w_format);
    QT_CHECK_ARG(N >= 1, "%s: %s: empty weight (N = %d)", fn, what, N);
    QT_CHECK_ARG(G == 1 || G == K / QT_WQ_FUSED_K_UNIT, "%s: %s: G must be 1 or K / %d = %d, got %d", fn, what,
                 QT_WQ_FUSED_K_UNIT, K / QT_WQ_FUSED_K_UNIT, G);
    QT_CHECK_ARG(((uintptr_t)Wq & 15) == 0, "%s: %s: Wq must be 16-byte aligned", fn, what);
    return QT_OK;
}

}  // namespace

extern "C" int qt_gemm_wq_skinny_act_mul(const void* X, int x_dtype, int M, int K, int64_t ldx, const qt_wq_weight* gate,
                                         const qt_wq_weight* up, int act, void* H, int64_t ldh, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* fn = "qt_gemm_wq_skinny_act_mul";
    QT_CHECK_ARG(gate && up && H, "%s: null pointer (gate, up and H are required)", fn);
    if (int e = check_x(fn, X, x_dtype, M, K, ldx)) return e;
    if (int e = check_w(fn, "gate", gate->Wq, gate->w_format, gate->N, K, gate->s_w, gate->G, gate->g_idx)) return e;
    if (int e = check_w(fn, "up", up->Wq, up->w_format, up->N, K, up->s_w, up->G, up->g_idx)) return e;
    QT_CHECK_ARG(act == QT_ACT_SILU, "%s: unknown act %d", fn, act);
    QT_CHECK_ARG(gate->w_format == up->w_format && gate->G == up->G && gate->N == up->N &&
                     (gate->zp_w != nullptr) == (up->zp_w != nullptr),
                 "%s: gate and up differ in format, N, G or zero-point presence", fn);
    QT_CHECK_ARG(!gate->bias && !up->bias && !gate->Y && !up->Y, "%s: no bias and no Y (H is the one output)", fn);
    QT_CHECK_ARG(ldh >= gate->N, "%s: ldh %lld is below I %d", fn, (long long)ldh, gate->N);
    const bool int4 = gate->w_format == QT_W_INT4_PACKED;
    const bool zp = gate->zp_w != nullptr;
    const FusedW g{gate->Wq, gate->s_w, gate->zp_w}, u{up->Wq, up->s_w, up->zp_w};
    const dim3 grid((unsigned)(((int64_t)gate->N + 15) / 16));
#define QT_WQ_FUSED_CASE(I4, D, Z)                                                                             \
    if (int4 == I4 && x_dtype == D && zp == Z)                                                                 \
        hipLaunchKernelGGL((wq_act_mul_kernel<I4, D, Z>), grid, dim3(WQ_THREADS), 0, stream,                   \
                           (const unsigned short*)X, ldx, M, K, gate->G, gate->N, g, u, (unsigned short*)H, ldh);
    QT_WQ_FUSED_CASE(true, QT_BF16, false) QT_WQ_FUSED_CASE(true, QT_BF16, true)
    QT_WQ_FUSED_CASE(true, QT_F16, false) QT_WQ_FUSED_CASE(true, QT_F16, true)
    QT_WQ_FUSED_CASE(false, QT_BF16, false) QT_WQ_FUSED_CASE(false, QT_BF16, true)
    QT_WQ_FUSED_CASE(false, QT_F16, false) QT_WQ_FUSED_CASE(false, QT_F16, true)
#undef QT_WQ_FUSED_CASE
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_gemm_wq_skinny_multi(const void* X, int x_dtype, int M, int K, int64_t ldx,
                                       const qt_wq_weight* weights, int count, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* fn = "qt_gemm_wq_skinny_multi";
    QT_CHECK_ARG(weights && count >= 1 && count <= QT_WQ_MULTI_MAX, "%s: 1 <= count <= %d weights, got %d", fn,
                 QT_WQ_MULTI_MAX, count);
    if (int e = check_x(fn, X, x_dtype, M, K, ldx)) return e;
    MultiTable t{};
    int64_t tiles = 0;
    for (int i = 0; i < count; ++i) {
        const qt_wq_weight& w = weights[i];
        char what[16];
        snprintf(what, sizeof what, "weight %d", i);
        if (int e = check_w(fn, what, w.Wq, w.w_format, w.N, K, w.s_w, w.G, w.g_idx)) return e;
        QT_CHECK_ARG(w.w_format == weights[0].w_format && w.G == weights[0].G &&
                         (w.zp_w != nullptr) == (weights[0].zp_w != nullptr),
                     "%s: %s differs from weight 0 in format, G or zero-point presence", fn, what);
        QT_CHECK_ARG(w.Y && w.ldy >= w.N, "%s: %s: Y is null or ldy %lld is below N %d", fn, what, (long long)w.ldy,
                     w.N);
        t.w[i] = FusedW{w.Wq, w.s_w, w.zp_w};
        t.bias[i] = (const unsigned short*)w.bias;
        t.Y[i] = (unsigned short*)w.Y;
        t.ldy[i] = w.ldy;
        t.N[i] = w.N;
        t.tile0[i] = (int)tiles;
        tiles += ((int64_t)w.N + 15) / 16;
        QT_CHECK_ARG(tiles <= 0x7fffffffLL, "%s: too many column tiles", fn);
    }
    for (int i = count; i < MULTI_MAX; ++i) t.tile0[i] = (int)tiles;   // past every workgroup: never selected
    const bool int4 = weights[0].w_format == QT_W_INT4_PACKED;
    const bool zp = weights[0].zp_w != nullptr;
    const int G = weights[0].G;
    const dim3 grid((unsigned)tiles);
#define QT_WQ_FUSED_CASE(I4, D, Z)                                                                             \
    if (int4 == I4 && x_dtype == D && zp == Z)                                                                 \
        hipLaunchKernelGGL((wq_multi_kernel<I4, D, Z>), grid, dim3(WQ_THREADS), 0, stream,                     \
                           (const unsigned short*)X, ldx, M, K, G, t);
    QT_WQ_FUSED_CASE(true, QT_BF16, false) QT_WQ_FUSED_CASE(true, QT_BF16, true)
    QT_WQ_FUSED_CASE(true, QT_F16, false) QT_WQ_FUSED_CASE(true, QT_F16, true)
    QT_WQ_FUSED_CASE(false, QT_BF16, false) QT_WQ_FUSED_CASE(false, QT_BF16, true)
    QT_WQ_FUSED_CASE(false, QT_F16, false) QT_WQ_FUSED_CASE(false, QT_F16, true)
#undef QT_WQ_FUSED_CASE
    QT_LAUNCH_CHECK();
    return QT_OK;
}
