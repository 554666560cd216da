// W4A16 / W8A16 decode GEMV for 1 .. 4 rows on the vector pipe: qt_gemm_wq_gemv and qt_gemm_wq_gemv_act_mul
// (include/quantool_amd.h, "A16 runtime").  Y[M, N] = X[M, K] W^T (+ bias), M <= QT_WQ_GEMV_MAX_M.
//
// WHY NOT THE SKINNY TILE.  qt_gemm_wq_skinny reads the weight in MFMA fragment shape: a workgroup owns 16 weight rows
// and a wave-load of int4 weights is sixteen 64-byte pieces a row pitch apart; 15 / 16 of each MFMA multiplies padding
// at M = 1.  Here a weight row is a stream: no MFMA, a wave-load of one row is 64 contiguous pieces.
//
// THE LAYOUT.  A workgroup of 4 waves owns GV_ROWS = 4 weight rows n0 .. n0 + 3 and all M activation rows.  Its waves
// split K into contiguous ranges of whole 128-column groups, wave v the k-blocks [nkb v / 4, nkb (v + 1) / 4).  A wave
// walks its range in slabs of 64 pieces; a piece is 8 U consecutive columns of one row (U = 1, 2, 4: 4 / 8 / 16 bytes
// of int4, U = 1, 2: 8 / 16 bytes of int8), so a wave-load of one row is 256 B .. 1 KiB contiguous.  U is chosen on the
// host from K (gv_units: the widest piece whose slab fits a wave's range; K = 4096 takes 8-byte int4 pieces, K = 14336
// 16-byte ones).  A piece is aligned to its size and never crosses a group, so a lane needs one (scale, zero-point)
// per weight row and slab.  All pieces of the next slab are issued before the current slab's arithmetic; weight loads
// are non-temporal.  The activations of a piece's columns come from L2 as 16-byte loads, once per slab and lane, and
// serve the 4 (act_mul: 8) weight rows.
// THE ARITHMETIC.  Eight columns at a time: v_cvt_f32_ubyte* on the masked nibbles / bytes, the exact u - (OFF + zp)
// and one multiply by the scale (without a zero-point: one fma against -OFF s), the pack to 16 bits -- frag_from_u,
// the statements every A16 kernel forms w = round_to_dtype((q - zp) s) with -- then per activation row four
// v_dot2_f32_{bf16,f16} into ONE fp32 accumulator per (weight row, activation row) and lane.  The file is built
// without the packed fp32 instructions (csrc/build.py), as every kernel that shares frag_from_u's values is.
// THE SUM.  Output (m, n): per lane the chain above over its slabs ascending; the 64 lane sums by a fixed xor tree
// (32, 16, 8, 4, 2, 1); the four waves' sums through LDS as ((c0 + c1) + c2) + c3; then the bias in fp32, then one
// rounding.  No atomics, no workspace.  Nothing in that order depends on M, and a chain reads its own activation row
// only: two runs give the same bits and row m of Y is the same for every M that holds it.  The products of two 16-bit
// values are exact in fp32, so inputs whose partial sums are all exact give the exact sum rounded once; otherwise the
// skinny kernel's bound |y - y_exact| <= ulp(y) / 2 + K 2^-24 sum |x w| holds (K / 2 + 8 additions per output).
// The output is NOT bit-equal to qt_gemm_wq_skinny or to F.linear.
// EDGES.  A lane whose piece starts past its wave's range loads nothing and adds nothing (K = 128: three waves idle).
// A weight row past N re-reads row N - 1 and is not stored.  No byte outside X[:M, :K], the weight, its scales /
// zero-points and bias[:N] is read; nothing outside Y[:M, :N] is written.  Row offsets are 64-bit.
//
// wq_gemv_act_mul_kernel: the same body (wq_gemv_tile.h, NW = 2) over the same 4 rows of the gate and of the up weight
// against the one x; both sums go through the same reduction, are rounded to the activation dtype, and h16_act.h's
// silu_mul makes h: what torch's SiLU and multiply leave of the two qt_gemm_wq_gemv outputs, to the bit.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own unless written as __builtin_fmaf.
#include "h16_act.h"
#include "wq_gemv_tile.h"

namespace {

struct GemvArgs {
    const unsigned short* X;
    int64_t ldx;
    int K, G, N;
    FusedW w0, w1;                  // the weight; gate and up in the paired form
    const unsigned short* bias;     // unpaired form only
    unsigned short* Y;              // Y, or H in the paired form
    int64_t ldy;
};

template <bool INT4, int DT, bool ZP, int M, int U>
__global__ void __launch_bounds__(GV_THREADS) wq_gemv_kernel(const GemvArgs p) {
    __shared__ float red[GV_WAVES][GV_ROWS * M];
    const int64_t n0 = (int64_t)blockIdx.x * GV_ROWS;
    const FusedW w[1] = {p.w0};
    float acc[1][GV_ROWS][M];
    gv_rows<INT4, DT, ZP, M, U, 1>(p.X, p.ldx, p.K, p.G, p.N, w, n0, acc);
    gv_reduce<M, 1>(acc, red);
    const int t = threadIdx.x;
    const int64_t n = n0 + t / M;
    if (t < GV_ROWS * M && n < p.N) {
        float y = gv_sum(red, t);
        if (p.bias) y = y + h2f<DT>(p.bias[n]);
        p.Y[(int64_t)(t % M) * p.ldy + n] = (unsigned short)(pack2<DT>(y, 0.0f) & 0xffffu);
    }
}

template <bool INT4, int DT, bool ZP, int M, int U>
__global__ void __launch_bounds__(GV_THREADS) wq_gemv_act_mul_kernel(const GemvArgs p) {
    __shared__ float red[GV_WAVES][2 * GV_ROWS * M];
    const int64_t n0 = (int64_t)blockIdx.x * GV_ROWS;
    const FusedW w[2] = {p.w0, p.w1};
    float acc[2][GV_ROWS][M];
    gv_rows<INT4, DT, ZP, M, U, 2>(p.X, p.ldx, p.K, p.G, p.N, w, n0, acc);
    gv_reduce<M, 2>(acc, red);
    const int t = threadIdx.x;
    const int64_t n = n0 + t / M;
    if (t < GV_ROWS * M && n < p.N) {
        constexpr bool F16 = DT == QT_F16;
        const float g = gv_sum(red, t), u = gv_sum(red, GV_ROWS * M + t);
        p.Y[(int64_t)(t % M) * p.ldy + n] = silu_mul<F16>(to_h16<F16>(g), to_h16<F16>(u));
    }
}

// The instance for (M, U) of one (format, dtype, zero-point) form; U = 4 exists for int4 alone (16-byte pieces).
template <bool PAIR, bool INT4, int DT, bool ZP, int M, int U>
void launch_one(const GemvArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)(((int64_t)a.N + GV_ROWS - 1) / GV_ROWS));
    if constexpr (PAIR)
        hipLaunchKernelGGL((wq_gemv_act_mul_kernel<INT4, DT, ZP, M, U>), grid, dim3(GV_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL((wq_gemv_kernel<INT4, DT, ZP, M, U>), grid, dim3(GV_THREADS), 0, stream, a);
}

template <bool PAIR, bool INT4, int DT, bool ZP, int M>
void launch_u(int U, const GemvArgs& a, hipStream_t stream) {
    if (U == 1) launch_one<PAIR, INT4, DT, ZP, M, 1>(a, stream);
    else if (U == 2) launch_one<PAIR, INT4, DT, ZP, M, 2>(a, stream);
    else if constexpr (INT4) launch_one<PAIR, INT4, DT, ZP, M, 4>(a, stream);
}

template <bool PAIR, bool INT4, int DT, bool ZP>
void launch_m(int M, const GemvArgs& a, hipStream_t stream) {
    const int U = gv_units(INT4, a.K);
    if (M == 1) launch_u<PAIR, INT4, DT, ZP, 1>(U, a, stream);
    else if (M == 2) launch_u<PAIR, INT4, DT, ZP, 2>(U, a, stream);
    else if (M == 3) launch_u<PAIR, INT4, DT, ZP, 3>(U, a, stream);
    else launch_u<PAIR, INT4, DT, ZP, 4>(U, a, stream);
}

template <bool PAIR>
void launch(bool int4, int x_dtype, bool zp, int M, const GemvArgs& a, hipStream_t stream) {
#define QT_WQ_GEMV_CASE(I4, D, Z) \
    if (int4 == I4 && x_dtype == D && zp == Z) launch_m<PAIR, I4, D, Z>(M, a, stream);
    QT_WQ_GEMV_CASE(true, QT_BF16, false) QT_WQ_GEMV_CASE(true, QT_BF16, true)
    QT_WQ_GEMV_CASE(true, QT_F16, false) QT_WQ_GEMV_CASE(true, QT_F16, true)
    QT_WQ_GEMV_CASE(false, QT_BF16, false) QT_WQ_GEMV_CASE(false, QT_BF16, true)
    QT_WQ_GEMV_CASE(false, QT_F16, false) QT_WQ_GEMV_CASE(false, QT_F16, true)
#undef QT_WQ_GEMV_CASE
}

// The conditions both entry points share, on X and on one weight; `what` names the weight in the message.
int check_x(const char* fn, const void* X, int x_dtype, int M, int K, int64_t ldx) {
    QT_CHECK_ARG(X, "%s: null pointer (X is required)", fn);
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "%s: x_dtype %d must be bf16 or fp16", fn, x_dtype);
    QT_CHECK_ARG(M >= 1 && M <= QT_WQ_GEMV_MAX_M, "%s: 1 <= M <= %d rows only, got M = %d", fn, QT_WQ_GEMV_MAX_M, M);
    QT_CHECK_ARG(K >= 1 && K % QT_WQ_GEMV_K_UNIT == 0 && K <= (1 << 30),
                 "%s: K = %d is not a multiple of the k-unit %d (or is above 2^30)", fn, K, QT_WQ_GEMV_K_UNIT);
    QT_CHECK_ARG(ldx >= K, "%s: bad pitch (ldx %lld is below K %d)", fn, (long long)ldx, K);
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
    QT_CHECK_ARG(G == 1 || G == K / QT_WQ_GEMV_K_UNIT, "%s: %s: G must be 1 or K / %d = %d, got %d", fn, what,
                 QT_WQ_GEMV_K_UNIT, K / QT_WQ_GEMV_K_UNIT, G);
    QT_CHECK_ARG(((uintptr_t)Wq & 15) == 0, "%s: %s: Wq must be 16-byte aligned", fn, what);
    return QT_OK;
}

}  // namespace

extern "C" int qt_gemm_wq_gemv(const void* X, int x_dtype, int M, int K, int64_t ldx, const void* Wq, int w_format,
                               int N, const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx,
                               const void* bias, void* Y, int64_t ldy, qt_stream_t stream_) {
    const char* fn = "qt_gemm_wq_gemv";
    QT_CHECK_ARG(Y, "%s: null pointer (Y is required)", fn);
    if (int e = check_x(fn, X, x_dtype, M, K, ldx)) return e;
    if (int e = check_w(fn, "weight", Wq, w_format, N, K, s_w, G, g_idx)) return e;
    QT_CHECK_ARG(ldy >= N, "%s: bad pitch (ldy %lld is below N %d)", fn, (long long)ldy, N);
    const GemvArgs a{(const unsigned short*)X, ldx, K, G, N, FusedW{Wq, s_w, zp_w}, FusedW{nullptr, nullptr, nullptr},
                     (const unsigned short*)bias, (unsigned short*)Y, ldy};
    launch<false>(w_format == QT_W_INT4_PACKED, x_dtype, zp_w != nullptr, M, a, (hipStream_t)stream_);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_gemm_wq_gemv_act_mul(const void* X, int x_dtype, int M, int K, int64_t ldx, const qt_wq_weight* gate,
                                       const qt_wq_weight* up, int act, void* H, int64_t ldh, qt_stream_t stream_) {
    const char* fn = "qt_gemm_wq_gemv_act_mul";
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
    const GemvArgs a{(const unsigned short*)X, ldx, K, gate->G, gate->N, FusedW{gate->Wq, gate->s_w, gate->zp_w},
                     FusedW{up->Wq, up->s_w, up->zp_w}, nullptr, (unsigned short*)H, ldh};
    launch<true>(gate->w_format == QT_W_INT4_PACKED, x_dtype, gate->zp_w != nullptr, M, a, (hipStream_t)stream_);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
