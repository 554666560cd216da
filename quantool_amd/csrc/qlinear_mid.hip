// W8A8 / W4A8 mid-M path: qt_gemm_i8 for 1 <= M <= 128 rows, equal to it to the bit
// (include/quantool_amd.h, "A8 runtime").
//
// qt_gemm_i8_mid  qlinear_skinny.hip's tile widened in M: a workgroup owns 16 output columns n (weight rows) and all M
//                 rows, and splits K over its 4 waves.  The tile, its bit-equality argument and its loads are stated
//                 once, in i8_mid_tile.h, which the expert-bank form (qlinear_moe_wide.hip) runs as well; this file is
//                 the dense instance (MOE = false) and its entry point.
#include "common.h"
#include "i8_args.h"
#include "i8_mid_tile.h"

namespace {

constexpr int MID_MAX_M = QT_I8_MID_MAX_M;

template <int MT, bool INT4, bool GROUPED>
__global__ void __launch_bounds__(MID_THREADS) gemm_i8_mid_kernel(const MidArgs p) {
    i8_mid_tile<MT, INT4, GROUPED, false>(p, MidMoe{nullptr, nullptr, 0, 0});
}

template <int MT>
void launch_mid(bool int4, bool grouped, dim3 grid, hipStream_t stream, const MidArgs& a) {
#define QT_MID_CASE(I4, GR) \
    if (int4 == I4 && grouped == GR) \
        hipLaunchKernelGGL((gemm_i8_mid_kernel<MT, I4, GR>), grid, dim3(MID_THREADS), 0, stream, a);
    QT_MID_CASE(false, false) QT_MID_CASE(false, true) QT_MID_CASE(true, false) QT_MID_CASE(true, true)
#undef QT_MID_CASE
}

}  // namespace

extern "C" int qt_gemm_i8_mid(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N, const float* s_x,
                              const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias,
                              void* Y, int out_dtype, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(M >= 1 && M <= MID_MAX_M, "qt_gemm_i8_mid: M %lld outside 1 .. %d", (long long)M, MID_MAX_M);
    QT_CHECK_ARG(K % MID_KB == 0, "qt_gemm_i8_mid: K %d is not a multiple of the k-unit %d", K, MID_KB);
    QT_CHECK_ARG(G == 1 || G == K / MID_KB, "qt_gemm_i8_mid: G %d must be 1 or K / 128 = %d", G, K / MID_KB);
    QT_CHECK_ARG((((uintptr_t)Xq | (uintptr_t)Wq) & 15) == 0, "qt_gemm_i8_mid: Xq and Wq must be 16-byte aligned");
    if (int st = qt_i8_check_dense("qt_gemm_i8_mid", Xq, M, K, Wq, w_format, N, s_x, zp_x, s_w, G, wsum, Y, out_dtype, ldy))
        return st;
    const bool int4 = w_format == QT_W_INT4_PACKED;
    MidArgs a{Xq, Wq, s_x, zp_x, s_w, wsum, bias, Y, (int)M, N, K, K / 8, G, ldy, out_dtype};
    const dim3 grid((unsigned)((N + MID_COLS - 1) / MID_COLS));
    if (M <= 32) launch_mid<2>(int4, G > 1, grid, stream, a);
    else if (M <= 64) launch_mid<4>(int4, G > 1, grid, stream, a);
    else launch_mid<8>(int4, G > 1, grid, stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
