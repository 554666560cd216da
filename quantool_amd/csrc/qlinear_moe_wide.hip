// W8A8 / W4A8 expert banks at batched-decode sizes: qt_gemm_i8_grouped on the weight-streaming 16-column tile, equal to
// it to the bit (include/quantool_amd.h, "Routed experts").
//
// qt_moe_gemm_i8_wide  i8_mid_tile.h's tile (qt_gemm_i8_mid's) over E weight matrices: grid (column tiles, slots), one
//                      slot per tile of up to 16 MT rows of one expert; a workgroup finds its (expert, tile) by walking
//                      offsets, as qt_gemm_i8_skinny_grouped's does, and a surplus one returns before its first weight
//                      load and its first barrier.  MT is chosen from R alone (an expert owns at most R rows), so no
//                      count is read on the host; an expert with more than 16 MT rows takes several slots and its
//                      weights are then read once per 128 rows, as the tiled kernel reads them.
//
// The tile, its bit-equality argument and the addressing of the gathered rows are stated in i8_mid_tile.h.
#include "common.h"
#include "i8_args.h"
#include "i8_mid_tile.h"

static_assert(QT_MOE_I8_WIDE_K_UNIT == MID_KB, "the tile's k-block is the form's k-unit");
static_assert(QT_MOE_I8_WIDE_TILE_ROWS == 16 * 8, "the largest instance holds 8 m-tiles of 16 rows");

namespace {

template <int MT, bool INT4, bool GROUPED>
__global__ void __launch_bounds__(MID_THREADS) moe_gemm_i8_wide_kernel(const MidArgs p, const MidMoe g) {
    i8_mid_tile<MT, INT4, GROUPED, true>(p, g);
}

template <int MT>
void launch_wide(bool int4, bool grouped, dim3 grid, hipStream_t stream, const MidArgs& a, const MidMoe& g) {
#define QT_WIDE_CASE(I4, GR) \
    if (int4 == I4 && grouped == GR) \
        hipLaunchKernelGGL((moe_gemm_i8_wide_kernel<MT, I4, GR>), grid, dim3(MID_THREADS), 0, stream, a, g);
    QT_WIDE_CASE(false, false) QT_WIDE_CASE(false, true) QT_WIDE_CASE(true, false) QT_WIDE_CASE(true, true)
#undef QT_WIDE_CASE
}

}  // namespace

extern "C" int qt_moe_gemm_i8_wide(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R, const int32_t* offsets,
                                   int E, const void* Wq, int w_format, int N, const float* s_x, const int32_t* zp_x,
                                   const float* s_w, int G, const int32_t* wsum, void* Y, int out_dtype, int64_t ldy,
                                   int64_t x_rows, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(x_rows > 0, "qt_moe_gemm_i8_wide: bad arguments");
    QT_CHECK_ARG(K % QT_MOE_I8_WIDE_K_UNIT == 0, "qt_moe_gemm_i8_wide: K %d is not a multiple of the k-unit %d", K,
                 QT_MOE_I8_WIDE_K_UNIT);
    QT_CHECK_ARG(G == 1 || G == K / QT_MOE_I8_WIDE_K_UNIT, "qt_moe_gemm_i8_wide: G %d must be 1 or K / 128 = %d", G,
                 K / QT_MOE_I8_WIDE_K_UNIT);
    QT_CHECK_ARG(E <= QT_MOE_I8_WIDE_MAX_E, "qt_moe_gemm_i8_wide: E %d > %d", E, QT_MOE_I8_WIDE_MAX_E);
    if (int st = qt_i8_check_grouped("qt_moe_gemm_i8_wide", Xq, K, R, offsets, E, Wq, w_format, N, s_x, zp_x, s_w, G,
                                     wsum, Y, out_dtype, ldy, /*aligned16=*/true))
        return st;
    QT_CHECK_ARG(!row_idx || x_rows * (int64_t)K <= (1LL << 32), "qt_moe_gemm_i8_wide: x_rows %lld x K %d > 2^32 "
                 "bytes: a gathered row is addressed by a 32-bit offset", (long long)x_rows, K);
    QT_CHECK_ARG(row_idx || x_rows >= R, "qt_moe_gemm_i8_wide: x_rows %lld < R %lld without row_idx",
                 (long long)x_rows, (long long)R);
    // an expert owns at most R rows: the m-tiles held follow from R alone
    const int mt = R <= 32 ? 2 : R <= 64 ? 4 : 8;
    const int64_t slots = R / (16 * mt) + (E < R ? E : R);
    QT_CHECK_ARG(slots <= 65535, "qt_moe_gemm_i8_wide: %lld row-tile slots (R = %lld, E = %d) exceed the grid",
                 (long long)slots, (long long)R, E);
    const bool int4 = w_format == QT_W_INT4_PACKED;
    MidArgs a{Xq, Wq, s_x, zp_x, s_w, wsum, nullptr, Y, (int)R, N, K, K / 8, G, ldy, out_dtype};
    MidMoe g{offsets, row_idx, x_rows, E};
    const dim3 grid((unsigned)((N + MID_COLS - 1) / MID_COLS), (unsigned)slots);
    if (mt == 2) launch_wide<2>(int4, G > 1, grid, stream, a, g);
    else if (mt == 4) launch_wide<4>(int4, G > 1, grid, stream, a, g);
    else launch_wide<8>(int4, G > 1, grid, stream, a, g);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
