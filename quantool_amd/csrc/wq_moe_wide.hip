// W4A16 / W8A16 expert banks at batched-decode sizes: qt_gemm_wq_grouped on the weight-streaming tile of several
// m-tiles, equal to it to the bit (include/quantool_amd.h, "A16 runtime").
//
// qt_moe_gemm_wq_wide  wq_stream_tile.h's tile (qt_gemm_wq_stream's) over E weight matrices: grid (column tiles, slots),
//                      one slot per tile of up to 16 MT rows of one expert; a workgroup finds its (expert, tile) by
//                      walking offsets, as wq_skinny_kernel<..., MOE> does with 16 in place of 16 MT, and a surplus one
//                      returns before its first weight load and its barrier.  MT is chosen from R and E alone (the
//                      smallest of 1 / 2 / 4 / 8 whose 16 MT rows hold ceil(R / E)), so no count is read on the host; an
//                      expert with more than 16 MT rows takes several slots.
//
// The tile, its bit-equality argument and the addressing of the gathered rows are stated in wq_stream_tile.h.
#include "common.h"
#include "wq_stream_tile.h"

static_assert(QT_MOE_WQ_WIDE_K_UNIT == WQ_KB, "the tile's k-block is the form's k-unit");

namespace {

template <bool INT4, int DT, bool ZP, int MT>
__global__ void __launch_bounds__(WQ_THREADS) moe_gemm_wq_wide_kernel(const WqArgs args, const int64_t x_rows) {
    // slot -> (expert, tile of 16 MT rows); offsets clamped to [0, R] so a bad table cannot move a write out of Y
    constexpr int64_t TILE = 16 * MT;
    WqArgs p = args;
    const int64_t slot = blockIdx.y;
    int64_t start = 0, hi = 0, m0 = 0;
    int e = -1;
    for (int j = 0; j < p.E; ++j) {
        const int64_t lo = min(max((int64_t)p.offsets[j], (int64_t)0), (int64_t)p.M);
        hi = min(max((int64_t)p.offsets[j + 1], lo), (int64_t)p.M);
        const int64_t nt = (hi - lo + TILE - 1) / TILE;
        if (slot < start + nt) {
            e = j;
            m0 = lo + (slot - start) * TILE;
            break;
        }
        start += nt;
    }
    if (e < 0) return;                  // surplus slot (uniform: before any load of the weights and the barrier)
    p.M = (int)min(hi - m0, TILE);      // live rows of the tile, 1 .. 16 MT
    const int64_t wrow = INT4 ? (int64_t)p.Kw : (int64_t)p.K;
    p.Wq = INT4 ? (const void*)((const int32_t*)p.Wq + (int64_t)e * p.N * wrow)
                : (const void*)((const int8_t*)p.Wq + (int64_t)e * p.N * wrow);
    p.s_w += (int64_t)e * p.N * p.G;
    if constexpr (ZP) p.zp_w += (int64_t)e * p.N * p.G;
    constexpr bool MOE = true;
#include "wq_stream_tile_body.h"
}

template <bool I4, int D, bool Z>
void launch_wide(int mt, dim3 grid, hipStream_t stream, const WqArgs& a, int64_t x_rows) {
#define QT_WQ_WIDE_MT(T) \
    case T: hipLaunchKernelGGL((moe_gemm_wq_wide_kernel<I4, D, Z, T>), grid, dim3(WQ_THREADS), 0, stream, a, x_rows); \
        break;
    switch (mt) { QT_WQ_WIDE_MT(1) QT_WQ_WIDE_MT(2) QT_WQ_WIDE_MT(4) QT_WQ_WIDE_MT(8) }
#undef QT_WQ_WIDE_MT
}

}  // namespace

extern "C" int qt_moe_gemm_wq_wide(const void* X, int x_dtype, int K, int64_t ldx, const int32_t* row_idx, int64_t R,
                                   const int32_t* offsets, int E, const void* Wq, int w_format, int N,
                                   const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx, void* Y,
                                   int64_t ldy, int64_t x_rows, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(X && Wq && s_w && offsets && Y,
                 "qt_moe_gemm_wq_wide: null pointer (X, offsets, Wq, s_w and Y are required)");
    QT_CHECK_ARG(g_idx == nullptr, "qt_moe_gemm_wq_wide: g_idx is not taken (an actorder-group bank runs on "
                 "qt_gemm_wq_grouped or on qt_dequantize_weight + a dense bank)");
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "qt_moe_gemm_wq_wide: x_dtype %d must be bf16 or fp16", x_dtype);
    QT_CHECK_ARG(w_format == QT_W_INT8 || w_format == QT_W_INT4_PACKED, "qt_moe_gemm_wq_wide: w_format %d unsupported",
                 w_format);
    QT_CHECK_ARG(N >= 1 && K >= 1, "qt_moe_gemm_wq_wide: empty weight (N = %d, K = %d)", N, K);
    QT_CHECK_ARG(K % QT_MOE_WQ_WIDE_K_UNIT == 0, "qt_moe_gemm_wq_wide: K = %d is not a multiple of the k-unit %d", K,
                 QT_MOE_WQ_WIDE_K_UNIT);
    QT_CHECK_ARG(G == 1 || G == K / QT_MOE_WQ_WIDE_K_UNIT, "qt_moe_gemm_wq_wide: G must be 1 or K / %d = %d, got %d",
                 QT_MOE_WQ_WIDE_K_UNIT, K / QT_MOE_WQ_WIDE_K_UNIT, G);
    QT_CHECK_ARG(R >= 1 && R <= 0x7fffffffLL && E >= 1 && E <= QT_MOE_WQ_WIDE_MAX_E && x_rows >= 1,
                 "qt_moe_gemm_wq_wide: bad sizes (1 <= R < 2^31, 1 <= E <= %d, x_rows >= 1; R = %lld, E = %d, "
                 "x_rows = %lld)", QT_MOE_WQ_WIDE_MAX_E, (long long)R, E, (long long)x_rows);
    QT_CHECK_ARG(ldx >= K && ldy >= N, "qt_moe_gemm_wq_wide: bad pitch (ldx >= K, ldy >= N)");
    QT_CHECK_ARG((((uintptr_t)X | (uintptr_t)Wq) & 15) == 0 && ldx % 8 == 0,
                 "qt_moe_gemm_wq_wide: X, Wq and the row pitch of X must be 16-byte aligned");
    QT_CHECK_ARG(x_rows <= (1LL << 32) / (2 * ldx) && x_rows * ldx * 2 + 2 * (int64_t)K < (1LL << 32),
                 "qt_moe_gemm_wq_wide: x_rows %lld x ldx %lld x 2 + 2 K reaches 2^32 bytes: a row of X is addressed by a "
                 "32-bit offset", (long long)x_rows, (long long)ldx);
    QT_CHECK_ARG(row_idx || x_rows >= R, "qt_moe_gemm_wq_wide: x_rows %lld < R %lld without row_idx",
                 (long long)x_rows, (long long)R);
    // the m-tiles held: the smallest instance whose 16 MT rows hold ceil(R / E), so that even routing puts one expert
    // in one slot
    const int64_t per = (R + E - 1) / E;
    const int mt = per <= 16 ? 1 : per <= 32 ? 2 : per <= 64 ? 4 : 8;
    const int64_t slots = R / (16 * mt) + (E < R ? E : R);
    QT_CHECK_ARG(slots <= QT_MOE_WQ_WIDE_MAX_SLOTS,
                 "qt_moe_gemm_wq_wide: %lld row-tile slots (R = %lld, E = %d) exceed the grid's %d", (long long)slots,
                 (long long)R, E, QT_MOE_WQ_WIDE_MAX_SLOTS);
    const bool int4 = w_format == QT_W_INT4_PACKED;
    WqArgs a{(const unsigned short*)X, ldx, (int)R, Wq, N, K, K / 8, s_w, G, zp_w, nullptr, nullptr,
             (unsigned short*)Y, ldy, 1, offsets, row_idx, E};
    const dim3 grid((unsigned)(((int64_t)N + 15) / 16), (unsigned)slots);
#define QT_WQ_WIDE_CASE(I4, D, Z) \
    if (int4 == I4 && x_dtype == D && (zp_w != nullptr) == Z) launch_wide<I4, D, Z>(mt, grid, stream, a, x_rows);
    QT_WQ_WIDE_CASE(true, QT_BF16, false) QT_WQ_WIDE_CASE(true, QT_BF16, true)
    QT_WQ_WIDE_CASE(true, QT_F16, false) QT_WQ_WIDE_CASE(true, QT_F16, true)
    QT_WQ_WIDE_CASE(false, QT_BF16, false) QT_WQ_WIDE_CASE(false, QT_BF16, true)
    QT_WQ_WIDE_CASE(false, QT_F16, false) QT_WQ_WIDE_CASE(false, QT_F16, true)
#undef QT_WQ_WIDE_CASE
    QT_LAUNCH_CHECK();
    return QT_OK;
}
