// W4A16 / W8A16 expert banks at prompt sizes: qt_moe_gemm_wq_tile (include/quantool_amd.h, "A16 runtime"; DESIGN.md
// 4.30).  qt_gemm_wq_tile's 128 x 128 MFMA tile over E weight matrices and routed, gathered rows: Y [R, N] in routed
// order, expert e owns rows [offsets[e], offsets[e + 1]) and weight matrix e, the X row behind routed row r is
// X[row_idx[r]].  The packed bank is read where it is; neither a dense weight nor a gathered copy of X is written.
//
// NUMERICS.  Row r of Y, owned by expert e, has the bits qt_gemm_wq_tile gives for the one activation row X[row_idx[r]]
// against expert e's weight, scales and zero-points, without bias: the statements behind the lane offsets are that
// kernel's own text (wq_tile_body.h) -- one fp32 accumulator per output, K-tiles of 64 columns ascending and the four
// k-steps ascending within each, the weight operand round_to_dtype((q - zp) s), one rounding at the end -- and a column
// of the MFMA's output reads its own B column only, so neither the slot's other rows, nor the padding rows, nor the
// place of the row in its tile reach its bits.  Not bit-equal to qt_gemm_wq_grouped / qt_moe_gemm_wq_wide or to the
// dense bank, as qt_gemm_wq_tile is not to the skinny kernels or to F.linear.  No atomics, no workspace, no split of K:
// two runs give the same bits.
//
// WORK SPLIT.  A slot is one tile of up to 128 routed rows of one expert; a workgroup owns (slot, column tile of 128).
//   The host takes slots = floor(R / 128) + min(E, R) from R and E alone -- per expert ceil(r / 128) <= floor(r / 128) +
//   [r > 0] and sum_e floor(r_e / 128) <= floor(R / 128), so this bounds the tiles of any routing -- and reads no count:
//   no host sync.  A workgroup walks offsets, clamped into [0, R] and made ascending (as moe_gemm_wq_wide_kernel), to
//   its (expert, first row, live rows); a surplus one returns before its first load and its first barrier (uniform:
//   the walk is scalar).  An expert without rows owns no slot and its weights are never addressed.
// GRID ORDER.  1-D, slots * ceil(N / 128) workgroups: a band of MOE_BAND = 8 consecutive slots walks the column tiles
//   together, the slot running fastest (pid -> slot = band first + pid % 8, column tile = pid / 8 within the band; the
//   last band is narrower).  Workgroups are dealt round-robin over the 8 XCDs, so with 8 slots to a band an XCD's L2 sees
//   ONE slot's gathered rows through all of the band's column tiles -- 128 x K x 2 B, 1 MiB at K = 4096 and 3.5 MiB at
//   K = 14336, against 4 MiB of L2 -- and they are fetched from memory once per XCD and band instead of once per column
//   tile.  The gathered rows are the operand chosen because they are the larger one: 128 x K x 2 B against the packed
//   panel's 128 x K / 2 B (int4) or 128 x K B (int8) per tile.  The panel of (expert, column tile) is then shared in
//   time rather than in one L2: the slots of an expert are consecutive, so the up to 8 workgroups that read one panel
//   are consecutive pids that start together on 8 XCDs, and memory serves it once to the first and from the memory-side
//   cache to the rest.  The other order -- column tile fastest inside a slot -- spreads one slot's rows over all 8 L2s
//   at once and reads every panel of the expert from memory again for each of its slots, at different times.
//   Surplus slots are the highest ones: they thin out the last band(s) only.  None of this is measured apart from the
//   end-to-end times in DESIGN.md 4.30.
// GATHERED ROWS.  Each lane of the X tile's LDS-DMA carries its own source byte offset already; here it is
//   clamp(row_idx[first row + min(tile row, live - 1)], 0, x_rows - 1) * ldx * 2 + chunk, read once in the prologue into
//   the lane's four offsets, from the base pointer X itself (+ 128 B per K-tile, scalar).  The offsets are unsigned
//   32-bit: the host keeps x_rows ldx 2 + 2 K below 2^32.  A tile row past the live rows re-reads the last live row and
//   is not stored.
// WEIGHT BASE.  Wq, s_w and zp_w advance by e N (row bytes) and e N G in 64-bit arithmetic before the lane offsets are
//   formed; a weight row past N re-reads row N - 1 and is dequantised with scale 0, as in the dense kernel.
// EPILOGUE.  Y advances by (first row) ldy in 64-bit arithmetic; 8-byte stores where Y and ldy allow, scalar ones at
//   the ragged end.  No byte outside X [x_rows, K] (pitch ldx), Wq [E, N, .], s_w / zp_w [E, N, G], offsets [E + 1] and
//   row_idx [R] is read; nothing outside Y[m < offsets[E], n < N] is written.
// LDS 95 / 107 KiB, the dense kernel's.  The kernel is in csrc/build.py's scratch, spill and M0 audits.
//
// -ffp-contract=off, no packed fp32 (csrc/build.py): wq_tile.hip's flags, so the shared text compiles to one arithmetic.
#include "wq_tile.h"

namespace {

static_assert(QT_MOE_WQ_TILE_K_UNIT == 2 * TKU && QT_MOE_WQ_TILE_K_UNIT == WQ_KB, "two K-tiles per weight group");

constexpr int MOE_BAND = 8;     // slots that walk the column tiles together: one per XCD

// workgroup pid -> its slot and column tile (GRID ORDER above)
__device__ __forceinline__ void moe_tile_of(int pid, int slots, int tiles_n, int& slot, int& n_tile) {
    const int per_band = MOE_BAND * tiles_n;
    const int first = pid / per_band * MOE_BAND;
    const int bsize = (slots - first) < MOE_BAND ? (slots - first) : MOE_BAND;
    const int in_b = pid % per_band;
    slot = first + in_b % bsize;
    n_tile = in_b / bsize;
}

template <bool INT4, int DT, bool ZP>
__global__ void __launch_bounds__(TTHREADS) moe_gemm_wq_tile_kernel(const WqArgs args, const int64_t x_rows,
                                                                    const int slots) {
    WqArgs p = args;
    int slot, n_tile;
    moe_tile_of(blockIdx.x, slots, (p.N + TT - 1) / TT, slot, n_tile);
    // slot -> (expert, first row, live rows); offsets clamped to [0, R] so a bad table cannot move a write out of Y
    int64_t start = 0, hi = 0, row0 = 0;
    int e = -1;
    for (int j = 0; j < p.E; ++j) {
        const int64_t lo = min(max((int64_t)p.offsets[j], (int64_t)0), (int64_t)p.M);
        hi = min(max((int64_t)p.offsets[j + 1], lo), (int64_t)p.M);
        const int64_t tiles = (hi - lo + TT - 1) / TT;
        if (slot < start + tiles) {
            e = j;
            row0 = lo + (slot - start) * TT;
            break;
        }
        start += tiles;
    }
    if (e < 0) return;                  // surplus slot (uniform: before any load of the operands and the first barrier)
    p.M = (int)min(hi - row0, (int64_t)TT);     // live rows of the slot, 1 .. 128
    const int64_t wrow = INT4 ? (int64_t)p.K / 2 : (int64_t)p.K;
    p.Wq = (const void*)((const char*)p.Wq + (int64_t)e * p.N * wrow);
    p.s_w += (int64_t)e * p.N * p.G;
    if constexpr (ZP) p.zp_w += (int64_t)e * p.N * p.G;
    p.Y += row0 * p.ldy;
    const int m0 = 0, n0 = n_tile * TT;
    constexpr bool MOE = true;
#include "wq_tile_body.h"
}

}  // namespace

extern "C" int qt_moe_gemm_wq_tile(const void* X, int x_dtype, int K, int64_t ldx, const int32_t* row_idx, int64_t R,
                                   const int32_t* offsets, int E, const void* Wq, int w_format, int N,
                                   const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx, void* Y,
                                   int64_t ldy, int64_t x_rows, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(X && Wq && s_w && offsets && Y,
                 "qt_moe_gemm_wq_tile: null pointer (X, offsets, Wq, s_w and Y are required)");
    QT_CHECK_ARG(g_idx == nullptr, "qt_moe_gemm_wq_tile: g_idx is not taken (an actorder-group bank runs on "
                 "qt_gemm_wq_grouped or on qt_dequantize_weight + a dense bank)");
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "qt_moe_gemm_wq_tile: x_dtype %d must be bf16 or fp16", x_dtype);
    QT_CHECK_ARG(w_format == QT_W_INT8 || w_format == QT_W_INT4_PACKED, "qt_moe_gemm_wq_tile: w_format %d unsupported",
                 w_format);
    QT_CHECK_ARG(N >= 1 && K >= 1, "qt_moe_gemm_wq_tile: empty weight (N = %d, K = %d)", N, K);
    QT_CHECK_ARG(K % QT_MOE_WQ_TILE_K_UNIT == 0, "qt_moe_gemm_wq_tile: K = %d is not a multiple of the k-unit %d", K,
                 QT_MOE_WQ_TILE_K_UNIT);
    QT_CHECK_ARG(G == 1 || G == K / QT_MOE_WQ_TILE_K_UNIT, "qt_moe_gemm_wq_tile: G must be 1 or K / %d = %d, got %d",
                 QT_MOE_WQ_TILE_K_UNIT, K / QT_MOE_WQ_TILE_K_UNIT, G);
    QT_CHECK_ARG(R >= 1 && R <= 0x7fffffffLL && E >= 1 && E <= QT_MOE_WQ_TILE_MAX_E && x_rows >= 1,
                 "qt_moe_gemm_wq_tile: bad sizes (1 <= R < 2^31, 1 <= E <= %d, x_rows >= 1; R = %lld, E = %d, "
                 "x_rows = %lld)", QT_MOE_WQ_TILE_MAX_E, (long long)R, E, (long long)x_rows);
    QT_CHECK_ARG(ldx >= K && ldy >= N, "qt_moe_gemm_wq_tile: bad pitch (ldx >= K, ldy >= N)");
    QT_CHECK_ARG((((uintptr_t)X | (uintptr_t)Wq) & 15) == 0 && ldx % 8 == 0,
                 "qt_moe_gemm_wq_tile: X, Wq and the row pitch of X must be 16-byte aligned");
    QT_CHECK_ARG(x_rows <= (1LL << 32) / (2 * ldx) && x_rows * ldx * 2 + 2 * (int64_t)K < (1LL << 32),
                 "qt_moe_gemm_wq_tile: x_rows %lld x ldx %lld x 2 + 2 K reaches 2^32 bytes: a row of X is addressed by a "
                 "32-bit offset", (long long)x_rows, (long long)ldx);
    QT_CHECK_ARG(row_idx || x_rows >= R, "qt_moe_gemm_wq_tile: x_rows %lld < R %lld without row_idx",
                 (long long)x_rows, (long long)R);
    // slots from R and E alone: an upper bound on sum_e ceil(rows_e / 128) for any routing
    const int64_t slots = R / TT + (E < R ? E : R);
    const int64_t tiles = slots * (((int64_t)N + TT - 1) / TT);
    QT_CHECK_ARG(tiles <= QT_MOE_WQ_TILE_MAX_TILES,
                 "qt_moe_gemm_wq_tile: %lld row-tile slots (R = %lld, E = %d) x ceil(N / %d) column tiles exceed the "
                 "grid's %d", (long long)slots, (long long)R, E, TT, QT_MOE_WQ_TILE_MAX_TILES);
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const bool vec = ((uintptr_t)Y & 7) == 0 && ldy % 4 == 0;
    WqArgs a{(const unsigned short*)X, ldx, (int)R, Wq, N, K, K / 8, s_w, G, zp_w, nullptr, nullptr,
             (unsigned short*)Y, ldy, (int)vec, offsets, row_idx, E};
#define QT_MOE_WQ_TILE_CASE(I4, D, Z)                                                                              \
    if (int4 == I4 && x_dtype == D && (zp_w != nullptr) == Z)                                                      \
        hipLaunchKernelGGL((moe_gemm_wq_tile_kernel<I4, D, Z>), dim3((unsigned)tiles), dim3(TTHREADS), 0, stream, a, \
                           x_rows, (int)slots);
    QT_MOE_WQ_TILE_CASE(true, QT_BF16, false) QT_MOE_WQ_TILE_CASE(true, QT_BF16, true)
    QT_MOE_WQ_TILE_CASE(true, QT_F16, false) QT_MOE_WQ_TILE_CASE(true, QT_F16, true)
    QT_MOE_WQ_TILE_CASE(false, QT_BF16, false) QT_MOE_WQ_TILE_CASE(false, QT_BF16, true)
    QT_MOE_WQ_TILE_CASE(false, QT_F16, false) QT_MOE_WQ_TILE_CASE(false, QT_F16, true)
#undef QT_MOE_WQ_TILE_CASE
    QT_LAUNCH_CHECK();
    return QT_OK;
}
