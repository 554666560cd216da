// W4A16 / W8A16 on packed weights from 129 rows up: qt_gemm_wq_tile (include/quantool_amd.h, "A16 runtime"; DESIGN.md
// 4.29).  A tiled GEMM Y[M, N] = X[M, K] W^T (+ bias) that reads the packed weights once per 128-row tile of X, never
// writes a dense weight, and carries a numerics contract of its own -- not the skinny kernel's bits, which is what frees
// the tile shape (qt_gemm_wq_panel is held to four accumulator chains and the 16 x 16 x 32 MFMA by that contract).
//
// NUMERICS.  The MFMA's weight operand is w = round_to_dtype((q - zp) s): q - zp exact in fp32, one multiply, one
// rounding to bf16 / fp16 -- the value StoredWeight.dequantize and qt_dequantize_weight give (the sign of a zero may
// differ).  Output (m, n) is ONE fp32 accumulator: K-tiles of 64 columns ascending and, within each, the four MFMA
// k-steps of 16 columns ascending; then the bias (read as 16-bit, added in fp32), then one rounding to the activation
// dtype.  No atomics, no workspace, no split of K.  So: two runs give the same bits; row m of Y depends on row m of X
// alone (a column of the MFMA's output reads its own B column only), not on M or the row's place in a tile; exactly
// summable inputs give the exact result rounded once; otherwise |y - y_exact| <= ulp(y) / 2 + K 2^-24 sum |x w|, the
// skinny kernel's bound.  The output is NOT bit-equal to qt_gemm_wq_skinny / _stream / _panel or to F.linear.
//
// THE TILE.  256 threads = 4 waves own a 128 x 128 tile of Y; wave w owns rows 64 (w >> 1) .. + 64 and columns 64 (w & 1)
// .. + 64 as 2 x 2 v_mfma_f32_32x32x16_{bf16,f16}, the weights as the A operand (D row = output column n) and the
// activations as B (D column = output row m), so a lane's four consecutive accumulator elements are four consecutive n
// of one row m: one 8-byte store.  A K-tile is 64 columns = half a weight group: one scale and one zero-point per weight
// row, four k-steps, 16 MFMAs per wave.
//
// THE UNITS.  Unit u = { X tile of K-tile u ; packed panel, scales and zero-points of K-tile u + 1 } lives in ring slot
// u % 3.  The packed panel runs one K-tile ahead of the activations because it is dequantised one phase ahead of its
// MFMAs (below).  Per wave and unit, N = 6 (int4) / 7 (int8) LDS-DMA instructions:
//   X       128 rows x 128 B, 16 KiB, 4 dwordx4 per wave, in i8_ring_tile.h's image: piece = 8 rows x 128 B, the 16-byte
//           chunk c of row r at chunk c ^ ((r >> 1) & 7); wave w fills rows 32 w .. 32 w + 31.
//   packed  128 rows x 32 B (int4, 1 dwordx4 per wave) or x 64 B (int8, 2 per wave).  Lane l of wave w always fetches
//           bytes of weight row 32 w + (l >> 1), and the lane that dequantises that row's half reads back exactly the
//           16-byte pieces its own instructions wrote: linear, no swizzle, no bank conflict.
//   scales  s_w[n, g] of the tile's 128 weight rows, one dword per lane (waves 0, 1: row 64 w + lane), and zp_w[n, g],
//           one sign-extended byte per lane into a dword (waves 2, 3; without zero-points they fetch the scales again
//           into the same place, so that N does not depend on the form).  g = 0 when G = 1, else K-tile / 2.
//   Unit -1 (the prologue's) has no X part: N - 4 instructions.  A unit whose packed K-tile would be past the end
//   fetches the last K-tile again: in bounds, dequantised into the idle image buffer, never multiplied.
// THE IMAGE.  Two buffers of 16 KiB hold the 16-bit weights of one K-tile in the X tile's own layout (128 rows n x 128 B,
// the same XOR), so one address expression serves both operands' fragment reads.  Behind barrier(t) wave w dequantises
// its quarter of K-tile t + 1 -- rows 32 w .. 32 w + 31, 32 weights per lane, two lanes per row -- into buffer (t + 1) & 1:
// v_cvt_f32_ubyte*, the exact u - (OFF + zp), one multiply by the scale, the pack; one 16-byte chunk (8 weights) behind
// each k-step's four MFMAs.  That VALU work does not depend on the MFMAs of the phase and is meant to run beside them;
// whether it does has not been measured.  The MFMAs of K-tile t read buffer t & 1, written in phase
// t - 1 (K-tile 0: in the prologue).
// BANKS.  A fragment read is one ds_read_b128 per lane: lane (lr = lane & 31, lh = lane >> 5) reads chunk 2 s + lh of
// row lr (+ 32, + 64, + 96).  Sixteen consecutive rows with one logical chunk: rows 2 i and 2 i + 1 share the XOR value
// and lie 128 B apart, the eight pairs have eight different XOR values, so the sixteen 16-byte reads of a quarter-wave
// cover sixteen different 16-byte bank groups = all 64 banks once.  (A padded row pitch, as wq_panel.hip's, is not
// available to the X image: one LDS-DMA instruction writes 1 KiB lane-linear, eight whole rows.)
//
// HAZARDS (R 3 slots, lead L 2 units, one workgroup barrier per K-tile, no stagger: the four waves run one program).
//   phase t = { counted vmcnt ; lgkmcnt(0) ; s_barrier(t) ; issue unit t + 2 into slot (t + 2) % 3 ; fragment reads of
//               X tile t (slot t % 3) and image t & 1 ; packed / scale reads of K-tile t + 1 (slot t % 3) ;
//               4 x { 4 MFMAs ; dequantise one chunk into image (t + 1) & 1 } }
//   In front of the wait of phase t a wave has units t and t + 1 outstanding: vmcnt(N) retires its part of unit t and
//   leaves unit t + 1 in flight under the MFMAs of phase t, unit t + 2 joining it behind the barrier.
//   RING RAW: every wave retires its part of unit t in front of s_barrier(t); all reads of slot t % 3 follow it.
//   RING WAR: slot (t + 2) % 3 held unit t - 1, all of whose reads -- X fragments, packed words, scales -- were issued
//        in phase t - 1 and retired by the lgkmcnt(0) in front of s_barrier(t); the issue follows that barrier.
//   IMAGE RAW: buffer t & 1 is written in phase t - 1; the writes are retired by the lgkmcnt(0) in front of
//        s_barrier(t), the MFMAs' fragment reads follow it.
//   IMAGE WAR: buffer (t + 1) & 1 was read by the fragment reads of phase t - 1, retired by the same lgkmcnt(0) in front
//        of s_barrier(t); the writes of phase t follow it.  (One buffer would put the writes of K-tile t + 1 beside the
//        reads of K-tile t.)
//   Prologue: units -1, 0, 1 are issued (K >= 128: there are always two K-tiles); vmcnt(2 N) retires unit -1, a barrier
//        makes its scales visible, K-tile 0 is dequantised into buffer 0; phase 0's wait and barrier are the loop's.
//   Drain: phase t with t + 2 >= nt issues nothing; the last phase has only its own unit outstanding and waits
//        vmcnt(0): the one place.
// LDS: 3 x (16 + 4 or 8 + 1) KiB + 2 x 16 KiB = 95 / 107 KiB: one workgroup per CU, one wave per SIMD.
// EDGES: a tile row past M re-reads row M - 1, a weight row past N re-reads row N - 1 (data, scale, zero-point) and is
// dequantised with scale 0; neither is stored.  K is a whole number of K-tiles.  No byte outside X[:M, :K], the weight,
// its scales / zero-points and bias[:N] is read, nothing outside Y[:M, :N] is written.  Lane offsets are 32-bit: the
// host keeps ldx <= QT_WQ_TILE_MAX_LDX, so 128 rows of X span less than 2^31 bytes, and the number of tiles below 2^31.
// The kernel is in csrc/build.py's spill and M0 audits.
//
// The statements are wq_tile_body.h, shared as text with moe_gemm_wq_tile_kernel (wq_moe_tile.hip; wq_tile.h says why).
// -ffp-contract=off (csrc/build.py): every multiply and add there rounds on its own.
#include "wq_tile.h"

namespace {

static_assert(QT_WQ_TILE_K_UNIT == 2 * TKU && QT_WQ_TILE_K_UNIT == WQ_KB, "two K-tiles per weight group");
static_assert((int64_t)TT * QT_WQ_TILE_MAX_LDX * 2 <= (1LL << 31), "tile offsets fit 31 bits");

template <bool INT4, int DT, bool ZP>
__global__ void __launch_bounds__(TTHREADS) wq_tile_kernel(const WqArgs p) {
    const int tiles_n = (p.N + TT - 1) / TT, tiles_m = (p.M + TT - 1) / TT;
    int m_tile, n_tile;
    i8_ring_tile_of(blockIdx.x, tiles_m, tiles_n, m_tile, n_tile);     // a band of m-tiles walks the n-tiles together
    const int m0 = m_tile * TT, n0 = n_tile * TT;
    constexpr bool MOE = false;
    constexpr int64_t row0 = 0, x_rows = 0;                     // the grouped form's names: not read
#include "wq_tile_body.h"
}

}  // namespace

extern "C" int qt_gemm_wq_tile(const void* X, int x_dtype, int M, int K, int64_t ldx, const void* Wq, int w_format,
                               int N, const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx,
                               const void* bias, void* Y, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(X && Wq && s_w && Y, "qt_gemm_wq_tile: null pointer (X, Wq, s_w and Y are required)");
    QT_CHECK_ARG(g_idx == nullptr,
                 "qt_gemm_wq_tile: g_idx is not taken (actorder group runs on qt_dequantize_weight + a dense GEMM)");
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "qt_gemm_wq_tile: x_dtype %d must be bf16 or fp16", x_dtype);
    QT_CHECK_ARG(w_format == QT_W_INT8 || w_format == QT_W_INT4_PACKED, "qt_gemm_wq_tile: w_format %d unsupported",
                 w_format);
    QT_CHECK_ARG(M >= 1, "qt_gemm_wq_tile: M >= 1 rows only, got M = %d", M);
    QT_CHECK_ARG(N >= 1 && K >= 1, "qt_gemm_wq_tile: empty weight (N = %d, K = %d)", N, K);
    QT_CHECK_ARG(K % QT_WQ_TILE_K_UNIT == 0, "qt_gemm_wq_tile: K = %d is not a multiple of the k-unit %d", K,
                 QT_WQ_TILE_K_UNIT);
    QT_CHECK_ARG(G == 1 || G == K / QT_WQ_TILE_K_UNIT, "qt_gemm_wq_tile: G must be 1 or K / %d = %d, got %d",
                 QT_WQ_TILE_K_UNIT, K / QT_WQ_TILE_K_UNIT, G);
    QT_CHECK_ARG(ldx >= K && ldy >= N && ldx <= QT_WQ_TILE_MAX_LDX,
                 "qt_gemm_wq_tile: bad pitch (ldx >= K, ldy >= N, ldx <= %d)", QT_WQ_TILE_MAX_LDX);
    QT_CHECK_ARG((((uintptr_t)X | (uintptr_t)Wq) & 15) == 0 && ldx % 8 == 0,
                 "qt_gemm_wq_tile: X, Wq and the row pitch of X must be 16-byte aligned");
    const int64_t tiles = (((int64_t)M + TT - 1) / TT) * (((int64_t)N + TT - 1) / TT);
    QT_CHECK_ARG(tiles <= 0x7fffffffLL, "qt_gemm_wq_tile: ceil(M / %d) * ceil(N / %d) tiles must stay below 2^31", TT, TT);
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const bool vec = ((uintptr_t)Y & 7) == 0 && ldy % 4 == 0;
    WqArgs a{(const unsigned short*)X, ldx, M, Wq, N, K, K / 8, s_w, G, zp_w, nullptr,
             (const unsigned short*)bias, (unsigned short*)Y, ldy, (int)vec, nullptr, nullptr, 0};
#define QT_WQ_TILE_CASE(I4, D, Z)                                       \
    if (int4 == I4 && x_dtype == D && (zp_w != nullptr) == Z)           \
        hipLaunchKernelGGL((wq_tile_kernel<I4, D, Z>), dim3((unsigned)tiles), dim3(TTHREADS), 0, stream, a);
    QT_WQ_TILE_CASE(true, QT_BF16, false) QT_WQ_TILE_CASE(true, QT_BF16, true)
    QT_WQ_TILE_CASE(true, QT_F16, false) QT_WQ_TILE_CASE(true, QT_F16, true)
    QT_WQ_TILE_CASE(false, QT_BF16, false) QT_WQ_TILE_CASE(false, QT_BF16, true)
    QT_WQ_TILE_CASE(false, QT_F16, false) QT_WQ_TILE_CASE(false, QT_F16, true)
#undef QT_WQ_TILE_CASE
    QT_LAUNCH_CHECK();
    return QT_OK;
}
