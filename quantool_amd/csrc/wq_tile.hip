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
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own.
#include "common.h"
#include "i8_ring_tile.h"
#include "wq_stream_tile.h"

namespace {

constexpr int TT = 128;                      // output tile edge
constexpr int TKU = 64;                      // columns per K-tile: half a weight group
constexpr int TSLOTS = 3;                    // units resident in LDS
constexpr int TLEAD = 2;                     // unit t + TLEAD is issued in phase t
constexpr int TTHREADS = 256;                // 4 waves: 2 (M) x 2 (N), 64 x 64 outputs per wave
constexpr int TX_BYTES = TT * TKU * 2;       // 16 KiB: the X tile, and one weight image
constexpr int TS_BYTES = 2 * TT * 4;         // 128 scales, 128 zero-points as dwords
static_assert(QT_WQ_TILE_K_UNIT == 2 * TKU && QT_WQ_TILE_K_UNIT == WQ_KB, "two K-tiles per weight group");
static_assert(TLEAD <= TSLOTS - 1, "WAR: see the head comment");
static_assert((int64_t)TT * QT_WQ_TILE_MAX_LDX * 2 <= (1LL << 31), "tile offsets fit 31 bits");

// One sign-extended byte per lane into a dword of LDS (64 x 4 B per wave-instruction): the gather of a column of the
// int8 zero-point table, whose entries no dword load can address.  ring_pipe.h's glds4_one with the byte opcode;
// counted in vmcnt like every other LDS-DMA.
__device__ __forceinline__ void glds1_one(unsigned voff, const void* sbase, unsigned lds_dst) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_sbyte %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}

template <int DT>
__device__ __forceinline__ f32x16 tile_mfma(const u32x4 a, const u32x4 b, f32x16 c) {
    if constexpr (DT == QT_F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0,
                                                      0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                       0, 0, 0);
}

// byte offset of the 16-byte chunk c of row r in the X tile / weight image
__device__ __forceinline__ int tile_img(int r, int c) {
    return (r >> 3) * 1024 + (r & 7) * 128 + 16 * (c ^ ((r >> 1) & 7));
}

template <bool INT4, int DT, bool ZP>
__global__ void __launch_bounds__(TTHREADS) wq_tile_kernel(const WqArgs p) {
    constexpr int W_BYTES = TT * TKU / (INT4 ? 2 : 1);          // packed panel of a K-tile: 4 / 8 KiB
    constexpr int WI = INT4 ? 1 : 2;                            // its LDS-DMA instructions per wave
    constexpr int NI = 4 + WI + 1;                              // LDS-DMA instructions per wave and unit
    constexpr int SLOT_BYTES = TX_BYTES + W_BYTES + TS_BYTES;
    __shared__ __attribute__((aligned(16))) char lds[TSLOTS * SLOT_BYTES + 2 * TX_BYTES];
    char* ring = lds;
    char* img = lds + TSLOTS * SLOT_BYTES;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1;
    const int tiles_n = (p.N + TT - 1) / TT, tiles_m = (p.M + TT - 1) / TT;
    int m_tile, n_tile;
    i8_ring_tile_of(blockIdx.x, tiles_m, tiles_n, m_tile, n_tile);     // a band of m-tiles walks the n-tiles together
    const int m0 = m_tile * TT, n0 = n_tile * TT;
    const int nt = p.K / TKU;                                   // K-tiles = phases, >= 2
    const int a_last = p.M - 1 - m0, b_last = p.N - 1 - n0;     // last valid row of each operand, relative to the tile
    const int wrow_b = p.K / (INT4 ? 2 : 1);                    // bytes of a packed weight row

    // ---- staging geometry: this lane's source byte offsets, relative to the K-tile's first byte in the tile's row 0 ----
    unsigned voffX[4], voffW, voffS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {                               // row 32 wave + 8 i + (lane >> 3), physical chunk lane & 7
        const int r = 32 * wave + 8 * i + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        voffX[i] = (unsigned)((int64_t)min(r, a_last) * p.ldx * 2 + 16 * c);
    }
    const int drow = 32 * wave + (lane >> 1);                   // the weight row this lane fetches and dequantises
    voffW = (unsigned)((int64_t)min(drow, b_last) * wrow_b + 16 * (lane & 1));     // int8: + 32 for the second piece
    const int scol = 64 * wave_n + lane;                        // the weight row whose scale / zero-point this lane fetches
    const bool zp_wave = ZP && wave_m;                          // waves 2, 3: the zero-points
    voffS = (unsigned)((int64_t)min(scol, b_last) * p.G * (zp_wave ? 1 : 4));
    const unsigned ring_lds = (unsigned)(size_t)(QT_LDS char*)ring;
    const unsigned dstX = __builtin_amdgcn_readfirstlane(ring_lds + wave * 4096);
    const unsigned dstW = __builtin_amdgcn_readfirstlane(ring_lds + TX_BYTES + wave * (1024 * WI));
    const unsigned dstS = __builtin_amdgcn_readfirstlane(ring_lds + TX_BYTES + W_BYTES + wave_m * 512 + wave_n * 256);
    const char* srcX = (const char*)(p.X + (int64_t)m0 * p.ldx);
    const char* srcW = (const char*)p.Wq + (int64_t)n0 * wrow_b;
    const char* srcS = zp_wave ? (const char*)p.zp_w + (int64_t)n0 * p.G : (const char*)p.s_w + (int64_t)n0 * p.G * 4;
    // unit u into `slot`: the X tile of K-tile u (none for u = -1) and the packed panel of K-tile min(u + 1, nt - 1)
    auto issue = [&](int u, int slot) {
        const unsigned off = (unsigned)slot * SLOT_BYTES;
        if (u >= 0) {
            const char* x = srcX + (size_t)u * (TKU * 2);
            glds16_pair(voffX[0], voffX[1], x, dstX + off, dstX + off + 1024);
            glds16_pair(voffX[2], voffX[3], x, dstX + off + 2048, dstX + off + 3072);
        }
        const int tw = min(u + 1, nt - 1);
        const char* w = srcW + (size_t)tw * (W_BYTES / TT);
        if constexpr (INT4) glds16_one(voffW, w, dstW + off);
        else glds16_pair(voffW, voffW + 32, w, dstW + off, dstW + off + 1024);
        const int g = p.G == 1 ? 0 : tw >> 1;
        if (zp_wave) glds1_one(voffS, srcS + g, dstS + off);
        else glds4_one(voffS, srcS + (size_t)g * 4, dstS + off);
    };

    // ---- fragment read geometry (per lane), byte offsets inside the X tile / the image ----
    const int lr = lane & 31, lh = lane >> 5;
    int xoff[4], woff[4];                                       // k-step s: chunk 2 s + lh; rows + 32: 4 pieces further
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        xoff[s] = tile_img(64 * wave_m + lr, 2 * s + lh);
        woff[s] = tile_img(64 * wave_n + lr, 2 * s + lh);
    }
    // ---- dequantise geometry: the lane's packed bytes, its scale, and where its four chunks go ----
    const int poff = TX_BYTES + wave * (1024 * WI) + 16 * lane; // int8: the second piece 1 KiB further
    const int soff = TX_BYTES + W_BYTES + 4 * drow;
    const bool drow_ok = drow <= b_last;
    const float off_u = INT4 ? 8.0f : 128.0f;
    int doff[4];                                                // chunk j of the lane's 32 weights
#pragma unroll
    for (int j = 0; j < 4; ++j)                                 // int4: columns 32 (lane & 1) + 8 j; int8: 16 ((lane & 1) + 2 (j >> 1)) + 8 (j & 1)
        doff[j] = tile_img(drow, INT4 ? 4 * (lane & 1) + j : 2 * ((lane & 1) + 2 * (j >> 1)) + (j & 1));

    unsigned pk[4 * WI];                                        // the lane's packed words of the K-tile being dequantised
    float dsc, dcz;
    auto load_packed = [&](const char* base) {
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            const u32x4 v = *(const u32x4*)(base + poff + 1024 * i);
            pk[4 * i] = v.x, pk[4 * i + 1] = v.y, pk[4 * i + 2] = v.z, pk[4 * i + 3] = v.w;
        }
        const float s = *(const float*)(base + soff);
        dsc = drow_ok ? s : 0.0f;
        dcz = off_u;
        if constexpr (ZP) dcz = off_u + (float)(int)(signed char)(*(const int*)(base + soff + TT * 4) & 0xff);
    };
    // chunk j: 8 weights -> w = round_to_dtype((u - cz) s), 16 bytes into the image
    auto dequant_chunk = [&](int j, char* image) {
        float u[8];
        if constexpr (INT4) u_int4(pk[j], u);
        else u_int8(pk[2 * j], pk[2 * j + 1], u);
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float d = u[i] - dcz;
            f[i] = d * dsc;
        }
        *(u32x4*)(image + doff[j]) =
            (u32x4){pack2<DT>(f[0], f[1]), pack2<DT>(f[2], f[3]), pack2<DT>(f[4], f[5]), pack2<DT>(f[6], f[7])};
    };

    f32x16 acc[2][2];                                           // [nj][mi]: D rows = columns n, D columns = rows m
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nj][mi][r] = 0.0f;

    // slot = t % 3 and ib = t & 1 are scalars carried beside t: one copy of the phase
    auto phase = [&](int t, int slot, int ib) {
        if (t + 1 < nt) wait_vmcnt<NI>();                       // unit t has landed; unit t + 1 stays in flight
        else wait_vmcnt<0>();                                   // drain: the last unit
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");                          // no LDS access moves in front of the barrier
        if (t + TLEAD < nt) issue(t + TLEAD, slot == 0 ? TLEAD : slot - 1);     // (slot + 2) % 3
        const char* base = ring + slot * SLOT_BYTES;
        const char* wimg = img + ib * TX_BYTES;
        char* dimg = img + (ib ^ 1) * TX_BYTES;
        u32x4 fx[2][4], fw[2][4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                fw[h][s] = *(const u32x4*)(wimg + woff[s] + h * 4096);
                fx[h][s] = *(const u32x4*)(base + xoff[s] + h * 4096);
            }
        load_packed(base);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int nj = 0; nj < 2; ++nj)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) acc[nj][mi] = tile_mfma<DT>(fw[nj][s], fx[mi][s], acc[nj][mi]);
            dequant_chunk(s, dimg);
        }
    };

    issue(-1, TSLOTS - 1);
    issue(0, 0);
    issue(1, 1);
    wait_vmcnt<2 * NI>();                                       // unit -1 has landed
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    load_packed(ring + (TSLOTS - 1) * SLOT_BYTES);
#pragma unroll
    for (int j = 0; j < 4; ++j) dequant_chunk(j, img);
    for (int t = 0, slot = 0; t < nt; ++t, slot = slot == TSLOTS - 1 ? 0 : slot + 1) phase(t, slot, t & 1);

    // ---- epilogue: y = acc (+ bias[n]), one rounding; element 4 j + i of (nj, mi) is column n + i of row m ----
    const bool has_bias = p.bias != nullptr;
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nn = n0 + 64 * wave_n + 32 * nj + 8 * j + 4 * lh;
            if (nn >= p.N) continue;
            float b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = (has_bias && nn + i < p.N) ? h2f<DT>(p.bias[nn + i]) : 0.0f;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int64_t m = (int64_t)m0 + 64 * wave_m + 32 * mi + lr;
                if (m >= p.M) continue;
                float y[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    y[i] = acc[nj][mi][4 * j + i];
                    if (has_bias) y[i] = y[i] + b[i];
                }
                unsigned short* dst = p.Y + m * p.ldy + nn;
                if (p.vec && nn + 3 < p.N) {                    // vec: Y and its pitch are 8-byte aligned
                    *(uint2*)dst = make_uint2(pack2<DT>(y[0], y[1]), pack2<DT>(y[2], y[3]));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (nn + i < p.N) dst[i] = (unsigned short)(pack2<DT>(y[i], 0.0f) & 0xffffu);
                }
            }
        }
    }
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
