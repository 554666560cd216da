// qt_w4_short_gemm_i8: the short-prompt form of qt_gemm_i8 for W4A8 (packed int4 weights, one scale per group of 128
// columns), for the rows between qt_gemm_i8_mid (<= 128) and qt_gemm_i8_ring_w4 (>= 8192): a 128 x 128 output tile per
// workgroup of four waves, two workgroups resident per CU, operands by LDS-DMA into a ring of three K-tiles, the packed
// weights unpacked at the fragment read, and the group fold of one accumulator set running beside the MFMAs that fill
// the other.  Y is equal to qt_gemm_i8's to the bit (include/quantool_amd.h).
//
// THE TILE.  Wave w owns the 64 x 64 sub-tile (w >> 1, w & 1) as 2 x 2 v_mfma_i32_32x32x32_i8 (mi: A half of 32 rows,
// nj: B half of 32 columns).  A K-tile is 128 k-bytes = exactly one weight group g = t, so the int32 result of the four
// k-steps of one (mi, nj) IS acc_g for its 32 x 32 outputs: complete and exact whatever order its k-bytes were summed
// in.  Two accumulator sets of 2 x i32x16 per lane exist, set nj for B half nj.  Phase t (K-tile t) runs
//     half 0:  8 MFMAs fill set 0 (K-tile t, nj 0)   beside   the fold of set 1 (K-tile t - 1, nj 1)
//     half 1:  8 MFMAs fill set 1 (K-tile t, nj 1)   beside   the fold of set 0 (K-tile t,     nj 0)
// one fold chunk (4 outputs per lane) written behind each MFMA, so that a wave's VALU work has an MFMA of its own to
// run under, and the second workgroup on the CU supplies another wave per SIMD for what is left.  Before phase 0 set 1
// is 0 with s_w = 0: tot stays +0; the last fold of set 1 runs behind the loop.  Only nj 1's s_w / wsum are carried
// from one phase into the next (two registers).
// THE FOLD is gemm_i8_kernel's GROUPED branch statement for statement, once per element and group, g ascending:
//     t = (float)(acc - zp_x[m] * wsum[n, g]);  prod = s_w[n, g] * t;  tot = tot + prod;
// and the epilogue y = s_x[m] * tot (+ bias), under the same -ffp-contract=off.  zp * wsum is a 24-bit multiply
// (|zp| <= 128, |wsum| <= 128 * 8: exact).  prod and tot are held as pairs of floats, so hipcc may use the packed fp32
// multiply and add (two elements per instruction, each rounded on its own); with contraction off it may not fuse them.
// The tile's 128 row zero-points sit in LDS and are re-read per fold (an opaque zero offset keeps hipcc from hoisting
// 32 of them per lane into registers, as in gemm_i8_kernel).
//
// THE UNITS.  K-tile t lives in slot t % 3 of 25 KiB:
//   A       128 rows x 128 k-bytes, 16 KiB, 4 LDS-DMA (dwordx4) per wave: i8_ring_tile.h's LDS image (piece = 8 rows x
//           128 B, 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7)); wave w fills pieces 4 w .. 4 w + 3.
//   B       128 rows x 128 k = 64 packed bytes per row, 8 KiB, 2 LDS-DMA per wave: qlinear_ring_w4.hip's image (piece =
//           16 rows x 64 B, chunk c (0..3) of row r at chunk c ^ ((r >> 2) & 3)); wave w fills pieces 2 w, 2 w + 1.
//   scales  s_w[n, t] of the tile's 128 columns (waves 0, 1: column 64 w + lane) and wsum[n, t] (waves 2, 3; s_w again
//           when the activations are symmetric, so that the count does not depend on the form), one dword per lane
//           (global_load_lds_dword), 1 KiB behind the B unit.
//   7 LDS-DMA instructions per wave and K-tile.  No other global load runs inside the loop.
// K-SPLIT OF A K-TILE OVER THE MFMA k-steps: as qlinear_ring_w4.hip.  Lane half lh takes k-bytes [64 lh, 64 lh + 64):
// k-step s is A chunk 4 lh + s and packed B bytes [32 lh + 8 s, + 8).  A B half is two ds_read_b128 per lane and K-tile,
// kept packed in registers (8 per lane and half) and unpacked with unpack_int4_word between the MFMAs.
//
// HAZARDS (R 3 slots, lead L 2 K-tiles, one workgroup barrier per K-tile, no stagger: the four waves run one program).
//   phase t = { counted vmcnt ; lgkmcnt(0) ; s_barrier(t) ; issue K-tile t + 2 into slot (t + 2) % 3 ; fragment,
//               packed-B and scale reads of slot t % 3 ; half 0 ; half 1 }
//   In front of the wait of phase t a wave has K-tiles t and t + 1 outstanding, 7 instructions each: vmcnt(7) retires
//   its part of K-tile t and leaves K-tile t + 1 in flight under the MFMAs of phase t, with K-tile t + 2 joining it
//   behind the barrier: two K-tiles = 50 KiB per workgroup in flight in the steady state.
//   RAW: every wave retires its part of K-tile t in front of s_barrier(t); the reads of slot t % 3 follow it.
//   WAR: slot (t + 2) % 3 held K-tile t - 1.  All of a wave's reads of it -- fragments, packed B, scales -- are issued
//        in phase t - 1 and retired by the lgkmcnt(0) in front of s_barrier(t); the issue follows that barrier.  The
//        fold of K-tile t - 1's set 1 in phase t reads registers and the zero-points only, never the ring.
//        (L = 3 = R would put the issue of K-tile t + 3 into slot t % 3 in phase t, beside the reads of K-tile t.)
//   Prologue: K-tiles 0 and 1 (if there is one) are issued; phase 0's wait is the loop's.
//   Drain: phase t with t + 2 >= nt issues nothing; the last phase (t + 1 == nt) has only its own K-tile outstanding
//        and waits vmcnt(0): the one place.  The row zero-points are stored and a barrier passed before any LDS-DMA.
// LDS: 512 B of zero-points + 3 x 25 KiB = 77 312 B <= 80 KiB: two workgroups per CU.  REGISTERS (budget 256 at two
// waves per SIMD): tot 64, two accumulator sets 64, A fragments of a K-tile 32, packed B 16, one unpacked k-step 4, DMA
// offsets 7; the figures of the build are in DESIGN.md 4.28.  The kernel is in csrc/build.py's spill and M0 audits.
// EDGES: a tile row past M (N) is fetched from row M - 1 (N - 1) -- data, scales and wsum -- is computed and never
// stored; K is a whole number of K-tiles and G = K / 128, so no byte outside Xq[M, K], Wq[N, K/8], s_w / wsum[N, G],
// s_x / zp_x[M] is read, and nothing outside Y[m < M, n < N] is written.
#include "common.h"
#include "i8_args.h"
#include "i8_unpack.h"
#include "i8_ring_tile.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int ST = 128;                      // output tile edge
constexpr int SKU = 128;                     // k per K-tile = the weight group
constexpr int SLOTS = 3;                     // K-tiles resident in LDS
constexpr int SLEAD = 2;                     // K-tile t + SLEAD is issued in phase t
constexpr int STHREADS = 256;                // 4 waves: 2 (M) x 2 (N), 64 x 64 outputs per wave
constexpr int A_BYTES = ST * SKU;            // 16 KiB
constexpr int B_BYTES = ST * SKU / 2;        // 8 KiB
constexpr int S_BYTES = 2 * ST * 4;          // 128 s_w, 128 wsum
constexpr int SLOT_BYTES = A_BYTES + B_BYTES + S_BYTES;
constexpr int ZP_BYTES = ST * 4;
static_assert(ZP_BYTES + SLOTS * SLOT_BYTES <= 80 * 1024, "two workgroups per CU");
static_assert(SLEAD <= SLOTS - 1, "WAR: see the head comment");

struct W4ShortArgs {
    const int8_t* Xq;
    const int8_t* Wq;                        // packed: K / 2 bytes per row
    const float* s_x;
    const int32_t* zp_x;
    const float* s_w;
    const int32_t* wsum;
    const void* bias;
    void* Y;
    int64_t M;
    int N, K, G;
    int64_t ldy;
    int out_dtype;
};

// One 128 x 128 tile of Y: rows [m0, m0 + 128) of the matrix that ends at row p.M, columns [n0, n0 + 128).  The body a
// grouped (expert-bank) form would wrap, as ring_w4_tile is.
template <bool ASYM>
__device__ __forceinline__ void w4_short_tile(const W4ShortArgs& p, int64_t m0, int n0) {
    __shared__ __attribute__((aligned(16))) char lds[ZP_BYTES + SLOTS * SLOT_BYTES];
    int* sZp = (int*)lds;
    char* ring = lds + ZP_BYTES;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1;
    const int K = p.K, G = p.G;
    const int Kb = K / 2;                             // bytes of a packed weight row
    const int nt = K / SKU;                           // K-tiles = phases
    const int64_t a_last = p.M - 1 - m0;              // last valid row of the A panel, relative to the tile
    const int b_last = p.N - 1 - n0;                  // last valid row of the B panel

    // the tile's row zero-points, before any LDS-DMA is in flight (plain loads: nothing counted yet)
    // (stored in the symmetric form too: the block's one plain store, everything else arrives by LDS-DMA)
    if (tid < ST) sZp[tid] = (ASYM && m0 + tid < p.M) ? p.zp_x[m0 + tid] : 0;
    __syncthreads();

    // ---- staging geometry: source byte offsets of this lane's 7 LDS-DMA instructions, relative to the K-tile ----
    unsigned voffA[4], voffB[2], voffS;
#pragma unroll
    for (int i = 0; i < 4; ++i) {                     // piece 4 wave + i: row 8 piece + (lane >> 3), physical chunk lane & 7
        const int r = 32 * wave + 8 * i + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        const int64_t ra = r < a_last ? r : a_last;
        voffA[i] = (unsigned)((size_t)ra * K + 16 * c);                 // < 128 * 32768
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {                     // piece 2 wave + i: row 16 piece + (lane >> 2), physical chunk lane & 3
        const int r = 32 * wave + 16 * i + (lane >> 2);
        const int c = (lane & 3) ^ ((r >> 2) & 3);
        const int rb = r < b_last ? r : b_last;
        voffB[i] = (unsigned)((size_t)rb * Kb + 16 * c);                // < 128 * 16384
    }
    {
        const int col = wave_n * 64 + lane;           // waves 0, 2: columns 0..63; waves 1, 3: 64..127
        voffS = (unsigned)((size_t)(col < b_last ? col : b_last) * G * 4);   // < 128 * 256 * 4
    }
    const unsigned ring_lds = (unsigned)(size_t)(QT_LDS char*)ring;
    const unsigned dstA_wave = __builtin_amdgcn_readfirstlane(ring_lds + wave * 4096);
    const unsigned dstB_wave = __builtin_amdgcn_readfirstlane(ring_lds + A_BYTES + wave * 2048);
    // waves 0, 1: s_w at dwords [64 wave_n, + 64); waves 2, 3: wsum at 128 + the same
    const unsigned dstS_wave = __builtin_amdgcn_readfirstlane(ring_lds + A_BYTES + B_BYTES + wave_m * 512 + wave_n * 256);
    const int8_t* srcA = p.Xq + m0 * (int64_t)K;      // scalar: k-byte 0 of the tile's first row
    const int8_t* srcB = p.Wq + (int64_t)n0 * Kb;
    const char* srcS = ((ASYM && wave_m) ? (const char*)p.wsum : (const char*)p.s_w) + (size_t)n0 * G * 4;
    auto issue = [&](int t, int slot) {
        const unsigned off = (unsigned)slot * SLOT_BYTES;
        const int8_t* a = srcA + (size_t)t * SKU;
        glds16_pair(voffA[0], voffA[1], a, dstA_wave + off, dstA_wave + off + 1024);
        glds16_pair(voffA[2], voffA[3], a, dstA_wave + off + 2048, dstA_wave + off + 3072);
        glds16_pair(voffB[0], voffB[1], srcB + (size_t)t * (SKU / 2), dstB_wave + off, dstB_wave + off + 1024);
        glds4_one(voffS, srcS + (size_t)t * 4, dstS_wave + off);
    };

    // ---- fragment read geometry (per lane), byte offsets inside a slot ----
    const int lr = lane & 31, lh = lane >> 5;
    // A: row r + 32 (mi = 1) is 4 pieces further with the same swizzle; B: row r + 32 (nj = 1) is 2 pieces further, and
    // chunk 2 lh + 1 is chunk 2 lh with bit 0 flipped
    int aoff[4], boff, soff;
    {
        const int r = wave_m * 64 + lr;
#pragma unroll
        for (int s = 0; s < 4; ++s)                   // k-step s: chunk 4 lh + s
            aoff[s] = (r >> 3) * 1024 + (r & 7) * 128 + 16 * ((4 * lh + s) ^ ((r >> 1) & 7));
    }
    {
        const int r = wave_n * 64 + lr;               // packed chunk 2 lh + j: k-steps 2 j, 2 j + 1
        boff = A_BYTES + (r >> 4) * 1024 + (r & 15) * 64 + 16 * ((2 * lh) ^ ((r >> 2) & 3));
        soff = A_BYTES + B_BYTES + 4 * r;
    }
    const int zrow = wave_m * 64 + 4 * lh;            // first zero-point row of this lane's C/D rows

    f32x2 tot[2][2][8];                               // [mi][nj][r >> 1]: element r of the 32 x 32 C/D map
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj)
#pragma unroll
            for (int r = 0; r < 8; ++r) tot[mi][nj][r] = (f32x2){0.0f, 0.0f};
    i32x16 acc[2][2] = {{(i32x16){}, (i32x16){}}, {(i32x16){}, (i32x16){}}};   // [set = nj][mi]
    float sw[2] = {0.0f, 0.0f}, swp = 0.0f;           // s_w[n, t] per B half; nj 1's of the K-tile before
    int ws[2] = {0, 0}, wsp = 0;                      // wsum[n, t] likewise
    i32x4 fa[2][4], pb[2][2];                         // A: [mi][k-step]; packed B: [nj][chunk]

    // the zero-points of chunk c of a fold: rows 8 (c & 3) + 4 lh + 0..3 of the 32 x 32 tile c >> 2, one ds_read_b128
    auto zp_chunk = [&](int c) -> i32x4 {
        i32x4 z = {};
        if (ASYM) {
            int zoff = 0;
            asm volatile("" : "+v"(zoff));
            z = *(const i32x4*)&sZp[zrow + (c >> 2) * 32 + 8 * (c & 3) + zoff];
        }
        return z;
    };
    // chunk c of set NJ's fold: tot += s_w * (float)(acc - zp * wsum), four outputs per lane.  nws = -wsum: acc - zp wsum
    // = acc + zp (-wsum) exactly (24-bit operands, 32-bit wrap-free sum), one multiply-add
    auto fold_chunk = [&](auto nj_c, int c, const i32x4 z, float swf, int nws) {
        constexpr int NJ = decltype(nj_c)::value;
        const int mi = c >> 2, k = c & 3;
        const f32x2 s2 = {swf, swf};
#pragma unroll
        for (int jp = 0; jp < 2; ++jp) {
            int a0 = acc[NJ][mi][4 * k + 2 * jp], a1 = acc[NJ][mi][4 * k + 2 * jp + 1];
            if (ASYM) {
                a0 = __mul24(z[2 * jp], nws) + a0;
                a1 = __mul24(z[2 * jp + 1], nws) + a1;
            }
            const f32x2 t = {(float)a0, (float)a1};
            const f32x2 prod = s2 * t;
            tot[mi][NJ][2 * k + jp] = tot[mi][NJ][2 * k + jp] + prod;
        }
    };
    // half NJ of a phase: the 8 MFMAs of B half NJ into set NJ, one chunk of the other set's fold behind each; the two
    // chunks' zero-points are read one k-step ahead
    auto half = [&](auto nj_c, float swf, int wsf) {
        constexpr int NJ = decltype(nj_c)::value;
        const int nws = -wsf;
        i32x4 z[2] = {zp_chunk(0), zp_chunk(1)};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            i32x4 zn[2] = {z[0], z[1]};
            if (s < 3) {
                zn[0] = zp_chunk(2 * s + 2);
                zn[1] = zp_chunk(2 * s + 3);
            }
            const uint2 lo = unpack_int4_word((unsigned)pb[NJ][s >> 1][2 * (s & 1)]);
            const uint2 hi = unpack_int4_word((unsigned)pb[NJ][s >> 1][2 * (s & 1) + 1]);
            const i32x4 fb = {(int)lo.x, (int)lo.y, (int)hi.x, (int)hi.y};
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                acc[NJ][mi] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[mi][s], fb, s == 0 ? (i32x16){} : acc[NJ][mi],
                                                                    0, 0, 0);
                fold_chunk(std::integral_constant<int, NJ ^ 1>{}, 2 * s + mi, z[mi], swf, nws);
            }
            z[0] = zn[0];
            z[1] = zn[1];
            // a k-step's unpack stays with its MFMAs: hoisted, the unpacked B of a whole half would be live at once
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // slot = t % 3, a scalar carried beside t: one copy of the phase, its LDS addresses a lane offset + the slot's base
    auto phase = [&](int t, int slot) {
        if (t + 1 < nt) wait_vmcnt<7>();              // K-tile t has landed; K-tile t + 1 stays in flight
        else wait_vmcnt<0>();                         // drain: the last K-tile
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");                // no read of the ring moves in front of the barrier
        if (t + SLEAD < nt) issue(t + SLEAD, slot == 0 ? SLEAD : slot - 1);   // (slot + 2) % 3
        const char* base = ring + slot * SLOT_BYTES;
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) fa[mi][s] = *(const i32x4*)(base + aoff[s] + mi * 4096);
#pragma unroll
        for (int nj = 0; nj < 2; ++nj) {
#pragma unroll
            for (int j = 0; j < 2; ++j) pb[nj][j] = *(const i32x4*)(base + (boff ^ (16 * j)) + nj * 2048);
            sw[nj] = *(const float*)(base + soff + nj * 128);
            if (ASYM) ws[nj] = *(const int*)(base + soff + ST * 4 + nj * 128);
        }
        half(std::integral_constant<int, 0>{}, swp, wsp);       // fold of K-tile t - 1, nj 1
        half(std::integral_constant<int, 1>{}, sw[0], ws[0]);   // fold of K-tile t, nj 0
        swp = sw[1];
        wsp = ws[1];
    };

    issue(0, 0);
    if (nt > 1) issue(1, 1);
    for (int t = 0, slot = 0; t < nt; ++t, slot = slot == SLOTS - 1 ? 0 : slot + 1) phase(t, slot);
#pragma unroll
    for (int c = 0; c < 8; ++c)                       // the last K-tile's nj 1
        fold_chunk(std::integral_constant<int, 1>{}, c, zp_chunk(c), swp, -wsp);

    // ---- epilogue: y = s_x[m] * tot (+ bias[n]), once per output element, by the lane that holds it ----
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
        const int n = n0 + wave_n * 64 + nj * 32 + lr;
        if (n >= p.N) continue;
        float bn = 0.0f;
        const bool has_bias = p.bias != nullptr;
        if (has_bias) bn = qt_load_w(p.bias, p.out_dtype, n);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = i8_ring_cd_row(m0 + wave_m * 64 + mi * 32, r, lh);
                if (m >= p.M) continue;
                float y = p.s_x[m] * tot[mi][nj][r >> 1][r & 1];
                if (has_bias) y = y + bn;
                qt_store_w(p.Y, p.out_dtype, (size_t)(m * p.ldy + n), y);
            }
        }
    }
}

template <bool ASYM>
__global__ __launch_bounds__(STHREADS, 2) void gemm_i8_w4_short_kernel(const W4ShortArgs p) {
    // tile order: GROUP_M m-tiles walk the n-tiles together (as gemm_i8_kernel), so that a weight tile is shared in L2
    const int tiles_n = (p.N + ST - 1) / ST;
    const int tiles_m = (int)((p.M + ST - 1) / ST);
    int m_tile, n_tile;
    i8_ring_tile_of(blockIdx.x, tiles_m, tiles_n, m_tile, n_tile);
    w4_short_tile<ASYM>(p, (int64_t)m_tile * ST, n_tile * ST);
}

}  // namespace

extern "C" int qt_w4_short_gemm_i8(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N,
                                   const float* s_x, const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum,
                                   const void* bias, void* Y, int out_dtype, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int st = qt_i8_check_packed_g128("qt_w4_short_gemm_i8", "qt_gemm_i8_ring", Xq, M, K, Wq, w_format, N, s_x, zp_x,
                                         s_w, G, wsum, Y, out_dtype, ldy))
        return st;
    static_assert(QT_I8_W4_SHORT_K_UNIT == SKU && QT_I8_W4_SHORT_SLOTS == SLOTS && QT_I8_W4_SHORT_LEAD == SLEAD,
                  "header constants");
    const int64_t tiles_m = (M + ST - 1) / ST;
    const int64_t tiles = tiles_m * (int64_t)((N + ST - 1) / ST);
    QT_CHECK_ARG(tiles_m <= 0x7fffffffLL && tiles <= 0x7fffffffLL, "qt_w4_short_gemm_i8: too many tiles");
    W4ShortArgs a{Xq, (const int8_t*)Wq, s_x, zp_x, s_w, wsum, bias, Y, M, N, K, G, ldy, out_dtype};
    if (zp_x) hipLaunchKernelGGL(gemm_i8_w4_short_kernel<true>, dim3((unsigned)tiles), dim3(STHREADS), 0, stream, a);
    else hipLaunchKernelGGL(gemm_i8_w4_short_kernel<false>, dim3((unsigned)tiles), dim3(STHREADS), 0, stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
