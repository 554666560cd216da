// qt_gemm_i8_ring_w4: the prefill / perplexity form of qt_gemm_i8 for W4A8 (packed int4 weights, one scale per group of
// 128 columns): qlinear_ring.hip's 256 x 256 tile and pipeline (ring_pipe.h: 8 waves, units A0, B0, B1, A1 per K-tile,
// one unit issued per phase, counted vmcnt, two-group stagger; what the two files share is in i8_ring_tile.h) with
// packed B units and the grouped fold in every phase.
// Y is equal to qt_gemm_i8's to the bit (include/quantool_amd.h).
//
// WHY THE FOLD FITS.  A K-tile is 128 k-bytes = exactly one weight group g = t, and phase 4t + q computes quadrant q
// (A half x B half) of the output tile over that whole K-tile.  So the int32 result of one phase IS acc_g for its
// 64 x 32 outputs per wave: complete, exact, whatever order its k-bytes were summed in.  It is a per-phase temporary
// (2 x i32x16 per lane, the first MFMA takes a zero C); only tot (4 quadrants x 2 x f32x16 = 128 fp32 per lane)
// persists.  The fold is gemm_i8_kernel's GROUPED branch statement for statement, once per element and group, g
// ascending:  t = (float)(acc - zp_x[m] * wsum[n, g]);  prod = s_w[n, g] * t;  tot = tot + prod;  and the epilogue
// y = s_x[m] * tot (+ bias), under the same -ffp-contract=off.  zp * wsum is a 24-bit multiply (|zp| <= 128,
// |wsum| <= 128 * 8: exact).  The fold of phase u runs in LOAD(u + 1), so under the partner group's MFMAs; the
// last one runs behind the loop.  The tile's 256 row zero-points sit in LDS and are re-read per phase (an opaque
// zero offset keeps hipcc from hoisting 64 of them per lane into registers, as in gemm_i8_kernel).
//
// THE UNITS.  K-tile t = units 4t .. 4t+3, slot = unit % 8 of 16 KiB each (A0, B0, B1, A1 at slots (4t & 4) + 0..3):
//   A0, A1  128 rows x 128 k-bytes, 16 KiB, 2 LDS-DMA (dwordx4) per wave: i8_ring_tile.h's unit and LDS image
//           (piece = 8 rows x 128 B, 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7)).
//   B0, B1  128 rows x 128 k = 64 packed bytes per row, 8 KiB (the lower half of the slot), 1 LDS-DMA per wave.
//           LDS image: 8 pieces of 1 KiB, piece = 16 rows x 64 B (wave w fills piece w lane-linear); the 16-byte
//           chunk c (0..3) of row r sits at chunk c ^ ((r >> 2) & 3) of its row (the XOR is on the source address).
//           A fragment read takes 16 lanes = 16 consecutive rows at one logical chunk: 4 rows span the 64 banks, and
//           rows r, r+4, r+8, r+12 land on the four different chunks, so each 16-lane group covers all banks once.
//   scales  s_w[n, t] and wsum[n, t] of the tile's 256 columns ride with A0 as a third instruction of that unit
//           (the DMA route): waves 0-3 gather s_w of columns 64 (w & 3) + lane, waves 4-7 wsum (s_w again when the
//           activations are symmetric, so the count does not depend on the form), one dword per lane
//           (global_load_lds_dword), into sc[t & 1] (2 x 2 KiB beside the ring).  They are read in LOAD(4t) only, as
//           A0 is, so A0's RAW / WAR argument covers them.  No other global load runs inside the loop.
// K-SPLIT OF A K-TILE OVER THE MFMA k-steps.  acc_g is order-free, so lane half lh takes k-bytes [64 lh, 64 lh + 64)
// of the K-tile: k-step s is A chunk 4 lh + s and packed B bytes [32 lh + 8 s, + 8).  A B half is then two
// ds_read_b128 per lane and K-tile (chunks 2 lh, 2 lh + 1), kept packed in registers (16 per lane for B0 and B1) and
// unpacked with unpack_int4_word between the MFMAs of every phase that uses them.
//
// HAZARDS (ring_pipe.h; R 8, L 6).  Instructions per wave: A0 3, B0 1, B1 1, A1 2 = 7 per K-tile, and ANY four
// consecutive units hold 7.
//   RAW: as qlinear_ring.hip, unit i is first read in phase i - 1 at the earliest, so the counted wait of phase u may
//        leave units u+3 .. u+6 in flight: four consecutive units = vmcnt(7), a constant.
//   WAR: unit i is last read in phase i, its slot is re-filled by unit i + 8, issued in phase i + 2: case L = R - 2.
//   Prologue: units 0 .. 5 are issued (3+1+1+2+3+1 = 11), units 2 .. 5 may stay in flight: 1+2+3+1 = vmcnt(7).
//        One K-tile only (nu = 4): units 0 .. 3 issued, units 2, 3 stay: vmcnt(3).
//   Drain: a phase u with u + 6 >= nu issues nothing and may leave units u+3 .. nu-1 in flight.  nu is a multiple of
//        4, so those are the last nu - u - 3 units of the last K-tile, and the phase's position q = u & 3 fixes them:
//          u = nu - 6 (q 2): B0, B1, A1 = vmcnt(4)     u = nu - 5 (q 3): B1, A1 = vmcnt(3)
//          u = nu - 4 (q 0): A1 = vmcnt(2)              later phases: vmcnt(0)
// REGISTERS: tot 128, acc 32, A fragments 32, packed B 16, one unpacked k-step 4, addresses and scales ~20; the
// figures of the build are in DESIGN.md 4.15.  The kernel is in csrc/build.py's spill and M0 audits.
// EDGES: as qlinear_ring.hip.  A tile row past M (N) is fetched from row M - 1 (N - 1) -- data, scales and wsum -- is
// computed and never stored; K is a whole number of K-tiles and G = K / 128, so no byte outside Xq[M, K],
// Wq[N, K/8], s_w / wsum[N, G], s_x / zp_x[M] is read.
//
// qt_moe_gemm_i8_ring_w4: the same tile over E packed weight matrices (ring_w4_tile<ASYM, true>), equal to
// qt_gemm_i8_grouped to the bit.  All it does differently lies outside the K loop.  The grid holds
// ceil(R/256) + E m-tile slots per n-tile; a workgroup walks the clamped offsets (i8_ring_tile.h) to its expert e, its
// first row m0 and the expert's end m_end, and a surplus one returns before the fills, their barrier and any LDS-DMA.
// e, m0 and m_end are wave-uniform, so the MOE bases are scalar as the dense ones are: srcB = Wq + (e N + n0) K/2 (K a
// multiple of 128 keeps every expert's matrix 16-byte aligned), srcS = (s_w | wsum) + (e N + n0) G 4, and for
// contiguous rows srcA = Xq + m0 K with rows clamped to m_end - 1.  The Xq / s_x / zp_x row of each of the tile's 256
// rows -- row_idx[m] clamped into [0, x_rows), or m -- is staged in LDS beside sZp (sRow, 1 KiB: 153 600 B in all)
// by the threads that fill sZp, and read from there for the A offsets (with row_idx the base is Xq itself and each
// lane's four A offsets are sRow[r] K + 16 c < x_rows K <= 2^32, written into sOff as ever) and for the epilogue's s_x.
// Nothing new is live in the loop.  A tile row past m_end takes the source row of m_end - 1 and is never stored.
#include "common.h"
#include "i8_args.h"
#include "i8_unpack.h"
#include "i8_ring_tile.h"

namespace {

// i8_ring_tile.h's instance with KU = the weight group; a B unit fills the lower half of its slot
constexpr int SC_BYTES = 2048;               // one K-tile's scales: 256 s_w, 256 wsum

struct RingW4Args {
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

template <bool ASYM, bool MOE>
__device__ __forceinline__ void ring_w4_tile(const RingW4Args& p, const RingMoe& g) {
    // one LDS block, the small tables first: their addresses (and those of the scales) then fit the 16-bit offset field
    // of a DS instruction and hold no register each.  The ring's slots lie beyond 64 KiB: see tile_base below.
    //   sOff  each thread's LDS-DMA source offsets {A0 i0, A0 i1, scales, -, A1 i0, A1 i1, B0, B1}, 32 B per thread:
    //         read back by their owner in front of the issue, so that they hold no registers across the phases
    //   sZp   the tile's 256 row zero-points;  sRow  (MOE) the Xq / s_x / zp_x row of each of the tile's 256 rows;
    //   sc  two K-tiles' scales;  ring  the 8 slots
    constexpr int ROW_BYTES = MOE ? BT * 4 : 0;
    __shared__ __attribute__((aligned(16))) char lds[NTHREADS * 32 + BT * 4 + ROW_BYTES + 2 * SC_BYTES +
                                                     RING * UNIT_BYTES];
    unsigned* sOff = (unsigned*)lds;
    int* sZp = (int*)(lds + NTHREADS * 32);
    [[maybe_unused]] int* sRow = (int*)(lds + NTHREADS * 32 + BT * 4);
    int* sc = (int*)(lds + NTHREADS * 32 + BT * 4 + ROW_BYTES);
    char* ring = lds + NTHREADS * 32 + BT * 4 + ROW_BYTES + 2 * SC_BYTES;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 2, wave_n = wave & 3;
    const bool group_b = wave >= 4;  // wave-uniform

    const int tiles_n = (p.N + BT - 1) / BT;
    const int tiles_m = (int)((p.M + BT - 1) / BT) + (MOE ? g.E : 0);
    int m_tile, n_tile;                               // the grouped form: m_tile is an m-tile slot
    i8_ring_tile_of(blockIdx.x, tiles_m, tiles_n, m_tile, n_tile);
    int64_t m0 = (int64_t)m_tile * BT;
    int64_t m_end = p.M;                              // rows [m0, m_end) of this tile's matrix exist
    const int n0 = n_tile * BT;
    const int K = p.K, G = p.G;
    const int Kb = K / 2;                             // bytes of a packed weight row
    const int nu = K / KU * 4;                        // units = phases
    int64_t w_row0 = n0;                              // the tile's first row of Wq / s_w / wsum: e N + n0
    if constexpr (MOE) {
        // m-tile slot -> (expert, tile within the expert): i8_ring_tile.h.  A surplus workgroup returns: uniform, before
        // the fills below, their barrier and any LDS-DMA; p.M = R <= 0x7fffffff (host)
        int e, lo_e, hi_e;
        if (!i8_ring_moe_walk(g, (int)p.M, m_tile, e, lo_e, hi_e)) return;
        e = __builtin_amdgcn_readfirstlane(e);        // wave-uniform: every base below stays scalar
        m0 = __builtin_amdgcn_readfirstlane(lo_e);
        m_end = __builtin_amdgcn_readfirstlane(hi_e);
        w_row0 = (int64_t)e * p.N + n0;
    }
    const int64_t a_last = m_end - 1 - m0;            // last valid row of the A panel, relative to the tile

    // the tile's row zero-points (and source rows), before any LDS-DMA is in flight (plain loads: nothing counted yet)
    if constexpr (MOE) {
        // a tile row past the expert's last row takes that row's source: fetched again, computed and never stored
        if (tid < BT) {
            const int64_t ms = i8_ring_moe_src_row(g, m0 + (tid < a_last ? tid : a_last));
            sRow[tid] = (int)ms;                      // < x_rows, R <= 2^31 - 1
            if (ASYM) sZp[tid] = (m0 + tid < m_end) ? p.zp_x[ms] : 0;
        }
    } else if (ASYM) {
        if (tid < BT) sZp[tid] = (m0 + tid < m_end) ? p.zp_x[m0 + tid] : 0;
    }
    __syncthreads();

    // ---- staging geometry ----
    // A: two LDS-DMA instructions per thread and unit (i8_ring_tile.h)
    // B: one; lane: row 16 wave + (lane >> 2) of the half panel, physical chunk lane & 3
    // scales: one dword per lane, column 64 (wave & 3) + lane of the tile
    const int b_last = p.N - 1 - n0;                  // last valid row of the B panel, relative to the tile
    {
        unsigned voffA[2][2], voffB[2], voffS;        // [half][instruction], [half]
#pragma unroll
        for (int i = 0; i < 2; ++i)
            i8_ring_a_voff(wave, lane, i, a_last, K, [](int64_t ra) { return ra; }, voffA[0][i], voffA[1][i]);
        if constexpr (MOE) {
            if (g.row_idx) {                          // gathered rows: offsets from Xq itself, < x_rows K <= 2^32
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    i8_ring_a_voff(wave, lane, i, a_last, K, [&](int64_t ra) { return (int64_t)sRow[ra]; }, voffA[0][i],
                                   voffA[1][i]);
            }
        }
        const int r = 16 * wave + (lane >> 2);
        const int c = (lane & 3) ^ ((r >> 2) & 3);
        const int rb0 = r < b_last ? r : b_last, rb1 = HP + r < b_last ? HP + r : b_last;
        voffB[0] = (unsigned)((size_t)rb0 * Kb + 16 * c);                // < 256 * 16384
        voffB[1] = (unsigned)((size_t)rb1 * Kb + 16 * c);
        const int col = wave_n * 64 + lane;
        voffS = (unsigned)((size_t)(col < b_last ? col : b_last) * G * 4);   // < 256 * 256 * 4
        *(uint4*)&sOff[tid * 8] = make_uint4(voffA[0][0], voffA[0][1], voffS, 0u);
        *(uint4*)&sOff[tid * 8 + 4] = make_uint4(voffA[1][0], voffA[1][1], voffB[0], voffB[1]);
    }
    // 32 tid, opaque: the loop addresses sOff with it, and what the fold, the scale reads and the epilogue need of the
    // lane (lane & 31 = (oa >> 5) & 31, lane >> 5 = (oa >> 10) & 1) is re-derived from a fresh opaque copy where it is
    // used, two VALU instructions, instead of living in registers of its own through every phase
    int oa = tid * 32;
    asm volatile("" : "+v"(oa));
    auto lane_bits = [&]() {
        int o = oa;
        asm volatile("" : "+v"(o));
        return o;
    };
    const unsigned* my_off = (const unsigned*)(lds + oa);
    const unsigned ring_lds = (unsigned)(size_t)(QT_LDS char*)ring;
    const unsigned sc_lds = (unsigned)(size_t)(QT_LDS char*)sc;
    const unsigned dstA_wave = __builtin_amdgcn_readfirstlane(ring_lds + wave * 2048);  // wave-uniform
    const unsigned dstB_wave = __builtin_amdgcn_readfirstlane(ring_lds + wave * 1024);
    const unsigned dstS_wave = __builtin_amdgcn_readfirstlane(sc_lds + wave * 256);
    const int8_t* srcA = p.Xq + m0 * (int64_t)K;      // scalar: k-byte 0 of the tile's first row
    if constexpr (MOE) {
        if (g.row_idx) srcA = p.Xq;
    }
    const int8_t* srcB = p.Wq + w_row0 * Kb;
    // waves 0-3: s_w, waves 4-7: wsum (symmetric: s_w again, never read)
    const char* srcS = ((ASYM && group_b) ? (const char*)p.wsum : (const char*)p.s_w) + (size_t)w_row0 * G * 4;
    // unit i = 4 t + J: J is a compile-time constant wherever the slot is
    auto off_of = [&](auto j_c) -> uint4 {            // read ahead of the phase's fragment reads
        constexpr int J = decltype(j_c)::value;
        if constexpr (J == 0) return *(const uint4*)my_off;
        else if constexpr (J == 3) return make_uint4(my_off[4], my_off[5], 0u, 0u);
        else return make_uint4(my_off[5 + J], 0u, 0u, 0u);
    };
    auto issue = [&](auto j_c, int t, int slot, const uint4 v) {
        constexpr int J = decltype(j_c)::value;
        const unsigned off = (unsigned)slot * UNIT_BYTES;
        if constexpr (J == 0 || J == 3) {
            const unsigned d = dstA_wave + off;
            glds16_pair(v.x, v.y, srcA + (size_t)t * KU, d, d + 1024);
            if constexpr (J == 0) glds4_one(v.z, srcS + (size_t)t * 4, dstS_wave + (unsigned)(slot >> 2) * SC_BYTES);
        } else {
            glds16_one(v.x, srcB + (size_t)t * (KU / 2), dstB_wave + off);
        }
    };
    auto issue_now = [&](auto j_c, int t, int slot) { issue(j_c, t, slot, off_of(j_c)); };

    // ---- fragment read geometry (per lane), byte offsets inside a unit ----
    const int lr = lane & 31, lh = lane >> 5;
    // A: row r + 32 (mi = 1) is 4 pieces further with the same swizzle; B: chunk 2 lh + 1 is chunk 2 lh with bit 0 flipped
    int aoff[4], boff;
    {
        const int r = wave_m * 64 + lr;               // row of the half panel, mi = 0
#pragma unroll
        for (int s = 0; s < 4; ++s)                   // k-step s: chunk 4 lh + s
            aoff[s] = (r >> 3) * 1024 + (r & 7) * 128 + 16 * ((4 * lh + s) ^ ((r >> 1) & 7));
    }
    {
        const int r = wave_n * 32 + lr;               // packed chunk 2 lh + j: k-steps 2 j, 2 j + 1
        boff = (r >> 4) * 1024 + (r & 15) * 64 + 16 * ((2 * lh) ^ ((r >> 2) & 3));
    }

    f32x16 tot[2][2][2];                              // [A half][B half][mi]
#pragma unroll
    for (int qa = 0; qa < 2; ++qa)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) tot[qa][qb][mi] = (f32x16){};
    i32x16 acc[2] = {(i32x16){}, (i32x16){}};         // the phase's acc_g, [mi]
    float sw[2] = {0.0f, 0.0f};                       // s_w[n, g], wsum[n, g] of the K-tile being folded, [B half]
    int ws[2] = {0, 0};

    // tot += s_w[n, g] * (float)(acc_g - zp_x[m] * wsum[n, g]) for the quadrant of phase q (gemm_i8_kernel's GROUPED
    // branch).  Before phase 0 it runs on acc = 0, s_w = 0: tot stays +0.
    auto fold = [&](auto q_c) {
        constexpr int Q = decltype(q_c)::value, QA = Q >> 1, QB = Q & 1;
        const int lh4 = ASYM ? (lane_bits() >> 8) & 4 : 0;    // 4 (lane >> 5)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {             // rows 8 k + 4 lh + 0..3 of the 32 x 32 tile: one ds_read_b128
                i32x4 z = {};
                if (ASYM) z = *(const i32x4*)&sZp[QA * HP + wave_m * 64 + mi * 32 + 8 * k + lh4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * k + j;
                    int a = acc[mi][r];
                    if (ASYM) a = a - __mul24(z[j], ws[QB]);
                    const float t = (float)a;
                    const float prod = sw[QB] * t;
                    tot[QA][QB][mi][r] = tot[QA][QB][mi][r] + prod;
                }
            }
            // the sums are complete here: hipcc may not carry the products on and add them phases later
            asm volatile("" : "+v"(tot[QA][QB][mi]));
        }
    };

    // ---- the pipeline (ring_pipe.h): R 8, L 6 ----
    i32x4 fa[2][4], pb[2][2];                         // A: [mi][k-step]; packed B: [half][chunk]
    auto drain_wait = [&](int u) {                    // the head comment's ladder
        const int later = nu - u - 3;
        if (later == 3) wait_vmcnt<4>();
        else if (later == 2) wait_vmcnt<3>();
        else if (later == 1) wait_vmcnt<2>();
        else wait_vmcnt<0>();
    };
    auto phase = [&](auto slot_c, auto steady_c, int u) {
        constexpr int S = decltype(slot_c)::value;
        constexpr bool STEADY = decltype(steady_c)::value;
        constexpr int Q = S & 3, QB = Q & 1;
        constexpr int ISLOT = (S + LEAD) & (RING - 1);
        // ---- LOAD: the K-tile's units sit in slots (S & 4) + {0: A0, 1: B0, 2: B1, 3: A1} ----
        // an opaque base per operand: hipcc would otherwise keep one address register per (slot, k-step) for the slots
        // beyond the DS offset field's 64 KiB, hoisted out of the loop
        auto tile_base = [&](int unit) {
            int o = ((S & 4) + unit) * UNIT_BYTES;
            asm volatile("" : "+v"(o));
            return (const char*)ring + o;
        };
        const uint4 voff = off_of(std::integral_constant<int, (S + LEAD) & 3>{});
        if constexpr (Q == 0 || Q == 2) {
            const char* base = tile_base(Q == 0 ? 0 : 3);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) fa[mi][s] = *(const i32x4*)(base + aoff[s] + mi * 4096);
        }
        if constexpr (Q == 0 || Q == 1) {
            const char* base = tile_base(1 + QB);
#pragma unroll
            for (int j = 0; j < 2; ++j) pb[QB][j] = *(const i32x4*)(base + (boff ^ (16 * j)));
        }
        if (STEADY || u + LEAD < nu) {
            issue(std::integral_constant<int, (S + LEAD) & 3>{}, (u + LEAD) >> 2, ISLOT, voff);
            wait_vmcnt<7>();                // everything up to unit u+2 has landed; 4 units stay in flight
        } else {
            drain_wait(u);
        }
        fold(std::integral_constant<int, (Q + 3) & 3>{});   // the previous phase's acc_g
        if constexpr (Q == 0) {             // this K-tile's scales (behind the fold of the last one's)
            const int* s = sc + (S >> 2) * (SC_BYTES / 4) + wave_n * 32 + ((lane_bits() >> 5) & 31);
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                sw[qb] = __int_as_float(s[qb * HP]);
                if (ASYM) ws[qb] = s[256 + qb * HP];
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // the unpack below stays behind the barrier, beside the MFMAs
        // ---- MATH ----
        ring_sync_math([&] {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint2 lo = unpack_int4_word((unsigned)pb[QB][s >> 1][2 * (s & 1)]);
                const uint2 hi = unpack_int4_word((unsigned)pb[QB][s >> 1][2 * (s & 1) + 1]);
                const i32x4 fb = {(int)lo.x, (int)lo.y, (int)hi.x, (int)hi.y};
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    acc[mi] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[mi][s], fb, s == 0 ? (i32x16){} : acc[mi], 0, 0, 0);
            }
        });
    };

    // prologue: units 0..LEAD-1 in flight (nu is 4 or at least 8), units 0 and 1 landed
    issue_now(std::integral_constant<int, 0>{}, 0, 0);
    issue_now(std::integral_constant<int, 1>{}, 0, 1);
    issue_now(std::integral_constant<int, 2>{}, 0, 2);
    issue_now(std::integral_constant<int, 3>{}, 0, 3);
    if (nu > 4) {
        issue_now(std::integral_constant<int, 0>{}, 1, 4);
        issue_now(std::integral_constant<int, 1>{}, 1, 5);
        wait_vmcnt<7>();
    } else {
        wait_vmcnt<3>();
    }
    ring_stagger_begin(group_b);

    int u = 0;
    for (; u + 8 + LEAD <= nu; u += 8)   // every phase issues a unit that exists
        ring_body<8>([&](auto slot_c, int uu) { phase(slot_c, std::true_type{}, uu); }, u);
    for (; u + 8 <= nu; u += 8)
        ring_body<8>([&](auto slot_c, int uu) { phase(slot_c, std::false_type{}, uu); }, u);
    if (u < nu) {  // nu is a multiple of 4: one K-tile left
        phase(std::integral_constant<int, 0>{}, std::false_type{}, u);
        phase(std::integral_constant<int, 1>{}, std::false_type{}, u + 1);
        phase(std::integral_constant<int, 2>{}, std::false_type{}, u + 2);
        phase(std::integral_constant<int, 3>{}, std::false_type{}, u + 3);
    }
    ring_stagger_end(group_b);
    fold(std::integral_constant<int, 3>{});           // the last phase's acc_g

    // ---- epilogue: y = s_x[m] * tot (+ bias[n]), once per output element, by the lane that holds it ----
    // (the grouped form: s_x at the row's source row, from sRow; no bias)
    const int ob = lane_bits();
    const int lr_e = (ob >> 5) & 31, lh_e = (ob >> 10) & 1;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const int n = n0 + qb * HP + wave_n * 32 + lr_e;
        if (n >= p.N) continue;
        float bn = 0.0f;
        const bool has_bias = !MOE && p.bias;
        if (has_bias) bn = qt_load_w(p.bias, p.out_dtype, n);
#pragma unroll
        for (int qa = 0; qa < 2; ++qa) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t m = i8_ring_cd_row(m0 + qa * HP + wave_m * 64 + mi * 32, r, lh_e);
                    if (m >= m_end) continue;
                    int64_t ms = m;
                    if constexpr (MOE) ms = sRow[m - m0];
                    float y = p.s_x[ms] * tot[qa][qb][mi][r];
                    if (has_bias) y = y + bn;
                    qt_store_w(p.Y, p.out_dtype, (size_t)(m * p.ldy + n), y);
                }
            }
        }
    }
}

template <bool ASYM>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_i8_ring_w4_kernel(const RingW4Args p) {
    ring_w4_tile<ASYM, false>(p, RingMoe{});
}
template <bool ASYM>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_i8_ring_w4_moe_kernel(const RingW4Args p, const RingMoe g) {
    ring_w4_tile<ASYM, true>(p, g);
}

}  // namespace

extern "C" int qt_gemm_i8_ring_w4(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N,
                                  const float* s_x, const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum,
                                  const void* bias, void* Y, int out_dtype, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(w_format == QT_W_INT4_PACKED, "qt_gemm_i8_ring_w4: w_format %d unsupported: packed int4 weights only "
                 "(int8 weights run on qt_gemm_i8_ring)", w_format);
    QT_CHECK_ARG(K % QT_I8_RING_W4_K_UNIT == 0, "qt_gemm_i8_ring_w4: K %d is not a multiple of the k-unit %d", K,
                 QT_I8_RING_W4_K_UNIT);
    QT_CHECK_ARG(G == K / QT_I8_RING_W4_K_UNIT, "qt_gemm_i8_ring_w4: G %d unsupported: one scale per group of %d "
                 "columns only, G = K / %d = %d (channel-wise scales run on qt_gemm_i8)", G, QT_I8_RING_W4_K_UNIT,
                 QT_I8_RING_W4_K_UNIT, K / QT_I8_RING_W4_K_UNIT);
    if (int st = qt_i8_check_dense("qt_gemm_i8_ring_w4", Xq, M, K, Wq, w_format, N, s_x, zp_x, s_w, G, wsum, Y, out_dtype,
                                   ldy, true))
        return st;
    static_assert(QT_I8_RING_W4_K_UNIT == KU && QT_I8_RING_W4_SLOTS == RING && QT_I8_RING_W4_LEAD == LEAD,
                  "header constants");
    const int64_t tiles = ((M + BT - 1) / BT) * (int64_t)((N + BT - 1) / BT);
    QT_CHECK_ARG(tiles <= 0x7fffffffLL, "qt_gemm_i8_ring_w4: too many tiles");
    RingW4Args a{Xq, (const int8_t*)Wq, s_x, zp_x, s_w, wsum, bias, Y, M, N, K, G, ldy, out_dtype};
    if (zp_x) hipLaunchKernelGGL(gemm_i8_ring_w4_kernel<true>, dim3((unsigned)tiles), dim3(NTHREADS), 0, stream, a);
    else hipLaunchKernelGGL(gemm_i8_ring_w4_kernel<false>, dim3((unsigned)tiles), dim3(NTHREADS), 0, stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

// The grouped form.  Its name joins the qt_moe_* family, not qt_gemm_i8*: the set of qt_gemm_i8* entry points is the
// table ops.I8_FORMS (hip/ops.py), which holds this form's row beside it (I8_MOE_RING_W4_FORM) until it moves in.
extern "C" int qt_moe_gemm_i8_ring_w4(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R,
                                      const int32_t* offsets, int E, const void* Wq, int w_format, int N,
                                      const float* s_x, const int32_t* zp_x, const float* s_w, int G,
                                      const int32_t* wsum, void* Y, int out_dtype, int64_t ldy, int64_t x_rows,
                                      qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(x_rows > 0, "qt_moe_gemm_i8_ring_w4: bad arguments");
    QT_CHECK_ARG(w_format == QT_W_INT4_PACKED, "qt_moe_gemm_i8_ring_w4: w_format %d unsupported: packed int4 weights "
                 "only (int8 weights run on qt_gemm_i8_ring_grouped)", w_format);
    QT_CHECK_ARG(K % QT_I8_RING_W4_K_UNIT == 0, "qt_moe_gemm_i8_ring_w4: K %d is not a multiple of the k-unit %d", K,
                 QT_I8_RING_W4_K_UNIT);
    QT_CHECK_ARG(G == K / QT_I8_RING_W4_K_UNIT, "qt_moe_gemm_i8_ring_w4: G %d unsupported: one scale per group of %d "
                 "columns only, G = K / %d = %d (channel-wise scales run on qt_gemm_i8_grouped)", G, QT_I8_RING_W4_K_UNIT,
                 QT_I8_RING_W4_K_UNIT, K / QT_I8_RING_W4_K_UNIT);
    QT_CHECK_ARG(R <= 0x7fffffffLL, "qt_moe_gemm_i8_ring_w4: R %lld too large", (long long)R);
    QT_CHECK_ARG(E <= 4096, "qt_moe_gemm_i8_ring_w4: E %d > 4096", E);
    if (int st = qt_i8_check_grouped("qt_moe_gemm_i8_ring_w4", Xq, K, R, offsets, E, Wq, w_format, N, s_x, zp_x, s_w, G,
                                     wsum, Y, out_dtype, ldy, true))
        return st;
    // gathered rows are addressed by a 32-bit byte offset from Xq; contiguous rows need R of them
    QT_CHECK_ARG(!row_idx || x_rows * (int64_t)K <= (1LL << 32), "qt_moe_gemm_i8_ring_w4: x_rows %lld x K %d > 2^32 "
                 "bytes: a gathered row is addressed by a 32-bit offset", (long long)x_rows, K);
    QT_CHECK_ARG(row_idx || x_rows >= R, "qt_moe_gemm_i8_ring_w4: x_rows %lld < R %lld without row_idx",
                 (long long)x_rows, (long long)R);
    const int64_t tiles = ((R + BT - 1) / BT + E) * (int64_t)((N + BT - 1) / BT);
    QT_CHECK_ARG(tiles <= 0x7fffffffLL, "qt_moe_gemm_i8_ring_w4: too many tiles");
    RingW4Args a{Xq, (const int8_t*)Wq, s_x, zp_x, s_w, wsum, nullptr, Y, R, N, K, G, ldy, out_dtype};
    RingMoe g{offsets, row_idx, x_rows, E};
    if (zp_x) hipLaunchKernelGGL(gemm_i8_ring_w4_moe_kernel<true>, dim3((unsigned)tiles), dim3(NTHREADS), 0, stream, a, g);
    else hipLaunchKernelGGL(gemm_i8_ring_w4_moe_kernel<false>, dim3((unsigned)tiles), dim3(NTHREADS), 0, stream, a, g);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
