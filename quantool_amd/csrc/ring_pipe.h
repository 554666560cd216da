// The LDS-ring MFMA pipeline of xtx_kernel, xtx16_kernel (xtx.hip) and gemm3_kernel (gemm3_tn.hip), stated once:
// the shared constants, LDS-DMA issue from inline asm, transposing fragment reads, the 16-bit MFMA k-step and tile
// loop, counted vmcnt waits with their drain ladder, the phase tail, the two-group stagger and the unrolled body.
// sgemm_ring_kernel (sgemm_tn.hip) runs a different ring (one barrier per pair of stages, no stagger) and takes
// only the LDS-DMA and vmcnt leaves from here.
// An edit here edits three hand-scheduled kernels: tools/isa_compare.py says, without a GPU, whether one meant to be
// neutral was (profiles/ring_pipe_isa_parent_vs_refactor.txt lists the pieces that could not move here and why).
//
// THE PIPELINE.  A workgroup of 8 waves owns one 256x256 output tile and streams "units" of the reduction
// dimension through a ring of R LDS slots.  Unit u lives in slot u % R and is consumed in phase u; the LDS-DMA of
// unit u+L (the lead) is issued in phase u, N instructions per wave:
//   phase u = { LOAD(u): transposing reads of unit u ; issue unit u+L ; counted vmcnt(N*(L-1)) ; s_barrier ;
//               MATH(u): lgkmcnt(0) ; setprio 1 ; MFMAs ; setprio 0 ; s_barrier }
// Waves 4-7 (group B) run the same program one barrier behind waves 0-3 (group A), so on every SIMD one wave's LDS
// reads / DMA issue run under its partner's MFMAs (ping-pong).
//
// HAZARDS.  Intervals between consecutive workgroup barriers are numbered; group A runs LOAD(u) in interval 2u and
// MATH(u) in 2u+1, group B one interval later.
//   RAW: unit u is read in intervals 2u (A) / 2u+1 (B).  The counted wait of LOAD(u-1) leaves only the L-1 units
//        u+1 .. u+L-1 of the wave's own DMA outstanding, so every wave has retired its part of unit u in intervals
//        2u-2 / 2u-1, and the barrier that ends interval 2u-1 follows both: "read one phase after the wait that
//        retires it".
//   WAR: unit u's reads retire at the lgkmcnt(0) that opens MATH(u): intervals 2u+1 (A) / 2u+2 (B).  Its slot is
//        re-filled with unit u+R, issued in LOAD(u+R-L): intervals 2(u+R-L) / 2(u+R-L)+1.  With L <= R-2 that is
//        2u+4 / 2u+5 at the earliest, after the barriers that end 2u+2 and 2u+3.  (L = R-1 would put group A's
//        issue into 2u+2, beside group B's outstanding reads.)
//   In flight at every wait: L-1 units = N*(L-1) LDS-DMA instructions per wave; never vmcnt(0) inside the loop.
//   Past the last unit nothing is issued, and the drain ladder lowers the count with the units that still exist.
// MID-LOOP FLUSH (the CHAIN forms of xtx_kernel / xtx16_kernel).  Between phase u-1 and phase u, where u is a multiple
// of the ring (slot numbers stay immediates), a wave may run plain global loads and stores of its own -- the epilogue's
// read-modify-write of G or of its slab -- provided it ends them with vmcnt(0).  Nothing above is disturbed:
//   - the flush holds no barrier, so the intervals keep their numbers and both groups their barrier counts; it only
//     lengthens the interval it stands in (2u for group A, 2u+1 for group B).  WAR is an argument about interval
//     numbers alone (issue in LOAD, reads retired at the lgkmcnt(0) of MATH) and the flush issues no LDS-DMA.
//   - RAW: unit u was retired by the counted wait of LOAD(u-1), in front of the barriers of phase u-1, as always.  The
//     compiler's own vmcnt waits inside the flush count only the flush's loads; the counter is in order, so they wait
//     for the older LDS-DMA too -- MORE than the ring needs, which is safe: the hazard argument is about minimum waits.
//   - the counted wait of LOAD(u) assumes that the N*(L-1) youngest outstanding operations are the ring's.  Stores of
//     the flush still in flight would be counted in their place (stores and loads share vmcnt on gfx9 and need not
//     retire in order against each other), hence the closing vmcnt(0): behind it nothing is outstanding, units
//     u+1 .. u+L-1 have landed early, and the following waits are satisfied sooner than they ask.
//   The cost is one short bubble per flush: the L-1 units in flight are waited for at once, with no MFMA under them.
// The instances:
//   xtx_kernel    R 8, L 6, unit = 16 tokens (16 KiB),             N 2: vmcnt(10), 5 units = 80 KiB per CU in flight
//   xtx16_kernel  R 5, L 3, unit = a pair of those ("double", 32 KiB), N 4: vmcnt(8), 2 doubles = 64 KiB in flight
//   gemm3_kernel  (chunk loop, QT_G3_LOOP=chunk)  R 8, L 6, unit = 16 k-rows of one plane pair (16 KiB), N 2:
//                 vmcnt(10), 5 units = 80 KiB in flight
//   gemm3_kernel  R 3, unit = 16 k-rows of all three planes of both operands ("tri-unit", 48 KiB), N 6: vmcnt(6), one
//                 tri-unit = 48 KiB in flight -- the half-phase form below
//   gemm3_kernel, f16x2  R 4, L 2, unit = 16 k-rows of the two fp16 planes of both operands ("duo-unit", 32 KiB), N 4:
//                 vmcnt(4), one duo-unit = 32 KiB in flight.  Four 32 KiB slots fit where three 48 KiB ones do, so L = 2
//                 = R-2 is the plain scheme above, both groups alike, no half-phase hooks.  RAW: unit u is retired by the
//                 vmcnt(4) of LOAD(u-1) (only u+1 stays outstanding), intervals 2u-2 / 2u-1, and first read in 2u.
//                 WAR: unit u's reads retire in 2u+1 (A) / 2u+2 (B); its slot takes unit u+4, issued in LOAD(u+2):
//                 intervals 2u+4 / 2u+5.  Prologue: units 0, 1 issued, vmcnt(4) retires unit 0.  Drain: nothing is
//                 issued from phase nu-2 on, whose wait is vmcnt(0) (ring_drain_wait<4, 2>); nu is a multiple of 4.
//
// R = 3, HALF-PHASE ISSUE (gemm3_kernel).  Three 48 KiB tri-units are all the LDS holds, and the scheme above then
// allows L = 1 only: its wait would be vmcnt(0) right behind the issue, with nothing in flight under the MFMAs.  What
// forbids L = 2 = R-1 is group A alone (its issue in LOAD(u), interval 2u, beside group B's reads of unit u-1 that
// retire in 2u), so this instance leads by two units and moves group A's issue and wait half a phase down
// (ring_sync_math's pre / post hooks); group B keeps them in LOAD.  Phase u:
//   group A: LOAD(u) = { reads of unit u } ; MATH(u) = { lgkmcnt(0) ; issue unit u+2 ; MFMAs ; vmcnt(6) }
//   group B: LOAD(u) = { issue unit u+2 ; reads of unit u ; vmcnt(6) } ; MATH(u) = { lgkmcnt(0) ; MFMAs }
//   Unit v is issued by A in MATH(v-2) and by B in LOAD(v-2): both interval 2v-3; it is retired by A at the end of
//   MATH(v-1) and by B at the end of LOAD(v-1): both interval 2v-1, the wait a vmcnt(6) because unit v+1 (6 DMA
//   instructions per wave) was issued earlier in that interval and stays in flight.
//   WAR: the slot's previous unit v-3 had its reads retired at the lgkmcnt(0) of MATH(v-3): intervals 2v-5 (A) /
//        2v-4 (B); the issue in 2v-3 follows the barrier that ends 2v-4, and A's also follows its own barrier + wait.
//   RAW: unit v is first read in interval 2v (A), after the barrier that ends 2v-1, where every wave has retired it.
//   Prologue: units 0 and 1 are issued, vmcnt(6) retires unit 0 in front of the stagger's first barrier; unit 1 is
//   retired in interval 1 by the waits of phase 0.  Drain: nothing is issued from phase nu-2 on, whose wait is
//   vmcnt(0) (ring_drain_wait<6, 2>).  A tri-unit has three barrier intervals (about three MATH lengths) to land.
//
// LDS-DMA from inline asm: hipcc does not track it, so it inserts no vmcnt drain in front of later
// ds_reads or barriers.  Every completion is ordered by hand (counted vmcnt + s_barrier, as above).
// saddr form: 64-bit scalar base + 32-bit per-lane byte offset; M0 = wave-uniform LDS destination.
// M0 is written in the statement that reads it and is not restored: nothing else in these kernels uses
// M0 (LDS instructions need none on gfx9+), which the build checks by grepping each translation unit's
// ISA for m0 outside the asm blocks (csrc/build.py:audit_m0).
#pragma once
#include <type_traits>

#include "common.h"

constexpr int BT = 256;                       // output tile edge
constexpr int UT = 16;                        // reduction rows (tokens / k-rows) per 16 KiB unit = one 32x32x16 MFMA k-step
constexpr int UNIT_BYTES = UT * 2 * BT * 2;   // A + B panels, 16 KiB; image: [A-lo, A-hi, B-lo, B-hi][16 rows][256 B]
constexpr int NTHREADS = 512;                 // 8 waves: 2 (M) x 4 (N), 128x64 outputs per wave
constexpr int NUM_CU = 256;

// Both LDS-DMA instructions of one unit (A panel, B panel) in one statement; one source matrix.
__device__ __forceinline__ void glds16_pair(unsigned voffA, unsigned voffB, const void* sbase, unsigned ldsA,
                                            unsigned ldsB) {
    asm volatile(
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %2\n\t"
        "s_mov_b32 m0, %4\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2"
        :
        : "v"(voffA), "v"(voffB), "s"(sbase), "s"(ldsA), "s"(ldsB)
        : "memory");
}
// The same with one scalar base per panel (A and B panels come from different matrices / planes).
__device__ __forceinline__ void glds16_pair2(unsigned voffA, unsigned voffB, const void* sbaseA, const void* sbaseB,
                                             unsigned ldsA, unsigned ldsB) {
    asm volatile(
        "s_mov_b32 m0, %4\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %2\n\t"
        "s_mov_b32 m0, %5\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %3"
        :
        : "v"(voffA), "v"(voffB), "s"(sbaseA), "s"(sbaseB), "s"(ldsA), "s"(ldsB)
        : "memory");
}
// One panel (sgemm_ring_kernel: its A and B panels are issued separately).
__device__ __forceinline__ void glds16_one(unsigned voff, const void* sbase, unsigned lds_dst) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}
// One dword per lane (64 x 4 B = 256 B of LDS per wave-instruction): a gather of strided scalars, e.g. one column of a
// row-major scale table (gemm_i8_ring_w4_kernel).  Counted in vmcnt like every other LDS-DMA.
__device__ __forceinline__ void glds4_one(unsigned voff, const void* sbase, unsigned lds_dst) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}
__device__ __forceinline__ void glds16_snapshot(unsigned voff, const void* sbase, unsigned lds_dst) {
    // 1 KiB of progress words -> LDS scratch; sc1: served by L2, never by this CU's L1 copy of the line
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1 sc1"
        :
        : "v"(voff), "s"(sbase), "s"(lds_dst)
        : "memory");
}

__device__ __forceinline__ s16x8 tr_load8(const char* lds_addr) {
    // two transposing reads: k rows +0..3 and +4..7 (rows are 256 B apart -> +1024 B)
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((QT_LDS s16x4*)(lds_addr));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((QT_LDS s16x4*)(lds_addr + 1024));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// one k-step (16 rows) of a 32x32 output tile; bf16 and fp16 products are both exact in the fp32
// accumulator and run at the same MFMA rate
template <bool F16>
__device__ __forceinline__ f32x16 mfma16(s16x8 a, s16x8 b, f32x16 c) {
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// one k-step (32 rows) of a 16x16 output tile
template <bool F16>
__device__ __forceinline__ f32x4 mfma32(s16x8 a, s16x8 b, f32x4 c) {
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// the MFMAs of one phase on 32x32 tiles: MI x 2 accumulators per wave (MI = 4; 2 only in a lab build of xtx_kernel)
template <bool F16, int MI = 4>
__device__ __forceinline__ void ring_mma32(const s16x8 (&fa)[4], const s16x8 (&fb)[2], f32x16 (&acc)[4][2]) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma16<F16>(fa[mi], fb[ni], acc[mi][ni]);
}
// ... and on 16x16 tiles: 8 x 4 accumulators per wave
template <bool F16>
__device__ __forceinline__ void ring_mma16(const s16x8 (&fa)[8], const s16x8 (&fb)[4], f32x4 (&acc)[8][4]) {
#pragma unroll
    for (int ai = 0; ai < 8; ++ai)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj) acc[ai][bj] = mfma32<F16>(fa[ai], fb[bj], acc[ai][bj]);
}

// The counted wait of a phase that has nothing left to issue: `later` units after u+1 exist (later = nu - u - 2),
// and exactly those may stay in flight.  N DMA instructions per unit and wave, lead L:
// N 2, L 6 -> vmcnt 10/8/6/4/2/0;  N 4, L 3 -> 8/4/0;  N 6, L 2 (the half-phase form) -> 6/0.
template <int N, int K>
__device__ __forceinline__ void ring_drain_step(int later) {
    if constexpr (K == 0) wait_vmcnt<0>();
    else if (later == K) wait_vmcnt<N * K>();
    else ring_drain_step<N, K - 1>(later);
}
template <int N, int L>
__device__ __forceinline__ void ring_drain_wait(int later) {
    if (later >= L - 1) wait_vmcnt<N * (L - 1)>();
    else ring_drain_step<N, L - 2>(later);
}

// The tail of a phase, behind the reads, the issue and the counted wait: MATH between two workgroup barriers.  The
// sched_barriers pin the order hipcc may not change: nothing moves across a barrier, the fragment reads are waited
// for only behind the first barrier, and the MFMAs run at raised priority.
template <class Math>
__device__ __forceinline__ void ring_sync_math(Math&& math) {
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    math();
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// The same with a hook behind the opening barrier and the lgkmcnt(0) (pre: e.g. an LDS-DMA issue into a slot whose last
// readers that barrier has just passed) and one in front of the closing barrier (post: a counted vmcnt).
template <class Pre, class Math, class Post>
__device__ __forceinline__ void ring_sync_math(Pre&& pre, Math&& math, Post&& post) {
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    pre();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    math();
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    post();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// The two-group stagger.  Begin (behind the prologue's wait for unit 0): one barrier for everyone, one more for
// group B, which from here on runs one interval behind.  End: group A's barrier that pairs with group B's last.
__device__ __forceinline__ void ring_stagger_begin(bool group_b) {
    __builtin_amdgcn_s_barrier();
    if (group_b) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void ring_stagger_end(bool group_b) {
    if (!group_b) __builtin_amdgcn_s_barrier();
    wait_vmcnt<0>();
}

// One trip round a ring of SLOTS slots: phase(slot as an integral_constant, unit index), so that every LDS address
// of a phase is an immediate.  8: xtx_kernel / gemm3_kernel's chunk loop, 5: xtx16_kernel, 4: gemm3_kernel on two fp16
// planes, 3: gemm3_kernel.
template <int SLOTS, class Phase>
__device__ __forceinline__ void ring_body(Phase&& phase, int u) {
    static_assert(SLOTS == 3 || SLOTS == 4 || SLOTS == 5 || SLOTS == 8, "unrolled by hand");
    phase(std::integral_constant<int, 0>{}, u);
    phase(std::integral_constant<int, 1>{}, u + 1);
    phase(std::integral_constant<int, 2>{}, u + 2);
    if constexpr (SLOTS >= 4) phase(std::integral_constant<int, 3>{}, u + 3);
    if constexpr (SLOTS >= 5) phase(std::integral_constant<int, 4>{}, u + 4);
    if constexpr (SLOTS == 8) {
        phase(std::integral_constant<int, 5>{}, u + 5);
        phase(std::integral_constant<int, 6>{}, u + 6);
        phase(std::integral_constant<int, 7>{}, u + 7);
    }
}
