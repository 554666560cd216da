// a11: the GPTQ column sweep (upstream quantize_weight's block loop,
// reached through gptq.py:86 / base.py:161).
//
// Rows of W are independent given U, so one lane owns one row.  Per 128-column block:
//   sweep_block_kernel : the 128 sequential quantise / error-feedback steps.  The U block and
//                        the lane's 128 weights live in LDS; the active 32-column sub-block
//                        lives in registers (statically indexed), the other columns receive
//                        rank-32 updates with float4 broadcasts of U.  Per element the update
//                        sequence is exactly upstream's: ascending source column, each step
//                        "w = w - (err * u)" with two roundings (no contraction).
//   sgemm_tn (SUB)     : W[:, i2:] -= Err1 @ U[i1:i2, i2:] as an ascending-k fmaf chain from 0
//                        on the f32 MFMA, then one subtraction -- the oracle's fixed order.
// Up to 6144 rows, on whole 128-tiles, a batch of blocks runs as ONE launch instead (sweep_fused_kernel below): its
// block steps and near updates per group of rows, beside the far update of the batch before it.
// Bit-exact against oracle/gptq_oracle.c:orc_gptq_sweep.
//
// Three kernel forms run the 128 steps of a block, and the contract is stated once for all of them:
//   sweep_block_kernel (QT_SWEEP_BLOCK=row)  one lane per row            quantise_weight + its own update loops
//   sweep_quad_kernel  (chain of launches)   4 lanes per row             col_step<QuadLayout, ...>
//   sweep_fused_kernel<16 | 8>               16 or 8 lanes per row       col_step<TriLayout<NL>, ...>
// quantise_weight is the fp32 op sequence of one weight; col_step is the whole column step of the multi-lane forms
// (read-ahead of U, quantise, broadcast of the owner's error, update of the lane's later columns), which differ only
// in their broadcast (row_bcast) and in where a lane finds its U values in LDS (the two layout traits).  The host
// side is sweep_run: the checks and the choice between sweep_run_fused and sweep_run_chain.
#include <stdlib.h>

#include <map>
#include <tuple>
#include <vector>

#include "common.h"
#include "gemm3_tn.h"
#include "sgemm_ring.h"
#include "sgemm_tn.h"

#pragma clang fp contract(off)

namespace {

constexpr int BS = 128;    // upstream block_size default
constexpr int SWEEP_MAX_BATCH = 8;  // blocks whose far update may be merged into one pass over W (workspace is sized for it)
constexpr int SB = 32;     // register sub-block
constexpr int ROWS = 128;  // rows (lanes) per workgroup: 2 waves
constexpr size_t SWEEP_LDS = (size_t)(BS * BS + BS * ROWS + 2 * BS) * sizeof(float);

// Row groups of a stacked sweep (qt_gptq_sweep_grouped): rows [row_end[g-1], row_end[g]) belong to problem g, whose factor
// is U + g * bsU and whose column groups are g_idx + g * K.  n == 0: one problem.
struct SweepGroups {
    int n;
    int64_t bsU;
    int row_end[SG_MAX_GROUPS];
};
__device__ __forceinline__ int sweep_group_of(const SweepGroups& sg, int row0) {
    int g = 0;
    while (g + 1 < sg.n && row0 >= sg.row_end[g]) ++g;
    return g;
}

// The quantise step of one weight, the only statement of it in this file: upstream's fp32 operations one by one, each
// rounded on its own (no contraction) -- IEEE division (-fhip-fp32-correctly-rounded-divide-sqrt), clamp, round half
// to even (rintf = v_rndne_f32), dequantise, and the error fed back to the later columns, diff / d with d = U[c][c].
struct Quantised {
    float q, dq, diff, e;   // level, dequantised value, w - dq, diff / d
};
__device__ __forceinline__ Quantised quantise_weight(float wv, float sc, float zz, float d, float qmin, float qmax) {
    float x = wv / sc;
    x = x + zz;
    x = fminf(fmaxf(x, qmin), qmax);
    const float q = rintf(x);
    const float dq = (q - zz) * sc;
    const float diff = wv - dq;
    return {q, dq, diff, diff / d};
}

__global__ __launch_bounds__(ROWS) void sweep_block_kernel(float* __restrict__ W, int R, int K,
                                                           const float* __restrict__ U,
                                                           const float* __restrict__ scale_t,
                                                           const float* __restrict__ zp_t,
                                                           const int32_t* __restrict__ g_idx, int i1, int cnt,
                                                           float qmin, float qmax, int8_t* __restrict__ Qt,
                                                           float* __restrict__ ErrT, float* __restrict__ loss,
                                                           int prio, SweepGroups sg) {
    qt_set_chain_prio(prio);
    if (sg.n > 1) {
        const int g = sweep_group_of(sg, blockIdx.x * ROWS);
        U += (size_t)g * sg.bsU;
        g_idx += (size_t)g * K;
    }
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Un = sm;                  // [BS][BS]   Un[i][j] = U[i1+i][i1+j], zero outside j>=i / cnt
    float* wl = sm + BS * BS;        // [BS cols][ROWS]
    float* dd = wl + BS * ROWS;      // [BS] diag, [BS] diag^2
    const int tid = threadIdx.x;
    const int row = blockIdx.x * ROWS + tid;
    const bool valid = row < R;
    const int rowc = valid ? row : R - 1;

    // Prologue loads are issued in batches of 16 independent float4 loads per thread and only then
    // written to LDS: a load -> wait -> store loop costs one memory round trip per iteration (32 + 128
    // of them used to be half of this kernel's time).  Out-of-block elements of a ragged last block are
    // read from a clamped in-block address and replaced by the inert value afterwards (cnt % 4 == 0
    // because K % 4 == 0, so a float4 is either wholly inside or wholly outside).
    {
        const float* ublk = U + (size_t)i1 * K + i1;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int e4 = tid + ROWS * (half * 16 + r);      // float4 index in the 128 x 32 grid
                const int i = e4 >> 5, j = (e4 & 31) * 4;
                const int ic = i < cnt ? i : cnt - 1, jc = j < cnt ? j : cnt - 4;
                v[r] = *(const f32x4*)(ublk + (size_t)ic * K + jc);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int e4 = tid + ROWS * (half * 16 + r);
                const int i = e4 >> 5, j = (e4 & 31) * 4;
                const bool inside = i < cnt && j < cnt;
#pragma unroll
                for (int q = 0; q < 4; ++q) Un[i * BS + j + q] = (inside && j + q >= i) ? v[r][q] : 0.0f;
            }
        }
    }
    {
        const float d = (tid < cnt) ? U[(size_t)(i1 + tid) * K + (i1 + tid)] : 1.0f;
        dd[tid] = d;
        dd[BS + tid] = 1.0f / (d * d);   // only the loss uses it (tolerance 1e-6, not part of the bit-exact contract)
    }
    {
        const float* wrow = W + (size_t)rowc * K + i1;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = (half * 16 + r) * 4;
                v[r] = *(const f32x4*)(wrow + (c < cnt ? c : cnt - 4));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = (half * 16 + r) * 4;
#pragma unroll
                for (int q = 0; q < 4; ++q) wl[(c + q) * ROWS + tid] = (c < cnt) ? v[r][q] : 0.0f;
            }
        }
    }
    __syncthreads();

    float blk_loss = 0.0f;
    for (int sb = 0; sb < BS / SB; ++sb) {
        const int cb = sb * SB;
        if (cb >= cnt) break;
        float w[SB], er[SB], sc[SB], zz[SB];
#pragma unroll
        for (int t = 0; t < SB; ++t) w[t] = wl[(cb + t) * ROWS + tid];
#pragma unroll
        for (int t = 0; t < SB; ++t) {
            const int c = cb + t;
            const int g = (c < cnt) ? g_idx[i1 + c] : g_idx[i1];
            sc[t] = scale_t[(size_t)g * R + rowc];
            zz[t] = zp_t[(size_t)g * R + rowc];
        }
#pragma unroll
        for (int t = 0; t < SB; ++t) {
            const int c = cb + t;
            {  // columns >= cnt of a ragged last block run as inert padding (w=0, U=0, d=1)
                const float d = dd[c], rd2 = dd[BS + c];
                const Quantised z = quantise_weight(w[t], sc[t], zz[t], d, qmin, qmax);
                blk_loss = blk_loss + (z.diff * z.diff) * rd2;
                const float e = z.e;
                er[t] = e;
                w[t] = z.dq;
                if (valid && c < cnt) {
                    Qt[(size_t)(i1 + c) * R + row] = (int8_t)z.q;
                    ErrT[(size_t)c * R + row] = e;
                }
                const float* urow = Un + c * BS + cb;
                // two columns per instruction (v_pk_mul_f32 / v_pk_add_f32: the same IEEE single
                // operations, so the roundings are unchanged); an odd first column goes alone
                if ((t + 1) & 1) {
                    const float pr = e * urow[t + 1];
                    w[t + 1] = w[t + 1] - pr;
                }
                const f32x2 e2 = {e, e};
#pragma unroll
                for (int u = (t + 2) & ~1; u < SB; u += 2) {
                    const f32x2 uu = *(const f32x2*)(urow + u);
                    const f32x2 pr = e2 * uu;
                    f32x2 wp = {w[u], w[u + 1]};
                    wp = wp - pr;
                    w[u] = wp[0];
                    w[u + 1] = wp[1];
                }
            }
            // keep each column step's LDS broadcasts next to their use (without this hipcc
            // hoists all 496 U reads of the triangle and spills)
            __builtin_amdgcn_sched_barrier(0);
        }
        // dequantised values of this sub-block back to W (upstream: W[:, i1:i2] = Q1)
        if (valid) {
            float* wrow = W + (size_t)row * K + i1 + cb;
#pragma unroll
            for (int t = 0; t < SB; t += 4) {
                if (cb + t + 3 < cnt) {
                    f32x4 v = {w[t], w[t + 1], w[t + 2], w[t + 3]};
                    *(f32x4*)(wrow + t) = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (cb + t + e < cnt) wrow[t + e] = w[t + e];
                }
            }
        }
        // rank-32 update of the block's remaining columns (ascending source column per element)
        for (int j4 = cb + SB; j4 < cnt; j4 += 4) {
            f32x2 wa = {wl[(j4 + 0) * ROWS + tid], wl[(j4 + 1) * ROWS + tid]};
            f32x2 wb = {wl[(j4 + 2) * ROWS + tid], wl[(j4 + 3) * ROWS + tid]};
#pragma unroll
            for (int t = 0; t < SB; ++t) {
                const f32x4 u = *(const f32x4*)(Un + (cb + t) * BS + j4);
                const f32x2 e2 = {er[t], er[t]};
                const f32x2 ua = {u[0], u[1]}, ub = {u[2], u[3]};
                const f32x2 pa = e2 * ua, pb = e2 * ub;
                wa = wa - pa;
                wb = wb - pb;
            }
            wl[(j4 + 0) * ROWS + tid] = wa[0];
            wl[(j4 + 1) * ROWS + tid] = wa[1];
            wl[(j4 + 2) * ROWS + tid] = wb[0];
            wl[(j4 + 3) * ROWS + tid] = wb[1];
        }
    }
    if (valid) loss[row] = loss[row] + blk_loss / 2.0f;
}

// ---------------------------------------------------------------------------------------------------
// sweep_quad_kernel: the same 128 sequential steps with FOUR LANES PER ROW.
//
// The row-per-lane kernel above is bound by what ONE wave can issue (a lone wave issues a VALU op every 4
// cycles; per column: ~30 dependent ops of the quantise step + 2 ops per later column of the block), and a
// launch has only R / 64 waves (64 waves for R = 4096 on a chip with 1024 SIMDs).  Here lane (r, p),
// p = lane & 3, owns the block's columns 4m + p (m = 0..31) of row r, all 32 in registers: no weight tile
// in LDS, no sub-blocks.  At step c = 4 m0 + p0 every lane of the quad runs the quantise step on its own
// column-m0 register (only the owner's, p == p0, is final and kept), the owner's error is broadcast inside
// the quad by one DPP move, and every lane updates its own later columns -- a quarter of the row's update
// work per lane, four times the waves.  Per ELEMENT the operation sequence is unchanged: ascending source
// column, each step  w = w - (err * u)  with two roundings, IEEE division, round-half-even -- so the
// outputs are bit for bit those of the row-per-lane kernel and of oracle/gptq_oracle.c:orc_gptq_sweep.
// The per-row loss is summed in column order too (every lane of a quad carries the same running sum).
// sweep_fused_kernel (further down) runs the same step with 16 or 8 lanes per row; the step is written once, for
// NL lanes (col_step), right below.
//
// LDS: only the U block (QuadLayout).  73 KiB per workgroup of 64 rows, so two workgroups share a CU
// with room left for a GEMM workgroup.
constexpr int QL = 4;                 // lanes per row
constexpr int QROWS = 64;             // rows per workgroup (128: half as many workgroups holding a CU's LDS, but the
                                      // stage is 9 % slower alone and the bench does not move: 76.7-77.0 vs 76.5-76.9 ms)
constexpr int QTHREADS = QROWS * QL;  // 256
constexpr int QM = BS / QL;           // columns per lane: 32
constexpr int UP_P = QM + 4;          // floats per (c, p) row
constexpr int UP_C = QL * UP_P;       // floats per step c
constexpr size_t QUAD_LDS = (size_t)(BS * UP_C + 2 * BS) * sizeof(float);

// every lane of a row's NL lanes gets lane P0's value: DPP quad_perm [P0, P0, P0, P0] within a quad, row_share within
// 16 lanes; for 8 lanes the two halves of a DPP row take their own source lane (hi: this lane is in the upper half)
template <int NL, int P0>
__device__ __forceinline__ float row_bcast(float v, bool hi) {
    const int x = __builtin_bit_cast(int, v);
    if constexpr (NL == 4) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, P0 * 0x55, 0xF, 0xF, true));
    } else if constexpr (NL == 16) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x150 + P0, 0xF, 0xF, true));
    } else {
        static_assert(NL == 8, "4, 8 or 16 lanes per row");
        const int lo = __builtin_amdgcn_update_dpp(0, x, 0x150 + P0, 0xF, 0xF, true);
        const int up = __builtin_amdgcn_update_dpp(0, x, 0x150 + P0 + 8, 0xF, 0xF, true);
        return __builtin_bit_cast(float, hi ? up : lo);
    }
}

// What lane (r, p) of NL carries through a block: its BS / NL columns NL m + p of row r
template <int NL>
struct StepState {
    static constexpr int NM = BS / NL;
    float w[NM], sc[NM], zz[NM];   // sweep_quad_kernel streams sc / zz: only entries M0 .. M0 + QPF are live at macro-step M0
    float u[2][NM], d[2];          // this lane's U values and the diagonal entry of step C in u[C & 1] / d[C & 1]: read one step ahead
    float lsum, qv, ev, dv;
};

// The U block in LDS.  The two layouts are all that differs between the forms' steps: where lane class p finds the
// row of its values of step C, and at which float4 of that row the group k4 (the lane's columns 4 k4 .. 4 k4 + 3,
// k4 >= band = C / (4 NL): the groups before it are wholly behind the step) lies.
//
// QuadLayout (sweep_quad_kernel): per (step c, lane class p): Up[c][p][m] = U[i1+c][i1+4m+p] for
// 4m+p > c, else 0 (a lane reads its 32 - m0 values of a step as float4s; 36-float rows keep the four
// classes of a quad on disjoint banks).
struct QuadLayout {
    static constexpr int NL = QL;
    template <int C>
    __device__ static __forceinline__ const f32x4* row(const float* __restrict__ Up, int p) {
        return (const f32x4*)(Up + C * UP_C + p * UP_P);
    }
    static constexpr int at(int k4, int /*band*/) { return k4; }
};

// TriLayout (sweep_fused_kernel): the U block's strict upper triangle per (step, float4 group, lane class): step c
// keeps only the groups its lanes still update, 48 KiB (NL = 16) / 40 KiB (NL = 8) instead of 64.
template <int NL>
struct LaneGeo {
    static constexpr int NM = BS / NL;            // columns per lane
    static constexpr int NK4 = NM / 4;            // float4 groups of a lane's columns
    static constexpr int ROWS = 512 / NL;         // rows per workgroup
    static constexpr int BLK = NL * 4;            // floats of one float4 group over the lane classes
    static constexpr int BAND = 4 * NL;           // steps over which the first live group stays the same
    // first float of step c: steps of band q = c / BAND keep groups q .. NK4 - 1
    __host__ __device__ static constexpr int ut_base(int c) {
        const int band = c / BAND, in = c % BAND;
        return BLK * (BAND * (band * NK4 - band * (band - 1) / 2) + in * (NK4 - band));
    }
    static constexpr int UT_FLOATS = ut_base(BS);
    static constexpr int ES_FLOATS = BS * ROWS;
    static constexpr size_t LDS = (size_t)(UT_FLOATS + ES_FLOATS + 2 * BS) * sizeof(float);
};
static_assert(LaneGeo<16>::UT_FLOATS == 12288 && LaneGeo<8>::UT_FLOATS == 10240, "triangle layout");
static_assert(LaneGeo<16>::LDS >= (size_t)RING_LDS_BYTES && LaneGeo<8>::LDS >= (size_t)RING_LDS_BYTES &&
                  LaneGeo<16>::LDS <= 80 * 1024 && LaneGeo<8>::LDS <= 80 * 1024,
              "the launch's LDS holds the ring, and two workgroups fit a CU");
template <int NL_>
struct TriLayout {
    static constexpr int NL = NL_;
    template <int C>
    __device__ static __forceinline__ const f32x4* row(const float* __restrict__ Ut, int p) {
        return (const f32x4*)(Ut + LaneGeo<NL>::ut_base(C) + p * 4);
    }
    static constexpr int at(int k4, int band) { return (k4 - band) * NL; }
};

// this lane's U values of step C (columns NL m + p, m >= C / NL) and U[C][C], from LDS into the registers of parity C & 1
template <class L, int C>
__device__ __forceinline__ void step_fetch(StepState<L::NL>& s, const float* __restrict__ Ub, const float* __restrict__ dd, int p) {
    if constexpr (C < BS) {
        constexpr int band = C / (4 * L::NL);
        const f32x4* urow = L::template row<C>(Ub, p);
#pragma unroll
        for (int k4 = band; k4 < BS / L::NL / 4; ++k4) {
            const f32x4 t = urow[L::at(k4, band)];
            s.u[C & 1][4 * k4 + 0] = t[0]; s.u[C & 1][4 * k4 + 1] = t[1]; s.u[C & 1][4 * k4 + 2] = t[2]; s.u[C & 1][4 * k4 + 3] = t[3];
        }
        s.d[C & 1] = dd[C];
    }
}

// Step C = NL M0 + P0 of a block, in every lane of the row (hi: row_bcast's, unused but for 8 lanes)
template <class L, int M0, int P0>
__device__ __forceinline__ void col_step(StepState<L::NL>& s, const float* __restrict__ Ub, const float* __restrict__ dd,
                                         int p, bool hi, float qmin, float qmax) {
    constexpr int NM = BS / L::NL;
    constexpr int C = L::NL * M0 + P0;
    // The LDS reads of step C + 1 are issued before step C's arithmetic (a lone wave per SIMD has nothing else to cover
    // their latency with; rows beyond a ragged block's last column are zero-filled, so the read ahead is always valid)
#if !defined(QT_SWEEP_LAB) || QT_SWEEP_LAB != 4     // lab build 4: the reads of a step at its own start, as up to round 4
    step_fetch<L, C + 1>(s, Ub, dd, p);
#else                                               // (of sweep_quad_kernel only: the fused kernel has no lab builds)
    step_fetch<L, L::NL == QL ? C : C + 1>(s, Ub, dd, p);
#endif
    const float* u = s.u[C & 1];
    // the quantise step on this lane's own column-M0 value (final only in the owner lane)
    const Quantised z = quantise_weight(s.w[M0], s.sc[M0], s.zz[M0], s.d[C & 1], qmin, qmax);
    const bool own = p == P0;
    s.dv = own ? z.diff : s.dv;
    s.qv = own ? z.q : s.qv;
    s.ev = own ? z.e : s.ev;
    const float eb = row_bcast<L::NL, P0>(z.e, hi);
    // column M0 of the lanes behind the owner; the owner's becomes the dequantised value; lanes before it keep theirs
    {
        const float pr = eb * u[M0];
        const float t = s.w[M0] - pr;
        s.w[M0] = p > P0 ? t : (own ? z.dq : s.w[M0]);
    }
    // every later column of this lane (two per instruction where a pair is available)
    constexpr int MS = M0 + 1;
    if (MS < NM && (MS & 1)) {
        const float pr = eb * u[MS];
        s.w[MS] = s.w[MS] - pr;
    }
    const f32x2 e2 = {eb, eb};
#pragma unroll
    for (int m = (MS + 1) & ~1; m < NM; m += 2) {
        const f32x2 uu = {u[m], u[m + 1]};
        const f32x2 pr = e2 * uu;
        f32x2 wp = {s.w[m], s.w[m + 1]};
        wp = wp - pr;
        s.w[m] = wp[0];
        s.w[m + 1] = wp[1];
    }
    __builtin_amdgcn_sched_barrier(0);   // keep a step's LDS reads next to their use (register pressure)
}

template <int NL, int M0, int P0>
__device__ __forceinline__ void lane_steps(StepState<NL>& s, const float* __restrict__ Ut, const float* __restrict__ dd,
                                           int p, bool hi, float qmin, float qmax) {
    if constexpr (P0 < NL) {
        col_step<TriLayout<NL>, M0, P0>(s, Ut, dd, p, hi, qmin, qmax);
        lane_steps<NL, M0, P0 + 1>(s, Ut, dd, p, hi, qmin, qmax);
    }
}

// the row's loss: the NL columns' terms of a macro-step added in column order, in every lane of the row alike (the
// row-per-lane kernel's and the oracle's order: ascending column)
template <int NL, int P0>
__device__ __forceinline__ void lane_loss(StepState<NL>& s, float t, bool hi) {
    if constexpr (P0 < NL) {
        s.lsum = s.lsum + row_bcast<NL, P0>(t, hi);
        lane_loss<NL, P0 + 1>(s, t, hi);
    }
}

// ---------------------------------------------------------------------------------------------------
// sweep_quad_kernel's own part: scales streamed ahead of the steps, ragged blocks, rows past R.
constexpr int QPF = 3;   // macro-steps (of 4 columns) a lane's scale / zero-point loads run ahead of their use

struct QuadScales {
    const float* scale_t;   // + rowc
    const float* zp_t;      // + rowc
    const int32_t* gcol;    // g_idx + i1 + p
    int R, nm;
};

template <int M>
__device__ __forceinline__ void quad_load_scales(StepState<QL>& s, const QuadScales& q) {
#if defined(QT_SWEEP_LAB) && QT_SWEEP_LAB == 3     // lab build 3 (timing only): no scale / zero-point loads inside the loop
    if constexpr (M >= QPF && M < QM) {
        s.sc[M] = s.sc[M - QPF];
        s.zz[M] = s.zz[M - QPF];
        return;
    }
#endif
    if constexpr (M < QM) {
        const int g = q.gcol[M < q.nm ? 4 * M : 0];
        s.sc[M] = q.scale_t[(size_t)g * q.R];
        s.zz[M] = q.zp_t[(size_t)g * q.R];
    }
}

template <int M0>
__device__ __forceinline__ void quad_macro_step(StepState<QL>& s, const QuadScales& qs, const float* __restrict__ Up,
                                                const float* __restrict__ dd,
                                                int p, float qmin, float qmax, bool valid, int row, int R, int i1,
                                                int8_t* __restrict__ Qt, float* __restrict__ ErrT) {
    quad_load_scales<M0 + QPF>(s, qs);
    col_step<QuadLayout, M0, 0>(s, Up, dd, p, false, qmin, qmax);
    col_step<QuadLayout, M0, 1>(s, Up, dd, p, false, qmin, qmax);
    col_step<QuadLayout, M0, 2>(s, Up, dd, p, false, qmin, qmax);
    col_step<QuadLayout, M0, 3>(s, Up, dd, p, false, qmin, qmax);
    // every lane now holds the level, the error and the rounding residual of its own column 4 M0 + p
    lane_loss<QL, 0>(s, (s.dv * s.dv) * dd[BS + 4 * M0 + p], false);
#if defined(QT_SWEEP_LAB) && QT_SWEEP_LAB == 2     // lab build 2 (timing only): no stores inside the loop
    if (valid && M0 == QM - 1) {
#else
    if (valid) {
#endif
        const int c = 4 * M0 + p;
        Qt[(size_t)(i1 + c) * R + row] = (int8_t)s.qv;
        ErrT[(size_t)c * R + row] = s.ev;
    }
}

template <int M0>
__device__ __forceinline__ void quad_run(StepState<QL>& s, const QuadScales& qs, const float* __restrict__ Up,
                                         const float* __restrict__ dd, int p,
                                         float qmin, float qmax, bool valid, int row, int R, int i1, int nm,
                                         int8_t* __restrict__ Qt, float* __restrict__ ErrT) {
    if constexpr (M0 < QM) {
        if (M0 >= nm) return;       // ragged last block: cnt = 4 nm columns (wave-uniform)
        quad_macro_step<M0>(s, qs, Up, dd, p, qmin, qmax, valid, row, R, i1, Qt, ErrT);
        quad_run<M0 + 1>(s, qs, Up, dd, p, qmin, qmax, valid, row, R, i1, nm, Qt, ErrT);
    }
}

__global__ __launch_bounds__(QTHREADS) void sweep_quad_kernel(float* __restrict__ W, int R, int K,
                                                              const float* __restrict__ U,
                                                              const float* __restrict__ scale_t,
                                                              const float* __restrict__ zp_t,
                                                              const int32_t* __restrict__ g_idx, int i1, int cnt,
                                                              float qmin, float qmax, int8_t* __restrict__ Qt,
                                                              float* __restrict__ ErrT, float* __restrict__ loss,
                                                              int prio, SweepGroups sg) {
    qt_set_chain_prio(prio);
    if (sg.n > 1) {
        const int g = sweep_group_of(sg, blockIdx.x * QROWS);
        U += (size_t)g * sg.bsU;
        g_idx += (size_t)g * K;
    }
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Up = sm;                      // [BS][QL][UP_P]
    float* dd = sm + BS * UP_C;          // [BS] diag, [BS] 1 / diag^2
    const int tid = threadIdx.x;
    const int p = tid & (QL - 1);
    const int row = blockIdx.x * QROWS + (tid >> 2);
    const bool valid = row < R;
    const int rowc = valid ? row : R - 1;
    const int nm = cnt >> 2;             // cnt % 4 == 0 (K % 4 == 0)

    {   // the U block, strictly above the diagonal, per (step, lane class); NV independent float4 loads per thread
        const float* ublk = U + (size_t)i1 * K + i1;
        constexpr int NV = BS * BS / 4 / QTHREADS;
        f32x4 v[NV];
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const int e4 = tid + QTHREADS * r;                 // float4 index in the 128 x 32 grid
            const int i = e4 >> 5, j = (e4 & 31) * 4;
            const int ic = i < cnt ? i : cnt - 1, jc = j < cnt ? j : cnt - 4;
            v[r] = *(const f32x4*)(ublk + (size_t)ic * K + jc);
        }
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const int e4 = tid + QTHREADS * r;
            const int i = e4 >> 5, m = e4 & 31, j = m * 4;
            const bool inside = i < cnt && j < cnt;
#pragma unroll
            for (int q = 0; q < 4; ++q) Up[i * UP_C + q * UP_P + m] = (inside && j + q > i) ? v[r][q] : 0.0f;
        }
    }
    if (tid < BS) {
        const float d = (tid < cnt) ? U[(size_t)(i1 + tid) * K + (i1 + tid)] : 1.0f;
        dd[tid] = d;
        dd[BS + tid] = 1.0f / (d * d);   // only the loss uses it (tolerance 1e-6, not part of the bit-exact contract)
    }
    StepState<QL> s;
    {
        const float* wrow = W + (size_t)rowc * K + i1 + p;
#pragma unroll
        for (int m = 0; m < QM; ++m) s.w[m] = m < nm ? wrow[4 * m] : 0.0f;
    }
    // the row's running loss, read with the row itself: as `loss[row] = loss[row] + ...` at the end it was one more
    // memory round trip behind the last column step of every block launch
    const float loss_in = (valid && p == 0) ? loss[row] : 0.0f;
    const QuadScales qs = {scale_t + rowc, zp_t + rowc, g_idx + i1 + p, R, nm};
    quad_load_scales<0>(s, qs);
    quad_load_scales<1>(s, qs);
    quad_load_scales<2>(s, qs);
    static_assert(QPF == 3, "the prologue loads the first QPF macro-steps' scales");
    s.lsum = 0.0f;
    s.qv = 0.0f;
    s.ev = 0.0f;
    s.dv = 0.0f;
    __syncthreads();
    // consume the early loss read here, where the row's own loads are waited for anyway: its use at the end would
    // otherwise carry an s_waitcnt vmcnt(0) that also waits for every store of the write-back to be acknowledged
    asm volatile("" ::"v"(loss_in));
    step_fetch<QuadLayout, 0>(s, Up, dd, p);

#if !defined(QT_SWEEP_LAB) || QT_SWEEP_LAB != 1   // lab build 1 (tools/sweep_lab.sh, timing only): prologue + epilogue alone
    quad_run<0>(s, qs, Up, dd, p, qmin, qmax, valid, row, R, i1, nm, Qt, ErrT);
#endif

    if (valid) {   // dequantised values back to W (upstream: W[:, i1:i2] = Q1)
        float* wrow = W + (size_t)row * K + i1 + p;
#pragma unroll
        for (int m = 0; m < QM; ++m)
            if (m < nm) wrow[4 * m] = s.w[m];
    }
    if (valid && p == 0) loss[row] = loss_in + s.lsum / 2.0f;
}

// ---------------------------------------------------------------------------------------------------
// sweep_fused_kernel: ONE launch = the whole batch b (all its 128-column blocks AND the near updates between
// them) for every group of rows  +  the far update of batch b - 1 on the columns right of batch b.
//
// Rows of W are independent given U, and the far update of batch b - 1 right of batch b touches no column that
// batch b reads or writes, so the two kinds of workgroup share nothing but the launch: no flag, no wait.  The
// first n_row_wgs workgroups own 512 / NL rows each; the others run sgemm_ring_body over the far update's tiles.
// Both kinds fit the ring's budget (512 threads, 128 registers, <= 80 KiB of LDS: two workgroups per CU, of
// either kind), so the latency-bound block steps run on SIMDs whose MFMA pipe the far update keeps busy.
//
// A row workgroup, per block of the batch:
//   * the 128 steps with NL lanes per row (lane (r, p) owns columns NL m + p): sweep_quad_kernel's step with a
//     wider broadcast -- per ELEMENT the same operations in the same order (ascending source column,
//     w = w - (err * u) with two roundings, IEEE divisions, rintf; loss in column order), so the same bits;
//   * the near update of the batch's remaining columns for its own rows: per 32 x 32 tile one ascending-k
//     chain from zero over the block's 128 k on v_mfma_f32_32x32x2f32, k paired (2 kk, 2 kk + 1) as in
//     sgemm_tn's kernels, then one subtraction -- the bits of the separate MODE_SUB launch.  The error rows come
//     from LDS (the steps leave them there), the U panel straight from global memory.
// LDS: the U block's strict upper triangle (TriLayout); the block's errors [128][rows];
// the diagonal.  66 560 B (NL = 16, 32 rows) / 74 752 B (NL = 8, 64 rows).
template <int NL, int M0>
__device__ __forceinline__ void lane_run(StepState<NL>& s, const float* __restrict__ Ut, const float* __restrict__ dd,
                                         float* __restrict__ Es, int p, bool hi, int rl, float qmin, float qmax, int row,
                                         int R, int i1, int8_t* __restrict__ Qt, float* __restrict__ ErrB) {
    if constexpr (M0 < LaneGeo<NL>::NM) {
        lane_steps<NL, M0, 0>(s, Ut, dd, p, hi, qmin, qmax);
        // every lane now holds the level, the error and the rounding residual of its own column NL M0 + p
        const int c = NL * M0 + p;
        lane_loss<NL, 0>(s, (s.dv * s.dv) * dd[BS + c], hi);
        asm volatile("" : "+v"(s.lsum));     // summed here: left alone, hipcc keeps all 128 terms for one sum at the block's end (spills)
        Qt[(size_t)(i1 + c) * R + row] = (int8_t)s.qv;
        ErrB[(size_t)c * R + row] = s.ev;
        Es[c * LaneGeo<NL>::ROWS + rl] = s.ev;
        lane_run<NL, M0 + 1>(s, Ut, dd, Es, p, hi, rl, qmin, qmax, row, R, i1, Qt, ErrB);
    }
}

struct FusedArgs {
    float* W;
    int R, K;
    const float* U;
    const float* scale_t;
    const float* zp_t;
    const int32_t* g_idx;
    int b0, nblk;              // the batch: columns [b0, b0 + 128 nblk)
    float qmin, qmax;
    int8_t* Qt;
    float* ErrT;               // [nblk * 128][R], this batch's buffer
    float* loss;
    int prio;
    int n_row_wgs;             // the launch's first workgroups; the others walk the far update's tiles
};

template <int NL>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void sweep_fused_kernel(const FusedArgs f,
                                                                                                     const SweepGroups sg,
                                                                                                     const RingArgs far) {
    using G = LaneGeo<NL>;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    if ((int)blockIdx.x >= f.n_row_wgs) {
        sgemm_ring_body<true>(far, (char*)sm, f.n_row_wgs);
        return;
    }
    qt_set_chain_prio(f.prio);
    const int R = f.R, K = f.K;
    const float* U = f.U;
    const int32_t* g_idx = f.g_idx;
    const int row0 = blockIdx.x * G::ROWS;
    if (sg.n > 1) {
        const int g = sweep_group_of(sg, row0);
        U += (size_t)g * sg.bsU;
        g_idx += (size_t)g * K;
    }
    float* Ut = sm;                          // the U block's triangle (LaneGeo::ut_base)
    float* Es = sm + G::UT_FLOATS;           // [BS k][ROWS]: the block's errors, the near update's A operand
    float* dd = Es + G::ES_FLOATS;           // [BS] diag, [BS] 1 / diag^2
    float* W = f.W;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int bend = f.b0 + f.nblk * BS;
    float lrow = (threadIdx.x & (NL - 1)) == 0 ? f.loss[row0 + threadIdx.x / NL] : 0.0f;

    for (int blk = 0; blk < f.nblk; ++blk) {
        // Every per-lane index of a block is derived from this opaque copy of the thread id: were they loop
        // invariants, hipcc would compute the block's ~100 per-lane addresses once in front of the loop and keep
        // them in scratch (the build refuses a private segment); recomputing them costs a few dozen integer
        // operations per 128 steps.
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63;
        const int p = tid & (NL - 1), rl = tid / NL;
        const bool hi = (tid & 8) != 0;
        const int row = row0 + rl;               // R % 128 == 0: every row exists
        const int h = lane >> 5, l31 = lane & 31;
        const int i1 = f.b0 + blk * BS, i2 = i1 + BS;
        const float* ublk = U + (size_t)i1 * K + i1;
        {   // the U block, strictly above the diagonal: 8 independent float4 loads per thread, then LDS
            f32x4 v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int e4 = tid + 512 * r;                      // float4 index in the 128 x 32 grid
                const int i = e4 >> 5, jj = e4 & 31;
                v[r] = *(const f32x4*)(ublk + (size_t)i * K + jj * 4);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int e4 = tid + 512 * r;
                const int i = e4 >> 5, jj = e4 & 31;
                const int m = jj / (NL / 4), pc = (jj % (NL / 4)) * 4;      // columns 4 jj + q = NL m + pc + q
                const int k4 = m >> 2, band = i / G::BAND;
                if (k4 >= band) {
                    float* dst = Ut + G::ut_base(i) + (k4 - band) * G::BLK + pc * 4 + (m & 3);
#pragma unroll
                    for (int q = 0; q < 4; ++q) dst[q * 4] = (jj * 4 + q > i) ? v[r][q] : 0.0f;
                }
            }
        }
        if (tid < BS) {
            const float d = ublk[(size_t)tid * K + tid];
            dd[tid] = d;
            dd[BS + tid] = 1.0f / (d * d);
        }
        StepState<NL> s;
        {
            const float* wrow = W + (size_t)row * K + i1 + p;
            const int32_t* gcol = g_idx + i1 + p;
#pragma unroll
            for (int m = 0; m < G::NM; ++m) {
                s.w[m] = wrow[NL * m];
                const int g = gcol[NL * m];
                s.sc[m] = f.scale_t[(size_t)g * R + row];
                s.zz[m] = f.zp_t[(size_t)g * R + row];
            }
        }
        s.lsum = 0.0f;
        s.qv = 0.0f;
        s.ev = 0.0f;
        s.dv = 0.0f;
        __syncthreads();
        step_fetch<TriLayout<NL>, 0>(s, Ut, dd, p);
        lane_run<NL, 0>(s, Ut, dd, Es, p, hi, rl, f.qmin, f.qmax, row, R, i1, f.Qt, f.ErrT + (size_t)blk * BS * R);
        {   // dequantised values back to W (upstream: W[:, i1:i2] = Q1)
            float* wrow = W + (size_t)row * K + i1 + p;
#pragma unroll
            for (int m = 0; m < G::NM; ++m) wrow[NL * m] = s.w[m];
        }
        lrow = lrow + s.lsum / 2.0f;
        if (blk + 1 == f.nblk) break;
        __syncthreads();      // the block's errors are in Es; nobody reads Ut any more
        // near update of the batch's remaining columns, this workgroup's rows: W[rows, i2:bend] -= Es^T U[i1:i2, i2:bend]
        {
            const int tiles_n = (bend - i2) / 32;
            const int n_t = tiles_n * (G::ROWS / 32);
            for (int t = wave; t < n_t; t += 8) {
                const int tm = t / tiles_n, tn = t - tm * tiles_n;
                const int col0 = i2 + tn * 32;
                float* cp = W + (size_t)(row0 + tm * 32 + 4 * h) * K + col0 + l31;
                float cin[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) cin[r] = cp[(size_t)((r & 3) + 8 * (r >> 2)) * K];
                const float* bp = U + (size_t)(i1 + h) * K + col0 + l31;
                const float* ap = Es + h * G::ROWS + tm * 32 + l31;
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
                for (int k0 = 0; k0 < BS / 2; k0 += 16) {
                    float b[16];
#pragma unroll
                    for (int kk = 0; kk < 16; ++kk) b[kk] = bp[(size_t)(2 * (k0 + kk)) * K];
#pragma unroll
                    for (int kk = 0; kk < 16; ++kk) {
                        const float a = ap[2 * (k0 + kk) * G::ROWS];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[kk], acc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) cp[(size_t)((r & 3) + 8 * (r >> 2)) * K] = cin[r] - acc[r];
            }
        }
        __syncthreads();      // the next block's columns are up to date for every row of the workgroup
    }
    if ((threadIdx.x & (NL - 1)) == 0) f.loss[row0 + threadIdx.x / NL] = lrow;
}

}  // namespace

// OPT-IN, NOT the parity contract (QT_SWEEP_FAR=bf16x3): the far update as a three-plane bf16 product (gemm3_tn.h) instead
// of the f32-MFMA chain.  Every product is fp32-accurate (what the planes drop is <= 2^-24 of it) but the sum is not the
// ascending-k fmaf chain the oracle fixes (that order is this repo's choice, upstream leaves it to BLAS),
// so the outputs agree with the oracle's to a rate, not to the bit -- as they already do across two factorisations.
// What it buys: the far update is 1.5 TFLOP of f32 MFMA per Llama-3-8B layer (~13 ms); as 9 TFLOP of bf16 MFMA ~7 ms.
static bool sweep_far_bf16x3(int R, int K) {
    const char* e = getenv("QT_SWEEP_FAR");
    return e && e[0] == 'b' && K % 8 == 0 && R % 4 == 0;
}
struct FarPlan {
    int64_t ldU, ldE;          // plane pitches (elements): U planes [K][ldU], error planes [kmax][ldE]
    size_t u_bytes, e_bytes, tab_bytes;
    int Tm, Tn_max, kmax;
};
static FarPlan far_plan(int R, int K, int blocksize) {
    FarPlan f;
    f.kmax = SWEEP_MAX_BATCH * blocksize;
    f.ldU = (int64_t)qt_align_up((size_t)K, 256);
    f.ldE = (int64_t)qt_align_up((size_t)R, 256);
    f.u_bytes = qt_align_up((size_t)3 * K * f.ldU * 2, 256);
    f.e_bytes = qt_align_up((size_t)3 * f.kmax * f.ldE * 2, 256);
    f.Tm = (R + 255) / 256;
    f.Tn_max = (K + 255) / 256;
    f.tab_bytes = qt_align_up((size_t)f.Tm * f.Tn_max * sizeof(G3Item), 256);
    return f;
}

static size_t sweep_err_bytes(int R, int blocksize) {
    return qt_align_up((size_t)SWEEP_MAX_BATCH * blocksize * R * 4, 256);
}

// Blocks per batch: 4, 8 from K = 8192 (measurements at the batch loop in sweep_run); QT_SWEEP_BATCH forces it.
static int sweep_batch_blocks(int K) {
    const char* e = getenv("QT_SWEEP_BATCH");
    const int b = e ? atoi(e) : (K >= 8192 ? 8 : 4);
    return b < 1 ? 1 : (b > SWEEP_MAX_BATCH ? SWEEP_MAX_BATCH : b);
}

// One of the fused form's two error buffers: the errors of one batch as long as this call's batches are.  Two
// batches of up to 4 blocks fit the room the chain of launches has always asked for (8 blocks).
static size_t sweep_fused_err_bytes(int R, int K, int blocksize) {
    return qt_align_up((size_t)sweep_batch_blocks(K) * blocksize * R * 4, 256);
}

// Whether a sweep of this shape may take the fused form (sweep_fused_kernel), as far as shape and environment say:
// whole 128-tiles, the f32 far update, and up to 6144 rows unless QT_SWEEP_FUSED=1 asks for it at any height
// (QT_SWEEP_FUSED=0: never).  Read per call; the workspace holds the second error buffer only where this holds.
static bool sweep_fused_shape(int R, int K) {
    const char* e = getenv("QT_SWEEP_FUSED");
    return !(e && e[0] == '0') && (R <= 6144 || (e && e[0] == '1')) && K % BS == 0 && R % 128 == 0 &&
           !sweep_far_bf16x3(R, K);
}

extern "C" size_t qt_gptq_sweep_workspace_bytes(int R, int K, int blocksize) {
    if (R <= 0 || blocksize <= 0) return 0;
    // ErrT[8][blocksize][R]; the fused form needs two buffers of one batch each: a batch writes one while the far
    // update of the batch before it, running in the same launch, still reads the other
    size_t n = sweep_err_bytes(R, blocksize);
    if (sweep_fused_shape(R, K) && 2 * sweep_fused_err_bytes(R, K, blocksize) > n) n = 2 * sweep_fused_err_bytes(R, K, blocksize);
    n += 256;
    if (sweep_far_bf16x3(R, K)) {
        const FarPlan f = far_plan(R, K, blocksize);
        n += f.u_bytes + f.e_bytes + f.tab_bytes;
    }
    return n;
}

// What every schedule of a sweep reads.
struct SweepCtx {
    float* W;
    int R, K;
    const float* U;
    const float* scale_t;
    const float* zp_t;
    const int32_t* g_idx;
    float qmin, qmax;
    int8_t* Qt;
    float* loss;
    float* ErrT;            // the workspace, 256-byte aligned: ErrT[batch][128][R]
    int batch_blocks;       // blocks per batch (sweep_batch_blocks)
    int prio;
    hipStream_t stream;
    const SweepGroups& sg;
};

// The update product  W[:, c0:c1] -= Err^T U[k0:k0+kdim, c0:c1]  (Err: [kdim][R]) as qt_sgemm_tn and the ring take it:
// per element one ascending-k chain, or with chain_len > 0 one chain per chain_len rows of Err, subtracted in turn.
static SgemmArgs sweep_update_args(const SweepCtx& c, const float* Err, int k0, int kdim, int c0, int c1, int chain_len) {
    SgemmArgs g;
    g.A = Err; g.lda = c.R;
    g.B = c.U + (size_t)k0 * c.K + c0; g.ldb = c.K;
    g.Cin = c.W + c0; g.ldcin = c.K;
    g.Cout = c.W + c0; g.ldcout = c.K;
    g.M = c.R; g.N = c1 - c0; g.kdim = kdim; g.k_mode = SG_K_FULL; g.mode = SG_MODE_SUB;
    g.chain_len = chain_len;
    // stacked problems: an update product's B operand (rows of U) depends on the row group of the output tile
    if (c.sg.n > 1) {
        g.n_groups = c.sg.n;
        g.group_bsB = c.sg.bsU;
        for (int i = 0; i < c.sg.n; ++i) g.group_m_end[i] = c.sg.row_end[i];
    }
    return g;
}

// A kernel's dynamic LDS beyond the default limit, asked for once per device.
template <auto Kernel>
static hipError_t sweep_lds_attr(size_t lds_bytes) {
    static QtOncePerDevice once;
    return once.run([&] {
        return hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    });
}

// The opt-in three-plane far update (sweep_far_bf16x3): its plan and its room in the workspace behind ErrT
// (never beside the fused form's second error buffer).
struct Far3 {
    FarPlan fp;
    unsigned short *Upl, *Epl;
    G3Item* tab;
};

static int sweep_far3_prepare(const SweepCtx& c, Far3& f) {
    const int K = c.K;
    const FarPlan& fp = f.fp = far_plan(c.R, K, BS);
    char* q = (char*)c.ErrT + sweep_err_bytes(c.R, BS);
    f.Upl = (unsigned short*)q;
    q += fp.u_bytes;
    f.Epl = (unsigned short*)q;
    q += fp.e_bytes;
    f.tab = (G3Item*)q;
    // planes of U once (pad columns zeroed: edge tiles read them), the tile list once: column-major in tiles, so a
    // far update over the first Tn' tile columns right of the batch is a prefix of it
    QT_HIP(hipMemsetAsync(f.Upl, 0, fp.u_bytes, c.stream));
    QT_HIP(hipMemsetAsync(f.Epl, 0, fp.e_bytes, c.stream));
    int rc = qt_split3_launch(c.U, K, K, K, f.Upl, fp.ldU, (int64_t)K * fp.ldU, 0, 0, 0, c.stream);
    if (rc) return rc;
    static std::mutex m;
    static std::map<std::tuple<int, int, int>, G3Item*> tabs;      // pinned, per (Tm, Tn_max, chunks)
    const int c_end = BS * c.batch_blocks / G3_CHUNK_ROWS;
    G3Item* host = nullptr;
    {
        std::lock_guard<std::mutex> lock(m);
        const auto key = std::make_tuple(fp.Tm, fp.Tn_max, c_end);
        auto it = tabs.find(key);
        if (it == tabs.end()) {
            if (hipHostMalloc((void**)&host, fp.tab_bytes, hipHostMallocDefault) != hipSuccess) {
                qt_set_error("qt_gptq_sweep: no pinned memory for the far update's tile table");
                return QT_ERR_HIP;
            }
            int n = 0;
            for (int tj = 0; tj < fp.Tn_max; ++tj)
                for (int ti = 0; ti < fp.Tm; ++ti) host[n++] = {(ti << 16) | tj, 0, c_end, -1};
            tabs[key] = host;
        } else {
            host = it->second;
        }
    }
    QT_HIP(hipMemcpyAsync(f.tab, host, (size_t)fp.Tm * fp.Tn_max * sizeof(G3Item), hipMemcpyHostToDevice, c.stream));
    return QT_OK;
}

// The far update of batch [b0, bend) as a three-plane product: error rows of the batch -> planes, then
// W[:, bend:] -= E^T U[b0:bend, bend:]
static int sweep_far3_update(const SweepCtx& c, const Far3& f, int b0, int bend) {
    const FarPlan& fp = f.fp;
    int rc = qt_split3_launch(c.ErrT, c.R, bend - b0, c.R, f.Epl, fp.ldE, (int64_t)fp.kmax * fp.ldE, 0, 0, 0, c.stream);
    if (rc) return rc;
    G3Args a;
    a.Apl = f.Epl; a.ld = fp.ldE; a.plane_stride = (int64_t)fp.kmax * fp.ldE; a.rowA0 = 0; a.colA0 = 0; a.colmax = (int)fp.ldE;
    a.Bpl = f.Upl; a.ldB = fp.ldU; a.plane_strideB = (int64_t)c.K * fp.ldU; a.rowB0 = b0; a.colB0 = bend; a.colmaxB = (int)fp.ldU;
    a.M = c.R; a.N = c.K - bend; a.C = c.W + bend; a.ldc = c.K; a.mode = G3_SUB;
    a.slabs = nullptr; a.red = nullptr; a.n_red = 0;
    a.items = f.tab; a.n_items = fp.Tm * ((c.K - bend + 255) / 256);
    return qt_gemm3_launch(a, c.stream);
}

// The fused form (sweep_fused_kernel): per batch b the stream carries far_near(b - 1) -- the far update of batch
// b - 1 on batch b's own columns -- and then ONE launch of [batch b's block steps and near updates] beside
// [far_rest(b - 1): the same far update on every column right of batch b].  far_near and far_rest are a column
// split of the one far update: the same chains in the same order per element.  Per element the subtractions
// still arrive in ascending block order (far_rest(b - 1) precedes far_near(b) and far_rest(b) on the stream).
// ErrT is double-buffered: batch b writes buffer b & 1 while far_rest(b - 1) reads the other.
static int sweep_run_fused(const SweepCtx& c) {
    const int R = c.R, K = c.K;
    // Lanes per row: 16 (32 rows per workgroup: R / 32 workgroups, the shortest step); QT_SWEEP_LANES=8 selects 8
    // (64 rows per workgroup), slower at both measured heights (at the choice of form in sweep_run) and kept for A/B runs.
    const char* lanes_env = getenv("QT_SWEEP_LANES");
    const int lanes = lanes_env && atoi(lanes_env) == 8 ? 8 : 16;
    QT_HIP(sweep_lds_attr<sweep_fused_kernel<16>>(LaneGeo<16>::LDS));
    QT_HIP(sweep_lds_attr<sweep_fused_kernel<8>>(LaneGeo<8>::LDS));
    float* Err[2] = {c.ErrT, (float*)((char*)c.ErrT + sweep_fused_err_bytes(R, K, BS))};
    const int span = BS * c.batch_blocks;
    const int n_row_wgs = R / (512 / lanes);
    int b = 0;
    for (int b0 = 0; b0 < K; b0 += span, ++b) {
        const int bend = (b0 + span < K) ? b0 + span : K;
        RingArgs far{};
        int far_wgs = 0;
        if (b > 0) {
            const float* err_prev = Err[(b - 1) & 1];
            // far_near(b - 1)
            const int rc = qt_sgemm_tn(sweep_update_args(c, err_prev, b0 - span, span, b0, bend, BS), c.stream);
            if (rc) return rc;
            if (bend < K) {                              // far_rest(b - 1)
                far = sgemm_ring_args(sweep_update_args(c, err_prev, b0 - span, span, bend, K, BS));
                // two workgroups per CU, 256 CUs: what the row workgroups leave, at least one per CU
                const int room = 512 - n_row_wgs > 256 ? 512 - n_row_wgs : 256;
                far_wgs = far.n_tiles < room ? far.n_tiles : room;
            }
        }
        FusedArgs f;
        f.W = c.W; f.R = R; f.K = K; f.U = c.U; f.scale_t = c.scale_t; f.zp_t = c.zp_t; f.g_idx = c.g_idx;
        f.b0 = b0; f.nblk = (bend - b0) / BS;
        f.qmin = c.qmin; f.qmax = c.qmax; f.Qt = c.Qt; f.ErrT = Err[b & 1]; f.loss = c.loss; f.prio = c.prio;
        f.n_row_wgs = n_row_wgs;
        qt_prof_mark(QT_PROF_SWEEP_BLOCK, c.stream);
        if (lanes == 16)
            hipLaunchKernelGGL(sweep_fused_kernel<16>, dim3(n_row_wgs + far_wgs), dim3(512), LaneGeo<16>::LDS, c.stream, f,
                               c.sg, far);
        else
            hipLaunchKernelGGL(sweep_fused_kernel<8>, dim3(n_row_wgs + far_wgs), dim3(512), LaneGeo<8>::LDS, c.stream, f,
                               c.sg, far);
        qt_prof_mark(QT_PROF_SWEEP_BLOCK, c.stream);
        QT_LAUNCH_CHECK();
    }
    return QT_OK;
}

// The chain of launches: per block one block kernel (quad: four lanes per row, else a lane per row) and the near
// update of the batch's remaining columns, per batch one far update (far3: as the opt-in three-plane product).
// Lazy far update: the blocks of a batch update only the batch's own later columns right away
// (k = 128, few columns); everything to the right of the batch gets the batch's chains in ONE
// pass over W (chain_len = 128: same roundings, in the same order, as one pass per block), so
// the read-modify-write traffic on W drops by the batch size.
static int sweep_run_chain(const SweepCtx& c, bool quad, bool far3) {
    const int R = c.R, K = c.K, span = BS * c.batch_blocks;
    QT_HIP(sweep_lds_attr<sweep_block_kernel>(SWEEP_LDS));
    QT_HIP(sweep_lds_attr<sweep_quad_kernel>(QUAD_LDS));
    Far3 f3{};
    if (far3) {
        const int rc = sweep_far3_prepare(c, f3);
        if (rc) return rc;
    }
    for (int b0 = 0; b0 < K; b0 += span) {
        const int bend = (b0 + span < K) ? b0 + span : K;   // first column right of the batch
        for (int i1 = b0; i1 < bend; i1 += BS) {
            const int i2 = (i1 + BS < K) ? i1 + BS : K;
            const int cnt = i2 - i1;
            float* err_blk = c.ErrT + (size_t)(i1 - b0) * R;
            qt_prof_mark(QT_PROF_SWEEP_BLOCK, c.stream);
            if (quad)
                hipLaunchKernelGGL(sweep_quad_kernel, dim3((R + QROWS - 1) / QROWS), dim3(QTHREADS), QUAD_LDS, c.stream, c.W,
                                   R, K, c.U, c.scale_t, c.zp_t, c.g_idx, i1, cnt, c.qmin, c.qmax, c.Qt, err_blk, c.loss,
                                   c.prio, c.sg);
            else
                hipLaunchKernelGGL(sweep_block_kernel, dim3((R + ROWS - 1) / ROWS), dim3(ROWS), SWEEP_LDS, c.stream, c.W, R,
                                   K, c.U, c.scale_t, c.zp_t, c.g_idx, i1, cnt, c.qmin, c.qmax, c.Qt, err_blk, c.loss,
                                   c.prio, c.sg);
            qt_prof_mark(QT_PROF_SWEEP_BLOCK, c.stream);
            QT_LAUNCH_CHECK();
            if (i2 < bend) {   // near update: the rest of this batch
                const int rc = qt_sgemm_tn(sweep_update_args(c, err_blk, i1, cnt, i2, bend, 0), c.stream);
                if (rc) return rc;
            }
        }
        if (bend == K) break;
        // far update: every chain of the batch, one pass
        const int rc = far3 && bend - b0 == span ? sweep_far3_update(c, f3, b0, bend)
                                                 : qt_sgemm_tn(sweep_update_args(c, c.ErrT, b0, bend - b0, bend, K, BS), c.stream);
        if (rc) return rc;
    }
    return QT_OK;
}

static int sweep_run(float* W, int R, int K, const float* U, const float* scale_t, const float* zp_t, int G,
                     const int32_t* g_idx, int blocksize, int num_bits, int8_t* Qt, float* loss, void* workspace,
                     size_t workspace_bytes, hipStream_t stream, const SweepGroups& sg) {
    QT_CHECK_ARG(W && U && scale_t && zp_t && g_idx && Qt && loss, "qt_gptq_sweep: null pointer");
    QT_CHECK_ARG(R > 0 && K > 0 && G > 0, "qt_gptq_sweep: bad shape R=%d K=%d G=%d", R, K, G);
    QT_CHECK_ARG(blocksize == BS, "qt_gptq_sweep: blocksize=%d unsupported (this build: 128)", blocksize);
    QT_CHECK_ARG(num_bits >= 2 && num_bits <= 8, "qt_gptq_sweep: num_bits=%d", num_bits);
    QT_CHECK_ARG(K % 4 == 0 && ((uintptr_t)W & 15) == 0, "qt_gptq_sweep: K %% 4 and 16-byte aligned W required");
    const size_t need = qt_gptq_sweep_workspace_bytes(R, K, blocksize);
    if (!workspace || workspace_bytes < need) {
        qt_set_error("qt_gptq_sweep: workspace %zu < required %zu", workspace_bytes, need);
        return QT_ERR_WORKSPACE;
    }
    float* ErrT = (float*)qt_align_up((size_t)workspace, 256);
    const bool far3 = sweep_far_bf16x3(R, K) && sg.n <= 1;      // the opt-in three-plane far update: single problem only
    const float qmin = -(float)(1 << (num_bits - 1)), qmax = (float)((1 << (num_bits - 1)) - 1);
    // QT_SWEEP_BLOCK=row: the row-per-lane block kernel (the round-1/2 form; A/B and cross-check); default: four lanes per row
    const char* blk_env = getenv("QT_SWEEP_BLOCK");
    const bool quad = !(blk_env && blk_env[0] == 'r');
    QT_HIP(hipMemsetAsync(loss, 0, (size_t)R * 4, stream));
    // Batch size: 4 blocks, 8 from K = 8192 up -- a longer batch halves the far update's traffic on W again but puts
    // more near-update columns between two block kernels (K = 14336 / R = 4096: 11.74 -> 11.35 ms; K = 4096 /
    // R = 28672: 5.9 -> 6.0 ms; K = 8192: +-0.5 %, profiles/r03_sweep_batch_ab.txt).  The bits do not depend on it.  QT_SWEEP_BATCH forces it.
    const SweepCtx c = {W, R, K, U, scale_t, zp_t, g_idx, qmin, qmax, Qt, loss, ErrT, sweep_batch_blocks(K), qt_chain_prio(),
                        stream, sg};
    // The choice of form.  QT_SWEEP_FUSED=0 (read per call) forces the chain of launches; so do shapes off the ring's whole tiles.
    // Unset, the fused form is taken up to 6144 rows: the row workgroups run the quantise step in all 16 (8) lanes of a
    // row, 2.6 (1.5) times the vector work of four lanes per row.  That is free while they are a latency-bound chain on
    // a chip the far update fills, and a loss once the rows alone fill the chip (K = 4096 / R = 28672: 5.76 ms as
    // launches, 6.02 fused with 8 lanes, 6.90 with 16; K = 14336 / R = 4096: 11.3 -> 9.45 ms with 16, 10.2 with 8;
    // K = 4096 / R = 6144: 2.35 -> 1.97; profiles/sweep_fused_ab.txt, sweep_fused_stage_times_*.txt).  6144 is the
    // tallest shape measured faster; with the form taken up to 8192 rows the Llama-3-70B layer (R = 8192 at K = 8192 and
    // 28672) ran 340 ms per step against the parent's 324 in the one run made.  QT_SWEEP_FUSED=1 takes it at any height.
    const bool fused = sweep_fused_shape(R, K) && quad && (((uintptr_t)U | (uintptr_t)ErrT) & 15) == 0 &&
                       (sg.n <= 1 || sg.bsU % 4 == 0) &&
                       // the far update's shape as the ring sees it (column count and offsets are multiples of 128)
                       sgemm_ring_applies(sweep_update_args(c, ErrT, 0, BS * c.batch_blocks, 0, BS, BS));
    return fused ? sweep_run_fused(c) : sweep_run_chain(c, quad, far3);
}

extern "C" int qt_gptq_sweep(float* W, int R, int K, const float* U, const float* scale_t, const float* zp_t, int G,
                             const int32_t* g_idx, int blocksize, int num_bits, int8_t* Qt, float* loss,
                             void* workspace, size_t workspace_bytes, qt_stream_t stream_) {
    SweepGroups sg{};
    return sweep_run(W, R, K, U, scale_t, zp_t, G, g_idx, blocksize, num_bits, Qt, loss, workspace, workspace_bytes,
                     (hipStream_t)stream_, sg);
}

extern "C" int qt_gptq_sweep_grouped(float* W, int R, int K, const float* U, int64_t strideU, int n_groups,
                                     const int32_t* row_end, const float* scale_t, const float* zp_t, int G,
                                     const int32_t* g_idx, int blocksize, int num_bits, int8_t* Qt, float* loss,
                                     void* workspace, size_t workspace_bytes, qt_stream_t stream_) {
    QT_CHECK_ARG(n_groups >= 1 && n_groups <= SG_MAX_GROUPS && row_end, "qt_gptq_sweep_grouped: 1 <= n_groups <= %d", SG_MAX_GROUPS);
    SweepGroups sg{};
    sg.n = n_groups;
    sg.bsU = strideU;
    int prev = 0;
    for (int g = 0; g < n_groups; ++g) {
        // 128: the update products' tile height (no tile may straddle two factors); the block kernels need 64
        QT_CHECK_ARG(row_end[g] > prev && (row_end[g] % 128 == 0 || g == n_groups - 1),
                     "qt_gptq_sweep_grouped: group %d ends at row %d (ascending; every boundary but the last a multiple of 128)", g,
                     row_end[g]);
        sg.row_end[g] = row_end[g];
        prev = row_end[g];
    }
    QT_CHECK_ARG(prev == R, "qt_gptq_sweep_grouped: the last group ends at row %d, R = %d", prev, R);
    QT_CHECK_ARG(n_groups == 1 || strideU >= (int64_t)K * K, "qt_gptq_sweep_grouped: strideU < K*K");
    return sweep_run(W, R, K, U, scale_t, zp_t, G, g_idx, blocksize, num_bits, Qt, loss, workspace, workspace_bytes,
                     (hipStream_t)stream_, sg);
}
