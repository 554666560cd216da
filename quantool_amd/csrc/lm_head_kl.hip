// qt_lm_head_kl: the LM head applied to two models' hidden states at once -- per-token KL(P || Q), both log-sum-exps,
// both target NLLs and both argmaxes of a = Hp[M, K] x W[V, K]^T and b = Hq[M, K] x W[V, K]^T, with neither [M, V] logit
// matrix stored (include/quantool_amd.h).  Two kernels: lm_head_kl_kernel (128 token rows x 256
// vocabulary columns of BOTH logit matrices per 8-wave workgroup, the reduction streamed through the LDS-DMA ring of
// ring_pipe.h, a joint softmax epilogue on the fp32 accumulators that leaves one P record {max, sum, argmax, t} and one
// Q record {max, sum, argmax} per row and vocabulary tile) and lm_head_kl_reduce_kernel (one thread per row merges the
// row's records in ascending tile order).
//
// THE INSTANCE is lm_head_nll_kernel's (lm_head_nll.hip) with other source pointers for the two A units: both operands
// are 16-bit and K-contiguous, a unit is a HALF PANEL of 128 rows x 128 k-bytes = 64 elements of k = 16 KiB, one cache
// line per row and fetch, two LDS-DMA instructions per wave.  K-tile t (elements [64 t, 64 t + 64)) is the four units
// 4t .. 4t+3 = A0, B0, B1, A1, where
//     A0 = Hp rows m0 .. m0 + 127,   B0 / B1 = W rows n0 .. n0 + 127 / n0 + 128 .. n0 + 255,   A1 = Hq rows m0 .. m0 + 127
// (m0 = 128 m_tile: the SAME 128 token rows on both sides, each with its own pitch ldhp / ldhq), and its four phases are
// the quadrants A0 x B0, A0 x B1, A1 x B0, A1 x B1: per wave (2 (M) x 4 (N) waves per quadrant, 64 x 32 logits each)
// 2 x 1 MFMA tiles x 4 k-steps = 8 v_mfma_f32_32x32x16_bf16 / _f16.  So acc[0][qb][mi][r] is a[m, v] and
// acc[1][qb][mi][r] is b[m, v] for the same (m, v): same lane, same register index.  Fragments stay in registers
// across the phases that share them: phase 4t reads A0 and B0, 4t+1 B1, 4t+2 A1, 4t+3 nothing.
//   R 8 slots (slot = unit % 8: two K-tiles), L 6 (unit u+6 is issued in phase u), N 2 per wave.
//   K is a multiple of 128 elements, so the unit count nu = K / 16 is a multiple of 8, at least 8: every trip round the
//   ring is whole, and the last trip is the one that issues nothing past nu (the drain ladder).
//   RAW: unit i is first read in phase i - 1 at the earliest (B0, B1, A1; A0 in phase i), so the counted wait of phase
//        u leaves only units u+3 .. u+6 in flight: vmcnt(2 * 4 = 8), and unit u+2 is read one phase after the wait
//        that retired it.  The prologue issues units 0 .. 5 and waits vmcnt(8): units 0 and 1 have landed in front of
//        the stagger's first barrier.  In the last trip the wait is ring_drain_wait<2, 5>(nu - u - 3): exactly the
//        units behind u+2 that exist stay in flight, and the last three phases wait vmcnt(0).  Which matrix a unit's
//        bytes come from does not enter: the count is per unit, two instructions each, as in lm_head_nll.hip.
//   WAR: unit i is last read in phase i at the latest (its reads retire at the lgkmcnt(0) that opens MATH(i)), and its
//        slot is re-filled by unit i+8, issued in phase i+2: ring_pipe.h's case L = R - 2.
//   THE EPILOGUE re-uses the first 14.5 KiB of the ring (targets, per-N-wave partial records of both sides).  It starts
//        behind ring_stagger_end (every wave has passed its last MATH, whose lgkmcnt(0) retired its last fragment read,
//        and has waited vmcnt(0) for its own LDS-DMA) and one more workgroup barrier: no read of a unit and no DMA
//        write into the ring is outstanding in any wave when the first epilogue store to LDS is issued.
// A tile row past M is fetched from row M - 1 on each side and a vocabulary row past V from row V - 1: the source row is
// clamped, the value is computed, columns >= V are masked and rows >= M are never stored.  K is a whole number of
// K-tiles, so no byte outside Hp[M, K], Hq[M, K] and W[V, K] is read.
//
// THE ROW'S SEQUENCE (what the header states).  One fp32 accumulator per logit, K-tiles in ascending k, four MFMA
// k-steps each: a[m, v] and b[m, v] are to the bit what lm_head_nll_kernel accumulates for (Hp, W) and (Hq, W).  The Q
// side is that kernel's record {m, s, i} and its merge (lm_head_rec.h).  The P side carries a fourth field
// t = sum exp(a - m) (a - b): the element record is {a, 1, col, a - b}, a masked column {-inf, 0, col, 0}, and t merges
// with the weights of s (t = t_lo w_lo + t_hi w_hi), so m, s and i of the P side are the NLL kernel's too.  Order, on
// both sides: the lane's two columns (c, c + 128), the 32 lanes by the xor steps 16, 8, 4, 2, 1 (lo = the lane whose
// bit is clear), the four N-waves in ascending order through the freed ring, the vocabulary tiles in ascending order in
// the reduce kernel.  The P and the Q scatter of an MFMA tile run one after the other, not side by side: 16 four-field
// records beside the 128 accumulator registers is what fits.  Nothing in that tree depends on the row's place in its
// tile or on the tile's place in the grid.  No atomics: every record and both target logits have exactly one writer.
#include <math.h>

#include "common.h"
#include "i8_ring_tile.h"
#include "lm_head_rec.h"

namespace {

struct KlArgs {
    const char* Hp;
    const char* Hq;
    const char* W;
    const void* targets;
    float4* rec_p;        // [tiles_n][M]: {max, sum, argmax (int bits), t}
    float4* rec_q;        // [tiles_n][M]: {max, sum, argmax (int bits), 0}
    float* tgt_p;         // [M]: the P-side accumulator at the target's column
    float* tgt_q;         // [M]: the Q-side one
    int64_t M;
    int64_t ldhp, ldhq, ldw;   // elements
    int V, K;
    int tgt64;
};

template <bool F16>
__global__ __launch_bounds__(NTHREADS, 2) void lm_head_kl_kernel(const KlArgs p) {
    __shared__ __attribute__((aligned(16))) char ring[RING * UNIT_BYTES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 2, wave_n = wave & 3;
    const bool group_b = wave >= 4;  // wave-uniform

    const int tiles_n = (p.V + BT - 1) / BT;
    const int tiles_m = (int)((p.M + HP - 1) / HP);
    int m_tile, n_tile;
    i8_ring_tile_of(blockIdx.x, tiles_m, tiles_n, m_tile, n_tile);
    const int64_t m0 = (int64_t)m_tile * HP;
    const int n0 = n_tile * BT;
    const int nu = p.K / 64 * 4;                      // units = phases; a multiple of 8 (host: K % 128 == 0)

    // ---- staging geometry: two LDS-DMA instructions per thread per unit (pieces 2 wave, 2 wave + 1) ----
    const int64_t a_last = p.M - 1 - m0;              // last valid row of the Hp / Hq / W panel, relative to the tile
    const int b_last = p.V - 1 - n0;
    const size_t pitch_p = (size_t)p.ldhp * 2, pitch_q = (size_t)p.ldhq * 2, pitch_b = (size_t)p.ldw * 2;   // bytes
    unsigned voff[4][2];                              // [A0 = Hp, B0, B1, A1 = Hq][instruction]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = 16 * wave + 8 * i + (lane >> 3);                   // row of the half panel
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        const int64_t ra = r < a_last ? r : a_last;                      // clamped: a valid row, the same on both sides
        const int rb0 = r < b_last ? r : b_last, rb1 = HP + r < b_last ? HP + r : b_last;
        voff[0][i] = (unsigned)((size_t)ra * pitch_p + 16 * c);          // < 128 * 2^23 (host: pitch <= 2^22 elements)
        voff[1][i] = (unsigned)((size_t)rb0 * pitch_b + 16 * c);
        voff[2][i] = (unsigned)((size_t)rb1 * pitch_b + 16 * c);
        voff[3][i] = (unsigned)((size_t)ra * pitch_q + 16 * c);
    }
    const unsigned ring_lds = (unsigned)(size_t)(QT_LDS char*)ring;
    const unsigned dst_wave = __builtin_amdgcn_readfirstlane(ring_lds + wave * 2048);  // wave-uniform
    const char* srcP = p.Hp + (size_t)m0 * pitch_p;   // scalar: k-byte 0 of the tile's first row
    const char* srcQ = p.Hq + (size_t)m0 * pitch_q;
    const char* srcB = p.W + (size_t)n0 * pitch_b;
    // unit i = 4 t + J: J is a compile-time constant wherever the slot is
    auto issue = [&](auto j_c, int t, int slot) {
        constexpr int J = decltype(j_c)::value;
        const unsigned d = dst_wave + (unsigned)slot * UNIT_BYTES;
        glds16_pair(voff[J][0], voff[J][1], (J == 0 ? srcP : J == 3 ? srcQ : srcB) + (size_t)t * KU, d, d + 1024);
    };

    // ---- fragment read geometry (per lane), byte offsets inside a unit ----
    const int lr = lane & 31, lh = lane >> 5;
    auto frag_off = [&](int r, int s) {               // row r of the half panel, k-step s
        const int x = (r >> 1) & 7;
        return (r >> 3) * 1024 + (r & 7) * 128 + 16 * ((2 * s + lh) ^ x);
    };
    int aoff[2][4], boff[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) aoff[mi][s] = frag_off(wave_m * 64 + mi * 32 + lr, s);
        boff[s] = frag_off(wave_n * 32 + lr, s);
    }

    f32x16 acc[2][2][2];                              // [side: 0 = P (Hp), 1 = Q (Hq)][B half][mi]
#pragma unroll
    for (int qa = 0; qa < 2; ++qa)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) acc[qa][qb][mi] = (f32x16){};

    // ---- the pipeline (ring_pipe.h): R 8, L 6, unit = a half panel, 2 LDS-DMA per wave and unit ----
    i32x4 fa[2][4], fb[2][4];                         // A: [mi][k-step], B: [half][k-step]
    // waits of ring_pipe.h one unit earlier: lead LEAD - 1 in its terms (units u+3 .. u+LEAD may stay in flight)
    auto drain_wait = [&](int u) { ring_drain_wait<2, LEAD - 1>(nu - u - 3); };
    auto phase = [&](auto slot_c, auto steady_c, int u) {
        constexpr int S = decltype(slot_c)::value;
        constexpr bool STEADY = decltype(steady_c)::value;
        constexpr int Q = S & 3, QA = Q >> 1, QB = Q & 1;
        constexpr int ISLOT = (S + LEAD) & (RING - 1);
        // ---- LOAD: the K-tile's units sit in slots (S & 4) + {0: A0, 1: B0, 2: B1, 3: A1} ----
        const char* tile = ring + (S & 4) * UNIT_BYTES;
        if constexpr (Q == 0 || Q == 2) {
            const char* base = tile + (Q == 0 ? 0 : 3) * UNIT_BYTES;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) fa[mi][s] = *(const i32x4*)(base + aoff[mi][s]);
        }
        if constexpr (Q == 0 || Q == 1) {
            const char* base = tile + (1 + QB) * UNIT_BYTES;
#pragma unroll
            for (int s = 0; s < 4; ++s) fb[QB][s] = *(const i32x4*)(base + boff[s]);
        }
        if (STEADY || u + LEAD < nu) {
            issue(std::integral_constant<int, (S + LEAD) & 3>{}, (u + LEAD) >> 2, ISLOT);
            wait_vmcnt<2 * (LEAD - 2)>();   // everything up to unit u+2 has landed; 4 units stay in flight
        } else {
            drain_wait(u);
        }
        // ---- MATH ----
        ring_sync_math([&] {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    acc[QA][QB][mi] = mfma16<F16>(__builtin_bit_cast(s16x8, fa[mi][s]),
                                                  __builtin_bit_cast(s16x8, fb[QB][s]), acc[QA][QB][mi]);
        });
    };

    // prologue: units 0..LEAD-1 in flight (nu >= 8), units 0 and 1 landed
    issue(std::integral_constant<int, 0>{}, 0, 0);
    issue(std::integral_constant<int, 1>{}, 0, 1);
    issue(std::integral_constant<int, 2>{}, 0, 2);
    issue(std::integral_constant<int, 3>{}, 0, 3);
    issue(std::integral_constant<int, 0>{}, 1, 4);
    issue(std::integral_constant<int, 1>{}, 1, 5);
    wait_vmcnt<2 * (LEAD - 2)>();
    ring_stagger_begin(group_b);

    int u = 0;
    for (; u + 8 + LEAD <= nu; u += 8)   // every phase issues a unit that exists
        ring_body<8>([&](auto slot_c, int uu) { phase(slot_c, std::true_type{}, uu); }, u);
    for (; u + 8 <= nu; u += 8)          // the last trip: the drain ladder
        ring_body<8>([&](auto slot_c, int uu) { phase(slot_c, std::false_type{}, uu); }, u);
    ring_stagger_end(group_b);
    __syncthreads();                     // the ring is free: see THE EPILOGUE above

    // ---- epilogue: targets -> LDS; per wave and row a P and a Q record over its 64 columns; 4 N-waves -> one each ----
    int* tgt_s = (int*)ring;                          // [128]: the row's target if it is a column of V, else -1
    float* pm = (float*)(ring + 512);                 // P side: [4 N-waves][128 rows] of m, s, i, t
    float* ps = pm + 4 * HP;
    int* pi = (int*)(ps + 4 * HP);
    float* pt = (float*)(pi + 4 * HP);
    float* qm = pt + 4 * HP;                          // Q side: m, s, i
    float* qs = qm + 4 * HP;
    int* qi = (int*)(qs + 4 * HP);                    // ends at 512 + 7 * 2048 bytes
    if (tid < HP) {
        const int64_t m = m0 + tid;
        int t = -1;
        if (m < p.M) {
            const int64_t tv = load_target(p.targets, p.tgt64, m);
            if (tv >= 0 && tv < p.V) t = (int)tv;
        }
        tgt_s[tid] = t;
    }
    __syncthreads();
    const int col0 = wave_n * 32 + lr;                // the lane's columns of the tile: col0 and col0 + 128
    const bool ok0 = n0 + col0 < p.V, ok1 = n0 + HP + col0 < p.V;
    const float ninf = -INFINITY;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int first = wave_m * 64 + mi * 32;
        const int out_row = (int)i8_ring_cd_row(first, lr >> 1, lh);     // the lane pair holds accumulator row lr >> 1
        {   // ---- Q side: lm_head_nll_kernel's record ----
            Rec v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float b0 = acc[1][0][mi][r], b1 = acc[1][1][mi][r];
                const Rec lo{ok0 ? b0 : ninf, ok0 ? 1.0f : 0.0f, col0};
                const Rec hi{ok1 ? b1 : ninf, ok1 ? 1.0f : 0.0f, col0 + HP};
                v[r] = rec_merge(lo, hi);
            }
            rec_scatter_step<16, 16>(v, lane);
            rec_scatter_step<8, 8>(v, lane);
            rec_scatter_step<4, 4>(v, lane);
            rec_scatter_step<2, 2>(v, lane);
            v[0] = rec_pair_step(v[0], lane);
            if ((lane & 1) == 0) {
                qm[wave_n * HP + out_row] = v[0].m;
                qs[wave_n * HP + out_row] = v[0].s;
                qi[wave_n * HP + out_row] = v[0].i;
            }
        }
        {   // ---- P side: the same record with t; the lane of the target's column stores both target logits ----
            RecT v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (int)i8_ring_cd_row(first, r, lh);
                const float a0 = acc[0][0][mi][r], a1 = acc[0][1][mi][r];
                const float b0 = acc[1][0][mi][r], b1 = acc[1][1][mi][r];
                const int d = tgt_s[row] - n0;        // rows >= M hold -1: no column matches
                if ((unsigned)d < (unsigned)BT && (d & (HP - 1)) == col0) {
                    p.tgt_p[m0 + row] = (d >> 7) ? a1 : a0;
                    p.tgt_q[m0 + row] = (d >> 7) ? b1 : b0;
                }
                const RecT lo{ok0 ? a0 : ninf, ok0 ? 1.0f : 0.0f, col0, ok0 ? a0 - b0 : 0.0f};
                const RecT hi{ok1 ? a1 : ninf, ok1 ? 1.0f : 0.0f, col0 + HP, ok1 ? a1 - b1 : 0.0f};
                v[r] = rec_merge(lo, hi);
            }
            rec_scatter_step<16, 16>(v, lane);
            rec_scatter_step<8, 8>(v, lane);
            rec_scatter_step<4, 4>(v, lane);
            rec_scatter_step<2, 2>(v, lane);
            v[0] = rec_pair_step(v[0], lane);
            if ((lane & 1) == 0) {
                pm[wave_n * HP + out_row] = v[0].m;
                ps[wave_n * HP + out_row] = v[0].s;
                pi[wave_n * HP + out_row] = v[0].i;
                pt[wave_n * HP + out_row] = v[0].t;
            }
        }
    }
    __syncthreads();
    if (tid < 2 * HP) {                               // threads 0-127: the P record of row tid; 128-255: the Q record
        const int row = tid & (HP - 1);
        if (m0 + row < p.M) {
            const int64_t at = (int64_t)n_tile * p.M + m0 + row;
            if (tid < HP) {
                RecT o{pm[row], ps[row], pi[row], pt[row]};
#pragma unroll
                for (int w = 1; w < 4; ++w)
                    o = rec_merge(o, RecT{pm[w * HP + row], ps[w * HP + row], pi[w * HP + row], pt[w * HP + row]});
                p.rec_p[at] = rec_pack(o, n0);
            } else {
                Rec o{qm[row], qs[row], qi[row]};
#pragma unroll
                for (int w = 1; w < 4; ++w) o = rec_merge(o, Rec{qm[w * HP + row], qs[w * HP + row], qi[w * HP + row]});
                p.rec_q[at] = rec_pack(o, n0);
            }
        }
    }
}

constexpr int RED_THREADS = 256;

struct KlOut {
    float* kl;
    float* nll_p;
    float* nll_q;
    float* lse_p;
    float* lse_q;
    int32_t* argmax_p;
    int32_t* argmax_q;
};

__global__ __launch_bounds__(RED_THREADS) void lm_head_kl_reduce_kernel(const float4* rec_p, const float4* rec_q,
                                                                         const float* tgt_p, const float* tgt_q,
                                                                         const void* targets, int tgt64, int64_t M,
                                                                         int V, int tiles_n, const KlOut out) {
    const int64_t m = (int64_t)blockIdx.x * RED_THREADS + threadIdx.x;
    if (m >= M) return;
    RecT a = rec_unpack_t(rec_p[m]);
    Rec b = rec_unpack(rec_q[m]);
    for (int t = 1; t < tiles_n; ++t) {
        a = rec_merge(a, rec_unpack_t(rec_p[(int64_t)t * M + m]));
        b = rec_merge(b, rec_unpack(rec_q[(int64_t)t * M + m]));
    }
    const float lp = a.m + logf(a.s);
    const float lq = b.m + logf(b.s);
    const int64_t tv = load_target(targets, tgt64, m);
    float np, nq;
    if (tv < 0) {
        np = 0.0f;
        nq = 0.0f;
    } else if (tv >= V) {
        np = __int_as_float(0x7fc00000);
        nq = np;
    } else {
        np = lp - tgt_p[m];
        nq = lq - tgt_q[m];
    }
    out.kl[m] = a.t / a.s - lp + lq;                  // not clamped at 0: rounding may leave a small negative value
    out.nll_p[m] = np;
    out.nll_q[m] = nq;
    out.lse_p[m] = lp;
    out.lse_q[m] = lq;
    out.argmax_p[m] = a.i;
    out.argmax_q[m] = b.i;
}

}  // namespace

extern "C" size_t qt_lm_head_kl_workspace_size(int64_t M, int V) {
    if (M <= 0 || V < 1) return 0;
    const size_t tiles_n = ((size_t)V + BT - 1) / BT;
    return 2 * (size_t)M * tiles_n * sizeof(float4) + 2 * (size_t)M * sizeof(float);
}

extern "C" int qt_lm_head_kl(const void* Hp, int64_t ldhp, const void* Hq, int64_t ldhq, const void* W, int64_t ldw,
                             int dtype, int64_t M, int K, int V, const void* targets, int target_bytes, float* kl,
                             float* nll_p, float* nll_q, float* lse_p, float* lse_q, int32_t* argmax_p,
                             int32_t* argmax_q, void* workspace, size_t workspace_bytes, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* fn = "qt_lm_head_kl";
    QT_CHECK_ARG(Hp, "%s: Hp is null", fn);
    QT_CHECK_ARG(Hq, "%s: Hq is null", fn);
    QT_CHECK_ARG(W, "%s: W is null", fn);
    QT_CHECK_ARG(targets, "%s: targets is null", fn);
    QT_CHECK_ARG(kl, "%s: kl is null", fn);
    QT_CHECK_ARG(nll_p, "%s: nll_p is null", fn);
    QT_CHECK_ARG(nll_q, "%s: nll_q is null", fn);
    QT_CHECK_ARG(lse_p, "%s: lse_p is null", fn);
    QT_CHECK_ARG(lse_q, "%s: lse_q is null", fn);
    QT_CHECK_ARG(argmax_p, "%s: argmax_p is null", fn);
    QT_CHECK_ARG(argmax_q, "%s: argmax_q is null", fn);
    QT_CHECK_ARG(qt_dtype_is16(dtype), "%s: dtype %d must be bf16 or fp16 (fp32 operands are not taken)", fn, dtype);
    QT_CHECK_ARG(target_bytes == 4 || target_bytes == 8, "%s: target_bytes %d must be 4 (int32) or 8 (int64)", fn,
                 target_bytes);
    QT_CHECK_ARG(M >= 0, "%s: M %lld is negative", fn, (long long)M);
    QT_CHECK_ARG(M <= 0x7fffffffLL, "%s: M %lld too large", fn, (long long)M);
    QT_CHECK_ARG(V >= 1, "%s: V %d must be at least 1", fn, V);
    QT_CHECK_ARG(K >= LMH_MIN_K, "%s: K %d is below %d, the smallest K the ring's prologue and drain take", fn, K,
                 LMH_MIN_K);
    QT_CHECK_ARG(K <= LMH_MAX_K, "%s: K %d exceeds %d", fn, K, LMH_MAX_K);
    QT_CHECK_ARG(K % LMH_MIN_K == 0, "%s: K %d is not a multiple of %d", fn, K, LMH_MIN_K);
    const struct {
        const char* name;
        const char* ld_name;
        const void* ptr;
        int64_t ld;
    } ops[3] = {{"Hp", "ldhp", Hp, ldhp}, {"Hq", "ldhq", Hq, ldhq}, {"W", "ldw", W, ldw}};
    for (const auto& o : ops) {
        QT_CHECK_ARG(o.ld >= K, "%s: %s %lld is below K %d", fn, o.ld_name, (long long)o.ld, K);
        QT_CHECK_ARG(o.ld % 8 == 0 && o.ld <= LMH_MAX_PITCH, "%s: %s %lld must be a multiple of 8 elements (16 bytes) "
                     "and at most %lld", fn, o.ld_name, (long long)o.ld, (long long)LMH_MAX_PITCH);
        QT_CHECK_ARG(((uintptr_t)o.ptr & 15) == 0, "%s: %s is not 16-byte aligned", fn, o.name);
    }
    if (M == 0) return QT_OK;
    const int tiles_n = (V + BT - 1) / BT;
    const int64_t tiles = ((M + HP - 1) / HP) * (int64_t)tiles_n;
    QT_CHECK_ARG(tiles <= 0x7fffffffLL, "%s: too many tiles (M %lld, V %d)", fn, (long long)M, V);
    const size_t need = qt_lm_head_kl_workspace_size(M, V);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15) != 0) {
        qt_set_error("%s: workspace of %zu bytes needed (16-byte aligned), got %zu at %p", fn, need, workspace_bytes,
                     workspace);
        return QT_ERR_WORKSPACE;
    }
    float4* rec_p = (float4*)workspace;
    float4* rec_q = rec_p + (size_t)M * tiles_n;
    float* tgt_p = (float*)(rec_q + (size_t)M * tiles_n);
    float* tgt_q = tgt_p + M;
    KlArgs a{(const char*)Hp, (const char*)Hq, (const char*)W, targets, rec_p, rec_q, tgt_p, tgt_q, M, ldhp, ldhq, ldw,
             V, K, target_bytes == 8};
    if (dtype == QT_F16)
        hipLaunchKernelGGL(lm_head_kl_kernel<true>, dim3((unsigned)tiles), dim3(NTHREADS), 0, stream, a);
    else
        hipLaunchKernelGGL(lm_head_kl_kernel<false>, dim3((unsigned)tiles), dim3(NTHREADS), 0, stream, a);
    QT_LAUNCH_CHECK();
    const KlOut out{kl, nll_p, nll_q, lse_p, lse_q, argmax_p, argmax_q};
    hipLaunchKernelGGL(lm_head_kl_reduce_kernel, dim3((unsigned)((M + RED_THREADS - 1) / RED_THREADS)),
                       dim3(RED_THREADS), 0, stream, rec_p, rec_q, tgt_p, tgt_q, targets, a.tgt64, M, V, tiles_n, out);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
