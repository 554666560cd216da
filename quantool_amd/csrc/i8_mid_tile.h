// The weight-streaming 16-column int8 tile, stated once for its two kernels: gemm_i8_mid_kernel (qlinear_mid.hip, a
// dense Linear of 1 .. 128 rows) and moe_gemm_i8_wide_kernel (qlinear_moe_wide.hip, the same tile over E weight
// matrices).  include/quantool_amd.h, "A8 runtime" and "Routed experts"; DESIGN.md 4.14 and 4.18.
//
// A workgroup of 256 threads owns 16 output columns n (weight rows) and up to 16 MT rows, and splits K over its 4
// waves: k-block kb of 128 columns (= the weight group) goes to wave kb % 4.  Per k-block a lane loads 32 bytes of its
// weight row (16 for packed int4, unpacked in registers once per k-block) straight into VGPRs, non-temporal (the
// weights are read once), and for each live m-tile the same 32 columns of its activation row (plain loads: X is small
// and stays in L2); two v_mfma_i32_16x16x64_i8 per m-tile give that tile's int32 sums (the weights are the A operand,
// 16 activation rows the B operand).  MT = 2 / 4 / 8 m-tiles are compiled; tiles past the live ones are skipped
// (uniform branches), rows past the last live row are zero in registers.  The next batch of weights is in flight
// while the current one is multiplied.
//
// Bit equality with the tiled kernels rests on the header's sequence being integer up to t_g: a group's int32 sum does
// not depend on who adds it.  The fp32 chain over g does, and with K split as kb % 4 no wave owns consecutive groups,
// so no wave sums in fp32: every wave leaves its groups' int32 sums in an LDS slab [group of the batch][m-tile][256
// elements], a barrier follows, thread t folds element t of every live m-tile over the batch in ascending g, carrying
// tot from batch to batch, and a second barrier frees the slab (one buffer: at 8 m-tiles a batch of 8 groups is
// 64 KiB).  With G = 1 the four waves' int32 partials of the whole row meet in LDS once and the epilogue runs once per
// element.
//
// K is a multiple of 128 and both operands are 16-byte aligned (checked on the host), so every load is a whole, aligned
// 16-byte chunk inside its row; a weight row past N re-reads row N - 1 and is never stored.
//
// MOE = false is the dense form: rows [0, M) of Xq, every `if constexpr (MOE)` below falls away.  MOE = true:
// blockIdx.y is a slot; the workgroup walks offsets (clamped to [0, R] and made ascending) to its expert e and its tile
// of up to 16 MT of e's rows, first row m0, and a surplus slot returns before its first weight load and before any
// barrier (uniform).  Activation row m of the tile is Xq[src(m0 + m)], src = row_idx clamped into [0, x_rows) or the
// identity, addressed as Xq (+ m0 K without row_idx) plus one 32-bit byte offset per m-tile and lane: the host refuses
// x_rows K > 2^32 with row_idx; s_x / zp_x are read at the same index; Wq / s_w / wsum are those of expert e.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own.
#pragma once
#include "common.h"
#include "i8_unpack.h"
#pragma clang fp contract(off)

constexpr int MID_THREADS = 256;
constexpr int MID_WAVES = MID_THREADS / 64;
constexpr int MID_KB = QT_I8_MID_K_UNIT;            // columns per k-block (= the weight group)
constexpr int MID_COLS = 16;                        // output columns per workgroup

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// k-blocks per wave per batch: 16 (k-block, m-tile) activation fragments of a lane are in registers at a time
__host__ __device__ constexpr int mid_unroll(int MT) { return MT <= 4 ? 4 : 2; }

struct MidArgs {
    const int8_t* Xq;
    const void* Wq;
    const float* s_x;
    const int32_t* zp_x;
    const float* s_w;
    const int32_t* wsum;
    const void* bias;
    void* Y;
    int M, N, K, Kw, G;         // M: rows, or the routed-row count R (MOE); Kw = K / 8: int32 words per packed row (int4)
    int64_t ldy;
    int out_dtype;
};

// MOE only: expert e owns output rows [offsets[e], offsets[e + 1]) and weight matrix e; the Xq / s_x / zp_x row of
// output row m is row_idx[m] clamped into [0, x_rows), or m when row_idx is NULL
struct MidMoe {
    const int32_t* offsets;
    const int32_t* row_idx;
    int64_t x_rows;
    int E;
};

template <bool INT4>
struct MidW {
    u32x4 w[INT4 ? 1 : 2];
};

// MT: m-tiles of 16 rows held (live rows <= 16 MT).  INT4: Wq is int32 [N, K/8]; else int8 [N, K].
// GROUPED: G = K/128, the fold runs per batch; else one group.  MOE: the form over E weight matrices.
template <int MT, bool INT4, bool GROUPED, bool MOE>
__device__ __forceinline__ void i8_mid_tile(const MidArgs& p, const MidMoe& g) {
    constexpr int U = mid_unroll(MT);
    constexpr int BATCH = MID_WAVES * U;            // groups per batch
    constexpr int SLAB_ROWS = GROUPED ? BATCH : MID_WAVES;
    __shared__ __attribute__((aligned(16))) int32_t slab[SLAB_ROWS][MT][MID_THREADS];

    int64_t m0 = 0;                     // output row of row 0 of the tile
    int Mt = p.M;                       // live rows of the tile, 1 .. 16 MT
    const void* Wq = p.Wq;
    const float* s_w = p.s_w;
    const int32_t* wsum = p.wsum;
    if constexpr (MOE) {
        // slot -> (expert, tile of 16 MT rows); offsets clamped to [0, R] so a bad table cannot move a write out of Y
        constexpr int64_t TILE = 16 * MT;
        const int64_t slot = blockIdx.y;
        int64_t start = 0, hi = 0;
        int e = -1;
        for (int j = 0; j < g.E; ++j) {
            const int64_t lo = min(max((int64_t)g.offsets[j], (int64_t)0), (int64_t)p.M);
            hi = min(max((int64_t)g.offsets[j + 1], lo), (int64_t)p.M);
            const int64_t nts = (hi - lo + TILE - 1) / TILE;
            if (slot < start + nts) {
                e = j;
                m0 = lo + (slot - start) * TILE;
                break;
            }
            start += nts;
        }
        if (e < 0) return;              // surplus slot (uniform: before any load of the weights and any barrier)
        Mt = (int)min(hi - m0, TILE);
        const int64_t wrow = INT4 ? (int64_t)p.Kw : (int64_t)p.K;
        Wq = INT4 ? (const void*)((const int32_t*)p.Wq + (int64_t)e * p.N * wrow)
                  : (const void*)((const int8_t*)p.Wq + (int64_t)e * p.N * wrow);
        s_w = p.s_w + (int64_t)e * p.N * p.G;
        if (wsum) wsum = p.wsum + (int64_t)e * p.N * p.G;
    }
    // MOE: the Xq / s_x / zp_x row of row m < Mt of the tile
    auto src_row = [&](int m) -> int64_t {
        if (g.row_idx) return min(max((int64_t)g.row_idx[m0 + m], (int64_t)0), g.x_rows - 1);
        return m0 + m;
    };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r = lane & 15;            // A row (weight row n0 + r) and B column (activation row 16 t + r)
    const int kq = lane >> 4;           // which 32 columns of the k-block
    const int n0 = blockIdx.x * MID_COLS;
    const int nt = (Mt + 15) >> 4;      // live m-tiles, <= MT
    const int64_t nrow = min(n0 + r, p.N - 1);          // a padding row reads row N - 1: in bounds, never stored
    const int8_t* wrow8 = (const int8_t*)Wq + nrow * p.K;
    const int32_t* wrow4 = (const int32_t*)Wq + nrow * p.Kw;
    // dense: row r of tile 0 (M >= 1: row 0 exists).  MOE: the base of the 32-bit offsets xoff, Xq itself for gathered
    // rows (offsets < x_rows K <= 2^32), the tile's first row for contiguous ones (offsets < 128 K)
    const int8_t* xbase = MOE ? p.Xq + (g.row_idx ? (int64_t)0 : m0 * p.K)
                              : p.Xq + (int64_t)r * p.K + 32 * kq;
    unsigned xoff[MOE ? MT : 1];        // MOE: byte offset of the lane's 32 columns of k-block 0 in its row of m-tile t
    if constexpr (MOE) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int m = 16 * t + r;
            const int64_t row = m < Mt ? (g.row_idx ? src_row(m) : (int64_t)m) : (int64_t)0;
            xoff[t] = (unsigned)((uint64_t)row * (uint64_t)p.K + (uint64_t)(32 * kq));
        }
    }
    const int nkb = p.K / MID_KB;
    const int nbatch = (nkb + BATCH - 1) / BATCH;

    // the output elements this thread folds: element 4 lane' + i of a wave's accumulator of m-tile t, lane' = tid >> 2,
    // i = tid & 3, i.e. D[row 4 (lane' >> 4) + i][column lane' & 15] = weight row n0 + 4 (tid >> 6) + i, activation row
    // 16 t + ((tid >> 2) & 15)
    const int fm = (tid >> 2) & 15;
    const int fn = n0 + 4 * (tid >> 6) + (tid & 3);
    const int64_t fnc = min(fn, p.N - 1);
    const bool asym = p.zp_x != nullptr;
    // zp_x of row m < Mt of the tile
    auto zp_of = [&](int m) -> int {
        if constexpr (MOE) return p.zp_x[src_row(m)];
        else return p.zp_x[m];
    };

    typedef MidW<INT4> WFrag;
    auto load_w = [&](int b, WFrag (&f)[U]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kb = b * BATCH + u * MID_WAVES + wave;
#pragma unroll
            for (int i = 0; i < (INT4 ? 1 : 2); ++i) f[u].w[i] = (u32x4){0u, 0u, 0u, 0u};
            if (kb < nkb) {             // uniform per wave
                const int c0 = kb * MID_KB + 32 * kq;
                if constexpr (INT4) {
                    f[u].w[0] = __builtin_nontemporal_load((const u32x4*)(wrow4 + (c0 >> 3)));
                } else {
                    f[u].w[0] = __builtin_nontemporal_load((const u32x4*)(wrow8 + c0));
                    f[u].w[1] = __builtin_nontemporal_load((const u32x4*)(wrow8 + c0 + 16));
                }
            }
        }
    };
    // the lane's 32 activation bytes of every live m-tile for the batch's k-blocks; zero for a row past the last
    auto load_x = [&](int b, i32x4 (&x)[U][MT][2]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kb = b * BATCH + u * MID_WAVES + wave;
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                x[u][t][0] = x[u][t][1] = (i32x4){0, 0, 0, 0};
                if (kb < nkb && 16 * t + r < Mt) {
                    const int8_t* xp;
                    if constexpr (MOE) xp = xbase + kb * MID_KB + xoff[t];
                    else xp = xbase + (int64_t)(16 * t) * p.K + kb * MID_KB;
                    x[u][t][0] = *(const i32x4*)xp;
                    x[u][t][1] = *(const i32x4*)(xp + 16);
                }
            }
        }
    };
    auto a_frags = [&](const WFrag& f, i32x4& a0, i32x4& a1) {
        if constexpr (INT4) {           // word j of the chunk = columns [8 j, 8 j + 8) of the lane's 32
            const uint2 u0 = unpack_int4_word(f.w[0][0]), u1 = unpack_int4_word(f.w[0][1]);
            const uint2 u2 = unpack_int4_word(f.w[0][2]), u3 = unpack_int4_word(f.w[0][3]);
            a0 = (i32x4){(int)u0.x, (int)u0.y, (int)u1.x, (int)u1.y};
            a1 = (i32x4){(int)u2.x, (int)u2.y, (int)u3.x, (int)u3.y};
        } else {
            a0 = __builtin_bit_cast(i32x4, f.w[0]);
            a1 = __builtin_bit_cast(i32x4, f.w[INT4 ? 0 : 1]);
        }
    };

    WFrag cur[U], nxt[U];
    i32x4 x[U][MT][2];
    float tv[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) tv[t] = 0.0f;

    if constexpr (GROUPED) {
        int zp[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) zp[t] = (asym && 16 * t + fm < Mt) ? zp_of(16 * t + fm) : 0;
        load_w(0, cur);
        for (int b = 0; b < nbatch; ++b) {
            if (b + 1 < nbatch) load_w(b + 1, nxt);
            // s_w / wsum of this thread's column for the batch's groups: fetched before the activations, so they have
            // landed when the fold needs them
            float sw[BATCH];
            int ws[BATCH];
#pragma unroll
            for (int gi = 0; gi < BATCH; ++gi) {
                const int gr = min(b * BATCH + gi, p.G - 1);
                sw[gi] = s_w[fnc * p.G + gr];
                ws[gi] = asym ? wsum[fnc * p.G + gr] : 0;
            }
            load_x(b, x);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (b * BATCH + u * MID_WAVES + wave < nkb) {
                    i32x4 a0, a1;
                    a_frags(cur[u], a0, a1);
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        if (t < nt) {
                            i32x4 acc = {0, 0, 0, 0};
                            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, x[u][t][0], acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, x[u][t][1], acc, 0, 0, 0);
                            *(i32x4*)&slab[u * MID_WAVES + wave][t][4 * lane] = acc;
                        }
                    }
                }
            }
            __syncthreads();
            // tot += s_w[n, g] * t_g, ascending g
#pragma unroll
            for (int gi = 0; gi < BATCH; ++gi) {
                if (b * BATCH + gi < nkb) {
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        if (t < nt) {
                            const int a = slab[gi][t][tid] - zp[t] * ws[gi];
                            const float tg = (float)a;
                            const float prod = sw[gi] * tg;
                            tv[t] = tv[t] + prod;
                        }
                    }
                }
            }
            __syncthreads();            // the slab is written again by the next batch
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    } else {
        i32x4 acc[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = (i32x4){0, 0, 0, 0};
        load_w(0, cur);
        for (int b = 0; b < nbatch; ++b) {
            if (b + 1 < nbatch) load_w(b + 1, nxt);
            load_x(b, x);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (b * BATCH + u * MID_WAVES + wave < nkb) {
                    i32x4 a0, a1;
                    a_frags(cur[u], a0, a1);
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        if (t < nt) {
                            acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, x[u][t][0], acc[t], 0, 0, 0);
                            acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, x[u][t][1], acc[t], 0, 0, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
#pragma unroll
        for (int t = 0; t < MT; ++t)
            if (t < nt) *(i32x4*)&slab[wave][t][4 * lane] = acc[t];
        __syncthreads();
        const int ws0 = asym ? wsum[fnc * p.G] : 0;
        const float sw0 = s_w[fnc * p.G];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            if (t < nt) {
                int a = slab[0][t][tid];
#pragma unroll
                for (int w = 1; w < MID_WAVES; ++w) a += slab[w][t][tid];
                const int zp = (asym && 16 * t + fm < Mt) ? zp_of(16 * t + fm) : 0;
                a = a - zp * ws0;
                const float tg = (float)a;
                const float prod = sw0 * tg;
                tv[t] = 0.0f + prod;
            }
        }
    }

    // y = s_x[m] * tot (+ bias[n]), one rounding to the output dtype
    if (fn < p.N) {
        const float bv = p.bias ? qt_load_w(p.bias, p.out_dtype, (size_t)fn) : 0.0f;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int m = 16 * t + fm;
            if (m < Mt) {
                float sx;
                if constexpr (MOE) sx = p.s_x[src_row(m)];
                else sx = p.s_x[m];
                float y = sx * tv[t];
                if (p.bias) y = y + bv;
                qt_store_w(p.Y, p.out_dtype, (size_t)((m0 + m) * p.ldy + fn), y);
            }
        }
    }
}
