// W8A8 / W4A8 mid-M path: qt_gemm_i8 for 1 <= M <= 128 rows, equal to it to the bit
// (include/quantool_amd.h, "A8 runtime").
//
// qt_gemm_i8_mid  qlinear_skinny.hip's tile widened in M.  A workgroup owns 16 output columns n (weight rows) and all M
//                 rows, and splits K over its 4 waves: k-block kb of 128 columns (= the weight group) goes to wave
//                 kb % 4.  Per k-block a lane loads 32 bytes of its weight row (16 for packed int4, unpacked in
//                 registers once per k-block) straight into VGPRs, non-temporal (the weights are read once), and for each
//                 of the ceil(M/16) live m-tiles the same 32 columns of its activation row (plain loads: X is small and
//                 stays in L2); two v_mfma_i32_16x16x64_i8 per m-tile give that tile's int32 sums (the weights are the A
//                 operand, 16 activation rows the B operand).  MT = 2 / 4 / 8 m-tiles are compiled; tiles past
//                 ceil(M/16) are skipped (uniform branches), rows past M inside a live tile are zero in registers.  The
//                 next batch of weights is in flight while the current one is multiplied.
//
// Bit equality with the tiled kernel rests on the header's sequence being integer up to t_g: a group's int32 sum does not
// depend on who adds it.  The fp32 chain over g does, and with K split as kb % 4 no wave owns consecutive groups, so no
// wave sums in fp32: every wave leaves its groups' int32 sums in an LDS slab [group of the batch][m-tile][256 elements],
// a barrier follows, thread t folds element t of every live m-tile over the batch in ascending g, carrying tot from
// batch to batch, and a second barrier frees the slab (one buffer: at 8 m-tiles a batch of 8 groups is 64 KiB).  With
// G = 1 the four waves' int32 partials of the whole row meet in LDS once and the epilogue runs once per element.
//
// K is a multiple of 128 and both operands are 16-byte aligned (checked on the host), so every load is a whole, aligned
// 16-byte chunk inside its row; a weight row past N re-reads row N - 1 and is never stored.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own.
#include "common.h"
#include "i8_args.h"
#include "i8_unpack.h"
#pragma clang fp contract(off)

namespace {

constexpr int MID_THREADS = 256;
constexpr int MID_WAVES = MID_THREADS / 64;
constexpr int MID_KB = QT_I8_MID_K_UNIT;            // columns per k-block (= the weight group)
constexpr int MID_COLS = 16;                        // output columns per workgroup
constexpr int MID_MAX_M = QT_I8_MID_MAX_M;

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
    int M, N, K, Kw, G;         // Kw = K / 8: int32 words per packed row (int4)
    int64_t ldy;
    int out_dtype;
};

template <bool INT4>
struct MidW {
    u32x4 w[INT4 ? 1 : 2];
};

// MT: m-tiles of 16 rows held (M <= 16 MT).  INT4: Wq is int32 [N, K/8]; else int8 [N, K].
// GROUPED: G = K/128, the fold runs per batch; else one group.
template <int MT, bool INT4, bool GROUPED>
__global__ void __launch_bounds__(MID_THREADS) gemm_i8_mid_kernel(const MidArgs p) {
    constexpr int U = mid_unroll(MT);
    constexpr int BATCH = MID_WAVES * U;            // groups per batch
    constexpr int SLAB_ROWS = GROUPED ? BATCH : MID_WAVES;
    __shared__ __attribute__((aligned(16))) int32_t slab[SLAB_ROWS][MT][MID_THREADS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r = lane & 15;            // A row (weight row n0 + r) and B column (activation row 16 t + r)
    const int kq = lane >> 4;           // which 32 columns of the k-block
    const int n0 = blockIdx.x * MID_COLS;
    const int nt = (p.M + 15) >> 4;     // live m-tiles, <= MT
    const int64_t nrow = min(n0 + r, p.N - 1);          // a padding row reads row N - 1: in bounds, never stored
    const int8_t* wrow8 = (const int8_t*)p.Wq + nrow * p.K;
    const int32_t* wrow4 = (const int32_t*)p.Wq + nrow * p.Kw;
    const int8_t* xbase = p.Xq + (int64_t)r * p.K + 32 * kq;        // row r of tile 0 (M >= 1: row 0 exists)
    const int nkb = p.K / MID_KB;
    const int nbatch = (nkb + BATCH - 1) / BATCH;

    // the output elements this thread folds: element 4 lane' + i of a wave's accumulator of m-tile t, lane' = tid >> 2,
    // i = tid & 3, i.e. D[row 4 (lane' >> 4) + i][column lane' & 15] = weight row n0 + 4 (tid >> 6) + i, activation row
    // 16 t + ((tid >> 2) & 15)
    const int fm = (tid >> 2) & 15;
    const int fn = n0 + 4 * (tid >> 6) + (tid & 3);
    const int64_t fnc = min(fn, p.N - 1);
    const bool asym = p.zp_x != nullptr;

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
    // the lane's 32 activation bytes of every live m-tile for the batch's k-blocks; zero for a row past M
    auto load_x = [&](int b, i32x4 (&x)[U][MT][2]) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kb = b * BATCH + u * MID_WAVES + wave;
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                x[u][t][0] = x[u][t][1] = (i32x4){0, 0, 0, 0};
                if (kb < nkb && 16 * t + r < p.M) {
                    const int8_t* xp = xbase + (int64_t)(16 * t) * p.K + kb * MID_KB;
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
        for (int t = 0; t < MT; ++t) zp[t] = (asym && 16 * t + fm < p.M) ? p.zp_x[16 * t + fm] : 0;
        load_w(0, cur);
        for (int b = 0; b < nbatch; ++b) {
            if (b + 1 < nbatch) load_w(b + 1, nxt);
            // s_w / wsum of this thread's column for the batch's groups: fetched before the activations, so they have
            // landed when the fold needs them
            float sw[BATCH];
            int ws[BATCH];
#pragma unroll
            for (int gi = 0; gi < BATCH; ++gi) {
                const int g = min(b * BATCH + gi, p.G - 1);
                sw[gi] = p.s_w[fnc * p.G + g];
                ws[gi] = asym ? p.wsum[fnc * p.G + g] : 0;
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
        const int ws0 = asym ? p.wsum[fnc * p.G] : 0;
        const float sw0 = p.s_w[fnc * p.G];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            if (t < nt) {
                int a = slab[0][t][tid];
#pragma unroll
                for (int w = 1; w < MID_WAVES; ++w) a += slab[w][t][tid];
                const int zp = (asym && 16 * t + fm < p.M) ? p.zp_x[16 * t + fm] : 0;
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
            if (m < p.M) {
                float y = p.s_x[m] * tv[t];
                if (p.bias) y = y + bv;
                qt_store_w(p.Y, p.out_dtype, (size_t)((int64_t)m * p.ldy + fn), y);
            }
        }
    }
}

template <int MT>
void launch_mid(bool int4, bool grouped, dim3 grid, hipStream_t stream, const MidArgs& a) {
#define QT_MID_CASE(I4, GR) \
    if (int4 == I4 && grouped == GR) \
        hipLaunchKernelGGL((gemm_i8_mid_kernel<MT, I4, GR>), grid, dim3(MID_THREADS), 0, stream, a);
    QT_MID_CASE(false, false) QT_MID_CASE(false, true) QT_MID_CASE(true, false) QT_MID_CASE(true, true)
#undef QT_MID_CASE
}

}  // namespace

extern "C" int qt_gemm_i8_mid(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N, const float* s_x,
                              const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias,
                              void* Y, int out_dtype, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(M >= 1 && M <= MID_MAX_M, "qt_gemm_i8_mid: M %lld outside 1 .. %d", (long long)M, MID_MAX_M);
    QT_CHECK_ARG(K % MID_KB == 0, "qt_gemm_i8_mid: K %d is not a multiple of the k-unit %d", K, MID_KB);
    QT_CHECK_ARG(G == 1 || G == K / MID_KB, "qt_gemm_i8_mid: G %d must be 1 or K / 128 = %d", G, K / MID_KB);
    QT_CHECK_ARG((((uintptr_t)Xq | (uintptr_t)Wq) & 15) == 0, "qt_gemm_i8_mid: Xq and Wq must be 16-byte aligned");
    if (int st = qt_i8_check_dense("qt_gemm_i8_mid", Xq, M, K, Wq, w_format, N, s_x, zp_x, s_w, G, wsum, Y, out_dtype, ldy))
        return st;
    const bool int4 = w_format == QT_W_INT4_PACKED;
    MidArgs a{Xq, Wq, s_x, zp_x, s_w, wsum, bias, Y, (int)M, N, K, K / 8, G, ldy, out_dtype};
    const dim3 grid((unsigned)((N + MID_COLS - 1) / MID_COLS));
    if (M <= 32) launch_mid<2>(int4, G > 1, grid, stream, a);
    else if (M <= 64) launch_mid<4>(int4, G > 1, grid, stream, a);
    else launch_mid<8>(int4, G > 1, grid, stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
