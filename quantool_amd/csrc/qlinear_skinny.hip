// W8A8 / W4A8 decode path: qt_gemm_i8 and qt_gemm_i8_grouped for 1 <= M <= 16 rows, equal to them to the bit
// (include/quantool_amd.h, "A8 runtime").
//
// qt_gemm_i8_skinny          A workgroup owns 16 output columns n (weight rows) and splits K over its 4 waves: k-block
//                            kb of 128 columns (= the weight group) goes to wave kb % 4.  Per k-block a lane loads 32
//                            bytes of its weight row (16 for packed int4, unpacked in registers) straight into VGPRs,
//                            non-temporal (the weights are read once), and the same 32 columns of its activation row;
//                            two v_mfma_i32_16x16x64_i8 give the group's int32 sums, M padded to 16 with zero rows
//                            (the weights are the A operand).  The next batch of 4 k-blocks per wave is in flight
//                            while the current one is multiplied.
// qt_gemm_i8_skinny_grouped  the same kernel over E weight matrices (MOE = true): grid (column tiles, slots), one slot
//                            per 16-row tile of one expert's rows; a workgroup finds its (expert, tile) by walking
//                            offsets and a surplus one returns before its first weight load and its barrier.
//
// Bit equality with the tiled kernel rests on the header's sequence being integer up to t_g: a group's int32 sum does not
// depend on who adds it.  The fp32 chain over g does, and with K split as kb % 4 no wave owns consecutive groups, so no
// wave sums in fp32: every wave leaves its groups' int32 sums in an LDS slab [group of the batch][256 elements], one
// barrier per batch of 16 groups follows, and thread t folds output element t over the batch in ascending g, carrying
// tot from batch to batch.  The slab is double-buffered, so the one barrier also orders its reuse.  With G = 1 the
// four waves' int32 partials of the whole row are added and the epilogue runs once.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own.
#include "common.h"
#include "i8_args.h"
#include "i8_unpack.h"

namespace {

constexpr int SK_THREADS = 256;
constexpr int SK_WAVES = SK_THREADS / 64;
constexpr int SK_KB = 128;                          // columns per k-block (= the weight group)
constexpr int SK_UNROLL = 4;                        // k-blocks per wave per batch
constexpr int SK_BATCH = SK_WAVES * SK_UNROLL;      // groups per batch (one barrier each)
constexpr int SK_MAX_M = 16;

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct SkinnyArgs {
    const int8_t* Xq;
    const void* Wq;
    const float* s_x;
    const int32_t* zp_x;
    const float* s_w;
    const int32_t* wsum;
    const void* bias;
    void* Y;
    int M;                      // rows (GEMV), or the routed-row count R (grouped form)
    int N, K, Kw, G;            // Kw: int32 words per packed row (int4)
    int64_t ldy;
    int out_dtype;
    // grouped form only: expert e owns output rows [offsets[e], offsets[e + 1]) and weight matrix e; the Xq / s_x / zp_x
    // row of output row m is row_idx[m] (or m when NULL)
    const int32_t* offsets;
    const int32_t* row_idx;
    int E;
};

// 16 bytes [k, k + 16) of a K-contiguous int8 row, zero beyond K.  NT: a once-read weight chunk (non-temporal).
template <bool VEC, bool NT>
__device__ __forceinline__ u32x4 sk_load16(const int8_t* rowp, int k, int K) {
    if constexpr (VEC) {
        if (k >= K) return (u32x4){0u, 0u, 0u, 0u};
        if constexpr (NT) return __builtin_nontemporal_load((const u32x4*)(rowp + k));
        else return *(const u32x4*)(rowp + k);
    } else {
        u32x4 w = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (k + i < K) w[i >> 2] |= ((unsigned)(uint8_t)rowp[k + i]) << (8 * (i & 3));
        return w;
    }
}

// 4 packed words [w, w + 4) of a weight row (32 columns), level 0 beyond Kw words
template <bool VEC>
__device__ __forceinline__ u32x4 sk_load_words4(const int32_t* rowp, int w, int Kw) {
    if constexpr (VEC) {
        if (w >= Kw) return (u32x4){0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u};
        return __builtin_nontemporal_load((const u32x4*)(rowp + w));
    } else {
        u32x4 v = {0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (w + i < Kw) v[i] = (unsigned)rowp[w + i];
        return v;
    }
}

// One k-block of a lane: its weight row's and its activation row's columns [128 kb + 32 kq, + 32) as the A and B
// fragments of two MFMAs.  Both operands take the same bytes in the same order, so the sum over k is the dot product
// whatever order the instruction gives the 64 k of a step.
// The weights stay as loaded (packed int4: one 16-byte chunk) until the MFMAs, so a batch in flight costs the
// registers of what was loaded.
template <bool INT4>
struct SkFrag {
    u32x4 w[INT4 ? 1 : 2];
    i32x4 b[2];
};

// INT4: Wq is int32 [N, ceil(K/8)]; else int8 [N, K].  GROUPED: G = ceil(K/128), the fold runs per batch; else one group.
// VEC: 16-byte loads are in bounds and aligned.  MOE: the grouped-by-expert form; blockIdx.y is a slot.
template <bool INT4, bool GROUPED, bool VEC, bool MOE>
__global__ void __launch_bounds__(SK_THREADS) gemm_i8_skinny_kernel(const SkinnyArgs p) {
    constexpr int SLABS = GROUPED ? 2 : 1;
    constexpr int SLAB_ROWS = GROUPED ? SK_BATCH : SK_WAVES;
    __shared__ __attribute__((aligned(16))) int32_t slab[SLABS][SLAB_ROWS][SK_THREADS];

    int64_t m0 = 0;                     // output row of activation row 0 of the tile
    int Mt = p.M;                       // live rows of the tile
    const void* Wq = p.Wq;
    const float* s_w = p.s_w;
    const int32_t* wsum = p.wsum;
    if constexpr (MOE) {
        // slot -> (expert, 16-row tile); offsets clamped to [0, R] so a bad table cannot move a write out of Y
        const int64_t slot = blockIdx.y;
        int64_t start = 0, hi = 0;
        int e = -1;
        for (int j = 0; j < p.E; ++j) {
            const int64_t lo = min(max((int64_t)p.offsets[j], (int64_t)0), (int64_t)p.M);
            hi = min(max((int64_t)p.offsets[j + 1], lo), (int64_t)p.M);
            const int64_t nt = (hi - lo + SK_MAX_M - 1) / SK_MAX_M;
            if (slot < start + nt) {
                e = j;
                m0 = lo + (slot - start) * SK_MAX_M;
                break;
            }
            start += nt;
        }
        if (e < 0) return;              // surplus slot (uniform: before any load of the weights and any barrier)
        Mt = (int)min(hi - m0, (int64_t)SK_MAX_M);
        const int64_t wrow = INT4 ? (int64_t)p.Kw : (int64_t)p.K;
        Wq = INT4 ? (const void*)((const int32_t*)p.Wq + (int64_t)e * p.N * wrow)
                  : (const void*)((const int8_t*)p.Wq + (int64_t)e * p.N * wrow);
        s_w = p.s_w + (int64_t)e * p.N * p.G;
        if (wsum) wsum = p.wsum + (int64_t)e * p.N * p.G;
    }
    // the Xq / s_x / zp_x row of output row m
    auto src_row = [&](int64_t m) -> int64_t { return (MOE && p.row_idx) ? (int64_t)p.row_idx[m] : m; };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int r = lane & 15;            // A row (weight row n0 + r) and B column (activation row r of the tile)
    const int kq = lane >> 4;           // which 32 columns of the k-block
    const int n0 = blockIdx.x * 16;
    const int64_t nrow = min(n0 + r, p.N - 1);          // a padding row reads row N - 1: in bounds, never stored
    const bool m_ok = r < Mt;
    const int8_t* xrow = p.Xq + (m_ok ? src_row(m0 + r) : (int64_t)0) * p.K;
    const int8_t* wrow8 = (const int8_t*)Wq + nrow * p.K;
    const int32_t* wrow4 = (const int32_t*)Wq + nrow * p.Kw;
    const int nkb = (p.K + SK_KB - 1) / SK_KB;
    const int nbatch = (nkb + SK_BATCH - 1) / SK_BATCH;

    // the output element this thread folds: element 4 lane' + i of the waves' accumulators, lane' = tid >> 2, i = tid & 3,
    // i.e. D[row 4 (lane' >> 4) + i][column lane' & 15] = weight row n0 + 4 (tid >> 6) + i, activation row (tid >> 2) & 15
    const int fm = (tid >> 2) & 15;
    const int fn = n0 + 4 * (tid >> 6) + (tid & 3);
    const bool f_ok = fm < Mt && fn < p.N;
    const int64_t fnc = min(fn, p.N - 1);
    const bool asym = p.zp_x != nullptr;
    const int64_t fsrc = f_ok ? src_row(m0 + fm) : (int64_t)0;
    const int zp = (asym && f_ok) ? p.zp_x[fsrc] : 0;

    typedef SkFrag<INT4> Frag;
    auto load_kb = [&](int kb, Frag& f) {
        const int c0 = kb * SK_KB + 32 * kq;
        f.b[0] = f.b[1] = (i32x4){0, 0, 0, 0};
        if (kb < nkb) {                 // uniform per wave
            if constexpr (INT4) {
                f.w[0] = sk_load_words4<VEC>(wrow4, c0 >> 3, p.Kw);
            } else {
                f.w[0] = sk_load16<VEC, true>(wrow8, c0, p.K);
                f.w[1] = sk_load16<VEC, true>(wrow8, c0 + 16, p.K);
            }
            if (m_ok) {
                f.b[0] = __builtin_bit_cast(i32x4, sk_load16<VEC, false>(xrow, c0, p.K));
                f.b[1] = __builtin_bit_cast(i32x4, sk_load16<VEC, false>(xrow, c0 + 16, p.K));
            }
        } else {                        // past the last k-block: the activations are zero, the weights anything
#pragma unroll
            for (int i = 0; i < (INT4 ? 1 : 2); ++i) f.w[i] = (u32x4){0u, 0u, 0u, 0u};
        }
    };
    auto load_batch = [&](int b, Frag (&f)[SK_UNROLL]) {
#pragma unroll
        for (int u = 0; u < SK_UNROLL; ++u) load_kb(b * SK_BATCH + u * SK_WAVES + wave, f[u]);
    };
    // s_w / wsum of this thread's column for the batch's groups (grouped form): fetched with the batch's weights, so
    // they have landed when the fold needs them
    auto load_scales = [&](int b, float (&sw)[SK_BATCH], int (&ws)[SK_BATCH]) {
#pragma unroll
        for (int gi = 0; gi < SK_BATCH; ++gi) {
            const int g = min(b * SK_BATCH + gi, p.G - 1);
            sw[gi] = s_w[fnc * p.G + g];
            ws[gi] = asym ? wsum[fnc * p.G + g] : 0;
        }
    };
    auto mfma2 = [&](const Frag& f, i32x4 acc) -> i32x4 {
        i32x4 a0, a1;
        if constexpr (INT4) {           // word j of the chunk = columns [8 j, 8 j + 8) of the lane's 32
            const uint2 u0 = unpack_int4_word(f.w[0][0]), u1 = unpack_int4_word(f.w[0][1]);
            const uint2 u2 = unpack_int4_word(f.w[0][2]), u3 = unpack_int4_word(f.w[0][3]);
            a0 = (i32x4){(int)u0.x, (int)u0.y, (int)u1.x, (int)u1.y};
            a1 = (i32x4){(int)u2.x, (int)u2.y, (int)u3.x, (int)u3.y};
        } else {
            a0 = __builtin_bit_cast(i32x4, f.w[0]);
            a1 = __builtin_bit_cast(i32x4, f.w[INT4 ? 0 : 1]);
        }
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, f.b[0], acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, f.b[1], acc, 0, 0, 0);
    };

    Frag cur[SK_UNROLL], nxt[SK_UNROLL];
    float tv;
    if constexpr (GROUPED) {
        float swc[SK_BATCH], swn[SK_BATCH];
        int wsc[SK_BATCH], wsn[SK_BATCH];
        load_scales(0, swc, wsc);
        load_batch(0, cur);
        float tot = 0.0f;
        for (int b = 0; b < nbatch; ++b) {
            if (b + 1 < nbatch) {
                load_scales(b + 1, swn, wsn);
                load_batch(b + 1, nxt);
            }
            int32_t(*sl)[SK_THREADS] = slab[b & 1];
#pragma unroll
            for (int u = 0; u < SK_UNROLL; ++u)
                *(i32x4*)&sl[u * SK_WAVES + wave][4 * lane] = mfma2(cur[u], (i32x4){0, 0, 0, 0});
            __syncthreads();
            // tot += s_w[n, g] * t_g, ascending g.  The other buffer is written next; the next barrier orders its reuse.
#pragma unroll
            for (int gi = 0; gi < SK_BATCH; ++gi) {
                if (b * SK_BATCH + gi < nkb) {
                    const int a = sl[gi][tid] - zp * wsc[gi];
                    const float t = (float)a;
                    const float prod = swc[gi] * t;
                    tot = tot + prod;
                }
            }
#pragma unroll
            for (int u = 0; u < SK_UNROLL; ++u) cur[u] = nxt[u];
#pragma unroll
            for (int gi = 0; gi < SK_BATCH; ++gi) {
                swc[gi] = swn[gi];
                wsc[gi] = wsn[gi];
            }
        }
        tv = tot;
    } else {
        i32x4 acc = {0, 0, 0, 0};
        load_batch(0, cur);
        for (int b = 0; b < nbatch; ++b) {
            if (b + 1 < nbatch) load_batch(b + 1, nxt);
#pragma unroll
            for (int u = 0; u < SK_UNROLL; ++u) acc = mfma2(cur[u], acc);
#pragma unroll
            for (int u = 0; u < SK_UNROLL; ++u) cur[u] = nxt[u];
        }
        *(i32x4*)&slab[0][wave][4 * lane] = acc;
        __syncthreads();
        int a = slab[0][0][tid];
#pragma unroll
        for (int w = 1; w < SK_WAVES; ++w) a += slab[0][w][tid];
        const int ws0 = asym ? wsum[fnc * p.G] : 0;
        a = a - zp * ws0;
        const float t = (float)a;
        const float prod = s_w[fnc * p.G] * t;
        tv = 0.0f + prod;
    }

    // y = s_x[m] * tot (+ bias[n]), one rounding to the output dtype
    if (f_ok) {
        float y = p.s_x[fsrc] * tv;
        if (p.bias) y = y + qt_load_w(p.bias, p.out_dtype, (size_t)fn);
        qt_store_w(p.Y, p.out_dtype, (size_t)((m0 + fm) * p.ldy + fn), y);
    }
}

template <bool MOE>
void launch_skinny(bool int4, bool grouped, bool vec, dim3 grid, hipStream_t stream, const SkinnyArgs& a) {
#define QT_SK_CASE(I4, GR, V) \
    if (int4 == I4 && grouped == GR && vec == V) \
        hipLaunchKernelGGL((gemm_i8_skinny_kernel<I4, GR, V, MOE>), grid, dim3(SK_THREADS), 0, stream, a);
    QT_SK_CASE(false, false, false) QT_SK_CASE(false, false, true) QT_SK_CASE(false, true, false)
    QT_SK_CASE(false, true, true) QT_SK_CASE(true, false, false) QT_SK_CASE(true, false, true)
    QT_SK_CASE(true, true, false) QT_SK_CASE(true, true, true)
#undef QT_SK_CASE
}

}  // namespace

extern "C" int qt_gemm_i8_skinny(const int8_t* Xq, int M, int K, const void* Wq, int w_format, int N, const float* s_x,
                                 const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias,
                                 void* Y, int out_dtype, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(M >= 1 && M <= SK_MAX_M, "qt_gemm_i8_skinny: M %d outside 1 .. %d", M, SK_MAX_M);
    if (int st = qt_i8_check_dense("qt_gemm_i8_skinny", Xq, M, K, Wq, w_format, N, s_x, zp_x, s_w, G, wsum, Y, out_dtype,
                                   ldy))
        return st;
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const bool vec = (((uintptr_t)Xq | (uintptr_t)Wq) & 15) == 0 && K % 16 == 0 && (!int4 || ((K + 7) / 8) % 4 == 0);
    SkinnyArgs a{Xq, Wq, s_x, zp_x, s_w, wsum, bias, Y, M, N, K, (K + 7) / 8, G, ldy, out_dtype, nullptr, nullptr, 0};
    launch_skinny<false>(int4, G > 1, vec, dim3((unsigned)((N + 15) / 16)), stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_gemm_i8_skinny_grouped(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R,
                                         const int32_t* offsets, int E, const void* Wq, int w_format, int N,
                                         const float* s_x, const int32_t* zp_x, const float* s_w, int G,
                                         const int32_t* wsum, void* Y, int out_dtype, int64_t ldy,
                                         qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int st = qt_i8_check_grouped("qt_gemm_i8_skinny_grouped", Xq, K, R, offsets, E, Wq, w_format, N, s_x, zp_x, s_w, G,
                                     wsum, Y, out_dtype, ldy))
        return st;
    const int64_t slots = R / SK_MAX_M + (E < R ? E : R);
    QT_CHECK_ARG(slots <= 65535, "qt_gemm_i8_skinny_grouped: %lld row-tile slots (R = %lld) exceed the grid",
                 (long long)slots, (long long)R);
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const int64_t wrow_bytes = int4 ? (int64_t)((K + 7) / 8) * 4 : (int64_t)K;
    // 16-byte loads need every expert's matrix aligned as well as the base
    const bool vec = (((uintptr_t)Xq | (uintptr_t)Wq) & 15) == 0 && K % 16 == 0 && (!int4 || ((K + 7) / 8) % 4 == 0) &&
                     ((int64_t)N * wrow_bytes) % 16 == 0;
    SkinnyArgs a{Xq, Wq, s_x, zp_x, s_w, wsum, nullptr, Y, (int)R, N, K, (K + 7) / 8, G, ldy, out_dtype, offsets,
                 row_idx, E};
    launch_skinny<true>(int4, G > 1, vec, dim3((unsigned)((N + 15) / 16), (unsigned)slots), stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
