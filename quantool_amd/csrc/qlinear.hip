// W8A8 / W4A8 inference path: dynamic per-token int8 activations and an int8 x int8 GEMM with an int32 accumulator on
// the i8 MFMA (v_mfma_i32_32x32x32_i8), for checkpoints this project writes (include/quantool_amd.h, "A8 runtime").
//
// qt_quantize_tokens_i8   one workgroup per row: a min/max pass, then a quantise pass over the same row (L2-resident).
// qt_gemm_i8              128 x 128 output tile per 4-wave workgroup, k-step 128 (= the weight group), register-staged
//                         single LDS buffer (A and B, 144-B rows: 36 KB); each wave owns 64 x 64 = 2 x 2 MFMA tiles.
//                         Packed int4 weights are unpacked to int8 between the global load and the LDS store.
// (decode sizes, 1 <= M <= 16: qlinear_skinny.hip, equal to qt_gemm_i8 to the bit)
// (SiLU(gate) * up fused into the quantiser, qt_act_mul_quantize_i8: act_quant.hip; the quantiser's constants and
//  per-element step, shared with it: i8_quant.h)
//
// Numerics are the header's fixed sequence; -ffp-contract=off (csrc/build.py) keeps every multiply and add its own
// rounding, so a torch restatement of the same steps is equal to the bit.
#include "common.h"
#include "i8_args.h"
#include "i8_quant.h"
#include "i8_unpack.h"

namespace {

constexpr int QT_THREADS = 256;

__device__ __forceinline__ float ld_x(const unsigned short* X, int dtype, size_t idx) {
    return qt_h16_to_f32(X[idx], dtype);
}

__global__ void __launch_bounds__(QT_THREADS) quantize_tokens_kernel(const unsigned short* __restrict__ X, int dtype,
                                                                     int K, int64_t ldx,
                                                                     const int32_t* __restrict__ col_perm, int symmetric,
                                                                     int vec, int8_t* __restrict__ Xq,
                                                                     float* __restrict__ s_x,
                                                                     int32_t* __restrict__ zp_x) {
    __shared__ float red[2][QT_THREADS / 64];
    const int64_t m = blockIdx.x;
    const unsigned short* row = X + m * ldx;
    int8_t* qrow = Xq + m * (int64_t)K;
    const int tid = threadIdx.x;

    float mn = 0.0f, mx = 0.0f;   // min(min_k x, 0), max(max_k x, 0): start from 0
    if (vec) {
        for (int k = tid * 8; k < K; k += QT_THREADS * 8) {
            const uint4 u = *(const uint4*)(row + k);
            const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float a = qt_h16_to_f32((unsigned short)(w[i] & 0xffffu), dtype);
                const float b = qt_h16_to_f32((unsigned short)(w[i] >> 16), dtype);
                mn = fminf(mn, fminf(a, b));
                mx = fmaxf(mx, fmaxf(a, b));
            }
        }
    } else {
        for (int k = tid; k < K; k += QT_THREADS) {
            const float a = ld_x(row, dtype, k);
            mn = fminf(mn, a);
            mx = fmaxf(mx, a);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = mn;
        red[1][tid >> 6] = mx;
    }
    __syncthreads();
    mn = red[0][0];
    mx = red[1][0];
#pragma unroll
    for (int w = 1; w < QT_THREADS / 64; ++w) {
        mn = fminf(mn, red[0][w]);
        mx = fmaxf(mx, red[1][w]);
    }
    float s, zp;
    qt_i8_row_qparams(mn, mx, symmetric, s, zp);   // i8_quant.h: the divisor's one home
    if (tid == 0) {
        s_x[m] = s;
        if (zp_x) zp_x[m] = (int32_t)zp;
    }

    if (vec) {   // no col_perm, K % 8 == 0: 8 elements -> one 8-byte store
        for (int k = tid * 8; k < K; k += QT_THREADS * 8) {
            *(uint2*)(qrow + k) = q_eight(*(const uint4*)(row + k), dtype, s, zp);
        }
    } else {
        for (int k = tid; k < K; k += QT_THREADS) {
            const int src = col_perm ? col_perm[k] : k;
            qrow[k] = (int8_t)q_one(ld_x(row, dtype, src), s, zp);
        }
    }
}

// ---- GEMM ---------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

constexpr int BM = 128, BN = 128, BK = 128;
constexpr int LDS_ROW = BK + 16;            // bytes; 36-dword pitch keeps eight lanes' ds_read_b128 on disjoint banks
constexpr int GROUP_M = 16;                 // m-tiles that walk the n-tiles together (a weight tile is read by 16
                                            // neighbouring workgroups while it is cache-resident)
constexpr int A_CHUNKS = BM * BK / 16 / QT_THREADS;        // 16-byte chunks of the A tile per thread: 4
constexpr int B8_CHUNKS = BN * BK / 16 / QT_THREADS;       // int8 weights: 4
constexpr int B4_CHUNKS = BN * BK / 2 / 16 / QT_THREADS;   // packed int4 weights (64 B per row per k-step): 2

// One 16-byte chunk of a K-contiguous int8 row [k, k + 16), zero beyond K / beyond the matrix.
template <bool VEC>
__device__ __forceinline__ uint4 load_row16(const int8_t* rowp, bool row_ok, int k, int K) {
    if (VEC) {
        if (row_ok && k < K) return *(const uint4*)(rowp + k);
        return make_uint4(0u, 0u, 0u, 0u);
    } else {
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (row_ok) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (k + i < K) w[i >> 2] |= ((unsigned)(uint8_t)rowp[k + i]) << (8 * (i & 3));
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// 4 packed words [w, w + 4) of one weight row (32 columns), zero beyond Kw words / beyond the matrix
template <bool VEC>
__device__ __forceinline__ uint4 load_words4(const int32_t* rowp, bool row_ok, int w, int Kw) {
    if (VEC) {
        if (row_ok && w < Kw) return *(const uint4*)(rowp + w);
        return make_uint4(0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u);   // level 0
    } else {
        unsigned v[4] = {0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u};
        if (row_ok) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (w + i < Kw) v[i] = (unsigned)rowp[w + i];
        }
        return make_uint4(v[0], v[1], v[2], v[3]);
    }
}

struct GemmArgs {
    const int8_t* Xq;
    const void* Wq;
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
    // grouped (MOE) form only: expert e owns rows [offsets[e], offsets[e + 1]) of Y and the e-th weight matrix;
    // A row m (and s_x / zp_x) is read at row_idx[m] when row_idx is given, else at m
    const int32_t* offsets;
    const int32_t* row_idx;
    int E;
};

// INT4: Wq is int32 [N, ceil(K/8)]; else int8 [N, K].  GROUPED: G = ceil(K/128) groups of 128 columns (the epilogue
// runs after every k-step), else one group.  ASYM: zp_x / wsum given.  VEC: 16-byte loads are in bounds and aligned.
// MOE: the grouped form (qt_gemm_i8_grouped): p.M is the routed-row count R and the grid holds ceil(R/BM) + E m-tiles
// per n-tile, an upper bound on sum_e ceil(rows_e / BM); each workgroup finds its expert from p.offsets, surplus
// workgroups exit.  Everything after that lookup is the same tile code.
template <bool INT4, bool GROUPED, bool ASYM, bool VEC, bool MOE>
__global__ void __launch_bounds__(QT_THREADS, 2) gemm_i8_kernel(const GemmArgs p) {
    __shared__ __attribute__((aligned(16))) int8_t lds[(BM + BN) * LDS_ROW + BM * 4];
    int8_t* sA = lds;
    int8_t* sB = lds + BM * LDS_ROW;
    int32_t* sZp = (int32_t*)(lds + (BM + BN) * LDS_ROW);

    // tile order: GROUP_M m-tiles walk the n-tiles together
    const int tiles_n = (p.N + BN - 1) / BN;
    const int64_t tiles_m = (p.M + BM - 1) / BM + (MOE ? p.E : 0);
    const int64_t pid = blockIdx.x;
    const int64_t per_group = (int64_t)GROUP_M * tiles_n;
    const int64_t gid = pid / per_group;
    const int64_t first_m = gid * GROUP_M;
    const int64_t gsize = (tiles_m - first_m) < GROUP_M ? (tiles_m - first_m) : GROUP_M;
    const int64_t in_g = pid % per_group;
    const int64_t tile_m = first_m + in_g % gsize;
    const int tile_n = (int)(in_g / gsize);
    int64_t m0 = tile_m * BM;
    int64_t m_end = p.M;                  // rows [m0, m_end) of this tile's matrix exist
    const int n0 = tile_n * BN;
    const void* Wq = p.Wq;
    const float* s_w = p.s_w;
    const int32_t* wsum = p.wsum;
    if constexpr (MOE) {
        // virtual m-tile tile_m -> (expert, tile within the expert); offsets clamped to [0, R] so a bad table cannot
        // move a write out of Y
        int64_t start = 0;
        int e = -1;
        for (int j = 0; j < p.E; ++j) {
            const int64_t lo = min(max((int64_t)p.offsets[j], (int64_t)0), p.M);
            const int64_t hi = min(max((int64_t)p.offsets[j + 1], lo), p.M);
            const int64_t nt = (hi - lo + BM - 1) / BM;
            if (tile_m < start + nt) {
                e = j;
                m0 = lo + (tile_m - start) * BM;
                m_end = hi;
                break;
            }
            start += nt;
        }
        if (e < 0) return;                // surplus workgroup (uniform: before any barrier)
        const int64_t wrow = INT4 ? (int64_t)((p.K + 7) / 8) : (int64_t)p.K;
        Wq = INT4 ? (const void*)((const int32_t*)p.Wq + (int64_t)e * p.N * wrow)
                  : (const void*)((const int8_t*)p.Wq + (int64_t)e * p.N * wrow);
        s_w = p.s_w + (int64_t)e * p.N * p.G;
        if (wsum) wsum = p.wsum + (int64_t)e * p.N * p.G;
    }
    // the A / s_x / zp_x row of output row m
    auto src_row = [&](int64_t m) -> int64_t { return (MOE && p.row_idx) ? (int64_t)p.row_idx[m] : m; };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = (wave >> 1) * 64;      // wave's 64 x 64 sub-tile
    const int wn = (wave & 1) * 64;
    const int lr = lane & 31;             // A row / B column of this lane's fragment
    const int lh = lane >> 5;             // which 16 bytes of the 32-deep k-step

    if (ASYM) {
        if (tid < BM) sZp[tid] = (m0 + tid < m_end) ? p.zp_x[src_row(m0 + tid)] : 0;
    }

    const int Kw = (p.K + 7) / 8;
    const int nk = (p.K + BK - 1) / BK;

    // staging: A chunk c of thread t is row (c * 256 + t) / 8, bytes 16 * ((c * 256 + t) % 8)
    uint4 ra[A_CHUNKS];
    uint4 rb[INT4 ? B4_CHUNKS : B8_CHUNKS];
    const int8_t* arow[MOE ? A_CHUNKS : 1];   // grouped form: the gathered A rows, looked up once (nullptr: no row)
    if constexpr (MOE) {
#pragma unroll
        for (int c = 0; c < A_CHUNKS; ++c) {
            const int64_t m = m0 + ((c * QT_THREADS + tid) >> 3);
            arow[c] = m < m_end ? p.Xq + src_row(m) * (int64_t)p.K : nullptr;
        }
    }

    auto load_tiles = [&](int kt) {
        const int k0 = kt * BK;
#pragma unroll
        for (int c = 0; c < A_CHUNKS; ++c) {
            const int idx = c * QT_THREADS + tid;
            if constexpr (MOE) {
                ra[c] = load_row16<VEC>(arow[c], arow[c] != nullptr, k0 + 16 * (idx & 7), p.K);
            } else {
                const int r = idx >> 3;
                const int64_t m = m0 + r;
                ra[c] = load_row16<VEC>(p.Xq + m * (int64_t)p.K, m < p.M, k0 + 16 * (idx & 7), p.K);
            }
        }
        if (INT4) {
#pragma unroll
            for (int c = 0; c < B4_CHUNKS; ++c) {
                const int idx = c * QT_THREADS + tid;
                const int r = idx >> 2;            // 4 chunks of 4 words per row
                const int n = n0 + r;
                rb[c] = load_words4<VEC>((const int32_t*)Wq + (int64_t)n * Kw, n < p.N, k0 / 8 + 4 * (idx & 3), Kw);
            }
        } else {
#pragma unroll
            for (int c = 0; c < B8_CHUNKS; ++c) {
                const int idx = c * QT_THREADS + tid;
                const int r = idx >> 3;
                const int n = n0 + r;
                rb[c] = load_row16<VEC>((const int8_t*)Wq + (int64_t)n * p.K, n < p.N, k0 + 16 * (idx & 7), p.K);
            }
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int c = 0; c < A_CHUNKS; ++c) {
            const int idx = c * QT_THREADS + tid;
            *(uint4*)(sA + (idx >> 3) * LDS_ROW + 16 * (idx & 7)) = ra[c];
        }
        if (INT4) {
#pragma unroll
            for (int c = 0; c < B4_CHUNKS; ++c) {
                const int idx = c * QT_THREADS + tid;
                const uint2 a = unpack_int4_word(rb[c].x), b = unpack_int4_word(rb[c].y);
                const uint2 d = unpack_int4_word(rb[c].z), e = unpack_int4_word(rb[c].w);
                int8_t* dst = sB + (idx >> 2) * LDS_ROW + 32 * (idx & 3);
                *(uint4*)dst = make_uint4(a.x, a.y, b.x, b.y);
                *(uint4*)(dst + 16) = make_uint4(d.x, d.y, e.x, e.y);
            }
        } else {
#pragma unroll
            for (int c = 0; c < B8_CHUNKS; ++c) {
                const int idx = c * QT_THREADS + tid;
                *(uint4*)(sB + (idx >> 3) * LDS_ROW + 16 * (idx & 7)) = rb[c];
            }
        }
    };

    i32x16 acc[2][2];
    f32x16 tot[GROUPED ? 2 : 1][GROUPED ? 2 : 1];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (i32x16){};
    if (GROUPED) {
#pragma unroll
        for (int i = 0; i < (GROUPED ? 2 : 1); ++i)
#pragma unroll
            for (int j = 0; j < (GROUPED ? 2 : 1); ++j) tot[i][j] = (f32x16){};
    }

    // the lane's output columns (C/D map of the 32x32 MFMA: column = lane & 31; row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
    int ncol[2];
    bool nok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ncol[j] = n0 + wn + 32 * j + lr;
        nok[j] = ncol[j] < p.N;
    }

    // t_g = (float)(acc_g - zp_x[m] * wsum[n, g]);  the group's weight scale applied by the caller.  zoff is an
    // opaque 0: it keeps the 32 row zero-points of a lane in LDS, re-read per group, instead of letting the compiler
    // hoist them into registers out of the k-loop (which spills the grouped asymmetric form).
    auto group_term = [&](int i, int j, int r, int ws, int zoff) -> float {
        int a = acc[i][j][r];
        if (ASYM) {
            const int row = wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
            a = a - sZp[row + zoff] * ws;
        }
        return (float)a;
    };
    auto wsum_at = [&](int j, int g) -> int { return (ASYM && nok[j]) ? wsum[(int64_t)ncol[j] * p.G + g] : 0; };

    load_tiles(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();             // previous k-step's fragment reads are done
        store_tiles();
        __syncthreads();
        if (kt + 1 < nk) load_tiles(kt + 1);   // in flight during this k-step's MFMAs
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            i32x4 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                fa[i] = *(const i32x4*)(sA + (wm + 32 * i + lr) * LDS_ROW + 32 * ks + 16 * lh);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                fb[j] = *(const i32x4*)(sB + (wn + 32 * j + lr) * LDS_ROW + 32 * ks + 16 * lh);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (GROUPED) {   // tot += s_w[n, g] * t_g, ascending g
            int zoff = 0;
            if (ASYM) asm volatile("" : "+v"(zoff));
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float sw = nok[j] ? s_w[(int64_t)ncol[j] * p.G + kt] : 0.0f;
                const int ws = wsum_at(j, kt);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float t = group_term(i, j, r, ws, zoff);
                        const float prod = sw * t;
                        tot[i][j][r] = tot[i][j][r] + prod;
                    }
                    acc[i][j] = (i32x16){};
                }
            }
        }
    }

    // y = s_x[m] * tot (+ bias[n]), one rounding to the output dtype
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!nok[j]) continue;
        const int n = ncol[j];
        float bn = 0.0f;
        if (p.bias) bn = qt_load_w(p.bias, p.out_dtype, n);
        const float sw0 = GROUPED ? 0.0f : s_w[(int64_t)n * p.G];
        const int ws0 = GROUPED ? 0 : wsum_at(j, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m >= m_end) continue;
                float tv;
                if (GROUPED) {
                    tv = tot[i][j][r];
                } else {
                    const float prod = sw0 * group_term(i, j, r, ws0, 0);
                    tv = 0.0f + prod;
                }
                float y = p.s_x[src_row(m)] * tv;
                if (p.bias) y = y + bn;
                qt_store_w(p.Y, p.out_dtype, (size_t)(m * p.ldy + n), y);
            }
        }
    }
}

template <bool INT4, bool GROUPED, bool ASYM, bool MOE>
void launch_vec(bool vec, dim3 grid, hipStream_t stream, const GemmArgs& a) {
    if (vec) hipLaunchKernelGGL((gemm_i8_kernel<INT4, GROUPED, ASYM, true, MOE>), grid, dim3(QT_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((gemm_i8_kernel<INT4, GROUPED, ASYM, false, MOE>), grid, dim3(QT_THREADS), 0, stream, a);
}
template <bool INT4, bool GROUPED, bool MOE>
void launch_asym(bool asym, bool vec, dim3 grid, hipStream_t stream, const GemmArgs& a) {
    if (asym) launch_vec<INT4, GROUPED, true, MOE>(vec, grid, stream, a);
    else launch_vec<INT4, GROUPED, false, MOE>(vec, grid, stream, a);
}
template <bool MOE>
void launch_gemm(bool int4, bool grouped, bool asym, bool vec, dim3 grid, hipStream_t stream, const GemmArgs& a) {
    if (int4) {
        if (grouped) launch_asym<true, true, MOE>(asym, vec, grid, stream, a);
        else launch_asym<true, false, MOE>(asym, vec, grid, stream, a);
    } else {
        if (grouped) launch_asym<false, true, MOE>(asym, vec, grid, stream, a);
        else launch_asym<false, false, MOE>(asym, vec, grid, stream, a);
    }
}

}  // namespace

extern "C" int qt_quantize_tokens_i8(const void* X, int x_dtype, int64_t M, int K, int64_t ldx, const int32_t* col_perm,
                                     int symmetric, int8_t* Xq, float* s_x, int32_t* zp_x, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(X && Xq && s_x && M > 0 && K > 0 && ldx >= K, "qt_quantize_tokens_i8: bad arguments");
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "qt_quantize_tokens_i8: x_dtype %d must be bf16 or fp16", x_dtype);
    QT_CHECK_ARG(symmetric || zp_x, "qt_quantize_tokens_i8: asymmetric activations need zp_x");
    QT_CHECK_ARG(M <= 0x7fffffffLL, "qt_quantize_tokens_i8: M %lld too large", (long long)M);
    const int vec = !col_perm && K % 8 == 0 && ldx % 8 == 0 && ((uintptr_t)X & 15) == 0;
    hipLaunchKernelGGL(quantize_tokens_kernel, dim3((unsigned)M), dim3(QT_THREADS), 0, stream,
                       (const unsigned short*)X, x_dtype, K, ldx, col_perm, symmetric, vec, Xq, s_x,
                       symmetric ? nullptr : zp_x);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_gemm_i8(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N, const float* s_x,
                          const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias, void* Y,
                          int out_dtype, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int st = qt_i8_check_dense("qt_gemm_i8", Xq, M, K, Wq, w_format, N, s_x, zp_x, s_w, G, wsum, Y, out_dtype, ldy))
        return st;
    const int64_t tiles = ((M + BM - 1) / BM) * (int64_t)((N + BN - 1) / BN);
    QT_CHECK_ARG(tiles <= 0x7fffffffLL, "qt_gemm_i8: too many tiles");
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const bool grouped = G > 1;
    const bool asym = zp_x != nullptr;
    const bool vec = (((uintptr_t)Xq | (uintptr_t)Wq) & 15) == 0 && K % 16 == 0 && (!int4 || ((K + 7) / 8) % 4 == 0);
    GemmArgs a{Xq, Wq, s_x, zp_x, s_w, wsum, bias, Y, M, N, K, G, ldy, out_dtype, nullptr, nullptr, 0};
    launch_gemm<false>(int4, grouped, asym, vec, dim3((unsigned)tiles), stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_gemm_i8_grouped(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R, const int32_t* offsets,
                                  int E, const void* Wq, int w_format, int N, const float* s_x, const int32_t* zp_x,
                                  const float* s_w, int G, const int32_t* wsum, void* Y, int out_dtype, int64_t ldy,
                                  qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int st = qt_i8_check_grouped("qt_gemm_i8_grouped", Xq, K, R, offsets, E, Wq, w_format, N, s_x, zp_x, s_w, G, wsum,
                                     Y, out_dtype, ldy))
        return st;
    const int64_t tiles = ((R + BM - 1) / BM + E) * (int64_t)((N + BN - 1) / BN);
    QT_CHECK_ARG(tiles <= 0x7fffffffLL, "qt_gemm_i8_grouped: too many tiles");
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const int64_t wrow_bytes = int4 ? (int64_t)((K + 7) / 8) * 4 : (int64_t)K;
    // 16-byte loads need every expert's matrix aligned as well as the base
    const bool vec = (((uintptr_t)Xq | (uintptr_t)Wq) & 15) == 0 && K % 16 == 0 && (!int4 || ((K + 7) / 8) % 4 == 0) &&
                     ((int64_t)N * wrow_bytes) % 16 == 0;
    GemmArgs a{Xq, Wq, s_x, zp_x, s_w, wsum, nullptr, Y, R, N, K, G, ldy, out_dtype, offsets, row_idx, E};
    launch_gemm<true>(int4, G > 1, zp_x != nullptr, vec, dim3((unsigned)tiles), stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
