// Routed-expert plumbing around the grouped int8 GEMM (include/quantool_amd.h, "Routed experts"):
//
// qt_moe_route    one workgroup: per-thread per-expert counts of a contiguous slice of the [T, k] routing table, one
//                 exclusive scan over (expert, thread), then a second pass over the same slice that places every entry.
//                 Integer only, no atomics: the output is a pure function of the table.
// qt_moe_combine  one workgroup per token: the token's routed rows of the down projection, weighted and summed in
//                 ascending row (= ascending expert) order, 8 columns per thread when the rows allow 16-byte access.
#include "common.h"

namespace {

constexpr int ROUTE_CELLS = 8192;   // counters in LDS: E * threads (32 KB)
constexpr int COMBINE_THREADS = 256;
constexpr int MAX_TOPK = 16;

__global__ void __launch_bounds__(256) moe_route_kernel(const void* __restrict__ idx, int idx64, int64_t T, int k,
                                                        int E, int32_t* __restrict__ offsets,
                                                        int32_t* __restrict__ src_token,
                                                        int32_t* __restrict__ src_slot,
                                                        int32_t* __restrict__ row_of) {
    extern __shared__ int cnt[];          // [E][nt]: entries of expert e in thread t's slice, then their first row
    __shared__ int part[256];
    __shared__ int routed;
    const int nt = blockDim.x;
    const int t = threadIdx.x;
    const int64_t n = T * k;
    const int64_t per = (n + nt - 1) / nt;
    const int64_t lo = min((int64_t)t * per, n), hi = min(lo + per, n);
    auto expert_at = [&](int64_t i) -> int64_t {
        return idx64 ? ((const int64_t*)idx)[i] : (int64_t)((const int32_t*)idx)[i];
    };

    for (int c = t; c < E * nt; c += nt) cnt[c] = 0;
    __syncthreads();
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t e = expert_at(i);
        if (e >= 0 && e < E) ++cnt[e * nt + t];   // column t is this thread's alone
    }
    __syncthreads();
    // exclusive scan of cnt in (e, t) order: thread t owns cells [t E, (t + 1) E)
    int s = 0;
    for (int c = t * E; c < (t + 1) * E; ++c) s += cnt[c];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int j = 0; j < nt; ++j) {
            const int v = part[j];
            part[j] = run;
            run += v;
        }
        offsets[E] = run;
        routed = run;
    }
    __syncthreads();
    int run = part[t];
    for (int c = t * E; c < (t + 1) * E; ++c) {
        const int v = cnt[c];
        cnt[c] = run;
        run += v;
    }
    __syncthreads();
    for (int e = t; e < E; e += nt) offsets[e] = cnt[e * nt];
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t e = expert_at(i);
        if (e >= 0 && e < E) {
            const int pos = cnt[e * nt + t]++;
            src_token[pos] = (int32_t)(i / k);
            src_slot[pos] = (int32_t)(i % k);
            if (row_of) row_of[i] = pos;
        } else if (row_of) {
            row_of[i] = -1;
        }
    }
    __syncthreads();
    // rows past the routed ones (dropped entries): zero, so the whole output is defined
    for (int64_t r = routed + t; r < n; r += nt) {
        src_token[r] = 0;
        src_slot[r] = 0;
    }
}

// v is an fp32 result already rounded to fp32; the empty asm keeps it one: without it the compiler folds the multiply or
// add that made v into the 16-bit conversion (v_fma_mixlo_f16: one rounding of the exact result), where torch rounds
// to fp32 first and then to the 16-bit dtype
__device__ __forceinline__ float round_to(float v, int dtype) {
    asm volatile("" : "+v"(v));
    return dtype == QT_F16 ? (float)(_Float16)v : (float)(__bf16)v;
}
__device__ __forceinline__ unsigned short to_bits(float v, int dtype) {
    return dtype == QT_F16 ? __builtin_bit_cast(unsigned short, (_Float16)v)
                           : __builtin_bit_cast(unsigned short, (__bf16)v);
}

template <bool VEC>
__global__ void __launch_bounds__(COMBINE_THREADS) moe_combine_kernel(const unsigned short* __restrict__ Y, int dtype,
                                                                      int H, int64_t ldy,
                                                                      const int32_t* __restrict__ row_of,
                                                                      const float* __restrict__ w, int k,
                                                                      unsigned short* __restrict__ out) {
    __shared__ int rows[MAX_TOPK];
    __shared__ float ws[MAX_TOPK];
    __shared__ int n_rows;
    const int64_t tok = blockIdx.x;
    // the token's routed rows, ascending (rows are sorted by expert, so this is ascending expert order)
    if (threadIdx.x == 0) {
        int n = 0;
        for (int j = 0; j < k; ++j) {
            const int r = row_of[tok * k + j];
            if (r < 0) continue;
            const float wj = w[tok * k + j];
            int p = n++;
            while (p > 0 && rows[p - 1] > r) {
                rows[p] = rows[p - 1];
                ws[p] = ws[p - 1];
                --p;
            }
            rows[p] = r;
            ws[p] = wj;
        }
        n_rows = n;
    }
    __syncthreads();
    const int n = n_rows;
    unsigned short* orow = out + tok * (int64_t)H;
    if (VEC) {
        for (int h = threadIdx.x * 8; h < H; h += COMBINE_THREADS * 8) {
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < n; ++j) {
                const uint4 u = *(const uint4*)(Y + (int64_t)rows[j] * ldy + h);
                const unsigned v[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float y = qt_h16_to_f32((unsigned short)(v[i >> 1] >> (16 * (i & 1))), dtype);
                    const float c = round_to(y * ws[j], dtype);
                    acc[i] = round_to(acc[i] + c, dtype);
                }
            }
            unsigned o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                o[i] = (unsigned)to_bits(acc[2 * i], dtype) | ((unsigned)to_bits(acc[2 * i + 1], dtype) << 16);
            *(uint4*)(orow + h) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    } else {
        for (int h = threadIdx.x; h < H; h += COMBINE_THREADS) {
            float acc = 0.f;
            for (int j = 0; j < n; ++j) {
                const float c = round_to(qt_h16_to_f32(Y[(int64_t)rows[j] * ldy + h], dtype) * ws[j], dtype);
                acc = round_to(acc + c, dtype);
            }
            orow[h] = to_bits(acc, dtype);
        }
    }
}

}  // namespace

extern "C" int qt_moe_route(const void* top_k_index, int index_is_int64, int64_t T, int k, int E, int32_t* offsets,
                            int32_t* src_token, int32_t* src_slot, int32_t* row_of, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(top_k_index && offsets && src_token && src_slot && T > 0 && k > 0 && E > 0,
                 "qt_moe_route: bad arguments");
    QT_CHECK_ARG(E <= ROUTE_CELLS / 32, "qt_moe_route: E %d > %d experts", E, ROUTE_CELLS / 32);
    QT_CHECK_ARG(T * (int64_t)k <= 0x7fffffffLL, "qt_moe_route: T * k too large");
    int nt = 256;
    while (nt > 32 && nt * E > ROUTE_CELLS) nt >>= 1;
    hipLaunchKernelGGL(moe_route_kernel, dim3(1), dim3(nt), (size_t)nt * E * sizeof(int), stream, top_k_index,
                       index_is_int64 ? 1 : 0, T, k, E, offsets, src_token, src_slot, row_of);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_moe_combine(const void* Y, int dtype, int H, int64_t ldy, const int32_t* row_of,
                              const float* weights, int64_t T, int k, void* out, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(Y && row_of && weights && out && H > 0 && T > 0 && k > 0 && ldy >= H, "qt_moe_combine: bad arguments");
    QT_CHECK_ARG(k <= MAX_TOPK, "qt_moe_combine: k %d > %d", k, MAX_TOPK);
    QT_CHECK_ARG(qt_dtype_is16(dtype), "qt_moe_combine: dtype %d must be bf16 or fp16", dtype);
    QT_CHECK_ARG(T <= 0x7fffffffLL, "qt_moe_combine: T too large");
    const bool vec = H % 8 == 0 && ldy % 8 == 0 && (((uintptr_t)Y | (uintptr_t)out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(moe_combine_kernel<true>, dim3((unsigned)T), dim3(COMBINE_THREADS), 0, stream,
                           (const unsigned short*)Y, dtype, H, ldy, row_of, weights, k, (unsigned short*)out);
    else
        hipLaunchKernelGGL(moe_combine_kernel<false>, dim3((unsigned)T), dim3(COMBINE_THREADS), 0, stream,
                           (const unsigned short*)Y, dtype, H, ldy, row_of, weights, k, (unsigned short*)out);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
