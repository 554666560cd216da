// qt_rmsnorm_quantize_i8: the glue in front of the q/k/v and gate/up products of an A8 decoder layer in one row pass --
// y = weight * RMSNorm(x), rounded as transformers' LlamaRMSNorm.forward rounds it, then qt_quantize_tokens_i8's row
// sequence on y (include/quantool_amd.h, "A8 runtime").
//
// One 256-thread workgroup per row, shaped as act_quant.hip is.  Pass 1 reads x from memory once, keeps the row in LDS
// as 16-bit values (2 K bytes, at most 64 KiB) and sums the squares; pass 2 turns the row in LDS into y (each lane its
// own chunks, so no barrier lies between the two), stores Y and reduces min / max; pass 3 quantises from LDS, so the
// col_perm gather is an LDS read.  16-byte loads, 16-byte Y stores and 8-byte Xq stores where the pointers, pitches and
// K allow; no atomics, no workspace, a row's result depends on nothing but the row: the element-load instances walk
// the same 8-element chunks in the same order as the 16-byte ones, so the sum of squares has one order.
//
// Numerics are the header's fixed sequence; -ffp-contract=off (csrc/build.py) keeps every multiply and add its own
// rounding.  The quantiser's constants and per-element step are qlinear.hip's own (i8_quant.h).
#include <math.h>

#include "common.h"
#include "i8_quant.h"

namespace {

constexpr int RQ_THREADS = 256;
constexpr int RQ_WAVES = RQ_THREADS / 64;
constexpr int RQ_MAX_K = 32768;                                   // the GEMMs' own bound
constexpr int RQ_RED_BYTES = 3 * RQ_WAVES * 4;                    // sum, min and max of each wave
constexpr int RQ_MAX_LDS = RQ_MAX_K * 2 + RQ_RED_BYTES;

// fp32 -> the bits of x_dtype, one rounding to nearest even
template <bool F16>
__device__ __forceinline__ unsigned short to_h16(float v) {
    if (F16) return __builtin_bit_cast(unsigned short, (_Float16)v);
    return __builtin_bit_cast(unsigned short, (__bf16)v);
}
template <bool F16>
__device__ __forceinline__ float from_h16(unsigned short b) {
    return F16 ? qt_f16_to_f32(b) : qt_bf16_to_f32(b);
}

// y = round(w * round(x * r)): the normalised row is narrowed before the weight multiplies it
template <bool F16>
__device__ __forceinline__ unsigned short norm_mul(unsigned short xb, unsigned short wb, float r) {
    float p = from_h16<F16>(xb) * r;
    // the fp32 product is a value of its own: left to itself the compiler folds an fp16 operand, the multiply and the
    // narrowing into one v_fma_mixlo_f16, which rounds once where torch's two kernels round twice (seen on the device
    // as rare last-bit differences of fp16 rows on the element-load path)
    asm volatile("" : "+v"(p));
    const float n = from_h16<F16>(to_h16<F16>(p));
    return to_h16<F16>(from_h16<F16>(wb) * n);
}

// VEC_IN: x rows and the weight take 16-byte loads (K % 8 == 0, both pointers 16-byte aligned, ldx % 8 == 0).
// vec_out: Xq rows take 8-byte stores and there is no col_perm;  y_vec: Y rows take 16-byte stores.
template <bool F16, bool VEC_IN>
__global__ void __launch_bounds__(RQ_THREADS) rmsnorm_quantize_kernel(
    const unsigned short* __restrict__ X, int64_t ldx, const unsigned short* __restrict__ weight, int K, float eps,
    const int32_t* __restrict__ col_perm, int symmetric, int vec_out, int8_t* __restrict__ Xq, float* __restrict__ s_x,
    int32_t* __restrict__ zp_x, unsigned short* __restrict__ Y, int64_t ldy, int y_vec, float* __restrict__ rstd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned short* row = (unsigned short*)smem;                          // [K], padded to 8 elements: x, then y
    float* red = (float*)(smem + (size_t)((K + 7) / 8) * 16);             // [3][waves]
    const int64_t m = blockIdx.x;
    const unsigned short* xrow = X + m * ldx;
    unsigned short* yout = Y ? Y + m * ldy : nullptr;
    int8_t* qrow = Xq + m * (int64_t)K;
    const int tid = threadIdx.x;
    constexpr int dtype = F16 ? QT_F16 : QT_BF16;

    // pass 1: lane t owns the chunks c = t, t + 256, ...; its squares are added in ascending k, from 0
    float part = 0.0f;
    if (VEC_IN) {
        for (int k = tid * 8; k < K; k += RQ_THREADS * 8) {
            const uint4 x4 = *(const uint4*)(xrow + k);
            const unsigned xw[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float a = from_h16<F16>((unsigned short)(xw[i] & 0xffffu));
                const float b = from_h16<F16>((unsigned short)(xw[i] >> 16));
                part = part + a * a;
                part = part + b * b;
            }
            *(uint4*)(row + k) = x4;
        }
    } else {
        for (int k0 = tid * 8; k0 < K; k0 += RQ_THREADS * 8) {
            const int n = min(8, K - k0);
            for (int i = 0; i < n; ++i) {
                const unsigned short xb = xrow[k0 + i];
                const float a = from_h16<F16>(xb);
                part = part + a * a;
                row[k0 + i] = xb;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part = part + __shfl_xor(part, off);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();              // the waves' sums are in LDS
    float sum = red[0];
#pragma unroll
    for (int w = 1; w < RQ_WAVES; ++w) sum = sum + red[w];
    const float mean = sum * (1.0f / (float)K);
    // correctly rounded, as torch.rsqrt is on the device (hipcc's rsqrtf is v_rsq_f32, 1 ulp off in one value of ten):
    // sqrt and the division are IEEE in fp64, and narrowing their result rounds 1 / sqrt(v) once
    const float r = (float)(1.0 / sqrt((double)(mean + eps)));
    if (tid == 0 && rstd) rstd[m] = r;

    // pass 2: every lane turns its own chunks of the row into y, in place
    float mn = 0.0f, mx = 0.0f;   // min(min_k y, 0), max(max_k y, 0): start from 0
    if (VEC_IN) {
        for (int k = tid * 8; k < K; k += RQ_THREADS * 8) {
            const uint4 x4 = *(const uint4*)(row + k);
            const uint4 w4 = *(const uint4*)(weight + k);
            const unsigned xw[4] = {x4.x, x4.y, x4.z, x4.w};
            const unsigned ww[4] = {w4.x, w4.y, w4.z, w4.w};
            unsigned yw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned short lo = norm_mul<F16>((unsigned short)(xw[i] & 0xffffu), (unsigned short)(ww[i] & 0xffffu), r);
                const unsigned short hi = norm_mul<F16>((unsigned short)(xw[i] >> 16), (unsigned short)(ww[i] >> 16), r);
                const float a = from_h16<F16>(lo), b = from_h16<F16>(hi);
                mn = fminf(mn, fminf(a, b));
                mx = fmaxf(mx, fmaxf(a, b));
                yw[i] = (unsigned)lo | ((unsigned)hi << 16);
            }
            const uint4 y4 = make_uint4(yw[0], yw[1], yw[2], yw[3]);
            *(uint4*)(row + k) = y4;
            if (yout) {
                if (y_vec) {
                    *(uint4*)(yout + k) = y4;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        yout[k + 2 * i] = (unsigned short)(yw[i] & 0xffffu);
                        yout[k + 2 * i + 1] = (unsigned short)(yw[i] >> 16);
                    }
                }
            }
        }
    } else {
        for (int k0 = tid * 8; k0 < K; k0 += RQ_THREADS * 8) {
            const int n = min(8, K - k0);
            for (int i = 0; i < n; ++i) {
                const unsigned short yb = norm_mul<F16>(row[k0 + i], weight[k0 + i], r);
                const float a = from_h16<F16>(yb);
                mn = fminf(mn, a);
                mx = fmaxf(mx, a);
                row[k0 + i] = yb;
                if (yout) yout[k0 + i] = yb;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    if ((tid & 63) == 0) {
        red[RQ_WAVES + (tid >> 6)] = mn;
        red[2 * RQ_WAVES + (tid >> 6)] = mx;
    }
    __syncthreads();              // y and the waves' min / max are in LDS
    mn = red[RQ_WAVES];
    mx = red[2 * RQ_WAVES];
#pragma unroll
    for (int w = 1; w < RQ_WAVES; ++w) {
        mn = fminf(mn, red[RQ_WAVES + w]);
        mx = fmaxf(mx, red[2 * RQ_WAVES + w]);
    }
    float s, zp;
    qt_i8_row_qparams(mn, mx, symmetric, s, zp);
    if (tid == 0) {
        s_x[m] = s;
        if (zp_x) zp_x[m] = (int32_t)zp;
    }

    if (vec_out) {   // no col_perm, K % 8 == 0: 8 elements -> one 8-byte store
        for (int k = tid * 8; k < K; k += RQ_THREADS * 8)
            *(uint2*)(qrow + k) = q_eight(*(const uint4*)(row + k), dtype, s, zp);
    } else {
        for (int k = tid; k < K; k += RQ_THREADS) {
            // clamped into the row: a bad table cannot move the read out of the K values this workgroup wrote
            const int src = col_perm ? min(max(col_perm[k], 0), K - 1) : k;
            qrow[k] = (int8_t)q_one(from_h16<F16>(row[src]), s, zp);
        }
    }
}

template <bool F16, bool VEC_IN>
int launch(int64_t M, size_t lds, hipStream_t stream, const unsigned short* X, int64_t ldx, const unsigned short* weight,
           int K, float eps, const int32_t* col_perm, int symmetric, int vec_out, int8_t* Xq, float* s_x, int32_t* zp_x,
           unsigned short* Y, int64_t ldy, int y_vec, float* rstd) {
    static QtOncePerDevice lds_attr;   // rows of more than 64 KiB - RQ_RED_BYTES need the raised limit
    QT_HIP(lds_attr.run([&] {
        return hipFuncSetAttribute((const void*)rmsnorm_quantize_kernel<F16, VEC_IN>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, RQ_MAX_LDS);
    }));
    hipLaunchKernelGGL((rmsnorm_quantize_kernel<F16, VEC_IN>), dim3((unsigned)M), dim3(RQ_THREADS), lds, stream, X, ldx,
                       weight, K, eps, col_perm, symmetric, vec_out, Xq, s_x, zp_x, Y, ldy, y_vec, rstd);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

}  // namespace

extern "C" int qt_rmsnorm_quantize_i8(const void* X, int64_t ldx, const void* weight, int x_dtype, int64_t M, int K,
                                      float eps, const int32_t* col_perm, int symmetric, int8_t* Xq, float* s_x,
                                      int32_t* zp_x, void* Y, int64_t ldy, float* rstd, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* fn = "qt_rmsnorm_quantize_i8";
    QT_CHECK_ARG(X, "%s: X is null", fn);
    QT_CHECK_ARG(weight, "%s: weight is null", fn);
    QT_CHECK_ARG(Xq, "%s: Xq is null", fn);
    QT_CHECK_ARG(s_x, "%s: s_x is null", fn);
    QT_CHECK_ARG(M > 0, "%s: M %lld must be positive", fn, (long long)M);
    QT_CHECK_ARG(K > 0, "%s: K %d must be positive", fn, K);
    QT_CHECK_ARG(K <= RQ_MAX_K, "%s: K %d exceeds %d, the int8 GEMMs' bound", fn, K, RQ_MAX_K);
    QT_CHECK_ARG(M <= 0x7fffffffLL, "%s: M %lld too large", fn, (long long)M);
    QT_CHECK_ARG(ldx >= K, "%s: ldx %lld is below K %d", fn, (long long)ldx, K);
    QT_CHECK_ARG(!Y || ldy >= K, "%s: ldy %lld is below K %d", fn, (long long)ldy, K);
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "%s: x_dtype %d must be bf16 or fp16", fn, x_dtype);
    QT_CHECK_ARG(symmetric || zp_x, "%s: asymmetric activations need zp_x", fn);
    QT_CHECK_ARG(eps >= 0.0f && isfinite(eps), "%s: eps %g must be finite and not negative", fn, (double)eps);

    const bool vec_in = K % 8 == 0 && ldx % 8 == 0 && (((uintptr_t)X | (uintptr_t)weight) & 15) == 0;
    const int vec_out = !col_perm && K % 8 == 0 && ((uintptr_t)Xq & 7) == 0;
    const int y_vec = Y && ldy % 8 == 0 && ((uintptr_t)Y & 15) == 0;
    const size_t lds = (size_t)((K + 7) / 8) * 16 + RQ_RED_BYTES;
    const unsigned short* x = (const unsigned short*)X;
    const unsigned short* w = (const unsigned short*)weight;
    unsigned short* y = (unsigned short*)Y;
    int32_t* zp = symmetric ? nullptr : zp_x;
    if (x_dtype == QT_F16) {
        if (vec_in) return launch<true, true>(M, lds, stream, x, ldx, w, K, eps, col_perm, symmetric, vec_out, Xq, s_x, zp, y, ldy, y_vec, rstd);
        return launch<true, false>(M, lds, stream, x, ldx, w, K, eps, col_perm, symmetric, vec_out, Xq, s_x, zp, y, ldy, y_vec, rstd);
    }
    if (vec_in) return launch<false, true>(M, lds, stream, x, ldx, w, K, eps, col_perm, symmetric, vec_out, Xq, s_x, zp, y, ldy, y_vec, rstd);
    return launch<false, false>(M, lds, stream, x, ldx, w, K, eps, col_perm, symmetric, vec_out, Xq, s_x, zp, y, ldy, y_vec, rstd);
}
