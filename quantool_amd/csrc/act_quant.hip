// qt_act_mul_quantize_i8: the glue between the two products of an A8 MLP or expert bank in one row pass --
// h = SiLU(gate) * up, rounded as torch's two elementwise kernels round it, then qt_quantize_tokens_i8's row sequence
// on h (include/quantool_amd.h, "A8 runtime").
//
// One 256-thread workgroup per row.  Pass 1 computes h once per element (one expf, one IEEE division), keeps the row in
// LDS as 16-bit values (2 K bytes, at most 64 KiB) and reduces min / max; pass 2 quantises from LDS, so the col_perm
// gather is an LDS read and gate / up are read from memory once.  16-byte loads and 8-byte stores where the pointers,
// pitches and K allow; no atomics, no workspace, a row's result depends on nothing but the row.
//
// Numerics are the header's fixed sequence; -ffp-contract=off (csrc/build.py) keeps every multiply and add its own
// rounding.  The quantiser's constants and per-element step are qlinear.hip's own (i8_quant.h).
#include <math.h>

#include "common.h"
#include "i8_quant.h"

namespace {

constexpr int AQ_THREADS = 256;
constexpr int AQ_MAX_K = 32768;                                   // the GEMMs' own bound
constexpr int AQ_RED_BYTES = 2 * (AQ_THREADS / 64) * 4;           // min / max of each wave
constexpr int AQ_MAX_LDS = AQ_MAX_K * 2 + AQ_RED_BYTES;

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

// h = round(round(silu(g)) * u): torch's SiLU kernel leaves a 16-bit tensor, its multiply another
template <bool F16>
__device__ __forceinline__ unsigned short silu_mul(unsigned short gb, unsigned short ub) {
    const float g = from_h16<F16>(gb);
    const float u = from_h16<F16>(ub);
    const float a = g / (1.0f + expf(-g));
    const float ar = from_h16<F16>(to_h16<F16>(a));
    const float p = ar * u;
    return to_h16<F16>(p);
}

// VEC_IN: gate and up rows take 16-byte loads (K % 8 == 0, both pointers 16-byte aligned, both pitches % 8 == 0).
// vec_out: Xq rows take 8-byte stores and there is no col_perm;  h_vec: H rows take 16-byte stores.
template <bool F16, bool VEC_IN>
__global__ void __launch_bounds__(AQ_THREADS) act_mul_quantize_kernel(
    const unsigned short* __restrict__ gate, int64_t ldg, const unsigned short* __restrict__ up, int64_t ldu, int K,
    const int32_t* __restrict__ col_perm, int symmetric, int vec_out, int8_t* __restrict__ Xq, float* __restrict__ s_x,
    int32_t* __restrict__ zp_x, unsigned short* __restrict__ H, int64_t ldh, int h_vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned short* hrow = (unsigned short*)smem;                         // [K], padded to 8 elements
    float* red = (float*)(smem + (size_t)((K + 7) / 8) * 16);             // [2][waves]
    const int64_t m = blockIdx.x;
    const unsigned short* grow = gate + m * ldg;
    const unsigned short* urow = up + m * ldu;
    unsigned short* hout = H ? H + m * ldh : nullptr;
    int8_t* qrow = Xq + m * (int64_t)K;
    const int tid = threadIdx.x;
    constexpr int dtype = F16 ? QT_F16 : QT_BF16;

    float mn = 0.0f, mx = 0.0f;   // min(min_k h, 0), max(max_k h, 0): start from 0
    if (VEC_IN) {
        for (int k = tid * 8; k < K; k += AQ_THREADS * 8) {
            const uint4 g4 = *(const uint4*)(grow + k);
            const uint4 u4 = *(const uint4*)(urow + k);
            const unsigned gw[4] = {g4.x, g4.y, g4.z, g4.w};
            const unsigned uw[4] = {u4.x, u4.y, u4.z, u4.w};
            unsigned hw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned short lo = silu_mul<F16>((unsigned short)(gw[i] & 0xffffu), (unsigned short)(uw[i] & 0xffffu));
                const unsigned short hi = silu_mul<F16>((unsigned short)(gw[i] >> 16), (unsigned short)(uw[i] >> 16));
                const float a = from_h16<F16>(lo), b = from_h16<F16>(hi);
                mn = fminf(mn, fminf(a, b));
                mx = fmaxf(mx, fmaxf(a, b));
                hw[i] = (unsigned)lo | ((unsigned)hi << 16);
            }
            const uint4 h4 = make_uint4(hw[0], hw[1], hw[2], hw[3]);
            *(uint4*)(hrow + k) = h4;
            if (hout) {
                if (h_vec) {
                    *(uint4*)(hout + k) = h4;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        hout[k + 2 * i] = (unsigned short)(hw[i] & 0xffffu);
                        hout[k + 2 * i + 1] = (unsigned short)(hw[i] >> 16);
                    }
                }
            }
        }
    } else {
        for (int k = tid; k < K; k += AQ_THREADS) {
            const unsigned short hb = silu_mul<F16>(grow[k], urow[k]);
            const float a = from_h16<F16>(hb);
            mn = fminf(mn, a);
            mx = fmaxf(mx, a);
            hrow[k] = hb;
            if (hout) hout[k] = hb;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = mn;
        red[AQ_THREADS / 64 + (tid >> 6)] = mx;
    }
    __syncthreads();              // the row and the waves' min / max are in LDS
    mn = red[0];
    mx = red[AQ_THREADS / 64];
#pragma unroll
    for (int w = 1; w < AQ_THREADS / 64; ++w) {
        mn = fminf(mn, red[w]);
        mx = fmaxf(mx, red[AQ_THREADS / 64 + w]);
    }
    float s, zp;
    qt_i8_row_qparams(mn, mx, symmetric, s, zp);
    if (tid == 0) {
        s_x[m] = s;
        if (zp_x) zp_x[m] = (int32_t)zp;
    }

    if (vec_out) {   // no col_perm, K % 8 == 0: 8 elements -> one 8-byte store
        for (int k = tid * 8; k < K; k += AQ_THREADS * 8)
            *(uint2*)(qrow + k) = q_eight(*(const uint4*)(hrow + k), dtype, s, zp);
    } else {
        for (int k = tid; k < K; k += AQ_THREADS) {
            // clamped into the row: a bad table cannot move the read out of the K values this workgroup wrote
            const int src = col_perm ? min(max(col_perm[k], 0), K - 1) : k;
            qrow[k] = (int8_t)q_one(from_h16<F16>(hrow[src]), s, zp);
        }
    }
}

template <bool F16, bool VEC_IN>
int launch(int64_t M, size_t lds, hipStream_t stream, const unsigned short* gate, int64_t ldg, const unsigned short* up,
           int64_t ldu, int K, const int32_t* col_perm, int symmetric, int vec_out, int8_t* Xq, float* s_x,
           int32_t* zp_x, unsigned short* H, int64_t ldh, int h_vec) {
    static QtOncePerDevice lds_attr;   // rows of more than 64 KiB - AQ_RED_BYTES need the raised limit
    QT_HIP(lds_attr.run([&] {
        return hipFuncSetAttribute((const void*)act_mul_quantize_kernel<F16, VEC_IN>,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, AQ_MAX_LDS);
    }));
    hipLaunchKernelGGL((act_mul_quantize_kernel<F16, VEC_IN>), dim3((unsigned)M), dim3(AQ_THREADS), lds, stream, gate,
                       ldg, up, ldu, K, col_perm, symmetric, vec_out, Xq, s_x, zp_x, H, ldh, h_vec);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

}  // namespace

extern "C" int qt_act_mul_quantize_i8(const void* gate, int64_t ldg, const void* up, int64_t ldu, int x_dtype, int64_t M,
                                      int K, int act, const int32_t* col_perm, int symmetric, int8_t* Xq, float* s_x,
                                      int32_t* zp_x, void* H, int64_t ldh, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* fn = "qt_act_mul_quantize_i8";
    QT_CHECK_ARG(gate, "%s: gate is null", fn);
    QT_CHECK_ARG(up, "%s: up is null", fn);
    QT_CHECK_ARG(Xq, "%s: Xq is null", fn);
    QT_CHECK_ARG(s_x, "%s: s_x is null", fn);
    QT_CHECK_ARG(M > 0, "%s: M %lld must be positive", fn, (long long)M);
    QT_CHECK_ARG(K > 0, "%s: K %d must be positive", fn, K);
    QT_CHECK_ARG(K <= AQ_MAX_K, "%s: K %d exceeds %d, the int8 GEMMs' bound", fn, K, AQ_MAX_K);
    QT_CHECK_ARG(M <= 0x7fffffffLL, "%s: M %lld too large", fn, (long long)M);
    QT_CHECK_ARG(ldg >= K, "%s: ldg %lld is below K %d", fn, (long long)ldg, K);
    QT_CHECK_ARG(ldu >= K, "%s: ldu %lld is below K %d", fn, (long long)ldu, K);
    QT_CHECK_ARG(!H || ldh >= K, "%s: ldh %lld is below K %d", fn, (long long)ldh, K);
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "%s: x_dtype %d must be bf16 or fp16", fn, x_dtype);
    QT_CHECK_ARG(act == QT_ACT_SILU, "%s: unknown act %d", fn, act);
    QT_CHECK_ARG(symmetric || zp_x, "%s: asymmetric activations need zp_x", fn);

    const bool vec_in = K % 8 == 0 && ldg % 8 == 0 && ldu % 8 == 0 && (((uintptr_t)gate | (uintptr_t)up) & 15) == 0;
    const int vec_out = !col_perm && K % 8 == 0 && ((uintptr_t)Xq & 7) == 0;
    const int h_vec = H && ldh % 8 == 0 && ((uintptr_t)H & 15) == 0;
    const size_t lds = (size_t)((K + 7) / 8) * 16 + AQ_RED_BYTES;
    const unsigned short* g = (const unsigned short*)gate;
    const unsigned short* u = (const unsigned short*)up;
    unsigned short* h = (unsigned short*)H;
    int32_t* zp = symmetric ? nullptr : zp_x;
    if (x_dtype == QT_F16) {
        if (vec_in) return launch<true, true>(M, lds, stream, g, ldg, u, ldu, K, col_perm, symmetric, vec_out, Xq, s_x, zp, h, ldh, h_vec);
        return launch<true, false>(M, lds, stream, g, ldg, u, ldu, K, col_perm, symmetric, vec_out, Xq, s_x, zp, h, ldh, h_vec);
    }
    if (vec_in) return launch<false, true>(M, lds, stream, g, ldg, u, ldu, K, col_perm, symmetric, vec_out, Xq, s_x, zp, h, ldh, h_vec);
    return launch<false, false>(M, lds, stream, g, ldg, u, ldu, K, col_perm, symmetric, vec_out, Xq, s_x, zp, h, ldh, h_vec);
}
