// The per-token int8 activation quantiser's constants and per-row / per-element steps (include/quantool_amd.h,
// qt_quantize_tokens_i8), shared by the kernels that end in it: quantize_tokens_kernel (qlinear.hip),
// act_mul_quantize_kernel (act_quant.hip) and rmsnorm_quantize_kernel (rmsnorm_quant.hip).
#pragma once
#include <float.h>

#include "common.h"

// Symmetric activation divisor: max(|min|, |max|) / ((qmax - qmin) / 2) with qmin = -128, qmax = 127, as the weight
// observer's /7.5 for 4 bits (SURVEY A.2 calculate_qparams, recalled, not pinned against the upstream
// source).  vLLM's own dynamic int8 path divides by 127 instead; a checkpoint's numbers are only reproduced by the
// divisor its calibration used, so the constant has one home.
constexpr float kActSymDivisor = 127.5f;
constexpr float kActAsymDivisor = 255.0f;
constexpr float kQmin = -128.0f;
constexpr float kQmax = 127.0f;

// (s, zp) of a row from mn = min(min_k x, 0) and mx = max(max_k x, 0)
__device__ __forceinline__ void qt_i8_row_qparams(float mn, float mx, int symmetric, float& s, float& zp) {
    zp = 0.0f;
    if (symmetric) {
        s = fmaxf(-mn, mx) / kActSymDivisor;
        s = fmaxf(s, FLT_EPSILON);
    } else {
        s = (mx - mn) / kActAsymDivisor;
        s = fmaxf(s, FLT_EPSILON);
        zp = fminf(fmaxf(__builtin_rintf(kQmin - mn / s), kQmin), kQmax);
    }
}

__device__ __forceinline__ int q_one(float x, float s, float zp) {
    float v = x / s + zp;
    v = fminf(fmaxf(v, kQmin), kQmax);
    return (int)__builtin_rintf(v);
}

// 8 elements of a 16-bit row (four words of two) -> 8 int8 levels as two words
__device__ __forceinline__ uint2 q_eight(const uint4 u, int dtype, float s, float zp) {
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
    unsigned o[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int qa = q_one(qt_h16_to_f32((unsigned short)(w[i] & 0xffffu), dtype), s, zp);
        const int qb = q_one(qt_h16_to_f32((unsigned short)(w[i] >> 16), dtype), s, zp);
        o[i >> 1] |= (((unsigned)qa & 0xffu) | (((unsigned)qb & 0xffu) << 8)) << (16 * (i & 1));
    }
    return make_uint2(o[0], o[1]);
}
