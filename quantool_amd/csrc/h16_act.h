// The 16-bit narrowing and SiLU(gate) * up as torch's two elementwise kernels leave it, stated once for the two kernels
// that run it: act_mul_quantize_kernel (act_quant.hip, between the int8 products of an A8 MLP) and wq_act_mul_kernel
// (wq_fused.hip, the epilogue of the paired A16 decode GEMV).  include/quantool_amd.h, qt_act_mul_quantize_i8, gives
// the sequence; DESIGN.md 4.20 how it is pinned over every 16-bit pattern.
// Everything sits in an unnamed namespace: each translation unit gets its own copy.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own.
#pragma once
#include <math.h>

#include "common.h"

namespace {

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

}  // namespace
