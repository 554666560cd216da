// Packed int4 -> int8 on chip, shared by the A8 GEMMs (qlinear.hip, qlinear_skinny.hip).
#pragma once
#include "common.h"

// packed word (nibble j = level + 8 of column 8w + j) -> 8 int8 levels, column order
__device__ __forceinline__ uint2 unpack_int4_word(unsigned w) {
    const unsigned lo = w & 0x0f0f0f0fu;          // nibbles 0, 2, 4, 6 in bytes 0..3
    const unsigned hi = (w >> 4) & 0x0f0f0f0fu;   // nibbles 1, 3, 5, 7
    // interleave: bytes [lo0 hi0 lo1 hi1] and [lo2 hi2 lo3 hi3] (v_perm_b32: selector byte i picks from {hi:lo}
    // of the first / second operand: 0..3 -> second operand's bytes, 4..7 -> first operand's)
    unsigned a = __builtin_amdgcn_perm(hi, lo, 0x05010400u);
    unsigned b = __builtin_amdgcn_perm(hi, lo, 0x07030602u);
    // x - 8 per byte for x in 0..15 without borrows: (x + 0x78) ^ 0x80
    a = (a + 0x78787878u) ^ 0x80808080u;
    b = (b + 0x78787878u) ^ 0x80808080u;
    return make_uint2(a, b);
}
