// calculate_qparams, the one statement of it for the weight observers: a range [mn, mx] ->
// (scale, zero point) of the integer grid [qmin, qmax].  fp32 operation by operation (no contraction), IEEE division.
#pragma once
#include "common.h"

__device__ __forceinline__ void qt_calculate_qparams(float mn, float mx, int symmetric, float qmin, float qmax,
                                                     float& s, float& z) {
    mn = fminf(mn, 0.0f);
    mx = fmaxf(mx, 0.0f);
    const float eps = 1.1920928955078125e-07f;
    if (symmetric) {
        const float amax = fmaxf(fabsf(mn), fabsf(mx));
        s = amax / ((qmax - qmin) / 2.0f);
        s = fmaxf(s, eps);
        z = 0.0f;
    } else {
        s = (mx - mn) / (qmax - qmin);
        s = fmaxf(s, eps);
        z = qmin - mn / s;
        z = fminf(fmaxf(rintf(z), qmin), qmax);
    }
}

static inline void qt_range(int num_bits, float* qmin, float* qmax) {
    *qmin = -(float)(1 << (num_bits - 1));
    *qmax = (float)((1 << (num_bits - 1)) - 1);
}
