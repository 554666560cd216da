// The MSE weight observer (upstream's `mse` observer): per group the min/max
// range is shrunk over a grid p_0 .. p_{n-1}, every candidate's (scale, zero point) comes from calculate_qparams --
// the min/max observer's own statement of it (qparams.h) -- and the candidate with the least
// sum |Q(w) - w|^norm wins, the first one on ties.  Modelled on gather_qparams_kernel (quant.hip): one read of W serves
// the observer and the sweep's permuted fp32 working copy.
//
// One 256-thread workgroup per row; the row is staged into LDS once, in its own dtype, with 16-byte loads.
//   * groups of up to 128 columns: a 16-lane segment (one DPP row) owns a group.  Lane j holds elements k * 16 + j
//     (k < group_size / 16 <= 8) in registers as fp32 across the whole candidate loop, so the 20 candidates cost no
//     further LDS traffic; a candidate's partial sums are folded over the segment by four DPP steps that leave the
//     SAME bits in all 16 lanes, so the running best (err, i) lives in registers and no lane waits for another segment.
//     A wave serves 4 groups per pass, the workgroup 16; there is no barrier after the staging one.
//   * wider groups and channel-wise: the workgroup owns a group, every thread re-reads its elements (c = tid, tid +
//     256, ...) from LDS per candidate; a candidate's four wave sums go to their own LDS slots, so the whole candidate
//     loop needs ONE barrier, after which thread 0 adds each candidate's four in a fixed order and picks the winner.
// |e|^norm is v_log_f32 / v_exp_f32 (exp2(norm * log2|e|)); log2(0) = -inf, norm > 0, exp2(-inf) = 0: e = 0 gives 0.
// The division w / s is the IEEE fp32 division the sweep performs (no contraction anywhere in this build).
// No atomics; every sum has a fixed order: deterministic.
#include "common.h"
#include "qparams.h"

namespace {

constexpr int kMaxSteps = 32;
constexpr int kWideScratchFloats = kMaxSteps * 4 + 8;      // wave sums per candidate + the waves' min / max

struct ShrinkGrid {
    float p[kMaxSteps];     // read with a uniform index only and never written: stays in the kernel arguments
};

// lane <- lane ^ 1, lane ^ 2 (quad permutes), then the mirrors of 8 and of 16 lanes: after each step both partners hold
// op(a, b) = op(b, a), so all 16 lanes of the row end with the same bits.
template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <class Op>
__device__ __forceinline__ float seg16_reduce(float v, Op op) {
    v = op(v, dpp_row<0xB1>(v));      // quad_perm [1, 0, 3, 2]
    v = op(v, dpp_row<0x4E>(v));      // quad_perm [2, 3, 0, 1]
    v = op(v, dpp_row<0x141>(v));     // row_half_mirror
    v = op(v, dpp_row<0x140>(v));     // row_mirror
    return v;
}
template <class Op>
__device__ __forceinline__ float wave_reduce(float v, Op op) {
    v = seg16_reduce(v, op);
    v = op(v, __shfl_xor(v, 16));
    v = op(v, __shfl_xor(v, 32));
    return v;
}

// |Q(w) - w|^norm for one weight: the sweep's quantise statement (sweep.hip), then the power
__device__ __forceinline__ float mse_term(float w, float s, float z, float qmin, float qmax, float norm) {
    float x = w / s;
    x = x + z;
    x = fminf(fmaxf(x, qmin), qmax);
    const float q = rintf(x);
    const float dq = (q - z) * s;
    const float e = fabsf(dq - w);
    return __builtin_amdgcn_exp2f(norm * __builtin_amdgcn_logf(e));
}

template <typename T>
__global__ __launch_bounds__(256) void observer_mse_kernel(const T* __restrict__ W, int dtype, int R, int K, int64_t ldw,
                                                           const int32_t* __restrict__ perm,
                                                           const uint8_t* __restrict__ dead, int gs, int symmetric,
                                                           float qmin, float qmax, int n_steps, ShrinkGrid grid,
                                                           float norm, float* __restrict__ out,
                                                           float* __restrict__ scale, float* __restrict__ zp,
                                                           float* __restrict__ scale_t, float* __restrict__ zp_t,
                                                           int64_t ld_t, int8_t* __restrict__ idx, int row_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* row = (T*)smem;
    const int r = blockIdx.x, tid = threadIdx.x;
    const T* src = W + (size_t)r * ldw;
    constexpr int V = 16 / sizeof(T);                    // elements per 16-byte load
    if ((((uintptr_t)src) & 15) == 0 && K % V == 0) {
        for (int c = tid * V; c < K; c += 256 * V) *(f32x4*)(row + c) = *(const f32x4*)(src + c);
    } else {
        for (int c = tid; c < K; c += 256) row[c] = src[c];
    }
    __syncthreads();
    auto val = [&](int c) -> float {
        if constexpr (sizeof(T) == 4) return (float)row[c];
        else return qt_h16_to_f32((unsigned short)row[c], dtype);
    };
    auto fmin_ = [](float a, float b) { return fminf(a, b); };
    auto fmax_ = [](float a, float b) { return fmaxf(a, b); };
    auto add_ = [](float a, float b) { return a + b; };
    const int G = K / gs;
    auto store = [&](int g, float mn, float mx, int bi, float bp) {
        float s, z;
        qt_calculate_qparams(bp * mn, bp * mx, symmetric, qmin, qmax, s, z);
        scale[(size_t)r * G + g] = s;
        zp[(size_t)r * G + g] = z;
        if (scale_t) scale_t[(size_t)g * ld_t + r] = s;
        if (zp_t) zp_t[(size_t)g * ld_t + r] = z;
        if (idx) idx[(size_t)r * G + g] = (int8_t)bi;
    };

    if (gs <= 128) {
        // ---- a 16-lane segment per group, elements in registers -----------------------------------------------
        const int seg = tid >> 4, j = tid & 15, nel = gs >> 4;
        for (int g = seg; g < G; g += 16) {
            float w[8];
            float mn = INFINITY, mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                // past the group: 0, which neither moves the 0-clamped range nor adds to any candidate's error
                w[k] = k < nel ? val(g * gs + k * 16 + j) : 0.0f;
                mn = fminf(mn, w[k]);
                mx = fmaxf(mx, w[k]);
            }
            mn = seg16_reduce(mn, fmin_);
            mx = seg16_reduce(mx, fmax_);
            float best = INFINITY, bp = grid.p[0];
            int bi = 0;
            for (int i = 0; i < n_steps; ++i) {
                const float p = grid.p[i];
                float s, z;
                qt_calculate_qparams(p * mn, p * mx, symmetric, qmin, qmax, s, z);
                float err = 0.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < nel) err = err + mse_term(w[k], s, z, qmin, qmax, norm);
                err = seg16_reduce(err, add_);
                if (err < best) {
                    best = err;
                    bi = i;
                    bp = p;
                }
            }
            if (j == 0) store(g, mn, mx, bi, bp);
        }
    } else {
        // ---- the workgroup per group, elements re-read from LDS per candidate ------------------------------------
        float* red = (float*)(smem + row_bytes);         // [n_steps][4] wave sums
        float* mm = red + kMaxSteps * 4;                 // [4] wave minima, [4] wave maxima
        const int lane = tid & 63, wave = tid >> 6;
        for (int g = 0; g < G; ++g) {
            const int c0 = g * gs;
            float mn = INFINITY, mx = -INFINITY;
            for (int c = tid; c < gs; c += 256) {
                const float w = val(c0 + c);
                mn = fminf(mn, w);
                mx = fmaxf(mx, w);
            }
            mn = wave_reduce(mn, fmin_);
            mx = wave_reduce(mx, fmax_);
            if (lane == 0) {
                mm[wave] = mn;
                mm[4 + wave] = mx;
            }
            __syncthreads();
            mn = fminf(fminf(mm[0], mm[1]), fminf(mm[2], mm[3]));
            mx = fmaxf(fmaxf(mm[4], mm[5]), fmaxf(mm[6], mm[7]));
            for (int i = 0; i < n_steps; ++i) {
                const float p = grid.p[i];
                float s, z;
                qt_calculate_qparams(p * mn, p * mx, symmetric, qmin, qmax, s, z);
                float err = 0.0f;
                for (int c = tid; c < gs; c += 256) err = err + mse_term(val(c0 + c), s, z, qmin, qmax, norm);
                err = wave_reduce(err, add_);
                if (lane == 0) red[i * 4 + wave] = err;
            }
            __syncthreads();
            if (tid == 0) {
                float best = INFINITY, bp = grid.p[0];
                int bi = 0;
                for (int i = 0; i < n_steps; ++i) {
                    const float err = (red[i * 4] + red[i * 4 + 1]) + (red[i * 4 + 2] + red[i * 4 + 3]);
                    if (err < best) {
                        best = err;
                        bi = i;
                        bp = grid.p[i];
                    }
                }
                store(g, mn, mx, bi, bp);
            }
            // no third barrier: the next group's mm is written after this one's second barrier (every read of mm lies
            // before it), and its red after its own first barrier (thread 0's reads of red lie before that)
        }
    }

    if (!out) return;
    float* dst = out + (size_t)r * K;
    if (K % 4 == 0) {
        for (int s4 = tid * 4; s4 < K; s4 += 1024) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int sp = s4 + e;
                const float x = val(perm ? perm[sp] : sp);
                v[e] = (dead && dead[sp]) ? 0.0f : x;
            }
            *(f32x4*)(dst + s4) = v;
        }
    } else {
        for (int sp = tid; sp < K; sp += 256) {
            const float x = val(perm ? perm[sp] : sp);
            dst[sp] = (dead && dead[sp]) ? 0.0f : x;
        }
    }
}

template <typename T>
int launch(const void* W, int w_dtype, int R, int K, int64_t ldw, const int32_t* perm, const uint8_t* dead, int gs,
           int symmetric, int num_bits, int n_steps, const ShrinkGrid& grid, float norm, float* W_f32, float* scale,
           float* zp, float* scale_t, float* zp_t, int64_t ld_t, int8_t* idx, size_t row_bytes, size_t lds,
           hipStream_t stream) {
    static QtOncePerDevice attr;
    QT_HIP(attr.run([&] {
        return hipFuncSetAttribute((const void*)observer_mse_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024);
    }));
    float qmin, qmax;
    qt_range(num_bits, &qmin, &qmax);
    hipLaunchKernelGGL(observer_mse_kernel<T>, dim3(R), dim3(256), lds, stream, (const T*)W, w_dtype, R, K, ldw, perm, dead,
                       gs, symmetric, qmin, qmax, n_steps, grid, norm, W_f32, scale, zp, scale_t, zp_t, ld_t, idx,
                       (int)row_bytes);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

}  // namespace

extern "C" int qt_weight_gather_qparams_mse(const void* W, int w_dtype, int R, int K, int64_t ldw, const int32_t* perm,
                                            const uint8_t* dead, int group_size, int symmetric, int num_bits,
                                            int n_steps, const float* shrink, float norm, float* W_f32, float* scale,
                                            float* zp, float* scale_t, float* zp_t, int64_t ld_t, int8_t* idx,
                                            qt_stream_t stream_) {
    const char* fn = "qt_weight_gather_qparams_mse";
    QT_CHECK_ARG(W && scale && zp && R > 0 && K > 0, "%s: bad arguments", fn);
    QT_CHECK_ARG(qt_dtype_ok(w_dtype), "%s: dtype %d unsupported", fn, w_dtype);
    QT_CHECK_ARG(num_bits >= 2 && num_bits <= 8, "%s: num_bits=%d", fn, num_bits);
    QT_CHECK_ARG(n_steps >= 1 && n_steps <= kMaxSteps && shrink, "%s: n_steps=%d outside 1..%d (or no shrink grid)", fn,
                 n_steps, kMaxSteps);
    ShrinkGrid grid = {};
    for (int i = 0; i < n_steps; ++i) {
        QT_CHECK_ARG(shrink[i] > 0.0f && shrink[i] <= 3.0e38f, "%s: shrink[%d]=%g is not positive and finite", fn, i,
                     (double)shrink[i]);
        grid.p[i] = shrink[i];
    }
    QT_CHECK_ARG(norm > 0.0f && norm <= 3.0e38f, "%s: norm=%g is not positive and finite", fn, (double)norm);
    const int gs = group_size <= 0 ? K : group_size;
    QT_CHECK_ARG(group_size <= 0 || (gs % 32 == 0 && K % gs == 0),
                 "%s: group_size=%d must be a multiple of 32 that divides K=%d (or <= 0: channel-wise)", fn, gs, K);
    QT_CHECK_ARG(R == 1 || ldw >= K, "%s: ldw=%lld < K=%d", fn, (long long)ldw, K);
    QT_CHECK_ARG(W_f32 || (!perm && !dead), "%s: perm / dead without W_f32 (the observer alone takes all three NULL)", fn);
    QT_CHECK_ARG(((uintptr_t)W_f32 & 15) == 0, "%s: W_f32 must be 16-byte aligned", fn);
    QT_CHECK_ARG((!scale_t && !zp_t) || ld_t >= R, "%s: ld_t=%lld < R=%d", fn, (long long)ld_t, R);
    const size_t row_bytes = qt_align_up((size_t)K * qt_dtype_size(w_dtype), 16);
    QT_CHECK_ARG(row_bytes <= 160 * 1024, "%s: a row of %d elements does not fit the LDS", fn, K);
    const size_t lds = row_bytes + (gs > 128 ? kWideScratchFloats * sizeof(float) : 0);
    QT_CHECK_ARG(lds <= 160 * 1024,
                 "%s: a row of %d elements and the %d bytes its wide groups reduce through do not fit the LDS", fn, K,
                 (int)(kWideScratchFloats * sizeof(float)));
    hipStream_t stream = (hipStream_t)stream_;
    if (qt_dtype_size(w_dtype) == 2)
        return launch<unsigned short>(W, w_dtype, R, K, ldw, perm, dead, gs, symmetric, num_bits, n_steps, grid, norm, W_f32,
                                      scale, zp, scale_t, zp_t, ld_t, idx, row_bytes, lds, stream);
    return launch<float>(W, w_dtype, R, K, ldw, perm, dead, gs, symmetric, num_bits, n_steps, grid, norm, W_f32, scale, zp,
                         scale_t, zp_t, ld_t, idx, row_bytes, lds, stream);
}
