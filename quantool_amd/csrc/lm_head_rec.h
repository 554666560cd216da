// What the two LM-head kernels share -- lm_head_nll_kernel (lm_head_nll.hip) and lm_head_kl_kernel (lm_head_kl.hip):
// the softmax record of a row over a range of vocabulary columns, the merge that the header's contract fixes, the
// reduce-scatter step that carries 16 accumulator rows across the 32 lanes of an MFMA tile, the record's layout in the
// workspace, the target load and the argument bounds of include/quantool_amd.h.  Each file's head comment keeps the
// hazard argument of its own instance and the order in which it applies the merge.
#pragma once
#include "common.h"

constexpr int LMH_MIN_K = 128, LMH_MAX_K = 32768;
constexpr int64_t LMH_MAX_PITCH = 1 << 22;            // elements: a tile row's byte offset stays below 2^32
static_assert(QT_LM_HEAD_K_UNIT == LMH_MIN_K && QT_LM_HEAD_MIN_K == LMH_MIN_K && QT_LM_HEAD_MAX_K == LMH_MAX_K,
              "header constants");

// {maximum, sum of exp(x - m), lowest column of the maximum}
struct Rec {
    float m, s;
    int i;
};

// Rec with t = sum of exp(x - m) * d over the same columns (d: a second value per column; lm_head_kl.hip: a - b)
struct RecT {
    float m, s;
    int i;
    float t;
};

// the weights of merge(lo, hi): 1 for the side that holds the maximum, exp(-|lo.m - hi.m|) for the other
__device__ __forceinline__ void rec_weights(float lo_m, float hi_m, float& wl, float& wh) {
    const float e = expf(-fabsf(lo_m - hi_m));        // NaN only where both are -inf, and then it is not selected
    wl = lo_m >= hi_m ? 1.0f : e;
    wh = hi_m >= lo_m ? 1.0f : e;
}

__device__ __forceinline__ int rec_index(float lo_m, int lo_i, float hi_m, int hi_i) {
    return hi_m > lo_m ? hi_i : (lo_m > hi_m ? lo_i : min(lo_i, hi_i));
}

__device__ __forceinline__ Rec rec_merge(const Rec& lo, const Rec& hi) {
    Rec o;
    o.m = fmaxf(lo.m, hi.m);
    float wl, wh;
    rec_weights(lo.m, hi.m, wl, wh);
    const float tl = lo.s * wl;
    const float th = hi.s * wh;
    o.s = tl + th;
    o.i = rec_index(lo.m, lo.i, hi.m, hi.i);
    return o;
}

// m, s and i are rec_merge's, operation for operation; t merges with the weights of s
__device__ __forceinline__ RecT rec_merge(const RecT& lo, const RecT& hi) {
    RecT o;
    o.m = fmaxf(lo.m, hi.m);
    float wl, wh;
    rec_weights(lo.m, hi.m, wl, wh);
    const float sl = lo.s * wl;
    const float sh = hi.s * wh;
    o.s = sl + sh;
    o.i = rec_index(lo.m, lo.i, hi.m, hi.i);
    const float tl = lo.t * wl;
    const float th = hi.t * wh;
    o.t = tl + th;
    return o;
}

__device__ __forceinline__ Rec rec_shfl_xor(const Rec& v, int x) {
    Rec got;
    got.m = __shfl_xor(v.m, x);
    got.s = __shfl_xor(v.s, x);
    got.i = __shfl_xor(v.i, x);
    return got;
}

__device__ __forceinline__ RecT rec_shfl_xor(const RecT& v, int x) {
    RecT got;
    got.m = __shfl_xor(v.m, x);
    got.s = __shfl_xor(v.s, x);
    got.i = __shfl_xor(v.i, x);
    got.t = __shfl_xor(v.t, x);
    return got;
}

// One reduce-scatter step over the lane bit X: N rows in, N / 2 out.  The lane whose bit is set keeps the upper half.
template <int N, int X, class R>
__device__ __forceinline__ void rec_scatter_step(R (&v)[16], int lane) {
    const bool hb = (lane & X) != 0;
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
        const R keep = hb ? v[j + N / 2] : v[j];
        const R send = hb ? v[j] : v[j + N / 2];
        const R got = rec_shfl_xor(send, X);
        v[j] = hb ? rec_merge(got, keep) : rec_merge(keep, got);
    }
}

// the last step, xor 1: both lanes of the pair end with the row's record
template <class R>
__device__ __forceinline__ R rec_pair_step(const R& v, int lane) {
    const R got = rec_shfl_xor(v, 1);
    return (lane & 1) ? rec_merge(got, v) : rec_merge(v, got);
}

// ---- the record in the workspace: one float4 per row and vocabulary tile, [tiles_n][M]: {m, s, i (int bits,
// a column of V), t or 0} ----
__device__ __forceinline__ float4 rec_pack(const Rec& o, int n0) {
    return make_float4(o.m, o.s, __int_as_float(n0 + o.i), 0.0f);
}

__device__ __forceinline__ float4 rec_pack(const RecT& o, int n0) {
    return make_float4(o.m, o.s, __int_as_float(n0 + o.i), o.t);
}

__device__ __forceinline__ Rec rec_unpack(const float4& q) { return Rec{q.x, q.y, __float_as_int(q.z)}; }

__device__ __forceinline__ RecT rec_unpack_t(const float4& q) { return RecT{q.x, q.y, __float_as_int(q.z), q.w}; }

__device__ __forceinline__ int64_t load_target(const void* targets, int tgt64, int64_t m) {
    return tgt64 ? ((const int64_t*)targets)[m] : (int64_t)((const int32_t*)targets)[m];
}
