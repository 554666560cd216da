// W4A16 / W8A16 on packed weights for 33 .. 512 rows: qt_gemm_wq_panel (include/quantool_amd.h, "A16 runtime";
// DESIGN.md 4.25).  Every row equals qt_gemm_wq_skinny's to the bit, as qt_gemm_wq_stream's does; what changes is how
// the activations reach the MFMAs.
//
// wq_panel_kernel      512 threads = 8 waves = 4 chains x 2 wave-columns own 64 output columns n (weight rows) and one
//                      row block of 16 MT activation rows, MT = 1 .. 4; grid (ceil(N / 64), row blocks).  Wave (chain c,
//                      wave-column wc) runs the skinny kernel's wave c on the two 16-column tiles n0 + 32 wc + {0, 16}:
//                      k-blocks kb = c, c + 4, ... ascending, the same A fragment statements, the same MFMA, one fp32
//                      accumulator per (column tile, m-tile).
//   stage t            the four k-blocks 4 t .. 4 t + 3, one per chain.  The workgroup copies X[row block, 512 t : 512 t +
//                      512] into LDS in whole rows: one wave moves one row of 1 KiB per load instruction, 16 bytes per
//                      lane, eight full 128-byte lines.  Register staging: the loads of stage t + 1 are issued before the
//                      MFMAs of stage t and written to the other LDS buffer after them; one barrier per stage.
//   LDS                two buffers of 16 MT rows x PN_PITCH bytes.  PN_PITCH = 1024 + 16: lane (row r, quarter kq) reads
//                      its B fragment of step s at r PN_PITCH + 256 c + 64 kq + 16 s, and the 16 lanes of one quarter
//                      fall into 16 different 16-byte bank groups.  Each B fragment feeds two MFMAs (both column tiles).
//   weights            per stage a lane loads its k-block's chunk of both weight rows (non-temporal 16-byte loads), two
//                      stages ahead of the MFMAs that use them, and dequantises them once into 2 x 4 A fragments that
//                      serve every m-tile.
//   no branch          nothing inside a stage is conditional.  A k-block past K / 128 (a chain's turn in a ragged last
//                      stage) re-reads the last k-block's weights with scale 0 against activations that are zero in LDS
//                      -- the skinny kernel's padded batch: all-zero products leave a sum that started at +0 unchanged.
//                      A row >= M and a column >= K are lanes out of the buffer descriptor's range: zeros, no access.
//                      A weight row >= N reads row 0 with scale 0 and is never stored.
//   epilogue           behind the last stage's barrier the partials of chains 1 .. 3 go through LDS (over the X buffers);
//                      chain 0 adds them in chain order, ((c0 + c1) + c2) + c3, then the bias, one rounding, the store.
//
// -ffp-contract=off (csrc/build.py): every multiply and add below rounds on its own unless written as __builtin_fmaf.
#include "common.h"
#include "wq_stream_tile.h"

static_assert(QT_WQ_PANEL_K_UNIT == WQ_KB, "the tile's k-block is the form's k-unit");

namespace {

constexpr int PN_THREADS = 512;
constexpr int PN_CHAINS = WQ_WAVES;                 // the skinny kernel's 4 waves
constexpr int PN_WAVES = PN_THREADS / 64;           // 4 chains x 2 wave-columns
constexpr int PN_COLS = 64;                         // output columns per workgroup: 2 wave-columns x 2 tiles of 16
constexpr int PN_MAX_MT = 4;                        // m-tiles of 16 rows per row block
constexpr int PN_STAGE_BYTES = PN_CHAINS * WQ_KB * 2;   // one staged row: 4 k-blocks of 16-bit values = 1 KiB
constexpr int PN_PITCH = PN_STAGE_BYTES + 16;       // the staged row's pitch in LDS (see above)
static_assert(QT_WQ_PANEL_MAX_M % (16 * PN_MAX_MT) == 0, "whole row blocks up to the largest M");
// the row block is addressed by 32-bit byte offsets below 2^31
static_assert((int64_t)(16 * PN_MAX_MT) * QT_WQ_PANEL_MAX_LDX * 2 <= (1LL << 31), "row block offsets fit 31 bits");

template <bool INT4, int DT, bool ZP, int MT>
__global__ void __launch_bounds__(PN_THREADS) wq_panel_kernel(const WqArgs p) {
    constexpr int ROWS = 16 * MT;                   // rows of the block
    constexpr int BUF = ROWS * PN_PITCH;
    constexpr int XL = ROWS / PN_WAVES;             // staged rows per wave and stage: rows 8 i + wave
    constexpr int WV = INT4 ? 1 : 2;                // 16-byte weight chunks per lane per k-block and weight row
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF];
    static_assert(3 * 2 * 2 * MT * 64 * (int)sizeof(f32x4) <= 2 * BUF, "the partials fit over the X buffers");

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chain = wave & (PN_CHAINS - 1);       // the skinny kernel's wave
    const int wc = wave / PN_CHAINS;                // wave-column
    const int r = lane & 15;            // A row (weight row) and B column (activation row 16 mt + r)
    const int kq = lane >> 4;           // which 32 columns of the k-block
    const int64_t n0 = (int64_t)blockIdx.x * PN_COLS + 32 * wc;
    const int m0 = blockIdx.y * ROWS;
    const int live = min(p.M - m0, ROWS);           // >= 1: the grid holds ceil(M / ROWS) row blocks
    const int nkb = p.K / WQ_KB;        // K is a multiple of WQ_KB
    const int nst = (nkb + PN_CHAINS - 1) / PN_CHAINS;
    const float off = INT4 ? 8.0f : 128.0f;

    bool n_ok[2];
    int64_t nrow[2];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int64_t n = n0 + 16 * ct + r;
        n_ok[ct] = n < p.N;
        nrow[ct] = n_ok[ct] ? n : 0;
    }

    // the row block of X behind one buffer descriptor that ends with the last column of its last live row
    const unsigned xsize = (unsigned)(((int64_t)(live - 1) * p.ldx + p.K) * 2);
    const auto xrs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.X + (int64_t)m0 * p.ldx), 0, (int)xsize, 0x00020000);
    unsigned xo[XL];                    // the lane's byte offset in stage 0 per staged row; xsize for a row >= M
#pragma unroll
    for (int i = 0; i < XL; ++i) {
        const int row = PN_WAVES * i + wave;
        xo[i] = row < live ? (unsigned)(((int64_t)row * p.ldx + 8 * lane) * 2) : xsize;
    }
    u32x4 xr[XL];
    auto load_x = [&](const int t) {    // stage t's rows into registers; a stage past K gives zeros
        const bool c_ok = t * (PN_CHAINS * WQ_KB) + 8 * lane < p.K;
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const unsigned o = (c_ok && xo[i] != xsize) ? xo[i] + (unsigned)t * PN_STAGE_BYTES : xsize;
            xr[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, (int)o, 0, 0));
        }
    };
    auto store_x = [&](const int buf) {
#pragma unroll
        for (int i = 0; i < XL; ++i)
            *(u32x4*)(lds + buf * BUF + (PN_WAVES * i + wave) * PN_PITCH + 16 * lane) = xr[i];
    };

    // weight chunks, scales and zero-point offsets of two stages in flight: slot = stage & 1
    uint4 wv[2][2][WV];
    float sc[2][2], cz[2][2];
    auto load_w = [&](const int t, auto slot) {
        constexpr int S = decltype(slot)::value;
        const int kb = min(PN_CHAINS * t + chain, nkb - 1);     // a k-block past the end: the last one, scaled by 0
        const int c0 = kb * WQ_KB + 32 * kq;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            if constexpr (INT4) {
                const uint4* src = (const uint4*)((const int32_t*)p.Wq + nrow[ct] * p.Kw + c0 / 8);
                wv[S][ct][0] = ld_nt16(src);
            } else {
                const uint4* src = (const uint4*)((const int8_t*)p.Wq + nrow[ct] * p.K + c0);
                wv[S][ct][0] = ld_nt16(src);
                wv[S][ct][1] = ld_nt16(src + 1);
            }
            group_params<INT4, ZP, false>(p, nrow[ct], c0, sc[S][ct], cz[S][ct]);
        }
    };

    f32x4 acc[2][MT];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[ct][mt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    const int boff = r * PN_PITCH + chain * (WQ_KB * 2) + 64 * kq;     // the lane's B fragment in m-tile 0, step 0

    // stage t out of LDS buffer and weight slot t & 1
    auto stage = [&](const int t, auto slot) {
        constexpr int S = decltype(slot)::value;
        load_x(t + 1);
        // the next stage's rows leave first: left to itself the scheduler sinks these loads into the MFMAs, and the
        // LDS writes below then wait for L2
        __builtin_amdgcn_sched_barrier(0);
        const bool kb_ok = PN_CHAINS * t + chain < nkb;     // uniform
        u32x4 a[2][4];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const float s = (kb_ok && n_ok[ct]) ? sc[S][ct] : 0.0f;
            const float noff = -(off * s);
            const unsigned wd[8] = {wv[S][ct][0].x, wv[S][ct][0].y, wv[S][ct][0].z, wv[S][ct][0].w,
                                    wv[S][ct][WV - 1].x, wv[S][ct][WV - 1].y, wv[S][ct][WV - 1].z, wv[S][ct][WV - 1].w};
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                float uu[8];
                if constexpr (INT4) u_int4(wd[s4], uu);
                else u_int8(wd[2 * s4], wd[2 * s4 + 1], uu);
                a[ct][s4] = frag_from_u<DT, ZP>(uu, s, cz[S][ct], noff);
            }
        }
        load_w(t + 2, slot);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            u32x4 b[4];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
                b[s4] = *(const u32x4*)(lds + S * BUF + 16 * mt * PN_PITCH + boff + 16 * s4);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                acc[0][mt] = mfma16<DT>(a[0][s4], b[s4], acc[0][mt]);
                acc[1][mt] = mfma16<DT>(a[1][s4], b[s4], acc[1][mt]);
            }
        }
        store_x(1 - S);
        __syncthreads();
    };

    load_x(0);
    load_w(0, WqInt<0>{});
    load_w(1, WqInt<1>{});
    store_x(0);
    __syncthreads();
    for (int t = 0; t < nst; t += 2) {
        stage(t, WqInt<0>{});
        if (t + 1 < nst) stage(t + 1, WqInt<1>{});
    }

    // every wave is past the last stage's barrier: the X buffers are free.  As the skinny kernel, per (column tile,
    // m-tile): y = ((c0 + c1) + c2) + c3 (+ bias), one rounding
    f32x4* red = (f32x4*)lds;           // [chain - 1][wc][ct][mt][lane]
    if (chain > 0) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                red[((((chain - 1) * 2 + wc) * 2 + ct) * MT + mt) * 64 + lane] = acc[ct][mt];
    }
    __syncthreads();
    if (chain == 0) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                f32x4 y4 = acc[ct][mt];
#pragma unroll
                for (int c = 0; c < PN_CHAINS - 1; ++c) {
                    const f32x4 o = red[(((c * 2 + wc) * 2 + ct) * MT + mt) * 64 + lane];
#pragma unroll
                    for (int i = 0; i < 4; ++i) y4[i] = y4[i] + o[i];
                }
                // D[row 4 kq + i][col r]: output columns nn .. nn + 3 of activation row m
                const int64_t m = m0 + 16 * mt + r;
                const int64_t nn = n0 + 16 * ct + 4 * kq;
                if (m >= p.M || nn >= p.N) continue;
                float y[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    y[i] = y4[i];
                    if (p.bias && nn + i < p.N) y[i] = y[i] + h2f<DT>(p.bias[nn + i]);
                }
                unsigned short* dst = p.Y + m * p.ldy + nn;
                if (p.vec && nn + 3 < p.N) {            // vec: Y and its pitch are 8-byte aligned
                    *(uint2*)dst = make_uint2(pack2<DT>(y[0], y[1]), pack2<DT>(y[2], y[3]));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (nn + i < p.N) dst[i] = (unsigned short)(pack2<DT>(y[i], 0.0f) & 0xffffu);
                }
            }
        }
    }
}

template <bool I4, int D, bool Z>
void launch_panel(int mt, dim3 grid, hipStream_t stream, const WqArgs& a) {
#define QT_WQ_PANEL_MT(T) \
    case T: hipLaunchKernelGGL((wq_panel_kernel<I4, D, Z, T>), grid, dim3(PN_THREADS), 0, stream, a); break;
    switch (mt) { QT_WQ_PANEL_MT(1) QT_WQ_PANEL_MT(2) QT_WQ_PANEL_MT(3) QT_WQ_PANEL_MT(4) }
#undef QT_WQ_PANEL_MT
}

}  // namespace

extern "C" int qt_gemm_wq_panel(const void* X, int x_dtype, int M, int K, int64_t ldx, const void* Wq, int w_format,
                                int N, const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx,
                                const void* bias, void* Y, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(X && Wq && s_w && Y, "qt_gemm_wq_panel: null pointer (X, Wq, s_w and Y are required)");
    QT_CHECK_ARG(g_idx == nullptr,
                 "qt_gemm_wq_panel: g_idx is not taken (actorder group runs on qt_dequantize_weight + a dense GEMM)");
    QT_CHECK_ARG(qt_dtype_is16(x_dtype), "qt_gemm_wq_panel: x_dtype %d must be bf16 or fp16", x_dtype);
    QT_CHECK_ARG(w_format == QT_W_INT8 || w_format == QT_W_INT4_PACKED, "qt_gemm_wq_panel: w_format %d unsupported",
                 w_format);
    QT_CHECK_ARG(M >= 1 && M <= QT_WQ_PANEL_MAX_M, "qt_gemm_wq_panel: 1 <= M <= %d rows only, got M = %d",
                 QT_WQ_PANEL_MAX_M, M);
    QT_CHECK_ARG(N >= 1 && K >= 1, "qt_gemm_wq_panel: empty weight (N = %d, K = %d)", N, K);
    QT_CHECK_ARG(K % QT_WQ_PANEL_K_UNIT == 0, "qt_gemm_wq_panel: K = %d is not a multiple of the k-unit %d", K,
                 QT_WQ_PANEL_K_UNIT);
    QT_CHECK_ARG(G == 1 || G == K / QT_WQ_PANEL_K_UNIT, "qt_gemm_wq_panel: G must be 1 or K / %d = %d, got %d",
                 QT_WQ_PANEL_K_UNIT, K / QT_WQ_PANEL_K_UNIT, G);
    QT_CHECK_ARG(ldx >= K && ldy >= N && ldx <= QT_WQ_PANEL_MAX_LDX,
                 "qt_gemm_wq_panel: bad pitch (ldx >= K, ldy >= N, ldx <= %d)", QT_WQ_PANEL_MAX_LDX);
    QT_CHECK_ARG((((uintptr_t)X | (uintptr_t)Wq) & 15) == 0 && ldx % 8 == 0,
                 "qt_gemm_wq_panel: X, Wq and the row pitch of X must be 16-byte aligned");
    const bool int4 = w_format == QT_W_INT4_PACKED;
    const bool vec = ((uintptr_t)Y & 7) == 0 && ldy % 4 == 0;
    WqArgs a{(const unsigned short*)X, ldx, M, Wq, N, K, K / 8, s_w, G, zp_w, nullptr,
             (const unsigned short*)bias, (unsigned short*)Y, ldy, (int)vec, nullptr, nullptr, 0};
    // the fewest row blocks of at most 64 rows, of equal height: M = 96 is two blocks of 48 rows, not 64 + 32
    const int blocks = (M + 16 * PN_MAX_MT - 1) / (16 * PN_MAX_MT);
    const int mt = (M + 16 * blocks - 1) / (16 * blocks);
    const dim3 grid((unsigned)(((int64_t)N + PN_COLS - 1) / PN_COLS), (unsigned)((M + 16 * mt - 1) / (16 * mt)));
#define QT_WQ_PANEL_CASE(I4, D, Z) \
    if (int4 == I4 && x_dtype == D && (zp_w != nullptr) == Z) launch_panel<I4, D, Z>(mt, grid, stream, a);
    QT_WQ_PANEL_CASE(true, QT_BF16, false) QT_WQ_PANEL_CASE(true, QT_BF16, true)
    QT_WQ_PANEL_CASE(true, QT_F16, false) QT_WQ_PANEL_CASE(true, QT_F16, true)
    QT_WQ_PANEL_CASE(false, QT_BF16, false) QT_WQ_PANEL_CASE(false, QT_BF16, true)
    QT_WQ_PANEL_CASE(false, QT_F16, false) QT_WQ_PANEL_CASE(false, QT_F16, true)
#undef QT_WQ_PANEL_CASE
    QT_LAUNCH_CHECK();
    return QT_OK;
}
