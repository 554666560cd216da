// qt_gemm_i8_ring: the prefill / perplexity form of qt_gemm_i8 for W8A8 / INT8 (int8 weights, channel-wise scales):
// a 256 x 256 output tile per 8-wave workgroup, the reduction streamed through the LDS-DMA ring of ring_pipe.h.
// Y is equal to qt_gemm_i8's to the bit (include/quantool_amd.h): the int32 sum is exact and the
// epilogue below is qlinear.hip's, statement for statement, under the same -ffp-contract=off.
//
// THE INSTANCE.  Both operands are K-contiguous, so what a DMA fetches from one row is a run of k-bytes, and a run
// shorter than a 128-byte cache line is paid for as a whole line every time (measured: the 32-k-byte unit the ring of
// xtx_kernel translates to, 16 B per lane and row, ran at 0.6 of the tiled kernel).  So the k-unit is 128
// bytes = one line per row, and what moves through the ring is a HALF PANEL: 128 rows x 128 k-bytes = 16 KiB of A or
// of B, two LDS-DMA instructions per wave, as a unit of xtx_kernel.  K-tile t (k-bytes [128 t, 128 t + 128)) is the
// four units 4t .. 4t+3 = A0, B0, B1, A1 (rows 0-127 / 128-255 of the tile's A and B panels), and its four phases
// 4t .. 4t+3 are the quadrants A0 x B0, A0 x B1, A1 x B0, A1 x B1 of the output tile over that k-range: per wave
// (2 (M) x 4 (N) waves per quadrant, 64 x 32 outputs each) 2 x 1 MFMA tiles x 4 k-steps = 8 v_mfma_i32_32x32x32_i8,
// the count of an xtx_kernel phase.  Fragments stay in registers across the phases that share them: phase 4t reads A0
// and B0 (12 ds_read_b128), 4t+1 B1 (4), 4t+2 A1 (8), 4t+3 nothing.
//   R 8 slots (slot = unit % 8: two K-tiles), L 6 (unit u+6 is issued in phase u), N 2 per wave.
//   RAW: unit i is first read in phase i - 1 at the earliest (B0, B1, A1; A0 in phase i), so the counted wait of phase
//        u leaves only units u+3 .. u+6 in flight: vmcnt(2 * 4 = 8), and unit u+2 is read one phase after the wait
//        that retired it.  64 KiB per CU in flight.
//   WAR: unit i is last read in phase i at the latest, and its slot is re-filled by unit i+8, issued in phase i+2:
//        ring_pipe.h's case L = R - 2.
// LDS image of a unit: 16 pieces of 1 KiB, piece = 8 rows x 128 B; the 16-byte chunk c of row r (of the half panel) sits
// at chunk c ^ ((r >> 1) & 7) of its row.  A wave-instruction of the DMA fills one piece lane-linear (the XOR is on the
// source address); a fragment read (lane l: row l & 31 of its MFMA tile, chunk 2 s + (l >> 5) of k-step s) is one
// ds_read_b128 whose 16-lane groups each cover all 64 banks once.
// A tile row past M (or N) is fetched from row M - 1 (N - 1): the source row is clamped, the value is computed and
// never stored.  K is a whole number of K-tiles, so no byte outside Xq[M, K] and Wq[N, K] is read.
//
// qt_gemm_i8_ring_grouped: the same tile over E weight matrices (ring_tile<true>), equal to qt_gemm_i8_grouped to the
// bit.  The grid holds ceil(R/256) + E m-tile slots per n-tile, an upper bound on
// sum_e ceil(rows_e / 256) that needs no host read of the counts; a workgroup walks the clamped offsets to its (expert,
// tile) and a surplus one returns before its first LDS-DMA and before any barrier.  The expert and the tile's first
// row are wave-uniform, so the B base (expert e's matrix) and, for contiguous rows, the A base stay scalar.  With row_idx
// the A base is Xq itself and each lane's 32-bit offset is row_idx[m] K + 16 c (the host refuses x_rows K > 2^32; the
// index is clamped into [0, x_rows)).  A tile row past the expert's last row re-reads that expert's last row.
//
// qt_splitk_gemm_i8: the same tile over a k-range (ring_tile<false, true>), for 129-2047 rows over a long reduction,
// where the whole-K ring has 16-64 tiles for 256 CUs.  A workgroup is (tile, split): split s owns
// K-tiles [t0(s), t1(s)) (splitk_range), its fetches start at k-byte 128 t0 and it runs 4 (t1 - t0) units.  A split of
// one K-tile is nu = 4 < LEAD: the prologue and the drain ladder take it as they take K = 128.  Nothing else of the
// pipeline knows about the split.  In place of the epilogue the accumulators go, unchanged, into slab s of an int32
// [S][Mp][Np] workspace, the tile's padding included; gemm_i8_splitk_reduce_kernel adds the S slabs in int32 at m < M,
// n < N and runs the epilogue once.  The int32 sum is exact in any order, so Y is qt_gemm_i8's to the bit.  Two
// launches, no atomics, no communication between workgroups inside a launch.
#include "common.h"
#include "i8_args.h"
#include "i8_ring_tile.h"

namespace {

struct RingArgs {
    const int8_t* Xq;
    const int8_t* Wq;
    const float* s_x;
    const int32_t* zp_x;
    const float* s_w;
    const int32_t* wsum;
    const void* bias;
    void* Y;
    int64_t M;
    int N, K;
    int64_t ldy;
    int out_dtype;
};

// The split-K mode (qt_splitk_gemm_i8): a workgroup is (tile, split) = (blockIdx.x, blockIdx.y) and stores its int32
// accumulators into slab blockIdx.y of int32 [splits][Mp][Np] instead of running the epilogue
struct RingSplit {
    int32_t* slab;
    int64_t Mp, Np;                                   // 256 ceil(M/256), 256 ceil(N/256)
    int splits;
};

// K-tiles [t0, t1) of split s out of S over kt K-tiles: contiguous, the first kt % S splits hold one more
__host__ __device__ __forceinline__ void splitk_range(int kt, int S, int s, int& t0, int& t1) {
    const int q = kt / S, r = kt % S;
    t0 = s * q + (s < r ? s : r);
    t1 = t0 + q + (s < r ? 1 : 0);
}

template <bool MOE, bool SPLIT = false>
__device__ __forceinline__ void ring_tile(const RingArgs& p, const RingMoe& g, const RingSplit& sk = RingSplit{}) {
    static_assert(!(MOE && SPLIT), "the split mode is dense");
    __shared__ __attribute__((aligned(16))) char ring[RING * UNIT_BYTES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 2, wave_n = wave & 3;
    const bool group_b = wave >= 4;  // wave-uniform

    const int tiles_n = (p.N + BT - 1) / BT;
    const int tiles_m = (int)((p.M + BT - 1) / BT) + (MOE ? g.E : 0);
    int m_tile, n_tile;                               // the grouped form: m_tile is an m-tile slot
    i8_ring_tile_of(blockIdx.x, tiles_m, tiles_n, m_tile, n_tile);
    int64_t m0 = (int64_t)m_tile * BT;
    int64_t m_end = p.M;                              // rows [m0, m_end) of this tile's matrix exist
    const int n0 = n_tile * BT;
    const int K = p.K;
    const int8_t* Wq = p.Wq;
    const float* s_w = p.s_w;
    const int32_t* wsum = p.wsum;
    if constexpr (MOE) {
        // m-tile slot -> (expert, tile within the expert): i8_ring_tile.h
        int e, lo_e, hi_e;
        // a surplus workgroup returns: uniform, before any LDS-DMA or barrier; p.M = R <= 0x7fffffff (host)
        if (!i8_ring_moe_walk(g, (int)p.M, m_tile, e, lo_e, hi_e)) return;
        e = __builtin_amdgcn_readfirstlane(e);        // wave-uniform: the A and B bases below stay scalar
        m0 = __builtin_amdgcn_readfirstlane(lo_e);
        m_end = __builtin_amdgcn_readfirstlane(hi_e);
        Wq = p.Wq + (int64_t)e * p.N * K;
        s_w = p.s_w + (int64_t)e * p.N;
        if (wsum) wsum = p.wsum + (int64_t)e * p.N;
    }
    // the Xq / s_x / zp_x row of output row m (m < m_end)
    auto src_row = [&](int64_t m) -> int64_t {
        if constexpr (MOE) return i8_ring_moe_src_row(g, m);
        return m;
    };
    int kt0 = 0, kt = K / KU;                         // K-tiles [kt0, kt0 + kt) are this workgroup's
    if constexpr (SPLIT) {
        int t1;
        splitk_range(K / KU, sk.splits, (int)blockIdx.y, kt0, t1);
        kt = t1 - kt0;                                // >= 1: the host refuses splits > K / KU
    }
    const int nu = kt * 4;                            // units = phases

    // ---- staging geometry: two LDS-DMA instructions per thread per unit (pieces 2 wave, 2 wave + 1) ----
    // lane: row lane >> 3 of its piece, physical chunk lane & 7; the logical chunk goes into the source address
    const int64_t a_last = m_end - 1 - m0;            // last valid row of the A / B panel, relative to the tile
    const int b_last = p.N - 1 - n0;
    unsigned voff[4][2];                              // [A0, B0, B1, A1][instruction]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = 16 * wave + 8 * i + (lane >> 3);                   // row of the half panel
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        const int64_t ra0 = r < a_last ? r : a_last, ra1 = HP + r < a_last ? HP + r : a_last;   // clamped: a valid row
        const int rb0 = r < b_last ? r : b_last, rb1 = HP + r < b_last ? HP + r : b_last;
        voff[0][i] = (unsigned)((size_t)ra0 * K + 16 * c);               // < 256 * 32768
        voff[1][i] = (unsigned)((size_t)rb0 * K + 16 * c);
        voff[2][i] = (unsigned)((size_t)rb1 * K + 16 * c);
        voff[3][i] = (unsigned)((size_t)ra1 * K + 16 * c);
    }
    const unsigned ring_lds = (unsigned)(size_t)(QT_LDS char*)ring;
    const unsigned dst_wave = __builtin_amdgcn_readfirstlane(ring_lds + wave * 2048);  // wave-uniform
    const int8_t* srcA = p.Xq + m0 * (int64_t)K;      // scalar: k-byte 0 of the tile's first row
    const int8_t* srcB = Wq + (int64_t)n0 * K;
    if constexpr (SPLIT) {                            // k-byte 128 kt0 of both panels: issue() counts K-tiles from here
        srcA += (size_t)kt0 * KU;
        srcB += (size_t)kt0 * KU;
    }
    if constexpr (MOE) {
        if (g.row_idx) {                              // gathered rows: offsets from Xq itself, < x_rows K <= 2^32
            srcA = p.Xq;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                i8_ring_a_voff(wave, lane, i, a_last, K, [&](int64_t ra) { return src_row(m0 + ra); }, voff[0][i],
                               voff[3][i]);
        }
    }
    // unit i = 4 t + J: J is a compile-time constant wherever the slot is
    auto issue = [&](auto j_c, int t, int slot) {
        constexpr int J = decltype(j_c)::value;
        const unsigned d = dst_wave + (unsigned)slot * UNIT_BYTES;
        glds16_pair(voff[J][0], voff[J][1], ((J == 0 || J == 3) ? srcA : srcB) + (size_t)t * KU, d, d + 1024);
    };

    // ---- fragment read geometry (per lane), byte offsets inside a unit ----
    const int lr = lane & 31, lh = lane >> 5;
    auto frag_off = [&](int r, int s) {               // row r of the half panel, k-step s
        const int x = (r >> 1) & 7;
        return (r >> 3) * 1024 + (r & 7) * 128 + 16 * ((2 * s + lh) ^ x);
    };
    int aoff[2][4], boff[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) aoff[mi][s] = frag_off(wave_m * 64 + mi * 32 + lr, s);
        boff[s] = frag_off(wave_n * 32 + lr, s);
    }

    i32x16 acc[2][2][2];                              // [A half][B half][mi]
#pragma unroll
    for (int qa = 0; qa < 2; ++qa)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) acc[qa][qb][mi] = (i32x16){};

    // ---- the pipeline (ring_pipe.h): R 8, L 6, unit = a half panel, 2 LDS-DMA per wave and unit ----
    i32x4 fa[2][4], fb[2][4];                         // A: [mi][k-step], B: [half][k-step]
    // waits of ring_pipe.h one unit earlier: lead LEAD - 1 in its terms (units u+3 .. u+LEAD may stay in flight)
    auto drain_wait = [&](int u) { ring_drain_wait<2, LEAD - 1>(nu - u - 3); };
    auto phase = [&](auto slot_c, auto steady_c, int u) {
        constexpr int S = decltype(slot_c)::value;
        constexpr bool STEADY = decltype(steady_c)::value;
        constexpr int Q = S & 3, QA = Q >> 1, QB = Q & 1;
        constexpr int ISLOT = (S + LEAD) & (RING - 1);
        // ---- LOAD: the K-tile's units sit in slots (S & 4) + {0: A0, 1: B0, 2: B1, 3: A1} ----
        const char* tile = ring + (S & 4) * UNIT_BYTES;
        if constexpr (Q == 0 || Q == 2) {
            const char* base = tile + (Q == 0 ? 0 : 3) * UNIT_BYTES;
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) fa[mi][s] = *(const i32x4*)(base + aoff[mi][s]);
        }
        if constexpr (Q == 0 || Q == 1) {
            const char* base = tile + (1 + QB) * UNIT_BYTES;
#pragma unroll
            for (int s = 0; s < 4; ++s) fb[QB][s] = *(const i32x4*)(base + boff[s]);
        }
        if (STEADY || u + LEAD < nu) {
            issue(std::integral_constant<int, (S + LEAD) & 3>{}, (u + LEAD) >> 2, ISLOT);
            wait_vmcnt<2 * (LEAD - 2)>();   // everything up to unit u+2 has landed; 4 units stay in flight
        } else {
            drain_wait(u);
        }
        // ---- MATH ----
        ring_sync_math([&] {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
                    acc[QA][QB][mi] =
                        __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[mi][s], fb[QB][s], acc[QA][QB][mi], 0, 0, 0);
        });
    };

    // prologue: units 0..LEAD-1 in flight (nu is 4 or at least 8), units 0 and 1 landed
    issue(std::integral_constant<int, 0>{}, 0, 0);
    issue(std::integral_constant<int, 1>{}, 0, 1);
    issue(std::integral_constant<int, 2>{}, 0, 2);
    issue(std::integral_constant<int, 3>{}, 0, 3);
    if (nu > 4) {
        issue(std::integral_constant<int, 0>{}, 1, 4);
        issue(std::integral_constant<int, 1>{}, 1, 5);
        wait_vmcnt<2 * (LEAD - 2)>();
    } else {
        wait_vmcnt<4>();
    }
    ring_stagger_begin(group_b);

    int u = 0;
    for (; u + 8 + LEAD <= nu; u += 8)   // every phase issues a unit that exists
        ring_body<8>([&](auto slot_c, int uu) { phase(slot_c, std::true_type{}, uu); }, u);
    for (; u + 8 <= nu; u += 8)
        ring_body<8>([&](auto slot_c, int uu) { phase(slot_c, std::false_type{}, uu); }, u);
    if (u < nu) {  // nu is a multiple of 4: one K-tile left
        phase(std::integral_constant<int, 0>{}, std::false_type{}, u);
        phase(std::integral_constant<int, 1>{}, std::false_type{}, u + 1);
        phase(std::integral_constant<int, 2>{}, std::false_type{}, u + 2);
        phase(std::integral_constant<int, 3>{}, std::false_type{}, u + 3);
    }
    ring_stagger_end(group_b);

    if constexpr (SPLIT) {
        // ---- the partial sums, unchanged, into this split's slab: the whole tile, padding included (rows past M and
        // columns past N come from the clamped source rows and are never read).  m0 + 255 < Mp and n0 + 255 < Np, so
        // no store needs a bounds test.  A wave-store is two runs of 32 lanes x 4 B = two 128-byte lines ----
        int32_t* slab = sk.slab + ((int64_t)blockIdx.y * sk.Mp + m0) * sk.Np + n0;   // scalar
#pragma unroll
        for (int qa = 0; qa < 2; ++qa)
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t row = i8_ring_cd_row(qa * HP + wave_m * 64 + mi * 32, r, lh);
                        slab[row * sk.Np + (qb * HP + wave_n * 32 + lr)] = acc[qa][qb][mi][r];
                    }
        return;
    }
    // ---- epilogue: qt_gemm_i8's sequence, once per output element, by the lane that holds it ----
    const bool asym = p.zp_x != nullptr;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const int n = n0 + qb * HP + wave_n * 32 + lr;
        if (n >= p.N) continue;
        float bn = 0.0f;
        const bool has_bias = !MOE && p.bias;         // the grouped form has none
        if (has_bias) bn = qt_load_w(p.bias, p.out_dtype, n);
        const float sw0 = s_w[n];
        const int ws0 = asym ? wsum[n] : 0;
#pragma unroll
        for (int qa = 0; qa < 2; ++qa) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t m = i8_ring_cd_row(m0 + qa * HP + wave_m * 64 + mi * 32, r, lh);
                    if (m >= m_end) continue;
                    const int64_t ms = src_row(m);
                    int a = acc[qa][qb][mi][r];
                    if (asym) a = a - p.zp_x[ms] * ws0;
                    const float prod = sw0 * (float)a;
                    const float tv = 0.0f + prod;
                    float y = p.s_x[ms] * tv;
                    if (has_bias) y = y + bn;
                    qt_store_w(p.Y, p.out_dtype, (size_t)(m * p.ldy + n), y);
                }
            }
        }
    }
}

__global__ __launch_bounds__(NTHREADS, 2) void gemm_i8_ring_kernel(const RingArgs p) { ring_tile<false>(p, RingMoe{}); }
__global__ __launch_bounds__(NTHREADS, 2) void gemm_i8_ring_moe_kernel(const RingArgs p, const RingMoe g) {
    ring_tile<true>(p, g);
}
// grid (tiles, splits): the tile's partial sum over its split's K-tiles -> slab blockIdx.y
__global__ __launch_bounds__(NTHREADS, 2) void gemm_i8_splitk_partial_kernel(const RingArgs p, const RingSplit sk) {
    ring_tile<false, true>(p, RingMoe{}, sk);
}

// The second launch of qt_splitk_gemm_i8: for m < M, n < N the int32 sum of the S slabs, then qt_gemm_i8's epilogue
// (the one above, statement for statement).  A thread owns four consecutive columns of one row: one 16-byte load per
// slab (Np is a multiple of 256 and the slab base is 16-byte aligned); the last quad of a row with N % 4 != 0 is read
// element by element, so no padded element is ever read.  grid (ceil(ceil(N/4) / 256), min(M, 65535)): rows stride
// by gridDim.y.  The sum is integer: no partial is ever converted before it is complete.
constexpr int REDUCE_THREADS = 256;
__global__ __launch_bounds__(REDUCE_THREADS) void gemm_i8_splitk_reduce_kernel(const RingArgs p, const RingSplit sk) {
    const int n = 4 * (int)(blockIdx.x * REDUCE_THREADS + threadIdx.x);
    if (n >= p.N) return;
    const int cnt = p.N - n;                          // columns of this quad that exist: 4 or more is a whole quad
    const bool asym = p.zp_x != nullptr;
    const bool has_bias = p.bias != nullptr;
    const int64_t stride = sk.Mp * sk.Np;
    float sw[4], bn[4];
    int ws[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int nj = j < cnt ? n + j : n;
        sw[j] = p.s_w[nj];
        ws[j] = asym ? p.wsum[nj] : 0;
        bn[j] = has_bias ? qt_load_w(p.bias, p.out_dtype, nj) : 0.0f;
    }
    for (int64_t m = blockIdx.y; m < p.M; m += gridDim.y) {
        const int32_t* src = sk.slab + m * sk.Np + n;
        i32x4 a = (i32x4){};
        if (cnt >= 4) {
#pragma unroll 4
            for (int s = 0; s < sk.splits; ++s) a += *(const i32x4*)(src + s * stride);
        } else {
            for (int s = 0; s < sk.splits; ++s) {
                const int32_t* e = src + s * stride;
                a[0] += e[0];
                if (cnt > 1) a[1] += e[1];
                if (cnt > 2) a[2] += e[2];
            }
        }
        const int zp = asym ? p.zp_x[m] : 0;
        const float sx = p.s_x[m];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= cnt) break;
            int acc = a[j];
            if (asym) acc = acc - zp * ws[j];
            const float prod = sw[j] * (float)acc;
            const float tv = 0.0f + prod;
            float y = sx * tv;
            if (has_bias) y = y + bn[j];
            qt_store_w(p.Y, p.out_dtype, (size_t)(m * p.ldy + n + j), y);
        }
    }
}

}  // namespace

extern "C" int qt_gemm_i8_ring(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N,
                               const float* s_x, const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum,
                               const void* bias, void* Y, int out_dtype, int64_t ldy, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(w_format == QT_W_INT8, "qt_gemm_i8_ring: w_format %d unsupported: int8 weights only (packed int4 runs "
                 "on qt_gemm_i8)", w_format);
    QT_CHECK_ARG(G == 1, "qt_gemm_i8_ring: G %d unsupported: one scale group per row only (grouped scales run on "
                 "qt_gemm_i8)", G);
    QT_CHECK_ARG(K % QT_I8_RING_K_UNIT == 0, "qt_gemm_i8_ring: K %d is not a multiple of the k-unit %d", K,
                 QT_I8_RING_K_UNIT);
    if (int st = qt_i8_check_dense("qt_gemm_i8_ring", Xq, M, K, Wq, w_format, N, s_x, zp_x, s_w, G, wsum, Y, out_dtype, ldy,
                                   true))
        return st;
    static_assert(QT_I8_RING_K_UNIT == KU && QT_I8_RING_SLOTS == RING && QT_I8_RING_LEAD == LEAD, "header constants");
    const int64_t tiles = ((M + BT - 1) / BT) * (int64_t)((N + BT - 1) / BT);
    QT_CHECK_ARG(tiles <= 0x7fffffffLL, "qt_gemm_i8_ring: too many tiles");
    RingArgs a{Xq, (const int8_t*)Wq, s_x, zp_x, s_w, wsum, bias, Y, M, N, K, ldy, out_dtype};
    hipLaunchKernelGGL(gemm_i8_ring_kernel, dim3((unsigned)tiles), dim3(NTHREADS), 0, stream, a);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_gemm_i8_ring_grouped(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R,
                                       const int32_t* offsets, int E, const void* Wq, int w_format, int N,
                                       const float* s_x, const int32_t* zp_x, const float* s_w, int G,
                                       const int32_t* wsum, void* Y, int out_dtype, int64_t ldy, int64_t x_rows,
                                       qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(x_rows > 0, "qt_gemm_i8_ring_grouped: bad arguments");
    QT_CHECK_ARG(w_format == QT_W_INT8, "qt_gemm_i8_ring_grouped: w_format %d unsupported: int8 weights only (packed "
                 "int4 runs on qt_gemm_i8_grouped)", w_format);
    QT_CHECK_ARG(G == 1, "qt_gemm_i8_ring_grouped: G %d unsupported: one scale group per row only (grouped scales run "
                 "on qt_gemm_i8_grouped)", G);
    QT_CHECK_ARG(K % QT_I8_RING_K_UNIT == 0, "qt_gemm_i8_ring_grouped: K %d is not a multiple of the k-unit %d", K,
                 QT_I8_RING_K_UNIT);
    QT_CHECK_ARG(R <= 0x7fffffffLL, "qt_gemm_i8_ring_grouped: R %lld too large", (long long)R);
    QT_CHECK_ARG(E <= 4096, "qt_gemm_i8_ring_grouped: E %d > 4096", E);
    if (int st = qt_i8_check_grouped("qt_gemm_i8_ring_grouped", Xq, K, R, offsets, E, Wq, w_format, N, s_x, zp_x, s_w, G,
                                     wsum, Y, out_dtype, ldy, true))
        return st;
    // gathered rows are addressed by a 32-bit byte offset from Xq; contiguous rows need R of them
    QT_CHECK_ARG(!row_idx || x_rows * (int64_t)K <= (1LL << 32), "qt_gemm_i8_ring_grouped: x_rows %lld x K %d > 2^32 "
                 "bytes: a gathered row is addressed by a 32-bit offset", (long long)x_rows, K);
    QT_CHECK_ARG(row_idx || x_rows >= R, "qt_gemm_i8_ring_grouped: x_rows %lld < R %lld without row_idx",
                 (long long)x_rows, (long long)R);
    const int64_t tiles = ((R + BT - 1) / BT + E) * (int64_t)((N + BT - 1) / BT);
    QT_CHECK_ARG(tiles <= 0x7fffffffLL, "qt_gemm_i8_ring_grouped: too many tiles");
    RingArgs a{Xq, (const int8_t*)Wq, s_x, zp_x, s_w, wsum, nullptr, Y, R, N, K, ldy, out_dtype};
    RingMoe g{offsets, row_idx, x_rows, E};
    hipLaunchKernelGGL(gemm_i8_ring_moe_kernel, dim3((unsigned)tiles), dim3(NTHREADS), 0, stream, a, g);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

extern "C" int qt_splitk_gemm_i8_range(int k_tiles, int splits, int s, int* t0, int* t1) {
    QT_CHECK_ARG(t0 && t1 && k_tiles > 0 && splits > 0 && splits <= k_tiles && s >= 0 && s < splits,
                 "qt_splitk_gemm_i8_range: bad arguments");
    splitk_range(k_tiles, splits, s, *t0, *t1);
    return QT_OK;
}

extern "C" int qt_splitk_gemm_i8_plan(int64_t M, int N, int K, int cus, int splits_requested, int* splits,
                                      size_t* workspace_size) {
    static_assert(QT_SPLITK_I8_K_UNIT == KU, "header constants");
    QT_CHECK_ARG(splits && workspace_size && M > 0 && N > 0 && K > 0 && splits_requested >= 0,
                 "qt_splitk_gemm_i8_plan: bad arguments");
    QT_CHECK_ARG(splits_requested > 0 || cus > 0, "qt_splitk_gemm_i8_plan: cus %d: the rule needs the device's compute "
                 "unit count", cus);
    QT_CHECK_ARG(K % QT_SPLITK_I8_K_UNIT == 0, "qt_splitk_gemm_i8_plan: K %d is not a multiple of the k-unit %d", K,
                 QT_SPLITK_I8_K_UNIT);
    QT_CHECK_ARG(K <= 32768, "qt_splitk_gemm_i8_plan: K %d > 32768 (the int32 accumulator bound)", K);
    const int64_t tiles_m = (M + BT - 1) / BT, tiles_n = ((int64_t)N + BT - 1) / BT;
    QT_CHECK_ARG(tiles_m <= 0x7fffffffLL / tiles_n, "qt_splitk_gemm_i8_plan: too many tiles");
    const int64_t tiles = tiles_m * tiles_n;
    const int kt = K / QT_SPLITK_I8_K_UNIT;
    const int cap = kt < QT_SPLITK_I8_MAX_SPLITS ? kt : QT_SPLITK_I8_MAX_SPLITS;
    int S;
    if (splits_requested == 0) {
        // about one workgroup per compute unit: S tiles' worth of workgroups fill the device once; and no split
        // shorter than QT_SPLITK_I8_MIN_K_TILES K-tiles: below that the slabs cost more than the splits save (4.24)
        const int64_t want = cus / tiles;
        const int longest = kt / QT_SPLITK_I8_MIN_K_TILES < cap ? kt / QT_SPLITK_I8_MIN_K_TILES : cap;
        S = (int)(want < 1 || longest < 1 ? 1 : want > longest ? longest : want);
    } else {
        QT_CHECK_ARG(splits_requested <= kt, "qt_splitk_gemm_i8_plan: splits %d > K / %d = %d: a split owns at least "
                     "one K-tile", splits_requested, QT_SPLITK_I8_K_UNIT, kt);
        QT_CHECK_ARG(splits_requested <= QT_SPLITK_I8_MAX_SPLITS, "qt_splitk_gemm_i8_plan: splits %d > "
                     "QT_SPLITK_I8_MAX_SPLITS = %d", splits_requested, QT_SPLITK_I8_MAX_SPLITS);
        S = splits_requested;
    }
    *splits = S;
    *workspace_size = (size_t)S * (size_t)(tiles_m * BT) * (size_t)(tiles_n * BT) * sizeof(int32_t);   // < 2^53
    return QT_OK;
}

extern "C" int qt_splitk_gemm_i8(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N,
                                 const float* s_x, const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum,
                                 const void* bias, void* Y, int out_dtype, int64_t ldy, int splits, void* workspace,
                                 size_t workspace_size, qt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    QT_CHECK_ARG(w_format == QT_W_INT8, "qt_splitk_gemm_i8: w_format %d unsupported: int8 weights only (packed int4 "
                 "runs on qt_gemm_i8)", w_format);
    QT_CHECK_ARG(G == 1, "qt_splitk_gemm_i8: G %d unsupported: one scale group per row only (grouped scales run on "
                 "qt_gemm_i8)", G);
    QT_CHECK_ARG(K % QT_SPLITK_I8_K_UNIT == 0, "qt_splitk_gemm_i8: K %d is not a multiple of the k-unit %d", K,
                 QT_SPLITK_I8_K_UNIT);
    if (int st = qt_i8_check_dense("qt_splitk_gemm_i8", Xq, M, K, Wq, w_format, N, s_x, zp_x, s_w, G, wsum, Y, out_dtype,
                                   ldy, true))
        return st;
    QT_CHECK_ARG(splits >= 1, "qt_splitk_gemm_i8: splits %d: take the count from qt_splitk_gemm_i8_plan", splits);
    QT_CHECK_ARG(splits != 1, "qt_splitk_gemm_i8: splits 1 is qt_gemm_i8_ring (the same tile, no slab)");
    QT_CHECK_ARG(workspace, "qt_splitk_gemm_i8: workspace is null");
    QT_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "qt_splitk_gemm_i8: workspace is not 16-byte aligned");
    int S = 0;
    size_t need = 0;
    if (int st = qt_splitk_gemm_i8_plan(M, N, K, 0, splits, &S, &need)) return st;
    QT_CHECK_ARG(workspace_size >= need, "qt_splitk_gemm_i8: workspace_size %zu < %zu needed (S %d x Mp x Np x 4)",
                 workspace_size, need, S);
    const int64_t tiles_m = (M + BT - 1) / BT, tiles_n = ((int64_t)N + BT - 1) / BT;
    RingArgs a{Xq, (const int8_t*)Wq, s_x, zp_x, s_w, wsum, bias, Y, M, N, K, ldy, out_dtype};
    RingSplit sk{(int32_t*)workspace, tiles_m * BT, tiles_n * BT, S};
    hipLaunchKernelGGL(gemm_i8_splitk_partial_kernel, dim3((unsigned)(tiles_m * tiles_n), (unsigned)S), dim3(NTHREADS), 0,
                       stream, a, sk);
    QT_LAUNCH_CHECK();
    const int64_t quads = ((int64_t)N + 3) / 4;
    const dim3 rgrid((unsigned)((quads + REDUCE_THREADS - 1) / REDUCE_THREADS), (unsigned)(M < 65535 ? M : 65535));
    hipLaunchKernelGGL(gemm_i8_splitk_reduce_kernel, rgrid, dim3(REDUCE_THREADS), 0, stream, a, sk);
    QT_LAUNCH_CHECK();
    return QT_OK;
}
