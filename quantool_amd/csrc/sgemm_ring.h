// The tile walk of sgemm_ring_kernel (sgemm_tn.hip) as a device function, so that a second kernel can run it beside
// other workgroups of its own launch (sweep.hip: the far update of one batch next to the block steps of the next).
//
// MODE_SUB on an LDS-DMA ring, persistent over the launch's tiles:
//   * panels go global -> LDS by LDS-DMA (16 B per lane, one instruction per thread and panel) into a ring
//     of RS = 4 stages of BK = 16 k-rows; stages are consumed in pairs: the next pair is requested while the
//     current one is multiplied (32 MFMAs per wave of latency cover), with ONE raw barrier per pair;
//   * a workgroup walks its tiles (wg, + nwg, ...) as ONE stream of stages: the ring never
//     drains between tiles; a tile's C is loaded during its own second k-step (into the registers the
//     previous tile's stores have just released) and is not needed before its first chain ends.
// Wave -> output mapping, MFMA shape and k order are those of sgemm_tn_kernel<128, 128, MODE_SUB, *, 8>:
// per output element the same ascending-k fmaf chain(s) from 0 and the same subtraction(s), so the results
// are bit-identical (tests/test_gpu_sgemm.py compares the two kernels bit for bit).
// Requirements: MODE_SUB, k_mode FULL, M % 128 == 0 and N % 128 == 0 (whole tiles only: no edge predicates
// anywhere), kdim % 32 == 0, kdim >= 64, chain_len % 32 == 0, lda / ldb % 4 == 0, A / B 16-byte aligned,
// 16 * ld * 4 < 2^32, 32 * ldc * 4 < 2^31.  512 threads, 128 registers (amdgpu_waves_per_eu(4, 4)), 64 KiB of LDS.
#pragma once
#include "ring_pipe.h"
#include "sgemm_tn.h"

namespace {

constexpr int RBK = 16;                       // k rows per stage
constexpr int RBM = 128, RBN = 128;
constexpr int RS = 4;                         // ring stages
constexpr int RSTAGE_BYTES = RBK * (RBM + RBN) * 4;   // 16 KiB: A panel then B panel
constexpr int RING_LDS_BYTES = RS * RSTAGE_BYTES;

struct RingArgs {
    const float* A; int64_t lda;
    const float* B; int64_t ldb;
    const float* Cin; int64_t ldcin;
    float* Cout; int64_t ldcout;
    int M, N, kdim, chain_len;     // chain_len > 0
    int tiles_n, n_tiles;          // n_tiles = tiles_m * tiles_n (upper_only: listed tiles only), per problem
    int upper_only;
    // several problems in one launch (SgemmArgs): `batch` problems of this shape at operand strides, walked as
    // batch * n_tiles tiles; or row groups whose B operand sits at B + g * group_bsB
    int batch;
    int64_t bsA, bsB, bsCin, bsCout;
    int n_groups;
    int64_t group_bsB;
    int group_m_end[SG_MAX_GROUPS];
};

// whether qt_sgemm_tn's MODE_SUB product `a` can run on the ring
inline bool sgemm_ring_applies(const SgemmArgs& a) {
    return a.mode == SG_MODE_SUB && a.k_mode == SG_K_FULL && a.k_chunk == 0 && a.kdim >= 4 * RBK &&
           a.kdim % (2 * RBK) == 0 && (a.chain_len == 0 || (a.chain_len % (2 * RBK) == 0 && a.kdim % a.chain_len == 0)) &&
           a.kdim % RBK == 0 && (a.chain_len == 0 || a.chain_len % RBK == 0) && a.M % RBM == 0 && a.N % RBN == 0 &&
           (size_t)40 * (size_t)(a.ldcin > a.ldcout ? a.ldcin : a.ldcout) * 4 < ((size_t)1 << 31) && a.lda % 4 == 0 &&
           a.ldb % 4 == 0 && (((uintptr_t)a.A | (uintptr_t)a.B) & 15) == 0 &&
           (size_t)RBK * (size_t)(a.lda > a.ldb ? a.lda : a.ldb) * 4 < ((size_t)1 << 32) && (!a.upper_only || a.M == a.N);
}

inline RingArgs sgemm_ring_args(const SgemmArgs& a) {
    RingArgs r;
    r.A = a.A; r.lda = a.lda; r.B = a.B; r.ldb = a.ldb;
    r.Cin = a.Cin; r.ldcin = a.ldcin; r.Cout = a.Cout; r.ldcout = a.ldcout;
    r.M = a.M; r.N = a.N; r.kdim = a.kdim;
    r.chain_len = a.chain_len > 0 ? a.chain_len : a.kdim;
    const int tm = (a.M + RBM - 1) / RBM, tn = (a.N + RBN - 1) / RBN;
    r.tiles_n = tn;
    r.upper_only = a.upper_only;
    r.n_tiles = a.upper_only ? tn * (tn + 1) / 2 : tm * tn;
    r.batch = a.batch > 1 ? a.batch : 1;
    r.bsA = a.bsA; r.bsB = a.bsB; r.bsCin = a.bsCin; r.bsCout = a.bsCout;
    r.n_groups = a.n_groups;
    r.group_bsB = a.group_bsB;
    for (int g = 0; g < SG_MAX_GROUPS; ++g) r.group_m_end[g] = a.group_m_end[g];
    return r;
}

// Workgroup wg of nwg walks tiles wg, wg + nwg, ... of the product; `ring` is RING_LDS_BYTES of LDS, 16-byte aligned.
// SHARED_LAUNCH: the launch's first wg0 workgroups do something else, the walkers are the others.  (A template
// switch, not two integer arguments: with wg / nwg as arguments hipcc reassociates the index arithmetic before
// inlining and sgemm_ring_kernel's ISA changes; tools/isa_compare.py holds it to the pre-header kernel.)
template <bool SHARED_LAUNCH>
__device__ __forceinline__ void sgemm_ring_body(RingArgs p, char* ring, const int wg0) {
    const int wg = SHARED_LAUNCH ? (int)blockIdx.x - wg0 : (int)blockIdx.x;
    const int nwg = SHARED_LAUNCH ? (int)gridDim.x - wg0 : (int)gridDim.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1;
    const int h = lane >> 5, l31 = lane & 31;
    const int steps = p.kdim / RBK;                 // per tile
    const int fold_every = p.chain_len / RBK;
    const int all_tiles = p.n_tiles * p.batch;
    const int my_tiles = (all_tiles - wg + nwg - 1) / nwg;
    if (my_tiles <= 0) return;
    const int total = my_tiles * steps;             // stages this workgroup streams

    // tile it (0 .. my_tiles) of this workgroup -> (m0, n0) and the element offsets of its problem's / row group's operands
    auto tile_origin = [&](int it, int& m0, int& n0, size_t& offA, size_t& offB, size_t& offCin, size_t& offCout) {
        int t = wg + it * nwg;
        offA = offB = offCin = offCout = 0;
        if (p.batch > 1) {
            const int b = t / p.n_tiles;
            t -= b * p.n_tiles;
            offA = (size_t)b * p.bsA;
            offB = (size_t)b * p.bsB;
            offCin = (size_t)b * p.bsCin;
            offCout = (size_t)b * p.bsCout;
        }
        int tm, tn;
        if (p.upper_only) {
            // tiles with tn >= tm, listed row by row: row tm holds tiles_n - tm of them (tiles_m == tiles_n)
            int rem = t;
            tm = 0;
            while (rem >= p.tiles_n - tm) { rem -= p.tiles_n - tm; ++tm; }
            tn = tm + rem;
        } else {
            tm = t / p.tiles_n;
            tn = t - tm * p.tiles_n;
        }
        m0 = tm * RBM;
        n0 = tn * RBN;
        if (p.n_groups > 0) {
            int g = 0;
            while (g + 1 < p.n_groups && m0 >= p.group_m_end[g]) ++g;
            offB = (size_t)g * p.group_bsB;
        }
    };

    // DMA geometry: thread t moves 16 bytes of k row (t >> 5), columns 4 * (t & 31) .. + 3 of each panel; a wave's
    // instruction writes 1 KiB = two whole 512-byte panel rows, so the LDS image is plain [k][128] per panel
    const int drow = tid >> 5, dcol = (tid & 31) * 4;
    const unsigned voffA = (unsigned)(((size_t)drow * (size_t)p.lda + dcol) * 4), voffB = (unsigned)(((size_t)drow * (size_t)p.ldb + dcol) * 4);
    const unsigned ring_lds = (unsigned)(size_t)(QT_LDS char*)ring;
    const unsigned dst_wave = __builtin_amdgcn_readfirstlane(ring_lds + (unsigned)wave * 1024u);
    // The stream of stages is issued in order, so its position is kept incrementally (no division per stage: SALU
    // work right behind a barrier is executed by every wave at once, with the MFMA pipe idle)
    int is_it = 0, is_s = 0, is_g = 0;          // next stage to request: tile is_it, k-step is_s, stream index is_g
    const float *is_a, *is_b;
    {
        int m0i, n0i;
        size_t oa, ob, oci, oco;
        tile_origin(0, m0i, n0i, oa, ob, oci, oco);
        is_a = p.A + oa + m0i;
        is_b = p.B + ob + n0i;
    }
    const size_t a_step = (size_t)RBK * p.lda, b_step = (size_t)RBK * p.ldb;
    auto issue_next = [&]() {
        const unsigned d = dst_wave + (unsigned)(is_g & (RS - 1)) * RSTAGE_BYTES;
        glds16_one(voffA, is_a, d);
        glds16_one(voffB, is_b, d + RBK * RBM * 4);
        ++is_g;
        if (++is_s == steps) {
            is_s = 0;
            ++is_it;
            if (is_it < my_tiles) {
                int m0i, n0i;
                size_t oa, ob, oci, oco;
                tile_origin(is_it, m0i, n0i, oa, ob, oci, oco);
                is_a = p.A + oa + m0i;
                is_b = p.B + ob + n0i;
            }
        } else {
            is_a += a_step;
            is_b += b_step;
        }
    };
    static_assert((RS & (RS - 1)) == 0, "slot = stream index & (RS - 1)");

    f32x16 acc[2], cpre[2];
    // C addressing through buffer instructions: descriptor base = the wave's corner of the tile (scalar), soffset =
    // row / sub-tile offset (scalar), voffset = ONE per-lane byte offset that never changes -- no 64-bit per-lane
    // addresses (32 of them cost 64 registers and spill the C tile)
    const int cvoff_in = (int)(((size_t)(4 * h) * (size_t)p.ldcin + (size_t)l31) * 4);
    const int cvoff_out = (int)(((size_t)(4 * h) * (size_t)p.ldcout + (size_t)l31) * 4);
    const int cstep_in = (int)((size_t)p.ldcin * 4), cstep_out = (int)((size_t)p.ldcout * 4);
    // register r of a 32x32 accumulator is row (r & 3) + 8 (r >> 2) (+ 4 h): the per-lane offset walks the rows
    // (+1 row, and +5 rows after every fourth), the sub-tile j is an immediate
    size_t c_off_in = 0, c_off_out = 0;      // the current tile's problem (batch): element offsets of its C
    auto load_c = [&](int m0, int n0) {
        const int rw = m0 + wave_m * 32, cw = n0 + wave_n * 64;      // wave-uniform
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.Cin + c_off_in + (size_t)rw * p.ldcin + cw), 0, 0x7FFFFFFF, 0x00020000);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = ((r & 3) + 8 * (r >> 2)) * cstep_in;      // scalar; the sub-tile j is an immediate
#pragma unroll
            for (int j = 0; j < 2; ++j)
                cpre[j][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, cvoff_in + j * 128, soff, 0));
        }
    };
    auto store_c = [&](int m0, int n0) {      // Cout = cpre - acc
        const int rw = m0 + wave_m * 32, cw = n0 + wave_n * 64;
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(p.Cout + c_off_out + (size_t)rw * p.ldcout + cw), 0, 0x7FFFFFFF, 0x00020000);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int soff = ((r & 3) + 8 * (r >> 2)) * cstep_out;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, cpre[j][r] - acc[j][r]), rs, cvoff_out + j * 128, soff, 0);
        }
    };
    auto zero_acc = [&]() {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    };

    // prologue: first tile's C (older than every DMA), stages 0 and 1
    int m0, n0;
    {
        size_t oa, ob;
        tile_origin(0, m0, n0, oa, ob, c_off_in, c_off_out);
    }
    load_c(m0, n0);
    issue_next();
    issue_next();

    // ONE barrier per PAIR of stages (32 MFMAs per wave between barriers: a barrier is a moment at which every wave
    // of the workgroup has stopped feeding the MFMA pipe).  At the top of pair-step P the stages 2P and 2P + 1 were
    // requested one pair-step ago; stages 2P + 2, 2P + 3 are requested right behind the barrier into the slots of
    // pair P - 1, whose reads every wave finished before arriving here.
    // vmcnt bookkeeping: vmcnt counts EVERY vector-memory operation of the wave in issue order (DMA, C loads, C
    // stores), so "pair P has landed" = "everything is done except what was issued after pair P's request", and the
    // only such operations are the C batch of the END of pair-step P - 1: a tile's 32 stores at the end of its last
    // pair-step, or the 32 loads of a tile (not the first: prologue) at the end of its FIRST pair-step, into the
    // registers the previous tile's stores released one pair-step earlier.
    const int nchains = steps / fold_every;
    const int pairs_per_chain = fold_every / 2;
    int batch_prev = 0;
    int g = 0;
    for (int it = 0; it < my_tiles; ++it) {
        for (int ch = 0; ch < nchains; ++ch) {
            zero_acc();      // every chain starts from zero (its own accumulator live range: no copies at the loop edges)
            for (int ps = 0; ps < pairs_per_chain; ++ps, g += 2) {
                if (batch_prev) wait_vmcnt<32>();
                else wait_vmcnt<0>();
                __builtin_amdgcn_s_barrier();
                if (g + 2 < total) {
                    issue_next();
                    issue_next();
                }
                batch_prev = 0;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const char* stage = ring + ((g + half) & (RS - 1)) * RSTAGE_BYTES;
                    const float* As = (const float*)stage + wave_m * 32 + l31;
                    const float* Bs = (const float*)(stage + RBK * RBM * 4) + wave_n * 64 + l31;
#pragma unroll
                    for (int kk = 0; kk < RBK / 2; ++kk) {
                        const float a = As[(2 * kk + h) * RBM];
                        const float b0 = Bs[(2 * kk + h) * RBN], b1 = Bs[(2 * kk + h) * RBN + 32];
                        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
                        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
                    }
                }
                if (ps == 0 && ch == 0 && it > 0) {
                    // this tile's C into the C registers; first needed when this tile's first chain ends
                    load_c(m0, n0);
                    __builtin_amdgcn_sched_barrier(0);
                    batch_prev = 32;
                }
            }
            if (ch + 1 < nchains) {
                // end of a chain inside the tile: fold it into the C registers
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) cpre[j][r] = cpre[j][r] - acc[j][r];
            }
        }
        // last chain of the tile: C - chain, stored (the batch of the end of the tile's last pair-step)
        store_c(m0, n0);
        __builtin_amdgcn_sched_barrier(0);
        batch_prev = 32;
        if (it + 1 < my_tiles) {
            size_t oa, ob;
            tile_origin(it + 1, m0, n0, oa, ob, c_off_in, c_off_out);     // after this tile's stores were issued
        }
    }
}

}  // namespace
