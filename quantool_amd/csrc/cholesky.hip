// a8: U = chol((H + damp I)^-1, upper)   (upstream quantize_weight:
// cholesky -> cholesky_inverse -> cholesky(upper), reached through gptq.py:86 / base.py:161).
//
// One factorisation instead of three.  With A = flat-reverse(Hd) (A[i][j] = Hd[K-1-i][K-1-j],
// built by qt_hessian_prepare):   A = R^T R (R upper)  =>  Hd = (J R^T J)(J R J) = Ut Ut^T with
// Ut = J R^T J upper, so Hd^-1 = (Ut^-1)^T (Ut^-1) and, by uniqueness of the Cholesky factor,
//     U = Ut^-1 = J R^-T J = flat-reverse(Y),   Y = R^-T (lower).
// Cost 2/3 K^3 flops (vs 4/3 K^3) and every block recurrence below is a k-major "TN" product.  Two block
// sizes: NB = 128 for the latency-bound panel kernels, NBO / NBI for everything that carries the K^3 (chol_blocks: 512
// where the plane products are live, 256 on the f32 chain).
//   potrf over NBO-wide outer blocks J, left-looking inside one (all in place in A):
//     block row j of J :  A[j, j:] -= sum_{p in J, p<j} R[p, j]^T R[p, j:]   (sgemm SUB, k <= NBO - 128)
//                         R_jj = chol(A_jj), 32x32 inverses                   (potf2_kernel)
//                         R[j, j+1:] = R_jj^-T A[j, j+1:]                     (trsm_rt_kernel)
//     outer level, small K (no product long enough for the bf16 MFMA) -- RIGHT-looking:
//       after block J  :  A[J1:, J1:] -= R[J, J1:]^T R[J, J1:]                (sgemm SUB, k = NBO, upper tiles only)
//     outer level, large K -- LEFT-looking, so the K^3/3 runs as long-k block-row products:
//       before block J :  A[J, J0:] -= R[:J0, J]^T R[:J0, J0:]                (gemm3 SUB, k = J0; sgemm where short)
//       after block J  :  bf16 plane copies of R[J, J0:]                      (split3_kernel)
//   R^-T by NBI-row block rows I (Y lower, so the k range of a tile starts at its first column):
//     inside I         :  Y_II by the 128-row recurrence  T = sum_{p in I, p<i} R[p, i]^T Y[p, I0:i];
//                         Y[i, I0:i] = -Dinv_i^T T ;  Y[i, i] = Dinv_i^T     (k <= NBI - 128)
//     left of I        :  T_I = sum_{p<I0} R[p, I]^T Y[p, :I0]               (gemm3 SET / sgemm SET, k = I0)
//                         Y[I, :I0] = -Y_II T_I = -(Y_II^T)^T T_I             (transpose + sgemm NEG, k = NBI)
//                         bf16 plane copies of Y[I, :I1]                      (split3_kernel, large K only)
// The two phases can also run as ONE walk over the block rows (QT_CHOL_MERGE, chol_merge_mode() below): block row J's
// two long products have the same A operand R[:J0, J], the same k range and need only rows before J of R and Y, so
// they fit one gemm3 launch with two output segments and one item table.
// gemm3 (gemm3_tn.h) = fp32-accurate product on the bf16 MFMA from three bf16 planes per operand; sgemm
// (sgemm_tn.h) = the f32-MFMA fmaf chain.
// With a lower bound on lambda_min(A) (the _bounded entry points) the gemm3 products run on TWO fp16 planes per
// operand and three plane products (G3_F16X2): the range fp16 lacks is supplied by two per-problem power-of-two scales,
//     |R[i][j]| <= sqrt(A[j][j]) <= sqrt(max diag A)              (A = R^T R: column j of R has norm sqrt(A[j][j]))
//     |Y[i][j]| <= ||R^-1||_2 = 1 / sqrt(lambda_min(A))           (Y = R^-T)
// computed on the device from A's diagonal and the caller's bound before A is overwritten (chol_scales_kernel).
// Host side, behind the kernels: CholLayout (chol_layout.h) is the one statement of a problem's workspace, CholCtx what
// every step reads, chol_sgemm_args / g3_row the two product builders, fac_product ... inv_row the steps above, and
// chol_run_two_phase / chol_run_walk the two orders in which chol_run enqueues them.
#include <stdlib.h>
#include <string.h>

#include <map>
#include <tuple>
#include <vector>

#include "chol_layout.h"
#include "common.h"
#include "gemm3_tn.h"
#include "sgemm_tn.h"

namespace {

static_assert(CHOL_CHUNK_ROWS == G3_CHUNK_ROWS, "chol_layout.h counts k chunks as gemm3_tn.h cuts them");
// Outer block of the factorisation / block-row height of the inverse (multiples of 128).  QT_CHOL_NBO /
// QT_CHOL_NBI force them (A/B runs); otherwise 256 on the f32 chain (measured at K = 14336 / 4096: 128: 40.5 /
// 4.30 ms, 256: 35.3 / 4.04, 512: 36.4 / 4.05, 1024: 38.5 / 4.40) and 512 where the bf16x3 products are in
// use -- two tile rows per product halve the k-split and the slab traffic (K = 14336 / 8192: 23.7 / 9.6 ms at
// 256 / 256, 23.0 / 9.2 at 512 / 256, 22.8 / 8.9 at 512 / 512; bench 84.5 -> 82.9 ms/step).
static int chol_block_env(const char* name) {
    const char* e = getenv(name);
    if (!e) return 0;
    int x = atoi(e) / 128 * 128;
    return x < 128 ? 128 : (x > NBO_MAX ? NBO_MAX : x);
}
// ---- bf16x3 block-row products (gemm3_tn.h) ---------------------------------------------------------
// Where a block-row product of the chain has enough k-chunks to fill the chip with xtx-class items, it
// runs on the bf16 MFMA from three-plane copies of R and Y (measured in the same process, k = 14080,
// 256 x 14080 outputs: 0.53 ms vs 0.90 ms on the f32 MFMA; tools/gemm3_bench.py).  The factorisation is
// then LEFT-looking at the outer level (block row J gathers  A[J, J:] -= R[:J0, J]^T R[:J0, J:]  in one
// long-k product: each element of A is read and written once, where the right-looking k = 256 update of
// the whole trailing matrix is bound by that read-modify-write), and the inverse's T_I product is the same
// shape.  QT_CHOL_G3=0 disables; QT_CHOL_G3_MIN_CHUNKS = k rows a product needs, in units of 128 (two 64-row chunks of gemm3_tn.h; 256 =
// one per CU in rounds 2-3; K = 14336 / 8192 / 4096: 24.2 / 9.5 / 3.6 ms at 64...256, 24.6 at 640, 24.9 at 768; off: 34.0 /
// 10.7 / 3.6.  Round 4: 64 -- with the short f32 products split less (sgemm_tn.hip) and the chains batched, more of
// the K = 4096 steps pay on the bf16 MFMA: single chain 3.82 -> 3.70 ms, three batched 5.55 -> 5.23, ten batched
// 10.9 -> 10.4; K = 8192 / 14336 unchanged).  Item tables for every step are built once per (K, block sizes) in pinned host memory and
// uploaded with one async copy per call.
struct G3Step {
    int n_items = 0, n_red = 0;
    size_t item_off = 0, red_off = 0;   // bytes into the table blob
};
struct CholG3Plan {
    bool any = false;
    std::vector<G3Step> fac, inv;       // per outer block / per block row (n_items == 0: sgemm_tn)
    std::vector<G3Step> row;            // merged plans: per block row, both products in one table (n_items == 0: fac / inv)
    char* blob = nullptr;               // pinned
    size_t blob_bytes = 0;
    int max_slabs = 0;
    bool any_row = false;               // some row is merged
};

static int chol_g3_min_chunks() {   // read per call: tests switch the path on for small K
    const char* on = getenv("QT_CHOL_G3");
    if (on && atoi(on) == 0) return 0;
    const char* e = getenv("QT_CHOL_G3_MIN_CHUNKS");
    const int x = e ? atoi(e) : 64;
    return x < 1 ? 1 : x;
}

// Items per product.  A product's k range is cut so that its items fill at most ONE round of the 256 CUs; below K = 8192
// the cap is 96 (QT_G3_TARGET_ITEMS forces a value for every K): those widths come as batches in practice (3 per Llama
// layer, 10 per Mixtral layer), a batch of n multiplies the items by n, and fewer, longer items mean fewer slabs to
// write and reduce.  K = 4096, cap 256 / 128 / 96 / 64: one chain 2.88 / 2.88 / 2.92 / 3.04 ms, three batched 4.15 / 3.92 /
// 3.84 / 3.59, ten batched 8.67 / 7.63 / 7.30 / 7.15; K = 8192 x 3: 13.4 / 13.6 / 13.8 / 13.4 (no gain: stays at 256).
// The cap is part of the bits and one value for single and batched calls (a batch stays bit-identical to its members).
static int chol_g3_target_items(int K) {
    const char* e = getenv("QT_G3_TARGET_ITEMS");
    if (e && atoi(e) > 0) return atoi(e);
    return K < 8192 ? 96 : 256;
}

// QT_CHOL_MERGE = 0 | order | 1 (read per call).  0: two phases -- the whole factorisation, all diagonal inverses, then
// Y row by row.  order: ONE walk over the block rows -- per row J the two long products, J's panel chain, the plane
// copy of R's row, the inverses of J's diagonal blocks, the Y_JJ recurrence with the transpose and the NEG product, the
// plane copy of Y's row -- with the kernels, tables and arguments of 0: every step reads only what earlier rows (and
// earlier steps of its own) finished, so the bits are those of 0.  1: the walk with the two long products of a row,
//     A[J, J0:] -= R[:J0, J]^T R[:J0, J0:]      and      T_J = R[:J0, J]^T Y[:J0, :J0]
// (one A operand, one k range) as the two segments of ONE gemm3 launch with one item table (g3_plan_row2): together
// they always cover K output columns, so each tile is cut into about half as many pieces and half the slabs are
// written and reduced.  The walk needs the plane products and NBO == NBI; anything else, and a size at which no row
// can be merged (chol_g3_build), runs as 0.
enum { CHOL_TWO_PHASE = 0, CHOL_WALK = 1, CHOL_WALK_MERGED = 2 };
static int chol_merge_mode() {
    const char* e = getenv("QT_CHOL_MERGE");
    if (!e) return CHOL_WALK_MERGED;
    if (strcmp(e, "order") == 0) return CHOL_WALK;
    return atoi(e) != 0 ? CHOL_WALK_MERGED : CHOL_TWO_PHASE;
}

// Host only: the steps and the table bytes of one (K, block sizes, thresholds).  merged: rows where BOTH products have
// a table get one table over both segments instead (pl.row; their fac / inv entries stay empty), cut under the slab
// budget of the separate tables so that the workspace of a size never depends on the switch.
static void chol_g3_build(int K, int NBO, int NBI, int min_chunks, int target_items, bool merged, CholG3Plan& pl,
                          std::vector<char>& bytes) {
    pl = CholG3Plan();
    bytes.clear();
    int slab_budget = 0;
    if (merged) {
        CholG3Plan sep;
        std::vector<char> sep_bytes;
        chol_g3_build(K, NBO, NBI, min_chunks, target_items, false, sep, sep_bytes);
        slab_budget = sep.max_slabs;
    }
    auto enough = [&](int Tm, int Tn, int c_end, int tri) {
        return min_chunks > 0 && K % 8 == 0 && g3_row_chunks(Tm, Tn, c_end, tri) * G3_CHUNK_ROWS >= (long)min_chunks * 128;
    };
    auto store = [&](const std::vector<G3Item>& items, const std::vector<G3Red>& red) {
        G3Step st;
        st.n_items = (int)items.size();
        st.n_red = (int)red.size();
        st.item_off = qt_align_up(bytes.size(), 256);
        bytes.resize(st.item_off + items.size() * sizeof(G3Item));
        memcpy(bytes.data() + st.item_off, items.data(), items.size() * sizeof(G3Item));
        st.red_off = qt_align_up(bytes.size(), 256);
        bytes.resize(st.red_off + red.size() * sizeof(G3Red));
        if (!red.empty()) memcpy(bytes.data() + st.red_off, red.data(), red.size() * sizeof(G3Red));
        for (const G3Red& r : red) pl.max_slabs = pl.max_slabs > r.first + r.count ? pl.max_slabs : r.first + r.count;
        pl.any = true;
        return st;
    };
    auto add = [&](int Tm, int Tn, int c_end, int tri) {
        if (!enough(Tm, Tn, c_end, tri)) return G3Step();
        std::vector<G3Item> items;
        std::vector<G3Red> red;
        g3_plan_row(Tm, Tn, c_end, tri, items, red, target_items);
        return store(items, red);
    };
    const bool walk = merged && NBO == NBI;
    const int cap = target_items > 0 && target_items < 256 ? target_items : 256;   // items per launch, as g3_plan_row
    pl.row.assign(walk ? BlockRow::count(K, NBO) : 0, G3Step());
    std::vector<char> is_merged(pl.row.size(), 0);
    for (BlockRow J(K, NBO); J; ++J) {
        const int Tm = J.Tm(), Tn0 = J.Tn0(), Tn1 = J.Tn1(), c_end = J.c_end();
        // A row is merged only where the cap leaves every tile of the launch at least two pieces: with more tiles than
        // half the cap the pieces become whole tiles and the launch lasts as long as the full k range (K = 28672: 224
        // tiles per 512-row block against a cap of 256 -- one 70B bench run 340.3 -> 345.1 ms per step merged).
        if (walk && J.J0 > 0 && 2 * Tm * (Tn0 + Tn1) <= cap && enough(Tm, Tn0, c_end, 0) && enough(Tm, Tn1, c_end, 1)) {
            std::vector<G3Item> items;
            std::vector<G3Red> red;
            g3_plan_row2(Tm, Tn0, Tn1, c_end, items, red, target_items, slab_budget);
            pl.row[J.Jb] = store(items, red);
            is_merged[J.Jb] = 1;
            pl.any_row = true;
        }
    }
    for (BlockRow J(K, NBO); J; ++J) {
        const bool skip = J.J0 == 0 || (walk && is_merged[J.Jb]);
        pl.fac.push_back(skip ? G3Step() : add(J.Tm(), J.Tn0(), J.c_end(), 0));
    }
    for (BlockRow I(K, NBI); I; ++I) {
        const bool skip = I.J0 == 0 || (walk && is_merged[I.Jb]);
        pl.inv.push_back(skip ? G3Step() : add(I.Tm(), I.Tn1(), I.c_end(), 1));
    }
    pl.blob_bytes = pl.any ? qt_align_up(bytes.size(), 256) : 0;
}

static const CholG3Plan* chol_g3_plan(int K, int NBO, int NBI, bool merged = false) {
    static std::mutex m;
    static std::map<std::tuple<int, int, int, int>, CholG3Plan*> plans;
    const int min_chunks = chol_g3_min_chunks();
    const int target_items = chol_g3_target_items(K);
    std::lock_guard<std::mutex> lock(m);
    const auto key = std::make_tuple(K, NBO, NBI, (merged ? 1 << 30 : 0) + min_chunks * 1024 + target_items);
    auto it = plans.find(key);
    if (it != plans.end()) return it->second;
    CholG3Plan* pl = new CholG3Plan();
    std::vector<char> bytes;
    chol_g3_build(K, NBO, NBI, min_chunks, target_items, merged, *pl, bytes);
    if (pl->any) {
        if (hipHostMalloc((void**)&pl->blob, pl->blob_bytes, hipHostMallocDefault) != hipSuccess) {
            pl->any = false;   // no pinned memory: stay on the f32 path
            pl->blob = nullptr;
        } else {
            memcpy(pl->blob, bytes.data(), bytes.size());
        }
    }
    if (!pl->any) {
        pl->blob_bytes = 0;
        pl->max_slabs = 0;
        for (G3Step& st : pl->fac) st = G3Step();
        for (G3Step& st : pl->inv) st = G3Step();
        for (G3Step& st : pl->row) st = G3Step();
    }
    plans[key] = pl;
    return pl;
}

// block sizes and item tables of one call
static const CholG3Plan* chol_blocks(int K, int& NBO, int& NBI) {
    const int eo = chol_block_env("QT_CHOL_NBO"), ei = chol_block_env("QT_CHOL_NBI");
    NBO = eo ? eo : 512;
    NBI = ei ? ei : 512;
    const CholG3Plan* pl = chol_g3_plan(K, NBO, NBI);
    if (pl->any) return pl;
    NBO = eo ? eo : 256;
    NBI = ei ? ei : 256;
    return chol_g3_plan(K, NBO, NBI);
}

constexpr int LDP = NB + 1;  // padded LDS leading dimension

// ---- panel kernels --------------------------------------------------------------------------
// All three keep a 128-long column in REGISTERS.  Registers cannot be indexed at run time, so a
// column is held as four 32-entry arrays: the 32 steps inside a sub-block are unrolled (static
// indices) and the sub-block loop stays a run-time loop with wave-uniform guards.
constexpr int LDT = NB + 4;  // LDS leading dimension with 16-byte aligned rows

#define QT_SEL4(kb, v0, v1, v2, v3) ((kb) == 0 ? (v0) : (kb) == 1 ? (v1) : (kb) == 2 ? (v2) : (v3))

// potf2: one workgroup (512 threads), Cholesky (upper, A = R^T R) of an n x n block (n <= 128),
// blocked by 32 inside the workgroup so that only 4 x 32 steps are sequential and everything
// else is f32 MFMA on LDS-resident tiles:
//   for kb = 0..3:
//     (i)   wave 0: factor the 32x32 diagonal sub-block with one column per lane in registers;
//           row c reaches the other lanes through v_readlane (no LDS, no barrier), then the
//           32-step back substitution for X_kb = R_kk^-1 the same way;
//     (ii)  R[kb, a] = X_kb^T A[kb, a]           for a > kb          (16 MFMAs per 32x32 tile)
//     (iii) A[a, a'] -= R[kb, a]^T R[kb, a']     for kb < a <= a'
//   P     : input block, upper triangle read, row stride ldp
//   Rout  : receives R (upper triangle written; strict lower untouched), stride ldr
//   Rd    : dense 128x128 row-major copy of R (zeros below the diagonal; identity padding >= n)
//           followed by D32[4][32][32], D32[b][k][i] = X_b[k][i]
//   info  : first non-positive pivot (1-based global index) if any; col0 = global offset
constexpr int LDA = NB + 4;

__device__ __forceinline__ float readlane_f(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// acc (+)= sum_k A[k][i] * B[k][n] over k = 0..31 for one 32x32 tile (TN form, LDS operands)
__device__ __forceinline__ void mma32_tn(const float* A, int lda, const float* B, int ldb, f32x16& acc,
                                         int l31, int h, bool negate_a) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        float a = A[(2 * kk + h) * lda + l31];
        const float b = B[(2 * kk + h) * ldb + l31];
        if (negate_a) a = -a;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
}

// P and Rout may be the same block (the factorisation runs in place): no __restrict__ on them.
constexpr int POTF2_THREADS = 512, POTF2_WAVES = POTF2_THREADS / 64;   // 8 waves: the six trailing tiles of a step in one round
__global__ __launch_bounds__(POTF2_THREADS) void potf2_kernel(const float* P, int64_t ldp, int n,
                                                    float* Rout, int64_t ldr,
                                                    float* __restrict__ Rd, int32_t* info, int col0, int prio,
                                                    int64_t bsP, int64_t bsRd) {
    qt_set_chain_prio(prio);
    if (blockIdx.x) {      // problem b of a batch: one workgroup each
        P += (size_t)blockIdx.x * bsP;
        Rout += (size_t)blockIdx.x * bsP;
        Rd += (size_t)blockIdx.x * bsRd;
        info += blockIdx.x;
    }
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* As = sm;                // [NB][LDA]
    float* Xs = sm + NB * LDA;     // [4][32][32]  Xs[b][k][i] = X_b[k][i]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;

    // Symmetric fill from the upper triangle (identity padding beyond n).  The 16 row-major float4
    // loads of a thread are all issued before the first is used: a load -> wait -> store loop pays one
    // memory round trip per element (64 of them were ~40 % of this kernel).  Needs ldp % 4 == 0 (then
    // n % 4 == 0 too: n is 128 or K % 128) and a 16-byte aligned P; odd K takes the scalar loop.
    if ((ldp & 3) == 0 && (n & 3) == 0 && (((uintptr_t)P) & 15) == 0) {
        constexpr int NV = NB * NB / 4 / POTF2_THREADS;
        f32x4 v[NV];
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const int e4 = tid + POTF2_THREADS * r;       // float4 index in the 128 x 32 grid
            const int i = e4 >> 5, j = (e4 & 31) * 4;
            const int ic = i < n ? i : n - 1, jc = j < n ? j : n - 4;
            v[r] = *(const f32x4*)(P + (size_t)ic * ldp + jc);
        }
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const int e4 = tid + POTF2_THREADS * r;
            const int i = e4 >> 5, j = (e4 & 31) * 4;
            // only the upper triangle is ever read back: (i) takes R[c][i] from lane i's column (i > c), (ii) and
            // (iii) touch blocks on or above the diagonal, and what (i) / (iii) compute below it is never stored.
            // Rows are written whole (float4, conflict-free); the strict lower part just holds the input's values.
            f32x4 x;
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = (i < n && j + q < n) ? v[r][q] : (i == j + q ? 1.0f : 0.0f);
            *(f32x4*)(As + i * LDA + j) = x;
        }
    } else {
        for (int e = tid; e < NB * NB; e += POTF2_THREADS) {
            const int i = e / NB, j = e % NB;
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            float v = (i == j) ? 1.0f : 0.0f;
            if (hi < n) v = P[(size_t)lo * ldp + hi];
            As[i * LDA + j] = v;
        }
    }
    __syncthreads();

    int bad = 0;
#pragma unroll 1
    for (int kb = 0; kb < 4; ++kb) {
        float* Akk = As + (32 * kb) * LDA + 32 * kb;
        // ---- (i) diagonal sub-block: factor AND inverse in one pass, wave 0 ----
        // Lanes 0..31 hold the columns of the 32x32 block, lanes 32..63 the columns of an identity.  One
        // right-looking step c -- rcj = col[c] / r_cc on every lane, then col[i] -= R[c][i] * rcj for i > c
        // with R[c][i] broadcast from lane i -- is the Cholesky step on the left half and the forward
        // substitution R^T Z = I on the right half: the same instructions, so Z = R^-T (= X^T) costs no
        // second 32-step loop.  Afterwards lane j < 32 holds R[i][j] in col[i], lane 32 + j holds X[j][c] in col[c].
        if (wave == 0) {
            // Both 32x32 blocks live in the f32 MFMA's accumulator layout (element (i, j) on lane j + 32 h(i), register
            // rho(i); i = (r & 3) + 8 (r >> 2) + 4 h): C1 = the diagonal block, C2 = an identity.  Step c:
            //     r[.] = C1[c][.] / sqrt(C1[c][c]),  z[.] = C2[c][.] / sqrt(C1[c][c])        (row c, one register of one half)
            //     C1[i][.] -= r[i] r[.],  C2[i][.] -= r[i] z[.]   for i > c                  (ONE MFMA each: a rank-1 update)
            // -- the Cholesky step on C1 and the forward substitution R^T Z = I on C2.  The A operand of both MFMAs is
            // the row itself: lane i + 32 k holds A[i][k], and row c sits on the lanes of half h(c) already, so
            // a = -r on those lanes (zero for i <= c and on the other half, whose k-slice then adds 0 * 0), b = r / z on
            // the same lanes.  Per element that is fmaf(-r_i, r_j, C1[i][j]), the operation of the lane-per-column loop this
            // replaces (31 v_readlane + fma pairs per step: ~6 us per 32x32 block; two MFMAs per step: ~2 us).
            f32x16 c1, c2;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
                c1[r] = Akk[i * LDA + l31];
                c2[r] = (i == l31) ? 1.0f : 0.0f;
            }
#pragma unroll
            for (int c = 0; c < 32; ++c) {
                const int rc = (c & 3) + 4 * (c >> 3);           // register of row c ...
                const int hc = (c >> 2) & 1;                     // ... on the lanes of this half
                float piv = readlane_f(c1[rc], c + 32 * hc);
                const bool isbad = !(piv > 0.0f);
                bad = (isbad && bad == 0 && 32 * kb + c < n) ? 32 * kb + c + 1 : bad;
                piv = isbad ? 1.0f : piv;
                float rs = __builtin_amdgcn_rsqf(piv);
                rs = rs * fmaf(-0.5f * piv * rs, rs, 1.5f);   // one Newton step: the inverse inherits rs
                const bool mine = h == hc;
                const float rr = c1[rc] * rs, zz = c2[rc] * rs;  // row c of R / of Z on the lanes of half hc
                c1[rc] = mine ? rr : c1[rc];
                c2[rc] = mine ? zz : c2[rc];
                if (c < 31) {
                    const float a = (mine && l31 > c) ? -rr : 0.0f;
                    // columns left of the diagonal hold whatever the caller's strict lower triangle held (never
                    // initialised): they must not meet the zero lanes of `a` (0 * NaN would reach finished rows)
                    const float b1 = (mine && l31 >= c) ? rr : 0.0f, b2 = mine ? zz : 0.0f;
                    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, c1, 0, 0, 0);
                    c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b2, c2, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
                Akk[i * LDA + l31] = (i <= l31) ? c1[r] : 0.0f;                       // R_kk, zeros below
                Xs[(kb * 32 + l31) * 32 + i] = (i >= l31) ? c2[r] : 0.0f;             // X[j][c] = Z[c][j]: row c = i, column j = l31
            }
        }
        __syncthreads();
        if (kb == 3) break;
        // ---- (ii) R[kb, a] = X_kb^T A[kb, a], a > kb: one tile per wave (round robin) ----
        for (int a = kb + 1 + wave; a < 4; a += POTF2_WAVES) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            float* Bt = As + (32 * kb) * LDA + 32 * a;
            mma32_tn(Xs + kb * 1024, 32, Bt, LDA, acc, l31, h, false);
#pragma unroll
            for (int r = 0; r < 16; ++r) Bt[((r & 3) + 8 * (r >> 2) + 4 * h) * LDA + l31] = acc[r];
        }
        __syncthreads();
        // ---- (iii) A[a, a'] -= R[kb, a]^T R[kb, a'], kb < a <= a' ----
        {
            int t = 0;
            for (int a = kb + 1; a < 4; ++a)
                for (int a2 = a; a2 < 4; ++a2, ++t) {
                    if ((t % POTF2_WAVES) != wave) continue;
                    float* Ct = As + (32 * a) * LDA + 32 * a2;
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = Ct[((r & 3) + 8 * (r >> 2) + 4 * h) * LDA + l31];
                    mma32_tn(As + (32 * kb) * LDA + 32 * a, LDA, As + (32 * kb) * LDA + 32 * a2, LDA, acc, l31, h,
                             true);
#pragma unroll
                    for (int r = 0; r < 16; ++r) Ct[((r & 3) + 8 * (r >> 2) + 4 * h) * LDA + l31] = acc[r];
                }
        }
        __syncthreads();
    }
    if (bad != 0 && tid == 0) atomicCAS(info, 0, col0 + bad);
    // R out (upper triangle; float4 groups that cross the diagonal carry zeros below it -- nothing reads the
    // strict lower part of a factored diagonal block) and the dense copy for trsm / the block inverses
    const bool vec_out = (ldr & 3) == 0 && (n & 3) == 0 && (((uintptr_t)Rout) & 15) == 0;
    for (int e4 = tid; e4 < NB * NB / 4; e4 += POTF2_THREADS) {
        const int i = e4 >> 5, j = (e4 & 31) * 4;
        f32x4 v = *(const f32x4*)(As + i * LDA + j);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (j + q >= i) ? v[q] : 0.0f;
        *(f32x4*)(Rd + i * NB + j) = v;
        if (i < n && j + 3 >= i && j < n) {
            if (vec_out) {
                *(f32x4*)(Rout + (size_t)i * ldr + j) = v;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (j + q >= i && j + q < n) Rout[(size_t)i * ldr + j + q] = v[q];
            }
        }
    }
    for (int e4 = tid; e4 < 4 * 32 * 32 / 4; e4 += POTF2_THREADS) *(f32x4*)(Rd + NB * NB + 4 * e4) = *(const f32x4*)(Xs + 4 * e4);
}

// trsm: Z = R^-T B for a 128 x ncols panel on the f32 MFMA, by BLOCKED forward substitution
// with the 32x32 inverses X_b of R's diagonal sub-blocks (no divisions, no 128-long chain):
//     Z_b = X_b^T B_b ;   B_a -= R[b, a]^T Z_b   for a > b            (b = 0..3)
// Each wave owns 32 columns and keeps its four 32x32 row-block tiles in accumulators.  A result
// tile feeds the next MFMA directly as its B operand (accumulator register r holds row
// rho(r) = (r&3) + 8*(r>>2) on lanes 0-31 and rho(r)+4 on lanes 32-63, which is just a pairing
// of the k indices: the k order of these sums is free), so Z never round-trips through LDS;
// only the A operands (X_b, -R[b,a], k-major as stored) are read from LDS, one b32 per MFMA.
//   Rd : dense 128x128 R followed by D32[4][32][32], D32[b][k][i] = X_b[k][i] (potf2_kernel)
// B and Z may be the same panel (in place: a thread reads its columns before it writes them).
__global__ __launch_bounds__(256) void trsm_rt_kernel(const float* __restrict__ Rd, int n,
                                                      const float* B, int64_t ldb,
                                                      float* Z, int64_t ldz, int ncols, int prio, int64_t bsRd,
                                                      int64_t bsB) {
    qt_set_chain_prio(prio);
    if (blockIdx.y) {      // problem b of a batch
        Rd += (size_t)blockIdx.y * bsRd;
        B += (size_t)blockIdx.y * bsB;
        Z += (size_t)blockIdx.y * bsB;
    }
    extern __shared__ __attribute__((aligned(16))) float Rs[];  // [RD_STRIDE]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* D32 = Rs + NB * NB;
    const int l31 = lane & 31, h = lane >> 5;
    const int col = blockIdx.x * 128 + wave * 32 + l31;
    const bool cok = col < ncols;
    const int colc = cok ? col : ncols - 1;

    f32x16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;
            acc[a][r] = (row < n) ? B[(size_t)row * ldb + colc] : 0.0f;
        }
    // R block + sub-block inverses into LDS: all 20 float4 loads of a thread in flight before the first is stored.  As a
    // load -> wait -> store loop (what `for (e = tid; ...) Rs[e] = Rd[e]` compiles to) the copy paid 20 memory round trips
    // one after the other -- more than half of this kernel's 17 us (ISA read in round 4; potf2's fill had the same shape).
    {
        constexpr int NV = RD_STRIDE / 4 / 256;
        static_assert(NV * 4 * 256 == RD_STRIDE, "whole float4s per thread");
        f32x4 v[NV];
#pragma unroll
        for (int r = 0; r < NV; ++r) v[r] = ((const f32x4*)Rd)[tid + 256 * r];
#pragma unroll
        for (int r = 0; r < NV; ++r) ((f32x4*)Rs)[tid + 256 * r] = v[r];
    }
    __syncthreads();

#pragma unroll
    for (int b = 0; b < 4; ++b) {
        // Z_b[i][col] = sum_k X_b[k][i] * B_b[k][col]
        f32x16 zb;
#pragma unroll
        for (int r = 0; r < 16; ++r) zb[r] = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
            const float av = D32[(b * 32 + k) * 32 + l31];  // X_b[k][i = l31]
            zb = __builtin_amdgcn_mfma_f32_32x32x2f32(av, acc[b][r], zb, 0, 0, 0);
        }
        acc[b] = zb;
#pragma unroll
        for (int a = b + 1; a < 4; ++a) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float av = -Rs[(32 * b + k) * NB + 32 * a + l31];  // -R[32b+k][32a+i]
                acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, zb[r], acc[a], 0, 0, 0);
            }
        }
    }
    if (cok) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (row < n) Z[(size_t)row * ldz + col] = acc[a][r];
            }
    }
}

// Batched inverse of the diagonal blocks (one workgroup per block, off the factorisation's
// critical path): X = R^-1, thread j < 128 owns column j (x = e_j) and runs the column-oriented
// back substitution p = 127..0: x_p /= R_pp; x_i -= R_ip x_p (i < p), reading column p of R as a
// contiguous row of the transposed LDS copy.
//   Dinv[b]  : R^-1 dense 128x128 row-major (zeros outside the triangle / n)
//   Ydiag(b) : (R^-1)^T dense n x n at Y + (b*128)*(ldy+1) (zeros above the diagonal)
__global__ __launch_bounds__(128) void trinv_batched_kernel(const float* __restrict__ Rd_all, int K,
                                                            float* __restrict__ Dinv_all,
                                                            float* __restrict__ Y, int64_t ldy, int64_t bsW, int64_t bsY,
                                                            int blk0) {
    if (blockIdx.y) {      // problem b of a batch
        Rd_all += (size_t)blockIdx.y * bsW;
        Dinv_all += (size_t)blockIdx.y * bsW;
        Y += (size_t)blockIdx.y * bsY;
    }
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Rt = sm;             // [NB][LDT]  Rt[p][i] = R[i][p]
    float* Xs = sm + NB * LDT;  // [NB][LDP]
    const int b = blk0 + blockIdx.x;   // the launch covers blocks blk0 .. blk0 + gridDim.x - 1
    const int n = (K - b * NB < NB) ? K - b * NB : NB;
    const float* Rd = Rd_all + (size_t)b * RD_STRIDE;
    const int j = threadIdx.x;
    for (int e = j; e < NB * NB; e += NB) {
        const int i = e / NB, c = e % NB;
        Rt[c * LDT + i] = Rd[e];
    }
    __syncthreads();
    float x0[32], x1[32], x2[32], x3[32];
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        x0[r] = (r == j) ? 1.0f : 0.0f;
        x1[r] = (32 + r == j) ? 1.0f : 0.0f;
        x2[r] = (64 + r == j) ? 1.0f : 0.0f;
        x3[r] = (96 + r == j) ? 1.0f : 0.0f;
    }
#pragma unroll 1
    for (int pb = 3; pb >= 0; --pb) {
#pragma unroll
        for (int pp = 31; pp >= 0; --pp) {
            const int p = 32 * pb + pp;
            const float* rp = Rt + p * LDT;  // rp[i] = R[i][p]
            const float xp = QT_SEL4(pb, x0[pp], x1[pp], x2[pp], x3[pp]) / rp[p];
            if (pb == 0) x0[pp] = xp;
            if (pb == 1) x1[pp] = xp;
            if (pb == 2) x2[pp] = xp;
            if (pb == 3) x3[pp] = xp;
#define QT_XUPD(arr, a, r_to)                                                 \
    _Pragma("unroll") for (int r4 = 0; r4 < (r_to); r4 += 4) {                 \
        const f32x4 v4 = *(const f32x4*)(rp + 32 * (a) + r4);                 \
        _Pragma("unroll") for (int e = 0; e < 4; ++e)                         \
            if (r4 + e < (r_to)) arr[r4 + e] = fmaf(-v4[e], xp, arr[r4 + e]); \
    }
            if (pb == 0) { QT_XUPD(x0, 0, pp) } else { QT_XUPD(x0, 0, 32) }
            if (pb == 1) { QT_XUPD(x1, 1, pp) } else if (pb > 1) { QT_XUPD(x1, 1, 32) }
            if (pb == 2) { QT_XUPD(x2, 2, pp) } else if (pb > 2) { QT_XUPD(x2, 2, 32) }
            if (pb == 3) { QT_XUPD(x3, 3, pp) }
#undef QT_XUPD
        }
    }
#pragma unroll
    for (int r = 0; r < 32; ++r) {
        Xs[r * LDP + j] = x0[r];
        Xs[(32 + r) * LDP + j] = x1[r];
        Xs[(64 + r) * LDP + j] = x2[r];
        Xs[(96 + r) * LDP + j] = x3[r];
    }
    __syncthreads();
    float* Dinv = Dinv_all + (size_t)b * NB * NB;
    float* Yd = Y + (size_t)(b * NB) * ldy + b * NB;
    for (int e = j; e < NB * NB; e += NB) {
        const int i = e / NB, jj = e % NB;
        const bool in = (i < n && jj < n);
        Dinv[e] = (in && jj >= i) ? Xs[i * LDP + jj] : 0.0f;
        if (in) Yd[(size_t)i * ldy + jj] = (jj <= i) ? Xs[jj * LDP + i] : 0.0f;
    }
}

// The same outputs on the f32 MFMA (round 4; QT_CHOL_TRINV=div selects the kernel above): Z = R^-T I by trsm_rt_kernel's
// blocked forward substitution with the 32x32 inverses potf2 already computed -- four stages of MFMAs instead of 128
// sequential divide-and-update steps (97 -> ~20 us per launch at K = 4096, 137 -> ~25 at K = 14336; one launch per chain).
// Z is lower triangular: Ydiag(b) = Z, Dinv[b] = Z^T.  Wave w owns the columns 32w .. 32w + 31 of the identity.
__global__ __launch_bounds__(256) void trinv_mfma_kernel(const float* __restrict__ Rd_all, int K,
                                                         float* __restrict__ Dinv_all,
                                                         float* __restrict__ Y, int64_t ldy, int64_t bsW, int64_t bsY,
                                                         int blk0) {
    if (blockIdx.y) {      // problem b of a batch
        Rd_all += (size_t)blockIdx.y * bsW;
        Dinv_all += (size_t)blockIdx.y * bsW;
        Y += (size_t)blockIdx.y * bsY;
    }
    extern __shared__ __attribute__((aligned(16))) float Rs[];  // [RD_STRIDE]
    const int blk = blk0 + blockIdx.x;   // the launch covers blocks blk0 .. blk0 + gridDim.x - 1
    const int n = (K - blk * NB < NB) ? K - blk * NB : NB;
    const float* Rd = Rd_all + (size_t)blk * RD_STRIDE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {   // as in trsm_rt_kernel: every load of the copy in flight before the first store
        constexpr int NV = RD_STRIDE / 4 / 256;
        f32x4 v[NV];
#pragma unroll
        for (int r = 0; r < NV; ++r) v[r] = ((const f32x4*)Rd)[tid + 256 * r];
#pragma unroll
        for (int r = 0; r < NV; ++r) ((f32x4*)Rs)[tid + 256 * r] = v[r];
    }
    const float* D32 = Rs + NB * NB;
    const int l31 = lane & 31, h = lane >> 5;
    const int col = wave * 32 + l31;

    f32x16 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;
            acc[a][r] = (row == col) ? 1.0f : 0.0f;
        }
    __syncthreads();

#pragma unroll
    for (int b = 0; b < 4; ++b) {
        f32x16 zb;
#pragma unroll
        for (int r = 0; r < 16; ++r) zb[r] = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
            const float av = D32[(b * 32 + k) * 32 + l31];  // X_b[k][i = l31]
            zb = __builtin_amdgcn_mfma_f32_32x32x2f32(av, acc[b][r], zb, 0, 0, 0);
        }
        acc[b] = zb;
#pragma unroll
        for (int a = b + 1; a < 4; ++a) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = (r & 3) + 8 * (r >> 2) + 4 * h;
                const float av = -Rs[(32 * b + k) * NB + 32 * a + l31];  // -R[32b+k][32a+i]
                acc[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, zb[r], acc[a], 0, 0, 0);
            }
        }
    }
    float* Dinv = Dinv_all + (size_t)blk * NB * NB;
    float* Yd = Y + (size_t)(blk * NB) * ldy + blk * NB;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * a + (r & 3) + 8 * (r >> 2) + 4 * h;
            const bool in = row < n && col < n;
            const float z = (in && row >= col) ? acc[a][r] : 0.0f;      // Z[row][col] = (R^-1)[col][row]
            Dinv[col * NB + row] = z;
            if (in) Yd[(size_t)row * ldy + col] = z;
        }
}

// XT[k][m] = Y_II[m][k] for a w x w diagonal block of the lower-triangular Y (entries above the diagonal
// of Y are not initialised outside the 128-blocks on the diagonal: written as zeros here)
__global__ __launch_bounds__(256) void transpose_lower_block_kernel(const float* __restrict__ Y, int64_t ldy, int w,
                                                                    float* __restrict__ XT, int ldx, int64_t bsY,
                                                                    int64_t bsXT) {
    if (blockIdx.z) {
        Y += (size_t)blockIdx.z * bsY;
        XT += (size_t)blockIdx.z * bsXT;
    }
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;   // XT rows k = by.., cols m = bx..
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int m = bx + r, k = by + tx;                   // read Y_II[m][k], coalesced along k
        tile[r][tx] = (m < w && k < w && k <= m) ? Y[(size_t)m * ldy + k] : 0.0f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int k = by + r, m = bx + tx;
        if (k < w && m < w) XT[(size_t)k * ldx + m] = tile[tx][r];
    }
}

// In-place flat reversal of the lower-triangular Y into the upper-triangular U:
// U[i][j] = Y[K-1-i][K-1-j] for j >= i, strict lower triangle of U = 0.
__global__ __launch_bounds__(256) void flat_reverse_lower_to_upper_kernel(float* __restrict__ U, int K, int64_t bsU) {
    U += (size_t)blockIdx.z * bsU;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= K || j < i) return;
    const size_t e = (size_t)i * K + j;
    const size_t pe = (size_t)(K - 1 - i) * K + (K - 1 - j);
    if (i == j) {
        if (e <= pe) {
            const float t = U[e];
            U[e] = U[pe];
            U[pe] = t;
        }
    } else {
        U[e] = U[pe];
        U[pe] = 0.0f;
    }
}

// Upstream's LinAlgError fallback, applied on the device so the host need not synchronise:
// if the factorisation hit a non-positive pivot, U = I (plain round-to-nearest).
__global__ __launch_bounds__(256) void identity_if_failed_kernel(float* __restrict__ U, int K,
                                                                 const int32_t* __restrict__ info, int64_t bsU) {
    // a fixed, small grid striding over the rows: in the normal case (info == 0) every workgroup leaves at once, and a
    // launch of K * K / 256 workgroups that all do so took 141 us at K = 14336 (16 us at K = 4096) for nothing
    if (info[blockIdx.z] == 0) return;
    U += (size_t)blockIdx.z * bsU;
    for (int i = blockIdx.x; i < K; i += gridDim.x)
        for (int j = threadIdx.x; j < K; j += blockDim.x) U[(size_t)i * K + j] = (i == j) ? 1.0f : 0.0f;
}

// Scale exponents of the two-fp16-plane products, one workgroup per problem: e[b] = eR = 3 - ceil(log2 sqrt(max diag A_b)),
// e[nprob + b] = eY = 3 - ceil(log2(1 / sqrt(min_eig_lb[b]))), clamped to +-G3_E_MAX.  A bound that is not a positive
// finite number cannot scale Y: the problem is flagged in info (K + 1) and ends as U = I, like a failed pivot.  A
// diagonal that is not positive belongs to a matrix potf2 will reject; its planes may hold anything.
__global__ __launch_bounds__(256) void chol_scales_kernel(const float* __restrict__ A, int64_t bsA, int K,
                                                          const float* __restrict__ min_eig_lb, int32_t* __restrict__ e,
                                                          int32_t* __restrict__ info) {
    __shared__ float red[256];
    const int b = blockIdx.x, nprob = gridDim.x;
    const float* Ab = A + (size_t)b * bsA;
    float m = 0.0f;
    for (int i = threadIdx.x; i < K; i += 256) m = fmaxf(m, Ab[(size_t)i * K + i]);   // fmaxf drops NaNs
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        auto clampe = [](float t) { return (int)fminf(fmaxf(t, (float)-G3_E_MAX), (float)G3_E_MAX); };
        const float d = red[0], lb = min_eig_lb[b];
        e[b] = (d > 0.0f && d < 3.0e38f) ? clampe(3.0f - ceilf(0.5f * log2f(d))) : 0;
        if (lb > 0.0f && lb < 3.0e38f) {
            e[nprob + b] = clampe(3.0f - ceilf(-0.5f * log2f(lb)));
        } else {
            e[nprob + b] = 0;
            info[b] = K + 1;
        }
    }
}

}  // namespace

// ---- host side: workspace, context, the steps, the two schedules ----------------------------

// ONE problem's share of the workspace as the plan g3 sizes it; a batch's is CholLayout::batch_bytes
static CholLayout chol_layout(int K, const CholG3Plan* g3) { return CholLayout(K, g3->any, g3->max_slabs); }

extern "C" size_t qt_cholesky_inverse_upper_batched_workspace_bytes(int K, int n_problems) {
    if (K <= 0 || n_problems <= 0) return 0;
    int nbo_, nbi_;
    const CholG3Plan* g3 = chol_blocks(K, nbo_, nbi_);
    return chol_layout(K, g3).batch_bytes(n_problems, g3->blob_bytes);
}

extern "C" size_t qt_cholesky_inverse_upper_workspace_bytes(int K) {
    return qt_cholesky_inverse_upper_batched_workspace_bytes(K, 1);
}

constexpr size_t INV_LDS = (size_t)(NB * LDT + NB * LDP) * sizeof(float);
constexpr size_t POTF2_LDS = (size_t)(NB * LDA + 4 * 32 * 32) * sizeof(float);
constexpr size_t RD_LDS = RD_STRIDE * sizeof(float);   // trsm_rt_kernel, trinv_mfma_kernel: one Rd block

// What every step of one call reads.  n problems of one size K in every launch of the chain: problem b's matrices at
// A + b * sA, Y + b * sY (elements), its share of the workspace at + b * sW, its pivot flag at info[b].
struct CholCtx {
    float *A, *Y;              // A: the input, R in place; Y = U: R^-T (lower) until the closing reversal
    int K, nprob, NBO, NBI;
    int64_t sA, sY, sW;        // batch strides in floats (sA, sY: 0 for one problem; sW: one problem's workspace)
    float *T, *TI, *XT, *Rd, *Dinv, *split_ws;   // CholLayout's regions in problem 0's share
    size_t split_ws_bytes;
    // bf16x3 products: plane copies of R and Y, slabs (per problem), item tables (one copy for the batch)
    unsigned short *Rpl, *Ypl;
    int64_t plane_stride;
    float* g3_slabs;
    char* g3_tab;
    const CholG3Plan* g3;      // sizes the workspace, whatever QT_CHOL_MERGE says
    const CholG3Plan* tab;     // the tables the launches use
    int planes;                // G3_BF16X3 | G3_F16X2
    int merge_mode;            // CHOL_TWO_PHASE | CHOL_WALK | CHOL_WALK_MERGED
    int32_t *info, *eR, *eY;   // eR, eY (G3_F16X2): the scale exponents, [nprob] each
    int prio;
    hipStream_t stream;
};

// The plane mode and the schedule of one call, from the arguments and the environment (read per call).
// min_eig_lb (device, one per problem; may be null): see the head of the file.  QT_CHOL_PLANES=bf16x3|f16x2 forces a plane
// mode (A/B runs): bf16x3 ignores the bound, f16x2 without one is an argument error.
static int chol_resolve(CholCtx& c, const float* min_eig_lb) {
    bool f16x2 = min_eig_lb != nullptr;
    if (const char* e = getenv("QT_CHOL_PLANES")) {
        if (strcmp(e, "bf16x3") == 0) f16x2 = false;
        else if (strcmp(e, "f16x2") == 0) {
            QT_CHECK_ARG(min_eig_lb, "qt_cholesky_inverse_upper: QT_CHOL_PLANES=f16x2 needs a bound on lambda_min (the _bounded entry points)");
        } else {
            QT_CHECK_ARG(false, "qt_cholesky_inverse_upper: QT_CHOL_PLANES=%s (bf16x3 | f16x2)", e);
        }
    }
    c.g3 = chol_blocks(c.K, c.NBO, c.NBI);
    c.planes = (f16x2 && c.g3->any) ? G3_F16X2 : G3_BF16X3;
    c.merge_mode = (c.g3->any && c.NBO == c.NBI) ? chol_merge_mode() : CHOL_TWO_PHASE;
    c.tab = c.g3;
    if (c.merge_mode == CHOL_WALK_MERGED) {
        c.tab = chol_g3_plan(c.K, c.NBO, c.NBI, true);
        // by construction the merged tables need no more slabs and no more table bytes than the separate ones
        // (a size with no merged row keeps the two phases: the walk alone buys nothing)
        if (!c.tab->any || !c.tab->any_row || c.tab->max_slabs > c.g3->max_slabs || c.tab->blob_bytes > c.g3->blob_bytes) {
            c.tab = c.g3;
            c.merge_mode = CHOL_TWO_PHASE;
        }
    }
    return QT_OK;
}

// Where an operand of a chain product lives decides its batch stride: in the matrix A (R, in place), in the matrix Y
// (= U), or in the problem's share of the workspace (T, T_I, X_II, Dinv).
enum CholHome { IN_A, IN_Y, IN_WS };
struct CholOperand { float* p; int64_t ld; CholHome home; };
static int64_t chol_stride(const CholCtx& c, CholHome h) { return h == IN_A ? c.sA : h == IN_Y ? c.sY : c.sW; }

// An f32 product of the chain, for all problems:  C (mode) A^T B  with A [kdim][M], B [kdim][N].  SG_MODE_SUB works in
// place on C; SET and NEG only write it.  offer_split: the product may take the split-K slabs -- the two long block-row
// products alone (fac_product, inv_product): a split changes the order of a sum, so the offer is part of the bits.
static SgemmArgs chol_sgemm_args(const CholCtx& c, CholOperand A, CholOperand B, CholOperand C, int M, int N, int kdim,
                                 int k_mode, int mode, bool offer_split) {
    SgemmArgs g;
    g.A = A.p; g.lda = A.ld;
    g.B = B.p; g.ldb = B.ld;
    g.Cin = mode == SG_MODE_SUB ? C.p : nullptr; g.ldcin = mode == SG_MODE_SUB ? C.ld : 0;
    g.Cout = C.p; g.ldcout = C.ld;
    g.M = M; g.N = N; g.kdim = kdim; g.k_mode = k_mode; g.mode = mode;
    g.split_ws = offer_split ? c.split_ws : nullptr; g.split_ws_bytes = offer_split ? c.split_ws_bytes : 0;
    g.batch = c.nprob;
    g.bsA = chol_stride(c, A.home); g.bsB = chol_stride(c, B.home); g.bsCin = g.bsCout = chol_stride(c, C.home);
    g.bs_split = c.sW;
    return g;
}

// A block-row product on the plane copies:  C[M][N] (mode) R[:k, col_a0:]^T B[:k, col_b0:]  with the items of st.
// second: the launch also carries segment 1 of a merged row, T_J = R[:J0, J]^T Y[:J0, :J0] -> TI (G3Args)
static int g3_row(const CholCtx& c, const G3Step& st, const unsigned short* Bplanes, int col_a0, int col_b0, int M, int N,
                  float* C, CholHome c_home, int mode, bool second = false) {
    G3Args a;
    a.Apl = c.Rpl; a.Bpl = Bplanes; a.plane_stride = c.plane_stride; a.ld = c.K;
    a.rowA0 = a.rowB0 = 0; a.colA0 = col_a0; a.colB0 = col_b0; a.colmax = c.K;
    a.M = M; a.N = N; a.C = C; a.ldc = c.K; a.mode = mode;
    a.slabs = c.g3_slabs;
    a.items = (const G3Item*)(c.g3_tab + st.item_off); a.n_items = st.n_items;
    a.red = (const G3Red*)(c.g3_tab + st.red_off); a.n_red = st.n_red;
    a.batch = c.nprob;
    a.bsApl = a.bsBpl = c.sW * 2;       // plane copies live in the problem's workspace (bf16 elements)
    a.bsC = chol_stride(c, c_home); a.bsSlabs = c.sW;
    if (c.planes == G3_F16X2) {
        a.planes = G3_F16X2; a.eA = c.eR; a.eB = Bplanes == c.Rpl ? c.eR : c.eY;
    }
    if (second) {
        a.Bpl1 = c.Ypl; a.colB01 = 0; a.eB1 = c.eY;
        a.C1 = c.TI; a.ldc1 = c.K; a.bsC1 = c.sW; a.mode1 = G3_SET;
        a.N1 = col_a0;   // J0 columns
    }
    return qt_gemm3_launch(a, c.stream);
}

// ---- A = R^T R over NBO-wide outer blocks, left-looking inside one; in place.  Outer level: right-looking
// (one k = NBO update of the trailing matrix per block) on the f32 MFMA, or -- when the bf16x3 products
// are in use for this K -- left-looking (block row J gathers all earlier block rows in one long-k product)
// A[J, J0:] -= R[:J0, J]^T R[:J0, J0:]
static int fac_product(const CholCtx& c, const BlockRow& J) {
    if (!(c.g3->any && J.J0 > 0)) return QT_OK;
    const int K = c.K, J0 = J.J0;
    const G3Step& st = c.tab->fac[J.Jb];
    float* C = c.A + (size_t)J0 * K + J0;
    if (st.n_items > 0) return g3_row(c, st, c.Rpl, J0, J0, J.rows(), K - J0, C, IN_A, G3_SUB);
    const CholOperand RJ = {c.A + J0, K, IN_A};   // R[:J0, J0:]
    return qt_sgemm_tn(chol_sgemm_args(c, RJ, RJ, {C, K, IN_A}, J.rows(), K - J0, J0, SG_K_FULL, SG_MODE_SUB, true), c.stream);
}

// the panel chain of block row J, then its plane copies (or the right-looking update)
static int fac_panels(const CholCtx& c, const BlockRow& J) {
    const int K = c.K, J0 = J.J0, J1 = J.J1, nprob = c.nprob;
    float* A = c.A;
    for (int j0 = J0; j0 < J1; j0 += NB) {
        const int j = j0 / NB, nbj = (K - j0 < NB) ? K - j0 : NB;
        float* Ajj = A + (size_t)j0 * K + j0;
        if (j0 > J0) {
            // rows J0..j0 of this outer block are final: fold them into block row j
            const CholOperand Rj = {A + (size_t)J0 * K + j0, K, IN_A};
            int rc = qt_sgemm_tn(chol_sgemm_args(c, Rj, Rj, {Ajj, K, IN_A}, nbj, K - j0, j0 - J0, SG_K_FULL, SG_MODE_SUB, false),
                                 c.stream);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(potf2_kernel, dim3(nprob), dim3(POTF2_THREADS), POTF2_LDS, c.stream, (const float*)Ajj, (int64_t)K, nbj,
                           Ajj, (int64_t)K, c.Rd + (size_t)j * RD_STRIDE, c.info, j0, c.prio, c.sA, c.sW);
        QT_LAUNCH_CHECK();
        const int rest = K - j0 - nbj;
        if (rest > 0) {
            hipLaunchKernelGGL(trsm_rt_kernel, dim3((rest + 127) / 128, nprob), dim3(256), RD_LDS, c.stream,
                               (const float*)(c.Rd + (size_t)j * RD_STRIDE), nbj, (const float*)(Ajj + nbj), (int64_t)K,
                               Ajj + nbj, (int64_t)K, rest, c.prio, c.sW, c.sA);
            QT_LAUNCH_CHECK();
        }
    }
    const int rem = K - J1;
    if (c.g3->any) {
        // plane copies of the finished block row (columns from its diagonal block on; only entries above
        // the diagonal are ever read back).  The factorisation never reads the last block row's; the inverse does
        // where one of its block rows starts inside it (QT_CHOL_NBI not a multiple of QT_CHOL_NBO): T_I takes R[:I0, I].
        if (rem > 0 || (K - 1) / c.NBI * c.NBI > J0) {
            float* RJ = A + (size_t)J0 * K + J0;
            unsigned short* pl = c.Rpl + (size_t)J0 * K + J0;
            int rc = c.planes == G3_F16X2
                         ? qt_split2h_launch(RJ, K, J1 - J0, K - J0, pl, K, c.plane_stride, 0, 0, 0, c.eR, c.stream, nprob, c.sA, c.sW * 2)
                         : qt_split3_launch(RJ, K, J1 - J0, K - J0, pl, K, c.plane_stride, 0, 0, 0, c.stream, nprob, c.sA, c.sW * 2);
            if (rc) return rc;
        }
    } else if (rem > 0) {
        // the K^3/3 of the factorisation: one SYRK-shaped update per outer block, upper tiles only
        const CholOperand RJ = {A + (size_t)J0 * K + J1, K, IN_A};
        SgemmArgs g = chol_sgemm_args(c, RJ, RJ, {A + (size_t)J1 * K + J1, K, IN_A}, rem, rem, J1 - J0, SG_K_FULL, SG_MODE_SUB, false);
        g.upper_only = 1;
        int rc = qt_sgemm_tn(g, c.stream);
        if (rc) return rc;
    }
    return QT_OK;
}

// the inverses of the 128x128 diagonal blocks blk0 .. blk0 + n - 1
static int trinv(const CholCtx& c, int blk0, int n) {
    const char* e = getenv("QT_CHOL_TRINV");   // read per call: the tests compare the two kernels in one process
    if (e && strcmp(e, "div") == 0)
        hipLaunchKernelGGL(trinv_batched_kernel, dim3(n, c.nprob), dim3(NB), INV_LDS, c.stream, (const float*)c.Rd, c.K, c.Dinv,
                           c.Y, (int64_t)c.K, c.sW, c.sY, blk0);
    else
        hipLaunchKernelGGL(trinv_mfma_kernel, dim3(n, c.nprob), dim3(256), RD_LDS, c.stream, (const float*)c.Rd, c.K, c.Dinv,
                           c.Y, (int64_t)c.K, c.sW, c.sY, blk0);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

// ---- Y = R^-T by NBI-row block rows ----
// left of the diagonal block: the K^3/3 of the inverse, one product per block row:  T_I = R[:I0, I]^T Y[:I0, :I0]
static int inv_product(const CholCtx& c, const BlockRow& I) {
    const int K = c.K, I0 = I.J0;
    if (I0 == 0) return QT_OK;
    if (c.g3->any && c.tab->inv[I.Jb].n_items > 0) return g3_row(c, c.tab->inv[I.Jb], c.Ypl, I0, 0, I.rows(), I0, c.TI, IN_WS, G3_SET);
    return qt_sgemm_tn(chol_sgemm_args(c, {c.A + I0, K, IN_A}, {c.Y, K, IN_Y}, {c.TI, K, IN_WS}, I.rows(), I0, I0, SG_K_FROM_N0,
                                       SG_MODE_SET, true),
                       c.stream);
}

// plane copy of the finished block row of Y (zeros above the diagonal), for the later rows' products
static int split_row(const CholCtx& c, const BlockRow& I) {
    const int K = c.K, I0 = I.J0;
    if (!c.g3->any || I.J1 >= K) return QT_OK;
    // up to the end of the row's last 256-column tile: a later product starts tile column tj's k range at row 256 tj
    // and reads whole tile columns, so a row that ends inside one (QT_CHOL_NBI = 128) owes it the zeros above the diagonal
    const int tile_end = (I.J1 + CHOL_TILE - 1) / CHOL_TILE * CHOL_TILE, cols = tile_end < K ? tile_end : K;
    if (c.planes == G3_F16X2)
        return qt_split2h_launch(c.Y + (size_t)I0 * K, K, I.rows(), cols, c.Ypl + (size_t)I0 * K, K, c.plane_stride, 1, I0, 0, c.eY,
                                 c.stream, c.nprob, c.sY, c.sW * 2);
    return qt_split3_launch(c.Y + (size_t)I0 * K, K, I.rows(), cols, c.Ypl + (size_t)I0 * K, K, c.plane_stride, 1, I0, 0, c.stream,
                            c.nprob, c.sY, c.sW * 2);
}

// the rest of block row I: Y_II, then Y[I, :I0] = -Y_II T_I from the T_I the product left in TI, then the plane copy
static int inv_row(const CholCtx& c, const BlockRow& I) {
    const int K = c.K, I0 = I.J0, I1 = I.J1, Wi = I.rows();
    float* Y = c.Y;
    // the diagonal 512-block Y_II by the 128-row recurrence (short k)
    for (int i0 = I0 + NB; i0 < I1; i0 += NB) {
        const int i = i0 / NB, nbi = (K - i0 < NB) ? K - i0 : NB;
        const CholOperand Yi = {Y + (size_t)i0 * K + I0, K, IN_Y}, Tp = {c.T, K, IN_WS};
        int rc = qt_sgemm_tn(chol_sgemm_args(c, {c.A + (size_t)I0 * K + i0, K, IN_A}, {Y + (size_t)I0 * K + I0, K, IN_Y}, Tp, nbi,
                                             i0 - I0, i0 - I0, SG_K_FROM_N0, SG_MODE_SET, false),
                             c.stream);
        if (rc) return rc;
        rc = qt_sgemm_tn(chol_sgemm_args(c, {c.Dinv + (size_t)i * NB * NB, NB, IN_WS}, Tp, Yi, nbi, i0 - I0, nbi, SG_K_FULL,
                                         SG_MODE_NEG, false),
                         c.stream);
        if (rc) return rc;
    }
    if (I0 == 0) return split_row(c, I);
    hipLaunchKernelGGL(transpose_lower_block_kernel, dim3((Wi + 31) / 32, (Wi + 31) / 32, c.nprob), dim3(256), 0, c.stream,
                       (const float*)(Y + (size_t)I0 * K + I0), (int64_t)K, Wi, c.XT, NBO_MAX, c.sY, c.sW);
    QT_LAUNCH_CHECK();
    int rc = qt_sgemm_tn(chol_sgemm_args(c, {c.XT, NBO_MAX, IN_WS}, {c.TI, K, IN_WS}, {Y + (size_t)I0 * K, K, IN_Y}, Wi, I0, Wi,
                                         SG_K_FULL, SG_MODE_NEG, false),
                         c.stream);
    if (rc) return rc;
    return split_row(c, I);
}

// QT_CHOL_MERGE=0: the whole factorisation, all diagonal-block inverses at once, then Y row by row
static int chol_run_two_phase(const CholCtx& c) {
    for (BlockRow J(c.K, c.NBO); J; ++J) {
        int rc = fac_product(c, J);
        if (!rc) rc = fac_panels(c, J);
        if (rc) return rc;
    }
    int rc = trinv(c, 0, (c.K + NB - 1) / NB);
    if (rc) return rc;
    for (BlockRow I(c.K, c.NBI); I; ++I) {
        rc = inv_product(c, I);
        if (!rc) rc = inv_row(c, I);
        if (rc) return rc;
    }
    return QT_OK;
}

// one walk over the block rows (NBO == NBI): see chol_merge_mode()
static int chol_run_walk(const CholCtx& c) {
    for (BlockRow J(c.K, c.NBO); J; ++J) {
        int rc;
        if (c.merge_mode == CHOL_WALK_MERGED && c.tab->row[J.Jb].n_items > 0) {
            rc = g3_row(c, c.tab->row[J.Jb], c.Rpl, J.J0, J.J0, J.rows(), c.K - J.J0, c.A + (size_t)J.J0 * c.K + J.J0, IN_A, G3_SUB,
                        /*second=*/true);
        } else {
            rc = fac_product(c, J);
            if (!rc) rc = inv_product(c, J);
        }
        if (!rc) rc = fac_panels(c, J);
        if (!rc) rc = trinv(c, J.J0 / NB, (J.rows() + NB - 1) / NB);
        if (!rc) rc = inv_row(c, J);
        if (rc) return rc;
    }
    return QT_OK;
}

// the panel kernels' dynamic LDS beyond the default limit, asked for once per device
static hipError_t chol_lds_attrs() {
    static QtOncePerDevice lds_attr;
    return lds_attr.run([] {
        const auto attr = hipFuncAttributeMaxDynamicSharedMemorySize;
        hipError_t e = hipFuncSetAttribute((const void*)potf2_kernel, attr, (int)POTF2_LDS);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)trsm_rt_kernel, attr, (int)RD_LDS);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)trinv_batched_kernel, attr, (int)INV_LDS);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)trinv_mfma_kernel, attr, (int)RD_LDS);
        return e;
    });
}

// n problems of one size K in every launch of the chain: problem b's matrices at A + b * strideA, U + b * strideU
// (elements), its pivot flag at info[b].  Per problem the kernels, their launch shapes and the order of every sum are
// those of a single-problem call (tile sizes and split-K decisions come from one problem's shape), so the factors are
// bit-identical to n separate calls; what changes is that the latency-bound panel kernels (potf2: ONE workgroup per
// problem; trsm, the short folds) and the block-row products serve all n problems per launch.
static int chol_run(float* A, int64_t strideA, int K, float* U, int64_t strideU, int32_t* info, int nprob, void* workspace,
                    size_t workspace_bytes, hipStream_t stream, const float* min_eig_lb = nullptr) {
    CholCtx c = {};
    c.A = A; c.Y = U; c.K = K; c.nprob = nprob; c.info = info; c.stream = stream;
    if (int rc = chol_resolve(c, min_eig_lb)) return rc;
    const CholLayout L = chol_layout(K, c.g3);
    const size_t need = L.batch_bytes(nprob, c.g3->blob_bytes);
    if (!workspace || workspace_bytes < need) {
        qt_set_error("qt_cholesky_inverse_upper: workspace %zu < required %zu", workspace_bytes, need);
        return QT_ERR_WORKSPACE;
    }
    char* ws = (char*)qt_align_up((size_t)workspace, 256);
    c.sW = (int64_t)(L.bytes() / 4); c.sA = nprob > 1 ? strideA : 0; c.sY = nprob > 1 ? strideU : 0;
    c.T = (float*)(ws + L.T); c.TI = (float*)(ws + L.TI); c.XT = (float*)(ws + L.XT);
    c.Rd = (float*)(ws + L.Rd); c.Dinv = (float*)(ws + L.Dinv);
    c.split_ws = (float*)(ws + L.split); c.split_ws_bytes = L.split_bytes;
    c.plane_stride = (int64_t)K * K;
    if (c.g3->any) {
        c.Rpl = (unsigned short*)(ws + L.Rpl); c.Ypl = (unsigned short*)(ws + L.Ypl);
        c.g3_slabs = (float*)(ws + L.slabs); c.g3_tab = ws + L.tables(nprob);
        QT_HIP(hipMemcpyAsync(c.g3_tab, c.tab->blob, c.tab->blob_bytes, hipMemcpyHostToDevice, stream));
    }
    // two fp16 planes use the first two plane slots; the scale exponents eR[nprob], eY[nprob] sit in problem 0's third
    static_assert(2 * SG_MAX_BATCH * sizeof(int32_t) <= (size_t)NB * NB * 2, "the exponents fit the smallest third plane");
    c.eR = c.planes == G3_F16X2 ? (int32_t*)(c.Rpl + 2 * c.plane_stride) : nullptr;
    c.eY = c.planes == G3_F16X2 ? c.eR + nprob : nullptr;
    QT_HIP(chol_lds_attrs());
    QT_HIP(hipMemsetAsync(info, 0, sizeof(int32_t) * nprob, stream));
    c.prio = qt_chain_prio();
    if (c.planes == G3_F16X2) {
        hipLaunchKernelGGL(chol_scales_kernel, dim3(nprob), dim3(256), 0, stream, (const float*)A, c.sA, K, min_eig_lb, c.eR, info);
        QT_LAUNCH_CHECK();
    }
    if (int rc = c.merge_mode == CHOL_TWO_PHASE ? chol_run_two_phase(c) : chol_run_walk(c)) return rc;
    hipLaunchKernelGGL(flat_reverse_lower_to_upper_kernel, dim3((K + 255) / 256, K, nprob), dim3(256), 0, stream, U, K, c.sY);
    QT_LAUNCH_CHECK();
    hipLaunchKernelGGL(identity_if_failed_kernel, dim3(K < 1024 ? K : 1024, 1, nprob), dim3(256), 0, stream, U, K,
                       (const int32_t*)info, c.sY);
    QT_LAUNCH_CHECK();
    return QT_OK;
}

// The batched entry points' argument checks (fn: the entry point, for the message; ptrs: its pointers are all there).
static int chol_check_batch(const char* fn, bool ptrs, int K, int n_problems, int64_t strideA, int64_t strideU) {
    QT_CHECK_ARG(K > 0 && ptrs && n_problems >= 1 && n_problems <= SG_MAX_BATCH, "%s: bad arguments (1 <= n_problems <= %d)", fn,
                 SG_MAX_BATCH);
    QT_CHECK_ARG(n_problems == 1 || (strideA >= (int64_t)K * K && strideU >= (int64_t)K * K && strideA % 4 == 0 && strideU % 4 == 0),
                 "%s: strides must be multiples of 4 elements and >= K*K", fn);
    return QT_OK;
}

extern "C" int qt_cholesky_inverse_upper(float* A, int K, float* U, int32_t* info, void* workspace,
                                         size_t workspace_bytes, qt_stream_t stream_) {
    QT_CHECK_ARG(K > 0 && A && U && info, "qt_cholesky_inverse_upper: bad arguments");
    return chol_run(A, 0, K, U, 0, info, 1, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int qt_cholesky_inverse_upper_batched(float* A, int64_t strideA, int K, float* U, int64_t strideU, int32_t* info,
                                                 int n_problems, void* workspace, size_t workspace_bytes,
                                                 qt_stream_t stream_) {
    if (int rc = chol_check_batch("qt_cholesky_inverse_upper_batched", A && U && info, K, n_problems, strideA, strideU)) return rc;
    return chol_run(A, strideA, K, U, strideU, info, n_problems, workspace, workspace_bytes, (hipStream_t)stream_);
}

// The same with a lower bound on lambda_min(A) per problem (device, fp32; for a Gram matrix plus damp * I any value <=
// damp, with a binade of margin for the rounding of the Gram sum): where the chain runs its block-row products on the
// matrix pipe they take two fp16 planes and three plane products instead of three bf16 planes and six.  A bound that is
// not positive and finite fails its problem (info = K + 1, U = I).  No host synchronisation.
extern "C" int qt_cholesky_inverse_upper_bounded(float* A, int K, float* U, int32_t* info, const float* min_eig_lb,
                                                 void* workspace, size_t workspace_bytes, qt_stream_t stream_) {
    QT_CHECK_ARG(K > 0 && A && U && info && min_eig_lb, "qt_cholesky_inverse_upper_bounded: bad arguments");
    return chol_run(A, 0, K, U, 0, info, 1, workspace, workspace_bytes, (hipStream_t)stream_, min_eig_lb);
}

extern "C" int qt_cholesky_inverse_upper_batched_bounded(float* A, int64_t strideA, int K, float* U, int64_t strideU,
                                                         int32_t* info, int n_problems, const float* min_eig_lb,
                                                         void* workspace, size_t workspace_bytes, qt_stream_t stream_) {
    if (int rc = chol_check_batch("qt_cholesky_inverse_upper_batched_bounded", A && U && info && min_eig_lb, K, n_problems,
                                  strideA, strideU))
        return rc;
    return chol_run(A, strideA, K, U, strideU, info, n_problems, workspace, workspace_bytes, (hipStream_t)stream_, min_eig_lb);
}

// Host-only self-check of the chain's item tables (no GPU needed; tests/test_chol_g3_plan.py) at the default block
// sizes (512 / 512): merged = 0 the separate tables of QT_CHOL_MERGE=0 / order, 1 those of QT_CHOL_MERGE=1; min_chunks
// <= 0: the default threshold.  Over all block rows it verifies that every tile of both segments is covered exactly once
// over its k range (the triangular start on segment 1 / the inverse's product), that a tile's pieces are contiguous,
// in slab order and at least 2 chunks long, that slab ids are unique per launch and below the count the workspace is
// sized for (the separate tables'), and that no launch has more items than the cap.  counts_out[5]: product launches,
// items, slabs (all rows), the workspace's slab count, table bytes.  Returns 0, or a negative code naming the property.
extern "C" int qt_chol_g3_plan_check(int K, int merged, int min_chunks, long long* counts_out) {
    if (K <= 0) return -1;
    constexpr int NBX = 512, TRI_STEP = 256 / G3_CHUNK_ROWS;
    if (min_chunks <= 0) min_chunks = 64;
    const int cap = chol_g3_target_items(K);
    CholG3Plan sep, pl;
    std::vector<char> sep_bytes, bytes;
    chol_g3_build(K, NBX, NBX, min_chunks, cap, false, sep, sep_bytes);
    chol_g3_build(K, NBX, NBX, min_chunks, cap, merged != 0, pl, bytes);
    if (pl.max_slabs > sep.max_slabs || pl.blob_bytes > sep.blob_bytes) return -2;
    long long launches = 0, n_items = 0, n_slabs = 0;
    // one table: segment 0 = Tm x Tn0 tiles from chunk 0 (tri0: from the tile column's own chunk), segment 1 = Tm x Tn1
    auto check = [&](const G3Step& st, int Tm, int Tn0, int tri0, int Tn1, int c_end) -> int {
        if (st.n_items <= 0) return 0;
        const G3Item* items = (const G3Item*)(bytes.data() + st.item_off);
        const G3Red* red = (const G3Red*)(bytes.data() + st.red_off);
        if (st.n_items > cap && st.n_items > Tm * (Tn0 + Tn1)) return -3;
        const int Tn[2] = {Tn0, Tn1};
        auto lo_of = [&](int seg, int tj) { return (seg == 1 || tri0) ? TRI_STEP * tj : 0; };
        std::vector<int> cover((size_t)2 * Tm * (Tn0 + Tn1 + 1) * c_end, 0);
        auto cell = [&](int seg, int ti, int tj, int c) { return (((size_t)seg * Tm + ti) * (Tn0 + Tn1 + 1) + tj) * c_end + c; };
        std::vector<int> owner(sep.max_slabs, -1);
        int slabs_here = 0;
        for (int q = 0; q < st.n_items; ++q) {
            const G3Item& it = items[q];
            const int seg = (it.tile & G3_SEG_BIT) ? 1 : 0, ti = it.tile >> 16, tj = it.tile & G3_TJ_MASK;
            if (ti < 0 || ti >= Tm || tj >= Tn[seg]) return -4;
            const int lo = lo_of(seg, tj);
            if (it.c_lo < lo || it.c_hi > c_end || it.c_hi - it.c_lo < 2) return -5;
            for (int c = it.c_lo; c < it.c_hi; ++c) cover[cell(seg, ti, tj, c)]++;
            if (it.slab < 0) {
                if (it.c_lo != lo || it.c_hi != c_end) return -6;
            } else {
                if (it.slab >= sep.max_slabs) return -7;
                if (owner[it.slab] >= 0) return -8;
                owner[it.slab] = q;
                ++slabs_here;
            }
        }
        for (int seg = 0; seg < 2; ++seg)
            for (int ti = 0; ti < Tm; ++ti)
                for (int tj = 0; tj < Tn[seg]; ++tj)
                    for (int c = 0; c < c_end; ++c)
                        if (cover[cell(seg, ti, tj, c)] != (c >= lo_of(seg, tj) ? 1 : 0)) return -9;
        int in_red = 0;
        for (int r = 0; r < st.n_red; ++r) {
            const G3Red& e = red[r];
            if (e.count < 2 || e.first < 0 || e.first + e.count > sep.max_slabs || (e.seg != 0 && e.seg != 1)) return -10;
            const int want_tile = e.tile | (e.seg ? G3_SEG_BIT : 0);
            int prev_hi = lo_of(e.seg, e.tile & G3_TJ_MASK);
            for (int q = 0; q < e.count; ++q) {
                const int o = owner[e.first + q];
                if (o < 0 || items[o].tile != want_tile || items[o].c_lo != prev_hi) return -11;
                prev_hi = items[o].c_hi;
                owner[e.first + q] = -2;   // listed once
            }
            if (prev_hi != c_end) return -12;
            in_red += e.count;
        }
        if (in_red != slabs_here) return -13;
        ++launches;
        n_items += st.n_items;
        n_slabs += slabs_here;
        return 0;
    };
    for (BlockRow J(K, NBX); J; ++J) {
        const int Jb = J.Jb, Tm = J.Tm(), Tn0 = J.Tn0(), Tn1 = J.Tn1(), c_end = J.c_end();
        int rc = 0;
        if (Jb < (int)pl.row.size() && pl.row[Jb].n_items > 0) {
            if (pl.fac[Jb].n_items > 0 || pl.inv[Jb].n_items > 0) return -14;
            rc = check(pl.row[Jb], Tm, Tn0, 0, Tn1, c_end);
        } else {
            rc = check(pl.fac[Jb], Tm, Tn0, 0, 0, c_end);
            if (!rc) rc = check(pl.inv[Jb], Tm, Tn1, 1, 0, c_end);
        }
        if (rc) return rc;
    }
    if (counts_out) {
        counts_out[0] = launches;
        counts_out[1] = n_items;
        counts_out[2] = n_slabs;
        counts_out[3] = sep.max_slabs;
        counts_out[4] = (long long)pl.blob_bytes;
    }
    return 0;
}
