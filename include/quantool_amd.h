/*
 * quantool_amd.h -- C ABI of the MI355X (gfx950) backend for quantool's GPTQ / AWQ /
 * SmoothQuant per-linear calibration hot path.
 *
 * The reference (langtech-bsc/quantool) has no FFI for this path: its plugins hand the whole
 * job to llmcompressor.oneshot (src/quantool/methods/llm_compressor/base.py:161).  Each entry
 * point below therefore cites the upstream step it replaces by SURVEY.md section 8(a) row
 * (a7..a14) and the reference line through which that step is reached.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says host;
 *   - the caller owns every buffer; nothing persistent is allocated here.  Scratch comes in
 *     through (workspace, workspace_bytes); sizes from the matching *_workspace_bytes().  An entry point writes
 *     nothing outside those bytes and asks no alignment of `workspace` (it aligns the pointer up to 256 itself; the
 *     sizes carry the slack).  A NULL or shorter workspace is refused with QT_ERR_WORKSPACE before anything is
 *     launched.  Where an environment variable changes a size (QT_PREPARE_TWO_PASS, QT_CHOL_G3*, QT_CHOL_NBO / NBI,
 *     QT_G3_TARGET_ITEMS, QT_SWEEP_FAR), the size function and the entry point must be called under the same setting;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); calls are
 *     asynchronous and re-entrant per stream; the current HIP device is used;
 *   - return value: QT_OK (0) or a negative qt_status; qt_last_error() gives a message for
 *     the calling thread.  Nothing throws across this boundary;
 *   - matrices are row-major; "ld" arguments are row strides in ELEMENTS.
 */
#ifndef QUANTOOL_AMD_H
#define QUANTOOL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* qt_stream_t; /* hipStream_t */

enum qt_status {
    QT_OK = 0,
    QT_ERR_INVALID = -1,     /* bad argument / unsupported shape */
    QT_ERR_NOT_PD = -2,      /* Hessian not positive definite (host-side check helper) */
    QT_ERR_WORKSPACE = -3,   /* workspace too small */
    QT_ERR_HIP = -4,         /* a HIP runtime call failed */
    QT_ERR_UNSUPPORTED = -5
};

enum qt_dtype { QT_F32 = 0, QT_BF16 = 1, QT_F16 = 2 };

int qt_version(void);
const char* qt_last_error(void);

/* ---- a7  accumulate_hessian (GPTQ hook under base.py:161) ----------------------------------
 * G[K,K] (fp32, lower triangle incl. diagonal tiles) += X^T X for X[n_tokens,K] in the model's
 * own 16-bit dtype (x_dtype QT_BF16 or QT_F16: the reference injects no dtype, base.py:222-241, and
 * upstream accumulates inp.float() -- both products are exact in the fp32 accumulator).
 * The caller keeps the raw Gram sum G and the sample count n; upstream's running
 * "H = H*n/(n+1) + (2/(n+1)) X^T X" equals (2/n)*G and is applied in qt_hessian_prepare.
 * Requires K % 8 == 0, ldx % 8 == 0, X 16-byte aligned.  Deterministic: a tile is either summed
 * by one workgroup over all tokens and added to G, or split over token chunks whose fp32 slabs are
 * reduced in fixed order -- no atomics. */
size_t qt_xtx_workspace_bytes(int64_t n_tokens, int K);
int qt_xtx_accumulate(const void* X, int x_dtype, int64_t n_tokens, int K, int64_t ldx, float* G,
                      void* workspace, size_t workspace_bytes, qt_stream_t stream);

/* Several Gram sums of ONE K and ONE 16-bit dtype in one launch: problem p computes
 * G[p][K,K] (lower triangle incl. diagonal tiles) += X[p]^T X[p] for X[p] [n_tokens[p], K] with pitch ldx[p].
 * X and G are HOST arrays of device pointers; n_problems is 1..16; the token counts may differ.  A problem with 0
 * tokens contributes nothing and its G (and its X, ldx) is not touched; a batch without tokens launches nothing.
 * Alignment and range rules per problem are those of qt_xtx_accumulate; no two problems may share a G.  A problem
 * whose token count is no multiple of 64 needs ldx[p] == K (the kernel reads an item with one pitch, and the staged
 * zero-padded tail tile has pitch K): otherwise QT_ERR_INVALID -- send that problem through qt_xtx_accumulate.
 * Deterministic, no atomics: a (problem, tile) pair is either summed by one work item over all of the problem's
 * token tiles and added into G from the epilogue, or by several items over disjoint token ranges whose fp32 slabs a
 * table-driven reduction adds in ascending token order.  Which of the two, and the ranges, is a pure function of
 * (n_tokens[], K) -- never of data or pointers -- and qt_xtx_batched_plan returns exactly the table the launch uses.
 * A batch with one non-empty problem is handed to qt_xtx_accumulate: bit-identical to it.  In a larger batch a
 * problem's bits may differ from its single launch (the fp32 partial sums group differently); they depend on the
 * other problems' SIZES only, never on their data.  Precision: a pair summed by one item is ONE fp32 chain over all of
 * the problem's tokens, so its rounding error grows with the square root of the token count (measured against the fp64
 * Gram, K = 4096: 4.9e-6 of sqrt(G_ii G_jj) at 65 536 tokens, 1.07e-5 at 196 608, where the single launch's two-level
 * sum stays below 1e-6).
 * qt_xtx_batched_plan (host-only, needs no device): rows of 6 ints -- problem, ti, tj, first token tile (of 64),
 * token tiles, slab index or -1 for an item added into G -- in launch order; writes min(*n_items, max_items) rows
 * (items may be NULL to ask for the counts alone).  The workspace the launch needs is a property of that plan (its
 * slabs, one staged tail tile per ragged problem, its tables), so the same call returns it in *workspace_bytes: there
 * is no separate size function, and every out pointer may be NULL.  0 bytes for a batch without tokens. */
int qt_xtx_accumulate_batched(const void* const* X, int x_dtype, const int64_t* n_tokens, const int64_t* ldx, int K,
                              float* const* G, int n_problems, void* workspace, size_t workspace_bytes,
                              qt_stream_t stream);
int qt_xtx_batched_plan(const int64_t* n_tokens, int n_problems, int K, int32_t* items, int max_items, int* n_items,
                        int* n_slabs, size_t* workspace_bytes);

/* The two calls above with a bound on the length of every fp32 accumulator chain INSIDE the launch.  chain_tokens is 0
 * (no bound: exactly the unchained call, its kernels and its bits) or a positive multiple of 640; anything else is
 * QT_ERR_INVALID, checked before every other argument.  Every chain_tokens tokens of its work item (counted from the
 * item's own first token) a workgroup runs its epilogue, zeroes its accumulators and goes on: an item that owns its
 * tile adds into G, an item of a split tile stores into its private slab the first time and adds into it afterwards.
 * So a tile with one owner ends as (((G + p1) + p2) + ...), p_i the fp32 MFMA sum over span i: bit for bit what
 * qt_xtx_accumulate computes for that tile when called on the chain_tokens-token slices one after the other.  Rounding
 * error then grows with sqrt(chain_tokens) + sqrt(spans) instead of sqrt(tokens) (figures: DESIGN 4.1).
 * Same plans, same workspace (qt_xtx_workspace_bytes / qt_xtx_batched_plan) and same determinism as the unchained
 * calls; no atomics.  With a ragged token count and ldx != K (two launches) the bound applies to the first launch; the
 * second holds 64 token rows. */
int qt_xtx_accumulate_chained(const void* X, int x_dtype, int64_t n_tokens, int K, int64_t ldx, float* G,
                              int64_t chain_tokens, void* workspace, size_t workspace_bytes, qt_stream_t stream);
int qt_xtx_accumulate_batched_chained(const void* const* X, int x_dtype, const int64_t* n_tokens, const int64_t* ldx,
                                      int K, float* const* G, int n_problems, int64_t chain_tokens, void* workspace,
                                      size_t workspace_bytes, qt_stream_t stream);

/* The same accumulation for fp32 activations X [n_tokens, K] (an fp32 checkpoint: upstream's `inp.float()` is
 * then an fp32 Gram product).  fp32-accurate on the bf16 MFMA: the tokens are split into three
 * bf16 planes (residual <= 2^-27 |x|) and the six plane products of weight >= 2^-16 are summed in one fp32
 * accumulator per lower-triangular tile, added into G.  K % 4 == 0, ldx % 4 == 0, X 16-byte aligned.
 * Deterministic; 6x the MFMA work of the 16-bit path. */
size_t qt_xtx_accumulate_f32_workspace_bytes(int64_t n_tokens, int K);
int qt_xtx_accumulate_f32(const float* X, int64_t n_tokens, int K, int64_t ldx, float* G, void* workspace,
                          size_t workspace_bytes, qt_stream_t stream);

/* ---- a12/a13  activation statistics (AWQ / SmoothQuant hooks under base.py:161) ------------
 * abs_sum[K] += sum_t |x[t,k]|;  cmin[k] = min(cmin[k], min_t x);  cmax likewise.  Any of the
 * three outputs may be NULL.  The caller initialises abs_sum = 0, cmin = +inf, cmax = -inf.
 * X [n_tokens, K] bf16 or fp16 (x_dtype), K % 8 == 0.  Deterministic (ordered chunk reduction). */
size_t qt_act_stats_workspace_bytes(int64_t n_tokens, int K);
int qt_act_stats_accumulate(const void* X, int x_dtype, int64_t n_tokens, int K, int64_t ldx, float* abs_sum,
                            float* cmin, float* cmax, void* workspace, size_t workspace_bytes,
                            qt_stream_t stream);

/* ---- a8/a9  dead columns, damping, activation ordering (quantize_weight, gptq.py:86) -------
 * From the Gram sum G (lower triangle) and sample count n builds (one pass; from K = 2048 two coalesced passes
 * through a symmetric copy of G in the workspace, K*K*4 bytes -- the result is the same to the bit)
 *   Hd = P^T (2/n * G) P  with  dead = diag==0 -> 1,  Hd += percdamp*mean(diag) * I
 * and writes A = flat-reversed Hd (A[i][j] = Hd[K-1-i][K-1-j]), upper triangle valid, which is
 * what qt_cholesky_inverse_upper consumes.  perm (int32[K], sweep position -> original column)
 * may be NULL (identity).  dead[K] (uint8, indexed by sweep position) and diag_out[K]
 * (fp32 diag of 2/n*G in ORIGINAL order, before dead/damp; may be NULL) are outputs. */
size_t qt_hessian_prepare_workspace_bytes(int K);
int qt_hessian_prepare(const float* G, int K, int64_t n_samples, float percdamp,
                       const int32_t* perm, float* A, uint8_t* dead, float* diag_out,
                       void* workspace, size_t workspace_bytes, qt_stream_t stream);
/* The same, and damp_out[0] (device fp32) = the damping term percdamp*mean(diag) that was added: up to the rounding of
 * G a lower bound on lambda_min(A), which qt_cholesky_inverse_upper_bounded takes (no host read needed). */
int qt_hessian_prepare_damp(const float* G, int K, int64_t n_samples, float percdamp,
                            const int32_t* perm, float* A, uint8_t* dead, float* diag_out, float* damp_out,
                            void* workspace, size_t workspace_bytes, qt_stream_t stream);
/* diag(2/n * G) only (input to the activation-ordering argsort). */
int qt_hessian_diag(const float* G, int K, int64_t n_samples, float* diag_out, qt_stream_t stream);
/* a9: perm = argsort(values, descending), stable (equal values keep ascending index; NaN orders as
 * the largest value, as torch.argsort does, so perm is a permutation for any input); inv (may be
 * NULL) receives the inverse permutation.  Rank counting, deterministic. */
int qt_argsort_desc(const float* values, int K, int32_t* perm, int32_t* inv, qt_stream_t stream);

/* ---- a8  cholesky -> cholesky_inverse -> cholesky(upper) ------------------------------------
 * Given A = flat-reversed damped Hessian (upper triangle read, destroyed), writes
 * U = chol(Hd^-1, upper) [K,K] row-major (strict lower triangle zero-filled).
 * Uses A = R^T R, U = flat-reverse(R^-T) (DESIGN.md "one factorisation instead of three").
 * info (device int32): 0 ok, else 1-based index of the first non-positive pivot; upstream's
 * LinAlgError fallback (U = I) is then applied on the device, with no host synchronisation.
 * For large K (from about 6 k; K % 8 == 0) the two block-row products that carry the K^3 run as fp32-accurate
 * three-plane bf16 products and the workspace grows by 12 K^2 bytes for the plane copies of
 * R and R^-T; QT_CHOL_G3=0 keeps the f32-MFMA chain.  Deterministic either way. */
size_t qt_cholesky_inverse_upper_workspace_bytes(int K);
int qt_cholesky_inverse_upper(float* A, int K, float* U, int32_t* info, void* workspace,
                              size_t workspace_bytes, qt_stream_t stream);

/* The same factorisation for n_problems (1..16) Hessians of ONE size K in every launch of the chain: the Linear groups
 * of a decoder layer that read different inputs of equal width (Llama: q/k/v, o, gate/up at K = hidden; Mixtral: the
 * eight experts' w2 at K = intermediate) -- upstream factorises them one after another inside one `oneshot` call
 * (base.py:161 -> quantize_weight per Linear).  Problem b: A + b * strideA (destroyed), U + b * strideU (elements;
 * multiples of 4, >= K*K), info[b].  Each problem's factor is bit-identical to a single-problem call (same kernels,
 * tile shapes, split-K decisions and summation orders per problem); the latency-bound panel kernels -- one workgroup
 * per problem -- and the short products serve all problems per launch.  Workspace: n_problems times a single
 * problem's share plus one copy of the item tables. */
size_t qt_cholesky_inverse_upper_batched_workspace_bytes(int K, int n_problems);
int qt_cholesky_inverse_upper_batched(float* A, int64_t strideA, int K, float* U, int64_t strideU, int32_t* info,
                                      int n_problems, void* workspace, size_t workspace_bytes, qt_stream_t stream);

/* Both with min_eig_lb (device fp32, one value per problem): a lower bound on lambda_min(A), e.g. half the damping
 * term of qt_hessian_prepare_damp.  Where the block-row products run on the matrix pipe they then take TWO fp16 planes
 * per operand and three plane products instead of three bf16 planes and six: |R| <= sqrt(max diag A)
 * and |R^-T| <= 1/sqrt(min_eig_lb) give the per-problem power-of-two scales that keep fp16 in range, computed on the
 * device.  Same workspace sizes.  A bound that is not positive and finite fails its problem (info = K + 1, U = I); a
 * bound above the true lambda_min may overflow the planes.  QT_CHOL_PLANES=bf16x3|f16x2 forces a mode for A/B runs
 * (f16x2 through the entry points without a bound is an argument error).  Deterministic; batch = single bit for bit. */
int qt_cholesky_inverse_upper_bounded(float* A, int K, float* U, int32_t* info, const float* min_eig_lb,
                                      void* workspace, size_t workspace_bytes, qt_stream_t stream);
int qt_cholesky_inverse_upper_batched_bounded(float* A, int64_t strideA, int K, float* U, int64_t strideU, int32_t* info,
                                              int n_problems, const float* min_eig_lb, void* workspace,
                                              size_t workspace_bytes, qt_stream_t stream);

/* ---- a10  minmax observer -> calculate_qparams ----------------------------------------------
 * W[R,K] (fp32, bf16 or fp16 by w_dtype -- every w_dtype / out_dtype argument below takes the three) -> scale, zp [R, K/group_size] fp32.  group_size <= 0:
 * channel-wise.  symmetric: scale = absmax/((qmax-qmin)/2), zp = 0.  scale_t / zp_t (may be
 * NULL) receive the same values group-major [G, R], the layout qt_gptq_sweep reads (one
 * coalesced load per column step: lanes are rows). */
int qt_group_minmax_qparams(const void* W, int w_dtype, int R, int K, int64_t ldw, int group_size,
                            int symmetric, int num_bits, float* scale, float* zp, float* scale_t,
                            float* zp_t, qt_stream_t stream);

/* W_f32[R,K] = float(W[:, perm]) with dead sweep positions zeroed (W = weight.clone().float();
 * W[:, perm]; W[:, dead] = 0).  perm / dead may be NULL. */
int qt_weight_gather_f32(const void* W, int w_dtype, int R, int K, int64_t ldw, const int32_t* perm,
                         const uint8_t* dead, float* W_f32, qt_stream_t stream);

/* Both of the above in ONE pass over W (static / no activation ordering, where the observer sees the ORIGINAL columns
 * and the sweep's working copy is in sweep order): scale, zp [R, G] and W_f32 [R, K] as qt_group_minmax_qparams and
 * qt_weight_gather_f32 give them, to the bit; scale_t / zp_t (may be NULL) at [g * ld_t + r] -- ld_t >= R lets a caller
 * write a Linear's columns of a table that spans the stacked rows of several Linears.  A row must fit the LDS
 * (K <= 81920 16-bit or 40960 fp32 elements). */
int qt_weight_gather_qparams(const void* W, int w_dtype, int R, int K, int64_t ldw, const int32_t* perm,
                             const uint8_t* dead, int group_size, int symmetric, int num_bits, float* W_f32, float* scale,
                             float* zp, float* scale_t, float* zp_t, int64_t ld_t, qt_stream_t stream);

/* ---- a11  the column sweep of quantize_weight -----------------------------------------------
 * W[R,K] fp32 in sweep order (updated in place: error-compensated, then dequantised values),
 * U[K,K] upper factor, scale_t/zp_t [G,R] fp32 (group-major, see qt_group_minmax_qparams),
 * g_idx[K] int32 = group of each sweep position.
 * Outputs Qt[K,R] int8 (integer levels, sweep-position major) and loss[R].
 * blocksize must be 128 (upstream default) in this build.  Bit-exact against
 * oracle/gptq_oracle.c:orc_gptq_sweep for identical inputs -- including when the updates of columns
 * far to the right are applied for several blocks in one pass over W (env QT_SWEEP_BATCH, 1..8 blocks,
 * default 4, 8 from K = 8192: every block's product is still its own ascending-k chain, subtracted in block order),
 * and when a batch's block steps share a launch with the previous batch's far update (env QT_SWEEP_FUSED, default
 * on up to 6144 rows; 0 = one launch per block).
 * Workspace: 8 * blocksize * R floats (the blocks' errors of the longest batch) rounded up to 256 bytes, + 256.
 * Where the shape and the environment at the time of the call allow the fused form (R and K multiples of 128,
 * R <= 6144 or QT_SWEEP_FUSED=1) it holds two buffers of one batch each (a batch writes its own errors while the
 * previous batch's far update still reads the other): no more than the above for batches of up to 4 blocks, twice
 * it for 8 (K >= 8192 or QT_SWEEP_BATCH).  Under QT_SWEEP_FAR=bf16x3 the far update's planes and tile table on top. */
size_t qt_gptq_sweep_workspace_bytes(int R, int K, int blocksize);
int qt_gptq_sweep(float* W, int R, int K, const float* U, const float* scale_t, const float* zp_t,
                  int G, const int32_t* g_idx, int blocksize, int num_bits, int8_t* Qt,
                  float* loss, void* workspace, size_t workspace_bytes, qt_stream_t stream);

/* The sweeps of several Linear groups of ONE in_features K as one stacked sweep: W holds the rows of all groups
 * (group g: rows [row_end[g-1], row_end[g]), row_end a HOST array, every boundary but the last a multiple of 128),
 * group g's factor is U + g * strideU (elements) and its column groups g_idx + g * K; scale_t / zp_t / Qt / loss span the
 * stacked rows.  Rows are independent given their factor, and per row the operation sequence is qt_gptq_sweep's, so
 * every group's outputs are bit-identical to its own qt_gptq_sweep call; the block kernel and the update products run
 * once per 128-column block for all groups (a Llama layer's q/k/v + o + gate/up: 38 912 rows instead of three launches
 * of 6144 / 4096 / 28 672). */
int qt_gptq_sweep_grouped(float* W, int R, int K, const float* U, int64_t strideU, int n_groups, const int32_t* row_end,
                          const float* scale_t, const float* zp_t, int G, const int32_t* g_idx, int blocksize,
                          int num_bits, int8_t* Qt, float* loss, void* workspace, size_t workspace_bytes,
                          qt_stream_t stream);

/* ---- a14  pack_to_int32 (save path, base.py:188) --------------------------------------------
 * packed[R, ceil(K/8)] int32: nibble j of word w = level(column 8w+j) + 8.  col_src (int32[K],
 * may be NULL) maps an output column to the sweep position holding it (undoes actorder). */
int qt_pack_int4(const int8_t* Qt, int R, int K, const int32_t* col_src, int32_t* packed,
                 qt_stream_t stream);

/* Dequantised weights in original column order: out[r,c] = (q - zp[r,g(c)]) * scale[r,g(c)],
 * out dtype by out_dtype (fp32 / bf16 / fp16, round to nearest even); g_of_col int32[K] group of each
 * ORIGINAL column. */
int qt_dequantize(const int8_t* Qt, int R, int K, const int32_t* col_src, const float* scale,
                  const float* zp, int G, const int32_t* g_of_col, void* out, int out_dtype,
                  int64_t ldo, qt_stream_t stream);

/* ---- a12  AWQ scale search (AWQModifier under awq.py:81) ----------------------------------------
 * w_sum[K] += sum_rows |w| / (group absmax + 1e-6) (call once per balance layer; w_mean = w_sum /
 * total rows).  group_size: any divisor of K; <= 0 = one group per row (W8A16).  The workspace size holds for every
 * group size (it has no such argument).  Group sizes of 64 and more that are above 512 or not a multiple of 64 take
 * R <= 65535 rows per call. */
size_t qt_awq_weight_mean_workspace_bytes(int R, int K);
int qt_awq_weight_mean_accumulate(const void* W, int w_dtype, int R, int K, int64_t ldw, int group_size,
                                  float* w_sum, void* workspace, size_t workspace_bytes,
                                  qt_stream_t stream);
/* scales[g][k], g = 0..n_grid-1 (ratio g/n_grid): s = clamp(x_mean^r / (w_mean^(1-r) + 1e-4), 1e-4),
 * s /= sqrt(max s * min s), inf/nan -> 1.  x_mean = x_abs_sum / n_tokens (qt_act_stats_accumulate). */
int qt_awq_scales(const float* x_abs_sum, int64_t n_tokens, const float* w_sum, int64_t n_rows, int K,
                  int n_grid, int duo_scaling, float* scales, qt_stream_t stream);
/* Mirror the lower triangle of the Gram sum into the upper one (G full symmetric afterwards). */
int qt_symmetrize_lower(float* G, int K, qt_stream_t stream);
/* Search loss of one grid point for one balance Linear:  L = mean((X W^T - X Wq^T)^2) with
 * Wq = pseudo_quant(W*s)/s, evaluated as <G, D^T D>_F / (n_tokens * R), D = W - Wq, G = X^T X (full
 * symmetric, see qt_symmetrize_lower).  exact == 0: D rounded to bf16, D^T D on the bf16 MFMA (moves L
 * by < 5e-4 relative; the form the 20-point search runs).  exact != 0: D and D^T D in fp32 on the f32
 * MFMA (16x the MFMA time; used to re-score grid points whose fast losses are closer than that error).
 * loss_out[0] = (accumulate ? loss_out[0] : 0) + weight * L   -- a mapping's loss is the row-weighted
 * mean over its balance Linears, so the caller passes weight = R / total rows. */
size_t qt_awq_loss_workspace_bytes(int R, int K);
int qt_awq_loss(const void* W, int w_dtype, int R, int K, int64_t ldw, const float* s, int group_size,
                int symmetric, int num_bits, const float* Gfull, int64_t n_tokens, int exact, float weight,
                int accumulate, float* loss_out, void* workspace, size_t workspace_bytes, qt_stream_t stream);
/* index_out[0] = index of the first minimum of values[0..n) (n <= 1024): the grid search's argmin. */
/* All n_grid fast search losses of one balance Linear at once (scales [n_grid][K] row-major): losses[g]
 * (+)= weight * loss_g, the same quantity n_grid qt_awq_loss(exact = 0) calls compute, from three launches. */
size_t qt_awq_losses_workspace_bytes(int R, int K, int n_grid);
int qt_awq_losses(const void* W, int w_dtype, int R, int K, int64_t ldw, const float* scales, int n_grid,
                  int group_size, int symmetric, int num_bits, const float* Gfull, int64_t n_tokens, float weight,
                  int accumulate, float* losses, void* workspace, size_t workspace_bytes, qt_stream_t stream);
int qt_argmin_f32(const float* values, int n, int32_t* index_out, qt_stream_t stream);
/* out[R,K] (W's dtype, leading dimension ldo) = pseudo_quant(W * s) / s: the trial weights of one
 * grid point, for mappings whose search loss is measured on a parent module's output (q/k/v under
 * self_attn, gate/up under mlp) rather than on the balance Linear's own.  out may alias W. */
int qt_awq_pseudo_quantize(const void* W, int w_dtype, int R, int K, int64_t ldw, const float* s, int group_size,
                           int symmetric, int num_bits, void* out, int64_t ldo, qt_stream_t stream);
/* out = W * s[None, :] (divide != 0: W / s), rounded to W's dtype (AWQ / SmoothQuant apply step). */
int qt_scale_columns(const void* W, int w_dtype, int R, int K, int64_t ldw, const float* s, int divide,
                     void* out, int64_t ldo, qt_stream_t stream);
/* Plain round-to-nearest levels Qt[K,R] under the given group parameters (AWQ's final step; also
 * the U = I degenerate case of the sweep). */
int qt_rtn_quantize(const void* W, int w_dtype, int R, int K, int64_t ldw, const float* scale,
                    const float* zp, int G, int group_size, int num_bits, int8_t* Qt, qt_stream_t stream);

/* ---- a13  SmoothQuant (SmoothQuantModifier under smoothquant.py:77) -----------------------------
 * wmax[k] = max(wmax[k], max_r |W[r,k]|);  s = (cmax-cmin)^alpha / wmax^(1-alpha), s = cmax-cmin
 * where wmax == 0. */
size_t qt_col_absmax_workspace_bytes(int R, int K);
int qt_col_absmax_accumulate(const void* W, int w_dtype, int R, int K, int64_t ldw, float* wmax,
                             void* workspace, size_t workspace_bytes, qt_stream_t stream);
int qt_smoothquant_scales(const float* cmin, const float* cmax, const float* wmax, int K, float alpha,
                          float* s, qt_stream_t stream);

/* ---- fp32 "TN" GEMM on the f32 MFMA (building block of a8 and a11; exposed for tests) ----------
 * acc[m][n] = sum_{k ascending} A[k*lda + m] * B[k*ldb + n]   (bit-for-bit an fmaf chain from 0)
 * mode 0: Cout = Cin - acc   1: Cout = acc   2: Cout = -acc.   skip_zero_k: B[k][n] == 0 for k < n.
 * allow_split_k != 0 lets latency-bound shapes split k over workgroups (ordered slab reduction:
 * deterministic, but no longer the single ascending chain -- the sweep never allows it).  The workspace is read
 * only with allow_split_k != 0, and is then required in full (QT_ERR_WORKSPACE otherwise: whether k is split must
 * follow from the shape alone); with allow_split_k == 0 it may be NULL. */
size_t qt_sgemm_tn_f32_workspace_bytes(int M, int N);
int qt_sgemm_tn_f32(const float* A, int64_t lda, const float* B, int64_t ldb, const float* Cin,
                    int64_t ldcin, float* Cout, int64_t ldcout, int M, int N, int kdim, int skip_zero_k,
                    int mode, int allow_split_k, void* workspace, size_t workspace_bytes, qt_stream_t stream);

/* Host-only self-check of the Gram kernel's tile table for K (runs without a GPU): 0 if every lower-triangular
 * 256 x 256 tile appears exactly once.  Also returns the distinct 256-channel panels per 32-entry chunk (one XCD's
 * workgroups) and per 256-entry round (the chip), summed over the table -- the locality figures DESIGN.md 4.1 quotes. */
int qt_xtx_tile_table_check(int K, int* n_tiles_out, int* chunk_panels_out, int* round_panels_out);

/* ---- scale * <H, X^T X>_F without storing X^T X (the Gram kernel's epilogue multiplies its tile with H's;
 * building block of a12's search loss <X^T X, D^T D>; exposed for tests) -----------------------------
 * X [n_tokens, K] bf16 / fp16 with ldx == K and n_tokens % 64 == 0; H [K, K] fp32, lower triangle read.
 * *out = (accumulate ? *out : 0) + scale * sum_{i,j} H[i][j] (X^T X)[i][j]; fp64 partial sums in a fixed order. */
size_t qt_xtx_dot_workspace_bytes(int64_t n_tokens, int K);
int qt_xtx_dot(const void* X, int x_dtype, int64_t n_tokens, int K, int64_t ldx, const float* H, double scale,
               float* out, int accumulate, void* workspace, size_t workspace_bytes, qt_stream_t stream);

/* ---- fp32-accurate "TN" product on the bf16 MFMA (three bf16 planes per operand, six plane products;
 * building block of a8's K^3 products; exposed for tests) ---------------------------------------
 * A [k][lda], B [k][ldb] fp32, k a multiple of 128, M / N / lda / ldb multiples of 4.
 * kind 0: C -= A^T B (one workgroup per 256x256 tile);  kind 1: C = A^T B, k split into slabs reduced in
 * fixed order.  Not an ascending-k fmaf chain: never used where the oracle pins the order (a11). */
size_t qt_gemm3_tn_f32_workspace_bytes(int M, int N, int k);
int qt_gemm3_tn_f32(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M,
                    int N, int k, int kind, void* workspace, size_t workspace_bytes, qt_stream_t stream);
/* Test face, as qt_gemm3_tn_f32 (not part of the quantisation path): the same for `batch` >= 1 problems of one shape
 * in one launch (problem b at A + b * bsA, B + b * bsB, C + b * bsC,
 * strides in elements; workspace: batch * qt_gemm3_tn_f32_workspace_bytes(M, N, k)).  tri != 0: B is lower-triangular
 * in 256-blocks (B[k][n] == 0 for k < 256 * (n / 256)) and a tile column's k range starts at its own column, as in the
 * factorisation's block-row products; needs k > 256 * ((N - 1) / 256).  tight != 0: the internal planes are pitched
 * max(M, N) rounded up to 8 instead of 256, so edge tiles clamp their loads (M, N multiples of 8). */
int qt_gemm3_tn_f32_ex(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N,
                       int k, int kind, int tri, int tight, int batch, int64_t bsA, int64_t bsB, int64_t bsC,
                       void* workspace, size_t workspace_bytes, qt_stream_t stream);

/* Test face: the same product on two fp16 planes per operand and three plane products (the mode of
 * qt_cholesky_inverse_upper_bounded).  bound_a / bound_b: HOST arrays, one value per problem (batch <= 32), with
 * |A_b| <= bound_a[b] and |B_b| <= bound_b[b] elementwise. */
int qt_gemm3_tn_f16x2(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N,
                      int k, int kind, int tri, int tight, int batch, int64_t bsA, int64_t bsB, int64_t bsC,
                      const float* bound_a, const float* bound_b, void* workspace, size_t workspace_bytes,
                      qt_stream_t stream);

/* Host-only self-check of the bf16x3 block-row planner (runs without a GPU): 0 if every k chunk of every tile is
 * covered exactly once and the slab / reduction tables are consistent, else a negative code. */
int qt_gemm3_plan_check(int Tm, int Tn, int c_end, int tri, int* n_items_out, int* n_slabs_out, int* longest_out);
/* The same for all item tables of one qt_cholesky_inverse_upper chain of size K at the default block sizes (runs
 * without a GPU).  merged = 0: one table per long product (QT_CHOL_MERGE=0 / order); 1: one table per block row over
 * both of its products (QT_CHOL_MERGE=1).  min_chunks <= 0: the default threshold (QT_CHOL_G3_MIN_CHUNKS otherwise).
 * 0 if every tile of both segments is covered exactly once over its k range by contiguous pieces of >= 2 chunks, slab
 * ids are unique per launch and below the count the workspace is sized for, and no launch exceeds the item cap; else a
 * negative code.  counts_out[5] (may be null): product launches, items, slabs, the workspace's slab count, table bytes. */
int qt_chol_g3_plan_check(int K, int merged, int min_chunks, long long* counts_out);
/* ---- A8 runtime: W8A8 / INT8 / W4A8 checkpoints on the int8 MFMA --------------------------------------
 * The inference side of the 8-bit dynamic per-token activation block these checkpoints carry
 * (config_groups.group_0.input_activations): activations are quantised per row on the fly and multiplied with the
 * stored integer weights in int32, as a served W8A8 runtime does.
 *
 * qt_quantize_tokens_i8: X [M, K] bf16 / fp16 (x_dtype), row pitch ldx >= K (any) -> Xq int8 [M, K] (pitch K),
 * s_x fp32 [M], zp_x int32 [M] (asymmetric only; may be NULL when symmetric).  col_perm (int32 [K], may be NULL):
 * Xq[m, k] = q(X[m, col_perm[k]]).  Per row, all in fp32 (SURVEY A.2 calculate_qparams / fake_quantize, 8 bits,
 * qmin = -128, qmax = 127):
 *   min = min(min_k x, 0), max = max(max_k x, 0)
 *   symmetric:  s = max(|min|, |max|) / 127.5, zp = 0       (divisor recalled, not pinned: DESIGN.md 4.7)
 *   asymmetric: s = (max - min) / 255
 *   s = max(s, FLT_EPSILON);  asymmetric: zp = clamp(rint(qmin - min / s), qmin, qmax)
 *   q = rint(clamp(x / s + zp, qmin, qmax))        IEEE division, round half to even, clamp before rounding
 *
 * qt_gemm_i8: Y [M, N] (out_dtype bf16 / fp16, row pitch ldy) = epilogue(Xq . Wq^T), both operands K-contiguous.
 *   w_format QT_W_INT8:        Wq int8 [N, K]
 *   w_format QT_W_INT4_PACKED: Wq int32 [N, ceil(K/8)], nibble j of word w = level of column 8w + j, plus 8
 *                              (qt_pack_int4's layout); unpacked to int8 on chip
 *   s_w fp32 [N, G]: G = 1 (channel-wise) or G = ceil(K/128) (groups of 128 contiguous columns)
 *   zp_x int32 [M] (may be NULL: symmetric activations); wsum int32 [N, G] = per-group row sums of the weight levels
 *   (read only with zp_x);  bias [N] in out_dtype (may be NULL).  K <= 32768 (the int32 accumulator cannot overflow).
 * Fixed fp32 sequence, no contraction -- a restatement of these steps is equal to the bit:
 *   acc_g[m, n] = sum_{k in g} Xq[m, k] * Wq[n, k]              int32, exact
 *   t_g  = (float)(acc_g - zp_x[m] * wsum[n, g])                 int32 difference, one rounding to fp32
 *   tot  = 0.0f;  tot = tot + s_w[n, g] * t_g  for g = 0, 1, ... ascending (product and sum rounded separately)
 *   y    = s_x[m] * tot;  y = y + (float)bias[n]  (when bias is given)
 *   Y[m, n] = y rounded once to out_dtype (round to nearest even)
 *
 * qt_gemm_i8_skinny: the decode form of qt_gemm_i8, 1 <= M <= 16 (any other M is QT_ERR_INVALID before any launch).
 *   Same arguments, same meanings, same refusals, and for every legal input Y is bit-identical to qt_gemm_i8's on the
 *   same arguments: both weight formats, G = 1 and G = ceil(K/128), with and without zp_x / wsum and bias, bf16 and fp16
 *   output, ragged K, N not a multiple of 16, operands not 16-byte aligned, K <= 32768.  A workgroup owns 16 output
 *   columns and splits K over its 4 waves (128-column k-block kb to wave kb % 4), the weights go from global memory
 *   straight to registers and are read once, v_mfma_i32_16x16x64_i8 with M padded to 16.  The sequence above is integer
 *   up to t_g, so acc_g does not depend on how K was split; the waves hand their acc_g over as int32 through LDS and one
 *   thread per output element runs the chain t_g -> tot -> y literally, g ascending.  No wave ever holds an fp32
 *   partial.  Deterministic, no atomics, no workspace.  
 *
 * qt_gemm_i8_ring: the prefill form of qt_gemm_i8 for W8A8 / INT8: w_format == QT_W_INT8 with G == 1 (int8 weights,
 *   channel-wise scales), K a multiple of QT_I8_RING_K_UNIT, K <= 32768, Xq and Wq 16-byte aligned.  Same arguments,
 *   same meanings; with and without zp_x / wsum and bias, bf16 and fp16 output, any M >= 1, any N >= 1, any ldy >= N.
 *   Everything else -- packed int4, G > 1, a ragged K, a misaligned operand -- is QT_ERR_INVALID before any launch, and
 *   qt_last_error names the reason.  For every legal input Y is bit-identical to qt_gemm_i8's on the same arguments: acc
 *   is an exact int32 sum, whatever the order, and the chain t -> tot = 0.0f + s_w t -> y above runs literally, once per
 *   output element, in the lane that holds it.  One 8-wave workgroup per 256 x 256 output tile streams the reduction
 *   QT_I8_RING_K_UNIT k-bytes (one cache line per row) at a time, as half panels of 128 rows, through a ring of
 *   QT_I8_RING_SLOTS LDS slots filled by LDS-DMA QT_I8_RING_LEAD half panels ahead (csrc/ring_pipe.h,
 *   csrc/qlinear_ring.hip), v_mfma_i32_32x32x32_i8.  A tile row past M or N re-reads row M - 1
 *   or N - 1 and is never stored: no byte outside Xq[M, K] and Wq[N, K] is read, no element outside Y[m < M, n < N] is
 *   written.  Deterministic, no atomics, no workspace.  
 *
 * qt_gemm_i8_ring_w4: the prefill form of qt_gemm_i8 for W4A8: w_format == QT_W_INT4_PACKED with G == K / 128 (packed
 *   int4 weights, one scale per group of 128 columns), K a multiple of QT_I8_RING_W4_K_UNIT, K <= 32768, Xq and Wq
 *   16-byte aligned.  Same arguments, same meanings; with and without zp_x / wsum and bias, bf16 and fp16 output, any
 *   M >= 1, any N >= 1, any ldy >= N.  Everything else -- int8 weights, channel-wise scales (G == 1 with K > 128), a
 *   ragged K, a misaligned operand -- is QT_ERR_INVALID before any launch, and qt_last_error names the reason.  (At
 *   K == 128 the one group is the whole row: G = K / 128 = 1 is taken.)  For every legal input Y is bit-identical to
 *   qt_gemm_i8's on the same arguments: it is qt_gemm_i8_ring's 256 x 256 tile and LDS ring, and because a K-tile of
 *   that ring is exactly one weight group, the int32 result of a phase is the complete acc_g of its outputs; the chain
 *   t_g -> tot = tot + s_w t_g -> y above runs literally, once per output element and group, g ascending, in the
 *   lane that holds the element.  wsum must be what its name says (|wsum[n, g]| <= 128 * 8): zp_x * wsum is a 24-bit
 *   multiply.  B half panels travel packed (64 B per row and K-tile) and are unpacked between LDS and the MFMA; s_w
 *   and wsum of a K-tile ride with the ring as a counted LDS-DMA gather (csrc/qlinear_ring_w4.hip).  A tile row past M
 *   or N re-reads row M - 1 or N - 1 and is never stored: no byte outside Xq[M, K], Wq[N, K/8], s_w / wsum[N, G],
 *   s_x / zp_x[M] is read, no element outside Y[m < M, n < N] is written.  Deterministic, no atomics, no workspace.
 *   
 *
 * qt_gemm_i8_mid: the form of qt_gemm_i8 for a few tiles of rows, 1 <= M <= QT_I8_MID_MAX_M.  qt_gemm_i8's arguments
 *   with the same meanings.  Taken: both weight formats, G = 1 and G = K/128, with and without zp_x / wsum and bias, bf16
 *   and fp16 output, any N >= 1, any ldy >= N, K a multiple of QT_I8_MID_K_UNIT, K <= 32768, Xq and Wq 16-byte aligned.
 *   Everything else -- M = 0 or M > QT_I8_MID_MAX_M, a ragged K, a misaligned operand, a null pointer, a G that is
 *   neither 1 nor K/128 -- is QT_ERR_INVALID before any launch, and qt_last_error names the reason.  For every legal
 *   input Y is bit-identical to qt_gemm_i8's on the same arguments, for qt_gemm_i8_skinny's reason: acc_g is an exact
 *   int32 sum whatever its order, the waves hand their acc_g over as int32 through LDS, and one thread per output
 *   element runs the chain t_g -> tot -> y literally, g ascending from 0.0f, with one rounding to out_dtype; no wave ever
 *   holds an fp32 partial of another wave's groups.  It is qt_gemm_i8_skinny's tile widened in M: a workgroup owns 16
 *   output columns and all M rows as ceil(M/16) m-tiles (2, 4 or 8 compiled), splits K over its 4 waves (k-block kb to
 *   wave kb % 4), the weights go from global memory straight to registers, non-temporal, and every weight byte is read
 *   from memory once per launch; v_mfma_i32_16x16x64_i8 with the weights as A and 16 activation rows as B.  An
 *   activation row past M is zero in registers, a weight row past N re-reads row N - 1, neither is stored: no byte
 *   outside Xq[M, K], Wq[N, K] (int4: [N, K/8] words), s_w / wsum[N, G], s_x / zp_x[M] is read, no element outside
 *   Y[m < M, n < N] is written.  Deterministic, no atomics, no workspace, no communication between workgroups.
 *   
 *
 * qt_splitk_gemm_i8: the short-prompt form of qt_gemm_i8 for W8A8 / INT8, a few tiles of rows over a long reduction:
 *   qt_gemm_i8_ring's 256 x 256 tile over a k-range, plus a reduce pass.  qt_gemm_i8's arguments with the same
 *   meanings, followed by splits, workspace and workspace_size.  Taken: w_format == QT_W_INT8 with G == 1, K a multiple
 *   of QT_SPLITK_I8_K_UNIT, K <= 32768, Xq, Wq and the workspace 16-byte aligned, bf16 and fp16 output, with and without
 *   zp_x / wsum and bias, any M >= 1, any N >= 1, any ldy >= N, and a split count S >= 2 out of qt_splitk_gemm_i8_plan.
 *   Everything else -- packed int4, G > 1, a ragged K, a misaligned operand, a null workspace, S == 1 (that is
 *   qt_gemm_i8_ring), S > K / QT_SPLITK_I8_K_UNIT or > QT_SPLITK_I8_MAX_SPLITS, a workspace smaller than the plan's
 *   (the message names the size needed) -- is QT_ERR_INVALID before any launch, and qt_last_error names the reason.
 *   For every legal input Y is bit-identical to qt_gemm_i8's on the same arguments: acc is an exact int32 sum in any
 *   order, so S partial sums over disjoint k-ranges, added in int32, are acc; the chain t -> tot = 0.0f + s_w t -> y
 *   above then runs literally, once per output element.  Two launches on the caller's stream.  (1) A workgroup is
 *   (tile, split): split s owns the K-tiles (QT_SPLITK_I8_K_UNIT k-bytes each) [t0(s), t1(s)) that
 *   qt_splitk_gemm_i8_range deals -- contiguous, sizes differing by at most one -- and stores its int32 accumulators,
 *   unchanged, into slab s of the workspace: int32 [S][Mp][Np] row-major, Mp = 256 ceil(M/256), Np = 256 ceil(N/256).
 *   Tile rows and columns past M or N are computed from the clamped source rows, as in qt_gemm_i8_ring, and land in
 *   the slab's padding, which nothing ever reads.  (2) The reduce pass reads the S slabs at m < M, n < N only, adds
 *   them in int32 and runs the epilogue.  The workspace need not be initialised.  No byte outside Xq[M, K], Wq[N, K]
 *   is read, no element outside Y[m < M, n < N] and no byte past workspace_size is written.  Deterministic, no
 *   atomics, no communication between workgroups inside a launch: a row's result depends on the row, the weight and
 *   the epilogue inputs alone.  
 * qt_splitk_gemm_i8_plan: host-only, no device needed: the split count and the workspace size for (M, N, K) on a
 *   device of `cus` compute units.  splits_requested == 0: tiles = ceil(M/256) ceil(N/256), kt = K / QT_SPLITK_I8_K_UNIT,
 *   S = clamp(cus / tiles, 1, min(max(kt / QT_SPLITK_I8_MIN_K_TILES, 1), QT_SPLITK_I8_MAX_SPLITS)) -- about one
 *   workgroup per compute unit, and no split shorter than QT_SPLITK_I8_MIN_K_TILES K-tiles (two trips round the ring;
 *   the measured rule).  splits_requested >= 1: that S, refused (QT_ERR_INVALID) above min(K / QT_SPLITK_I8_K_UNIT,
 *   QT_SPLITK_I8_MAX_SPLITS).  *workspace_size = S Mp Np 4 bytes (also for S == 1, which qt_splitk_gemm_i8 refuses).
 * qt_splitk_gemm_i8_range: host-only: the K-tiles [*t0, *t1) of split s out of `splits` over k_tiles K-tiles:
 *   t0 = s q + min(s, r) with q = k_tiles / splits, r = k_tiles % splits; the first r splits hold q + 1.
 *
 * qt_act_mul_quantize_i8: the glue between the two products of an MLP in one row pass -- h = act(gate) * up as torch's
 *   two elementwise kernels leave it in a 16-bit tensor, then qt_quantize_tokens_i8 on h -- without h ever reaching
 *   memory.  gate and up are [M, K] bf16 / fp16 (x_dtype) with unit column stride and row pitches ldg, ldu >= K; they may
 *   be the two halves of one [M, 2K] tensor (up = gate + K, ldg = ldu = 2K) and need no alignment: 16-byte loads are
 *   taken when both pointers, both pitches and K allow, element loads otherwise.  act: QT_ACT_SILU.  Xq, s_x, zp_x,
 *   col_perm and symmetric mean what they mean in qt_quantize_tokens_i8, with one difference on a malformed table: an
 *   entry of col_perm outside [0, K) is clamped into the row here (the gather reads the workgroup's own K values and
 *   nothing else), where qt_quantize_tokens_i8 reads X at the entry as given.  H (may be NULL): when given, h is also stored
 *   as [M, K] in x_dtype with row pitch ldh >= K, in natural column order (col_perm does not apply to it); it exists so
 *   that the activation can be pinned bit for bit apart from the quantiser.  A null gate, up, Xq or s_x, M <= 0,
 *   K <= 0, a pitch below K, an x_dtype that is not 16-bit, an unknown act, asymmetric activations without zp_x,
 *   K > 32768 (the GEMMs' bound) and M > INT32_MAX are QT_ERR_INVALID before any launch, and qt_last_error names the
 *   reason.  Fixed sequence per element, in fp32 with no contraction:
 *     g  = (float)gate[m, k];  u = (float)up[m, k]
 *     a  = g / (1.0f + expf(-g))              IEEE division
 *     a' = a rounded once to x_dtype (RNE)    -- what torch's SiLU leaves in a 16-bit tensor
 *     p  = (float)a' * u
 *     h  = p rounded once to x_dtype (RNE)    -- what torch's multiply leaves
 *   then exactly qt_quantize_tokens_i8's row sequence on h: min / max including 0, s, zp,
 *   q = rint(clamp(h / s + zp, -128, 127)), Xq[m, k] = q(h[m, col_perm[k]]).
 *   So (Xq, s_x, zp_x) equal qt_quantize_tokens_i8(F.silu(gate) * up) to the bit wherever this expf is torch's (pinned
 *   over all 65536 patterns of both dtypes by the tests).  One workgroup per row: h is computed once,
 *   held in LDS as 16-bit values (2 K bytes) while min / max are reduced, and quantised from there.  A row's result
 *   depends on the row alone.  Deterministic, no atomics, no workspace.  (csrc/act_quant.hip)
 *
 * qt_rmsnorm_quantize_i8: the glue in front of the products that share one normalised input (q/k/v, gate/up) in one row
 *   pass -- y = weight * RMSNorm(x) as transformers' LlamaRMSNorm.forward leaves it in a 16-bit tensor, then
 *   qt_quantize_tokens_i8 on y.  X is [M, K] bf16 / fp16 (x_dtype) with unit column stride and row pitch ldx >= K, weight
 *   [K] in x_dtype; neither needs alignment: 16-byte loads are taken when both pointers, ldx and K allow, element
 *   loads otherwise.  Xq, s_x, zp_x, col_perm and symmetric mean what they mean in qt_act_mul_quantize_i8, the clamp of
 *   a malformed col_perm entry into the row included.  Y (may be NULL): when given, y is stored as [M, K] in x_dtype
 *   with row pitch ldy >= K, in natural column order (col_perm does not apply to it); it is what the residual stream
 *   and every consumer that does not take Xq read.  rstd (may be NULL): fp32 [M], the row's r below.  A null X, weight,
 *   Xq or s_x, M <= 0, K <= 0, ldx < K, Y given with ldy < K, an x_dtype that is not 16-bit, asymmetric activations
 *   without zp_x, an eps that is negative or not finite, K > 32768 (the GEMMs' bound) and M > INT32_MAX are
 *   QT_ERR_INVALID before any launch, and qt_last_error names the reason.  Fixed sequence per row, in fp32 with no
 *   contraction (every multiply and add its own rounding):
 *     1. sq_k = x_k * x_k
 *     2. lane t of 256 owns the 8-element chunks c = t (mod 256), chunk c being columns 8c ... 8c+7, and adds their
 *        sq_k to its partial in ascending k, starting from 0.0f (the element-load path walks the same chunks)
 *     3. the lane partials combine by the xor butterfly 32, 16, ..., 1 inside each wave of 64, then
 *        sum = ((wave0 + wave1) + wave2) + wave3
 *     4. mean = sum * (1.0f / (float)K);  v = mean + eps;  r = (float)(1.0 / sqrt((double)v)), the correctly rounded
 *        fp32 value of 1 / sqrt(v), which is what torch.rsqrt returns on the device (rsqrtf, the hardware's approximation,
 *        is 1 ulp off in about one value of ten);  rstd[m] = r
 *     5. n_k = (x_k * r) rounded once to x_dtype (RNE);  y_k = ((float)w_k * (float)n_k) rounded once to x_dtype (RNE)
 *        -- the normalised row is narrowed before the weight multiplies it, as LlamaRMSNorm.forward does
 *     6. exactly qt_quantize_tokens_i8's row sequence on y: min / max including 0, s, zp,
 *        q = rint(clamp(y / s + zp, -128, 127)), Xq[m, k] = q(y[m, col_perm[k]]).
 *   The sum order of steps 2 and 3 depends on K alone -- not on alignment, pitch, M or the row's index -- so a row's
 *   result depends on the row alone.  It is not torch's order: given r, Y is exactly step 5 and (Xq, s_x, zp_x) are
 *   exactly qt_quantize_tokens_i8(Y); r itself is within (8 ceil(K/2048) + 13) 2^-24 (relative) of the exact value and
 *   equals torch's to the bit wherever the sum of squares is exact in fp32.  One workgroup per row: the
 *   row is held in LDS as 16-bit values (2 K bytes), x first and y in its place.  Deterministic, no atomics, no
 *   workspace.  (csrc/rmsnorm_quant.hip) */
enum qt_act { QT_ACT_SILU = 0 };
#define QT_I8_MID_MAX_M 128
#define QT_I8_MID_K_UNIT 128
#define QT_I8_RING_K_UNIT 128
#define QT_I8_RING_SLOTS 8
#define QT_I8_RING_LEAD 6
#define QT_I8_RING_W4_K_UNIT 128
#define QT_I8_RING_W4_SLOTS 8
#define QT_I8_RING_W4_LEAD 6
#define QT_SPLITK_I8_K_UNIT 128
#define QT_SPLITK_I8_MAX_SPLITS 32
#define QT_SPLITK_I8_MIN_K_TILES 4
#define QT_MOE_I8_WIDE_K_UNIT 128
#define QT_MOE_I8_WIDE_TILE_ROWS 128
#define QT_MOE_I8_WIDE_MAX_E 4096
enum qt_weight_format { QT_W_INT8 = 0, QT_W_INT4_PACKED = 1 };
int qt_quantize_tokens_i8(const void* X, int x_dtype, int64_t M, int K, int64_t ldx, const int32_t* col_perm,
                          int symmetric, int8_t* Xq, float* s_x, int32_t* zp_x, qt_stream_t stream);
int qt_act_mul_quantize_i8(const void* gate, int64_t ldg, const void* up, int64_t ldu, int x_dtype, int64_t M, int K,
                           int act, const int32_t* col_perm, int symmetric, int8_t* Xq, float* s_x, int32_t* zp_x,
                           void* H, int64_t ldh, qt_stream_t stream);
int qt_rmsnorm_quantize_i8(const void* X, int64_t ldx, const void* weight, int x_dtype, int64_t M, int K, float eps,
                           const int32_t* col_perm, int symmetric, int8_t* Xq, float* s_x, int32_t* zp_x,
                           void* Y, int64_t ldy, float* rstd, qt_stream_t stream);
int qt_gemm_i8(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N, const float* s_x,
               const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias, void* Y,
               int out_dtype, int64_t ldy, qt_stream_t stream);
int qt_gemm_i8_skinny(const int8_t* Xq, int M, int K, const void* Wq, int w_format, int N, const float* s_x,
                      const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias, void* Y,
                      int out_dtype, int64_t ldy, qt_stream_t stream);
int qt_gemm_i8_ring(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N, const float* s_x,
                    const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias, void* Y,
                    int out_dtype, int64_t ldy, qt_stream_t stream);
int qt_gemm_i8_ring_w4(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N, const float* s_x,
                       const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias, void* Y,
                       int out_dtype, int64_t ldy, qt_stream_t stream);
int qt_gemm_i8_mid(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N, const float* s_x,
                   const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias, void* Y,
                   int out_dtype, int64_t ldy, qt_stream_t stream);
int qt_splitk_gemm_i8_plan(int64_t M, int N, int K, int cus, int splits_requested, int* splits,
                           size_t* workspace_size);
int qt_splitk_gemm_i8_range(int k_tiles, int splits, int s, int* t0, int* t1);
int qt_splitk_gemm_i8(const int8_t* Xq, int64_t M, int K, const void* Wq, int w_format, int N, const float* s_x,
                      const int32_t* zp_x, const float* s_w, int G, const int32_t* wsum, const void* bias, void* Y,
                      int out_dtype, int64_t ldy, int splits, void* workspace, size_t workspace_size,
                      qt_stream_t stream);

/* ---- Routed experts: W8A8 / INT8 / W4A8 sparse-MoE banks on the same int8 GEMM ------------------------------
 * The A8 expert forward (engine/qlinear.py QuantizedExperts) restates transformers' MixtralExperts.forward with the
 * two F.linear calls replaced by the A8 runtime above:
 *   route -> quantize_tokens_i8 (all T tokens once) -> gemm_i8_grouped (gate_up, rows gathered by src_token)
 *   -> act_fn(gate) * up in torch -> quantize_tokens_i8 (routed rows) -> gemm_i8_grouped (down, contiguous) -> combine
 * Per-token quantisation is a function of the row alone, so quantising the T tokens and gathering equals gathering
 * and quantising.  With QuantizedExperts.fused_act and a SiLU act_fn the two steps of the second line's start run as
 * one, act_mul_quantize_i8 on the two halves of the gate_up output, to the same bits.
 *
 * qt_moe_route: top_k_index [T, k] (int32, or int64 when index_is_int64) -> offsets int32 [E + 1],
 *   src_token / src_slot int32 [T k], row_of int32 [T k] (may be NULL).  The routed rows are the entries (t, j) with
 *   0 <= top_k_index[t, j] < E (others are dropped, as transformers' loop skips expert_idx == num_experts), sorted by
 *   expert and, within an expert, by the flat index t k + j (token ascending): a stable argsort of the flattened
 *   table.  (transformers' torch.where(expert_mask[e]) lists an expert's rows slot-major; the order of rows within an
 *   expert changes no output -- every row is computed alone and the combine sums per token.)
 *   Row r in [offsets[e], offsets[e + 1]) is (src_token[r], src_slot[r]); row_of[t k + j] = its row, or -1 when
 *   dropped; rows [offsets[E], T k) read 0.  Integer work in one workgroup, no atomics, no host read; E <= 256.
 *
 * qt_gemm_i8_grouped: qt_gemm_i8 over E weight matrices at once.  Y [R, N] (pitch ldy): expert e owns output rows
 *   [offsets[e], offsets[e + 1]) (offsets int32 [E + 1], on the device, ascending, offsets[E] <= R; rows past
 *   offsets[E] are not written) and weight matrix e of Wq ([E, N, K] int8 or [E, N, ceil(K/8)] packed int4), s_w
 *   fp32 [E, N, G], wsum int32 [E, N, G].  A row of output row m is Xq[row_idx[m]] (row_idx int32 [R], values index
 *   rows of Xq; the caller's contract) or Xq[m] when row_idx is NULL; s_x and zp_x are read at the same index.
 *   Every expert's rows are equal to the bit to qt_gemm_i8 on that expert's (gathered) rows: it is the same tile code
 *   and the same fixed fp32 epilogue.  The grid is (ceil(R/128) + E) m-tiles x n-tiles, an upper bound that needs no
 *   host read of the counts; each workgroup finds its expert from offsets and surplus workgroups exit.  No bias.
 *
 * qt_gemm_i8_skinny_grouped: the decode form of qt_gemm_i8_grouped: same arguments, same meanings, same refusals, and Y
 *   bit-identical to qt_gemm_i8_grouped's on the same arguments (rows past offsets[E] are not written).  It is
 *   qt_gemm_i8_skinny's tile over E weight matrices: every expert's rows go in tiles of 16, the grid is ceil(N/16)
 *   column tiles x (floor(R/16) + min(E, R)) row-tile slots, an upper bound on sum_e ceil(rows_e / 16) that needs no
 *   host read of offsets; a workgroup finds its expert and tile by walking the clamped offsets and a surplus one exits
 *   before any weight load.  Only the experts that own rows have their weights read, each once per 16 of its rows, so
 *   this is the form for a few tokens.  R / 16 + min(E, R) <= 65535, else QT_ERR_INVALID.  Deterministic, no atomics.
 *
 * qt_gemm_i8_ring_grouped: the prefill form of qt_gemm_i8_grouped for W8A8 / INT8 banks: qt_gemm_i8_ring's 256 x 256
 *   LDS-ring tile over E weight matrices.  qt_gemm_i8_grouped's arguments with the same meanings, plus x_rows, the
 *   number of rows of Xq.  Taken: w_format == QT_W_INT8 with G == 1, K a multiple of QT_I8_RING_K_UNIT, K <= 32768, Xq
 *   and Wq 16-byte aligned, E <= 4096, and with row_idx x_rows K <= 2^32 (a gathered row is addressed by a 32-bit byte
 *   offset from Xq), without it x_rows >= R; anything else is QT_ERR_INVALID before any launch and qt_last_error names
 *   the reason.  For every legal input Y is bit-identical to qt_gemm_i8_grouped's on the same arguments: the int32 sum
 *   is exact and the chain t -> tot = 0.0f + s_w t -> y runs literally, once per output element.  The grid is
 *   (ceil(R/256) + E) m-tile slots x ceil(N/256) n-tiles, an upper bound that needs no host read of the counts; a
 *   workgroup walks offsets (clamped to [0, R] and made ascending) to its expert and tile, and a surplus one exits
 *   before its first load.  row_idx values are clamped into [0, x_rows); a tile row past the expert's last row re-reads
 *   that expert's last row and is never stored: no byte outside Xq[x_rows, K] and Wq[E, N, K] is read, no element
 *   outside Y[m < offsets[E], n < N] is written.  No bias, no workspace, no atomics: deterministic.  
 *
 * qt_moe_gemm_i8_ring_w4: the prefill form of qt_gemm_i8_grouped for W4A8 banks: qt_gemm_i8_ring_w4's 256 x 256
 *   LDS-ring tile and per-K-tile group fold over E packed weight matrices.  qt_gemm_i8_ring_grouped's arguments with
 *   the same meanings (x_rows, the number of rows of Xq, in front of the stream; no bias).  Taken: w_format ==
 *   QT_W_INT4_PACKED with G == K / 128, K a multiple of QT_I8_RING_W4_K_UNIT, K <= 32768, Xq and Wq 16-byte aligned,
 *   E <= 4096, R <= 2^31 - 1, (ceil(R/256) + E) ceil(N/256) < 2^31, and with row_idx x_rows K <= 2^32 (a gathered row
 *   is addressed by a 32-bit byte offset from Xq), without it x_rows >= R; zp_x needs wsum.  Anything else is
 *   QT_ERR_INVALID before any launch and qt_last_error names the reason (int8 weights run on qt_gemm_i8_ring_grouped,
 *   G == 1 runs on qt_gemm_i8_grouped).  For every legal input Y is bit-identical to qt_gemm_i8_grouped's on the same
 *   arguments: acc_g is exact and the fold t -> prod = s_w t -> tot = tot + prod, g ascending, then y = s_x tot, runs
 *   literally, once per output element.  The grid and the walk are qt_gemm_i8_ring_grouped's; rows >= offsets[E] are
 *   not written; row_idx values are clamped into [0, x_rows); a tile row past the expert's last row re-reads that
 *   expert's last row and is never stored: no byte outside Xq[x_rows, K], Wq[E, N, K/8], s_w / wsum[E, N, G] is read,
 *   no element outside Y[m < offsets[E], n < N] is written.  No workspace, no atomics: deterministic.  The name is of
 *   the qt_moe_* family; the form's limits are those of the two entry points it joins.  
 *
 * qt_moe_gemm_i8_wide: the form of qt_gemm_i8_grouped between the decode range and the rings -- batched decode,
 *   speculative verification, short prompts: qt_gemm_i8_mid's weight-streaming 16-column tile over E weight matrices.
 *   qt_moe_gemm_i8_ring_w4's argument list with the same meanings (x_rows, the number of rows of Xq, in front of the
 *   stream; no bias).  Taken: both weight formats, G = 1 and G = K/128, with and without zp_x / wsum (zp_x needs wsum),
 *   bf16 and fp16 output, any R >= 1 up to the slot bound below, any N >= 1, any ldy >= N, K a multiple of
 *   QT_MOE_I8_WIDE_K_UNIT, K <= 32768, Xq and Wq 16-byte aligned, E <= QT_MOE_I8_WIDE_MAX_E, and with row_idx
 *   x_rows K <= 2^32 (a gathered row is addressed by a 32-bit byte offset from Xq), without it x_rows >= R.  Anything
 *   else is QT_ERR_INVALID before any launch and qt_last_error names the reason.  For every legal input Y is
 *   bit-identical to qt_gemm_i8_grouped's on the same arguments, for qt_gemm_i8_mid's reason: acc_g is an exact int32
 *   sum whatever its order, the waves hand their acc_g over as int32 through LDS, and one thread per output element
 *   runs the chain t_g -> tot = tot + s_w t_g -> y = s_x tot literally, g ascending from 0.0f, with one rounding to
 *   out_dtype; no wave ever holds an fp32 partial.  A workgroup holds MT = 2, 4 or 8 m-tiles of 16 rows, chosen from R
 *   alone (R <= 32: 2, R <= 64: 4, else 8: an expert owns at most R rows); the grid is ceil(N/16) column tiles x
 *   (floor(R / (16 MT)) + min(E, R)) row-tile slots, an upper bound on sum_e ceil(rows_e / (16 MT)) that needs no host
 *   read of the counts, and must not exceed 65535 slots.  A workgroup walks offsets (clamped to [0, R] and made
 *   ascending) to its expert and its tile of up to 16 MT of that expert's rows; a surplus one exits before its first
 *   weight load and its first barrier.  An expert's weights are read once per QT_MOE_I8_WIDE_TILE_ROWS of its rows,
 *   and only the experts that own rows are read.  rows >= offsets[E] are not written; row_idx values are clamped into
 *   [0, x_rows); a tile row past the expert's last row is zero in registers, a weight row past N re-reads row N - 1 of
 *   the same expert, neither is stored: no byte outside Xq[x_rows, K], Wq[E, N, K] (int4: [E, N, K/8] words), s_w /
 *   wsum[E, N, G], s_x / zp_x[x_rows] is read, no element outside Y[m < offsets[E], n < N] is written.  No workspace,
 *   no atomics: deterministic, no communication between workgroups.  
 *
 * qt_moe_combine: out [T, H] (dtype bf16 / fp16) = the weighted sum of each token's routed rows of Y [R, H] (pitch
 *   ldy), transformers' MixtralExperts.forward restated: for the token's rows r = row_of[t k + j] >= 0 in ascending
 *   row order (= ascending expert), with w = weights[t, j] fp32 [T, k]:
 *     c = round_to_dtype((float)Y[r, h] * w);  out = round_to_dtype(out + c),  out starting at 0
 *   k <= 16; one workgroup per token, no atomics: deterministic. */
int qt_moe_route(const void* top_k_index, int index_is_int64, int64_t T, int k, int E, int32_t* offsets,
                 int32_t* src_token, int32_t* src_slot, int32_t* row_of, qt_stream_t stream);
int qt_gemm_i8_grouped(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R, const int32_t* offsets, int E,
                       const void* Wq, int w_format, int N, const float* s_x, const int32_t* zp_x, const float* s_w,
                       int G, const int32_t* wsum, void* Y, int out_dtype, int64_t ldy, qt_stream_t stream);
int qt_gemm_i8_skinny_grouped(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R, const int32_t* offsets,
                              int E, const void* Wq, int w_format, int N, const float* s_x, const int32_t* zp_x,
                              const float* s_w, int G, const int32_t* wsum, void* Y, int out_dtype, int64_t ldy,
                              qt_stream_t stream);
int qt_gemm_i8_ring_grouped(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R, const int32_t* offsets, int E,
                            const void* Wq, int w_format, int N, const float* s_x, const int32_t* zp_x,
                            const float* s_w, int G, const int32_t* wsum, void* Y, int out_dtype, int64_t ldy,
                            int64_t x_rows, qt_stream_t stream);
int qt_moe_gemm_i8_ring_w4(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R, const int32_t* offsets, int E,
                           const void* Wq, int w_format, int N, const float* s_x, const int32_t* zp_x,
                           const float* s_w, int G, const int32_t* wsum, void* Y, int out_dtype, int64_t ldy,
                           int64_t x_rows, qt_stream_t stream);
int qt_moe_gemm_i8_wide(const int8_t* Xq, int K, const int32_t* row_idx, int64_t R, const int32_t* offsets, int E,
                        const void* Wq, int w_format, int N, const float* s_x, const int32_t* zp_x, const float* s_w,
                        int G, const int32_t* wsum, void* Y, int out_dtype, int64_t ldy, int64_t x_rows,
                        qt_stream_t stream);
int qt_moe_combine(const void* Y, int dtype, int H, int64_t ldy, const int32_t* row_of, const float* weights,
                   int64_t T, int k, void* out, qt_stream_t stream);

/* ---- A16 runtime: W4A16 / W4A16_ASYM / W8A16 checkpoints on their stored integer weights ----------------------
 * Both kernels take one weight description:
 *   Wq    w_format QT_W_INT4_PACKED: int32 [N, ceil(K/8)] (qt_gemm_i8's nibble layout), or QT_W_INT8: int8 [N, K]
 *   s_w   fp32 [N, G], G = 1 (channel-wise) or ceil(K/128)
 *   zp_w  int8 [N, G] or NULL (symmetric)
 *   g_idx int32 [K] or NULL: the group of every column (actorder "group"; values clamped to [0, G)); when NULL the group of
 *         column k is k / 128 (G > 1) or 0.  Columns stay in their original order: no permutation anywhere.
 * The weight both kernels multiply is defined as engine/qlinear.py dequantized_weight computes it:
 *   w[n, k] = round_to_dtype( ((float)q[n, k] - (float)zp[n, g(k)]) * s_w[n, g(k)] )     fp32, one rounding each
 * (q - zp is exact in fp32; the product rounds once; round_to_dtype is round to nearest even.)
 *
 * qt_dequantize_weight: W [N, K] (dtype bf16 / fp16, row pitch ldw) = w, bit-identical to dequantized_weight.
 *
 * qt_gemm_wq_skinny: the decode GEMV, 1 <= M <= 16.  X [M, K] and Y [M, N] in x_dtype (bf16 / fp16), row pitches ldx /
 *   ldy; bias [N] in x_dtype or NULL.
 *     Y[m, n] = round_to_dtype( sum_k (float)x[m, k] * w[n, k]  (+ (float)bias[n]) )
 *   The products run on v_mfma_f32_16x16x32_{bf16,f16} with the activations as the B operand, M padded to 16 with zero
 *   rows: a workgroup owns 16 columns n, its 4 waves take the 128-column k-blocks kb = wave, wave + 4, ... in ascending
 *   order (one MFMA per 8 columns, fp32 accumulator), and the waves' partial sums are added in wave order, then the bias.
 *   The order is fixed and there are no atomics: two runs give the same bits.  The exact-input guarantee rests on two
 *   facts: a product of two bf16 (or two fp16) values is exact in fp32, and the MFMA's fp32 accumulation is exact
 *   whenever every partial sum is representable in fp32 (no denormals).  Inputs whose partial sums are all exact (small
 *   integer x, power-of-two scales, bounded K) therefore give round_to_dtype of the exact sum, bit for bit; for any
 *   other input |y - y_exact| <= ulp_dtype(y) / 2 + K 2^-24 sum_k |x w|.
 *   Without a zero-point the kernel forms w as fma(q + OFF, s, -OFF s) (OFF = 8 or 128, so -OFF s is exact): the same
 *   value, except that a zero weight is +0 whatever the sign of s. */
int qt_dequantize_weight(const void* Wq, int w_format, int N, int K, const float* s_w, int G, const int8_t* zp_w,
                         const int32_t* g_idx, void* W, int dtype, int64_t ldw, qt_stream_t stream);
int qt_gemm_wq_skinny(const void* X, int x_dtype, int M, int K, int64_t ldx, const void* Wq, int w_format, int N,
                      const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx, const void* bias, void* Y,
                      int64_t ldy, qt_stream_t stream);

/* qt_gemm_wq_stream: qt_gemm_wq_skinny for a few tiles of rows, 1 <= M <= QT_WQ_STREAM_MAX_M (batched decode,
 *   speculative verification, short prompts).  The arguments and the weight definition are
 *   qt_gemm_wq_skinny's.  Taken: QT_W_INT4_PACKED and QT_W_INT8, G = 1 and G = K / 128, with and without zp_w and bias,
 *   bf16 and fp16, any N >= 1, ldy >= N, K <= ldx <= QT_WQ_STREAM_MAX_LDX, K a multiple of QT_WQ_STREAM_K_UNIT, and X,
 *   Wq and ldx * 2 multiples of 16 bytes (the skinny kernel's 16-byte path).  Everything else -- g_idx != NULL (actorder group runs on
 *   qt_dequantize_weight + a dense GEMM), a ragged K, M = 0 or M > QT_WQ_STREAM_MAX_M, a misaligned operand or pitch, a
 *   null pointer, a G that is neither 1 nor K / 128, a dtype that is not 16-bit -- returns QT_ERR_INVALID before any
 *   launch, and qt_last_error names the reason.
 *   Row m of Y is bit-identical to qt_gemm_wq_skinny applied to row m alone (equivalently: to row m of the skinny kernel
 *   on any slice of at most 16 rows that holds it).  A workgroup owns 16 columns n and all M rows; wave w accumulates
 *   the k-blocks kb = w, w + 4, ... in ascending order on the same MFMA, with column 128 kb + 32 kq + 8 s + j at the
 *   same (step s, lane quarter kq, element j), one fp32 accumulator per tile of 16 rows; then ((c0 + c1) + c2) + c3,
 *   the bias, one rounding.  The weight fragment is formed by the skinny kernel's statements, once per k-block, and used
 *   for every tile of rows; a row of the MFMA's output reads its own activation row only, so a row's result depends
 *   neither on M nor on the other rows.  qt_gemm_wq_skinny's error bound and exact-input guarantee carry over.
 *   Deterministic, no atomics, no workspace.  Every weight byte is read from memory once per launch.  No byte outside
 *   X [M, K] (pitch ldx), Wq, s_w / zp_w [N, G] and bias [N] is read; nothing outside Y[m < M, n < N] is written. */
int qt_gemm_wq_stream(const void* X, int x_dtype, int M, int K, int64_t ldx, const void* Wq, int w_format, int N,
                      const float* s_w, int G, const int8_t* zp_w, const int32_t* g_idx, const void* bias, void* Y,
                      int64_t ldy, qt_stream_t stream);
#define QT_WQ_STREAM_MAX_M 128
#define QT_WQ_STREAM_K_UNIT 128
#define QT_WQ_STREAM_MAX_LDX 33554432 /* 2^25 elements: a tile of 16 rows is addressed by 32-bit byte offsets */

/* qt_gemm_wq_grouped: qt_gemm_wq_skinny over E weight matrices at once, for routed-expert banks (engine/qlinear.py
 *   WeightOnlyExperts).  Y [R, N] in x_dtype (pitch ldy): expert e owns output rows
 *   [offsets[e], offsets[e + 1]) (offsets int32 [E + 1], on the device, ascending, offsets[E] <= R; rows past
 *   offsets[E] are not written) and weight matrix e: Wq [E, N, ceil(K/8)] packed int4 or [E, N, K] int8, s_w fp32
 *   [E, N, G], zp_w int8 [E, N, G] or NULL, g_idx int32 [E, K] or NULL, each with the meaning above.  The X row of
 *   output row m is X[row_idx[m]] (row_idx int32 [R], values index rows of X [., K] of pitch ldx; the caller's
 *   contract) or X[m] when row_idx is NULL.  No bias.
 *   Every expert's rows are processed in tiles of 16 rows, in ascending order, and every row is equal to the bit to
 *   qt_gemm_wq_skinny with that expert's weight applied to that row: it is the same tile code with the same k-block
 *   order, wave order and fixed reduction, and a row of the MFMA depends on its own input row alone, so the padding
 *   rows and the other rows of the tile change nothing.  Deterministic, no atomics, no host read of the counts: the
 *   grid is ceil(N/16) column tiles x (floor(R/16) + min(E, R)) row-tile slots, an upper bound on
 *   sum_e ceil(rows_e / 16); each workgroup finds its expert and tile by walking offsets, and a surplus one exits
 *   before any weight load.  Only the experts that own rows have their weights read.  R / 16 + min(E, R) <= 65535. */
int qt_gemm_wq_grouped(const void* X, int x_dtype, int K, int64_t ldx, const int32_t* row_idx, int64_t R,
                       const int32_t* offsets, int E, const void* Wq, int w_format, int N, const float* s_w, int G,
                       const int8_t* zp_w, const int32_t* g_idx, void* Y, int64_t ldy, qt_stream_t stream);

/* qt_moe_gemm_wq_wide: qt_gemm_wq_grouped for more than a few rows per expert -- batched decode, speculative
 *   verification, short prompts.  The arguments and their meanings are qt_gemm_wq_grouped's, plus
 *   x_rows, the number of rows of X.  No bias, no workspace, no atomics.
 *   Taken: QT_W_INT4_PACKED and QT_W_INT8, G = 1 and G = K / 128, with and without zp_w, bf16 and fp16, any R >= 1 up to
 *   the slot bound below, any N >= 1, any ldy >= N, K a multiple of QT_MOE_WQ_WIDE_K_UNIT, X, Wq and ldx * 2 multiples of
 *   16 bytes, E <= QT_MOE_WQ_WIDE_MAX_E, x_rows * ldx * 2 + 2 K < 2^32 (a row of X is addressed by a 32-bit byte offset
 *   from X), and without row_idx x_rows >= R.  Everything else -- g_idx != NULL, a ragged K, a misaligned operand or
 *   pitch, a null pointer, a G that is neither 1 nor K / 128, a dtype that is not 16-bit, too many slots, the 2^32
 *   bound -- returns QT_ERR_INVALID before any launch, and qt_last_error names the reason.
 *   Every row of Y is bit-identical to qt_gemm_wq_grouped's row on the same arguments, and so to qt_gemm_wq_skinny with
 *   that expert's weight on that row alone: per output element, wave w accumulates the k-blocks kb = w, w + 4, ... in
 *   ascending order on the same MFMA with the same fragment layout, then ((c0 + c1) + c2) + c3, then one rounding;
 *   and a row of the MFMA's output reads its own activation row only.  qt_gemm_wq_skinny's error bound and
 *   exact-input guarantee carry over.  Deterministic: two runs give the same bits.
 *   A workgroup holds MT tiles of 16 rows of one expert and reads that expert's weights once for all of them.  MT is
 *   chosen on the host from R and E alone: the smallest of 1, 2, 4, 8 with 16 MT >= ceil(R / E) (8 when none is), so
 *   that evenly routed rows put one expert in one workgroup per 16 columns; no count is read on the host.  The grid is
 *   ceil(N/16) column tiles x (floor(R / (16 MT)) + min(E, R)) row-tile slots, an upper bound on
 *   sum_e ceil(rows_e / (16 MT)) for any routing (per expert ceil(r/q) <= floor(r/q) + [r > 0], and
 *   sum_e floor(r_e/q) <= floor(R/q)); that count must not exceed QT_MOE_WQ_WIDE_MAX_SLOTS = 65535.  A workgroup walks
 *   offsets, clamped to [0, R] and made ascending, to its expert and tile; a surplus one exits before its first weight
 *   load and its barrier; an expert with more than 16 MT rows takes several slots; only the experts that own rows
 *   have their weights read.
 *   row_idx values are clamped into [0, x_rows), not followed.  No byte outside X [x_rows, K] (pitch ldx),
 *   Wq [E, N, .], s_w / zp_w [E, N, G], offsets [E + 1] and row_idx [R] is read; rows >= offsets[E] are not written,
 *   and nothing outside Y[m < offsets[E], n < N] is. */
int qt_moe_gemm_wq_wide(const void* X, int x_dtype, int K, int64_t ldx, const int32_t* row_idx, int64_t R,
                        const int32_t* offsets, int E, const void* Wq, int w_format, int N, const float* s_w, int G,
                        const int8_t* zp_w, const int32_t* g_idx, void* Y, int64_t ldy, int64_t x_rows,
                        qt_stream_t stream);
#define QT_MOE_WQ_WIDE_K_UNIT 128
#define QT_MOE_WQ_WIDE_MAX_E 4096
#define QT_MOE_WQ_WIDE_MAX_SLOTS 65535

/* ---- evaluation: the LM head and its cross-entropy, logits never stored ------------------------------------------
 * qt_lm_head_nll: for every row m of H [M, K] (the final hidden states, row pitch ldh) and W [V, K] (the LM-head
 *   weight, row pitch ldw), both bf16 or both fp16 (dtype), with x[m, v] = sum_k H[m, k] W[v, k] in an fp32
 *   accumulator:
 *     lse[m]    = log sum_v exp(x[m, v])
 *     tgt[m]    = x[m, targets[m]], the fp32 accumulator of the target column, to the bit
 *     argmax[m] = the lowest v of maximal x[m, v]
 *     nll[m]    = lse[m] - tgt[m]
 *   targets is [M] int32 (target_bytes 4) or int64 (target_bytes 8).  targets[m] < 0 (the ignore index): nll[m] = 0 and
 *   tgt[m] = 0; lse[m] and argmax[m] are still written.  targets[m] >= V: nll[m] and tgt[m] are NaN -- the host cannot
 *   see device targets without a sync, so the kernel says it.  The [M, V] logits are never written: a 256 x 256 tile
 *   of them lives in the accumulators of one workgroup (the LDS-ring pipeline over K, v_mfma_f32_32x32x16_bf16 / _f16),
 *   whose epilogue masks columns >= V to -inf and leaves one record {max, sum of exp(x - max), argmax} per row and
 *   vocabulary tile in the workspace; a second kernel merges a row's records.
 *   Contract: the k order of one accumulator is fixed (ascending 64-element K-tiles, four MFMA k-steps each), and so
 *   is the tree that combines a row's columns: the lane's two columns (c, c + 128 of the tile), the 32 lanes by the
 *   xor steps 16, 8, 4, 2, 1, the four column waves in ascending order, the vocabulary tiles in ascending order, each
 *   by m = max(m1, m2), s = s1 exp(m1 - m) + s2 exp(m2 - m) with the lower columns first, ties of the maximum going
 *   to the lower index; lse = m + logf(s).  Row m's four outputs depend only on H[m, :], W, V, K and targets[m] -- not
 *   on M, the row's index, the pitches or the alignment of H.  Deterministic, no atomics.
 *   Workspace: qt_lm_head_nll_workspace_size(M, V) = 16 M ceil(V / 256) bytes of records + 4 M bytes of target
 *   logits, 16-byte aligned; a short, NULL or misaligned workspace is QT_ERR_WORKSPACE with nothing launched.
 *   M = 0 returns QT_OK and touches nothing.  QT_ERR_INVALID before any launch, with qt_last_error naming the argument:
 *   a dtype that is not bf16 or fp16 (fp32 operands are not taken); K not a multiple of QT_LM_HEAD_K_UNIT = 128,
 *   below QT_LM_HEAD_MIN_K = 128 (the smallest K the ring's prologue and drain take: one trip round its eight slots)
 *   or above QT_LM_HEAD_MAX_K = 32768; ldh < K or ldw < K; a pitch that is not a multiple of 8 elements or exceeds 2^22
 *   elements, or a base of H or W that is not 16-byte aligned; V < 1; M < 0 or M > INT32_MAX; a target_bytes that is
 *   neither 4 nor 8; a NULL H, W, targets, nll, lse, tgt or argmax.  Tile rows past M and vocabulary rows past V are
 *   fetched clamped (row M - 1, row V - 1), computed and never stored: no byte outside H [M, K], W [V, K] and
 *   targets [M] is read, nothing outside the four outputs [M] and the workspace is written.
 *   (csrc/lm_head_nll.hip) */
#define QT_LM_HEAD_K_UNIT 128
#define QT_LM_HEAD_MIN_K 128
#define QT_LM_HEAD_MAX_K 32768
size_t qt_lm_head_nll_workspace_size(int64_t M, int V);
int qt_lm_head_nll(const void* H, int64_t ldh, const void* W, int64_t ldw, int dtype, int64_t M, int K, int V,
                   const void* targets, int target_bytes, float* nll, float* lse, float* tgt, int32_t* argmax,
                   void* workspace, size_t workspace_bytes, qt_stream_t stream);

/* qt_lm_head_kl: the distance of two models that share one LM-head weight, per token and with neither [M, V] logit
 *   matrix written.  For every row m of Hp [M, K] (the original model's final hidden states, row pitch ldhp), Hq [M, K]
 *   (the quantised model's, row pitch ldhq) and W [V, K] (row pitch ldw), all bf16 or all fp16 (dtype), with
 *   a[m, v] = sum_k Hp[m, k] W[v, k] and b[m, v] = sum_k Hq[m, k] W[v, k] in fp32 accumulators, P = softmax(a[m, :]) and
 *   Q = softmax(b[m, :]):
 *     lse_p[m] = log sum_v exp(a[m, v]),  lse_q[m] = log sum_v exp(b[m, v])
 *     kl[m]    = KL(P || Q) = sum_v P[v] (a[m, v] - b[m, v]) - lse_p[m] + lse_q[m]
 *              = t / s_a - lse_p[m] + lse_q[m],  t = sum_v exp(a[m, v] - max_a) (a[m, v] - b[m, v]),
 *                s_a = sum_v exp(a[m, v] - max_a).  kl[m] is not clamped at 0: it is exactly 0 where Hp[m, :] and
 *                Hq[m, :] are equal, and rounding may leave a negative value of the size of an fp32 ulp of the lse.
 *     argmax_p[m], argmax_q[m] = the lowest v of maximal a[m, v], of maximal b[m, v]
 *     nll_p[m] = lse_p[m] - a[m, targets[m]],  nll_q[m] = lse_q[m] - b[m, targets[m]]
 *   targets as in qt_lm_head_nll: targets[m] < 0 (the ignore index) gives nll_p[m] = nll_q[m] = 0, targets[m] >= V gives
 *   NaN in both; kl, both lse and both argmax are still written.
 *   One workgroup holds 128 token rows x 256 vocabulary columns of a AND b in its accumulators: the K-tile's four
 *   half-panel units are Hp rows, two halves of W rows, Hq rows (the same 128 token rows), so a[m, v] and b[m, v] lie
 *   in one lane and a[m, v] - b[m, v] is formed in fp32 from the accumulators -- never from rounded logits.
 *   Contract: a and b are qt_lm_head_nll's accumulators of (Hp, W) and (Hq, W), and {lse_p, argmax_p, nll_p} and
 *   {lse_q, argmax_q, nll_q} are its outputs for them, to the bit: the same k order, the same records {m, s, i} and
 *   the same merge order -- the lane's two columns (c, c + 128 of the tile), the 32 lanes by the xor steps 16, 8, 4, 2,
 *   1, the four column waves in ascending order, the vocabulary tiles in ascending order.  The P record carries t as a
 *   fourth field: an element is {a, 1, v, a - b}, a masked column (>= V) {-inf, 0, v, 0}, and t merges with the weights
 *   of s: t = t1 exp(m1 - m) + t2 exp(m2 - m).  Row m's seven outputs depend only on Hp[m, :], Hq[m, :], W, V, K and
 *   targets[m] -- not on M, the row's index, the pitches or the alignment of Hp and Hq.  Deterministic, no atomics.
 *   Workspace: qt_lm_head_kl_workspace_size(M, V) = 32 M ceil(V / 256) bytes of records + 8 M bytes of target logits,
 *   16-byte aligned; a short, NULL or misaligned workspace is QT_ERR_WORKSPACE with nothing launched.
 *   M = 0 returns QT_OK and touches nothing.  QT_ERR_INVALID before any launch, with qt_last_error naming the argument:
 *   the refusals of qt_lm_head_nll, for both hidden-state operands -- a dtype that is not bf16 or fp16 (fp32 operands
 *   are not taken); K not a multiple of QT_LM_HEAD_K_UNIT, below QT_LM_HEAD_MIN_K or above QT_LM_HEAD_MAX_K; ldhp < K,
 *   ldhq < K or ldw < K; a pitch that is not a multiple of 8 elements or exceeds 2^22 elements, or a base of Hp, Hq or W
 *   that is not 16-byte aligned; V < 1; M < 0 or M > INT32_MAX; a target_bytes that is neither 4 nor 8; a NULL Hp, Hq,
 *   W, targets, kl, nll_p, nll_q, lse_p, lse_q, argmax_p or argmax_q.  Tile rows past M and vocabulary rows past V are
 *   fetched clamped (row M - 1 on each side, row V - 1), computed and never stored: no byte outside Hp [M, K],
 *   Hq [M, K], W [V, K] and targets [M] is read, nothing outside the seven outputs [M] and the workspace is written.
 *   (csrc/lm_head_kl.hip) */
size_t qt_lm_head_kl_workspace_size(int64_t M, int V);
int qt_lm_head_kl(const void* Hp, int64_t ldhp, const void* Hq, int64_t ldhq, const void* W, int64_t ldw, int dtype,
                  int64_t M, int K, int V, const void* targets, int target_bytes, float* kl, float* nll_p, float* nll_q,
                  float* lse_p, float* lse_q, int32_t* argmax_p, int32_t* argmax_q, void* workspace,
                  size_t workspace_bytes, qt_stream_t stream);

/* ---- measurement aid (bench.py roofline leg; not part of the reference surface) -------------
 * When enabled, HIP events are recorded on the launch stream immediately around the named
 * kernel; qt_profile_read synchronises them, returns the summed device time and the launch
 * count since the last read, and resets the slot. */
enum qt_prof_kernel { QT_PROF_XTX = 0, QT_PROF_SWEEP_BLOCK = 1, QT_PROF_LM_HEAD_NLL = 2, QT_PROF_NUM_KERNELS = 3 };
int qt_profile_enable(int on);
int qt_profile_read(int kernel_id, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* QUANTOOL_AMD_H */
