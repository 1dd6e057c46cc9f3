/* maest_hip.h -- C ABI of libmaest_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * MAEST mel-spectrogram -> patchout-ViT hot path.
 *
 * The reference (palonso/MAEST) is pure Python with NO plugin / operator / FFI interface: its
 * boundary for this path is the Python API get_maest() / MAEST.forward() / predict_labels() /
 * Module.training_step() (models/maest.py:1467-1569, 831-939; models/module.py:73-102), and every
 * tensor op underneath is a stock torch / torchaudio call.  This header therefore declares the
 * entry points that the drop-in Python package (maest_amd/, same API as the reference) binds with
 * ctypes; each one cites the reference call site whose library op it replaces.
 *
 * Conventions
 *  - Every function returns int status: 0 = MAEST_OK; non-zero -> maest_last_error() has the text.
 *  - All tensor arguments are CALLER-OWNED DEVICE pointers (e.g. torch.Tensor.data_ptr()), row-major,
 *    with explicit sizes / leading dimensions in ELEMENTS.  The library never allocates, frees or
 *    retains memory and never synchronises: work is enqueued on `stream` (a hipStream_t passed as
 *    void*; NULL = the null stream), so every entry point is hipGraph-capturable.
 *  - dtype codes: MAEST_F32 (fp32, "parity mode": exact-fp32 MFMA) and MAEST_BF16 (bf16 operands,
 *    fp32 accumulate, "perf mode").  The residual stream, LayerNorm statistics, softmax statistics,
 *    logits and all parameter gradients are fp32 in both modes.
 *  - No torch types, no C++ types: plain pointers and integers only.
 *  - Memory contract (pinned by tests/guard.py, which runs every entry point with each argument between NaN-filled bands):
 *      * an entry point reads and writes only [ptr, ptr + extent) of each argument, the extent being what its sizes and its leading
 *        dimension say (rows x ld elements, the last row only as wide as the logical row); a `const` argument is never written, and
 *        an output or workspace is never read before the call itself has written it (ACCUMULATED outputs excepted: the caller
 *        initialises those);
 *      * rows past a ragged edge (a partial last tile of M, N, K or of a clip's tokens) are re-read from the last valid row or
 *        zero-filled on chip -- never fetched from beyond it, not even to be multiplied by zero: the neighbour's memory may hold inf / NaN;
 *      * pad columns of a leading dimension wider than the logical row are left alone unless the entry says otherwise
 *        (maest_transpose and maest_cast_rows zero them); rows an entry declares "not written" / "untouched" keep their bytes;
 *      * a workspace of exactly the documented minimum size is enough.
 */
#ifndef MAEST_HIP_H
#define MAEST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAEST_ABI_VERSION 9

#define MAEST_OK 0
#define MAEST_ERR_INVALID 1 /* bad argument (shape / alignment / dtype) */
#define MAEST_ERR_LAUNCH 2  /* HIP launch failure */

#define MAEST_F32 0
#define MAEST_BF16 1
#define MAEST_F32X3 2 /* fp32 tensors, matrix products in split-bf16 ("bf16 x 3") precision: accepted as the INPUT dtype
                         of maest_gemm_nt / maest_gemm_tn and as the dtype of maest_attn_fwd / maest_attn_bwd only (the
                         other entry points take MAEST_F32 for the same tensors); ~2^-16 per-product error on the
                         full-rate bf16 matrix pipe */

#define MAEST_BF16_QS 4 /* bf16 qkv tensor whose q columns hold q' = scale * log2(e) * q (the factor folded into the q rows of the qkv
                           projection's operand copy by maest_cast_weights_multi: q' is rounded once, forward and backward read the
                           same operand): accepted as the dtype of maest_attn_fwd(_rows) / maest_attn_bwd(_rows) only.  `scale` stays
                           the TRUE softmax scale; dQ comes out as the gradient with respect to the true q (so the projection's
                           dgrad / wgrad run on the unscaled weights), lse and the output are those of MAEST_BF16 up to rounding. */

/* The split-bf16 ("bf16 x 3") product as ONE bf16 GEMM of three times the depth (round 5): an fp32 value x is hi + lo with hi = bf16(x),
 * lo = bf16(x - hi); a row of K values is stored as 3 K bf16 values -- activations [ hi | hi | lo ] (MAEST_SPLIT3_A), weights
 * [ hi | lo | hi ] (MAEST_SPLIT3_B) -- so that the plain bf16 GEMM over K' = 3 K accumulates hi*hi + hi*lo + lo*hi, the three terms of
 * MAEST_F32X3, on the fast bf16 kernels (gemm_nt_ow.hip).  MAEST_SPLIT3_A: accepted as y_dtype of maest_layernorm_fwd /
 * maest_add_layernorm_fwd (y: bf16 [rows, 3 * 768], ldy = 2304); MAEST_SPLIT3_B as the dtype of maest_cast_weights_multi (dst: bf16
 * [rows, 3 * cols]; dst_t must be NULL); MAEST_F32X3_A3 as the dtype of maest_attn_fwd(_rows): MAEST_F32X3 with `out` written as
 * MAEST_SPLIT3_A rows (bf16 [B * N, 3 * 768]). */
#define MAEST_SPLIT3_A 5
#define MAEST_SPLIT3_B 6
#define MAEST_F32X3_A3 7

/* GEMM epilogues */
#define MAEST_F16 3 /* IEEE half: accepted as the INPUT dtype of maest_patch_im2col only (the loader's float16 mel batches,
                       discogs/dataset.py:58-67), and as the dx dtype of its backward maest_patch_im2col_bwd */

#define MAEST_EPI_NONE 0     /* C = acc + bias                                           */
#define MAEST_EPI_GELU 1     /* C = gelu_erf(acc+bias) ; aux_out (optional) = gelu_erf'(acc+bias), saved for backward */
#define MAEST_EPI_RESIDUAL 2 /* C(fp32) = acc + bias + aux_in(fp32)                      */
#define MAEST_EPI_MUL 3      /* C = acc * aux_in   (aux_in in out_dtype; dgrad through GELU)  */
#define MAEST_EPI_ATOMIC 4   /* C(fp32) += acc   (split-K accumulate, C pre-zeroed)      */
#define MAEST_EPI_ROWDOT 5   /* internal to maest_gemm_nt_rowdot (not accepted by maest_gemm_nt) */

int maest_version(void);
const char* maest_last_error(void);

/* Which of the hand-scheduled kernels that own fixed registers are in this build.  maest_amd/build.py audits their code objects
 * (maest_amd/pw_audit.py); a kernel whose audit fails under some other hipcc is left out and the dispatch keeps the kernel it
 * replaced (same results: the forms are bit-equal for the GEMMs, equal to rounding for the attention forward).  *mask = OR of: */
#define MAEST_FORM_GEMM_NT_OW 1  /* gemm_nt_ow.hip: bf16 NT GEMM, one wave per SIMD (else the eight-wave kernel)            */
#define MAEST_FORM_GEMM_TN_OW 2  /* gemm_tn_ow.hip: bf16 wgrad GEMM, one wave per SIMD (else the eight-wave kernel)         */
#define MAEST_FORM_ATTN_FWD_PW 4 /* attn_fwd_pw.hip: persistent bf16 attention forward for N > 320 (else four-wave LDS-DMA) */
int maest_kernel_forms(int* mask);

/* ---- process-wide tuning / test switches.  Thread-safe (atomics); the defaults are taken from the environment
 * variables named below, which are read ONCE, at the first use of any switch.  restore_default != 0 ignores `value`.
 *   MAEST_OPT_GEMM_MIN_M    (env MAEST_GEMM_MIN_M,    default 8192): smallest M routed to the 256-row-tile GEMMs
 *   MAEST_OPT_GEMM_VARIANT  (env MAEST_GEMM_VARIANT,  default 0):    0 = full-line 256x256 kernels (bf16 operands, every epilogue
 *                            form incl. row-dot: four waves, one per SIMD, 128 x 128 outputs each -- gemm_nt_ow.hip / gemm_tn_ow.hip;
 *                            fp32 / split-bf16 operands and the 128-row tail tiles: eight waves -- gemm256.hip),
 *                            3 = as 0 with the eight-wave kernels for bf16 too (A/B, tests), 4 = 256-tile TN kernel at any qualifying
 *                            shape (1 / 2 selected two earlier 256-row kernels, removed in round 6)
 *   MAEST_OPT_GEMM_EPILOGUE (env MAEST_GEMM_EPILOGUE, default -1):   -1 = per-epilogue choice, 0/1/2 force a C-tile
 *                            epilogue form of the eight-wave full-line kernel (ignored by the one-wave-per-SIMD kernel, i.e. for
 *                            bf16 operands under MAEST_OPT_GEMM_VARIANT = 0) */
#define MAEST_OPT_GEMM_MIN_M 0
#define MAEST_OPT_GEMM_VARIANT 1
#define MAEST_OPT_GEMM_EPILOGUE 2
#define MAEST_OPT_ATTN_BWD 3 /* env MAEST_ATTN_BWD, default 0: fused one-pass attention backward where it applies
                                (bf16, N <= 320), query tiles fed by LDS-DMA; 1 = always the two-kernel dK/dV + dQ
                                form; (2 selected the register-fed fused form, removed in round 6: the library maps 2 to 0
                                wherever a value enters -- environment, maest_set_option, maest_set_option_thread --, so
                                maest_get_option reports 0;)
                                3 = as 0 without the persistent form (one workgroup per (batch, head) at every shape).
                                4 = as 1 with the register-staged padded tiles (the bf16 two-kernel form otherwise streams its
                                tiles by LDS-DMA, bit-equal; A/B and tests).
                                Under 0, complete backward passes with 257 <= N <= 320 run the persistent form (one
                                workgroup per CU walks its (batch, head) items, the next item's K / V / query tiles
                                arriving while the current one computes) */
#define MAEST_OPT_GEMM_TAIL 5 /* env MAEST_GEMM_TAIL, default 1: the last partial round of a large NT GEMM runs in 128-row
                                 tiles (a second launch) when at most half a round of 256-row tiles is left over; 0: off;
                                 2: every tile a 128-row tile (tests) */
#define MAEST_OPT_ATTN_FWD 6 /* env MAEST_ATTN_FWD, default 0: bf16 attention forward by shape -- N > 320 (complete passes): the
                                persistent one-wave-per-SIMD kernel (attn_fwd_pw.hip: 96 query rows per wave, K / V tiles streamed
                                by LDS-DMA across work items); otherwise four-wave workgroups with K / V tiles fed by LDS-DMA into
                                unpadded bank-swizzled tiles; 1: the register-staged, padded-pitch form every other dtype uses;
                                2: the four-wave LDS-DMA form at every N; 3: the persistent form at every N (tests) */
#define MAEST_OPT_ATTN_FWD_WAVES 7 /* env MAEST_ATTN_FWD_WAVES, default 0: waves (32-query blocks) per workgroup of the DMA-fed bf16
                                      attention forward chosen by shape; 4 / 5 / 6 / 8 force one (tests, A/B) */
#define MAEST_OPT_TN_REDUCE 8 /* env MAEST_TN_REDUCE, default 0: split-K partials of the wgrad GEMM are combined with fp32 atomics; 1:
                                 maest_gemm_tn_ws uses the workspace it is given (partial tiles stored plainly, summed in split
                                 order by a second kernel: dW repeats bit for bit at the shapes the 256-tile kernels take; no
                                 measurable cost on the training step).  NOT a reproducible wgrad by itself: colsum (the bias
                                 gradient) keeps its atomics under this switch, and so do C and colsum at the shapes gemm_tn_kernel
                                 serves (ragged M / N, few output tiles).  MAEST_OPT_DETERMINISTIC orders all of them. */
#define MAEST_OPT_GEMM_WGS 9 /* env MAEST_GEMM_WGS, default 0: the bf16 NT GEMM (gemm_nt_ow.hip) launches one workgroup per tile; n > 0:
                               at most n workgroups, workgroup b walking tiles b, b + n, ... with the next tile's first operand units
                               requested from inside the epilogue (256 = one per CU; small values make a workgroup walk several tiles
                               at test shapes) */
#define MAEST_OPT_GEMM_PANEL 10 /* env MAEST_GEMM_PANEL, default 0: the bf16 NT GEMM (gemm_nt_ow.hip) walks its tiles row-major
                                  inside an XCD's range; -1: in column panels where a traffic estimate says so (B larger than ~3 MB: N = 3072
                                  at K = 768 in panels of 6, N = 2304 in 5 + 4); n > 0: panels of n tiles.  Results do not depend on it.
                                  Measured (profiles/r06_gemm_panels.txt): fabric reads of fc1 5.8 -> 4.0 x the operand bytes, time equal
                                  (they are Infinity-Cache hits), inference step +0.4 % -- hence off by default. */
#define MAEST_OPT_DETERMINISTIC 11 /* env MAEST_DETERMINISTIC, default 0.  1: every entry point that sums gradients with fp32 atomics in an order
                                     that varies from run to run takes an ORDERED form instead, so that -- for a fixed build, device type,
                                     shapes and option values -- its results repeat bit for bit.  The default (0) launches exactly what it
                                     launched before the switch existed.  With 1:
                                     * maest_gemm_tn_ws: the split-K partials of C AND of colsum go through the caller's workspace and are
                                       summed by a second kernel in this order, per element:  s = 0;  s += partial[split] for split = 0, 1,
                                       ... (ascending K ranges; for colsum the j-tiles of a split in ascending order inside it);  dest =
                                       dest + s -- the destination LAST (the order tn256_reduce_kernel always had for C).  All three TN
                                       kernels have the form: the one-wave-per-SIMD bf16 kernel (its accumulators leave as they sit in
                                       a0 .. a255), the eight-wave kernel, and the 128 x 128 kernel that serves ragged M / N and shapes of
                                       few tiles (partials [split][M pad 128][N pad 128]).  maest_gemm_tn_workspace_bytes reports the
                                       size: C partials plus colsum partials; non-zero for every shape with more than one split.  The
                                       alignment conditions are those of MAEST_OPT_TN_REDUCE (workspace, C 16-byte aligned, ldc % 4 == 0).
                                       maest_gemm_tn (no workspace), a workspace that is too small or misaligned, or a 256-tile plan of a
                                       single split: the 128 x 128 kernel with ONE split -- one writer and one add per element of C and of
                                       colsum: reproducible, and slow at large K (a training loop passes the workspace).
                                     * maest_layernorm_bwd(_headres): the workgroups' dgamma / dbeta partials are parked in the first
                                       2 x workgroups rows of dx_out, a second kernel sums them in workgroup order (16 ascending runs of
                                       workgroups, then the runs in ascending order) and adds the sum to dgamma / dbeta last, a third
                                       computes the parked rows of dx_out / dx_lp.  dres must not alias dx_out.  dx_out = NULL with more
                                       than four rows: one workgroup (one add per column).  The order depends on rows and on
                                       MAEST_OPT_LN_BWD_BLOCKS only.
                                     * maest_head_pool_bwd: one workgroup; one add per column.
                                     * maest_token_assemble_bwd: dpatches as before; every element of d_cls, d_dist, d_new_pos, d_freq_pos
                                       and d_time_pos is summed by one thread over its tokens in ascending order, the clips in ascending
                                       order inside a token, and added once.
                                     * maest_colsum: one thread per column walks the rows in ascending order (chunks of 512 rows summed from 0, the chunk
                                       sums added in ascending order, the destination last).
                                     * maest_gemm_nt with split_k > 1 (MAEST_EPI_ATOMIC): MAEST_ERR_INVALID -- its combine has no ordered form.
                                     Scope: one process, one GPU; across builds, shapes or option values (the split counts) sums differ. */
#define MAEST_OPT_LN_BWD_BLOCKS 4 /* env MAEST_LN_BWD_BLOCKS, default 1024: workgroup cap of the LayerNorm backward grid */
int maest_set_option(int opt, int value, int restore_default);
int maest_get_option(int opt, int* value);
/* ABI 7: an override of one switch for the CALLING THREAD only (clear != 0 removes it; `value` is then ignored).  Launches made by this
 * thread see the override, every other thread the process-wide value; maest_get_option on this thread returns the override.  The
 * engine sets the launch form of a forward / backward pass this way (maest_amd/maest.py: _gemm_form), so that two models driven
 * from two threads of one process cannot change each other's launches. */
int maest_set_option_thread(int opt, int value, int clear);

/* ---- K8, K10-K12, K13 head, K4 (im2col form) and their dgrad / wgrad ---------------------------
 * nn.Linear: models/maest.py:353,355,361,376 ; :197-199,203-206 ; :572,579 ; nn.Conv2d :238-240.
 *   C[M,N] = epilogue( sum_k A[m,k] * B[n,k] )      A:[M,K] lda, B:[N,K] ldb (both k-contiguous)
 * in_dtype = dtype of A and B; out_dtype = dtype of C / aux_out (and aux_in for MUL).
 * GELU uses libm erf in fp32 mode and a 4-term erf of the Abramowitz-Stegun 7.1.26 form (|err| <= 1.7e-6) in bf16 mode.
 * K must be a multiple of 64 (bf16) / 32 (fp32): callers zero-pad.  bias: fp32 [N] or NULL. */
int maest_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, int in_dtype,
                  void* C, int64_t ldc, int out_dtype, int M, int N, int K,
                  const float* bias, int epi, const void* aux_in, void* aux_out, int64_t ld_aux,
                  int split_k, void* stream);

/* ---- the same GEMM (no epilogue other than the bias) plus, out of the same C-tile pass, the dot products of every row of
 * the STORED C (rounded to out_dtype) with the same row of `other` (out_dtype, [M, N], ld_other), per group of 64
 * columns:
 *   rowdot[((m / rows_per_item) * (N / 64) + g) * rows_per_item + m % rows_per_item] = sum_{c < 64} C[m, 64 g + c] * other[m, 64 g + c]
 * (fp32, [M / rows_per_item, N / 64, rows_per_item]).  With C = dO (the gradient of the attention output, produced by the
 * dgrad GEMM of the output projection, models/maest.py:376), other = O and rows_per_item = tokens per clip this is the
 * `delta = rowsum(dO * O)` per (clip, head, query) the attention backward needs: pass it to maest_attn_bwd_rows with
 * out = NULL and the separate pass over dO and O disappears.  N % 64 == 0, M % rows_per_item == 0.  Shapes the 256-row
 * tile kernels do not take run the plain GEMM followed by a small reduction kernel (same result). */
int maest_gemm_nt_rowdot(const void* A, int64_t lda, const void* B, int64_t ldb, int in_dtype, void* C, int64_t ldc,
                         int out_dtype, int M, int N, int K, const float* bias, const void* other, int64_t ld_other,
                         float* rowdot, int rows_per_item, void* stream);

/* ---- wgrad + bias grad, no transposed copies ("TN": both operands token-major as they sit in HBM) ----
 *   C[M,N] (fp32, ACCUMULATED: zero it first) += sum_k A[k,m] * B[k,n]      A:[K,M] lda, B:[K,N] ldb
 *   colsum[m] (fp32, ACCUMULATED, may be NULL) += sum_k A[k,m]              (= the bias gradient)
 * dW = dY^T X of nn.Linear backward with A = dY [tokens, out], B = X [tokens, in].  Any K (the token
 * tail is zero-filled in LDS); rows of A / B must be 16-byte multiples (lda / ldb) and may be wider
 * than M / N.  split_k partials are combined with fp32 atomics (MAEST_OPT_DETERMINISTIC: see there); split_k = 0 picks it
 * automatically. */
int maest_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb, int dtype, float* C,
                  int64_t ldc, int M, int N, int K, float* colsum, int split_k, void* stream);
/* The same with a caller-owned scratch buffer (ABI 5): the workspace form of the split-K combine of C, selected by
 * MAEST_OPT_TN_REDUCE = 1 (and, with the column sums ordered as well and at every shape, by MAEST_OPT_DETERMINISTIC = 1).  Given `workspace_bytes` >= the figure maest_gemm_tn_workspace_bytes reports, of 16-byte aligned device
 * memory (and C 16-byte aligned, ldc % 4 == 0), the K-split partial tiles are written to it with plain 16-byte stores and a second
 * kernel adds them to C in split order: no atomics on C, so dW is bit-reproducible from run to run (colsum still uses atomics).
 * Measured against the atomics (profiles/r03_ab_tn_workspace_combine.txt): the GEMM + reduce pair timed alone is 21 % faster at the
 * proj shape (28 splits), 6 % at qkv, equal at fc1 / fc2; the training step is equal within the pairs' spread -- opt-in because
 * there is no gain to claim, not because it costs.  workspace = NULL, a smaller buffer, the option at 0, or a shape
 * for which maest_gemm_tn_workspace_bytes reports 0 = exactly maest_gemm_tn.  The workspace is dead when the call's work on
 * `stream` has completed. */
int maest_gemm_tn_workspace_bytes(int dtype, int M, int N, int K, int split_k, int64_t* bytes);
int maest_gemm_tn_ws(const void* A, int64_t lda, const void* B, int64_t ldb, int dtype, float* C, int64_t ldc, int M, int N,
                     int K, float* colsum, int split_k, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- 2-D transpose with zero padding: dst[c, r] = src[r, c], dst rows padded to ld_dst ----------
 * (operand preparation for the wgrad GEMMs: dW = dY^T X needs both operands token-contiguous). */
int maest_transpose(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int rows, int cols,
                    int dtype, void* stream);

/* ---- fp32 -> bf16 cast of parameters, optionally also emitting the transpose ---------------------
 * dst[r,c] = bf16(src[r,c]) ; dst_t[c,r] = bf16(src[r,c]) (dst / dst_t may be NULL).
 * With dtype == MAEST_F32 it is a plain copy / transpose (parity mode). */
int maest_cast_weights(const float* src, void* dst, void* dst_t, int rows, int cols, int dtype,
                       void* stream);
/* The same for n parameters in one launch (HOST arrays of n device pointers / shapes; dst[i] or dst_t[i] may
 * be NULL): the operand-copy refresh after an optimizer step (autocast's per-call weight casts in the
 * reference, ex_maest.py:51 precision="16-mixed").  scaled_rows (HOST array of n, or NULL): rows [0, scaled_rows[i]) of dst[i] --
 * not of dst_t[i] -- are multiplied by row_scale before the rounding: the q rows of a qkv projection's forward operand copy carry
 * scale * log2(e) for MAEST_BF16_QS attention (the transposed copy, which serves the dgrad, stays unscaled). */
int maest_cast_weights_multi(int n, const float* const* src, void* const* dst, void* const* dst_t,
                             const int* rows, const int* cols, const int* scaled_rows, float row_scale, int dtype,
                             void* stream);

/* ---- K7 LayerNorm over the last dim (nn.LayerNorm: models/maest.py:395,405,499,553,571) ---------
 * x: fp32 [rows, cols] (ldx); y: y_dtype [rows, cols] (ldy); mean/rstd: fp32 [rows] or NULL.
 * cols must be 768. */
int maest_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, void* y,
                        int64_t ldy, int y_dtype, float* mean, float* rstd, int rows, int cols,
                        float eps, void* stream);
/* The residual add fused into the LayerNorm that follows it (models/maest.py:418-419 then :395/:405 of the next
 * LayerNorm): x_out[r,:] = x[r,:] + delta[r,:] (fp32, contiguous [rows, 768]; may alias x) and y = LN(x_out).
 * delta: the proj / fc2 Linear output including its bias, in delta_dtype. */
int maest_add_layernorm_fwd(const float* x, const void* delta, int delta_dtype, float* x_out, const float* gamma,
                            const float* beta, void* y, int y_dtype, float* mean, float* rstd, int rows, int cols,
                            float eps, void* stream);
/* dx_out[r,:] = dres[r,:] (may be NULL) + LN'(dy)[r,:]   (fp32), plus an optional copy of dx_out in
 * `dx_lp_dtype` (operand of the next dgrad GEMM).  dgamma/dbeta (fp32 [cols]) are ACCUMULATED
 * (atomics) -- zero them first. */
int maest_layernorm_bwd(const void* dy, int64_t lddy, int dy_dtype, const float* x, int64_t ldx,
                        const float* gamma, const float* mean, const float* rstd,
                        const float* dres, float* dx_out, void* dx_lp, int dx_lp_dtype,
                        float* dgamma, float* dbeta, int rows, int cols, void* stream);

/* The same with a COMPACT residual gradient: dres is [rows / n_tok][n_head][768] -- the first n_head tokens of every
 * clip of n_tok tokens; the other tokens' residual gradient is zero.  (Last block of the network: only the tokens the
 * head reads, cls and dist, carry a gradient above it -- models/maest.py:819-826.)  n_head = 0: dense dres / NULL. */
int maest_layernorm_bwd_headres(const void* dy, int64_t lddy, int dy_dtype, const float* x, int64_t ldx,
                                const float* gamma, const float* mean, const float* rstd,
                                const float* dres, float* dx_out, void* dx_lp, int dx_lp_dtype,
                                float* dgamma, float* dbeta, int rows, int cols, int n_tok, int n_head, void* stream);

/* ---- K9 fused softmax attention (Attention.forward: models/maest.py:362-375) ---------------------
 * qkv: [B*N, 2304] with column = s*768 + h*64 + d  (s = 0,1,2 for q,k,v), exactly the layout the
 * reference's qkv Linear produces before its reshape/permute (:362-363).
 * out: [B*N, 768] (column = h*64 + d), i.e. the reference's (attn @ v).transpose(1,2).reshape(B,N,C).
 * lse: fp32 [B, 12, N] log-sum-exp of the scaled scores (saved for backward) or NULL.
 *
 * ATTENTION MAPS.  Two flag bits, ORed into `dtype` of maest_attn_fwd_rows / maest_attn_fwd, turn the call into one that writes the
 * probabilities themselves instead of attn @ v (base codes MAEST_F32, MAEST_BF16, MAEST_BF16_QS, MAEST_F32X3; with MAEST_F32X3_A3:
 * MAEST_ERR_INVALID):
 *   MAEST_ATTN_PROBS                          out: fp32 [B, 12, q_rows, N], contiguous, EXACTLY q_rows rows per head (not the forward's rows
 *                                             up to the next multiple of 32): out[b, h, q, k] = softmax_k(scale * q_{b,h,q} . k_{b,h,k}) for
 *                                             the first q_rows queries of every clip against all N keys.
 *   MAEST_ATTN_PROBS | MAEST_ATTN_PROBS_MEAN  out: fp32 [B, q_rows, N], the mean over the heads, defined as
 *                                             (((p_0 + p_1) + p_2) + ... + p_11) * fp32(1 / 12) in fp32, heads ascending, p_h the values the
 *                                             per-head form writes: one writer per element, no atomics, bit-reproducible.
 * The kernel is self-contained: it forms every row's maximum and sum (of the unrounded exponentials, fp32) in a first pass over the keys
 * and writes 2^(t - m) / l in a second; it reads no lse of another kernel, and `lse` must be NULL (MAEST_ERR_INVALID otherwise).  qkv and
 * out 16-byte aligned, q_rows in 1..N as ever.  Under MAEST_BF16_QS the q columns hold q' and the exponent factor is 1. */
#define MAEST_ATTN_PROBS 0x100
#define MAEST_ATTN_PROBS_MEAN 0x200
int maest_attn_fwd(const void* qkv, void* out, float* lse, int B, int N, int dtype, float scale,
                   void* stream);
/* delta: fp32 [B,12,N] workspace (rowsum(dO*O)); dqkv: [B*N, 2304] same layout as qkv.
 * out == NULL: `delta` already holds rowsum(dO*O) (maest_gemm_nt_rowdot) and is only read. */
int maest_attn_bwd(const void* qkv, const void* out, const void* dout, const float* lse,
                   float* delta, void* dqkv, int B, int N, int dtype, float scale, void* stream);
/* Attention of the LAST block, where only the first q_rows tokens of a clip (cls, dist) are read by what follows
 * (final norm + head, models/maest.py:819-826): the same functions restricted to those queries; keys / values stay
 * complete.  Forward: rows / lse of queries >= roundup(q_rows, 32) are NOT written.  Backward: dout rows
 * [q_rows, roundup(q_rows, 32)) must be zero, later rows are not read (nor are out / lse there); dK, dV complete, dQ = 0
 * for every query >= q_rows.  q_rows = N is maest_attn_fwd / maest_attn_bwd.  Backward with q_rows < N is served by
 * the fused bf16 kernel only (N <= 320): MAEST_ERR_INVALID otherwise. */
/* WEIGHTED ATTENTION POOLING (the step of attention rollout).  MAEST_ATTN_APPLY | MAEST_ATTN_APPLY_ROWS(R), ORed into `dtype` of
 * maest_attn_bwd_rows / maest_attn_bwd (base codes those of MAEST_ATTN_PROBS: MAEST_F32, MAEST_F32X3, MAEST_BF16 -- the half build: IEEE
 * half --, MAEST_BF16_QS; MAEST_F32X3_A3: MAEST_ERR_INVALID), turns the call into R <= 8 row vectors times the head-mean attention matrix,
 * without an N x N write:
 *   dout  = W, fp32 [B, R, N].  Only columns < q_rows are read; columns >= q_rows may hold anything (NaN included).
 *   dqkv  = Y, fp32 [B, R, N], contiguous: the call writes exactly these elements.
 *   delta = workspace, fp32 [B, 12, N]: rows < q_rows of each (clip, head) are written with lse2 = m + log2(l), the row statistic in the
 *           log2 domain; nothing beyond them.
 *   out, lse must be NULL (MAEST_ERR_INVALID otherwise; `out` carries dO under MAEST_ATTN_APPLY_GRAD, below): like the maps, the call
 *           normalises by its own arithmetic.
 * With c2 as for the forward (scale * log2 e; 1 under MAEST_BF16_QS) and t_h[q, k] = c2 * q_h . k_h on the operands as stored,
 *   Y[b, r, k] = fp32(1 / 12) * (((s_0 + s_1) + s_2) + ... + s_11),   s_h = sum_{q < q_rows} W[b, r, q] * 2^(t_h[q, k] - lse2_h[q]),
 * heads ascending, the order of the sum over q the kernel's own but fixed, one writer per element, no atomics: two calls are bit-identical.
 * P and W stay fp32 in this product in every mode; only q k^T takes the mode's arithmetic.  q_rows in 1..N (maest_attn_bwd: q_rows = N);
 * qkv, dout, delta, dqkv 16-byte aligned. */
#define MAEST_ATTN_APPLY 0x400
#define MAEST_ATTN_APPLY_ROWS(r) (((r) - 1) << 16)     /* R = 1 .. 8 weight rows */
/* GRADIENT-WEIGHTED POOLING (the step of gradient-weighted attention rollout: Chefer, Gur & Wolf 2021, self-attention rule).
 * MAEST_ATTN_APPLY_GRAD, valid only together with MAEST_ATTN_APPLY (alone, or with MAEST_ATTN_PROBS*: MAEST_ERR_INVALID), pools the
 * rectified product of every probability with its gradient instead of the probability:
 *   out   = dO, [B * N, 768] of the operand type (column = head * 64 + d), 16-byte aligned: the gradient of a scalar with respect to the
 *           attention output, as maest_attn_bwd takes it in `dout`.  Only rows < q_rows of each clip are read; later rows may hold anything
 *           (NaN included).  Without the flag `out` must stay NULL.
 *   lse stays NULL; dout = W, delta = the lse2 workspace and dqkv = Y keep the meaning, the shapes and the base codes of the plain form.
 * With p_h[q, k] = 2^(t_h[q, k] - lse2_h[q]) as above and g_h[q, k] = dO_h[q] . V_h[k] (the v columns as stored; under MAEST_BF16_QS only the
 * q columns are pre-scaled),
 *   Y[b, r, k] = fp32(1 / 12) * (((s_0 + s_1) + s_2) + ... + s_11),   s_h = sum_{q < q_rows} W[b, r, q] * max(p_h[q, k] * g_h[q, k], 0),
 * in the order and with the single writer of the plain form: two calls are bit-identical.  p, g, W and the sums are fp32 in every mode;
 * q k^T and dO V^T take the mode's arithmetic. */
#define MAEST_ATTN_APPLY_GRAD 0x800
/* PER-HEAD POOLING (which heads carry the pooled attention, or the evidence for a label).  MAEST_ATTN_APPLY_HEADS, valid only together
 * with MAEST_ATTN_APPLY, with or without MAEST_ATTN_APPLY_GRAD (alone, or with MAEST_ATTN_PROBS*: MAEST_ERR_INVALID; base codes those of
 * the plain form, MAEST_F32X3_A3: MAEST_ERR_INVALID), keeps the twelve heads of the pooling apart instead of averaging them:
 *   dqkv  = Y, fp32 [B, 12, R, N], contiguous, 16-byte aligned: the call writes exactly these elements.
 *   dout = W, delta = the lse2 workspace [B, 12, N], out (dO under MAEST_ATTN_APPLY_GRAD, else NULL), lse = NULL, q_rows and the tails
 *           that may hold anything keep the meaning and the shapes they have without the flag.
 *   Y[b, h, r, k] = s_h, with s_h exactly the per-head term defined above for the plain form and, under MAEST_ATTN_APPLY_GRAD, for the
 *           gradient-weighted form: no sum over the heads and no 1 / 12.
 * IDENTITY: fp32(1 / 12) * (((Y[b, 0] + Y[b, 1]) + Y[b, 2]) + ... + Y[b, 11]), evaluated in fp32 (every add and the product rounded once,
 * in this order), is BIT-IDENTICAL to what the same call without the flag writes: per head both forms run the same arithmetic in the same
 * order.  One writer per element, no atomics: two calls are bit-identical. */
#define MAEST_ATTN_APPLY_HEADS 0x1000
/* TOKEN COUNTS PER CLIP (ragged batches: MAEST.forward_tokens(ragged=True), MAEST.forward_lengths, perturbation_curve(by="mass")).
 * MAEST_ATTN_LENS, ORed into `dtype` of maest_attn_fwd_rows / maest_attn_fwd (base codes MAEST_F32, MAEST_F32X3, MAEST_F32X3_A3, MAEST_BF16
 * -- the half build: IEEE half --, MAEST_BF16_QS), turns the call into an evaluation form in which every clip attends over its own number
 * of tokens.  Under the flag `lse` is NOT an output: it carries
 *   n_tok = (const int32_t*) lse, [B], on the device, 4-byte aligned, only read.  NULL: MAEST_ERR_INVALID.  No lse is saved.
 * Clip b has n_b = n_tok[b] real tokens, 1 <= n_b <= N: rows [0, n_b) of its N-row slab of qkv (the pitch stays N).  Values outside 1..N
 * are the caller's error (the Python layer checks them; the kernels do not).
 *   keys >= n_b are not attended, and rows >= n_b of qkv are never read: they may hold anything, NaN included (the tile rows the kernels
 *           clamp to row N - 1 without the flag are clamped to row n_b - 1).
 *   out rows q < n_b: softmax attention over the clip's n_b keys -- the key tiles are walked in the order and with the masking of an
 *           unflagged call at B = 1, N = n_b on those rows: BIT-IDENTICAL to it in every form (and to the unflagged call when n_b = N).
 *   out rows n_b <= q < N that the call would have written without the flag (q_rows < N: those below roundup(q_rows, 32), as ever) are
 *           written as zeros (+0.0; under MAEST_F32X3_A3 all three thirds), so that padded rows stay finite and repeatable through the
 *           per-token kernels behind; rows the unflagged call leaves unwritten stay unwritten.
 * Work is skipped: a workgroup or wave whose queries are all >= n_b writes its zeros and leaves, and the key loop runs ceil(n_b / 64)
 * tiles; padded tiles are not loaded.  The cost is sum_b n_b^2, not B N^2.  16-bit operands take the LDS-DMA kernel at every N (the
 * persistent N > 320 kernel knows no counts); MAEST_OPT_ATTN_FWD = 1 and MAEST_OPT_ATTN_FWD_WAVES keep their meaning.
 * Together with MAEST_ATTN_PROBS*: MAEST_ERR_INVALID.  maest_attn_bwd(_rows) does not know the flag: MAEST_ERR_INVALID. */
#define MAEST_ATTN_LENS 0x2000
int maest_attn_fwd_rows(const void* qkv, void* out, float* lse, int B, int N, int dtype, float scale, int q_rows,
                        void* stream);
int maest_attn_bwd_rows(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                        int B, int N, int dtype, float scale, int q_rows, void* stream);
/* Rows of the first n_head tokens of every clip, [clips][n_tok][768] -> compact [clips][n_head][768] (dtype fp32 / bf16),
 * and back: dst rows [0, n_pad) of every clip = the compact rows followed by zeros, rows >= n_pad untouched.
 *
 * GRID POOLS (the hidden states: MAEST.hidden_states, pools "time" / "freq").  MAEST_GATHER_POOLS | MAEST_GATHER_POOLS_T(Tk), ORed into `dtype`
 * of maest_gather_head_rows, turns the call into one that also pools the patch rows behind the head rows.  The base code must be MAEST_F32
 * (the operands are fp32 in both builds).  With h = n_head and P = n_tok - h the call needs P > 0, Tk >= 1 and P % Tk == 0; Fk = P / Tk: the
 * patch rows of a clip are an Fk x Tk grid in frequency-major order, row h + f * Tk + t = (frequency patch f, time patch t).
 *   src: fp32 [clips][n_tok][768], only read.   dst: fp32 [clips][h + 1 + Fk + Tk][768], contiguous; both 16-byte aligned.
 *   dst row 0 .. h-1        the head rows of src, copied bit for bit
 *   dst row h               s / (float)P,   s = (..((0.0f + x[h]) + x[h+1]) + ..) over the patch rows in ascending order: the statement of
 *                           maest_embed_pool (for h = 2 the first three rows are bit-identical to its output)
 *   dst row h + 1 + f       (sum_t x[h + f * Tk + t]) / (float)Tk,   t ascending        (the mean over time of frequency patch f)
 *   dst row h + 1 + Fk + t  (sum_f x[h + f * Tk + t]) / (float)Fk,   f ascending        (the mean over frequency of time patch t)
 * Every sum starts at 0.0f, its adds are fp32 in the stated order, then one IEEE division; one writer per element, no atomics, no partial
 * sums combined across lanes: two calls are bit-identical, with and without MAEST_OPT_DETERMINISTIC.  The call writes exactly these elements.
 * MAEST_ERR_INVALID: a base code other than MAEST_F32 beside the flag, Tk = 0, P % Tk != 0, n_tok == n_head, any other bit of bits 8 .. 15,
 * a misaligned pointer.  Without the flag the entry point is what it was (Tk bits alone: "bad dtype"). */
#define MAEST_GATHER_POOLS 0x100
#define MAEST_GATHER_POOLS_T(t) ((t) << 16)     /* Tk = 1 .. 32767 kept time patches */
int maest_gather_head_rows(const void* src, int clips, int n_tok, int n_head, int dtype, void* dst, void* stream);
int maest_scatter_head_rows(const void* src, int clips, int n_tok, int n_head, int n_pad, int dtype, void* dst,
                            void* stream);

/* ---- K16 + K4 operand: mixup + im2col of the 16x16 / stride-10 patches ---------------------------
 * PatchEmbed.forward (models/maest.py:243-256) fused with Module.training_step's mixup
 * (models/module.py:77-83) and with EVERY patchout variant of models/maest.py:678-780 (structured time /
 * frequency, fixed index lists, interleaved, unstructured): the host resolves them into one list of kept
 * patch tokens and dropped patches are never computed -- mathematically identical to compute-then-drop.
 * x: [B, F, T] in x_dtype = MAEST_F32 or MAEST_F16 (the loader hands out float16 mel batches, discogs/dataset.py:58-67;
 * a half sample is widened exactly as x.float() would, in the load); perm: int32 [B] or NULL; lam: fp32 [B] or NULL (x' = lam*x + (1-lam)*x[perm]).
 * tok_ft: int32 [P, 2] = (frequency patch index f, time patch index t) of each kept token, in sequence
 * order.  out: dtype [B*P, 256], row = b*P + j, col = ky*16 + kx, patch origin (10 f, 10 t).
 * Optional K17 SpecMasking fused into the same load (helpers/spec_masking.py:27-33; the loader masks each clip
 * before the batch is mixed up, discogs/datamodule.py:140-152): t_stripes int32 [B, n_t, 2] / f_stripes int32
 * [B, n_f, 2] = (start, width) per clip, as in maest_spec_mask; a masked sample reads as 0.0 (for the clip and,
 * with its own stripes, for its mixup partner).  n_t = n_f = 0 (pointers may be NULL) disables it. */
int maest_patch_im2col(const void* x, int x_dtype, int B, int F, int T, const int32_t* perm, const float* lam,
                       const int32_t* tok_ft, int P, const int32_t* t_stripes, int n_t,
                       const int32_t* f_stripes, int n_f, void* out, int dtype, void* stream);
/* The same with the convolution's stride as an argument (ABI 8): patch origin (stride_f * f, stride_t * t).  The reference takes the
 * strides as constructor arguments (get_maest(stride_f=, stride_t=): models/maest.py:1505-1507, 1537; PatchEmbed: models/maest.py:214-241) and
 * only warns that the checkpoints were trained with (10, 10); maest_patch_im2col is this entry with (10, 10). */
int maest_patch_im2col_strided(const void* x, int x_dtype, int B, int F, int T, int stride_f, int stride_t, const int32_t* perm,
                               const float* lam, const int32_t* tok_ft, int P, const int32_t* t_stripes, int n_t,
                               const int32_t* f_stripes, int n_f, void* out, int dtype, void* stream);
/* KEPT TOKENS PER CLIP (the perturbation curves: MAEST.forward_tokens, MAEST.perturbation_curve).  MAEST_IM2COL_CLIP_TOKENS, ORed into
 * `dtype` (the output code) of maest_patch_im2col_strided -- and of maest_patch_im2col, which forwards to it --, gives every clip a table of
 * its own: the reference's unstructured patchout (u_patchout, models/maest.py:773-780) with a chosen index list per clip.
 *   tok_ft: int32 [B, P, 2], only read; every clip keeps the same number P of tokens.  With prow = b * P + j (64-bit),
 *           fw = tok_ft[2 * prow], t = tok_ft[2 * prow + 1], f = fw & ~MAEST_TOK_BLANK.
 *   out[prow, ky * 16 + kx] = m(b, s_f * f + ky, s_t * t + kx)                                            without mixup,
 *                           = m(b, ..) * lam[b] + m(perm[b], ..) * (1.0f - lam[b])                        with it: the partner at clip b's (f, t),
 *     m(c, r, s) = 0.0f where sample (r, s) lies in one of clip c's stripes, else (float)x[c, r, s]: the arithmetic of the shared form,
 *     element by element, rounded to the output type as there (fp32: stored as is).  x in MAEST_F32 or MAEST_F16, every stride, every
 *     stripe list, out in MAEST_F32 or MAEST_BF16 (the half build: IEEE half) as without the flag.  All index arithmetic is 64-bit.
 *   MAEST_TOK_BLANK, a bit of the f word of an entry, honoured under the flag only: out[prow, 0 .. 255] = +0.0 -- all-zero bits in both
 *     output types --, after mixup and stripes, and NO element of x is read for that row (neither the clip's nor its partner's: the row is
 *     zero over NaN samples too).  f and t must still be valid positions: the token keeps its positional terms in maest_token_assemble,
 *     which takes the table with the bit cleared.  A table without blank bits gives what the shared form gives clip by clip, bit for bit.
 * The call writes exactly out[0 .. B * P * 256).  MAEST_ERR_INVALID: any other bit above bit 7 beside the flag ("unknown flag bits"), a
 * base code other than MAEST_F32 / MAEST_BF16.  Without the flag the entry point is what it was (any bit above the base code: "bad dtype").
 * maest_patch_im2col_bwd, HIP-graph replay and the outputs that save activations do not take per-clip tables.
 * maest_token_assemble needs no flag: called with B = 1, P = B * P and the flattened table it writes every clip's patch rows in (b, j)
 * order behind one cls and one dist row, with the arithmetic of the [B, 2 + P, 768] call per element (maest_amd/ops.py: token_assemble_clips). */
#define MAEST_IM2COL_CLIP_TOKENS 0x100
#define MAEST_TOK_BLANK 0x40000000

/* Backward of maest_patch_im2col_strided (ABI 9): the gradient w.r.t. its input x, for a loss that reaches the mel input
 * through the patch-embedding convolution (autograd of PatchEmbed.forward, models/maest.py:243-256, with the mixup of
 * models/module.py:77-83 and the SpecMasking of helpers/spec_masking.py:27-33 in front of it).  Every option of the forward:
 * dcols: dtype [B*P, 256] (MAEST_F32 / MAEST_BF16), the gradient of `out`; stride_f / stride_t, perm / lam, tok_ft, t_stripes /
 * f_stripes exactly as the forward got them.  dx: x_dtype [B, F, T] (MAEST_F32 or MAEST_F16: the dtype the forward read), fully
 * written:  dx[c] = lam[c] * g_c + sum_{b : perm[b] == c} (1 - lam[b]) * g_b, where g_b scatters the rows of clip b back onto
 * the samples they read (no mixup: dx[c] = g_c).  A sample that no kept patch covers, or that lies inside one of clip c's stripes,
 * gets exactly 0.  tok_ft must list distinct (f, t) positions.  Deterministic: one gather per sample in a fixed order, no atomics.
 * work: int32 device workspace of work_elems >= Fp * Tp (+ 2 * B + 1 with mixup) elements, Fp = (F - 16) / stride_f + 1,
 * Tp = (T - 16) / stride_t + 1: the (f, t) -> token lookup and the mixup partner lists are built there on the device, so the
 * call makes no host round trip.  perm / lam may be NULL together; t_stripes / f_stripes may be NULL with n_t / n_f = 0. */
int maest_patch_im2col_bwd(const void* dcols, int dtype, int B, int F, int T, int stride_f, int stride_t,
                           const int32_t* perm, const float* lam, const int32_t* tok_ft, int P, const int32_t* t_stripes,
                           int n_t, const int32_t* f_stripes, int n_f, int32_t* work, int64_t work_elems, void* dx,
                           int x_dtype, void* stream);

/* ---- K5 + K6: positional add + token assembly (models/maest.py:645-675, 769, 785-796) ------------
 * patches: fp32 [B*P, 768] (conv output incl. bias); x0: fp32 [B, 2 + P, 768]
 *   x0[b,0] = cls + new_pos[0]; x0[b,1] = dist + new_pos[1];
 *   x0[b, 2 + j] = (patches[b*P + j] + time_pos[:, toffset + t_j]) + freq_pos[:, f_j]
 * time_pos: fp32 [768, Tt]; freq_pos: fp32 [768, Fg]. */
int maest_token_assemble(const float* patches, const float* cls_token, const float* dist_token,
                         const float* new_pos, const float* freq_pos, const float* time_pos, int Fg,
                         int Tt, int toffset, const int32_t* tok_ft, int B, int P, float* x0,
                         void* stream);
/* Backward of the above: dx0 fp32 [B, 2+P, 768] -> dpatches (dtype, [B*P, 768]) and ACCUMULATED
 * fp32 grads d_cls[768], d_dist[768], d_new_pos[2,768], d_freq_pos[768,Fg], d_time_pos[768,Tt]. */
int maest_token_assemble_bwd(const float* dx0, int B, int P, int Fg, int Tt, int toffset,
                             const int32_t* tok_ft, void* dpatches, int dtype, float* d_cls,
                             float* d_dist, float* d_new_pos, float* d_freq_pos, float* d_time_pos,
                             void* stream);

/* ---- K13 / K14: final LayerNorm on the cls/dist tokens + feature pooling -------------------------
 * models/maest.py:806-810, 905-906: xn = LN_eps(x)[:, 0:2]; cls = xn[:,0]; dist = xn[:,1];
 * feat = (cls + dist)/2.   x: fp32 [B, N, 768].  Outputs fp32 [B,768] each; mean/rstd fp32 [B,2]. */
int maest_head_pool_fwd(const float* x, int B, int N, const float* gamma, const float* beta, float eps,
                        float* cls, float* dist, float* feat, float* mean, float* rstd, void* stream);
/* d_cls_total = d_cls + d_feat/2 (either may be NULL), same for dist; writes dx fp32 [B,N,768]
 * rows 0,1 (all other rows are ZEROED), accumulates dgamma/dbeta. */
int maest_head_pool_bwd(const float* d_cls, const float* d_dist, const float* d_feat, const float* x,
                        int B, int N, const float* gamma, const float* mean, const float* rstd,
                        float* dx, float* dgamma, float* dbeta, void* stream);
/* early-exit embedding (models/maest.py:825-829): emb[b] = cat(x[b,0], x[b,1], mean(x[b,2:], 0)) */
int maest_embed_pool(const float* x, int B, int N, float* emb, void* stream);
/* Backward of maest_embed_pool (ABI 9; autograd of the early-exit cat in forward_features, models/maest.py:825-829):
 * d_emb fp32 [B, 2304] -> dx fp32 [B, N, 768], fully written: rows 0 and 1 get d_emb[:, :768] and d_emb[:, 768:1536], every
 * token row n >= 2 gets d_emb[:, 1536:] / (N - 2).  dx_lp: the same rows in the 16-bit operand type (dx_lp_dtype = MAEST_BF16)
 * for the block backward's dgrad GEMM, as maest_layernorm_bwd's dx_lp; may be NULL. */
int maest_embed_pool_bwd(const float* d_emb, int B, int N, float* dx, void* dx_lp, int dx_lp_dtype, void* stream);

/* ---- K18: BCE-with-logits, mean reduction (models/module.py:90, 299-301) ------------------------
 * loss (fp32 scalar, ACCUMULATED: zero it first) += weight * mean(max(z,0) - z*y + log1p(exp(-|z|)))
 * dlogits = weight * (sigmoid(z) - y) / (rows*cols)  (or NULL).
 * Optional fused label mixup: y' = lam[b]*y[b] + (1-lam[b])*y[perm[b]]. */
int maest_bce_logits(const float* z, const float* y, const int32_t* perm, const float* lam, int rows,
                     int cols, float weight, float* loss, float* dlogits, void* stream);

/* ---- K15: predict_labels tail (models/maest.py:936-938): act[c] = mean_b sigmoid(z[b,c]) */
int maest_sigmoid_mean(const float* z, int rows, int cols, float* act, void* stream);

/* ---- column sums (bias gradients): out[c] += sum_r src[r,c]  (fp32 out, ACCUMULATED) */
int maest_colsum(const void* src, int64_t ld, int rows, int cols, int dtype, float* out, void* stream);

/* ---- K17 SpecMasking on explicit stripes (helpers/spec_masking.py:27-33): zero x[b,:,s:s+w] for the
 * time stripes and x[b,s:s+w,:] for the frequency stripes.  stripes: int32 [B, n, 2] (start,width). */
int maest_spec_mask(float* x, int B, int F, int T, const int32_t* t_stripes, int n_t,
                    const int32_t* f_stripes, int n_f, void* stream);

/* ---- K1-K3 fused log-mel front end (models/helpers/melspectrogram.py:47-60) -----------------------
 * wave: fp32 [B, S]; out: fp32 [B, 96, T] with T = 1 + S/256.  window: fp32 [512] periodic Hann;
 * fb_start/fb_len: int32 [96] first FFT bin and number of non-zero taps of each mel band;
 * fb_w: fp32 [96, fb_stride] tap weights; twiddle: fp32 [512, 2] = (re, im) of exp(-2*pi*i*k/512).
 * out = (log10(1 + log_scale * mel) - norm_mean) / norm_2std.  Requires S > 256 (reflect padding). */
int maest_logmel(const float* wave, int B, int S, const float* window, const float* twiddle,
                 const int32_t* fb_start, const int32_t* fb_len, const float* fb_w, int fb_stride,
                 float log_scale, float norm_mean, float norm_2std, float* out, void* stream);
/* Backward of maest_logmel (added within ABI version 9: a new entry, no existing one changes).
 * grad_out: fp32 [B, 96, T] = dL/dout; dwave: fp32 [B, S] = dL/dwave (written, not accumulated).  The forward's arguments as there;
 * bin_band: int32 [257, 2] and bin_w: fp32 [257, 2] = the transpose of the filterbank: the (at most two) bands of each FFT bin and
 * their weights (an unused slot: band 0, weight 0).  norm_mean does not enter the gradient.  work: fp32 scratch of
 * work_elems >= B * T * 512 floats (the windowed gradient of every frame before overlap-add).  Deterministic: every dwave sample is
 * summed by one thread in a fixed order, reflect folds included; the spectrum is recomputed from wave. */
int maest_logmel_bwd(const float* wave, const float* grad_out, int B, int S, const float* window, const float* twiddle,
                     const int32_t* fb_start, const int32_t* fb_len, const float* fb_w, int fb_stride,
                     const int32_t* bin_band, const float* bin_w, float log_scale, float norm_mean, float norm_2std,
                     float* work, int64_t work_elems, float* dwave, void* stream);
/* The log-mel of maest_logmel into the on-disk mel file's layout (added within ABI version 9): a RAGGED batch of tracks packed in
 * `wave` (fp32, total_in samples) -> IEEE half rows [frame][96] = log10(1 + log_scale mel), no z-norm, rounded to nearest even, packed
 * in `rows` (total_rows rows, 16-byte aligned).  tracks: int64 [n_tracks][5] = {sample offset, S > 256, first frame f0, frame count n,
 * row offset}: frames f0 .. f0 + n - 1 of the track's T = 1 + S / 256 (framing and reflect padding per track as maest_logmel) go to rows
 * row offset .. + n - 1.  block_start: int32 [n_tracks + 1], the first block of each track (ceil(n / 64) blocks each), n_blocks = its last
 * entry.  The device tables are not read here: an entry outside the buffers is computed on valid memory and stores nothing.  Each
 * track's frame values are those of maest_logmel (norm_mean 0, norm_2std 1) bit for bit; a track starting on an 8-byte boundary
 * takes the aligned fetch in its interior. */
int maest_logmel_rows_f16(const float* wave, int64_t total_in, const int64_t* tracks, const int32_t* block_start, int n_tracks,
                          int n_blocks, const float* window, const float* twiddle, const int32_t* fb_start, const int32_t* fb_len,
                          const float* fb_w, int fb_stride, float log_scale, void* rows, int64_t total_rows, void* stream);
/* Polyphase resampler, a ragged batch (added within ABI version 9): torchaudio.functional.resample's sinc_interp_hann with the rates
 * reduced by their gcd to orig -> new_rate.  Output j = new_rate q + p of a track = sum_i taps[i][p] x[orig q + first[p] + i - width],
 * x = the track (zero outside it).  taps: fp32 [n_taps][new_rate] (each phase's non-zero band, zero-padded to n_taps), first: int32
 * [new_rate].  tracks: int64 [n_tracks][4] = {input offset, input length, output offset, output length}; block_start: int32
 * [n_tracks + 1], 256 outputs per block, n_blocks = its last entry.  Entries outside the buffers store nothing. */
int maest_resample(const float* in, int64_t total_in, const int64_t* tracks, const int32_t* block_start, int n_tracks,
                   int n_blocks, int orig, int new_rate, int width, const float* taps, const int32_t* first, int n_taps,
                   float* out, int64_t total_out, void* stream);

/* ---- second mel parameterisation: AugmentMelSTFT (models/preprocess.py:17-128; north_star names the file, the
 * reference's MAEST path never calls it).  wave: fp32 [B, S] at 32 kHz; out: fp32 [B, n_mels, T], T = 1 + (S-1)/320.
 * y = pre0*x[n] + pre1*x[n+1] (pre-emphasis, reference [-0.97, 1]); STFT n_fft 1024 / hop 320 / center / reflect with
 * `window` = the 800-point non-periodic Hann zero-padded to 1024; power; band-sparse filterbank over 513 bins
 * (fb_start / fb_len / fb_w as in maest_logmel); out = (log(mel + log_eps) + norm_add) / norm_div.
 * twiddle: fp32 [1024, 2] = exp(-2*pi*i*k/1024).  n_mels <= 128. */
int maest_augment_mel(const float* wave, int B, int S, const float* window, const float* twiddle,
                      const int32_t* fb_start, const int32_t* fb_len, const float* fb_w, int fb_stride,
                      int n_mels, float pre0, float pre1, float log_eps, float norm_add, float norm_div,
                      float* out, void* stream);
/* Backward of maest_augment_mel (added within ABI version 9: a new entry, no existing one changes).
 * grad_out: fp32 [B, n_mels, T] = dL/dout; dwave: fp32 [B, S] = dL/dwave (written, not accumulated).  The forward's arguments as there
 * (norm_add does not enter the gradient and is not passed); bin_band: int32 [513, 2] and bin_w: fp32 [513, 2] = the transpose of the
 * filterbank: the (at most two) bands of each FFT bin and their weights (an unused slot: band 0, weight 0).  work: fp32 scratch of
 * work_elems >= B * T * 1024 floats (the windowed gradient of every frame before overlap-add).  Requires S > 513, 1 <= n_mels <= 128,
 * fb_stride > 0.  Deterministic: every dwave sample is summed by one thread in a fixed order, both reflect folds and the pre-emphasis
 * adjoint included; the spectrum is recomputed from wave, nothing is saved by the forward.  Masked stripes (training mode): zero them
 * in a copy of grad_out first (maest_spec_mask); grad_out is only read. */
int maest_augment_mel_bwd(const float* wave, const float* grad_out, int B, int S, const float* window, const float* twiddle,
                          const int32_t* fb_start, const int32_t* fb_len, const float* fb_w, int fb_stride, int n_mels,
                          const int32_t* bin_band, const float* bin_w, float pre0, float pre1, float log_eps, float norm_div,
                          float* work, int64_t work_elems, float* dwave, void* stream);

/* ---- optimizer-side helper: scale a flat fp32 gradient bucket (after the RCCL all-reduce) */
int maest_scale_f32(float* x, int64_t n, float alpha, void* stream);
/* x *= *alpha_dev with the factor read from DEVICE memory: the upstream gradient of the scalar loss applied to the
 * logit gradients (autograd of F.binary_cross_entropy_with_logits, models/module.py:90) without a host round trip */
int maest_scale_dev_f32(float* x, int64_t n, const float* alpha_dev, void* stream);
/* dst[r, c] = cast(src[r, c]) for c < cols and 0 for cols <= c < ld_dst: fp32 rows (the logit gradients [B, C]) ->
 * zero-padded operand rows of the head's dgrad / wgrad GEMMs (K must be a multiple of 64 there) */
int maest_cast_rows(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int rows, int cols, int dtype,
                    void* stream);
/* stochastic weight averaging of n parameters in one launch (HOST arrays of device pointers / sizes):
 * avg[i] += (cur[i] - avg[i]) * inv_count   (Lightning StochasticWeightAveraging.avg_fn, helpers/swa_callback.py) */
int maest_swa_update_multi(int n, float* const* avg, const float* const* cur, const int64_t* numel,
                           float inv_count, void* stream);
/* x = (x + add) / div in place (AugmentMelSTFT's "fast normalization" after the training-time masks,
 * models/preprocess.py:129) */
int maest_affine_f32(float* x, int64_t n, float add, float div, void* stream);

/* ---- on-disk mel chunks -> network input (the step before the hot path) ------------
 * Replaces DiscogsDataset.load_melspectrogram (discogs/dataset.py:69-140) + norm_func
 * (discogs/datamodule.py:126-136) for a whole batch.
 * frames: raw float16 rows [sum_b frames_read[b], n_bands] as stored on disk (helpers/
 * melspectrogram_extractor.py:44-48), clip b starting at row row_start[b] (device arrays).
 * out: fp32 [B, n_bands, T]; clip b = its frames_read[b] <= T frames, zero padded to T, the padding
 * centred by a roll of (T - frames_read) / 2, transposed; with normalize != 0 then (x - mean) / div with both
 * constants and both results rounded to float16 exactly as numpy evaluates the reference expression. */
int maest_melfile_assemble(const uint16_t* frames, const int64_t* row_start, const int32_t* frames_read,
                           int B, int n_bands, int T, int normalize, float norm_mean, float norm_div,
                           float* out, void* stream);

/* ---- training-time regularisers: element dropout and stochastic depth (added within ABI version 9: new entries only) -----------
 * Reference: MAEST(drop_rate=, drop_path_rate=), models/maest.py:452-454; pos_drop :800, Attention.proj_drop :354-377, Mlp.drop
 * :200-207, DropPath in Block.forward :404-419 with per-block rates linspace(0, drop_path_rate, depth) :532-546.
 *
 * RANDOM NUMBERS.  Masks are never stored and never passed in: every kernel recomputes them from a counter, and the counter is made of
 * the element's coordinates, not of a buffer layout -- every engine path draws the same mask for the same element.
 *   generator   Philox4x32-10: multipliers 0xD2511F53 (on counter word 0), 0xCD9E8D57 (on word 2), Weyl constants 0x9E3779B9, 0xBB67AE85
 *               added to the key words after each round.  philox(counter 0,0,0,0; key 0,0) = 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 *   key         (seed & 0xffffffff, seed >> 32) of a 64-bit seed.
 *   dropout     at a site of width C (768 or 3072), element (clip b, token t, column c), N = the clip's FULL token count:
 *               e = ((b * N + t) * C + c) >> 2; counter = (e & 0xffffffff, e >> 32, site, step); output word c & 3.  One call serves
 *               the four consecutive columns a lane holds as a float4 / 4 x 16-bit group.
 *   drop-path   clip b: counter = (b >> 2, 0, site, step); output word b & 3.
 *   keep rule   an element (a clip) is kept iff word >= thr, thr = (uint32) floor(p * 2^32) computed by the caller; a kept value is
 *               multiplied by `scale` = 1 / (1 - p), a dropped one by 0.  thr = 0 keeps everything.
 *   sites       block i: 8 i + 0 proj_drop, 8 i + 1 drop-path of the attention branch, 8 i + 2 Mlp.drop behind fc1, 8 i + 3 Mlp.drop
 *               behind fc2, 8 i + 4 drop-path of the MLP branch; 8 * depth: pos_drop.
 *   step        a 32-bit counter in DEVICE memory beside the seed: state = uint32 {seed lo, seed hi, step, unused}.  maest_rng_advance
 *               copies the state into `snapshot` (uint32 [4], same layout) and then adds 1 to the step, in one launch on `stream`: a
 *               forward calls it once, its kernels and the backward of that forward read the snapshot POINTER, never a host value --
 *               so a captured training graph draws fresh masks at every replay.
 * Every kernel takes the row -> (b, t) mapping as arguments: a buffer of B * n_rows_per_clip rows holds tokens 0 .. n_rows_per_clip - 1
 * of every clip of N tokens (n_rows_per_clip = N: dense; = 2: the last block's head-token rows). */
int maest_rng_advance(uint32_t* state, uint32_t* snapshot, void* stream);
/* In place: x[r, c] *= keep * scale, and the same for `aux` (same shape and dtype, or NULL): the Mlp site passes gelu(fc1) and the saved
 * gelu'(fc1), so that the MAEST_EPI_MUL dgrad yields the gradient through both; fp32 [B, N, 768]: pos_drop forward, and its backward on
 * the gradient.  dtype MAEST_F32 / MAEST_BF16; C a multiple of 8. */
int maest_dropout(void* x, void* aux, int dtype, int B, int N, int n_rows_per_clip, int C, uint32_t thr, float scale, int site,
                  const uint32_t* snapshot, void* stream);
/* maest_add_layernorm_fwd with the branch multiplier:
 *   x_out = x + (delta * keep_e(b, t, c) * scale_e) * keep_p(b) * scale_p ; y = LN(x_out)        rows = B * n_rows_per_clip
 * site_e < 0 switches the element part off, site_p < 0 the path part (not both).  y_dtype MAEST_F32 / MAEST_BF16. */
int maest_drop_add_layernorm_fwd(const float* x, const void* delta, int delta_dtype, float* x_out, const float* gamma,
                                 const float* beta, void* y, int y_dtype, float* mean, float* rstd, int B, int N,
                                 int n_rows_per_clip, int cols, float eps, int site_e, uint32_t thr_e, float scale_e, int site_p,
                                 uint32_t thr_p, float scale_p, const uint32_t* snapshot, void* stream);
/* The same without the LayerNorm (the last block's fc2 branch, the head-token tail, a truncated forward). */
int maest_drop_add(const float* x, const void* delta, int delta_dtype, float* x_out, int B, int N, int n_rows_per_clip, int cols,
                   int site_e, uint32_t thr_e, float scale_e, int site_p, uint32_t thr_p, float scale_p, const uint32_t* snapshot,
                   void* stream);
/* dst = cast((src * keep_e * scale_e) * keep_p * scale_p): the gradient ENTERING a regularised branch (operand of its wgrad / dgrad
 * GEMMs); the residual stream's fp32 gradient `src` passes unmodified, so dst must not alias it (MAEST_F32 dst: a separate buffer). */
int maest_drop_cast(const float* src, void* dst, int dst_dtype, int B, int N, int n_rows_per_clip, int cols, int site_e,
                    uint32_t thr_e, float scale_e, int site_p, uint32_t thr_p, float scale_p, const uint32_t* snapshot, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAEST_HIP_H */
