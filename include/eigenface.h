/*
 * eigenface.h — C ABI of libeigenface.so, the MI355X (gfx950) eigenfaces engine.
 *
 * The reference (saladbkp/face-detection-recognization-PCA) has no FFI: its hot
 * path is Python calling NumPy/LAPACK and scikit-learn.  Each entry point below
 * replaces one of those call sites; the Python host layer
 * (face-detection-recognization-pca_amd/eigenface) binds them with ctypes and
 * keeps the reference's Python surface (INTEGRATION.md shows the bindings).
 *
 * Conventions
 *   - Every function returns EF_OK (0) or a negative EF_E_* code; the message is
 *     available from ef_last_error(ctx) until the next call on that ctx.
 *   - Sizes are int64_t, matrices are row-major and dense (leading dimension =
 *     row length) unless stated otherwise.
 *   - Pointer arguments are HOST pointers unless EF_MEM_DEVICE is set in
 *     `flags`, in which case they are device pointers on the ctx's device
 *     (e.g. torch-ROCm data_ptr()).  Host-pointer calls are synchronous on
 *     return; device-pointer calls are stream-ordered on the ctx's stream and
 *     return without synchronising.
 *   - A ctx is not thread-safe.  One process per GPU.
 */
#ifndef EIGENFACE_H_
#define EIGENFACE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EF_API_VERSION 7

/* status codes */
#define EF_OK 0
#define EF_E_INVALID (-1) /* bad argument / unsupported shape            */
#define EF_E_HIP (-2)     /* HIP runtime error                           */
#define EF_E_STATE (-3)   /* call out of order (no model / no gallery)   */
#define EF_E_NOMEM (-4)   /* device allocation failed                    */
#define EF_E_NUMERIC (-5) /* eigensolver did not converge / non-finite   */

/* element types */
#define EF_U8 0
#define EF_F32 1
#define EF_F64 2

/* similarity metrics (ef_search) */
#define EF_METRIC_L2 0     /* argmin ||q-g||^2, lowest index on ties (north star)           */
#define EF_METRIC_COSINE 1 /* argmax q.g/(|q||g|), first max wins (scan-template-v4.py:274-275) */

/* flags */
#define EF_FIT_STANDARDIZE 0x1u /* StandardScaler before PCA (train-v4.py:131)                */
#define EF_MODEL_BF16 0x2u      /* ef_model_set: project on bf16 MFMA (config 5), fp32 features */
#define EF_MEM_DEVICE 0x100u    /* pointer args are device pointers, call is asynchronous    */
#define EF_IMG_RGB 0x200u       /* ef_preprocess: 3/4-channel pixels are RGB(A), not BGR(A)  */
#define EF_ROI_RECTS_DEVICE 0x400u /* ef_preprocess_rois: rects is a device pointer          */
#define EF_BANK_GATE_RELATIVE 0x800u /* gated bank calls: gate[m] bounds eps2 / E, not eps2     */

/* kernels whose device time can be queried with ef_timing_get */
#define EF_KERNEL_SEARCH 0  /* distance GEMM + fused arg-best   */
#define EF_KERNEL_PROJECT 1 /* (p - mean).W projection GEMM     */
#define EF_KERNEL_TMATCH 2  /* template localiser, one frame    */
#define EF_KERNEL_INGEST 3  /* grey + resize of one image batch */
#define EF_KERNEL_HAAR 4    /* Haar cascade detection, one frame (GPU part) */
#define EF_KERNEL_JPEG 5    /* JPEG entropy decode + IDCT + colour, one batch */
#define EF_KERNEL_SYRK 6    /* the fit's int8 covariance/Gram SYRK, all passes of one fit */
#define EF_KERNEL_JPEG_HOST 7 /* host staging of one ef_jpeg_ingest part (marker parse, destuff, tables):
                                wall time on the host, not a device kernel (API v7) */
#define EF_KERNEL_SCAN 8    /* everything one ef_scan_frame queues: grey, localiser, selection, ROI rows, bank.
                                The bank's launches inside it also count under EF_KERNEL_PROJECT and
                                EF_KERNEL_SEARCH (one launch each per frame, as in ef_bank_recognize), and their
                                two event pairs are recorded inside the scan's span; EF_KERNEL_TMATCH and
                                EF_KERNEL_INGEST do not count scans */
#define EF_KERNEL_RECON 9   /* back-projection GEMM of ef_reconstruct / ef_face_distance with its epilogue; the
                               bank's grouped residual GEMM (ef_bank_face_distance and the gated calls) too */
#define EF_KERNEL_RECON_REDUCE 10 /* ef_face_distance: the fixed-order sum of the pixel splits' partials; the
                                     bank's grouped reduce too */
/* 11: EF_KERNEL_HAAR_SCAN, defined with ef_haar_scan_frame below */

/* No-result sentinel in a key array (empty gallery). */
#define EF_KEY_NONE INT64_MAX

typedef struct ef_ctx ef_ctx;

/* ---------------------------------------------------------------- context */
int ef_api_version(void);
int ef_device_count(int* out);
int ef_create(int device, ef_ctx** out);
void ef_destroy(ef_ctx* ctx);
const char* ef_last_error(const ef_ctx* ctx);
/* Launch on an external hipStream_t, e.g. torch.cuda.current_stream().cuda_stream;
 * NULL means the default (null) stream.  ef_use_own_stream restores the ctx's own
 * non-blocking stream (the default after ef_create). */
int ef_set_stream(ef_ctx* ctx, void* hip_stream);
int ef_use_own_stream(ef_ctx* ctx);
/* The hipStream_t the ctx launches on now (*out; NULL = the default stream): lets a caller
 * order its own stream after an asynchronous EF_MEM_DEVICE call (hipStreamWaitEvent, or
 * torch.cuda.ExternalStream + wait_stream). */
int ef_get_stream(const ef_ctx* ctx, void** out);
int ef_synchronize(ef_ctx* ctx);
/* ef_fit keeps its device workspaces (operand copies, covariance, subspace blocks) in
 * the context between calls, so repeated fits do not pay hipMalloc/hipFree; ef_trim
 * frees them (ef_destroy does too). */
int ef_trim(ef_ctx* ctx);

/* -------------------------------------------------------------------- fit
 * Replaces manual_pca (useless/train.py:56-128) and, with EF_FIT_STANDARDIZE,
 * StandardScaler.fit_transform + PCA(svd_solver='full').fit_transform
 * (train-v4.py:126-146).  X is n x d uint8 pixels (train-v4.py:68,73).
 * Computes mean -> centre(+scale) -> covariance (Gram A.A^T/(n-1) when n<d,
 * A^T.A/(n-1) otherwise) -> symmetric eigensolve -> back-project -> unit
 * eigenfaces with the sklearn svd_flip sign rule -> training projection.
 * k is clamped to min(n, d) as manual_pca does (useless/train.py:114).
 * Outputs (host or device, all float64; NULL skips an optional output):
 *   mean_out[d]        column mean of X (train-v4.py:127, useless/train.py:70)
 *   var_out[d]         population variance (StandardScaler.var_)        optional
 *   scale_out[d]       StandardScaler.scale_ (1 for constant pixels)     optional
 *   components_out[k*d] eigenfaces as rows (pca.components_; manual_pca's
 *                      eigenfaces matrix is its transpose)
 *   eigvals_out[k]     covariance eigenvalues, descending (explained_variance_)
 *   proj_out[n*k]      training projection (projected_data / face_features) optional
 *   total_var_out[1]   trace of the covariance                         optional
 *   k_out[1]           number of components actually produced          optional
 *   iters_out[1]       eigensolver iterations (0 = direct Jacobi)       optional
 */
int ef_fit(ef_ctx* ctx, const uint8_t* X, int64_t n, int64_t d, int32_t k, uint32_t flags,
           double* mean_out, double* var_out, double* scale_out, double* components_out,
           double* eigvals_out, double* proj_out, double* total_var_out, int32_t* k_out,
           int32_t* iters_out);
/* ef_fit for any element type: x_dtype EF_U8 (= ef_fit), EF_F32 or EF_F64 — manual_pca's
 * float64 faces (useless/train.py:40, :56-128) and ManualPCA.fit on standardised,
 * non-integral data (scripts/manual/train-v2.py:16-42, fed by ManualStandardScaler :53-72).
 * Float input: fp64 two-pass column statistics, covariance / Gram, back-projection and
 * training projection on the fp64 MFMA GEMM with centring (and 1/scale) in the operand
 * loads; uint8 input keeps the exact integer kernels. */
int ef_fit_ex(ef_ctx* ctx, const void* X, int32_t x_dtype, int64_t n, int64_t d, int32_t k, uint32_t flags,
              double* mean_out, double* var_out, double* scale_out, double* components_out,
              double* eigvals_out, double* proj_out, double* total_var_out, int32_t* k_out,
              int32_t* iters_out);
/* Column mean and population variance of X (n x d, EF_U8 / EF_F32 / EF_F64), float64 out:
 * ManualStandardScaler.fit (np.mean / np.std, scripts/manual/train-v2.py:58-64) and
 * StandardScaler.fit's statistics (train-v4.py:131).  uint8: exact integer sums; float:
 * two passes in fp64 (sum, then sum of (x - mean) and (x - mean)^2, sklearn's
 * _incremental_mean_and_var form).  var_out may be NULL. */
int ef_colstats(ef_ctx* ctx, const void* X, int32_t x_dtype, int64_t n, int64_t d, uint32_t flags,
                double* mean_out, double* var_out);
/* The fit's CholQR factor alone (API v7): Li = L^-1 (row-major, zeros above the diagonal)
 * for G = L L^T, 1 <= m <= 256, G row-major with row stride ldg >= m; host pointers.  A
 * pivot <= tol_rel * max diag(G) sets *info = -(column + 1) and leaves Li as given;
 * *info = 0 on success. */
int ef_chol_inv(ef_ctx* ctx, const double* G, int32_t m, int64_t ldg, double tol_rel, double* Li, int32_t* info);

/* ---------------------------------------------------- sample-sharded fit (API v6)
 * The fit collective of SURVEY §8(e): rank r holds uint8 rows X_r (n_r x d) on its GPU.
 * ef_fit_shard_stats: the exact integer pieces of the local rows —
 *   sum_out[d] = sum x, sumsq_out[d] = sum x^2 (uint64) per pixel,
 *   cross_out[d*d] (int64) = X'_r^T X'_r with X' = X - 128 (the upper 64 x 64 blocks exact,
 *   the rest of the matrix unspecified);
 * the caller sums the three arrays over ranks (an all-reduce, integer sum — e.g. RCCL
 * int64 over xGMI), then every rank calls
 * ef_fit_from_stats with the sums and n_total = sum n_r: mean / var / scale / components /
 *   eigenvalues / total variance exactly as ef_fit computes them on the concatenated rows
 *   (the same integers give the same covariance, bit for bit), covariance path only
 *   (n_total >= d; EF_FIT_STANDARDIZE as in ef_fit);
 * ef_fit_transform: the training projection (projected_data / fit_transform output) of
 *   local rows with a fitted model (mean[d], scale[d] or NULL = no StandardScaler,
 *   comps[k*d]) — the rows ef_fit's proj_out would hold for them.
 * Host pointers unless EF_MEM_DEVICE (then every array argument is a device pointer). */
int ef_fit_shard_stats(ef_ctx* ctx, const uint8_t* X, int64_t n, int64_t d, uint64_t* sum_out, uint64_t* sumsq_out,
                       int64_t* cross_out, uint32_t flags);
int ef_fit_from_stats(ef_ctx* ctx, const uint64_t* sum, const uint64_t* sumsq, const int64_t* cross, int64_t n_total,
                      int64_t d, int32_t k, uint32_t flags, double* mean_out, double* var_out, double* scale_out,
                      double* components_out, double* eigvals_out, double* total_var_out, int32_t* k_out,
                      int32_t* iters_out);
int ef_fit_transform(ef_ctx* ctx, const uint8_t* X, int64_t n, int64_t d, const double* mean, const double* scale,
                     const double* components, int32_t k, uint32_t flags, double* proj_out);

/* --------------------------------------------------------------- projection
 * Recognition model f = (p - mean) . W  (useless/scan.py:93-96; sklearn
 * scaler.transform + pca.transform folded, scan-template-v4.py:265-266).
 * mean[d], W[d*k] float32, row-major (d rows of k), 1 <= k <= 65536 (k > 512 is padded
 * to a multiple of 128: the full-rank per-person models of train-v5.py:539-545).  Kept
 * resident.
 * EF_MODEL_BF16: f = (p - round(mean)).bf16(W) - (mean - round(mean)).W with
 * fp32 accumulation (exact bf16 inputs for uint8 pixels; only W is rounded). */
int ef_model_set(ef_ctx* ctx, const float* mean, const float* W, int64_t d, int32_t k, uint32_t flags);
/* P[b*d] pixels (EF_U8 or EF_F32) -> F[b*k] float32. */
int ef_project(ef_ctx* ctx, const void* P, int32_t p_dtype, int64_t b, float* F, uint32_t flags);

/* ----------------------------------------------- reconstruction, distance from face space
 * The way back out of face space, for the resident model (mean, W):
 *   x^   = mean + f . R                        reconstruction, b x d
 *   eps2 = sum_j (s_j (p_j - x^_j))^2          squared distance from face space, per probe
 *   E    = sum_j (s_j (p_j - mean_j))^2        total energy, per probe
 * sklearn's scaler.inverse_transform(pca.inverse_transform(f)) and Turk-Pentland's face / non-face
 * measure.  R[k*d] float32 row-major (k rows of d), weight[d] float32 or NULL (= 1).  manual_pca
 * models: R = eigenfaces^T, no weight.  Standardised models (W = diag(1/sigma) V^T): R = V diag(sigma),
 * weight = 1/sigma, so the residual is measured in the scaler's space, where the components are
 * orthonormal.  eps2 is summed from the residual itself, never as E - |f|^2.
 * Added after API v7 without a version bump: probe by symbol.
 * ef_recon_set: EF_E_STATE without a model, EF_E_INVALID when d or k differ from the model's; a
 *   failed call leaves no reconstruction state and the model untouched.  ef_model_set drops the
 *   reconstruction state.  Synchronous on return.
 * ef_reconstruct: F[b*k] float32 -> out[b*d] as EF_F32, or EF_U8 (clamped to [0, 255], then
 *   rounded half to even: np.rint, OpenCV's saturate_cast<uchar>).
 * ef_face_distance: P[b*d] pixels (EF_U8 or EF_F32) -> dffs2[b] = eps2 and, each optional,
 *   energy[b] = E and F_out[b*k], the features exactly as ef_project returns them.  Projection,
 *   its reduce and the residual are queued on the ctx's stream with nothing downloaded in
 *   between; x^ is never written.  Works with the fp32 and the EF_MODEL_BF16 model (the
 *   back-projection is fp32 either way).  The same inputs give the same bits on every call.
 * Both: EF_E_STATE without reconstruction state; b = 0 is EF_OK. */
int ef_recon_set(ef_ctx* ctx, const float* R, const float* weight, int64_t d, int32_t k, uint32_t flags);
int ef_reconstruct(ef_ctx* ctx, const float* F, int64_t b, int32_t out_dtype, void* out, uint32_t flags);
int ef_face_distance(ef_ctx* ctx, const void* P, int32_t p_dtype, int64_t b, float* dffs2, float* energy,
                     float* F_out, uint32_t flags);

/* ------------------------------------------------------------------ search
 * Gallery rows G[n*k] float32 (face_features / projected_data), kept resident; any
 * 1 <= k <= 65536 (as ef_model_set).
 * global_offset is added to every returned index (row sharding across ranks). */
int ef_gallery_set(ef_ctx* ctx, const float* G, int64_t n, int32_t k, int64_t global_offset,
                   uint32_t flags);
/* Q[b*k] float32 probe features -> keys[b].  A key packs the exact fp32 score
 * of the winning row in its high 32 bits (order-preserving) and the global
 * row index in its low 32 bits, so min over keys == argbest with lowest-index
 * tie-break; an all-reduce(MIN) over ranks combines sharded galleries.
 *
 * Input domain of the arg-best guarantee (ef_search, ef_search_matches, ef_search_topk*,
 * ef_search_labelled*, ef_recognize* on the context's gallery; not the model bank, whose slots
 * keep the domain "fp32 squares neither overflow nor underflow"): ANY finite fp32 values.  The
 * returned row is the lowest index among the rows whose fp64 score is within
 * 1e-12 * (|min| + scale) of the fp64 minimum, whatever the features' scale, offset or spread
 * of norms.  The fp32 / bf16 scan decides a probe only where its error bound holds: fp32
 * max |g|^2 in [2^-80, 2^126] together with 2.02 |q| max|g|, for cosine also |q|^2 >= 2^-80
 * and no non-zero row with |g|^2 < 2^-80.  Outside it the probe is re-scored against every
 * row in fp64: exact, at the cost of b * n fp64 row products.  scale takes max |g|^2 over the
 * rows whose fp32 |g|^2 is finite, so where squares overflow the window is narrower than
 * stated, never wider.
 * NaN and +-inf: a gallery row with such a component is never returned (unless the probe has
 * none to prefer: then EF_KEY_NONE), does not enter scale, and sends every probe of that
 * gallery to the fp64 re-scoring; the other rows rank as if it were absent.  A probe with such
 * a component gets EF_KEY_NONE (all m slots of a top-m search; the record {+inf, 0,
 * EF_KEY_NONE}) on every call and route, and does not affect the other probes of its batch. */
int ef_search(ef_ctx* ctx, const float* Q, int64_t b, int32_t metric, int64_t* keys, uint32_t flags);
/* Fused pipeline: project P then search; feats (b*k float32) optional. */
int ef_recognize(ef_ctx* ctx, const void* P, int32_t p_dtype, int64_t b, int32_t metric,
                 int64_t* keys, float* feats, uint32_t flags);
/* Host-side key decoding: L2 -> squared distance, COSINE -> similarity;
 * EF_KEY_NONE -> idx -1, best NaN. */
void ef_keys_decode(const int64_t* keys, int64_t b, int32_t metric, float* best, int64_t* idx);
/* Host-side introspection (no ctx, no GPU): the launches a search of b probes of k features
 * over an n-row gallery makes.  A batch whose padded probe block would pass 2 GiB (k > 512)
 * is searched in pieces of whole 256-probe tiles.  *n_pieces = the piece count; for the
 * first max_pieces pieces, pieces_out[6*i ..] = {first probe, probes, padded rows the
 * piece is launched with, probe tiles of its plan, gallery chunks, row tiles per chunk}.
 * split_bf16 as EF_OPT_SEARCH_SPLIT_BF16.  (API v6) */
int ef_search_schedule(int64_t b, int32_t k, int64_t n, int32_t split_bf16, int64_t* pieces_out, int32_t max_pieces,
                       int32_t* n_pieces);

/* ------------------------------------------------ exact cross-shard arg-best
 * A key's fp32 score cannot order two shards' winners whose fp64 scores differ by less
 * than one fp32 ulp, and a MIN over keys would then fall back to the lower index.  The
 * match record of a probe carries the winner's fp64 score, so shards merge exactly:
 *   score  fp64 score of the winning row (L2: squared distance; COSINE: -similarity;
 *          +inf with key == EF_KEY_NONE for an empty shard)
 *   scale  tie-tolerance scale (L2: |q|^2 + max |g|^2 of the shard; COSINE: 1)
 *   key    the packed key of ef_search (global row index in the low 32 bits)
 * Merging picks, per probe, the lowest global index among the parts whose score is within
 * 1e-12 * (|min score| + max scale) of the minimum — the rule a single engine applies to
 * its fp32-ambiguous candidates (np.argmin / np.argmax first-index semantics,
 * scan-template-v4.py:274-275). */
typedef struct ef_match {
  double score;
  double scale;
  int64_t key;
} ef_match;
int ef_search_matches(ef_ctx* ctx, const float* Q, int64_t b, int32_t metric, ef_match* out, uint32_t flags);
int ef_recognize_matches(ef_ctx* ctx, const void* P, int32_t p_dtype, int64_t b, int32_t metric, ef_match* out,
                         float* feats, uint32_t flags);
/* parts: nparts x b records (part-major) -> keys_out[b] (and merged records in merged_out,
 * optional).  Host pointers: computed on the host, ctx may be NULL (usable without a GPU).
 * EF_MEM_DEVICE: device pointers, stream-ordered on ctx's stream. */
int ef_matches_merge(ef_ctx* ctx, const ef_match* parts, int32_t nparts, int64_t b, int64_t* keys_out,
                     ef_match* merged_out, uint32_t flags);

/* ------------------------------------------------------ top-m search (ranked list)
 * The m best gallery rows per probe, 1 <= m <= 64, best first, with the guarantees of
 * ef_search: fp64-exact order, first-index ties, no score matrix in memory.  Per probe the
 * result is m slots (keys[b][m], probe-major):
 *   - rank 0 is exactly what ef_search returns for that probe: the lowest index among the
 *     rows whose fp64 score is within 1e-12 * (|min| + scale) of the minimum;
 *   - ranks 1 .. m-1 are the remaining rows in pure (fp64 score, row index) lexicographic
 *     order; the fp64 score is the one the key is built from, deterministic per (probe, row);
 *   - rows are distinct, so exact duplicates come out in ascending index;
 *   - scores are non-decreasing from rank 1 on; rank 0 may exceed rank 1 by at most the
 *     tie window;
 *   - when fewer than m rows exist (an empty gallery included) the trailing slots are
 *     EF_KEY_NONE, as records {+inf, 0, EF_KEY_NONE};
 *   - a key is pack((float)fp64 score, global row), as for ef_search.
 * The scan arithmetic follows EF_OPT_SEARCH_SPLIT_BF16 (3, the single-bf16 screen, counts
 * as 1 here); the prefix scan never engages.  EF_E_INVALID for m outside 1 .. 64 or
 * EF_OPT_SEARCH_TOPK_CAND below m.  With a communicator of more than one rank attached the
 * three search calls return EF_E_STATE: search each shard on its own context
 * (ef_search_topk_matches) and merge the records with ef_matches_merge_topk.  (API v7) */
int ef_search_topk(ef_ctx* ctx, const float* Q, int64_t b, int32_t m, int32_t metric, int64_t* keys /* [b][m] */,
                   uint32_t flags);
int ef_recognize_topk(ef_ctx* ctx, const void* P, int32_t p_dtype, int64_t b, int32_t m, int32_t metric,
                      int64_t* keys /* [b][m] */, float* feats, uint32_t flags);
int ef_search_topk_matches(ef_ctx* ctx, const float* Q, int64_t b, int32_t m, int32_t metric,
                           ef_match* out /* [b][m] */, uint32_t flags);
/* parts: nparts x b x m records (part-major) -> keys_out[b][m] (and merged_out[b][m],
 * optional), by the rule above applied to a probe's nparts * m records: rank 0 is the lowest
 * global index among the records within 1e-12 * (|min| + max scale) of the minimum
 * (ef_matches_merge's rule), the rest follow in (score, global index) order; EF_KEY_NONE
 * records are skipped and missing ranks padded.  The result equals the single-engine one
 * unless more than m rows sit inside the best row's tie window (a shard then reports only m
 * of them).  Host pointers: computed on the host, ctx may be NULL; EF_MEM_DEVICE: device
 * pointers, stream-ordered on ctx's stream. */
int ef_matches_merge_topk(ef_ctx* ctx, const ef_match* parts, int32_t nparts, int64_t b, int32_t m,
                          int64_t* keys_out, ef_match* merged_out, uint32_t flags);
/* Counters of the most recent top-m search on this context: {probes, probes whose first
 * candidate list overflowed EF_OPT_SEARCH_TOPK_CAND, probes resolved by the full fp64 sweep,
 * candidate rows re-scored in fp64}.  Synchronises the context's stream. */
int ef_search_topk_stats(ef_ctx* ctx, int64_t out[4]);

/* ------------------------------------------------- labelled search (leave-one-out)
 * Added by symbol (EF_API_VERSION stays 7).  The nearest row of the probe's own identity (the
 * genuine match) and the nearest row of any other identity (the impostor), with the probe's own
 * gallery row left out: what a leave-one-out recognition rate and a threshold derived from a
 * labelled gallery need.  The rows are masked inside the scan, so the answers carry ef_search's
 * guarantee whatever the number of same-label rows in front of the nearest other-label one.
 *
 * ef_gallery_labels: one int32 label per resident gallery row (any value is an ordinary label),
 *   copied to the device from host memory, or from device memory with EF_MEM_DEVICE.  EF_E_STATE
 *   without a gallery; EF_E_INVALID when n differs from the resident row count; labels == NULL
 *   drops the labels (n is not read); ef_gallery_set drops them, because the rows changed.  A
 *   failed call leaves the previous labels in place.
 * ef_search_labelled: Q[b*k] probe features -> keys[b] and / or matches[b] (at least one).  The
 *   result for probe p is exactly what ef_search / ef_search_matches would return on the
 *   sub-gallery of qualifying rows, the rows keeping their indices.  A row qualifies when its
 *   label stands in `relation` to probe_labels[p] and its global index (local row +
 *   global_offset, the index a key carries) is not exclude_rows[p]; a negative exclude_rows
 *   entry, or one outside this shard, excludes nothing, and so does exclude_rows == NULL.  The
 *   answer is the lowest qualifying row among those whose fp64 score is within
 *   1e-12 * (|min| + scale) of the qualifying minimum, with ef_search's own scale: |q|^2 +
 *   max |g|^2 of the WHOLE resident gallery for L2, 1 for cosine (the scan's error bound keeps
 *   using the whole gallery's maximum as well: it remains an upper bound).  So with
 *   EF_LABEL_OTHER and a probe label no row carries, or EF_LABEL_ANY without exclusion, keys and
 *   records equal ef_search's bit for bit.  A probe with no qualifying row gets EF_KEY_NONE and
 *   the record {+inf, 0, EF_KEY_NONE}, as an empty gallery gives.  The records merge across
 *   shards with ef_matches_merge unchanged (pass global exclude_rows to every shard).
 *   The call always runs the fp32 scan: EF_OPT_SEARCH_SPLIT_BF16 and EF_OPT_SEARCH_PREFIX are
 *   ignored here, as the prefix scan is by the top-m search.  Every k of ef_search is supported.
 *   Memory: ef_search's workspace plus O(b); no score matrix is written.
 *   With EF_MEM_DEVICE every pointer is a device pointer and the call does not wait.  b = 0 is
 *   EF_OK.  EF_E_STATE: no gallery; SAME or OTHER without gallery labels; a communicator of more
 *   than one rank attached (search each shard on its own context and merge the records).
 *   EF_E_INVALID: SAME or OTHER with probe_labels == NULL; an unknown relation or metric; neither
 *   keys nor matches. */
#define EF_LABEL_SAME  0   /* rows whose label equals the probe's                */
#define EF_LABEL_OTHER 1   /* rows whose label differs from the probe's           */
#define EF_LABEL_ANY   2   /* every row (labels not consulted; only the exclusion) */
int ef_gallery_labels(ef_ctx* ctx, const int32_t* labels /* [n] or NULL */, int64_t n, uint32_t flags);
int ef_search_labelled(ef_ctx* ctx, const float* Q, int64_t b, int32_t metric, int32_t relation,
                       const int32_t* probe_labels /* [b]; may be NULL for ANY */,
                       const int64_t* exclude_rows /* [b] or NULL */,
                       int64_t* keys /* [b] or NULL */, ef_match* matches /* [b] or NULL */, uint32_t flags);

/* ------------------------------------------------- score census (verification evaluation)
 * Added by symbol (EF_API_VERSION stays 7).  Histograms of ALL genuine and ALL impostor pair
 * scores of b probes against the resident labelled gallery: what FMR(t), FNMR(t), TAR at a fixed
 * FMR, the pairwise equal-error rate, AUC and d' are computed from.  A distance GEMM whose
 * epilogue bins each score instead of taking an arg-best: one gallery sweep per 128-probe tile,
 * no b x n array of any kind.
 *
 * What is counted: each (probe p, resident row r) is one pair, unless r's global index (local row
 *   + global_offset) equals exclude_rows[p]; a negative entry, one outside this shard, or
 *   exclude_rows == NULL excludes nothing (ef_search_labelled's rule).  Side 0 (genuine) takes
 *   the pairs with label[r] == probe_labels[p], side 1 (impostor) the rest.  The score is the one
 *   ef_keys_decode shows: squared L2 distance, or cosine similarity, where a zero row or a zero
 *   probe scores 0.
 * counts[side][nbins + 3], overwritten by the call (nothing accumulates across calls), with
 *   w = (hi - lo) / nbins:
 *     [0]          scores below lo
 *     [1 + j]      lo + j w <= score < lo + (j + 1) w,  j = 0 .. nbins - 1
 *     [nbins + 1]  scores at or above hi
 *     [nbins + 2]  pairs whose scan score is not finite (a NaN or +-inf component in the row or
 *                  in the probe); such a pair is counted in no other slot.
 * Guarantee: every qualifying pair is counted exactly once; all accumulation is in integers, so
 *   the counts are the same on every run.  Inside the scan's domain (as for ef_search: fp32
 *   max |g|^2 in [2^-80, 2^126] together with 2.02 |q| max|g|, for cosine also |q|^2 >= 2^-80 and
 *   no non-zero row with |g|^2 < 2^-80) a pair lands in the bin of its fp64 score, or in a
 *   neighbouring bin when that score lies within delta of an edge: for every edge
 *   e_j = lo + j w, the number of pairs binned below e_j lies between the fp64 counts of
 *   score < e_j - delta and of score < e_j + delta.  With u = 2^-24, kp the padded k
 *   (16, 32, 64, 128, 256, 512, then multiples of 128), |q| and |g| Euclidean norms and the
 *   maxima taken over the call's probes, the gallery's rows and the pairs' scores s:
 *     L2      delta = 2 [(kp + 4) u 1.01 (2 max|q| max|g| + max|g|^2) + 4 u max|s|]
 *                     + 8 u max(|lo|, |hi|)
 *     cosine  delta = 2 (kp + 12) u 1.01 + 8 u max(|lo|, |hi|)
 *   derived from the kernel's arithmetic: a chain of kp fp32 fused multiply-adds
 *   from the row's fp32 -|g|^2 / 2 (L2), |q|^2 and 1/|q| rounded once from fp64, the row's fp32
 *   1/|g|, one rounding for the score; the last term is the bin index, floor((s - lo) nbins /
 *   (hi - lo)) in fp32.  lo, hi and the scores are fp32: scores that are integers below 2^23, with
 *   lo = -0.5 and hi - lo = nbins, are binned exactly.
 *   Outside the domain every pair is still counted once, in a bin that need not be its own; a row
 *   with finite components whose squares overflow fp32 scores 0 under cosine.
 * Arguments: 1 <= nbins <= 2048; lo < hi, both finite; probe_labels and counts non-NULL; b = 0
 *   (or an empty gallery) is EF_OK with all zeros.  EF_E_STATE: no gallery; no gallery labels; a
 *   communicator of more than one rank attached (run each shard on its own context and add the
 *   counts: they are additive across shards given global exclude_rows).  EF_E_INVALID for every
 *   other bad argument.  With EF_MEM_DEVICE every pointer is a device pointer and the call does
 *   not wait.  Every k of ef_search is supported.  Memory: O(b) + O(nbins) beside the padded
 *   probes. */
#define EF_CENSUS_MAX_BINS 2048
int ef_score_census(ef_ctx* ctx, const float* Q, int64_t b, int32_t metric,
                    const int32_t* probe_labels /* [b] */,
                    const int64_t* exclude_rows /* [b] or NULL */,
                    float lo, float hi, int32_t nbins,
                    int64_t* counts /* [2][nbins + 3] */, uint32_t flags);

/* ------------------------------------------------- gallery clustering (labels for unlabelled rows)
 * Added by symbol (EF_API_VERSION stays 7).  Groups the rows of the resident gallery by identity
 * without labels: a self-join that links every pair of rows within a threshold and returns the
 * connected components.  It produces what ef_gallery_labels, ef_score_census and ef_lda_* take,
 * and the list of near-duplicate rows.  The distance GEMM is the census's; its epilogue joins the
 * linked pairs in a bounded lock-free union-find instead of binning scores.  No n x n array of any
 * kind is written.
 *
 * Linked: rows i != j with fp64 squared distance <= threshold (L2), or fp64 cosine similarity
 *   >= threshold (cosine; a zero row scores 0 against everything), both computed from the fp32
 *   features as stored, as ef_keys_decode shows them.  A pair whose fp32 scan score is not finite
 *   (a NaN or +-inf component in either row, fp32 squares that overflow under L2) is never linked:
 *   such rows are clusters of their own, or noise under a density floor.
 * Guarantee: inside the scan's domain (ef_score_census's: fp32 max |g|^2 in [2^-80, 2^126 / 3.02],
 *   for cosine also no non-zero row with |g|^2 < 2^-80 and no row with a non-finite norm) every
 *   edge is decided as in fp64.  The fp32 scan score s^ decides alone when |s^ - threshold| >
 *   delta; a pair inside the band is re-scored in fp64 by a whole wave and decided on that.  With
 *   u = 2^-24 and kp the padded k, delta is ef_score_census's bound without its bin-index term,
 *   taken per call at |q|, |g| <= max|g| and |s| <= 4 max|g|^2, plus the rounding of the threshold
 *   to fp32:
 *     L2      delta = 2 [(kp + 4) u 1.01 (3 max|g|^2) + 16 u max|g|^2] + |fp32(t) - t|
 *     cosine  delta = 2 (kp + 12) u 1.01 + |fp32(t) - t|
 *   Outside the domain delta is +inf: every pair with a finite scan score is decided in fp64
 *   (correct, and slow).  The components of an exactly decided graph do not depend on the order in
 *   which its edges arrive, and every count is an integer: the same input gives the same outputs
 *   on every run.
 * min_samples (DBSCAN's density floor): <= 1 gives plain connected components.  Otherwise a row is
 *   core when degree + 1 >= min_samples; only core-core pairs are joined; a non-core row linked
 *   to a core row takes the cluster of its lowest-index linked core row; a non-core row linked to
 *   none is noise.
 * Outputs (rows are local rows of this context's shard):
 *   labels[n]  the cluster of each row, clusters numbered 0 .. by their lowest member row (under
 *              a density floor: by their lowest core row); -1 for noise.
 *   degree[n]  optional (NULL): the number of other rows linked to each row.
 *   info[4]    {clusters, noise rows, linked unordered pairs, pairs settled in fp64}, all exact.
 * Termination: every union-find walk is cut at n links and every union at 2 n + 2 attempts;
 *   nothing waits for another workgroup.  A walk that reached its bound (never seen: the forest is
 *   acyclic by construction) makes a host call return EF_E_NUMERIC after its synchronisation;
 *   with EF_MEM_DEVICE it sets the bit EF_CLUSTER_UNCONVERGED of info[3].
 * n = 0 is EF_OK with info all zero.  EF_E_STATE: no gallery; a communicator of more than one rank
 *   attached.  EF_E_INVALID: a NaN threshold, an unknown metric, labels or info NULL, more than
 *   2^31 - 129 rows.  With EF_MEM_DEVICE every pointer is a device pointer and the call does not
 *   wait (and reads nothing back to size anything).  Every k of ef_search is supported.  Memory:
 *   O(n) (six 4-byte values per row).  ef_timing_get: EF_KERNEL_CLUSTER.
 *
 * ef_cluster_schedule: the link pass's work items for n rows of padded length kp, on the host (no
 *   context, no device): n_items triples {first row tile, end row tile, probe tile} of 128-row
 *   tiles, of which up to max_items are written.  Every unordered tile pair (row tile <= probe
 *   tile) belongs to exactly one item.  EF_E_INVALID for n < 0 or kp not a positive multiple of 16. */
#define EF_KERNEL_CLUSTER 12 /* everything one ef_gallery_cluster queues */
#define EF_CLUSTER_UNCONVERGED ((int64_t)1 << 62)
int ef_gallery_cluster(ef_ctx* ctx, int32_t metric, double threshold, int32_t min_samples,
                       int32_t* labels /* [n] */, int32_t* degree /* [n] or NULL */,
                       int64_t* info /* [4] */, uint32_t flags);
int ef_cluster_schedule(int64_t n, int32_t kp, int64_t* items_out /* [max_items][3] */, int32_t max_items,
                        int32_t* n_items);

/* ------------------------------------------------- range search (every row within a threshold)
 * Added by symbol (EF_API_VERSION stays 7).  For each probe, ALL rows of the resident gallery
 * within a threshold (scikit-learn's radius_neighbors, faiss's range_search), as a CSR list.  The
 * distance GEMM is the census's over the census's work items; its epilogue decides membership as
 * ef_gallery_cluster decides a link, with a probe in place of the second row.  Two passes of one
 * kernel: the first counts, a scan turns the counts into offsets, the second writes.  No b x n
 * array of any kind is written.
 *
 * A hit: a pair (probe p, resident row r) with fp64 squared distance <= threshold (L2), or fp64
 *   cosine similarity >= threshold (cosine; a zero row or a zero probe scores 0), both computed
 *   from the fp32 features as stored.  Never a hit: a pair whose fp32 scan score is not finite (a
 *   NaN or +-inf component on either side, fp32 squares that overflow under L2); the pair of p
 *   with the row whose global index is exclude_rows[p] (a negative entry, one outside the shard or
 *   a NULL array excludes nothing: ef_score_census's rule).
 * Guarantee: inside the scan's domain (fp32 max |g|^2 in [2^-80, 2^126] together with
 *   2.02 |q| max|g|; for cosine also no non-zero row with |g|^2 < 2^-80, no row with a non-finite
 *   norm, and a probe that is zero or has |q|^2 >= 2^-80) every membership is decided as in fp64.
 *   The fp32 scan score s^ decides alone when |s^ - fp32(t)| > delta_p; a pair inside the band is
 *   re-scored in fp64 by a whole wave and decided on that.  delta_p is taken per probe (a lane of
 *   the kernel owns its probe), from ef_score_census's bound without its bin-index term, with
 *   |s| <= (|q| + max|g|)^2, plus the rounding of the threshold to fp32.  With u = 2^-24, kp the
 *   padded k, |q| the probe's Euclidean norm and max|g| the gallery's largest:
 *     L2      delta_p = 2 [(kp + 4) u 1.01 (2 |q| max|g| + max|g|^2) + 4 u (|q| + max|g|)^2]
 *                       + |fp32(t) - t|
 *     cosine  delta_p = 2 (kp + 12) u 1.01 + |fp32(t) - t|
 *   (the kernel widens it by 0.1 % for its own roundings of |q| and max|g|).  Outside the domain
 *   delta_p is +inf: every pair with a finite scan score is decided in fp64 (correct, and slow).
 * Outputs:
 *   lims[b + 1]  probe p's hits are entries lims[p] .. lims[p + 1] - 1 of rows / scores;
 *                lims[0] = 0 and lims[b] is the exact total.  Always written in full, whatever cap.
 *   rows[cap]    GLOBAL row indices (local row + the gallery's global offset), ascending inside
 *                each segment.
 *   scores[cap]  scores[i] belongs to rows[i]: s^ for a pair the scan decided alone, (float) of
 *                the fp64 score for a pair settled in the band.  Every reported score is within
 *                delta_p of the pair's fp64 score and on the accepting side of fp32(t).
 *   info[4]      {total hits, pairs settled in fp64 (by the counting pass), hits not written for
 *                lack of capacity, 0}, all exact.
 * Capacity: a segment is written only when it fits whole, lims[p + 1] <= cap (these segments are a
 *   prefix of the probes); nothing is ever written at or past rows[cap] / scores[cap].  rows == NULL
 *   or cap == 0 is the count-only form: one pass, only lims and info are written (info[2] is then
 *   the total).  Overflow is no error: compare lims[b] with cap and call again.
 * Determinism: every position is a function of exactly decided memberships and every count is an
 *   integer sum, so the output is byte-identical on every run and between the host and the
 *   EF_MEM_DEVICE form.
 * b = 0 is EF_OK (lims[0] = 0); an empty gallery is EF_OK with lims and info all zero.
 *   EF_E_STATE: no gallery; a communicator of more than one rank attached (search each shard on a
 *   context of its own; the segments of shards in ascending offset order concatenate).
 *   EF_E_INVALID: a NaN threshold, an unknown metric, lims or info NULL, cap < 0, rows without
 *   scores, more than 2^31 - 129 rows.  With EF_MEM_DEVICE every pointer is a device pointer, the
 *   call is stream-ordered and it never waits or reads anything back to size anything.  Every k of
 *   ef_search is supported.  Memory beside the padded probes: O(b chunks) (4 bytes per probe and
 *   gallery chunk; a host call also stages its outputs).  ef_timing_get: EF_KERNEL_RANGE.
 *
 * ef_search_range_plan: the work items of a call with b probes, n rows and padded length kp, on
 *   the host (no context, no device): the gallery's 128-row tiles are cut into n_chunks chunks of
 *   tiles_per_item tiles (the last chunk may be shorter); a work item is one chunk against one tile
 *   of 128 probes (b padded to a multiple of 256).  Both are 0 for b = 0 or n = 0.  EF_E_INVALID for
 *   b < 0, n < 0 or beyond 2^31 - 129, kp not a positive multiple of 16, or a NULL output. */
#define EF_KERNEL_RANGE 13 /* everything one ef_search_range queues */
int ef_search_range(ef_ctx* ctx, const float* Q, int64_t b, int32_t metric, double threshold,
                    const int64_t* exclude_rows /* [b] or NULL */,
                    int64_t* lims /* [b + 1] */,
                    int64_t* rows /* [cap] or NULL */,
                    float* scores /* [cap] or NULL */,
                    int64_t cap, int64_t* info /* [4] */, uint32_t flags);
int ef_search_range_plan(int64_t b, int64_t n, int32_t kp, int64_t* n_chunks, int64_t* tiles_per_item);

/* ------------------------------------------------- identification rank (CMC curves)
 * Added by symbol (EF_API_VERSION stays 7).  For each probe, the number of OTHER identities that
 * come before the probe's own: better[p], the identification rank less one.  A cumulative match
 * characteristic is the distribution of better + 1.  The rank of an identity counts identities,
 * not rows, so no top-m list answers it on a gallery with many rows per person.  The scan is
 * the range search's counting pass with one threshold per probe (the score of the probe's genuine
 * row) and one bit per (probe, identity) in place of the count.  No b x n array is written.
 *
 * Definition, for probe p with label probe_labels[p] on a gallery with labels (ef_gallery_labels):
 *   A row qualifies unless its global index is exclude_rows[p] (ef_search_labelled's rule); a pair
 *   whose fp32 scan score is not finite qualifies for nothing (ef_search_range's rule).
 *   The genuine row is the one ef_search_labelled(.., EF_LABEL_SAME, ..) returns, row_gen its global
 *   index, and tau_p its fp64 score (squared L2 distance, or the negated cosine similarity, as
 *   ef_match.score carries it), recomputed by this call from the stored fp32 features, so that
 *   bit-identical rows score bit-identically.
 *   A qualifying row r with a label other than the probe's BEATS the genuine row when its fp64 score
 *   s(p, r) < tau_p, or s(p, r) == tau_p and its global index is below row_gen (the first-index rule
 *   of the whole search family).
 *   better[p] = the number of distinct labels with at least one beating row; rank = better[p] + 1.
 *   better[p] = -1 when the probe has no genuine row (no qualifying row of its label, a label no
 *   row carries, a NaN or +-inf component in the probe), or when tau_p is not finite (fp32 squares
 *   that overflow under L2): no finite score is comparable with it, in any form of the call.
 * Guarantee: inside the scan's domain (ef_search_range's, evaluated per probe) every "beats" is
 *   decided as in fp64.  The fp32 scan score decides alone when it is further than delta_p from
 *   fp32(tau_p); the pairs inside the band are settled by a whole wave on the fp64 score.  delta_p
 *   is ef_search_range's formula with |fp32(tau_p) - tau_p| as the threshold's rounding term.
 *   Outside the domain delta_p is +inf: every pair with a finite scan score is settled in fp64
 *   (correct, and slow).  All accumulation is a bitwise OR and a popcount: the output is
 *   byte-identical on every run and between the host and the EF_MEM_DEVICE form, and it does not
 *   depend on EF_OPT_RANK_BITMAP_BYTES.
 * Outputs:
 *   better[b]   as defined.
 *   genuine[b]  optional: the records of the labelled SAME scan, unchanged.
 *   info[4]     {pairs settled in fp64 (whatever their label), pieces, distinct labels C, 0}.
 * EF_RANK_GENUINE_GIVEN: genuine[b] is an INPUT, e.g. the records of several shards merged with
 *   ef_matches_merge.  tau_p is recomputed when the record's row lies in this shard, else the
 *   record's score is taken as given; a record with EF_KEY_NONE, or a tau_p that is not finite,
 *   gives -1.  With a gallery sharded by identity (no identity on two shards) every identity is
 *   counted on exactly one shard, so the shards' better[p] add up exactly to the single-gallery
 *   answer (pass global exclude_rows to every shard; a probe is -1 on every shard or on none).
 * The dense class map (label -> 0 .. C - 1) is built on the host by the first call after
 *   ef_gallery_labels (4 n bytes down, sorted, 4 n bytes up) and cached until the labels or the
 *   gallery change: THAT call waits for the stream, even with EF_MEM_DEVICE.  Apart from it, with
 *   EF_MEM_DEVICE every pointer is a device pointer and the call does not wait.
 * Memory beside the labelled scan's workspace: O(b), and the bitmap: ceil(C / 32) words per
 *   probe.  The probes run in pieces of whole 256-probe blocks so that a piece's bitmap stays
 *   within EF_OPT_RANK_BITMAP_BYTES (256 MiB by default; at least one block per piece).
 * b = 0 is EF_OK; an empty gallery is EF_OK with better all -1 and info all zero.
 *   EF_E_STATE: no gallery; no gallery labels; a communicator of more than one rank attached.
 *   EF_E_INVALID: probe_labels, better or info NULL; an unknown metric; EF_RANK_GENUINE_GIVEN
 *   without genuine; more than 2^31 - 129 rows.  Every k of ef_search is supported.
 *   ef_timing_get: EF_KERNEL_RANK.
 *
 * ef_search_rank_plan: the bitmap's shape for b probes, n rows, n_classes labels and a budget, on
 *   the host (no context, no device): words_per_probe = max(1, ceil(n_classes / 32)),
 *   probes_per_piece = 256 max(1, floor(bitmap_bytes / (1024 words_per_probe))), at most b padded
 *   to 256 (and at least 256), n_pieces = ceil(padded b / probes_per_piece), 0 for b = 0 or
 *   n = 0.  EF_E_INVALID for a negative argument or a NULL output. */
#define EF_KERNEL_RANK 14 /* everything one ef_search_rank queues (the labelled scan included) */
#define EF_RANK_GENUINE_GIVEN 0x1000u /* ef_search_rank: genuine[b] is an input */
int ef_search_rank(ef_ctx* ctx, const float* Q, int64_t b, int32_t metric,
                   const int32_t* probe_labels /* [b] */, const int64_t* exclude_rows /* [b] or NULL */,
                   ef_match* genuine /* [b]: out (may be NULL), or in with EF_RANK_GENUINE_GIVEN */,
                   int32_t* better /* [b] */, int64_t* info /* [4] */, uint32_t flags);
int ef_search_rank_plan(int64_t b, int64_t n, int64_t n_classes, int64_t bitmap_bytes,
                        int64_t* words_per_probe, int64_t* probes_per_piece, int64_t* n_pieces);

/* ------------------------------------------------- Fisher discriminant (Fisherfaces)
 * Added by symbol (EF_API_VERSION stays 7).  A linear discriminant inside face space
 * (Belhumeur, Hespanha, Kriegman 1997): from features F[n][k] (EF_F32 / EF_F64; a fit's
 * projection or a gallery) and one label in [0, n_classes) per row, the k x m matrix A whose
 * columns maximise between-identity over within-identity scatter.  A folds into a projection
 * matrix (W' = W . A, same mean), so every call that takes a model runs a Fisher model as is.
 *
 * ef_lda_order: the stable grouping of rows by label on the host (no context, no device):
 *   order[n] lists the rows class by class, each class in input order (np.argsort(labels,
 *   kind="stable")); offsets[n_classes + 1] are the class borders (offsets[c + 1] - offsets[c] =
 *   rows of class c).  n = 0 is EF_OK.  EF_E_INVALID for a label outside [0, n_classes), with
 *   nothing written.  It is the grouping the scatter runs on.
 * ef_lda_scatter: all outputs float64, each optional (NULL):
 *   counts[C]; mean[k] the mean m of all rows; class_means[C][k] (a zero row for an empty class);
 *   Sb[k][k] = sum_c n_c (M_c - m)(M_c - m)^T;  Sw[k][k] = sum_c sum_{i in c} (f_i - M_c)(f_i - M_c)^T.
 *   Any number of classes up to n, empty and one-row classes and unsorted labels included.  Every
 *   sum is taken on rows centred first, in an order fixed by (n, k, labels): the same input
 *   gives the same bytes.  Sw is formed directly from the rows centred on their class means.
 *   Sums and products are carried as unevaluated pairs of doubles (compensated arithmetic), so
 *   each output is the rounding of a result far more accurate than fp64: the discriminant's
 *   error is the scatters' error times cond(Sw).  Sw and Sb are exactly symmetric.
 *   1 <= k <= 1024.
 *   A label outside [0, n_classes) is found on the device before any label is used as an index:
 *   EF_E_INVALID, and the context stays usable.
 * ef_lda_fit: the scatter, then on the device
 *     Sw_g = (1 - g) Sw + g tr(Sw)/k I  (g = shrinkage in [0, 1]),  Sw_g = L L^T,
 *     T = L^-1 Sb L^-T = V diag(lambda) V^T,  A = sqrt(n - C+) L^-T V  (leading m columns),
 *   with C+ the number of non-empty classes.  Conventions:
 *     - evals[m] are the generalised eigenvalues of (Sb, Sw_g), descending;
 *     - A^T (Sw_g / (n - C+)) A = I, so L2 distance in the new space is the within-class
 *       Mahalanobis distance, and A^T Sb A / (n - C+) = diag(evals);
 *     - in each column the entry of largest magnitude is positive (first index on ties), the
 *       rule of the eigenfaces;
 *     - A is row-major [k][m];  1 <= m <= min(k, C+ - 1), else EF_E_INVALID;
 *     - k > 256 is EF_E_INVALID (the Cholesky-inverse kernel's limit, see ef_chol_inv).
 *   EF_E_NUMERIC when Sw_g is singular: n - C+ < k without shrinkage (rank Sw <= n - C+; too few
 *   rows per identity for k, the classic small-sample case), or a pivot of the factorisation not
 *   above 1e-12 of the largest diagonal entry; ef_last_error names n - C+, k and the shrinkage.
 *   mean and class_means may be NULL.
 * With EF_MEM_DEVICE every pointer is a device pointer and the work is ordered on the context's
 * stream; both calls return after it has completed (the labels are grouped on the host: 4 bytes
 * per row come down and 8 go up, these are fit-time calls). */
int ef_lda_order(const int32_t* labels, int64_t n, int32_t n_classes, int64_t* order /* [n] */,
                 int64_t* offsets /* [n_classes + 1] */);
int ef_lda_scatter(ef_ctx* ctx, const void* F, int32_t f_dtype, int64_t n, int32_t k, const int32_t* labels,
                   int32_t n_classes, int64_t* counts, double* mean, double* class_means, double* Sw, double* Sb,
                   uint32_t flags);
int ef_lda_fit(ef_ctx* ctx, const void* F, int32_t f_dtype, int64_t n, int32_t k, const int32_t* labels,
               int32_t n_classes, int32_t m, double shrinkage, double* A /* [k][m] */, double* evals /* [m] */,
               double* mean /* [k] or NULL */, double* class_means /* [C][k] or NULL */, uint32_t flags);

/* ------------------------------------------------------------------ model bank
 * Added after API v7 without a version bump (purely additive): detect the entry points by
 * symbol (dlsym / hasattr), not by ef_api_version().
 *
 * Replaces the per-model loop of recognize_face_all_models (scan-template-v4.py:289-319),
 * where every person has a scaler + PCA (folded into mean, W) and a small gallery of their
 * own.  A bank holds any number of (mean, W, gallery) triples resident together on one
 * context, beside and independent of the context's single model (ef_model_set) and gallery
 * (ef_gallery_set).  One ef_bank_recognize call projects a batch of probes through every
 * model and searches every gallery; the number of kernel launches does not depend on the
 * number of models.
 *
 * ef_bank_add appends a slot (slots are numbered in order of addition, *slot_out optional):
 *   mean[d], W[d*k] as ef_model_set, G[n*k] as ef_gallery_set (n >= 0; an empty gallery
 *   answers EF_KEY_NONE), 1 <= k <= 65536, host pointers or device pointers with
 *   EF_MEM_DEVICE.  The first slot fixes d.  EF_E_INVALID for another d, EF_MODEL_BF16 or a
 *   slot beyond EF_BANK_MAX_MODELS.  A failed add (EF_E_NOMEM included) leaves the bank as it
 *   was.  Synchronous on return in both forms.
 * ef_bank_clear drops every slot and frees the bank's memory (ef_destroy does too).
 * ef_bank_info: slots, d, sum of k, sum of gallery rows (each output optional; zeros when empty).
 *
 * ef_bank_recognize: P[b*d] pixels (EF_U8 or EF_F32), b <= EF_BANK_MAX_PROBES, M = slots:
 *   keys[b][M]      per (probe, slot) the key ef_search would return for that slot's gallery
 *                   given that slot's features of the probe (global_offset 0): the fp64 score
 *                   of every row, the lowest row among those within 1e-12 * (|min| + scale) of
 *                   the minimum, key = pack((float)score, row); EF_KEY_NONE for an empty slot
 *   matches[b][M]   optional: the records ef_search_matches would return (scale: L2
 *                   |q|^2 + the slot's max |g|^2, COSINE 1)
 *   best_slot[b]    optional: the reference's choice over models on the decoded fp32 scores.
 *                   COSINE: start from 0.0, slots in order, a slot wins only with a strictly
 *                   greater similarity (scan-template-v4.py:293-309); L2: the same walk on
 *                   the negated distance from -inf (the first smallest distance).  -1 when no
 *                   slot wins; empty slots never win
 *   feats[b][sum k] optional: slot m's k_m columns start at column sum_{j<m} k_j.  The
 *                   features are deterministic and within ef_project's error bound, but not
 *                   bit-identical to ef_project's (another fp32 summation order)
 * b = 0 is EF_OK; EF_E_STATE for an empty bank or with a communicator of more than one rank
 * attached.  Host pointers: synchronous.  EF_MEM_DEVICE: every array is a device pointer,
 * stream-ordered on the ctx's stream, no host synchronisation (the first call after the bank
 * changed uploads its tables and waits for that once).
 *
 * ef_bank_schedule (host only, no ctx, no GPU): the grouped projection's plan for b probes of
 * d pixels through n_models models of widths k[]: one K-split count for all work items
 * (*nsplit, 1 .. 64) of *pix_per_split pixels each (a multiple of 32), *n_workgroups =
 * ceil(b / 128) x (sum of 128-column tiles) x nsplit, and *scratch_bytes of partial slabs
 * and padded feature blocks.  Each output is optional. */
#define EF_BANK_MAX_MODELS 4096
#define EF_BANK_MAX_PROBES 4096 /* per ef_bank_recognize call */
int ef_bank_clear(ef_ctx* ctx);
int ef_bank_add(ef_ctx* ctx, const float* mean, const float* W, int64_t d, int32_t k, const float* G, int64_t n,
                uint32_t flags, int32_t* slot_out);
int ef_bank_info(const ef_ctx* ctx, int32_t* n_models, int64_t* d, int64_t* total_k, int64_t* total_rows);
int ef_bank_recognize(ef_ctx* ctx, const void* P, int32_t p_dtype, int64_t b, int32_t metric,
                      int64_t* keys /* [b][M] */, ef_match* matches /* [b][M], optional */,
                      int32_t* best_slot /* [b], optional */, float* feats /* [b][sum k], optional */,
                      uint32_t flags);
int ef_bank_schedule(int64_t b, int64_t d, const int32_t* k, int32_t n_models, int32_t* nsplit,
                     int64_t* pix_per_split, int64_t* n_workgroups, int64_t* scratch_bytes);

/* --------------------------------- model bank: distance from face space and a face gate
 * Added the same way (by symbol, EF_API_VERSION stays 7).  Turk-Pentland's face / non-face test
 * (ef_face_distance) for every slot of the bank at once: per (probe, slot)
 *   dffs2  = sum_j (s_j (p_j - mean_j - (f . R)_j))^2     the distance from slot m's face space
 *   energy = sum_j (s_j (p_j - mean_j))^2
 * at slot m's own features f of the probe, the ones ef_bank_recognize returns.
 *
 * ef_bank_recon_set gives slot `slot` its way back: R[k*d] and weight[d] (NULL: ones) mean what
 *   they mean in ef_recon_set, for the slot's k and the bank's d; host pointers, or device
 *   pointers with EF_MEM_DEVICE.  EF_E_INVALID for a slot outside the bank.  The new state is
 *   built completely, then published: a failed call (EF_E_NOMEM included) leaves the slot's
 *   previous state and the bank as they were.  Synchronous on return in both forms.  A later
 *   ef_bank_add keeps the earlier slots' state; ef_bank_clear and ef_destroy free it.
 *
 * ef_bank_face_distance: P[b*d] pixels (EF_U8 or EF_F32), b <= EF_BANK_MAX_PROBES -> dffs2[b][M]
 *   and, each optional, energy[b][M] and feats[b][sum k] (as ef_bank_recognize lays them out,
 *   and the same bits: they are the features the residual consumed).  Four launches whatever M
 *   is: the grouped projection, its reduce, the grouped residual GEMM (timer EF_KERNEL_RECON)
 *   and its reduce (EF_KERNEL_RECON_REDUCE); no search.  No floating-point atomics: the same
 *   inputs on the same bank give the same bits on every call.  EF_E_STATE for an empty bank,
 *   for a bank in which a slot has no reconstruction state (ef_last_error names the first such
 *   slot), or with a communicator of more than one rank attached.  b = 0 is EF_OK.
 *
 * ef_bank_recognize_gated: ef_bank_recognize and ef_bank_face_distance from one projection.
 *   keys, matches and feats are bit-identical to ef_bank_recognize on the same bank, rows and
 *   b; dffs2 (required) and energy to ef_bank_face_distance.  Only best_slot differs: the walk
 *   over models skips slot m for probe p when dffs2[p][m] > bound is true, where bound is
 *   gate[m], or gate[m] * energy[p][m] (one fp32 multiply) with EF_BANK_GATE_RELATIVE.  The
 *   comparison is made on the fp32 values returned and is false for NaN, so a gate of +inf or
 *   NaN rejects nothing and the host can reproduce the decision exactly.  gate[M] is a host
 *   pointer, or a device pointer with EF_MEM_DEVICE.
 *
 * ef_scan_frame_gated: ef_scan_frame whose step e is ef_bank_recognize_gated on the same rows
 *   (bit-identical to that call with b = n_groups); dets, keys and rows are ef_scan_frame's.
 *   dffs2[n_groups][M] is required, energy optional.  Host pointers: still one upload of the
 *   frame (the gate stays resident with the scan plan and travels again only when its values
 *   change), one download of one pinned result block (it grows only in this call) and one
 *   synchronisation; EF_MEM_DEVICE: nothing waits on the host.
 *
 * ef_bank_recon_schedule (host only, no ctx, no GPU): the grouped residual's plan for b probes
 * of d pixels against n_models slots: one pixel-split count for the launch (*nsplit, 1 .. 64,
 * chosen so that ceil(b / 128) x n_models x nsplit is about 512 workgroups, capped at the
 * number of 128-pixel tiles) of *tiles_per_split tiles each, *n_workgroups = ceil(b / 128) x
 * n_models x nsplit, and *scratch_bytes = 2 x nsplit x n_models x round_up(b, 128) x 4 of
 * partials.  Each output is optional; EF_E_INVALID for the sizes ef_bank_schedule rejects. */
int ef_bank_recon_set(ef_ctx* ctx, int32_t slot, const float* R /* [k*d] */, const float* weight /* [d] or NULL */,
                      uint32_t flags);
int ef_bank_face_distance(ef_ctx* ctx, const void* P, int32_t p_dtype, int64_t b, float* dffs2 /* [b][M] */,
                          float* energy /* [b][M], optional */, float* feats /* [b][sum k], optional */,
                          uint32_t flags);
int ef_bank_recognize_gated(ef_ctx* ctx, const void* P, int32_t p_dtype, int64_t b, int32_t metric,
                            const float* gate /* [M] */, int64_t* keys /* [b][M] */,
                            ef_match* matches /* [b][M], optional */, int32_t* best_slot /* [b], optional */,
                            float* dffs2 /* [b][M] */, float* energy /* [b][M], optional */,
                            float* feats /* [b][sum k], optional */, uint32_t flags);
int ef_bank_recon_schedule(int64_t b, int64_t d, int32_t n_models, int32_t* nsplit, int32_t* tiles_per_split,
                           int64_t* n_workgroups, int64_t* scratch_bytes);

/* ------------------------------------------------------------- multi-GPU (RCCL)
 * Row-sharded gallery across the ranks of one job, one process per GPU:
 * rank r sets its shard with ef_gallery_set(..., global_offset = first global row).
 * Once a communicator is attached, ef_search / ef_recognize (and the _matches forms) on
 * every rank return the GLOBAL result: each rank searches its shard, the match records
 * are all-gathered over RCCL (xGMI) and merged exactly (ef_matches_merge) on the ctx's
 * stream.  ef_recognize additionally splits the projection: rank r projects probes
 * [r*c, (r+1)*c), c = ceil(b / nranks), and the features are all-gathered.  Every rank
 * must make the same calls with the same b and metric (collectives).  RCCL is loaded at
 * run time (librccl.so.1); EF_E_STATE if it is unavailable.
 * ef_comm_unique_id: rank 0 creates the id (EF_UNIQUE_ID_BYTES bytes) and the caller
 * broadcasts it (e.g. over torch.distributed or MPI). */
#define EF_UNIQUE_ID_BYTES 128
int ef_comm_unique_id(void* id_out);
int ef_comm_init(ef_ctx* ctx, int32_t nranks, int32_t rank, const void* unique_id);
int ef_comm_destroy(ef_ctx* ctx);
int ef_comm_info(const ef_ctx* ctx, int32_t* nranks, int32_t* rank);

/* ------------------------------------------------------------------ options
 * Per-context tunables (defaults in brackets). */
#define EF_OPT_FIT_MAX_ITERS 1   /* subspace-iteration cap [500]; reaching it unconverged -> EF_E_NUMERIC */
#define EF_OPT_FIT_FP32_COARSE 2 /* 1 [default]: a coarse phase of reduced-precision C.Q products while
                                    the Ritz values still move (self-correcting; split-bf16 matrix-core
                                    products for a 256-wide block, fp32 otherwise); 2: the same with
                                    fp32 products; 0: fp64 products throughout */
#define EF_OPT_COV_SLAB_BYTES 3  /* device budget of the int32 covariance partial sums [8 GiB];
                                    smaller budgets run the multi-pass int64 schedule */
#define EF_OPT_TM_INT64_SUMS 4   /* 1: int64 integral images in the template localiser [0: auto] */
#define EF_OPT_HAAR_ORDERED 5    /* 1: sequential stage sums even when reassociation is exact [0] */
#define EF_OPT_JPEG_CHUNK_BITS 6 /* entropy-decode chunk per GPU thread, bits (multiple of 32) [0: auto] */
#define EF_OPT_SEARCH_SPLIT_BF16 7 /* 1: gallery scans on bf16 MFMA with split (hi + lo) fp32 operands
                                      and a widened error bound; identities and scores are still
                                      fp64-resolved, so results equal the fp32 scan's [0]; 2: the same
                                      with the 32x32x16 kernel at k in (64, 128] (comparison); 3: at
                                      k > 128 a single-bf16 screen (one bf16 MFMA per product, fp32
                                      accumulation, a bf16-wide bound) — still fp64-resolved, same
                                      results, fewer MFMAs; more probes reach the resolution when
                                      the best two rows are within ~2% (k <= 128: as 1) */
#define EF_OPT_JPEG_PART_FILES 8   /* ef_jpeg_ingest decodes in parts of this many files, staging
                                      part i + 1 on a host thread while part i decodes [8192] */
#define EF_OPT_FIT_CHEBYSHEV 9     /* 1 [default]: the subspace iteration advances a Chebyshev
                                      three-term recurrence on [0, theta_m] between Rayleigh-Ritz
                                      steps; 0: one shifted power step per iteration */
#define EF_OPT_HOST_THREADS 10     /* host worker threads for the JPEG parse / destuff, PROCESS-WIDE
                                      (any context sets it) [0: min(16, hardware threads)]; the
                                      Python Engine sets the job's CPU share (API v7) */
#define EF_OPT_SEARCH_PREFIX 11    /* L2 fp32 scans at padded k <= 128: scan the first K1 components of
                                      every row (a lower bound of the distance), prove the winner
                                      from it and send only unproven probes through the full-k
                                      scan; results are those of 0.  0: off; 1 [default]: auto
                                      (K1 = 32 at padded k = 128 and >= 65536 rows, else off);
                                      16 / 32 / 64: that K1 at any size (must be < the padded k of
                                      the gallery in place) */
#define EF_OPT_SEARCH_TOPK_CAND 12 /* top-m search: candidate rows kept per probe for the fp64
                                      resolution [1024], 16 .. 4096 and at least the m of the call;
                                      scratch is (padded probes) x this x 4 B.  A probe with more
                                      rows inside its cut gets a tighter cut and a second round,
                                      then a full fp64 sweep; results never depend on it */
#define EF_OPT_SEARCH_PREFIX_SPLIT 13 /* arithmetic of the EF_OPT_SEARCH_PREFIX scan.  1 [default]:
                                      split-bf16 operands on bf16 MFMA (hi.hi' + hi.lo' + lo.hi')
                                      over a split copy of the prefix, proven with the split
                                      chain's wider bound; 0: the fp32 scan.  Results are the same;
                                      the compact copy (n x K1 x 4 B + 8 n B either way) is rebuilt
                                      on the next search after a change */
#define EF_OPT_PROJECT_SPLIT_BF16 14 /* projection of uint8 probes with an fp32 model (added by symbol,
                                      EF_API_VERSION stays 7).  1 [default]: where eligible (uint8
                                      probes on a 16-byte aligned pointer, d % 64 == 0, more than 64
                                      padded components, a model without EF_MODEL_BF16 that passes
                                      the guard) the projection runs on bf16 MFMA as
                                      (p - round(mean)).(W_hi + W_mid + W_lo) - (mean - round(mean)).W:
                                      the three bf16 pieces sum to the fp32 W exactly and
                                      p - round(mean) is an integer of at most 8 bits, so no input
                                      is rounded and only the fp32 accumulation rounds; the
                                      correction row is computed in fp64 once per model.  The guard,
                                      run once per model on the device: every W element finite and
                                      equal to the sum of its pieces, every piece zero or a normal
                                      bf16, every round(mean) in 0..255; a model that fails it, and
                                      every ineligible call, takes the fp32 kernel.  The pieces
                                      (6 B per padded W element) are built by the first eligible
                                      projection after ef_model_set.  Features differ from option
                                      0's in their last bits (as between two batch sizes) and
                                      repeat bit for bit from call to call.  0: always the fp32
                                      kernel */
#define EF_OPT_SEARCH_PREFIX_SCREEN 16 /* the EF_OPT_SEARCH_PREFIX scan as a cascade (added by symbol,
                                      EF_API_VERSION stays 7).  1 [default]: where the split-bf16
                                      prefix scan runs at K1 <= 32, a single-bf16 screen (one bf16
                                      product per element over a bf16 copy of the prefix, n x K1 x
                                      2 B) goes first and proves a probe's winner with a bound
                                      taken per row and per probe, es (||q[:K1]||^2 + ||g[:K1]||^2),
                                      es = 2.01 2^-8; the split scan runs for the probes it cannot
                                      prove alone, the full-k scan for the rest.  Results are those
                                      of 0.  0: the split scan for every probe */
#define EF_OPT_RANK_BITMAP_BYTES 15 /* diagnostic (added by symbol): device budget of ef_search_rank's
                                      (probe, identity) bitmap [256 MiB]; the probes run in pieces
                                      of whole 256-probe blocks that fit it, a value below one
                                      block's need means one block per piece.  The result does not
                                      depend on it.  >= 1 */
int ef_set_option(ef_ctx* ctx, int32_t option, int64_t value);
int ef_get_option(const ef_ctx* ctx, int32_t option, int64_t* value);

/* ------------------------------------------------------------------ ingest
 * Replaces the per-image cv2.cvtColor(img, COLOR_BGR2GRAY) + cv2.resize(gray, (w, h))
 * (INTER_LINEAR) of train-v4.py:59-68 and scan-template-v4.py:257-263 for a ragged
 * batch of decoded images in one launch, with OpenCV's CV_8U fixed-point arithmetic
 * (parity against OpenCV unpinned: OpenCV is not installed where this was built).
 * Image i: heights[i] x widths[i] x channels[i] (1, 3 = BGR, 4 = BGRA; EF_IMG_RGB for
 * RGB order; channels NULL = all 1) uint8 pixels at data + offsets[i], row-major.
 * out: count x out_h x out_w uint8 (the probe / training row layout, train-v4.py:68).
 * data/out are host pointers, or device pointers with EF_MEM_DEVICE; the metadata
 * arrays are always host arrays.  At most 65535 images per call. */
int ef_preprocess(ef_ctx* ctx, const uint8_t* data, const int64_t* offsets, const int32_t* heights,
                  const int32_t* widths, const int32_t* channels, int64_t count, int32_t out_h,
                  int32_t out_w, uint8_t* out, uint32_t flags);

/* ------------------------------------------------------------------ JPEG decode
 * Replaces the per-file cv2.imread of the ingest paths (train-v4.py:59 IMREAD_COLOR;
 * useless/train.py:33 and scan-template-v4.py:52 IMREAD_GRAYSCALE) for a batch of
 * JPEG files: image i is sizes[i] bytes at data + offsets[i] (data is always a host
 * pointer).  Decoded on the GPU with libjpeg-turbo's default arithmetic (islow IDCT,
 * fancy upsampling, its YCbCr->RGB tables), so the pixels equal what imread returns:
 *   EF_JPEG_GRAY  h x w luma (libjpeg JCS_GRAYSCALE output, IMREAD_GRAYSCALE)
 *   EF_JPEG_BGR   h x w x 3 BGR (IMREAD_COLOR)
 * written at out + out_offsets[i] (host, or device with EF_MEM_DEVICE — then the
 * pixels can go straight into ef_preprocess with EF_MEM_DEVICE).  Supported: sequential
 * Huffman (SOF0/SOF1) 8-bit, 1 or 3 components, luma at the maximal sampling factors,
 * chroma at 1x or 2x horizontally and vertically (4:4:4, 4:2:2, 4:2:0), one scan,
 * restart intervals.  status[i] (optional) is 0, or EF_JPEG_E_UNSUPPORTED /
 * EF_JPEG_E_CORRUPT for a file the caller must decode on the host (nothing is written
 * for it).  ef_jpeg_info parses the headers on the host (no context, no GPU). */
#define EF_JPEG_GRAY 0
#define EF_JPEG_BGR 1
#define EF_JPEG_E_UNSUPPORTED (-10)
#define EF_JPEG_E_CORRUPT (-11)
int ef_jpeg_info(const uint8_t* data, const int64_t* offsets, const int64_t* sizes, int32_t count, int32_t* heights,
                 int32_t* widths, int32_t* components, int32_t* status);
int ef_jpeg_decode(ef_ctx* ctx, const uint8_t* data, const int64_t* offsets, const int64_t* sizes, int32_t count,
                   int32_t mode, uint8_t* out, const int64_t* out_offsets, int32_t* status, uint32_t flags);
/* Fused ingest (train-v4.py:59-68 for a batch of files): decode, then ef_preprocess's
 * grey + INTER_LINEAR resize to out_h x out_w computed straight from the decoded planes
 * (the same pixels as ef_jpeg_decode followed by ef_preprocess).  out: count x out_h x out_w
 * uint8 rows (host, or device with EF_MEM_DEVICE); the row of a file with status[i] != 0 is
 * zero and the caller decodes that file itself.  status is final on return.  With
 * EF_MEM_DEVICE the rows are stream-ordered on ctx's stream and the call returns once the
 * decode is queued (no host wait), so the next call's host-side parse overlaps this
 * decode; ef_jpeg_decode with EF_MEM_DEVICE behaves the same.  Host outputs return complete. */
int ef_jpeg_ingest(ef_ctx* ctx, const uint8_t* data, const int64_t* offsets, const int64_t* sizes, int32_t count,
                   int32_t mode, int32_t out_h, int32_t out_w, uint8_t* out, int32_t* status, uint32_t flags);

/* -------------------------------------------------------- template localiser
 * Replaces template_match_all_models' inner loops (scan-template-v4.py:127-200):
 * for every problem p = (template t, scaled size h x w):
 *   R_p = cv2.matchTemplate(frame, cv2.resize(template_t, (w, h)), TM_CCOEFF_NORMED)
 *   (best, (x, y)) = cv2.minMaxLoc(R_p) maximum (first in raster order).
 * The correlation is exact (int8 matrix cores, int64 sums); the normalisation follows
 * OpenCV's rule in float64, R is float32.  ef_tm_prepare uploads the grey templates
 * (templ_h[i] x templ_w[i] at templ_data + templ_offsets[i]), resizes them on the GPU
 * and builds the resident operands for a frame_h x frame_w frame; ef_tm_match then
 * runs one frame (row stride frame_ld bytes) and returns per problem best_out, x_out,
 * y_out (each optional) and, if maps_out is non-NULL, every R_p concatenated
 * (sizes from ef_tm_info).  Host pointers unless EF_MEM_DEVICE. */
int ef_tm_prepare(ef_ctx* ctx, const uint8_t* templ_data, const int64_t* templ_offsets,
                  const int32_t* templ_h, const int32_t* templ_w, int32_t n_templates,
                  const int32_t* prob_templ, const int32_t* prob_h, const int32_t* prob_w,
                  int32_t n_problems, int32_t frame_h, int32_t frame_w, uint32_t flags);
int ef_tm_match(ef_ctx* ctx, const uint8_t* frame, int64_t frame_ld, float* best_out, int32_t* x_out,
                int32_t* y_out, float* maps_out, uint32_t flags);
int ef_tm_info(ef_ctx* ctx, int32_t* n_problems, int64_t* map_elems, int32_t* result_h,
               int32_t* result_w);
/* Host-only (API v7): the integral-image width ef_tm_prepare picks for a frame_h x frame_w
 * frame whose largest template area is max_template_area: 32 (wrapping uint32 sums) when
 * every area is < 2^18 and (frame_h + 1)(frame_w + 1) < 2^30, else 64 (int64 sums); the
 * EF_OPT_TM_INT64_SUMS option forces 64 per context.  EF_E_INVALID on bad sizes. */
int ef_tm_sums_bits(int32_t frame_h, int32_t frame_w, int64_t max_template_area);

/* ------------------------------------------------------------------ ROI ingest
 * Added after API v7 without a version bump (purely additive): detect by symbol.
 *
 * ef_preprocess for n rectangles of one frame, without copying the crops out: row i of out
 * (n x out_h x out_w uint8) is bit-identical to ef_preprocess of the contiguous copy of
 * frame[y:y+h, x:x+w] (scan-template-v4.py:360, :390; useless/scan.py:231-249), with the same
 * meaning of EF_IMG_RGB and the same identity and exact-2x shortcuts.  The frame is
 * frame_h x frame_w x channels (1, 3, 4) with a row stride of frame_ld >= frame_w * channels
 * bytes; rects[i] = {x, y, w, h}.  The bilinear neighbours clamp to the rectangle, never to
 * the frame.
 *   host rects (default): x, y >= 0, w, h > 0, x + w <= frame_w and y + h <= frame_h, else
 *     EF_E_INVALID naming the rectangle; the call waits for the stream before it returns.
 *   EF_ROI_RECTS_DEVICE: rects is a device pointer (it may have been written by a kernel
 *     queued earlier on the ctx's stream).  Nothing can be validated on the host, so the
 *     kernel clips every rectangle to the frame before any load: a rectangle that overhangs
 *     gives the row of its clipped part, one that is empty after clipping or has a negative
 *     origin gives an all-zero row, and no value makes the kernel read outside
 *     frame_h x frame_ld bytes.
 *   EF_MEM_DEVICE: frame and out are device pointers; with EF_ROI_RECTS_DEVICE too the call is
 *     stream-ordered with no host wait.
 * n <= 65535; n = 0 is EF_OK. */
int ef_preprocess_rois(ef_ctx* ctx, const uint8_t* frame, int64_t frame_ld, int32_t frame_h, int32_t frame_w,
                       int32_t channels, const int32_t* rects, int64_t n, int32_t out_h, int32_t out_w,
                       uint8_t* out, uint32_t flags);

/* ------------------------------------------------------------------ frame scan
 * Added after API v7 without a version bump (purely additive): detect by symbol.
 *
 * One frame of the live loop (scan-template-v4.py:340-391) as one stream-ordered sequence:
 * BGR -> grey, template_match_all_models (:127-200), the crop + grey + resize of every
 * detection (:360, :257-263) and recognize_face_all_models (:289-319) through the model bank.
 *
 * ef_scan_prepare: needs a prepared localiser (ef_tm_prepare), else EF_E_STATE.  Problem p of
 *   the localiser belongs to group prob_group[p] in [0, n_groups) (a group is a person, the
 *   reference's models in order), 1 <= n_groups <= EF_BANK_MAX_PROBES.  Faces are resized to
 *   face_h x face_w; `threshold` is template_match_all_models' (0.6).  The four integers of
 *   is_detection_in_corner, int(W*0.15), int(H*0.15), int(W*0.05), int(H*0.05), are computed
 *   here once, in double arithmetic.  The plan belongs to the localiser: a new ef_tm_prepare
 *   drops it.  Host pointer; synchronous.
 *
 * ef_scan_frame: frame is frame_h x frame_w (of ef_tm_prepare) x channels (1 grey; 3, 4 BGR(A),
 *   or RGB(A) with EF_IMG_RGB), row stride frame_ld bytes.  On the ctx's stream it queues
 *     a. channels 3, 4: the grey plane, BT.601 fixed point as ef_preprocess;
 *     b. the localiser's kernels (as ef_tm_match) on that plane;
 *     c. per group template_match_all_models' rule over the group's problems in index order: a
 *        candidate with v > best (strict, best from 0.0) that is_detection_in_corner rejects
 *        never changes the state, any other becomes the best; a best with (double)v >
 *        threshold is a detection -> dets[g] = {found, problem, x, y, w, h, confidence};
 *        every field is 0 where found = 0;
 *     d. ef_preprocess_rois of the dets' rectangles on the grey plane -> rows[g] (zero where
 *        found = 0);
 *     e. ef_bank_recognize of those n_groups rows (EF_U8, b = n_groups, `metric`) ->
 *        keys[n_groups][M] and best_slot[n_groups], with exactly ef_bank_recognize's meaning
 *        (bit-identical to that call on the same rows with the same b).
 *   best_slot and rows are optional.  EF_E_STATE without a scan plan, with an empty bank, when
 *   the bank's d is not face_h * face_w, or with a communicator of more than one rank attached.
 *   Host pointers: one upload of the frame, one download of one pinned result block, one
 *   stream synchronisation.  EF_MEM_DEVICE: every array is a device pointer and nothing waits
 *   on the host (apart from the bank's one-time table upload after the bank changed). */
typedef struct ef_scan_det {
  int32_t found, problem, x, y, w, h;
  float confidence;
  int32_t pad;
} ef_scan_det;
int ef_scan_prepare(ef_ctx* ctx, const int32_t* prob_group /* [n_problems] */, int32_t n_groups, int32_t face_h,
                    int32_t face_w, double threshold);
int ef_scan_frame(ef_ctx* ctx, const uint8_t* frame, int64_t frame_ld, int32_t channels, int32_t metric,
                  ef_scan_det* dets /* [n_groups] */, int64_t* keys /* [n_groups][M] */,
                  int32_t* best_slot /* [n_groups], optional */, uint8_t* rows /* [n_groups][face_h*face_w], optional */,
                  uint32_t flags);
/* the gated form: see ef_bank_recognize_gated above */
int ef_scan_frame_gated(ef_ctx* ctx, const uint8_t* frame, int64_t frame_ld, int32_t channels, int32_t metric,
                        const float* gate /* [M] */, ef_scan_det* dets, int64_t* keys, int32_t* best_slot,
                        uint8_t* rows, float* dffs2 /* [n_groups][M] */, float* energy /* [n_groups][M], optional */,
                        uint32_t flags);

/* --------------------------------------------------------- Haar cascade detector
 * Replaces face_cascade.detectMultiScale(gray, scaleFactor, minNeighbors, minSize)
 * (detection-v4.py:18, :50-55) for a stump-based HAAR cascade as OpenCV stores it
 * (stages of depth-1 trees over up-to-3-rectangle features, no tilted features):
 *   features i: rects[i][k] = {x, y, w, h} in window coordinates, weights[i][k] (k < 3,
 *               weight 0 = unused third rectangle);
 *   stages s:   stage_count[s] consecutive stumps, stage_threshold[s];
 *   stumps j:   feature index, threshold, left leaf (value < threshold), right leaf.
 * ef_haar_detect runs the image pyramid, variance normalisation and cascade on the GPU
 * and cv::groupRectangles(min_neighbors, 0.2) on the host; rects_out holds up to
 * max_rects {x, y, w, h}, *n_rects the total; cand_out (optional) the ungrouped
 * candidates in OpenCV's (scale, y, x) order.  max_w/max_h <= 0 means the frame size.
 * The frame is a host pointer (row stride ld) unless EF_MEM_DEVICE.  Parity against
 * OpenCV is unpinned (OpenCV and its cascade files are absent where this was built);
 * OpenCV's pyramid uses INTER_LINEAR_EXACT, this one INTER_LINEAR. */
int ef_haar_set_cascade(ef_ctx* ctx, int32_t win_w, int32_t win_h, int32_t n_features, const int32_t* rects,
                        const float* weights, int32_t n_stages, const int32_t* stage_count,
                        const float* stage_threshold, int32_t n_stumps, const int32_t* stump_feature,
                        const float* stump_threshold, const float* stump_left, const float* stump_right);
int ef_haar_detect(ef_ctx* ctx, const uint8_t* gray, int32_t h, int32_t w, int64_t ld, double scale_factor,
                   int32_t min_neighbors, int32_t min_w, int32_t min_h, int32_t max_w, int32_t max_h,
                   int32_t* rects_out, int32_t max_rects, int32_t* n_rects, int32_t* cand_out, int32_t max_cand,
                   int32_t* n_cand, uint32_t flags);

/* ------------------------------------------------------- Haar route in one call
 * Added after API v7 without a version bump (purely additive): detect by symbol.
 *
 * One frame of the Haar live loop (useless/scan.py:168-290, detection-v4.py:47-60:
 * cvtColor -> detectMultiScale -> crop -> resize -> recognise) as one stream-ordered sequence,
 * with cv::groupRectangles on the GPU.
 *
 * ef_haar_group: cv::groupRectangles(rects, min_neighbors, 0.2) on the GPU for n rectangles
 *   {x, y, w, h} in list order -> the grouped rectangles in OpenCV's order (classes numbered by
 *   their first member), value for value what ef_haar_detect's host grouping gives.  rects_out
 *   takes up to max_rects of them, *n_rects the total.  min_neighbors <= 0 is EF_E_INVALID (the
 *   host function returns its input there).  n > EF_HAAR_GROUP_MAX: the kernels group nothing,
 *   *n_rects is 0 and the call returns EF_E_INVALID naming EF_HAAR_SCAN_OVERFLOW.  Host pointers
 *   (synchronous), or device pointers with EF_MEM_DEVICE (stream-ordered, n_rects too).  Needs no
 *   cascade.  The same input gives the same bits on every call.
 *
 * ef_haar_scan_prepare: needs a cascade (ef_haar_set_cascade), else EF_E_STATE; a new cascade
 *   drops the plan.  Fixes, for frames of frame_h x frame_w, everything ef_haar_detect derives
 *   per call from (scale_factor, min_w/h, max_w/h; max <= 0: the frame size): the scale list, the
 *   pyramid layers, the row table, the resize descriptors and the buffer sizes.  min_neighbors
 *   >= 1; faces are resized to face_h x face_w; 1 <= max_faces <= EF_BANK_MAX_PROBES;
 *   1 <= max_candidates <= EF_HAAR_GROUP_MAX.  Synchronous.
 *
 * ef_haar_scan_frame: frame is frame_h x frame_w x channels (1 grey; 3, 4 BGR(A), or RGB(A) with
 *   EF_IMG_RGB), row stride frame_ld bytes.  On the ctx's stream it queues
 *     a. channels 3, 4: the grey plane, BT.601 fixed point as ef_preprocess;
 *     b. ef_haar_detect's kernels on that plane (stage-group grids sized by the plan's bound);
 *     c. the grouping kernels -> rects[max_faces] (zeros behind the grouped rectangles) and
 *        head = {status, n_candidates, n_rects, n_faces = min(n_rects, max_faces)}: the rectangles
 *        and n_rects are ef_haar_detect's on the grey plane.  More than max_candidates
 *        candidates: nothing is grouped, status has EF_HAAR_SCAN_OVERFLOW and n_rects = 0 (the
 *        caller redoes the frame with ef_haar_detect);
 *     d. ef_preprocess_rois of rects on the grey plane -> rows[max_faces] (zero behind n_rects);
 *     e. ef_bank_recognize of those rows (EF_U8, b = max_faces, `metric`), or with gate non-null
 *        ef_bank_recognize_gated (EF_BANK_GATE_RELATIVE as there; dffs2 is then required) ->
 *        keys, best_slot, dffs2, energy with exactly that call's meaning and bits.
 *   best_slot, rows and energy are optional.  EF_E_STATE without a plan, with an empty bank, when
 *   the bank's d is not face_h * face_w, or with a communicator of more than one rank attached.
 *   Host pointers: one upload of the frame, one download of one pinned result block, one stream
 *   synchronisation.  EF_MEM_DEVICE: every array is a device pointer and nothing waits on the host
 *   (apart from the bank's one-time table upload after the bank changed). */
#define EF_HAAR_GROUP_MAX 16384       /* rectangles per grouping; the ceiling of max_candidates */
#define EF_HAAR_SCAN_OVERFLOW 0x1     /* head.status: more candidates than the plan's max_candidates */
#define EF_HAAR_SCAN_UNCONVERGED 0x2  /* head.status: a grouping loop reached its iteration bound */
#define EF_KERNEL_HAAR_SCAN 11 /* everything one ef_haar_scan_frame queues; the bank's launches inside it also
                                  count under EF_KERNEL_PROJECT and EF_KERNEL_SEARCH; EF_KERNEL_HAAR and
                                  EF_KERNEL_INGEST do not count these frames */
typedef struct ef_haar_scan_head {
  int32_t status, n_candidates, n_rects, n_faces;
} ef_haar_scan_head;
int ef_haar_group(ef_ctx* ctx, const int32_t* rects /* [n][4] */, int32_t n, int32_t min_neighbors,
                  int32_t* rects_out /* [max_rects][4] */, int32_t max_rects, int32_t* n_rects, uint32_t flags);
int ef_haar_scan_prepare(ef_ctx* ctx, int32_t frame_h, int32_t frame_w, double scale_factor, int32_t min_neighbors,
                         int32_t min_w, int32_t min_h, int32_t max_w, int32_t max_h, int32_t face_h, int32_t face_w,
                         int32_t max_faces, int32_t max_candidates);
/* the plan's pyramid layers, its bound on the windows one frame can visit (what the stage-group
 * grids and lists are sized by), max_faces and max_candidates; each optional; EF_E_STATE without a plan */
int ef_haar_scan_info(ef_ctx* ctx, int32_t* n_layers, int64_t* visitable, int32_t* max_faces, int32_t* max_candidates);
int ef_haar_scan_frame(ef_ctx* ctx, const uint8_t* frame, int64_t frame_ld, int32_t channels, int32_t metric,
                       const float* gate /* [M] or NULL */, ef_haar_scan_head* head,
                       int32_t* rects /* [max_faces][4] */, int64_t* keys /* [max_faces][M] */,
                       int32_t* best_slot /* optional */, uint8_t* rows /* [max_faces][face_h*face_w], optional */,
                       float* dffs2 /* [max_faces][M], with gate */, float* energy /* optional */, uint32_t flags);

/* ------------------------------------------------------------------ timing
 * Device time of each launch of a kernel, measured with hipEvents on the
 * stream the kernel is launched on. */
int ef_timing_enable(ef_ctx* ctx, int on);
int ef_timing_get(ef_ctx* ctx, int32_t kernel_id, double* total_ms, int64_t* launches);
int ef_timing_reset(ef_ctx* ctx);

/* Prefix-scan counters of the most recent search on this context (EF_OPT_SEARCH_PREFIX):
 * out = {probes, proven by the prefix scan, sent to the full-k scan, 1 if the guard skipped
 * the prefix scan}.  A search the prefix scan does not apply to reports {probes, 0, 0, 0}.
 * Synchronises the context's stream. */
int ef_search_stats(ef_ctx* ctx, int64_t out[4]);

/* Added by symbol (EF_API_VERSION stays 7).  The screen's counters of the most recent search
 * (EF_OPT_SEARCH_PREFIX_SCREEN): out = {probes screened, proven by the screen, 1 if the screen's
 * guard sent the search straight to the split scan}.  A search without the screen reports
 * {0, 0, 0 or 1}.  ef_search_stats counts a probe as proven whichever prefix stage proved it.
 * Python: Engine.search_screen_stats().  Synchronises the context's stream. */
int ef_prefix_screen_stats(ef_ctx* ctx, int64_t out[3]);

#ifdef __cplusplus
}
#endif
#endif /* EIGENFACE_H_ */
