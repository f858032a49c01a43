/*
 * rqhip.h -- C ABI of librqhip.so: the MI355X (gfx950) residual-quantisation hot path.
 *
 * The reference (EdoardoBotta/RQ-VAE-Recommender) is pure Python: it has no FFI, plugin or operator
 * registry for this path, so the drop-in boundary is its Python module API (modules.quantize.Quantize,
 * modules.rqvae.RqVae, init.kmeans.kmeans_init_, ...; mirrored under rq-vae-recommender_amd/).  This
 * header is the C boundary UNDER that mirror: plain pointers and sizes, no torch types.  Each entry
 * point names the reference code it replaces (paths relative to the reference root); INTEGRATION.md
 * shows the ctypes stub a maintainer of the reference would add to call it from modules/quantize.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'ed / torch CUDA tensor data_ptr), fp32 row-major
 *     contiguous, ids int64; optional outputs/inputs may be NULL where stated.
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and the call returns
 *     without synchronising.  The library never allocates, frees or retains device memory: scratch
 *     comes from the caller (`workspace`, size from the matching *_workspace_bytes()).
 *   - return value: 0 = success; negative = RQHIP_E* argument/shape error; positive = hipError_t.
 *     rqhip_last_error() returns a thread-local message for the last failure.
 *   - results are bit-exact with oracle/rq_oracle.c (which fixes every floating-point reduction
 *     order) for everything except transcendental functions in the Gumbel path.
 */
#ifndef RQHIP_H
#define RQHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RQHIP_VERSION 462 /* 462: rqhip_linear_wgrad_f16_batch; 461: rqhip_unique_fraction; 460: rqhip_linear_small; 450: rqhip_rq_seam (round 6); major*10000 + minor*100 + patch; 200: rqhip_rq_forward gained tie_margin; 300: rqhip_rq_forward_ex; 301: rqhip_gemm_split_recon;
                            400: RQHIP_SPLIT_F16X2 (rqhip_gemm_split_ex, rqhip_weight_images, rqhip_maxima, rqhip_linear_wgrad_f16), tagged profile records */

#define RQHIP_OK 0
#define RQHIP_EARG (-1)         /* bad pointer / size / mode */
#define RQHIP_EUNSUPPORTED (-2) /* shape outside what the kernels implement (e.g. D > 128) */
#define RQHIP_EWORKSPACE (-3)   /* workspace missing or too small */

/* forward modes == the reference's QuantizeForwardMode (modules/quantize.py:16-20) plus eval */
#define RQHIP_MODE_EVAL 0     /* module.eval(): quantize.py:159-161 */
#define RQHIP_MODE_STE 1      /* QuantizeForwardMode.STE, training: quantize.py:137-139 */
#define RQHIP_MODE_ROTATION 2 /* QuantizeForwardMode.ROTATION_TRICK, training: quantize.py:140-153 */
#define RQHIP_MODE_GUMBEL 3   /* QuantizeForwardMode.GUMBEL_SOFTMAX, training: quantize.py:131-136 */

typedef void *rqhip_stream_t;

int rqhip_version(void);
const char *rqhip_last_error(void);
/* number of compute units of the current device (grid sizing, reported by bench.py) */
int rqhip_device_cu_count(int *cu_count);

/* ------------------------------------------------------------------------------------------------
 * Residual quantisation, forward.  Replaces the level loop of RqVae.get_semantic_ids
 * (modules/rqvae.py:118-139) together with every Quantize.forward it calls (modules/quantize.py:
 * 104-163: L2 distance :112-117, argmin :128, STE :137-139 / rotation trick :140-153 / eval :159-161,
 * QuantizeLoss modules/loss.py:33-41) and the embs.sum / embs.norm consumers (rqvae.py:146,158).
 * L = 1 is a single Quantize.forward.
 *
 *   res0      [B,D]    level-0 input (encoder output)
 *   codebooks [L,K,D]  out_proj(embedding.weight) of each level
 *   mode      RQHIP_MODE_EVAL | _STE | _ROTATION
 *   beta      commitment weight
 *   ids       [L,B] int64 (required)   -- sem_ids[b,l] = ids[l*B + b]
 *   embs      [L,B,D] or NULL          -- quantized.embeddings per level
 *   residuals [L,B,D] or NULL          -- input of each level
 *   emb_sum   [B,D]   or NULL          -- sum over levels of embs, ((e0+e1)+e2)+...
 *   loss      [B]     or NULL          -- sum over levels of the quantize loss
 *   embs_norm [B,L]   or NULL          -- L2 norm of embs per level
 *   tie_margin [L,B]  or NULL          -- how decisively each level's argmin was taken (SURVEY.md section 8b
 *                                         `tie_margin_flags`): (d2 - d1) / (|x|^2 + |c_id|^2), d1 = dist[id],
 *                                         d2 = smallest distance among the OTHER codes (a duplicate of the minimum
 *                                         counts: margin 0); 0 for rows that took the exact non-finite scan and when
 *                                         the quotient is NaN, +Inf when K == 1.  Two correct fp32 evaluations of
 *                                         quantize.py:113-117 (this kernel's FMA chain, the reference's BLAS) differ by
 *                                         a few ulp of |x|^2 + |c|^2, so ids can only differ on rows whose margin is
 *                                         below ~1e-6: a caller that needs the reference's ids bit for bit adjudicates
 *                                         exactly those rows (tests/test_gpu_reference_parity.py does, in fp64).
 *                                         Requesting it selects a kernel variant with more work per code (+6 % kernel time at 100 000 x 3 x 256).
 *   workspace rqhip_rq_forward_workspace_bytes(L,K) bytes of scratch (codebook norms)
 * Limits: 1 <= D <= 128, 1 <= K <= 65536, 1 <= L <= 16.
 */
size_t rqhip_rq_forward_workspace_bytes(int L, int K);
int rqhip_rq_forward(const float *res0, int64_t B, int D, const float *codebooks, int L, int K,
                     int mode, float beta, int64_t *ids, float *embs, float *residuals,
                     float *emb_sum, float *loss, float *embs_norm, float *tie_margin, void *workspace,
                     size_t workspace_bytes, rqhip_stream_t stream);
/* The same call with explicit kernel-selection flags (bench.py's A/B lines and the tests; rqhip_rq_forward passes 0).
 * Every selection returns the same bits -- ids, embeddings, losses -- only the time differs:
 *   RQHIP_FWD_SCAN_FP32    distances on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, the oracle's FMA chain) even where
 *                          the filtered scan applies (D = 32 / 64, 16-byte aligned rows, no tie_margin): the default
 *                          there scans bf16-split scores on the bf16 matrix cores and re-decides exactly every row whose
 *                          two best scores are closer than the proven error bound (rqhip_filter_bound)
 *   RQHIP_FWD_SCAN_VALU    distances with packed fp32 FMAs on the vector ALU, codes broadcast from LDS, no matrix
 *                          instruction at all (D = 32, 16-byte aligned rows, K <= 1024, no tie_margin; otherwise
 *                          RQHIP_EUNSUPPORTED) -- the LDS/VALU form BASELINE.json's north_star asks the MFMA form to be
 *                          measured against
 *   RQHIP_FWD_NO_COOP_TAIL the partly filled last round of row tiles runs as ordinary tiles (A/B of the cooperative tail)
 */
#define RQHIP_FWD_SCAN_FP32 0x1u
#define RQHIP_FWD_SCAN_VALU 0x2u
#define RQHIP_FWD_NO_COOP_TAIL 0x10u
int rqhip_rq_forward_ex(const float *res0, int64_t B, int D, const float *codebooks, int L, int K,
                        int mode, float beta, int64_t *ids, float *embs, float *residuals,
                        float *emb_sum, float *loss, float *embs_norm, float *tie_margin, void *workspace,
                        size_t workspace_bytes, unsigned flags, rqhip_stream_t stream);
/* The filtered scan's too-close-to-call threshold, distance units: a row is re-decided exactly unless the gap between its
 * two smallest approximate distances exceeds  c1 * |x| * max_k|c_k| + c2 * (|x|^2 + max_k|c_k|^2).  Host-side accessor (no
 * GPU needed): tests/test_filter_bound.py checks the constants against the error bound derived in DESIGN.md section 4.1. */
void rqhip_filter_bound(float *c1, float *c2);             /* D = 32 */
void rqhip_filter_bound_d(int D, float *c1, float *c2);    /* per embedding width: D = 64 uses c1 = 2^-11 */
/* Test hook for that bound: scores[b,k] = the approximate score x_b.c_k - |c_k|^2/2 exactly as the filtered scan's
 * matrix-instruction chain produces it (same staging, same split, same instruction order), D = 32 / 64, x [B,D],
 * codebook [K,D], scores [B,K].  tests/test_gpu_filter_bound.py compares it with the real-arithmetic score on adversarial
 * operands: the hardware's accumulation error must stay inside the share of the bound assigned to it.
 * workspace: rqhip_rq_forward_workspace_bytes(1, K). */
int rqhip_filter_scores(const float *x, int64_t B, int D, const float *codebook, int K, float *scores,
                        void *workspace, size_t workspace_bytes, rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Residual quantisation, backward: what torch.autograd computes through the code above
 * (embedding backward + STE / rotation / eval branches + QuantizeLoss), in closed form.
 *
 *   upstream gradients (each may be NULL = zeros):
 *     g_embs [L,B,D] wrt embs, g_embsum [B,D] wrt emb_sum, g_resid [L,B,D] wrt residuals,
 *     g_loss [B] wrt loss
 *   outputs: g_res0 [B,D] (may be NULL; exact per-row arithmetic), g_codebooks [L,K,D] (may be NULL; OVERWRITTEN).
 *     For L <= 4 and either D <= 32 or (EVAL / STE, D % 4 == 0, D <= 64) -- rqhip_rq_backward_plan returns 1 -- the rows
 *     of a code are summed in a FIXED order: no atomics, bit-reproducible, restated by the oracle.  Other shapes scatter
 *     with LDS float atomics: the sum order is then not fixed and g_codebooks is reproducible to fp32 rounding only.
 *   workspace: rqhip_rq_backward_workspace_bytes(B,D,L,K) bytes
 */
size_t rqhip_rq_backward_workspace_bytes(int64_t B, int D, int L, int K);
/* 1 when a fixed-order kernel is used (tensors 16-byte aligned, as torch allocates them); then *n_wg, *units_per_wg
 * and *unit_rows give the geometry the summation order is a function of (workgroup b takes the unit_rows-row units
 * (round * units_per_wg + j) * n_wg + b in ascending order: oracle/rq_oracle.c:rqo_rq_backward_ordered) */
int rqhip_rq_backward_plan(int64_t B, int D, int L, int K, int mode, int *n_wg, int *units_per_wg, int *unit_rows);
int rqhip_rq_backward(const float *res0, int64_t B, int D, const float *codebooks, int L, int K,
                      int mode, float beta, const int64_t *ids, const float *g_embs,
                      const float *g_embsum, const float *g_resid, const float *g_loss,
                      float *g_res0, float *g_codebooks, void *workspace, size_t workspace_bytes,
                      rqhip_stream_t stream);
/* The same call with a kernel-selection flag (rqhip_rq_backward passes 0).  RQHIP_BWD_CBGRAD_MATRIX: where rqhip_rq_backward_matrix_form(D,
 * K, L, mode) says so (D = 32, STE, the training step's upstream gradients g_embsum + g_loss only; 3 x <= 256 or 3-4 x 1024 codes) the
 * codebook gradient is accumulated as a one-hot matrix product on the bf16 matrix cores (three exact bf16 pieces of every staged fp32
 * value; the sum's order is the matrix pipe's: reproducible run to run, not restatable by the oracle -- held to "no further from fp64
 * than the ordered kernel"); g_res0 has the same bits either way.  Other shapes ignore the flag. */
#define RQHIP_BWD_CBGRAD_MATRIX 0x1u
int rqhip_rq_backward_matrix_form(int D, int K, int L, int mode);
int rqhip_rq_backward_ex(const float *res0, int64_t B, int D, const float *codebooks, int L, int K, int mode, float beta,
                         const int64_t *ids, const float *g_embs, const float *g_embsum, const float *g_resid, const float *g_loss,
                         float *g_res0, float *g_codebooks, void *workspace, size_t workspace_bytes, unsigned flags,
                         rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * One Gumbel-softmax level, training mode.  Replaces quantize.py:112-117,128,131-136,157 and
 * distributions/gumbel.py:8-20.  The uniform noise U [B,K] is supplied by the caller (torch.rand on
 * the device), exactly where the reference draws it.
 *   outputs: ids [B] (argmin of the noise-free distance), emb [B,D] (= embeddings), loss [B]
 */
int rqhip_gumbel_forward(const float *x, int64_t B, int D, const float *codebook, int K,
                         const float *U, float temperature, float beta, int64_t *ids, float *emb,
                         float *loss, rqhip_stream_t stream);
/*   g_emb [B,D] / g_loss [B] upstream (may be NULL); outputs g_x [B,D], g_codebook [K,D] (overwritten).
 *   workspace: rqhip_gumbel_backward_workspace_bytes(B,D,K) */
size_t rqhip_gumbel_backward_workspace_bytes(int64_t B, int D, int K);
/* Both Gumbel entry points pick between two implementations with the same results: from `min_rows` rows (default 4096;
 * D = 32, K in {32, 64, 128, 256}, 16-byte aligned rows) the matrix-instruction kernels (32 rows per wave), below it the
 * one-row-per-wave kernels.  set_to > 0 changes the process-wide threshold (tests force the matrix path on small ragged
 * batches with 1); returns the previous value; set_to <= 0 only queries. */
int64_t rqhip_gumbel_matrix_path_min_rows(int64_t set_to);
int rqhip_gumbel_backward(const float *x, int64_t B, int D, const float *codebook, int K,
                          const float *U, float temperature, float beta, const float *g_emb,
                          const float *g_loss, float *g_x, float *g_codebook, void *workspace,
                          size_t workspace_bytes, rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * k-means codebook initialisation (init/kmeans.py).  The Lloyd loop, the np.random.choice seeding
 * and the torch.randint reseed of empty clusters stay on the host (they consume host RNG streams
 * the reference's results depend on); rqhip_kmeans_assign / _update are the two data-parallel steps of one
 * iteration, rqhip_kmeans_lloyd runs batches of iterations between two host visits.
 *
 * rqhip_kmeans_assign : kmeans.py:40-43  assign[i] = argmin_k sum_d (x[i,d]-c[k,d])^2
 * rqhip_kmeans_update : kmeans.py:44-59  c[k] <- mean of its rows (ascending-row sum / count);
 *                       empty clusters are left untouched, counts[k] == 0 reports them;
 *                       shift_sq_max (device scalar, may be NULL) <- max_k sum_d (c_new-c_old)^2,
 *                       i.e. the square of kmeans.py:68's torch.norm(...).max(), computed BEFORE any
 *                       host reseed (the host adds the reseeded rows' shift itself).
 */
int rqhip_kmeans_assign(const float *x, int64_t B, int D, const float *centroids, int K,
                        int64_t *assign, rqhip_stream_t stream);
int rqhip_kmeans_update(const float *x, int64_t B, int D, const int64_t *assign, int K,
                        float *centroids, int64_t *counts, float *shift_sq_max,
                        rqhip_stream_t stream);
/* rqhip_kmeans_lloyd : a BATCH of up to n_iters Lloyd iterations (kmeans.py:64-70) with no host round trip.
 *   Enqueues n_iters x (assign, update, finalize); each launch first reads state[0] and returns at once when an
 *   earlier iteration of the batch stopped the run.  state: 4 device ints, zero them before the first batch --
 *     state[0] stop flag: 0 running, 1 converged (sqrt of the max squared shift < stop_threshold, kmeans.py:68-69),
 *              2 an empty cluster appeared: its reseed draws from the host's torch RNG (kmeans.py:50-54), so the host
 *              reseeds (counts[k] == 0 names the clusters; their centroids are untouched), clears state[0] and goes on;
 *     state[1] iterations completed so far (the one that raised a flag included);
 *     state[2] fp32 bits of max_k |c_new - c_old|^2 of the last completed iteration (empty clusters excluded).
 *   centroids [K,D] updated in place, assign [B] / counts [K] hold the last completed iteration's values.
 *   The host reads the 16-byte state once per batch. */
int rqhip_kmeans_lloyd(const float *x, int64_t B, int D, float *centroids, int K, int64_t *assign,
                       int64_t *counts, int *state, int n_iters, float stop_threshold, rqhip_stream_t stream);
/* Row-sharded form of one iteration: every rank owns a block of rows,
 *   rqhip_kmeans_partial_sums : assign + this rank's per-cluster sums and counts -> sums [K, D+1] fp32 (count last);
 *   <caller all-reduces `sums` over the ranks: ONE collective of K (D+1) floats per iteration, RCCL on the stream>
 *   rqhip_kmeans_apply_sums   : means, shift, empty / convergence flags from the reduced sums (identical on every rank).
 * Same state words and early-exit rule as rqhip_kmeans_lloyd, so batches of iterations (collectives included) can be
 * enqueued between two host visits. */
int rqhip_kmeans_partial_sums(const float *x, int64_t B, int D, const float *centroids, int K, int64_t *assign,
                              float *sums, int *state, rqhip_stream_t stream);
int rqhip_kmeans_apply_sums(const float *sums, int K, int D, float *centroids, int64_t *counts, int *state,
                            float stop_threshold, rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Semantic-id statistics.
 * rqhip_dedup_rank: rank[i] = number of rows j < i whose L-tuple equals row i's -- the dedup column
 *   of SemanticIdTokenizer.precompute_corpus_ids (modules/tokenizer/semids.py:92-108).  Also yields
 *   n_distinct = number of rows with no LATER duplicate, i.e. B * p_unique_ids of rqvae.py:159-167.
 *   ids [L,B] int64 with 0 <= id < K; rank [B] int64 or NULL; n_distinct device int64 scalar or NULL.
 *   workspace: rqhip_dedup_workspace_bytes(B)
 */
size_t rqhip_dedup_workspace_bytes(int64_t B);
int rqhip_dedup_rank(const int64_t *ids, int64_t B, int L, int K, int64_t *rank,
                     int64_t *n_distinct, void *workspace, size_t workspace_bytes,
                     rqhip_stream_t stream);
/* p_unique_ids of RqVae.forward (modules/rqvae.py:159-167) as the reference returns it: *p_unique = float(n_distinct) / float(B), a device
 * fp32 scalar (torch: int64 tensor / int -> both to fp32, IEEE division); B >= 1; one fill + one kernel; workspace as rqhip_dedup_rank. */
int rqhip_unique_fraction(const int64_t *ids, int64_t B, int L, float *p_unique, void *workspace, size_t workspace_bytes,
                          rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Decoder-side consumers of semantic ids: exact integer tuple matching.
 *
 * Prefix index -- replaces EncoderDecoderRetrievalModel._check_valid_prefix (modules/model.py:169-182), the
 *   [N, P, h] equality tensor rebuilt at every beam step of generate() (model.py:349,364).
 *   corpus [N, H] int64, row stride ld elements (>= H): the model's `codebooks` buffer (model.py:75), i.e.
 *   tokenizer.cached_ids[:, :n_layers] (train_decoder.py:131).  Any int64 values are accepted.
 *   rqhip_prefix_index_build: fills `index` (rqhip_prefix_index_bytes(N, H) bytes, caller-owned, opaque) with
 *     the set of all prefixes of length 1..H of all corpus rows.  Build once per corpus.
 *   rqhip_prefix_lookup: valid[q] = 1 iff prefix[q, 0:h] equals corpus[n, 0:h] for some n; prefix [P, h]
 *     int64 with row stride ldp (>= h), 0 <= h <= H (h = 0: valid iff N > 0, as all()/any() give), valid [P]
 *     bytes (a torch.bool buffer).  `corpus`, N, H, ld must be the ones the index was built from: the index
 *     stores row numbers and every hit is confirmed against the corpus row itself.
 * Top-k match -- the array step of TopKAccumulator.accumulate (evaluate/metrics.py:16-25):
 *   rank[b] = the first k with top_k[b, k, :] == actual[b, :], or -1; actual [B, D], top_k [B, K, D], dense.
 */
#define RQHIP_MAX_PREFIX_LEN 16
size_t rqhip_prefix_index_bytes(int64_t N, int H);
int rqhip_prefix_index_build(const int64_t *corpus, int64_t N, int H, int64_t ld, void *index,
                             size_t index_bytes, rqhip_stream_t stream);
int rqhip_prefix_lookup(const void *index, size_t index_bytes, const int64_t *corpus, int64_t N, int H,
                        int64_t ld, const int64_t *prefix, int64_t P, int h, int64_t ldp, uint8_t *valid,
                        rqhip_stream_t stream);
int rqhip_topk_first_match(const int64_t *actual, const int64_t *top_k, int64_t B, int K, int D,
                           int64_t *rank, rqhip_stream_t stream);

/* Item index -- from semantic-id tuples to corpus item numbers (csrc/sid_items.hip): the inverse of
 * SemanticIdTokenizer._lookup (modules/tokenizer/semids.py).  Several items share a tuple; the tokenizer tells them
 * apart by the dedup column, which the decoder never generates.
 *   corpus [N, >= L] int64 with row stride ld (>= L) and rank [N] int64, the dedup column: rank[i] = the number of rows
 *   j < i with row i's L-tuple (rqhip_dedup_rank), so that rows are unique in (tuple, rank) and, within a tuple,
 *   ascending rank is ascending item number.
 *   rqhip_sid_item_index_build: fills `index` (rqhip_sid_item_index_bytes(N) bytes -- 0 for N < 0 --, caller-owned,
 *     opaque, 12 to 20 bytes per item) with the exact map (L-tuple, rank) -> item number.  Build once per corpus; one
 *     fill and one kernel.  `rank` is copied into the index and not needed afterwards; `corpus`, N, L, ld must be the
 *     same in every later call: the index stores row numbers, and membership is always decided by comparing the stored
 *     row's ids and rank with the query, never by a hash alone.  Where a row sits in the index may differ from build to
 *     build; no answer does.
 *   rqhip_sid_item_lookup: items[p] = the item with tuple ids[p, 0:L] and rank ids[p, L], or -1 when no corpus row has
 *     that tuple and rank; ids [P, L + 1] int64 with row stride ld_ids (>= L + 1) -- a row of tokenizer.cached_ids, or of
 *     batch.sem_ids_fut.  One thread per query.  P = 0 returns RQHIP_OK without a launch.
 *   rqhip_sid_items_topn: the beams of `generate` expanded to the items a recommender returns, ONE launch, no fill, no
 *     atomics.  beams [B, k, L] int64 and scores [B, k] fp32, dense, best beam first; history NULL, or [B, T * (L + 1)]
 *     int64 with row stride ld_hist (>= T * (L + 1)) in the form of batch.sem_ids (a history item with any negative id,
 *     its rank included, is padding); items [B, n] int64 and item_scores [B, n] fp32, dense.  For user u:
 *         out = []
 *         for b in 0 .. k-1:                               -- best beam first
 *             if not (scores[u,b] > -inf): continue        -- -inf and NaN beams contribute nothing
 *             if beams[u,b] == beams[u,b'] for an earlier contributing b' < b: continue
 *             for r in 0, 1, 2, ...:                       -- ascending dedup rank = ascending item number
 *                 item = map.get((beams[u,b], r));  if item is None: break
 *                 if history and (beams[u,b], r) is one of u's non-padding history items: continue
 *                 out.append((item, scores[u,b]));  if len(out) == n: stop
 *         items[u] = out padded with -1;  item_scores[u] = the beams' scores (their bits), padded with -inf
 *     Every element of both outputs is written by the call.  One wave per user, lane b owns beam b.  Probe bound: a lane
 *     walks its tuple's ranks at most twice (count, then write), and each probe of a walk either emits an item, hits a
 *     distinct history item of the user, or ends the group -- at most n + (distinct history items) + 1 probes per walk.
 *     The same bits on every run, and on an index built a second time from the same corpus.
 * Limits: 1 <= L and L + 1 <= RQHIP_MAX_PREFIX_LEN, N < 2^30, ld >= L; for rqhip_sid_items_topn also 1 <= k <= 64,
 * 1 <= n <= 256, T >= 0, B < 2^31 (B = 0 returns RQHIP_OK without a launch).  Outside them RQHIP_EARG /
 * RQHIP_EUNSUPPORTED, and RQHIP_EWORKSPACE for an index buffer that is too small, with the limit named in
 * rqhip_last_error(); every argument check runs before any HIP call.  No allocation, copy or sync (graph-capturable). */
size_t rqhip_sid_item_index_bytes(int64_t N);
int rqhip_sid_item_index_build(const int64_t *corpus, int64_t N, int L, int64_t ld, const int64_t *rank, void *index,
                               size_t index_bytes, rqhip_stream_t stream);
int rqhip_sid_item_lookup(const void *index, size_t index_bytes, const int64_t *corpus, int64_t N, int L, int64_t ld,
                          const int64_t *ids, int64_t P, int64_t ld_ids, int64_t *items, rqhip_stream_t stream);
int rqhip_sid_items_topn(const void *index, size_t index_bytes, const int64_t *corpus, int64_t N, int L, int64_t ld,
                         const int64_t *beams, const float *scores, int64_t B, int k, const int64_t *history, int64_t T,
                         int64_t ld_hist, int n, int64_t *items, float *item_scores, rqhip_stream_t stream);

/* Beam step -- one hierarchy step of EncoderDecoderRetrievalModel.generate (modules/model.py) in one launch: softmax,
 * sampling without replacement, log, prefix validity, masked_fill, sort and gathers.  Row r of the B * beams_in rows
 * (beams_in = 1 at h = 0, else the k beams of the previous step; row b * beams_in + beam):
 *   p = softmax(logits[r]) (fp32, row max subtracted); samples[r, 0..n) = indices of the n largest p[c] / noise[r, c]
 *   in descending order, equal keys to the lower code (ATen's multinomial(p, n, replacement=False) with its Exp(1) draw
 *   q passed as `noise` [B * beams_in, K], dense); lp = logf(p[sample]).
 *   Candidate j = beam * n + s of user b: score = lp + parent_scores[b, beam] (lp alone at h = 0), or -inf unless
 *   parent_ids[b, beam, 0:h] ++ sample is a prefix of some corpus row (the exact test of rqhip_prefix_lookup against an
 *   index built by rqhip_prefix_index_build from corpus / N / H / ld).
 *   Per user the k best candidates, descending, equal scores (-inf included) to the lower j:
 *   out_ids [B, k, h+1] = parent ids ++ sample, out_scores [B, k], out_parent [B, k] = b * beams_in + beam.
 * logits [B * beams_in, K] with row stride ld_logits; parent_scores [B, beams_in] and parent_ids [B, beams_in, h]
 * dense (NULL at h = 0).  Limits: K <= 4096, n_cands <= min(64, K), k <= 64 and k <= beams_in * n_cands,
 * beams_in <= 64, h + 1 <= min(H, RQHIP_MAX_PREFIX_LEN); outside them RQHIP_EUNSUPPORTED / RQHIP_EARG with the limit
 * named in rqhip_last_error().  Deterministic; no allocation, copy or sync (graph-capturable). */
size_t rqhip_beam_step_workspace_bytes(int64_t B, int beams_in, int K, int n_cands, int k);
int rqhip_beam_step(const float *logits, int64_t ld_logits, const float *noise, const float *parent_scores,
                    const int64_t *parent_ids, int h, int64_t B, int beams_in, int K, int n_cands, int k,
                    const void *index, size_t index_bytes, const int64_t *corpus, int64_t N, int H, int64_t ld,
                    int64_t *out_ids, float *out_scores, int64_t *out_parent, void *workspace, size_t workspace_bytes,
                    rqhip_stream_t stream);

/* Exact beam step -- one hierarchy step of the deterministic constrained beam search (model.beam_impl = "exact") in one
 * launch (csrc/beam_step.hip): every corpus-valid child of every kept beam is scored, no random numbers.  Arguments as
 * rqhip_beam_step without `noise`, `n_cands` and the workspace.  Row r = b * beams_in + beam of the B * beams_in rows:
 *   m = max_c x[c], s = sum_c expf(x[c] - m), lp[c] = (x[c] - m) - logf(s): the log-softmax form, which (unlike the
 *   sampling step's logf(p)) does not underflow to -inf for an unlikely code.  fp32 throughout, fixed reduction order.
 *   Candidate j = beam * K + c of user b: score = lp[c] + parent_scores[b, beam] (lp[c] alone at h = 0), or -inf unless
 *   parent_ids[b, beam, 0:h] ++ c is a prefix of some corpus row (the exact test of rqhip_prefix_lookup, confirmed
 *   against the corpus row).  A NaN score counts as -inf.
 *   Per user the k best candidates, descending, equal scores (-inf included) to the lower j -- the stable descending
 *   sort of the [beams_in * K] score row, so the whole output is determined, the -inf beams included:
 *   out_ids [B, k, h+1] = parent ids ++ code, out_scores [B, k], out_parent [B, k] = b * beams_in + beam.
 *   A -inf beam in the output means that fewer than k corpus prefixes of length h + 1 extend the user's finite beams.
 * Limits: K <= 4096, k <= 64, beams_in <= 64, k <= beams_in * K, beams_in = 1 at h = 0,
 * h + 1 <= min(H, RQHIP_MAX_PREFIX_LEN); outside them RQHIP_EUNSUPPORTED / RQHIP_EARG with the limit named in
 * rqhip_last_error(); every argument check runs before any HIP call.  The same bits on every run; no atomics,
 * allocation, copy or sync (graph-capturable). */
int rqhip_beam_topk_step(const float *logits, int64_t ld_logits, const float *parent_scores, const int64_t *parent_ids,
                         int h, int64_t B, int beams_in, int K, int k, const void *index, size_t index_bytes,
                         const int64_t *corpus, int64_t N, int H, int64_t ld, int64_t *out_ids, float *out_scores,
                         int64_t *out_parent, rqhip_stream_t stream);

/* T5 attention for inference (modules/t5.py:_attend) in one launch, fp32 throughout (csrc/t5_attention.hip):
 *   out[r, i, h*64 : h*64+64] = softmax_j(q[r, i, h] . k[b, j, h] + bias + mask) . v[b, :, h]      b = r / (R / Rk)
 * with T5's semantics: no 1/sqrt(d) scaling, d_kv = 64, masked scores get finfo(float32).min ADDED (a row with every key
 * masked is the uniform average of V).  Token (r, i) of q / out is row r * Tq + i with row stride ld_q / ld_out (elements),
 * head h at columns h*64 ..: the q Linear's output and the o Linear's input as they are, no transposes.
 *   K/V, dense (anc NULL): token (b, j) of k / v is row b * Tk + j with row stride ld_kv; the R / Rk query rows
 *     b * (R / Rk) .. read group b (the beams of a user in cross-attention), whose K/V are staged once per (b, h).
 *   K/V, cached decode step (anc [R, ld_anc] int32, Tq = 1, Rk = R, Tk = past + 1): k / v are per-position slabs, row
 *     t * slab_rows + x with row stride ld_kv; key t < past of row r is slab row x = anc[r * ld_anc + t], key `past` is
 *     the row's own x = r.  No cache tensor is copied.
 *   bias_by_delta [n_delta, H] (or NULL): table[(j - i - past) + bias_offset][h] is added; the caller gathers it from
 *     the relative-position embedding, the kernel computes no bucket.
 *   key_mask [Rk, Tk] bytes (or NULL; 0 = masked); causal != 0 keeps j <= i + past.
 * Limits (rqhip_t5_attention_supported): d_kv = 64, 1 <= Tq, Tk <= 256, any H >= 1; else RQHIP_EUNSUPPORTED.  Pointers
 * 16-byte aligned, strides multiples of 4.  Deterministic; no allocation, copy or sync (graph-capturable). */
int rqhip_t5_attention_supported(int d_kv, int H, int Tq, int Tk);
int rqhip_t5_attention(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R, int64_t Rk,
                       int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta, int bias_offset,
                       const uint8_t *key_mask, int causal, int past, const int32_t *anc, int64_t ld_anc,
                       int64_t slab_rows, float *out, int64_t ld_out, rqhip_stream_t stream);

/* The same attention for training (csrc/t5_attention.hip): a forward that also writes the row log-sum-exp and applies the
 * attention-weight dropout, and the backward.  Dense K/V with one K/V per query row only (Rk = R, else
 * RQHIP_EUNSUPPORTED), no `past`; q, k, v, bias_by_delta, bias_offset, key_mask and causal as above.
 *   Dropout (0 <= p < 1): weight (r, h, i, j) is kept iff hash(seed, ((r * H + h) * Tq + i) * Tk + j) >= round(p * 2^32)
 *     and kept weights are scaled by 1 / (1 - p), AFTER the softmax's normalisation.  The scale is computed in fp32, as
 *     1.0f / (1.0f - (float)p), in the forward and in the backward: at some p (0.15, 0.6, 0.8, 0.9; not 0.1 or 0.5) its
 *     last bits differ from the (float)(1 / (1 - p)) evaluated in double of rqhip_t5_add_norm_* and rqhip_t5_ffn_* below.
 *     With x = the index, s = *seed and fmix = murmur3's 32-bit finaliser:
 *     hash = fmix((fmix(lo(s) ^ lo(x)) ^ hi(s) ^ hi(x) * 0x85EBCA6B) + 0x9E3779B9).
 *     `seed` points to ONE int64 on the device (NULL allowed at p = 0); the host never reads it.  The forward and both
 *     passes of the backward recompute the decision; no mask is stored (rqhip/ops.py:t5_attention_dropout_keep restates
 *     it in torch).
 *   rqhip_t5_attention_fwd_train: out as rqhip_t5_attention (bit for bit at p = 0) and lse [R, H, Tq] = max + log(sum)
 *     of each row's scores.
 *   rqhip_t5_attention_bwd: from d_out (row stride ld_do) writes d_q [R, Tq, H * 64], d_k and d_v [R, Tk, H * 64] (dense)
 *     and, with a bias table, d_bias_by_delta [n_delta, H] (zero outside the deltas -(Tq - 1) .. Tk - 1 of the call)
 *     through the scratch d_bias_partial [R * H, Tq + Tk - 1].  P is recomputed: dP = (dO V^T) o M / (1 - p),
 *     D_i = dO_i . O_i, dS = P o (dP - D), dQ = dS K, dK = dS^T Q, dV = (P o M / (1 - p))^T dO, with no special case for
 *     masked keys; nothing of size Tq x Tk is stored.  Two of the saved tensors are recomputed rather than read, for
 *     accuracy.  Each row's max and sum come from q and k with the forward's bits, not from lse, which cannot carry
 *     log(sum) beside max = -FLT_MAX (a row with every key masked keeps its uniform P and non-zero dS, as with the
 *     operators).  D is evaluated as sum_j P_ij dP_ij, the same number as dO_i . O_i, from the very dP it is subtracted
 *     from: the rounding of the 64-term products cancels in dP - D as in the operators' softmax backward, and a row
 *     with one live key has dS = 0 exactly.  out and lse stay part of the call (what autograd saves) and must be
 *     non-NULL.
 * Limits (rqhip_t5_attention_bwd_supported, both functions): d_kv = 64, 1 <= Tq, Tk <= 256, any H >= 1, Tq <= Tk with
 * a bias table or causal.  No float atomics, fixed reduction orders: the same bits on every run; no allocation, copy
 * or sync. */
int rqhip_t5_attention_bwd_supported(int d_kv, int H, int Tq, int Tk);
int rqhip_t5_attention_fwd_train(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R,
                                 int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta,
                                 int bias_offset, const uint8_t *key_mask, int causal, double p, const int64_t *seed,
                                 float *out, int64_t ld_out, float *lse, rqhip_stream_t stream);
int rqhip_t5_attention_bwd(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, const float *out,
                           int64_t ld_out, const float *lse, const float *d_out, int64_t ld_do, int64_t R, int64_t Rk,
                           int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta, int bias_offset,
                           const uint8_t *key_mask, int causal, double p, const int64_t *seed, float *d_q, float *d_k,
                           float *d_v, float *d_bias_by_delta, float *d_bias_partial, rqhip_stream_t stream);

/* The same three calls on PACKED variable-length rows (csrc/t5_attention.hip, the same kernel bodies): R groups, one
 * K/V per group, whose tokens lie in 2-D tensors without padding.  cu_q and cu_k are int32 [R + 1] cumulative row
 * tables on the device, either of which may be NULL (not both):
 *   with cu_k the keys of group b are rows cu_k[b] .. cu_k[b + 1] - 1 of k, v [n_k, H * 64] (row stride ld_kv) and of
 *     d_k, d_v (dense); with cu_q the same holds for q, out, d_out [n_q, H * 64] (their strides) and d_q (dense);
 *   NULL is the dense layout above for that side (row b * T + t; n_q = R * Tq, n_k = R * Tk): the cross-attention is
 *     dense decoder queries over packed K/V.
 * Tq and Tk are the padded lengths, upper BOUNDS of every group's own: they keep the bias index (j - i), the dropout
 * element index ((b * H + h) * Tq + i) * Tk + j, the kernel instantiation and the LDS layout of the padded call, and a
 * group's own lengths give its loops, its row bases and the K/V rows it stages.  A table entry is clamped to [0, n] and a
 * length to its bound: a bad table gives an empty or a short group, never an address.  Every packed key is valid:
 * key_mask must be NULL and causal 0 (RQHIP_EARG otherwise; both stay in the signature to say so), beams = 1, no `past`.
 *   lse: [n_q, H] with cu_q (a token's heads side by side), [R, H, Tq] without.
 *   d_bias_partial: [R * H, Tq + Tk - 1] as above.
 *   A group without keys gives out = 0, lse = -inf and d_q = 0; one without queries gives d_k = d_v = 0.
 * On every valid (group, head, query, key) out, lse, d_q, d_k, d_v and the rows of d_bias_partial have the BITS of the
 * padded call on the scattered tensors with the prefix key mask (and d_out = 0 on the padded query rows): a masked
 * key's weight is exactly 0 there, its dS and its share of every sum too, and a skipped key tile is a sum of zeros that
 * is not added.  Limits: those of rqhip_t5_attention_bwd_supported on the bounds; n_q, n_k < 2^31. */
int rqhip_t5_attention_packed_supported(int d_kv, int H, int Tq, int Tk);
int rqhip_t5_attention_packed(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R,
                              int64_t n_q, int64_t n_k, int H, int d_kv, int Tq, int Tk, const int32_t *cu_q,
                              const int32_t *cu_k, const float *bias_by_delta, int n_delta, int bias_offset,
                              const uint8_t *key_mask, int causal, float *out, int64_t ld_out, rqhip_stream_t stream);
int rqhip_t5_attention_packed_fwd_train(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                        int64_t R, int64_t n_q, int64_t n_k, int H, int d_kv, int Tq, int Tk,
                                        const int32_t *cu_q, const int32_t *cu_k, const float *bias_by_delta,
                                        int n_delta, int bias_offset, const uint8_t *key_mask, int causal, double p,
                                        const int64_t *seed, float *out, int64_t ld_out, float *lse,
                                        rqhip_stream_t stream);
int rqhip_t5_attention_packed_bwd(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                  const float *out, int64_t ld_out, const float *lse, const float *d_out, int64_t ld_do,
                                  int64_t R, int64_t n_q, int64_t n_k, int H, int d_kv, int Tq, int Tk,
                                  const int32_t *cu_q, const int32_t *cu_k, const float *bias_by_delta, int n_delta,
                                  int bias_offset, const uint8_t *key_mask, int causal, double p, const int64_t *seed,
                                  float *d_q, float *d_k, float *d_v, float *d_bias_by_delta, float *d_bias_partial,
                                  rqhip_stream_t stream);

/* The cross-attention of a cached decode step over PACKED encoder rows (csrc/t5_attention.hip, the same kernel body),
 * inference only, ONE launch: the groups of beams of rqhip_t5_attention over the packed K/V of
 * rqhip_t5_attention_packed.  q and out are dense [R, Tq, H * 64] with R = Rk * beams: query rows b * beams ..
 * b * beams + beams - 1 read group b, whose keys are rows cu_k[b] .. cu_k[b + 1] - 1 of k, v [n_k, H * 64] (row stride
 * ld_kv), staged once per (group, head) with the group's own length.  cu_k: int32 [Rk + 1] on the device, required, and
 * clamped as above (a bad table gives a short group, never an address); Tk is the padded bound of every group.  No bias
 * table, key mask, causal flag, `past` or ancestor table: a cross-attention has none.
 *   The kernel instantiation, launch plan and LDS layout are those of the padded call, chosen by the bounds (Tq, Tk).
 *   With beams = 1 (Rk = R) out has the bits of rqhip_t5_attention_packed(cu_q = NULL); on every query it has the bits of
 *   rqhip_t5_attention on the scattered K/V [Rk, Tk, H * 64] with the prefix key mask and Rk groups.  A group without
 *   keys gives out = 0 on its beams' rows.
 * Limits: those of rqhip_t5_attention_packed_supported on (Tq, Tk); R % Rk == 0; beams * Tq < 2^24; 0 <= n_k <= Rk * Tk
 * and n_k < 2^31; pointers 16-byte aligned, strides multiples of 4 and >= H * 64.  Outside them RQHIP_EARG /
 * RQHIP_EUNSUPPORTED with the argument named, before any HIP call.  Deterministic; no allocation, copy, memset or sync.
 * There is no training pair: under grad a cross-attention has beams = 1 and takes rqhip_t5_attention_packed_fwd_train. */
int rqhip_t5_attention_packed_beams(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                    int64_t R, int64_t Rk, int64_t n_k, int H, int d_kv, int Tq, int Tk,
                                    const int32_t *cu_k, float *out, int64_t ld_out, rqhip_stream_t stream);

/* Between padded [B, T, d] rows and packed [N, d] rows (csrc/rows_pack.hip), fp32, d a multiple of 4
 * (rqhip_rows_pack_supported), 16-byte accesses.  cu: int32 [B + 1] on the device, clamped as above.
 *   rqhip_rows_pack: out[cu[b] + t] = x[b, t] for t < cu[b + 1] - cu[b]; rows of out no group covers are not written.
 *   rqhip_rows_unpack: out[b, t] = x[cu[b] + t] for those t and 0 for the padded tail, in the same launch.
 * Exact copies; each is the other's backward.  No allocation, copy or sync. */
int rqhip_rows_pack_supported(int d);
int rqhip_rows_pack(const float *x, const int32_t *cu, int64_t B, int T, int d, int64_t N, float *out,
                    rqhip_stream_t stream);
int rqhip_rows_unpack(const float *x, const int32_t *cu, int64_t B, int T, int d, int64_t N, float *out,
                      rqhip_stream_t stream);

/* The same attention beyond 256 tokens (csrc/t5_attention_long.hip): inference, training forward and backward for
 * 1 <= Tq, Tk <= 2048 (rqhip_t5_attention_long_supported: d_kv = 64, any H >= 1; shorter lengths are accepted too).  The
 * mathematics, the T5 semantics, q / k / v / out, bias_by_delta, bias_offset, key_mask, causal, the K/V groups (R / Rk
 * query rows read group b) and the dropout decision are those of rqhip_t5_attention* above; the bits are not, because the
 * keys are walked in chunks of RQHIP_T5_ATTENTION_LONG_CHUNK with an online softmax, by workgroups of
 * RQHIP_T5_ATTENTION_LONG_QBLOCK query rows that never hold more than one chunk of K/V in LDS.  Dense K/V only: past must
 * be 0 and anc NULL (else RQHIP_EUNSUPPORTED; the cached decode step never has more keys than levels and stays on
 * rqhip_t5_attention).
 *   Forward, per query row and per chunk of keys, ascending, from m = -inf, l = 0, o = 0:
 *     s_j = q . k_j + bias (+ finfo(float32).min when masked);  m' = max(m, max_j s_j);  alpha = expf(m - m');
 *     p_j = expf(s_j - m');  l = l * alpha + sum_j p_j;  p_j = 0 where the dropout drops (i, j);
 *     o = o * alpha + sum_j p_j v_j (the chunk's sum formed from zero, keys ascending);  m = m'
 *   and out = o / l behind the last chunk.  A score (and, in the backward, a dP) is four chains of sixteen products
 *   each, features ascending, added as (c0 + c1) + (c2 + c3): shorter chains round less where scores reach 40, and the
 *   backward's scores have the forward's bits.  The backward likewise forms each chunk's share of d_q, d_k and d_v from
 *   zero and adds the chunks in ascending order.  The dropout mask is applied to the UNNORMALISED chunk weights while l
 *   accumulates every weight, dropped or not; the scale 1.0f / (1.0f - (float)p) multiplies out = o / l once, at the end
 *   (training forward only).  No chunk is skipped under `causal`: a row with every key masked is the uniform average of
 *   ALL Tk rows of V, as with the operators.
 *   rqhip_t5_attention_long_fwd_train (Rk = R): out, lse [R, H, Tq] = m + log(l), and ml [R, H, Tq, 2] = the pair
 *     (m, l), which the backward reads: lse cannot carry log(l) beside m = -FLT_MAX.
 *   rqhip_t5_attention_long_bwd (Rk = R): d_q [R, Tq, H * 64], d_k, d_v [R, Tk, H * 64] (dense) and, with a bias table,
 *     d_bias_by_delta [n_delta, H] (zero outside the deltas of the call).  P_ij = expf(s_ij - m_i) / l_i is recomputed;
 *     dP, dS, dQ, dK, dV as in rqhip_t5_attention_bwd.  D_i is sum_j P_ij dP_ij from a first loop over the keys, not
 *     dO_i . O_i: it is made of the very dP it is subtracted from, so a row with one live key (P = 1, the others exactly
 *     0) has D = dP and dS = 0 exactly, and the rounding of the 64-term products cancels in dP - D.  out and lse stay part
 *     of the call (what autograd saves) and must be non-NULL.  A query-major launch writes d_q, D and per-workgroup sums
 *     of dS along the diagonals j - i, a key-major launch d_k and d_v, a small launch adds the diagonal sums in ascending
 *     (row, workgroup) order.  Nothing of size Tq x Tk is stored: `workspace` (16-byte aligned,
 *     rqhip_t5_attention_long_bwd_workspace_bytes(R, H, Tq, Tk) bytes, which grow with R * H * (Tq + Tk)) holds D and at
 *     most four diagonal rows per (row, head).
 * Tq <= Tk with a bias table or causal.  Pointers 16-byte aligned, strides multiples of 4; every argument check precedes
 * the first HIP call.  No float atomics, fixed reduction orders: the same bits on every run, and a row's bits depend on
 * Tq, Tk and that row's data only (not on R, the beams or the grid).  No allocation, copy, memset or sync. */
#define RQHIP_T5_ATTENTION_LONG_CHUNK 128   /* keys per chunk */
#define RQHIP_T5_ATTENTION_LONG_QBLOCK 64   /* query rows per workgroup */
int rqhip_t5_attention_long_supported(int d_kv, int H, int Tq, int Tk);
int rqhip_t5_attention_long(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R,
                            int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta,
                            int bias_offset, const uint8_t *key_mask, int causal, int past, const int32_t *anc, float *out,
                            int64_t ld_out, rqhip_stream_t stream);
int rqhip_t5_attention_long_fwd_train(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                      int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta,
                                      int n_delta, int bias_offset, const uint8_t *key_mask, int causal, double p,
                                      const int64_t *seed, float *out, int64_t ld_out, float *lse, float *ml,
                                      rqhip_stream_t stream);
size_t rqhip_t5_attention_long_bwd_workspace_bytes(int64_t R, int H, int Tq, int Tk);
int rqhip_t5_attention_long_bwd(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                const float *out, int64_t ld_out, const float *lse, const float *ml, const float *d_out,
                                int64_t ld_do, int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk,
                                const float *bias_by_delta, int n_delta, int bias_offset, const uint8_t *key_mask,
                                int causal, double p, const int64_t *seed, float *d_q, float *d_k, float *d_v,
                                float *d_bias_by_delta, void *workspace, size_t workspace_bytes, rqhip_stream_t stream);

/* The "bf16" arithmetic of the same three calls (modules/t5.py, attention_arith = "bf16"): the parameter lists, shapes,
 * limits, strides, K/V groups and beams, argument checks (the messages carry these names), launch counts, workspace
 * layout and size (rqhip_t5_attention_long_supported and rqhip_t5_attention_long_bwd_workspace_bytes serve both arms) and
 * graph capturability of their fp32 twins above; the chunk and the query block are RQHIP_T5_ATTENTION_LONG_CHUNK and
 * RQHIP_T5_ATTENTION_LONG_QBLOCK.  Storage stays fp32 everywhere: q, k, v, out, lse, (m, l), d_out, d_q, d_k, d_v, the
 * bias table and its gradient, and the workspace.  The mask and bias semantics and the dropout decision (the same
 * element index) are unchanged.  Arithmetic contract ("bf16"), in the terms of rqhip_t5_ffn_*_bf16 below:
 *   - Every operand of a matrix instruction is the round-to-nearest-even bf16 rounding of the fp32 value the fp32 arm
 *     feeds at that place.  Forward: q, k, v and the unnormalised chunk weights p_j, rounded AFTER the dropout zeroing.
 *     Backward: q, k, v, d_out, the dropped and scaled P (P o M / (1 - p)) that multiplies d_out for d_v, and dS for d_q
 *     and d_k.
 *   - Products are exact and accumulate in fp32 inside v_mfma_f32_16x16x32_bf16.  A score and a dP are ONE chain of two
 *     instructions (features 0 .. 31, then 32 .. 63) from +0; a chunk's share of o, d_q, d_k and d_v is one chain from
 *     +0 over the chunk's groups of 32 keys (queries for d_k, d_v) in ascending order, and the chunks are added in
 *     ascending order as in the fp32 arm.  The order of the 32 terms inside an instruction is the instruction's.  A last
 *     half group (an odd number of 16-row tiles) multiplies zeros.
 *   - In fp32 on the UNROUNDED values: bias add, mask add, running max, expf, the row sum l (every weight, dropped or
 *     not), alpha, o * alpha + chunk, the final divide, 1 / (1 - p), lse, (m, l), D = sum P dP, dS = P (dP - D) and the
 *     diagonal sums for the table gradient (dS is not rounded on that path).
 *   - The forward and the three backward passes form a score with one shared function, so the backward's scores have
 *     the forward's bits.  D is made of the very dP it is subtracted from: a row with one live key gives dS = 0 exactly.
 *     Under `causal` the first query of a live row returns the bf16 rounding of its first V row exactly.
 *   - The (m, l) pair (and lse) of a bf16 forward belong to bf16 scores: only the bf16 backward may read them.
 *   - No float atomics, fixed orders: the same bits on every run; a row's bits depend on Tq, Tk and that row's data
 *     only, not on R, the beams or the grid.  No allocation, copy, memset or sync.
 * Error against the fp64 attention on the bf16-rounded q, k, v, d_out, beyond the fp32 arm's own N on those tensors and
 * with u = 2^-8: out u (P~ |v|), d_v u (P~^T |d_out|), d_q u (|dS| |k|), d_k u (|dS|^T |q|), where P~ = P o M / (1 - p)
 * (tests/test_gpu_t5_attention_long_bf16.py; measured ratios in profiles/t5_attention_long_bf16.txt). */
int rqhip_t5_attention_long_bf16(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv, int64_t R,
                                 int64_t Rk, int H, int d_kv, int Tq, int Tk, const float *bias_by_delta, int n_delta,
                                 int bias_offset, const uint8_t *key_mask, int causal, int past, const int32_t *anc,
                                 float *out, int64_t ld_out, rqhip_stream_t stream);
int rqhip_t5_attention_long_fwd_train_bf16(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                           int64_t R, int64_t Rk, int H, int d_kv, int Tq, int Tk,
                                           const float *bias_by_delta, int n_delta, int bias_offset,
                                           const uint8_t *key_mask, int causal, double p, const int64_t *seed, float *out,
                                           int64_t ld_out, float *lse, float *ml, rqhip_stream_t stream);
int rqhip_t5_attention_long_bwd_bf16(const float *q, int64_t ld_q, const float *k, const float *v, int64_t ld_kv,
                                     const float *out, int64_t ld_out, const float *lse, const float *ml,
                                     const float *d_out, int64_t ld_do, int64_t R, int64_t Rk, int H, int d_kv, int Tq,
                                     int Tk, const float *bias_by_delta, int n_delta, int bias_offset,
                                     const uint8_t *key_mask, int causal, double p, const int64_t *seed, float *d_q,
                                     float *d_k, float *d_v, float *d_bias_by_delta, void *workspace,
                                     size_t workspace_bytes, rqhip_stream_t stream);

/* "Add-norm": the glue between two T5 sub-layers in one launch (csrc/t5_add_norm.hip; modules/t5.py, norm_impl = "hip"):
 * the dropout of a sub-layer's output y, the residual add, the NEXT RMS norm and, behind a stack's final norm, its
 * dropout.  x (the residual stream, or NULL), y, x_new, n are dense [N, d] fp32, w [d], rstd [N]; all arithmetic is fp32
 * without contraction.  With e = row * d + col and `hash`, `seed` as in rqhip_t5_attention_fwd_train above:
 *   keep_in(e) = hash(seed, e) >= round(p_in * 2^32)     keep_out(e) = hash(seed, N * d + e) >= round(p_out * 2^32)
 *   s_in = (float)(1 / (1 - p_in)), s_out = (float)(1 / (1 - p_out)), evaluated in double and rounded once
 *   t     = y at p_in = 0, else keep_in ? y * s_in : +0          x_new = t without x, else x + t
 *   rstd  = 1 / sqrt(sum_c x_new[c]^2 / d + eps)                 (IEEE divide and square root)
 *   n     = w * (x_new * rstd), then at p_out > 0: keep_out ? n * s_out : +0
 * (rqhip/ops.py:t5_attention_dropout_keep(seed, 2, 1, N, d, p) restates both masks: plane 0 keep_in, plane 1 keep_out.)
 * A row sum adds each lane's elements (columns 4 l .. 4 l + 3, then + 256, + 512, + 768 of lane l) in ascending order and
 * then the 64 lanes in an xor butterfly: the order is a function of d alone, so a row's bits depend neither on N nor on
 * the row's position.
 *   rqhip_t5_add_norm_bwd, from d_n and d_xnew (either may be NULL = zero):
 *     g = d_n * (keep_out ? s_out : 0), gw = g * w, xh = x_new * rstd, c = (sum_c gw * xh) / d,
 *     d_res = d_xnew + rstd * (gw - xh * c); d_x = d_res; d_y = d_res at p_in = 0, else keep_in ? d_res * s_in : 0;
 *     d_w[c] = sum over the rows of g * xh.  d_x or d_y NULL: that gradient is not wanted.
 *   d_w without float atomics: each workgroup owns a contiguous range of rows (64 up to N = 16384, then the smallest
 *   64 * 2^k that needs at most 256 workgroups: a function of N alone), writes one partial [d] block into `workspace`
 *   (rqhip_t5_add_norm_bwd_workspace_bytes(N, d) bytes), and a second kernel of the same call adds the blocks in
 *   ascending order.  At N = 0 d_w (when not NULL) is set to zero.
 * Limits (rqhip_t5_add_norm_supported): d a multiple of 4, 4 <= d <= 1024, else RQHIP_EUNSUPPORTED; x, y, w, x_new, n and
 * the gradients 16-byte aligned; 0 <= p < 1; seed may be NULL when both probabilities are 0.  Same bits on every run and
 * device; no allocation, copy or sync (graph-capturable). */
int rqhip_t5_add_norm_supported(int d);
size_t rqhip_t5_add_norm_bwd_workspace_bytes(int64_t N, int d);
int rqhip_t5_add_norm_fwd(const float *x, const float *y, const float *w, int64_t N, int d, float eps, double p_in,
                          double p_out, const int64_t *seed, float *x_new, float *n, float *rstd, rqhip_stream_t stream);
int rqhip_t5_add_norm_bwd(const float *x_new, const float *rstd, const float *w, const float *d_n, const float *d_xnew,
                          int64_t N, int d, double p_in, double p_out, const int64_t *seed, float *d_x, float *d_y,
                          float *d_w, void *workspace, size_t workspace_bytes, rqhip_stream_t stream);

/* Semantic-id heads and their cross-entropy losses in one call forward and one backward (csrc/sid_head_loss.hip;
 * modules/model.py, head_impl = "hip").  B rows, T positions per row (T >= L), L levels, K codes, width d; all fp32.
 *   x       the decoder's hidden states [B, T, d]: row stride ld_xb, position stride ld_xt (elements, multiples of 4);
 *           positions t >= L are never read
 *   w       a HOST array of L device pointers, w[h] a dense [K, d] matrix; the entry points copy the pointers into the
 *           kernels' argument block, so the array may be a temporary
 *   target  [B, >= L] int64 with row stride ld_t >= L; columns h >= L are never read
 * rqhip_sid_head_loss_fwd:
 *   z[b,h,k]  = sum_j x[b,h,j] * w[h][k,j]        one fmaf chain from 0 in ascending j
 *   m = max_k z,  s = sum_k expf(z - m),  lse[b,h] = m + logf(s)
 *   row_loss[h,b] = lse[b,h] - z[b,h,target[b,h]]
 *   loss_d[h] = (sum_b row_loss[h,b]) / B          loss = ((0 + loss_d[0]) + loss_d[1]) + ...
 *   Outputs: z [B, L, K], lse [B, L], row_loss [L, B] (all dense; the backward reads z and lse), loss_d [L], loss [1].
 * rqhip_sid_head_loss_bwd, from d_loss (a DEVICE pointer to the upstream gradient of `loss`; the host never reads it):
 *   q[b,h,k]    = (expf(z - lse) - [k == target[b,h]]) * (d_loss / B)
 *   d_x[b,h,:]  = sum_k q[b,h,k] * w[h][k,:]       one fmaf chain from 0 in ascending k;  d_x[b,t,:] = 0 for t >= L
 *   d_w[h][k,:] = sum_b q[b,h,k] * x[b,h,:]        blocks of 64 rows: a block is one fmaf chain from 0 in ascending b,
 *                                                   the blocks are added in ascending order from 0
 *   d_x is a dense [B, T, d] tensor, the zeros of t >= L written by the kernel; d_w a HOST array of L device pointers to
 *   dense [K, d] matrices.  d_x NULL, d_w NULL or an entry d_w[h] NULL: that gradient is not wanted.
 * Reductions: max and sum over K add per-lane partials (lane l holds k = l, l + 64, ... in ascending order) and then the
 * 64 lanes in an xor butterfly (32, 16, 8, 4, 2, 1); the mean over B does the same over the rows.  Every order is a
 * function of the sizes alone and there are no atomics, so the same inputs give the same bits on every run and device,
 * a level's outputs depend on that level's targets only, and a row's lse on neither B nor the row's position.
 * The softmax subtracts the row maximum: logits of several hundred give a finite loss.
 * Targets: a target outside [0, K) is never used as an address; it makes row_loss of its row, loss_d[h] and loss NaN, and
 * the row contributes no one-hot term to the backward.  torch's ignore_index (-100) is NOT reproduced: -100 is out of
 * range like any other negative value.
 * Limits (rqhip_sid_head_loss_supported): d a multiple of 4, 4 <= d <= 1024; 1 <= K <= 1024; 1 <= L <= 8, else
 * RQHIP_EUNSUPPORTED; B >= 1; x and every w[h] 16-byte aligned.  No allocation, copy, memset or sync (graph-capturable);
 * forward: two launches, backward: one. */
int rqhip_sid_head_loss_supported(int d, int K, int L);
int rqhip_sid_head_loss_fwd(const float *x, int64_t ld_xb, int64_t ld_xt, const float *const *w, const int64_t *target,
                            int64_t ld_t, int64_t B, int T, int L, int K, int d, float *z, float *lse, float *row_loss,
                            float *loss_d, float *loss, rqhip_stream_t stream);
int rqhip_sid_head_loss_bwd(const float *x, int64_t ld_xb, int64_t ld_xt, const float *const *w, const int64_t *target,
                            int64_t ld_t, const float *z, const float *lse, const float *d_loss, int64_t B, int T, int L,
                            int K, int d, float *d_x, float *const *d_w, rqhip_stream_t stream);

/* The T5 feed-forward body in one launch forward and at most two backward (csrc/t5_ffn.hip; modules/t5.py, ffn_impl =
 * "hip").  N rows, d = d_model, F = d_ff; x, y, d_y, d_x dense [N, d], h and the workspace's g dense [N, F], wi [F, d] and
 * wo [d, F] the two nn.Linear weights as stored; all fp32.  With `hash`, `seed` as in rqhip_t5_attention_fwd_train above:
 *   keep(n, f) = hash(seed, n * F + f) >= round(p * 2^32)        s = (float)(1 / (1 - p)), evaluated in double
 *   h  = x . wi^T, then +0 wherever that is <= 0 (a NaN stays)   hd = h at p = 0, else keep ? h * s : +0
 *   y  = hd . wo^T                                               (hd is never stored)
 * (rqhip/ops.py:t5_attention_dropout_keep(seed, 1, 1, N, F, p)[0, 0] restates the mask.)  h NULL: it is not stored.
 *   rqhip_t5_ffn_bwd, from d_y:
 *     g    = (h > 0 and keep) ? (d_y . wo) * s : 0      (at p = 0: h > 0 ? d_y . wo : 0)
 *     d_x  = g . wi        d_wi = g^T . x        d_wo = d_y^T . hd, hd recomputed from h and the seed
 *   d_x, d_wi or d_wo NULL: that gradient is not wanted (all three: nothing is launched).  Launch 1 (skipped when only
 *   d_wo is wanted) forms g tile by tile, writes it to `workspace` when d_wi is wanted (rqhip_t5_ffn_bwd_workspace_bytes
 *   = 4 * N * F bytes; the workspace may be NULL otherwise) and produces d_x; launch 2 (skipped when neither weight
 *   gradient is wanted) produces d_wi and d_wo.
 * Arithmetic contract.  All products and sums are fp32 FMAs of v_mfma_f32_16x16x4_f32, every chain starts from +0, and
 * the order of every chain is a function of the sizes alone:
 *   - a GROUP of 32 consecutive reduction terms is consumed in the order 0 8 16 24 1 9 17 25 ... 7 15 23 31
 *     (csrc/mlp_small.hip's order); 4 consecutive groups (128 terms) are ONE chain from +0, and a reduction's chains
 *     are added in ascending order from +0: h and g over the chains of d, y and d_x over those of F.  The order
 *     depends on (d, F) alone, so a row's h, y, g and d_x do not depend on N, on the row's position or on the other
 *     rows of the batch (the row-tile height, 16 up to N = 16384 and 32 above, changes which workgroup computes a
 *     row, not how);
 *   - d_wi and d_wo reduce over the rows in blocks of 32 (rows 4 ks + kq of a block are the k-slots kq of instruction
 *     ks = 0 .. 7; rows past N count as zero); with nb = ceil(N / 32), wave w = 0 .. 3 of the tile's owning workgroup
 *     takes blocks [w nb / 4, (w + 1) nb / 4), starts a fresh chain every 8 blocks and adds its chains in ascending
 *     order from +0; the result is ((s_0 + s_1) + s_2) + s_3 over the waves' sums.  The order depends on N alone.
 * No atomics: the same bits on every run and device.  Rows past N read a valid row and store nothing.
 * Limits (rqhip_t5_ffn_supported): d a multiple of 32 in 32 .. 512 and F a multiple of 32 in 32 .. 8192, else
 * RQHIP_EUNSUPPORTED; any N >= 0 (N = 0 launches nothing); every pointer 16-byte aligned; 0 <= p < 1; `seed` is a
 * one-element int64 DEVICE pointer the host never reads, required iff p > 0.  All argument checks come before any HIP
 * call; no allocation, copy, memset or sync (graph-capturable). */
int rqhip_t5_ffn_supported(int d, int F);
size_t rqhip_t5_ffn_bwd_workspace_bytes(int64_t N, int d, int F);
int rqhip_t5_ffn_fwd(const float *x, const float *wi, const float *wo, int64_t N, int d, int F, double p,
                     const int64_t *seed, float *y, float *h, rqhip_stream_t stream);
int rqhip_t5_ffn_bwd(const float *x, const float *wi, const float *wo, const float *h, const float *d_y, int64_t N, int d,
                     int F, double p, const int64_t *seed, float *d_x, float *d_wi, float *d_wo, void *workspace,
                     rqhip_stream_t stream);

/* The "bf16" arithmetic of the same two calls (modules/t5.py, matmul_arith = "bf16"): the parameter lists, limits,
 * argument checks, workspace size, launch counts and graph capturability of their fp32 twins above.  Storage stays fp32
 * everywhere: x, y, h, g, the weights and every gradient; no tensor changes shape, stride or owner.
 * Arithmetic contract ("bf16").
 *   - Every operand of a matrix instruction is the round-to-nearest-even bf16 rounding (v_cvt_pk_bf16_f32) of the fp32
 *     value the fp32 arm feeds at that place: x, wi, wo and d_y; the values of the LDS chunk, hd = keep ? h * s : 0
 *     forward and g backward, each computed in fp32 first; in the weight-gradient kernel g, x, d_y and the recomputed
 *     hd.  The values are rounded as the fragments are packed (where a value is rounded does not change it).
 *   - Products are exact and accumulate in fp32 inside v_mfma_f32_16x16x32_bf16.
 *   - The chain structure is the fp32 arm's: one GROUP of 32 terms is one instruction (the order inside it is the
 *     instruction's), 4 groups are one chain from +0, and a reduction's chains are added in ascending order from +0.
 *     Weight gradients: blocks of 32 rows (one instruction each; the lane's rows 4 ks + kq are elements j = ks of both
 *     fragments, a consistent permutation of the block), a fresh chain every 8 blocks, wave ranges [w nb / 4, (w + 1)
 *     nb / 4) and ((s_0 + s_1) + s_2) + s_3.
 *   - Orders depend on the sizes alone and there are no atomics: the same bits on every run and device, and a row's h,
 *     y, g and d_x depend neither on N nor on the row's position.  (The backward at d > 384 keeps 16-row tiles above
 *     N = 16384 too; the tile height changes no bit.)
 *   - h is stored unrounded, the fp32 ReLU of the fp32 accumulation; the backward's active set is h > 0 of that tensor.
 *     h does not know about the dropout; p = 0 with and without a seed gives the same bits.  Rows past N read a valid
 *     row and store nothing.
 * Error against exact arithmetic on the rounded operands: at most (K + 8) 2^-23 sum |a_k| |b_k| per element over a
 * reduction of K terms (tests/test_gpu_t5_ffn_bf16.py; measured ratios in profiles/t5_bf16_error.txt).  The operand
 * rounding itself is bf16's: 2^-9 relative per operand. */
int rqhip_t5_ffn_fwd_bf16(const float *x, const float *wi, const float *wo, int64_t N, int d, int F, double p,
                          const int64_t *seed, float *y, float *h, rqhip_stream_t stream);
int rqhip_t5_ffn_bwd_bf16(const float *x, const float *wi, const float *wo, const float *h, const float *d_y, int64_t N,
                          int d, int F, double p, const int64_t *seed, float *d_x, float *d_wi, float *d_wo,
                          void *workspace, rqhip_stream_t stream);

/* A group of 1 <= n <= 8 bias-free linear maps that share their input rows, as one launch forward and at most two
 * backward (csrc/t5_proj.hip; modules/t5.py, proj_impl = "hip": the q / k / v, the o and the cross-attention K/V
 * projections).  N rows; all fp32.
 *   x       [N, d_in] with row stride ld_x >= d_in (elements, a multiple of 4)
 *   w       a HOST array of n device pointers, w[j] the nn.Linear weight [d_out, d_in] as stored (dense); the entry
 *           points copy this array and the ones below into the kernels' argument block, so they may be temporaries
 *   y       a HOST array of n device pointers, y[j] [N, d_out] with its own row stride ld_y[j] >= d_out (a HOST array):
 *           columns >= d_out of a row and rows >= N are never written, so y[j] may be a position of a decode-cache slab
 * rqhip_t5_proj_fwd:   y[j] = x . w[j]^T for j < n.  One launch.
 * rqhip_t5_proj_bwd, from the HOST array d_y of n device pointers, d_y[j] [N, d_out] with row stride ld_dy[j] >= d_out
 * (a multiple of 4):
 *     d_x = sum_j d_y[j] . w[j]          d_w[j] = d_y[j]^T . x
 *   A d_y[j] that is NULL contributes to nothing: it is left out of d_x's sum and its d_w[j] is not written.  d_x
 *   (dense [N, d_in]) NULL, d_w NULL or an entry d_w[j] NULL: that gradient is not wanted.  At most two launches: one
 *   for d_x, one for all wanted d_w[j] (dense [d_out, d_in]); none when nothing is wanted or every d_y[j] is NULL (d_x
 *   is then not written).
 * Arithmetic contract: that of rqhip_t5_ffn_* above.  All products and sums are fp32 FMAs of v_mfma_f32_16x16x4_f32,
 * every chain starts from +0, and the order of every chain is a function of the sizes alone:
 *   - a GROUP of 32 consecutive reduction terms is consumed in the order 0 8 16 24 1 9 17 25 ... 7 15 23 31; 4
 *     consecutive groups (128 terms) are ONE chain from +0, and a reduction's chains are added in ascending order from
 *     +0.  y[j] reduces over d_in.  d_x reduces over the concatenation of the (j, term) pairs, ascending in j and then
 *     in the term, of the d_y[j] that are not NULL: a chain is 128 consecutive terms of that concatenation, across the
 *     boundaries between the j.  So a row's y[j] depends on neither N, nor the row's position, nor n, nor which other
 *     weights are in the group; a row's d_x depends on neither N nor the row's position, and with a d_y[j] NULL it has
 *     the bits of the call on the remaining group (the row-tile height, 16 up to N = 8192, 32 up to 16384 and 64 above,
 *     changes which workgroup computes a row, not how);
 *   - d_w[j] reduces over the rows by rqhip_t5_ffn_bwd's rule: blocks of 32 rows (rows 4 ks + kq of a block are the
 *     k-slots kq of instruction ks = 0 .. 7; rows past N count as zero); with nb = ceil(N / 32), wave w = 0 .. 3 of the
 *     tile's owning workgroup takes blocks [w nb / 4, (w + 1) nb / 4), starts a fresh chain every 8 blocks and adds
 *     its chains in ascending order from +0; the result is ((s_0 + s_1) + s_2) + s_3.  The order depends on N alone.
 * No atomics: the same bits on every run and device.  Rows past N read a valid row and store nothing.
 * Limits (rqhip_t5_proj_supported): d_in and d_out multiples of 32 in 32 .. 512 and 1 <= n <= 8, else
 * RQHIP_EUNSUPPORTED; any N >= 0 (N = 0 launches nothing); x, d_x, every w[j] and d_y[j] 16-byte aligned, y[j] and
 * d_w[j] 4-byte aligned; a null pointer, a row stride below its width (ld_x, ld_dy[j] also: not a multiple of 4) or a
 * misaligned pointer returns RQHIP_EARG.  All argument checks come before any HIP call; no allocation, copy, memset or
 * sync (graph-capturable). */
int rqhip_t5_proj_supported(int d_in, int d_out, int n);
int rqhip_t5_proj_fwd(const float *x, int64_t ld_x, const float *const *w, float *const *y, const int64_t *ld_y, int n,
                      int64_t N, int d_in, int d_out, rqhip_stream_t stream);
int rqhip_t5_proj_bwd(const float *x, int64_t ld_x, const float *const *w, const float *const *d_y, const int64_t *ld_dy,
                      int n, int64_t N, int d_in, int d_out, float *d_x, float *const *d_w, rqhip_stream_t stream);

/* The "bf16" arithmetic of the same two calls: everything of their fp32 twins above but the arithmetic, which is the
 * "bf16" contract of rqhip_t5_ffn_*_bf16.  The operands x, w[j] and d_y[j] are rounded to bf16 (nearest even) as the
 * fragments are packed, products are exact and accumulate in fp32 inside v_mfma_f32_16x16x32_bf16, one group of 32
 * terms is one instruction, and groups, chains, the concatenation of the live (j, term) pairs in d_x and the row blocks
 * of d_w[j] are the fp32 arm's.  So the independence statements hold bit for bit: a row's y[j] depends on neither N,
 * the row's position, n nor the other weights; d_x with a d_y[j] NULL has the bits of the call on the remaining group. */
int rqhip_t5_proj_fwd_bf16(const float *x, int64_t ld_x, const float *const *w, float *const *y, const int64_t *ld_y, int n,
                           int64_t N, int d_in, int d_out, rqhip_stream_t stream);
int rqhip_t5_proj_bwd_bf16(const float *x, int64_t ld_x, const float *const *w, const float *const *d_y,
                           const int64_t *ld_dy, int n, int64_t N, int d_in, int d_out, float *d_x, float *const *d_w,
                           rqhip_stream_t stream);

/* bf16 weight images for the "bf16" arithmetic of the four calls above (csrc/t5_images.hip; modules/t5.py,
 * weight_images = "bf16").  The image of a row-major fp32 matrix w [rows, cols] is the dense bf16 matrix img [rows, cols]
 * with img[r][c] = the round-to-nearest-even bf16 rounding of w[r][c] -- the compiler's (__bf16) conversion, the very
 * bits the "bf16" arithmetic packs into a fragment (a NaN stays a NaN; the largest finite fp32 values round to inf) --
 * and its transposed image is img_t [cols, rows], img_t[c][r] = img[r][c].  An element is a 16-bit pattern. */
typedef uint16_t rqhip_bf16_t;
/* One launch makes the images of any number of matrices.  The job table is built on the host and lives in DEVICE memory:
 *   rqhip_bf16_images_job_bytes(n_jobs)   bytes of a table of n_jobs jobs (0 for n_jobs < 0)
 *   rqhip_bf16_images_fill_jobs           writes the table for the device pointers src[j] [rows[j], cols[j]], img[j] and
 *       img_t[j] (an entry, or img_t itself, NULL: no transposed image) into the HOST buffer host_jobs (8-byte aligned)
 *       and returns the launch's workgroup count in *n_tiles: one per 32 x 32 tile, the jobs' tiles in ascending j.  It
 *       makes no HIP call.  A null host_jobs, src, img, rows, cols, n_tiles, src[j] or img[j], a pointer that is not
 *       16-byte aligned or n_jobs < 0 returns RQHIP_EARG; rows[j] or cols[j] not a positive multiple of 32 (every tile
 *       is full: the shapes rqhip_t5_ffn_supported and rqhip_t5_proj_supported admit), or more than 2^31 - 1 tiles,
 *       returns RQHIP_EUNSUPPORTED.  The caller copies the table to the device and rebuilds it only when a pointer
 *       changes.
 *   rqhip_bf16_images(jobs, n_jobs, n_tiles, stream)   with the DEVICE copy of the table: exactly one kernel launch
 *       and nothing else -- no copy, allocation, memset, host read or sync (graph-capturable).  A workgroup finds its
 *       job from the table's tile prefix sums; a tile goes through LDS, so that the loads and the stores of both images
 *       are contiguous.  n_jobs == 0 returns RQHIP_OK and launches nothing; a null table or one that is not 16-byte
 *       aligned, n_jobs < 0, n_tiles < n_jobs or n_tiles > 2^31 - 1 returns RQHIP_EARG before any HIP call.  src must
 *       not overlap an image. */
size_t rqhip_bf16_images_job_bytes(int n_jobs);
int rqhip_bf16_images_fill_jobs(void *host_jobs, const float *const *src, rqhip_bf16_t *const *img,
                                rqhip_bf16_t *const *img_t, const int64_t *rows, const int64_t *cols, int n_jobs,
                                int64_t *n_tiles);
int rqhip_bf16_images(const void *jobs, int n_jobs, int64_t n_tiles, rqhip_stream_t stream);

/* The "bf16" arithmetic reading its weights from images: the parameter lists of the *_bf16 calls with the weight
 * pointers typed as images, and their limits, argument checks (shared; the messages name the entry point called),
 * workspace size, launch plan and launch counts.  Each call reads the images whose ROWS hold its reduction terms:
 *   rqhip_t5_ffn_fwd_bf16w    wi16 [F, d], wo16 [d, F]                       the images of wi and wo
 *   rqhip_t5_ffn_bwd_bf16w    wi16t [d, F], wo16t [F, d]                     their transposed images
 *   rqhip_t5_proj_fwd_bf16w   w16[j] [d_out, d_in]                           (a HOST array of n device pointers)
 *   rqhip_t5_proj_bwd_bf16w   w16t[j] [d_in, d_out]                          the transposed images (likewise)
 * Arithmetic contract: results are those of `*_bf16` on the weights the images were made from, bit for bit, for every
 * output (y, h, d_x, the workspace's g, d_wi, d_wo, d_w[j]).  An image element is the rounded operand itself, a lane's
 * eight terms of a column are one 16-byte load, groups, chains and their order are unchanged, and which lane serves a
 * column does not enter its sum.  Keeping the images current is the caller's business: a stale image gives the result
 * of *_bf16 on the OLD weights.  The weight gradients read no weights. */
int rqhip_t5_ffn_fwd_bf16w(const float *x, const rqhip_bf16_t *wi16, const rqhip_bf16_t *wo16, int64_t N, int d, int F,
                           double p, const int64_t *seed, float *y, float *h, rqhip_stream_t stream);
int rqhip_t5_ffn_bwd_bf16w(const float *x, const rqhip_bf16_t *wi16t, const rqhip_bf16_t *wo16t, const float *h,
                           const float *d_y, int64_t N, int d, int F, double p, const int64_t *seed, float *d_x,
                           float *d_wi, float *d_wo, void *workspace, rqhip_stream_t stream);
int rqhip_t5_proj_fwd_bf16w(const float *x, int64_t ld_x, const rqhip_bf16_t *const *w16, float *const *y,
                            const int64_t *ld_y, int n, int64_t N, int d_in, int d_out, rqhip_stream_t stream);
int rqhip_t5_proj_bwd_bf16w(const float *x, int64_t ld_x, const rqhip_bf16_t *const *w16t, const float *const *d_y,
                            const int64_t *ld_dy, int n, int64_t N, int d_in, int d_out, float *d_x, float *const *d_w,
                            rqhip_stream_t stream);

/* bf16 saved activations for the "bf16" feed-forward (csrc/t5_ffn.hip; modules/t5.py, saved_activations = "bf16"): the
 * forward keeps, and the backward's row kernel hands its weight-gradient kernel, blocked bf16 IMAGES of the operands the
 * "bf16" arithmetic rounds in registers, in place of fp32 tensors.
 * The blocked image of an activation [N, C], C a multiple of 32.  With NB = ceil(N / 32), b = n >> 5, rho = n & 31,
 * kq = rho & 3 and ks = rho >> 2, element (n, c) is bf16 number ((b * C + c) * 32 + 8 * kq + ks) of a buffer of NB * C * 32
 * bf16: rqhip_t5_ffn_act_image_bytes(N, C) = 64 * NB * C bytes (0 for N < 0 or a C that is no positive multiple of 32).
 * The eight rows 4 ks + kq, ks = 0 .. 7, of block b and column c are 16 consecutive bytes: the elements j = ks of the
 * weight-gradient kernel's fragment for lane (i, kq), as the "bf16" contract above assigns them.  An element is the
 * round-to-nearest-even bf16 rounding of the fp32 value, the (__bf16) conversion of the weight images.  Rows >= N of the
 * last block are UNSPECIFIED in memory (a 16-row tile that ends the batch leaves half a block without a writer); every
 * reader treats them as zero or feeds them only to rows it never stores.
 *   rqhip_t5_ffn_fwd_bf16a   rqhip_t5_ffn_fwd_bf16 with, in place of h, the images hd16 of hd = keep ? h * s : +0 (h at
 *                            p = 0) [N, F] and x16 of x [N, d]; either NULL: not stored.  y has the bits of
 *                            rqhip_t5_ffn_fwd_bf16.  One launch; LDS and the arithmetic are unchanged.
 *   rqhip_t5_ffn_bwd_bf16a   from x16, hd16, the weights and fp32 d_y; no seed:
 *                              g = hd16 > 0 ? (d_y . wo) * s : 0   (an ordered compare: a NaN is off, as in h > 0)
 *                              d_x = g . wi      d_wi = bf16(g)^T . x16      d_wo = bf16(d_y)^T . hd16
 *                            Launch 1 (the row kernel) writes the image dy16 of d_y into the workspace when a weight
 *                            gradient is wanted, the image g16 of g behind it when d_wi is wanted, and d_x when wanted;
 *                            with d_wo alone it only stages d_y and writes dy16.  Launch 2 (when a weight gradient is
 *                            wanted) reads g16, x16, dy16 and hd16, four 16-byte loads per block and lane, with the
 *                            blocks, chains, wave ranges and sums of rqhip_t5_ffn_bwd_bf16 and no dropout decision.
 *                            d_x alone: one launch; all three NULL: none.  rqhip_t5_ffn_bwd_bf16a_workspace_bytes(N, d,
 *                            F) = act_image_bytes(N, d) + act_image_bytes(N, F) (0 for N < 0 or an unsupported shape);
 *                            required whenever d_wi or d_wo is wanted (else RQHIP_EWORKSPACE), may be NULL otherwise;
 *                            without d_wi only its first act_image_bytes(N, d) bytes are touched.
 *   rqhip_t5_ffn_fwd_bf16wa, rqhip_t5_ffn_bwd_bf16wa   the same reading weight images, as rqhip_t5_ffn_*_bf16w.
 * Arithmetic contract: every output (y, d_x, d_wi, d_wo) has the bits of rqhip_t5_ffn_*_bf16 on the same inputs, and an
 * image element is the operand that arm packs.  hd enters that arm as a matrix operand only as bf16(hd), which hd16
 * stores; g, x and d_y enter the weight gradients only rounded; and the arm's active set h > 0 and keep is hd16 > 0 --
 * with ONE difference: a kept element with h > 0 whose h * s rounds to bf16 zero (h * s <= 2^-134) is OFF here and on in
 * rqhip_t5_ffn_bwd_bf16 (its g differs); its contribution as an operand is zero in both.
 * Limits, the checks of N, d, F and p, 16-byte alignment of every pointer, `seed` (forward only) and graph capturability
 * are those of the twins; a null x16 or hd16 in the backward is RQHIP_EARG.  All argument checks come before any HIP
 * call. */
size_t rqhip_t5_ffn_act_image_bytes(int64_t N, int C);
size_t rqhip_t5_ffn_bwd_bf16a_workspace_bytes(int64_t N, int d, int F);
int rqhip_t5_ffn_fwd_bf16a(const float *x, const float *wi, const float *wo, int64_t N, int d, int F, double p,
                           const int64_t *seed, float *y, rqhip_bf16_t *hd16, rqhip_bf16_t *x16, rqhip_stream_t stream);
int rqhip_t5_ffn_bwd_bf16a(const rqhip_bf16_t *x16, const float *wi, const float *wo, const rqhip_bf16_t *hd16,
                           const float *d_y, int64_t N, int d, int F, double p, float *d_x, float *d_wi, float *d_wo,
                           void *workspace, rqhip_stream_t stream);
int rqhip_t5_ffn_fwd_bf16wa(const float *x, const rqhip_bf16_t *wi16, const rqhip_bf16_t *wo16, int64_t N, int d, int F,
                            double p, const int64_t *seed, float *y, rqhip_bf16_t *hd16, rqhip_bf16_t *x16,
                            rqhip_stream_t stream);
int rqhip_t5_ffn_bwd_bf16wa(const rqhip_bf16_t *x16, const rqhip_bf16_t *wi16t, const rqhip_bf16_t *wo16t,
                            const rqhip_bf16_t *hd16, const float *d_y, int64_t N, int d, int F, double p, float *d_x,
                            float *d_wi, float *d_wo, void *workspace, rqhip_stream_t stream);

/* The retrieval model's input embedding in one launch forward and one backward (csrc/sid_embed.hip; modules/model.py,
 * embed_impl = "hip"): semantic ids -> a T5 stack's inputs_embeds, for the encoder and the decoder front alike.
 * B rows, `items` items per row, L levels, K codes per level, width d; table [V = L * K, d], x dense [B, T, d], fp32.
 * has_sep = (sep != NULL), has_prefix = (prefix_table != NULL), T = has_prefix + items * (L + has_sep).  Row b of x:
 *   prefix (t = 0, optional)     row floor_mod(prefix_idx[b * prefix_idx_ld], prefix_rows) of prefix_table
 *                                [prefix_rows, d] (torch.remainder: never negative); prefix_idx NULL: row 0 for every b
 *   id position (item i, level h)   m = mask ? (mask[b, i * ld_item + h] != 0) : 1
 *                                row (ids[b, i * ld_item + h] + h * K) * m of table
 *   separator after each item (optional)   sep [d]
 *   ids   [B, items * ld_item] int64, dense rows; ld_item >= L columns per item, columns h >= L of an item never read
 *   mask  the same layout, elements of mask_elt_size bytes: 1 (bool) or 8 (int64); NULL = all ones
 *   mask_out [B, T] bytes (optional): 1 at the prefix, m at an id position, at a separator the m of level L - 1
 * A padded id (-1 with mask 0) reads row 0.  An index outside [0, V) after the offset and the mask is never used as an
 * address: the forward clamps it into the table (it reads row 0 or row V - 1), the backward drops that token.
 * rqhip_sid_embed_bwd, from d_x dense [B, T, d] and the same plan (has_sep, has_prefix given as flags):
 *   d_table  [V, d]: row r = the sum of d_x over the id positions whose index is r, zero where there is none
 *   d_sep    [d]: the sum over every separator position            d_prefix [prefix_rows, d]: per prefix row, the sum
 *   over the rows b that read it (prefix_idx NULL: row 0 is the sum over b).  Each is written whole; NULL: not wanted.
 *   One workgroup per destination row scans the tokens in chunks of 1024, keeps a chunk's matches in ascending token
 *   order, and with G = max(1, 256 / (d / 4)) adds per column the entries g, g + G, g + 2G, ... of a chunk from +0 for
 *   g = 0 .. G - 1, then those G sums in ascending g, then the chunks in ascending order from +0.  No atomics, no host
 *   read: the order is a function of the shape and the ids alone, so the same inputs give the same bits on every run.
 *   rqhip_sid_embed_bwd_workspace_bytes is the size of `workspace` (a function of the shape alone; this version keeps
 *   every partial sum on chip and returns 0, and `workspace` may then be NULL).
 * Limits (rqhip_sid_embed_supported): d a multiple of 4 in 4 .. 1024, 1 <= L <= 8, else RQHIP_EARG; any K >= 1, items >= 1,
 * B >= 0 (B = 0 returns RQHIP_OK without a launch); B * T and L * K + prefix_rows below 2^31; table, sep,
 * prefix_table, x and the gradients 16-byte aligned.  All argument checks come before any HIP call; no allocation, copy,
 * memset or sync (graph-capturable). */
int rqhip_sid_embed_supported(int d, int L);
size_t rqhip_sid_embed_bwd_workspace_bytes(int64_t B, int items, int L, int K, int d);
int rqhip_sid_embed_fwd(const int64_t *ids, const void *mask, int mask_elt_size, int64_t B, int items, int L, int ld_item,
                        int K, int d, const float *table, const float *sep, const float *prefix_table,
                        const int64_t *prefix_idx, int64_t prefix_idx_ld, int64_t prefix_rows, float *x, uint8_t *mask_out,
                        rqhip_stream_t stream);
int rqhip_sid_embed_bwd(const float *d_x, const int64_t *ids, const void *mask, int mask_elt_size, int64_t B, int items,
                        int L, int ld_item, int K, int d, int has_sep, int has_prefix, const int64_t *prefix_idx,
                        int64_t prefix_idx_ld, int64_t prefix_rows, float *d_table, float *d_sep, float *d_prefix,
                        void *workspace, size_t workspace_bytes, rqhip_stream_t stream);

/* The retrieval model's training batch in one launch (csrc/seq_batch.hip; rqhip/ops.py:seq_batch, data/seq_loader.py):
 * device-resident user histories + the tokenizer's cached id table + two random integers per row -> every tensor of a
 * TokenizedSeqBatch.  All tensors int64 and dense unless said otherwise.
 *   offsets [U + 1], items [nnz]: the histories in CSR form, user r owns items[offsets[r] .. offsets[r + 1]);
 *   fut [U]: the item that follows user r's history; user [U]: the user ids; rows [B]: user indices, repeats allowed
 *   table [n_items, w]: the ids of every item (w = levels + the dedup column)
 *   draws [B, 2] or NULL.  With n_hist = offsets[r + 1] - offsets[r], seq = the history followed by fut[r], n = n_hist + 1:
 *     NULL     history = the last min(S, n_hist) items, target = fut[r]
 *     else     start = u0 mod (max(0, n - 3) + 1), end = min(start + 3 + u1 mod (S - 1), n) with (u0, u1) = draws[b]
 *              read as unsigned; window = seq[start .. end): its last element is the target, the rest the history
 *              (data/processed.py:seq_window is the same law on the host)
 *   sem_ids [B, S * w]: the history's table rows, -1 in the slots behind it; seq_mask [B, S * w] bytes (bool): 1 where
 *   sem_ids holds a table row; sem_ids_fut [B, w]: the target's row; user_ids [B] (the [B, 1] of a batch);
 *   token_type [B, S * w] and token_type_fut [B, w] (each optional, NULL: not written): column mod w.
 * An item id outside [0, n_items) is padding: -1 and mask 0 (all -1 for a target), and nothing is read outside the
 * table.  A user index outside [0, U) gives an empty history, target -1 and user id -1; offsets are clamped into
 * [0, nnz]: no index taken from device memory is used as an address unchecked.
 * One thread per 16 bytes of output ids when w is even and table, sem_ids, sem_ids_fut and the token types are 16-byte
 * aligned (seq_mask 2-byte aligned), else one per id.  Limits (rqhip_seq_batch_supported): 2 <= w <= 9, 2 <= S <= 256,
 * else RQHIP_EARG; B * (S + 1) * w below 2^31; B = 0 returns RQHIP_OK without a launch.  All argument checks come before
 * any HIP call; no allocation, copy, memset, sync or workspace (graph-capturable). */
int rqhip_seq_batch_supported(int w, int S);
int rqhip_seq_batch(const int64_t *offsets, const int64_t *items, const int64_t *fut, const int64_t *user, int64_t U,
                    int64_t nnz, const int64_t *rows, int64_t B, const int64_t *draws, const int64_t *table,
                    int64_t n_items, int w, int S, int64_t *sem_ids, uint8_t *seq_mask, int64_t *sem_ids_fut,
                    int64_t *user_ids, int64_t *token_type, int64_t *token_type_fut, rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Reconstruction loss (modules/loss.py:5-10 ReconstructionLoss, called at modules/rqvae.py:152), fused.
 *   forward : out[b] = sum_d (x_hat[b,d] - x[b,d])^2        x_hat, x: [B,N] with row strides ld_* (elements, >= N)
 *   backward: g_x_hat[b,d] = 2 (x_hat[b,d] - x[b,d]) g_out[b]; g_x = -g_x_hat; either output may be NULL;
 *             outputs are dense [B,N].
 */
int rqhip_recon_loss_forward(const float *x_hat, int64_t ld_hat, const float *x, int64_t ld_x, int64_t B,
                             int N, float *out, rqhip_stream_t stream);
int rqhip_recon_loss_backward(const float *x_hat, int64_t ld_hat, const float *x, int64_t ld_x,
                              const float *g_out, int64_t B, int N, float *g_x_hat, float *g_x,
                              rqhip_stream_t stream);

/* Speculative form of the pair above for the training step: the forward also writes the gradient it expects to be
 * asked for, g_spec[b,:] = (2 (x_hat - x)) * row_scale -- `(reconstruction + quantize_loss).mean().backward()`
 * (modules/rqvae.py:152-154) sends row_scale = 1/B to every row -- and the backward only re-does rows whose upstream
 * gradient g_out[b] is NOT bit-identical to row_scale (exactly what rqhip_recon_loss_backward would write).  Same
 * results as the plain pair in every case; one HBM pass instead of two when the expectation holds.
 * Needs N and the strides multiples of 4 and 16-byte aligned pointers (else RQHIP_EUNSUPPORTED: use the plain pair). */
int rqhip_recon_loss_forward_spec(const float *x_hat, int64_t ld_hat, const float *x, int64_t ld_x, int64_t B, int N,
                                  float row_scale, float *out, float *g_spec, rqhip_stream_t stream);
int rqhip_recon_loss_backward_spec(const float *x_hat, int64_t ld_hat, const float *x, int64_t ld_x,
                                   const float *g_out, int64_t B, int N, float row_scale, float *g_spec,
                                   rqhip_stream_t stream);

/* The three batch means of RqVae.forward (modules/rqvae.py:154,171-172) in one launch:
 *   out3[0] = mean(recon + quant), out3[1] = mean(recon), out3[2] = mean(quant);  recon, quant [B] fp32, B >= 1. */
int rqhip_loss_means(const float *recon, const float *quant, int64_t B, float *out3, rqhip_stream_t stream);
/* the same means by many workgroups (one launch; block partials met by the last block to arrive, in block order: deterministic).
 * workspace: rqhip_loss_means_workspace_bytes() bytes, 16-byte aligned, zeroed ONCE by the caller and then reusable launch after launch
 * on one stream (the kernel re-arms its counter). */
size_t rqhip_loss_means_workspace_bytes(void);
int rqhip_loss_means_ws(const float *recon, const float *quant, int64_t B, float *out3, void *workspace, size_t workspace_bytes,
                        rqhip_stream_t stream);
/* Its backward (autograd of the three `.mean()`s): g_loss, g_recon_mean, g_quant_mean are device scalars (gradients wrt
 * out3[0..2]; each may be NULL = no gradient).  rows_recon[i] = (g_loss + g_recon_mean) * (1/B) and
 * rows_quant[i] = (g_loss + g_quant_mean) * (1/B) for every i < B, 1/B rounded to fp32 first as PyTorch's mean backward
 * does on the device (either output may be NULL). */
int rqhip_loss_means_backward(const float *g_loss, const float *g_recon_mean, const float *g_quant_mean, int64_t B,
                              float *rows_recon, float *rows_quant, rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Weight gradient of a bias-free Linear(+ReLU) layer with the ReLU backward fused in (SURVEY.md section 8 row f2;
 * reference modules/encoder.py:25-38, autograd of `relu(x @ W.T)`).
 *   g [M,N] gradient wrt the layer output, y [M,N] the layer's (ReLU) output or NULL (no ReLU), x [M,K] its input;
 *   all dense row-major fp32, 16-byte aligned.
 *   dW [N,K] = g_pre^T x  with  g_pre = g where y > 0 else 0  (g itself when y is NULL)      -- overwritten
 *   g_masked [M,N] or NULL: receives g_pre for the data-gradient GEMM that follows; may alias g.
 * The batch rows are split into ranges reduced in a fixed order (workspace holds the partial blocks): the result is
 * bit-reproducible.  Layer shapes: rqhip_linear_wgrad_supported(N, K) (N, K multiples of the 32..256 tile shapes
 * listed in csrc/wgrad.hip; every layer of the shipped 768-512-256-128-32 MLPs); others return RQHIP_EUNSUPPORTED
 * and the caller keeps the library GEMM.
 */
int rqhip_linear_wgrad_supported(int N, int K);
/* returns the tile configuration (>= 0) or -1, and the number of row ranges the kernel will reduce over (tests restate
 * the summation order with it) */
int rqhip_linear_wgrad_plan(int64_t M, int N, int K, int *msplit);
size_t rqhip_linear_wgrad_workspace_bytes(int64_t M, int N, int K);
int rqhip_linear_wgrad(const float *g, const float *y, const float *x, int64_t M, int N, int K,
                       float *g_masked, float *dW, void *workspace, size_t workspace_bytes,
                       rqhip_stream_t stream);
/* The same call with a kernel-selection flag (rqhip_linear_wgrad passes 0).  Layers whose dimensions are multiples of
 * 128 x 256 / 256 x 128 run by default on the bf16 matrix cores with every fp32 operand split into three bf16 pieces and
 * the six piece products that matter (dropped terms <= 2^-23 of a product: below fp32's own rounding of it; fp32
 * accumulation; csrc/wgrad_split.hip): same fixed row ranges and reduction tree, bit-reproducible run to run, but the
 * order inside the matrix instruction is not one the oracle can restate, so that result is held to "no less exact than the
 * library's fp32 GEMM against fp64", not bit-exactness.  RQHIP_WGRAD_FP32 selects the fp32-MFMA kernel whose summation
 * order oracle/rq_oracle.c:rqo_linear_wgrad restates bit for bit (and which small layers always use). */
#define RQHIP_WGRAD_FP32 0x1u
int rqhip_linear_wgrad_ex(const float *g, const float *y, const float *x, int64_t M, int N, int K,
                          float *g_masked, float *dW, void *workspace, size_t workspace_bytes,
                          unsigned flags, rqhip_stream_t stream);
/* The weight gradient in RQHIP_SPLIT_F16X2 arithmetic (the product path for the layers csrc/wgrad_split.hip tiles; see the
 * GEMM section below): the reduction runs over the batch rows, so the exact power-of-two scales are per COLUMN of g and of
 * x -- g_col_max [N], x_col_max [K]: bit patterns of the columns' largest |value| (rqhip_maxima, or the c_col_max of the
 * epilogue that wrote the matrix); two fp16 pieces per scaled value, products hh + hm + mh, the result multiplied back by
 * 2^(e_n + e_k).  With y given the ReLU mask is applied inside as above and g_col_max may hold the maxima of the unmasked
 * g (an upper bound costs low-order bits of the small elements only).  Same row ranges, reduction tree and workspace as
 * rqhip_linear_wgrad; layers the split kernel does not tile run the fp32 kernel and ignore the maxima. */
int rqhip_linear_wgrad_f16(const float *g, const float *y, const float *x, int64_t M, int N, int K,
                           const unsigned *g_col_max, const unsigned *x_col_max, float *g_masked, float *dW,
                           void *workspace, size_t workspace_bytes, rqhip_stream_t stream);
/* Several layers' weight gradients in ONE launch (ABI 462): dW_j [N_j, K_j] = g_j^T x_j for 2..4 layers over the same M rows, EITHER every dW
 * tiled 256 x 256 (N_j, K_j multiples of 256) OR every dW tiled 128 x 256 / 256 x 128 (one dimension a multiple of 256, the other of 128 but
 * not 256; the two kinds mix freely), g_j ALREADY masked by its layer's ReLU, f16x2 arithmetic under the column maxima (as
 * rqhip_linear_wgrad_f16).  The jobs share one number of row ranges (rqhip_linear_wgrad_f16_batch_plan: CUs / tiles of all jobs; 0 = not
 * batchable), so the launch writes and reduces one workgroup's worth of partial blocks per CU for ALL its layers instead of per layer --
 * the weight gradients of reference modules/encoder.py:25-38's Linear layers, which autograd forms one by one.  Results are those of
 * rqhip_linear_wgrad_f16 run with that number of ranges (bit-reproducible; another balanced tree than the per-layer call's). */
typedef struct {
    const float *g;              /* [M, N] */
    const float *x;              /* [M, K] */
    int N, K;
    const unsigned *g_col_max;   /* [N] */
    const unsigned *x_col_max;   /* [K] */
    float *dW;                   /* [N, K] */
} rqhip_wgrad_job;
int rqhip_linear_wgrad_f16_batch_plan(int64_t M, const int *N, const int *K, int n);
size_t rqhip_linear_wgrad_f16_batch_workspace_bytes(int64_t M, const int *N, const int *K, int n);
int rqhip_linear_wgrad_f16_batch(const rqhip_wgrad_job *jobs, int n, int64_t M, void *workspace, size_t workspace_bytes, rqhip_stream_t stream);

/* The weight gradients of SEVERAL layers in one launch, for the batch sizes the reference's gin files train with (64-640 rows:
 * configs/rqvae_ml32m.gin, rqvae_amazon.gin), where the kernels above are latency and launches (csrc/wgrad_jobs.hip).  Job i:
 * dW[i] [N[i], K[i]] = g[i]^T x[i] with g[i] [M, N[i]] ALREADY masked by the layer's ReLU and x[i] [M, K[i]], all row-major
 * fp32; every job has the same M.  g, x, dW, N, K are HOST arrays of n_jobs <= 8 entries (read during the call).  Every (job,
 * 64 x 64 block of dW) is one workgroup that reduces over all M rows -- no row ranges, no workspace, no reduction launch, a fixed
 * summation order, a job's bits independent of the other jobs -- in three-piece bf16 arithmetic: v = h + m + l exactly, the six
 * piece products that matter (dropped terms <= 2^-23 of a product), fp32 accumulation; an entry's error is within
 * (sqrt(M) + 8) 2^-24 of the sum of its terms' magnitudes (tests/test_gpu_wgrad.py).  Shapes: N and K multiples of 32
 * (rqhip_linear_wgrad_jobs_supported); anything else is RQHIP_EARG.  Correct for any M; meant for M up to a few thousand. */
int rqhip_linear_wgrad_jobs_supported(int N, int K);
int rqhip_linear_wgrad_jobs(const float *const *g, const float *const *x, float *const *dW, const int *N, const int *K,
                            int n_jobs, int64_t M, rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The activation GEMMs of the MLPs (reference modules/encoder.py:25-38: `relu(x W^T)` forward; autograd's `g W` data
 * gradient and ReLU backward; modules/rqvae.py:146,152 + modules/loss.py:5-10: the last decoder layer with the
 * reconstruction loss) on the 16-bit matrix cores, carrying fp32's accuracy (csrc/gemm_split.hip).  Two arithmetics:
 *   RQHIP_SPLIT_F16X2  (the product path) every row of A and every weight row is scaled by an exact power of two (the
 *       exponent of its largest |value|), every scaled value is split into two fp16 pieces (11 + 11 significant bits and a
 *       sign), the product is hh + hm + mh (each piece product exact in fp32, fp32 accumulation), and the epilogue multiplies
 *       back by 2^(e_row + e_column).  Needs the row maxima of A: `a_row_max`, written by the kernel that produced A (every
 *       epilogue below can emit the row / column maxima of what it stores) or by rqhip_maxima.
 *   RQHIP_SPLIT_BF16X3 (round 3, kept for A/B) three exact bf16 pieces per operand, six products, no scaling.
 * Both are held to: max error against fp64 <= the library fp32 GEMM's on the same inputs (tests/test_gpu_gemm_split.py:
 * unit-norm rows, post-ReLU activations, 1e-5-scale masked gradients, twelve decades of row scales, five decades inside a
 * row, the worst-case mantissas of the 11-bit split, cancellation-heavy rows), results bit-reproducible run to run.
 *
 *   rqhip_weight_images : split weight matrices w [rows, cols] into the kernel's images, ALL jobs in one launch (an MLP's
 *       layers, both directions).  transpose = 0: the image of w itself (Nc = rows output columns, reduction R = cols: the
 *       forward, C = A w^T); transpose = 1: of w^T (Nc = cols, R = rows: the data gradient, C = A w).  `image`:
 *       rqhip_weight_image_bytes(Nc, R, arith) bytes, caller-owned, 16-byte aligned.  `jobs` is a HOST array.
 *   rqhip_maxima        : row_max [M] and / or col_max [R] (bit patterns of the largest |value|; col_max is maxed into
 *       atomically: zero it first) of A [M, R] in one pass; with Y given, of A masked by Y > 0 (the ReLU backward), which is
 *       also written to masked_out when that is not NULL.  R % 4 == 0, R <= 16384 (columns are taken in chunks of 1024).
 *   rqhip_gemm_split_ex : C [M, Nc] = epilogue(A [M, R] . image^T).  Needs Nc % 128 == 0 (256-column tiles when
 *       Nc % 256 == 0, else 128), R % 16 == 0 (rqhip_gemm_split_supported), 16-byte aligned pointers; one launch at a time
 *       per image (it holds the kernel's tile dispenser).
 */
#define RQHIP_SPLIT_F16X2 0
#define RQHIP_SPLIT_BF16X3 1
#define RQHIP_EPI_STORE 0
#define RQHIP_EPI_RELU 1  /* C = relu(A.B^T) */
#define RQHIP_EPI_RECON 2 /* the last decoder layer fused with ReconstructionLoss: x_hat = A.B^T is never stored; loss_rows[m] =
                             sum_n (x_hat - aux)^2 and C = (2 (x_hat - aux)) * row_scale, the gradient `(reconstruction +
                             quantize_loss).mean().backward()` sends back when row_scale = loss scale / B.  Nc % 256 == 0;
                             workspace: rqhip_gemm_split_recon_workspace_bytes(M, Nc) bytes */
#define RQHIP_EPI_MASK 3  /* C = A.B^T where aux > 0, else 0: a data gradient fused with the ReLU backward of the layer below
                             (aux = that layer's output); RQHIP_SPLIT_F16X2 only */
typedef struct {
    const float *w;      /* [rows, cols] */
    int rows, cols, transpose, arith;
    void *image;
    size_t image_bytes;
} rqhip_image_job;
typedef struct {
    const float *A;      /* [M, R] */
    int64_t M;
    int R;
    const void *image;   /* of B [Nc, R] (rqhip_weight_images) */
    int Nc;
    int arith;           /* RQHIP_SPLIT_* the image was built with */
    int epilogue;        /* RQHIP_EPI_* */
    int tile_rows;       /* 0 (tools only: staged-B kernels 256 / 128 force big tiles, 64 / 32 small ones; -9: 32-row leftover tiles allowed (A/B); -12: the atomic tile dispenser of rounds 4-5 instead of the static schedule (A/B); -8: gemm_f16_kernel with one
                            tile dispenser per XCD instead of one for the chip -- measured slower, profiles/r05_gemm_xcd_dispenser_ab.txt) */
    float *C;            /* [M, Nc] */
    const float *aux;    /* RQHIP_EPI_RECON: X [M, Nc]; RQHIP_EPI_MASK: Y [M, Nc]; else NULL */
    float row_scale;     /* RQHIP_EPI_RECON */
    float *loss_rows;    /* RQHIP_EPI_RECON: [M] */
    void *workspace;     /* RQHIP_EPI_RECON */
    size_t workspace_bytes;
    const unsigned *a_row_max; /* RQHIP_SPLIT_F16X2: [a_row_parts][M]; a row's largest |value| is the maximum over the parts */
    int a_row_parts;
    unsigned *c_row_max; /* optional output [column tiles][M] (Nc / 256 tiles when Nc % 256 == 0, else Nc / 128): largest |value| of
                            each row of C per column tile (plain stores) */
    unsigned *c_col_max; /* optional output [Nc]: largest |value| of each column of C, maxed into atomically (zero it first) */
} rqhip_gemm_args;
int rqhip_gemm_split_supported(int Nc, int R);
size_t rqhip_weight_image_bytes(int Nc, int R, int arith);
int rqhip_weight_images(const rqhip_image_job *jobs, int n_jobs, rqhip_stream_t stream);
int rqhip_maxima(const float *A, const float *Y, float *masked_out, int64_t M, int R, unsigned *row_max, unsigned *col_max,
                 rqhip_stream_t stream);
size_t rqhip_gemm_split_recon_workspace_bytes(int64_t M, int Nc);
int rqhip_gemm_split_ex(const rqhip_gemm_args *args, rqhip_stream_t stream);
/* the round-3 entry points: RQHIP_SPLIT_BF16X3 with one image per call */
size_t rqhip_weight_planes_bytes(int Nc, int R);
int rqhip_weight_planes(const float *w, int rows, int cols, int transpose, void *planes, size_t planes_bytes,
                        rqhip_stream_t stream);
int rqhip_gemm_split(const float *A, int64_t M, int R, const void *planes, int Nc, int relu, float *C,
                     rqhip_stream_t stream);
int rqhip_gemm_split_recon(const float *A, int64_t M, int R, const void *planes, int Nc, const float *X, float row_scale,
                           float *G, float *loss_rows, void *workspace, size_t workspace_bytes, rqhip_stream_t stream);
/* backward fix-up of RQHIP_EPI_RECON: rows of g_out that are not row_scale (bit compare) get G * (g / row_scale) */
int rqhip_recon_rescale_rows(const float *g_out, int64_t B, int N, float row_scale, float *g_spec, rqhip_stream_t stream);
/* ... which also brings the maxima the epilogue emitted for G up to date for the rows it changes: row_max [row_parts][B]
 * (the row's new maximum in part 0, the other parts cleared) and col_max [N] (maxed into); either may be NULL */
int rqhip_recon_rescale_rows_ex(const float *g_out, int64_t B, int N, float row_scale, float *g_spec, unsigned *row_max,
                                int row_parts, unsigned *col_max, rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The RQ <-> MLP seam (first clause): the encoder's last Linear (128 -> D), every quantisation level and the
 * decoder's first Linear (D -> 128) + ReLU as ONE row-local launch -- reference modules/rqvae.py:118-139 (`res = self.encode(x)` ends
 * in that Linear, modules/encoder.py:25-38; the level loop) and :146 (`self.decode(embs.sum(axis=-1))` starts with the other).  D = 32
 * and a hidden width of 128 (the reference's configs/rqvae_amazon.gin); all levels' codebooks must fit the LDS next to the two weights
 * (rqhip_rq_seam_supported).  Either GEMM and the quantisation can be switched off, which makes the same kernel the stand-alone
 * 128 -> D / D -> 128 layer: the data gradients of the backward, with the ReLU backward applied on load (h_mask) or in the epilogue
 * (RQHIP_EPI_MASK).  Arithmetic: every GEMM output is ONE fp32 FMA chain over the input features in ascending order (the fp32 matrix
 * instruction, as the distance scan of rqhip_rq_forward): independent of batch size and launch form, restated by
 * oracle/rq_oracle.c:rqo_linear_chain; the quantisation is rqhip_rq_forward's, bit for bit, on the res0 the input GEMM produced.
 */
typedef struct {
    int64_t B;
    int D;                  /* 32 */
    int H;                  /* width of h / out: 128 */
    /* input side: h given -> res0 = h' . Win^T, h' = h where h_mask > 0 else 0 (h_mask NULL: h' = h); h NULL -> rows come from res0 */
    const float *h;         /* [B, H] or NULL */
    const float *h_mask;    /* [B, H] or NULL */
    const float *w_in;      /* [D, H] row-major (nn.Linear.weight of the H -> D layer); w_in_transposed: [H, D], used as its transpose */
    int w_in_transposed;
    const float *res0;      /* [B, D]: the rows when h == NULL */
    float *res0_out;        /* [B, D] or NULL: the input GEMM's result */
    /* quantisation: L == 0 skips it (the rows go straight to the output GEMM); else as rqhip_rq_forward (filtered scan, all levels resident) */
    const float *codebooks; /* [L, K, D] */
    int L, K, mode;         /* RQHIP_MODE_EVAL / STE / ROTATION */
    float beta;
    int64_t *ids;           /* [L, B] */
    float *emb_sum;         /* [B, D] or NULL */
    float *loss;            /* [B] or NULL */
    float *embs_norm;       /* [B, L] or NULL */
    /* output side: w_out given -> out = epilogue(s . Wout^T), s = the sum of the levels' outputs (L == 0: the rows) */
    const float *w_out;     /* [H, D] row-major (nn.Linear.weight of the D -> H layer); w_out_transposed: [D, H], used as its transpose; or NULL */
    int w_out_transposed;
    int out_epilogue;       /* RQHIP_EPI_STORE / RQHIP_EPI_RELU / RQHIP_EPI_MASK (out where out_mask > 0 else 0) */
    const float *out_mask;  /* [B, H]: RQHIP_EPI_MASK */
    float *out;             /* [B, H] */
    unsigned *out_row_max;  /* optional [H / 32][B]: bit patterns of the largest |value| of each row of `out` per 32-column block (the
                               a_row_max / a_row_parts = H / 32 of the rqhip_gemm_split_ex that reads `out` next) */
    unsigned *out_col_max;  /* optional [H]: column maxima of `out`, maxed into atomically (zero it first) */
} rqhip_seam_args;
int rqhip_rq_seam_supported(int D, int H, int L, int K);   /* 1 when rqhip_rq_seam takes these shapes on the current device */
int rqhip_rq_seam(const rqhip_seam_args *args, rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The encoder / decoder Linear layers at the batch sizes the reference ships (M < 4096 rows: configs/rqvae_amazon.gin:7 batch 640,
 * rqvae_ml32m.gin:7 batch 64) -- reference modules/encoder.py:25-38 (`relu(x W^T)`) and its autograd data gradient `g W` with the ReLU
 * backward of the layer below.  out [M, N] = epilogue(a [M, Kr] . B), B = w^T for w [N, Kr] (w_kn = 0: the forward, nn.Linear.weight
 * as stored) or B = w for w [Kr, N] (w_kn = 1: the data gradient, the same nn.Linear.weight).  N, Kr multiples of 32; a, w, out, aux
 * 16-byte aligned, contiguous.  epilogue: RQHIP_EPI_STORE / RQHIP_EPI_RELU / RQHIP_EPI_MASK (out where aux [M, N] > 0, else 0).
 * Arithmetic: exact fp32 on the fp32 matrix instruction.  The reduction runs as `waves` contiguous ranges of 32-term groups (wave v:
 * groups [v ng / waves, (v + 1) ng / waves), ng = Kr / 32), each ONE fp32 FMA chain from +0 taking a group's terms in the order
 * 0 8 16 24 1 9 17 25 ... 7 15 23 31; out = ((p_0 + p_1) + ...) + p_{waves-1}, then the epilogue.  (col_blocks, waves) = (0, 0): chosen from the shape
 * (rqhip_linear_small_plan reports the choice: the same bits on every box, eager or replayed); restated by
 * oracle/rq_oracle.c:rqo_linear_small.  Valid overrides: col_blocks 1 | 2 (N % 64 == 0), waves 4 | 8 | 16 (16: col_blocks 1). */
int rqhip_linear_small_supported(int64_t M, int N, int Kr);
int rqhip_linear_small_plan(int64_t M, int N, int Kr, int *col_blocks, int *waves);
int rqhip_linear_small(const float *a, const float *w, int w_kn, float *out, int64_t M, int N, int Kr, int epilogue, const float *aux,
                       int col_blocks, int waves, rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The AdamW update of all parameters in one launch (reference train_rqvae.py:136-138: AdamW with decoupled weight decay on every
 * parameter, codebooks included).  Arithmetic of torch's `_fused_adamw_` in fp32 (no amsgrad, no maximize); tensors p / g / m / v of
 * numel[i] contiguous fp32 elements, 16-byte aligned, caller-owned; `step`: device float scalar = steps taken so far, incremented by
 * the call (on the device, so a captured hipGraph advances it on replay); `scratch`: 8 device bytes (8-byte aligned) the call may overwrite. */
int rqhip_adamw_step(float *const *p, const float *const *g, float *const *m, float *const *v, const int64_t *numel, int n,
                     float *step, unsigned *scratch, float lr, float beta1, float beta2, float eps, float weight_decay,
                     rqhip_stream_t stream);

/* The optimizer tail of the retrieval model's training loop (reference train_decoder.py:147-151, 202-205: clip_grad_norm_, AdamW,
 * InverseSquareRootScheduler) with every scalar formed on the device, so that a captured hipGraph replays this step's clip coefficient
 * and learning rate rather than the capture's.  Tensors, `step` and the AdamW hyper-parameters as for the adamw_step call above.  In order:
 *   max_norm > 0: norm = 2-norm of all gradients (one fp32 partial per 1024 elements in `workspace`, stored and summed in a fixed order:
 *     the same bits on every run), coef = min(1, max_norm / (norm + 1e-6)) as torch.nn.utils.clip_grad_norm_; max_norm <= 0: coef = 1,
 *     norm = NaN (not computed), workspace unused;
 *   warmup >= 0: lr = base_lr if *lr_step <= warmup else base_lr sqrt(warmup) / sqrt(*lr_step) (in double, rounded once), then
 *     *lr_step += 1 (device int64); warmup < 0: lr = the argument `lr`, lr_step unused (may be null);
 *   the update of the adamw_step call above with g coef in place of g (gradients are not written back).
 * `scalars`: RQHIP_ADAMW_TAIL_SCALARS device floats, 16-byte aligned, written by the call: [0] lr / (1 - beta1^t), [1] sqrt(1 - beta2^t),
 * [2] lr, [3] coef, [4] norm.  With max_norm <= 0 and warmup < 0, [0] and [1] and the updated tensors are adamw_step's bits.
 * rqhip_adamw_tail_workspace_bytes needs no GPU; -1 (and an error message) for a negative count, a null list or a negative numel.
 * All arguments are checked before the first launch. */
#define RQHIP_ADAMW_TAIL_SCALARS 8
int64_t rqhip_adamw_tail_workspace_bytes(const int64_t *numel, int n);
int rqhip_adamw_tail_step(float *const *p, const float *const *g, float *const *m, float *const *v, const int64_t *numel, int n,
                          float *step, int64_t *lr_step, float *scalars, float *workspace, size_t workspace_bytes, float max_norm,
                          float lr, double base_lr, int64_t warmup, float beta1, float beta2, float eps, float weight_decay,
                          rqhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Kernel timing for bench.py's roofline objects (no reference counterpart).  While enabled, the calls below bracket
 * their MAIN kernel(s) with a hipEvent pair recorded on the call's stream and note what the launch was: a tag, its
 * algorithmic FLOPs and its algorithmic bytes.  rqhip_profile_read_tagged synchronises the recorded events and returns
 * the per-launch records (at most `cap`), then clears the log; rqhip_profile_read returns the durations of the
 * RQHIP_PROF_RQ_FORWARD records only (round 1's interface) and clears the log too.
 */
#define RQHIP_PROF_RQ_FORWARD 1  /* rqhip_rq_forward(_ex): the scan kernel, not the codebook-norm prologue */
#define RQHIP_PROF_RQ_BACKWARD 2 /* rqhip_rq_backward: all of its kernels (flat kernel + table reduce) */
#define RQHIP_PROF_GEMM_SPLIT 3  /* rqhip_gemm_split_ex */
#define RQHIP_PROF_WGRAD 4       /* rqhip_linear_wgrad*: the kernel and its partial-sum reduction */
#define RQHIP_PROF_MAXIMA 5      /* rqhip_maxima */
#define RQHIP_PROF_IMAGES 6      /* rqhip_weight_images */
#define RQHIP_PROF_SEAM 7        /* rqhip_rq_seam: flops = the GEMMs' 2 B D H each + the levels' L (2 D K + 5 D) per row */
#define RQHIP_PROF_LINEAR_SMALL 8 /* rqhip_linear_small: flops = 2 M N Kr */
typedef struct {
    int tag;
    float ms;
    double flops, bytes;
} rqhip_profile_record;
int rqhip_profile_enable(int max_records); /* 0 disables and frees the events */
int rqhip_profile_select(unsigned tag_mask); /* bit t set: record launches tagged t (default: all) */
int rqhip_profile_read(float *ms_out, int cap, int *n_out);
int rqhip_profile_read_tagged(rqhip_profile_record *out, int cap, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* RQHIP_H */
