/* =============================================================================
 * fspann_eval.h — companion of fspann.h: ForwardSecureANNSystem.runQueries' loop
 * (FSA:622-748) over a resident store, exported by libfspann_hip.so.
 *
 * Per query runQueries makes one QueryServiceImpl.search at max(kVariants)
 * (FSA:660-664), searches again with more probes if that returned nothing
 * (FSA:667-678), and computes recall, distance ratio and candidate ratio for every k
 * of kVariants over prefixes of the one result list (FSA:684-692, 770-835).  The
 * first step is fspann_search_retry_dev of fspann.h; the other two are the calls
 * below.  They stand in a header of their own for the reason
 * fspann_groundtruth_rows.h gives: the entry points of fspann.h are a counted set
 * (94).  They are evaluation calls of the native and the Python side; the JVM shim
 * does not bind them.  Conventions are fspann.h's.
 * ========================================================================== */
#ifndef FSPANN_EVAL_H
#define FSPANN_EVAL_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

/* computeMetricsAtK (FSA:770-835) for every k of ks over one result list, one launch.
 * ks [nk] is HOST memory, 1 <= nk <= 64, every k in 1..1024, any order, repeats allowed; it travels in the kernel arguments.
 * base / q, their dtypes, n, dim, ann_ids_dev [nq][ann_stride], ann_count_dev (NULL: ann_stride results per query) and
 * gt_ids_dev [nq][gt_stride] are the arguments of fspann_eval_metrics_typed_dev; gt_stride >= max(ks), ann_stride >= 1.  The
 * accepted (base, query) dtype pairs are that call's and the others are refused as it refuses them (FSPANN_E_ARG naming both).
 * recall_dev / ratio_dev [nk][nq]: row j is bit-identical (NaN payload included) to what
 * fspann_eval_metrics_typed_dev(..., k = ks[j], ...) writes over the same arguments.  Every distance is computed once: the
 * reference's ratio sum for k is the index-ordered fold `sum += dAnn_i / dGt_i` over i < k from 0.0 (FSA:800-815; a skipped
 * term, FSA:807-811, makes the ratio NaN), so the fold for k is a prefix of the fold for max(ks) and one running fold yields
 * every k; result i is a hit for k iff i < k and its id is among gt[0..k), i.e. iff max(i, first place of the id in gt) < k.
 * unique_dev [nq] (may be NULL) is QueryServiceImpl.getLastUniqueCandidates, |F_q| of the query's last pass (sel_count of the
 * search calls); cand_ratio_dev [nk][nq] = unique > 0 ? (double) unique / ks[j] : NaN (FSA:824-828).  cand_ratio_dev is NULL
 * iff unique_dev is NULL (FSPANN_E_ARG otherwise) and is then not written.
 * nq == 0: FSPANN_OK, nothing written.  Stream order, no host synchronisation.                                               */
int fspann_eval_kvariants_dev(fspann_ctx* ctx, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype,
                              int dim, const int32_t* ks, int nk, const int32_t* ann_ids_dev, int64_t ann_stride, const int32_t* ann_count_dev,
                              const int32_t* gt_ids_dev, int64_t gt_stride, const int32_t* unique_dev, double* recall_dev, double* ratio_dev,
                              double* cand_ratio_dev);

/* runQueries' search step: fspann_search_retry_dev (search 1, QSI.search with its adaptive retry), then the empty-result
 * fallback (FSA:667-678) on the device, in stream order, no host synchronisation.  Arguments as fspann_search_retry_dev.
 * A query falls back iff it is not bad (a non-finite query never reaches search: createToken throws), Route flagged it in
 * neither pass of search 1 (count -1) and out_count == 0 (kept == 0, QSI:159; nothing scored, QSI:293; an empty second pass).
 * Fallback probes F = max(2 base, 4), base = po >= 0 ? po : cfg.default_probes, po = probe_override >= 0 ? probe_override :
 * cfg.probe_override (FSA:640, 668-673): probe_override = 0 gives F = 4 although search 1 ran at the default.
 * Search 2 is a whole QSI.search of those queries (search 1's codes) at F probes: list-mode Route and refine, then the adaptive
 * retry (QSI:327-337, 444-447) among them at 10 probes, also when F > 10; when F and 10 are the same effective probes the retry
 * pass is not run and the query is reported retried, as in fspann_search_retry_dev.
 * A fallen-back query's ids, dist, count, scored, sel_ids / sel_count (F_q of its last pass) and retried are search 2's,
 * written in place, even when empty; fellback_dev [nq] (optional) says 1 for it.  Every other query keeps search 1's rows.
 * Touch tracking marks behind every refine: the tracker sees the union of both searches.
 * fspann_search_fallback_finish_dev (same arguments) synchronises and completes the call on the host: search 1's flagged
 * queries as fspann_search_retry_finish_dev does, the fallback of those it just finished, and queries flagged inside search 2
 * with the probes of the pass that flagged them (rescored, retry rule applied).  *resolved = queries finished on the host.
 * Without a preceding fspann_search_fallback_dev of that size: FSPANN_E_STATE.                                                */
int fspann_search_fallback_dev(fspann_ctx* ctx, int64_t nq, const void* q_dev, int q_dtype, int probe_override, int64_t B, int k,
                               int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev,
                               int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, int32_t* retried_dev, int32_t* fellback_dev);
int fspann_search_fallback_finish_dev(fspann_ctx* ctx, int64_t nq, const void* q_dev, int q_dtype, int probe_override, int64_t B, int k,
                                      int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev,
                                      int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, int32_t* retried_dev,
                                      int32_t* fellback_dev, int64_t* resolved);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_EVAL_H */
