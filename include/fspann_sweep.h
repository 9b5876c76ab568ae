/* =============================================================================
 * fspann_sweep.h — companion of fspann.h: QueryServiceImpl.search at several
 * refinement limits in one pass over a resident store, exported by
 * libfspann_hip.so.
 *
 * runtime.refinementLimit (B, the number of candidates stage B decrypts and scores)
 * is the knob that trades recall against cost; the reference exposes it per query
 * (QueryServiceImpl.setRefinementLimit, QSI:454-466).  The override only enters
 * stage A.5 (QSI:170-171): the candidate list lookupCandidatesWithScores returns is
 * the same for every override (its cap comes from the config, PIS:612-615), stage
 * A.5 takes its first B entries (QSI:177-214), and stages B and C keep the K best of
 * those, ties broken by candidate position (QSI:238-316).  The result at limit B is
 * therefore the top-K of the first B candidates, and the results at B_0 < B_1 < ...
 * are snapshots of ONE walk over the list at the largest limit: one encode, one
 * Route, one read of the candidate rows.
 *
 * These calls stand in a header of their own for the reason
 * fspann_groundtruth_rows.h gives: the entry points of fspann.h are a counted set
 * (94).  They are evaluation calls of the native and the Python side; the JVM shim
 * does not bind them.  Conventions are fspann.h's.
 *
 * Common arguments.  limits [nl] is HOST memory, 1 <= nl <= 16, strictly ascending,
 * every value acceptable as B of fspann_search_retry_dev (1 .. INT32_MAX);
 * Bmax = limits[nl - 1].  1 <= k <= 1024.  Anything else is FSPANN_E_ARG with a
 * message naming the argument.  Outputs are planes, one per limit:
 * out_ids_dev [nl][nq][k], out_dist_dev [nl][nq][k], out_count_dev [nl][nq],
 * scored_dev [nl][nq] (may be NULL).  Stream order, no host synchronisation (the
 * finish call excepted).  nq == 0: FSPANN_OK, nothing written.
 *
 * Out of scope: ForwardSecureANNSystem.runQueries' empty-result fallback
 * (FSA:667-678) per limit.  The sweep is QueryServiceImpl.search, not runQueries; a
 * plane with out_count == 0 for a query that is not bad is where runQueries would
 * have searched again (fspann_search_fallback_dev of fspann_eval.h, one limit at a
 * time).
 * ========================================================================== */
#ifndef FSPANN_SWEEP_H
#define FSPANN_SWEEP_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Refine at every limit over caller-held candidate rows (cand_dev, dense [nq][stride][dim] of cand_dtype) or over the resident
 * store (row j of query q is store[cand_ids[q * stride + j]]).  stride >= Bmax is the row pitch of cand_ids_dev and cand_dev.
 * Plane j is bit-identical to what fspann_refine_dev / fspann_refine_store_dev write with B = stride and cand_count[q] replaced by
 * min(max(cand_count[q], 0), limits[j]).  Touch tracking marks what that call at Bmax marks.                                    */
int fspann_refine_sweep_dev(fspann_ctx* ctx, int64_t nq, const void* q_dev, int q_dtype, const void* cand_dev, int cand_dtype, int64_t stride,
                            const int32_t* cand_ids_dev, const int32_t* cand_count_dev, const int64_t* limits, int nl, int k,
                            int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev);
int fspann_refine_store_sweep_dev(fspann_ctx* ctx, int64_t nq, const void* q_dev, int q_dtype, int64_t stride, const int32_t* cand_ids_dev,
                                  const int32_t* cand_count_dev, const int64_t* limits, int nl, int k, int32_t* out_ids_dev,
                                  double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev);

/* QueryServiceImpl.search with its adaptive retry at every limit: plane j of every output is what fspann_search_retry_dev followed
 * by fspann_search_retry_finish_dev writes at B = limits[j].  unique_dev [nl][nq] is that call's sel_count (|F_q| of the query's
 * last pass, what fspann_eval_kvariants_dev takes as unique_dev), bad_dev [nq], retried_dev [nl][nq]; scored_dev and these three are
 * optional.  One encode, one Route at limit Bmax with the caller's probes, one sweep refine over the store; QSI's retry predicate
 * (QSI:327-337, 444-447) is applied per (query, limit), and the queries for which any limit retries take one second pass — Route
 * with 10 probes at Bmax, a sweep refine that overwrites only their retried planes.  When pass 1 already ran at 10 effective
 * probes, pass 2 is not run and the planes are still reported retried, as fspann_search_retry_dev does.
 * Touch tracking sees the union of what the nl separate calls mark: pass 1 marks the rows below min(count, Bmax), pass 2 those
 * below the query's largest retried limit.
 * fspann_search_sweep_finish_dev (same arguments) synchronises and completes the call on the host as
 * fspann_search_retry_finish_dev does: pass 1's flagged queries (count -1) are finished at Bmax with pass 1's probes and scored
 * through the sweep, the predicate is applied per limit, their pass 2 runs, and pass 2's flagged queries are finished with 10
 * probes.  *resolved = queries finished on the host.  Without a preceding fspann_search_sweep_dev of that size: FSPANN_E_STATE. */
int fspann_search_sweep_dev(fspann_ctx* ctx, int64_t nq, const void* q_dev, int q_dtype, int probe_override, const int64_t* limits, int nl, int k,
                            int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev, int32_t* unique_dev,
                            int32_t* bad_dev, int32_t* retried_dev);
int fspann_search_sweep_finish_dev(fspann_ctx* ctx, int64_t nq, const void* q_dev, int q_dtype, int probe_override, const int64_t* limits, int nl,
                                   int k, int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev,
                                   int32_t* unique_dev, int32_t* bad_dev, int32_t* retried_dev, int64_t* resolved);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_SWEEP_H */
