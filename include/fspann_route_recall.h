/* =============================================================================
 * fspann_route_recall.h — companion of fspann.h: recall attribution, exported by
 * libfspann_hip.so.
 *
 * A true neighbour can go missing in exactly two places.  Route never offered it
 * (a matter of probes and tables), or Route offered it at position j >= B of the
 * candidate list and stage A.5 cut it (QSI:170-214; a matter of refinementLimit).
 * fspann_route_dev with limit = INT32_MAX writes the whole
 * lookupCandidatesWithScores list in the reference's order, and the rank of an id in
 * that list is exactly the refinement limit at which the search starts to score it.
 * One pass over the list per query gives the rank of every ground-truth id, and from
 * the ranks the recall ceiling of Route and the ceiling at any refinement limit —
 * with no candidate row read.
 *
 * The reference wanted this diagnostic: QueryServiceImpl declares trueNearestId,
 * lastTrueNNRank and lastTrueNNSeen and resets them (QSI:63-65, 391-392, 422-423,
 * 438-442), runQueries sets the id and exports both values as profiler columns
 * (FSA:651-658, 740-741) — and nothing ever assigns them.
 *
 * These calls stand in a header of their own for the reason
 * fspann_groundtruth_rows.h gives: the entry points of fspann.h are a counted set
 * (94).  The JVM shim does not bind them.  Conventions are fspann.h's: stream order,
 * no host synchronisation; nq == 0: FSPANN_OK, nothing written; a bad argument is
 * FSPANN_E_ARG with a message naming it.
 * ========================================================================== */
#ifndef FSPANN_ROUTE_RECALL_H
#define FSPANN_ROUTE_RECALL_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The position of every ground-truth id in a list of ids, per query.  list_ids_dev [nq][list_stride] with
 * c = min(list_count_dev[q], list_stride) live entries (list_count_dev NULL: list_stride); gt_ids_dev [nq][gt_stride], of which the
 * first kg are read; rank_dev [nq][kg], gt_score_dev [nq][kg].
 *   rank[q][i]     = the smallest j < c with list_ids[q][j] == gt_ids[q][i], -1 when there is none: a negative ground-truth id (the
 *                    padding of a short row), an id present only at a position >= c, c <= 0.  list_count[q] == -1 — a query Route
 *                    flagged and nobody resolved (fspann_route_resolve_dev) — gives -2 for every i: the list is unknown, which is
 *                    not "not seen".  A ground-truth id that repeats gets the same rank at every copy; of an id the list holds
 *                    twice the smallest position wins.
 *   gt_score[q][i] = list_score[q][rank], -1 where rank < 0: the Hamming score under which Route ranked the true neighbour.
 *                    list_score_dev [nq][list_stride] and gt_score_dev are both given or both NULL.
 * 1 <= kg <= 1024, gt_stride >= kg, 1 <= list_stride <= INT32_MAX.  The list may be Route's full list, sel_ids of a search (the
 * candidates stage A.5 selected, F_q) or the result ids of a search.                                                            */
int fspann_gt_rank_dev(fspann_ctx* ctx, int64_t nq, const int32_t* list_ids_dev, const int32_t* list_score_dev, int64_t list_stride,
                       const int32_t* list_count_dev, const int32_t* gt_ids_dev, int64_t gt_stride, int kg, int32_t* rank_dev,
                       int32_t* gt_score_dev);

/* The recall ceilings the ranks rank_dev [nq][rank_stride] imply.  ks [nk] and limits [nl] are HOST memory: 1 <= nk <= 64 in any
 * order, repeats allowed, 1 <= ks[j] <= rank_stride; 0 <= nl <= 16, strictly ascending, values 1 .. INT32_MAX (limits may be NULL
 * when nl == 0).  hits_dev and ceiling_dev (may be NULL) are planes [nl + 1][nk][nq]:
 *   plane l < nl:  hits = #{ i < ks[j] : 0 <= rank[q][i] < limits[l] }   what a search at refinement limit limits[l] can find
 *   plane nl:      hits = #{ i < ks[j] : rank[q][i] >= 0 }               Route's own ceiling, the limit at infinity
 *   ceiling = hits / (double) ks[j]                                      (the division of FSA:794)
 * A rank of -2 among the first ks[j] gives hits = -1 and ceiling = NaN.                                                          */
int fspann_recall_ceiling_dev(fspann_ctx* ctx, int64_t nq, const int32_t* rank_dev, int64_t rank_stride, const int32_t* ks, int nk,
                              const int64_t* limits, int nl, int32_t* hits_dev, double* ceiling_dev);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_ROUTE_RECALL_H */
