/* =============================================================================
 * fspann_route_coverage.h — companion of fspann.h: the Route coverage map, exported
 * by libfspann_hip.so.
 *
 * fspann_route_recall.h says whether a lost neighbour was never offered by Route or
 * was cut by stage A.5.  This header breaks the first half down: how many tables,
 * divisions and probes Route needs before it offers the true neighbours, for every
 * (tables, divisions, probes) at once, from one index and one pass.
 *
 *   - Probe order is a prefix.  For one (query, table) the order in which
 *     lookupCandidatesWithScores polls partitions (PIS:643-685) does not depend on
 *     the probe count P; P only cuts that order off.
 *   - A smaller index is a sub-grid.  The GFunction of table (t, d) depends on
 *     seed(t, d) = base + t * 1000003 + d, the sample, m and lambda
 *     (GFunctionRegistry.java:291-293), not on T or D, and partitions are cut per
 *     table.  The index a Setup at (T' <= T, D' <= D) builds is the set of tables
 *     { t * D + d : t < T', d < D' } of the index at (T, D), visited in the same order.
 *
 * So one record per (query, true neighbour, table) — the probe step at which Route
 * reaches the neighbour's partition, and that partition's Hamming score — decides for
 * every (T', D', P) whether Route offers the neighbour and under which score it ranks
 * it.  No candidate row is read, nothing is set up or routed again, and a treeified
 * HashMap bin does not matter: membership does not depend on iteration order.
 *
 * These calls stand in a header of their own for the reason
 * fspann_groundtruth_rows.h gives: the entry points of fspann.h are a counted set
 * (94).  The JVM shim does not bind them.  Conventions are fspann.h's: stream order,
 * no host synchronisation; no allocation beyond the context's grow-on-demand work
 * areas (these two calls use none); nq == 0: FSPANN_OK, nothing written on the device;
 * a bad argument is FSPANN_E_ARG with a message naming it; a context that is not
 * finalized is FSPANN_E_STATE.
 * ========================================================================== */
#ifndef FSPANN_ROUTE_COVERAGE_H
#define FSPANN_ROUTE_COVERAGE_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Where Route reaches every ground-truth id, per table.  codes_dev [nq][T*D][W] (fspann_encode_dev), gt_ids_dev [nq][gt_stride] of
 * which the first kg are read, reach_dev [nq][kg][T*D]:
 *   reach[q][i][td] = (step << 16) | hamming, or -1
 *     step     the 0-based position of the id's partition in the order Route polls table td's partitions for this query: the index
 *              into the probe list of that table at P = probes_max
 *     hamming  that partition's hamming(q, rep): the score the id takes from this table
 * probes_max is literal (it does not go through the probe override or the default probes): 1 <= probes_max <= 32.
 * 1 <= kg <= 1024, gt_stride >= kg.
 * -1 for every table: a negative id (the padding of a short row), an id >= n_ids, an id whose deleted bit is set
 * (collectPartitionOrdered skips it, PIS:736-751; the id range is checked before the bit is read).  -1 for one table: the table
 * does not hold the id, holds it in a partition that is not among the first probes_max polled, or has no partitions (PIS:638).
 * A ground-truth id that repeats gets the same records at every copy.  A table that holds an id in two partitions gives the earlier
 * step, with that step's Hamming; this happens in imported tables only (fspann_set_index), GreedyPartitioner never does it.    */
int fspann_gt_reach_dev(fspann_ctx* ctx, int64_t nq, const uint64_t* codes_dev, int probes_max, const int32_t* gt_ids_dev,
                        int64_t gt_stride, int kg, int32_t* reach_dev);

/* The coverage of nc configurations from the records reach_dev [nq][kg][T*D] of a reach call at probes_max = reach_probes.
 * ks [nk] and grid [nc][3] = {tables, divisions, probes} are HOST memory: 1 <= nk <= 64, 1 <= ks[j] <= kg; 1 <= nc <= 64,
 * 1 <= tables_c <= T, 1 <= divisions_c <= D, 1 <= probes_c <= reach_probes <= 32.
 *   offered(q, i, c)  <=>  there is t < tables_c, d < divisions_c with 0 <= step(q, i, t * D + d) < probes_c
 *   score[c][q][i]    = the minimum hamming over exactly those records, -1 when there is none      (score_dev may be NULL)
 *   hits[c][j][q]     = #{ i < ks[j] : offered(q, i, c) }
 *   ceiling[c][j][q]  = hits / (double) ks[j]     (the division of FSA:794)                       (ceiling_dev may be NULL)
 *   exact[c]          = 1 iff tables_c * divisions_c * probes_c * block_size < HARD_CAP             (host memory, may be NULL)
 * exact is the rule under which Route plans without the cap; it is computed on the host, needs no launch and is written whenever
 * the arguments are valid (also at nq == 0).
 * Where exact[c] = 1, offered is membership in lookupCandidatesWithScores' list of the index (tables_c, divisions_c) at probes_c
 * probes, and score is that entry's score.
 * Where exact[c] = 0, Route may have stopped early (PIS:624,628,657-659): offered is then a superset and ceiling an upper bound. */
int fspann_route_coverage_dev(fspann_ctx* ctx, int64_t nq, const int32_t* reach_dev, int kg, int reach_probes, const int32_t* ks,
                              int nk, const int32_t* grid, int nc, int32_t* hits_dev, double* ceiling_dev, int32_t* score_dev,
                              uint8_t* exact);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_ROUTE_COVERAGE_H */
