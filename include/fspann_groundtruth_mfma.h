/* =============================================================================
 * fspann_groundtruth_mfma.h — companion of fspann.h: the exact ground truth of fp32
 * queries over typed rows with an fp32 pre-filter on the matrix cores, exported by
 * libfspann_hip.so.
 *
 * fspann_groundtruth_rows_dev runs the reference's fp64 chain for every (query, row,
 * element).  These calls estimate every distance in fp32 on the matrix cores, keep per
 * query the rows that a proven error interval cannot exclude from its top-k, and run
 * the reference's chain on those alone.  The results are the other
 * call's, bit for bit.
 *
 * The calls stand in a header of their own for the reason fspann_groundtruth_rows.h
 * gives: the entry points of fspann.h are a counted set (94).  The JVM shim does not
 * bind them.  Conventions are fspann.h's.
 * ========================================================================== */
#ifndef FSPANN_GROUNDTRUTH_MFMA_H
#define FSPANN_GROUNDTRUTH_MFMA_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What a call did (host memory, filled when the call returns).
 * queries_fast      queries answered from their survivor list
 * queries_exact     queries finished by the exact path of fspann_groundtruth_rows_dev: those with more survivors than a list
 *                   holds (4096: heavy ties, degenerate data), or all nq of a call with whole_call_exact
 * survivors_max, survivors_total   rows per query that the pre-filter could not exclude, over the call's queries (0 with
 *                   whole_call_exact)
 * whole_call_exact  1: the base or the queries hold a non-finite element, a squared norm above 2^120, or dim > 65536; the
 *                   error interval does not cover those and the whole call went to the exact path                            */
typedef struct fspann_gt_mfma_stats {
    int64_t queries_fast;
    int64_t queries_exact;
    int64_t survivors_max;
    int64_t survivors_total;
    int32_t whole_call_exact;
    int32_t reserved;
} fspann_gt_mfma_stats;

/* fspann_groundtruth_rows_dev / fspann_groundtruth_store_dev by another method: the same arguments, the same refusals in the same
 * words, and out_ids / out_d2 bit-identical to theirs for every input they accept — padding (-1 / +inf beyond n), NaN and +-inf
 * rows, ties by lower id, k up to 1024, every row type they take (FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16,
 * FSPANN_F8E4M3).  Scratch and chunks follow FSPANN_GT_SCRATCH_MB (4 bytes per query and base row, and the survivor lists).
 * Unlike those calls this one synchronises the context's stream once, to read how many survivors each query had (what the exact path then
 * finishes follows in stream order, as in those calls).  stats may be NULL.                                                                            */
int fspann_groundtruth_mfma_dev(fspann_ctx* ctx, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const float* q_dev,
                                int dim, int k, int32_t* out_ids_dev, double* out_d2_dev, fspann_gt_mfma_stats* stats);
int fspann_groundtruth_mfma_store_dev(fspann_ctx* ctx, int64_t nq, const float* q_dev, int k, int32_t* out_ids_dev,
                                      double* out_d2_dev, fspann_gt_mfma_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_GROUNDTRUTH_MFMA_H */
