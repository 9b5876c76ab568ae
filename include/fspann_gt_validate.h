/* =============================================================================
 * fspann_gt_validate.h — companion of fspann.h: GroundtruthValidator.validate
 * (api/.../GroundtruthValidator.java:81-184, called at FSA:2144-2193), the gate in
 * front of runQueries, exported by libfspann_hip.so.
 *
 * The validator draws a deterministic sample of the queries, finds the nearest base
 * row of each by brute force and compares it with the first id of its ground-truth
 * row; more than `tolerance` of them disagreeing means the ground truth belongs to
 * another dataset (or carries an id offset).  Its arithmetic is NOT the ground
 * truth's: BaseVectorReader.l2sq (:219-242) subtracts in DOUBLE (`double d =
 * query[i] - v`, query a double[]), GroundtruthPrecompute.l2sq in float, and the two
 * can name different rows.  The calls stand in a header of their own for the reason
 * fspann_groundtruth_rows.h gives: the entry points of fspann.h are a counted set
 * (94).  The JVM shim does not bind them.  Conventions are fspann.h's.
 * ========================================================================== */
#ifndef FSPANN_GT_VALIDATE_H
#define FSPANN_GT_VALIDATE_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ValidationResult (GroundtruthValidator.java:30-65) and what the reference prints beside it (FSA:2135, GroundtruthManager). */
typedef struct fspann_gt_validation {
    int32_t valid;            /* !(mismatch_rate > tolerance); 1 when there are no queries, 0 when the ground truth is empty        */
    int32_t consistent;       /* GroundtruthManager.isConsistentWithDatasetSize(n): n > 0 && gt_max_id < n && gt_min_id >= 0         */
    int64_t sample_size;      /* effectiveSample = min(sample_size, nq); 0 on the two early returns                                 */
    int64_t mismatches;
    double mismatch_rate;     /* mismatches / (double) effectiveSample (0 / 0 = NaN, which is valid); 1.0 when the ground truth is empty */
    int32_t n_mismatched;     /* min(mismatches, 10)                                                                                */
    int32_t gt_min_id;        /* over all gt_rows x gt_stride ids, from INT32_MAX (GroundtruthManager.minId)                         */
    int32_t gt_max_id;        /* ... from -1 (GroundtruthManager.maxId)                                                              */
    int32_t reserved;
    int64_t mismatched[10];   /* mismatchedQueries: the first 10 mismatching query indices, in the sample's iteration order         */
} fspann_gt_validation;

/* The validator's sample (:112-121): new Random(42), nextInt(nq) into a HashSet<Integer> until it holds min(sample_size, nq)
 * values, then the set's ITERATION order (java.util.Random's LCG and both branches of nextInt(bound); HashMap's spread hash,
 * default capacity 16, load factor 0.75, growth as values arrive, tree bins included).  No context, no device.
 * out_idx holds min(sample_size, nq) entries; *out_n = that count.  nq <= 0 or sample_size <= 0: *out_n = 0.
 * nq >= 2^31 (no Java int): FSPANN_E_ARG.  out_n null, or out_idx null with something to write: FSPANN_E_NULL.                 */
int fspann_gt_validator_sample(int64_t nq, int64_t sample_size, int64_t* out_idx, int64_t* out_n);

/* BaseVectorReader.bruteForceNN (:252-265) for a list of queries, one fused kernel and no distance matrix.
 * Per (query, row): d = (double) q[i] - (double) v[i], sum = sum + d * d from 0.0 in dimension order (no contraction), every sum
 * bit-identical to the JVM's.  The winner is the first row, in ascending index, whose sum is smaller than every sum before it,
 * from +inf: the lexicographic minimum of (sum, index) among rows with sum < +inf.  A NaN or infinite sum never wins; no such
 * row: index -1, distance +inf.
 * base [n][dim] of base_dtype FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3, every element widened
 * exactly, packed, any alignment, any dim >= 1 (rows that start and end on 16-byte boundaries are read 16 bytes at a time);
 * FSPANN_F64 or an unknown dtype: FSPANN_E_ARG naming it (the reference reads floats or bytes).  0 < n < 2^31.
 * q [nq][dim] of q_dtype FSPANN_F64 (the reference's double[]) or FSPANN_F32 (widened exactly).
 * qsel_dev [nsel] (int64, device) lists the rows of q to run, in any order, repeats allowed; an entry outside [0, nq) gives
 * -1 / +inf.  qsel_dev NULL: the queries 0 .. nsel - 1, and nsel <= nq.
 * out_idx_dev [nsel] int32, out_d2_dev [nsel] fp64 (may be NULL).  nsel == 0: FSPANN_OK, nothing written.
 * Scratch (the widened queries and one partial result per query and workgroup) is bounded by FSPANN_GT_SCRATCH_MB; more queries
 * run in chunks.  Stream order, no host synchronisation.                                                                       */
int fspann_nn1_exact_dev(fspann_ctx* ctx, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype,
                         int dim, const int64_t* qsel_dev, int64_t nsel, int32_t* out_idx_dev, double* out_d2_dev);

/* The same with the context's resident store as the base (its n, its dtype, cfg.dim).  No store: FSPANN_E_STATE.  An FSPANN_F64
 * store: FSPANN_E_ARG.                                                                                                         */
int fspann_nn1_exact_store_dev(fspann_ctx* ctx, int64_t nq, const void* q_dev, int q_dtype, const int64_t* qsel_dev, int64_t nsel,
                               int32_t* out_idx_dev, double* out_d2_dev);

/* GroundtruthValidator.validate, statement for statement, HOST-SYNCHRONOUS.  base / q as fspann_nn1_exact_dev takes them;
 * gt_ids_dev [gt_rows][gt_stride] int32 (device), gt_stride >= 1 when gt_rows > 0; sample_size and tolerance as given (the
 * defaults of FSA:2151-2152 are the caller's).
 *   nq == 0: valid, sample 0 ("No queries to validate").  gt_rows == 0: invalid, sample 0, rate 1.0 ("Groundtruth is empty").
 *   Otherwise the sample of fspann_gt_validator_sample(nq, sample_size) is walked in its order: a query with index >= gt_rows
 *   has no ground truth and is skipped — not a mismatch, but it stays in the denominator (:128-131); any other query is a
 *   mismatch iff gt_ids[qi][0] != its exact nearest row.  mismatch_rate = mismatches / (double) min(sample_size, nq);
 *   valid = !(rate > tolerance).
 * gt_min_id / gt_max_id / consistent are filled on every path.  *out is written only when the call returns FSPANN_OK.          */
int fspann_gt_validate_dev(fspann_ctx* ctx, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype,
                           int dim, const int32_t* gt_ids_dev, int64_t gt_rows, int64_t gt_stride, int64_t sample_size, double tolerance,
                           fspann_gt_validation* out);

/* The same against the resident store (states and refusals of fspann_nn1_exact_store_dev).                                     */
int fspann_gt_validate_store_dev(fspann_ctx* ctx, int64_t nq, const void* q_dev, int q_dtype, const int32_t* gt_ids_dev, int64_t gt_rows,
                                 int64_t gt_stride, int64_t sample_size, double tolerance, fspann_gt_validation* out);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_GT_VALIDATE_H */
