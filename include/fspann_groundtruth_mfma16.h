/* =============================================================================
 * fspann_groundtruth_mfma16.h — companion of fspann.h: the exact ground truth of fp32
 * queries over narrow rows with a pre-filter on the 16-bit matrix cores, exported by
 * libfspann_hip.so.
 *
 * fspann_groundtruth_mfma_dev estimates every distance on the fp32 matrix cores, into
 * which it widens every row element.  Every element of an FSPANN_F16, FSPANN_U8,
 * FSPANN_I8 or FSPANN_F8E4M3 row is a half and every element of an FSPANN_BF16 row a
 * bfloat16, so 16 bytes of such a row are an operand of the f16 / bf16 matrix
 * instructions as they are; the fp32 query is split, once, into two halves or three
 * bfloat16s.  The estimate's error interval is wider than the fp32 one's and proven
 * in the same way; the exact finish and the results are the same:
 * fspann_groundtruth_rows_dev's, bit for bit.
 *
 * A header of its own for the reason fspann_groundtruth_rows.h gives: the entry points
 * of fspann.h are a counted set (94).  The JVM shim does not bind these.  Conventions
 * are fspann.h's.
 * ========================================================================== */
#ifndef FSPANN_GROUNDTRUTH_MFMA16_H
#define FSPANN_GROUNDTRUTH_MFMA16_H

#include "fspann_groundtruth_mfma.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fspann_groundtruth_mfma_dev / fspann_groundtruth_mfma_store_dev for narrow rows: the same arguments, the same results, the same
 * stats (fspann_gt_mfma_stats, unchanged), one synchronisation of the context's stream.  base_dtype is FSPANN_U8, FSPANN_I8,
 * FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3.  FSPANN_F32 rows are refused with FSPANN_E_ARG — an fp32 row is no 16-bit operand:
 * fspann_groundtruth_mfma_dev takes them —, FSPANN_F64 rows in the words of fspann_groundtruth_rows_dev; the store call refuses a
 * store of either type likewise.  Scratch and chunks follow FSPANN_GT_SCRATCH_MB (per query: 4 bytes per base row, the survivor
 * list, and 4 or 6 bytes per dimension for its terms).  stats may be NULL.                                                        */
int fspann_groundtruth_mfma16_dev(fspann_ctx* ctx, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const float* q_dev,
                                  int dim, int k, int32_t* out_ids_dev, double* out_d2_dev, fspann_gt_mfma_stats* stats);
int fspann_groundtruth_mfma16_store_dev(fspann_ctx* ctx, int64_t nq, const float* q_dev, int k, int32_t* out_ids_dev,
                                        double* out_d2_dev, fspann_gt_mfma_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_GROUNDTRUTH_MFMA16_H */
