/* =============================================================================
 * fspann_groundtruth_rows.h — companion of fspann.h: the exact ground truth of fp32
 * queries over typed rows and over the resident store, exported by libfspann_hip.so.
 *
 * The two calls stand in a header of their own because the entry points of fspann.h
 * are a counted set (94: the generated JNI shim and the Python binding table hold
 * exactly those).  They are evaluation calls of the native and the Python side; the
 * JVM shim does not bind them.  Conventions are fspann.h's.
 * ========================================================================== */
#ifndef FSPANN_GROUNDTRUTH_ROWS_H
#define FSPANN_GROUNDTRUTH_ROWS_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ground truth of the fp32 queries searches are made with, over typed rows as they are: what fspann_eval_metrics_typed_dev
 * needs for recall against a resident typed store, with no fp32 copy of the base.  GroundtruthPrecompute.run as
 * fspann_groundtruth_dev states it, a row element being the typed value widened EXACTLY to fp32 (every value of the five row
 * types is a float) and the arithmetic the reference's from there (float subtraction, fp64 squares summed in dimension order):
 * out_ids / out_d2 are bit-identical to fspann_groundtruth_dev over the same values held as fp32, padding (-1 / +inf beyond n)
 * included.  Non-finite rows take part: +-inf gives an infinite distance, NaN sorts last.
 * fspann_groundtruth_rows_dev: base [n][dim] of base_dtype FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3,
 * packed, any alignment, any dim >= 1 (rows that start and end on 16-byte boundaries are read 16 bytes at a time); FSPANN_F32
 * is fspann_groundtruth_dev; FSPANN_F64 or an unknown dtype: FSPANN_E_ARG naming it.  n, dim, k (1..1024) and nq == 0 as in
 * fspann_groundtruth_dev, the same scratch and chunks.
 * fspann_groundtruth_store_dev: the base is the context's resident store (fspann_store_set or fspann_store_attach_dev: its n,
 * its dtype, cfg.dim).  No store: FSPANN_E_STATE.  An FSPANN_F64 store: FSPANN_E_ARG (the reference's ground truth reads
 * floats).  The refusals of fspann_groundtruth_typed_dev stand: that call is the reference's file pairs, these two are not.   */
int fspann_groundtruth_rows_dev(fspann_ctx* ctx, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const float* q_dev,
                                int dim, int k, int32_t* out_ids_dev, double* out_d2_dev);
int fspann_groundtruth_store_dev(fspann_ctx* ctx, int64_t nq, const float* q_dev, int k, int32_t* out_ids_dev, double* out_d2_dev);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_GROUNDTRUTH_ROWS_H */
