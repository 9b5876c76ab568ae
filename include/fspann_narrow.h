/* =============================================================================
 * fspann_narrow.h — companion of fspann.h: lossless row narrowing on the device,
 * exported by libfspann_hip.so.
 *
 * The narrow row types of fspann.h (FSPANN_U8, _I8, _F8E4M3, _F16, _BF16) make the
 * Refine scan read fewer bytes with bit-identical results — for a caller who knows
 * that the data is, say, byte-valued and converts it on the host.  The data the
 * reference reads is SIFT .fvecs, integers 0..255 held as floats and widened to
 * double[] by its loaders; a JVM integrator hands over fp64 rows.  These calls
 * decide ON THE GPU which row types hold a block of fp32 or fp64 rows exactly,
 * re-pack the rows, and let a resident store narrow itself in place.
 *
 * The library never rounds, shifts or scales: a type is taken only when EVERY
 * element already is a value of it, so every search, ground-truth and metric result
 * is bit-identical before and after.  A value of a type, per type:
 *   FSPANN_U8      an integer in 0..255 (-0.0 counts as 0)
 *   FSPANN_I8      an integer in -128..127
 *   FSPANN_F8E4M3  NaN; or finite with |x| <= 448, a multiple of 2^-9, at most four
 *                  significant bits (-0.0 keeps its sign; +-inf is none)
 *   FSPANN_F16, FSPANN_BF16, FSPANN_F32
 *                  x survives the round trip by value; +-inf and NaN do
 * NaN and +-inf are never values of the byte types.  A NaN narrows to some NaN of the
 * target type (rows holding one are skipped, not scored).
 *
 * Source dtypes are FSPANN_F32 and FSPANN_F64; any other dtype is FSPANN_E_ARG
 * naming it.  `allowed` is a mask of (1u << FSPANN_x), 0 = every type; the source's
 * own type is always a candidate.  "Narrowest" is: fewest bytes per element; among
 * the one-byte types FSPANN_U8, then _I8, then _F8E4M3 (the byte types never need a
 * finite test in the scan); among the two-byte types FSPANN_F16, then _BF16; then
 * FSPANN_F32; then the source itself.
 *
 * These calls stand in a header of their own for the reason
 * fspann_groundtruth_rows.h gives: the entry points of fspann.h are a counted set
 * (94).  The JVM shim does not bind them.  Conventions are fspann.h's.
 * ========================================================================== */
#ifndef FSPANN_NARROW_H
#define FSPANN_NARROW_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fspann_fit {
    uint32_t fits;             /* bit (1u << FSPANN_x): every element is exactly a value of that type; the source's own bit (and that of a wider type) is always set */
    int32_t  narrowest;        /* the type the order above picks among fits & allowed */
    int64_t  first_misfit[8];  /* per dtype id: flat index row * dim + col of the first element that is not a value of it, -1 if it fits */
    int64_t  nonfinite;        /* elements that are NaN or +-inf */
} fspann_fit;

/* Which row types hold the packed rows rows_dev [n][dim] of dtype (device memory, any alignment) exactly: one streaming
 * pass.  row_fits_dev [n] (device, may be NULL) receives one byte per row, bit FSPANN_x set when the whole row fits that type.
 * Synchronises the context's stream and fills *out (host).                                                                      */
int fspann_rows_fit_dev(fspann_ctx* ctx, int64_t n, const void* rows_dev, int dtype, int dim, uint32_t allowed, uint8_t* row_fits_dev,
                        fspann_fit* out);

/* src_dev [n][dim] of src_dtype re-packed as dst_dev [n][dim] of the narrower dst_dtype (else FSPANN_E_ARG), one pass; both in
 * device memory (src_dev at any alignment, dst_dev aligned to its element), not overlapping.  Synchronises.  If an element is not a value of dst_dtype the call
 * returns FSPANN_E_ARG with a message naming the type, the count and the first index, *misfits (host, may be NULL) is that count,
 * and the contents of dst_dev are unspecified; otherwise *misfits = 0.                                                          */
int fspann_rows_narrow_dev(fspann_ctx* ctx, int64_t n, const void* src_dev, int src_dtype, int dim, void* dst_dev, int dst_dtype,
                           int64_t* misfits);

/* fspann_rows_fit_dev over the context's resident store.  A store of a row-only type is not scanned: fits is its own bit,
 * narrowest its type, nonfinite -1.  No store: FSPANN_E_STATE.                                                                   */
int fspann_store_fit(fspann_ctx* ctx, uint32_t allowed, fspann_fit* out);

/* The resident store re-packed as the narrowest allowed type that holds it: the fit pass, then the narrow pass into a fresh
 * allocation; the store's pointer and dtype are swapped under the context's lock and the old rows freed.  *dtype_out (may be NULL)
 * is the store's dtype afterwards.  When nothing narrower fits, or the store already is a row-only type, it is left untouched
 * (FSPANN_OK).  Handles keep their meaning: touch tracking, fspann_set_deleted and the frozen index are unaffected.
 * FSPANN_E_STATE: no store; a store shared with clones (destroy them first); an attached, caller-owned store (narrow into a
 * buffer of your own with fspann_rows_narrow_dev and attach that).                                                               */
int fspann_store_narrow(fspann_ctx* ctx, uint32_t allowed, int* dtype_out);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_NARROW_H */
