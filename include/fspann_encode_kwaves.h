/* =============================================================================
 * fspann_encode_kwaves.h — companion of fspann.h: the k-wave variant of the MFMA
 * encode for small query batches, exported by libfspann_hip.so.
 *
 * The MFMA encode (fspann_set_encode_mode 2 or 3) gives a query batch one workgroup of
 * four waves per 32 rows x 128 projections, each wave walking all ceil(dim / 32) k
 * tiles alone.  With k-groups set, a query batch runs one workgroup of 4 x groups
 * waves per tile instead: the k tiles are dealt to the groups in turn, the partial
 * sums are joined in LDS in a fixed order, and the epilogue is shared by all the waves
 * (encode_mfma_kwave_kernel).  Hashes and codes are those of every
 * other mode, bit for bit.  It is for batches that leave most CUs without a workgroup.
 *
 * The calls stand in a header of their own for the reason fspann_groundtruth_rows.h
 * gives: the entry points of fspann.h are a counted set (94), and
 * fspann_set_encode_mode keeps its four modes.  The JVM shim does not bind them.
 * Conventions are fspann.h's.
 * ========================================================================== */
#ifndef FSPANN_ENCODE_KWAVES_H
#define FSPANN_ENCODE_KWAVES_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

/* groups: 0 = off (the default), 2 or 4 k-groups of four waves per workgroup; anything else is FSPANN_E_ARG.  A context starts with
 * the value of the environment variable FSPANN_ENCODE_KWAVES, read once when it is made (unset, or not 2 or 4: 0); a clone starts
 * with its source's.  It applies to an encode call when encode mode 2 or 3 chose the MFMA path (never under mode 0), the call codes
 * a query batch (not the rows of a build in progress), the codes have at most three words, and dim > 32 (two k tiles or more);
 * every other call launches what it launches with groups = 0.  Where both apply it goes ahead of mode 3's split over workgroups. */
int fspann_set_encode_kwaves(fspann_ctx* ctx, int groups);

/* The k-groups the context's last encode call ran with; 0 if it ran another kernel.  Negative: an FSPANN_E_* code. */
int fspann_last_encode_kwaves(fspann_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_ENCODE_KWAVES_H */
