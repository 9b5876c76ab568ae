/* =============================================================================
 * fspann_route_plan.h — companion of fspann.h: the plan of a Route call, as a
 * diagnostic, exported by libfspann_hip.so.
 *
 * Which ordering path of the full select a candidate list takes (DESIGN.md,
 * "ordering paths") depends on the plan the library makes for a call — sizes of
 * the hash table, the LDS regions and the sort buffer, the workgroup size — and on
 * the list.  The tests that aim a scene at one path read the plan through this call.
 * It stands in a header of its own for the reason fspann_groundtruth_rows.h gives:
 * the entry points of fspann.h are a counted set (94).  The JVM shim does not bind
 * it.  Conventions are fspann.h's.
 * ========================================================================== */
#ifndef FSPANN_ROUTE_PLAN_H
#define FSPANN_ROUTE_PLAN_H

#include "fspann.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only (nothing is launched or synchronised): the plan fspann_route[_dev] would run with for (probe_override, limit, kept /
 * raw_seen requested or not) under the context's current route mode.
 * out[0..] = ht_size, lds_sort_words, sort_cap, lds_mode, threads, max_tuples, maxcand, nbins, cap0, slice_ht, lazy (1: the bounded
 * select runs first), g_sub (1: the grouped ordering has its sub-key buffer), seq_bits, wave_sort, lazy_cap, probes.
 * Returns the number of fields (16; < 0: an error code) and writes min(n_out, 16) of them.                                       */
int fspann_route_plan_info(fspann_ctx* ctx, int probe_override, int32_t limit, int want_counters, int32_t* out, int n_out);

#ifdef __cplusplus
}
#endif
#endif /* FSPANN_ROUTE_PLAN_H */
