// api_route_coverage.hip.h — include/fspann_route_coverage.h: where Route reaches every ground-truth id, per table, and the recall
// ceiling of every (tables, divisions, probes) those records imply (fspann_gt_reach_dev / fspann_route_coverage_dev).  Kernels in
// route_coverage.hip.h; semantics, the kernels and their LDS budget: DESIGN.md 3.6e.  Neither call allocates or synchronises:
// checks, one launch.
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_route_coverage.h"

extern "C" {

int fspann_gt_reach_dev(fspann_ctx* c, int64_t nq, const uint64_t* codes_dev, int probes_max, const int32_t* gt_ids_dev, int64_t gt_stride, int kg,
                        int32_t* reach_dev) {
    CHECK_CTX(c);
    if (!c->frozen) return fail(FSPANN_E_STATE, "Index not finalized");
    if (nq < 0 || nq > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or nq > INT32_MAX");
    if (probes_max < 1 || probes_max > kReachMaxProbes) return fail(FSPANN_E_ARG, "probes_max %d: 1 .. %d", probes_max, kReachMaxProbes);
    if (kg < 1 || kg > kRankMaxKg) return fail(FSPANN_E_ARG, "kg %d: 1 .. %d", kg, kRankMaxKg);
    if (gt_stride < kg) return fail(FSPANN_E_ARG, "gt_stride %lld is below kg %d", static_cast<long long>(gt_stride), kg);
    if (nq == 0) return FSPANN_OK;
    if (!codes_dev) return fail(FSPANN_E_ARG, "codes_dev is null");
    if (!gt_ids_dev) return fail(FSPANN_E_ARG, "gt_ids_dev is null");
    if (!reach_dev) return fail(FSPANN_E_ARG, "reach_dev is null");
    const IndexFamily& fam = *c->fam;
    RouteParams p{};                                // what the probe and the id walk read (gt_reach_kernel)
    p.codes = codes_dev; p.tables = fam.d_tables.get(); p.recs = fam.d_recs.get(); p.rec_words = fam.rec_words; p.ids = fam.d_ids.get();
    p.dir = c->knob_probe_dir ? fam.d_dir.get() : nullptr; p.dir_bits = fam.dir_bits;
    p.deleted_bits = fam.d_deleted_bits.load(std::memory_order_acquire);
    p.nq = nq; p.TD = c->TD; p.W = c->W; p.P = probes_max; p.S = c->cfg.block_size; p.n_ids = fam.n_ids;
    const int slots = rank_table_slots(kg);
    hipLaunchKernelGGL(gt_reach_kernel, dim3(static_cast<unsigned>(nq)), dim3(kReachThreads), reach_lds_bytes(kg, probes_max), c->stream, p, gt_ids_dev,
                       gt_stride, kg, slots, 32 - __builtin_ctz(static_cast<unsigned>(slots)), reach_dev);
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

int fspann_route_coverage_dev(fspann_ctx* c, int64_t nq, const int32_t* reach_dev, int kg, int reach_probes, const int32_t* ks, int nk, const int32_t* grid,
                              int nc, int32_t* hits_dev, double* ceiling_dev, int32_t* score_dev, uint8_t* exact) {
    CHECK_CTX(c);
    if (!c->frozen) return fail(FSPANN_E_STATE, "Index not finalized");
    if (nq < 0 || nq > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or nq > INT32_MAX");
    if (kg < 1 || kg > kRankMaxKg) return fail(FSPANN_E_ARG, "kg %d: 1 .. %d", kg, kRankMaxKg);
    if (reach_probes < 1 || reach_probes > kReachMaxProbes) return fail(FSPANN_E_ARG, "reach_probes %d: 1 .. %d", reach_probes, kReachMaxProbes);
    if (nk < 1 || nk > kCovMaxK) return fail(FSPANN_E_ARG, "nk must be in [1, %d]: %d", kCovMaxK, nk);
    if (!ks) return fail(FSPANN_E_ARG, "ks is null");
    if (nc < 1 || nc > kCovMaxConfigs) return fail(FSPANN_E_ARG, "nc must be in [1, %d]: %d", kCovMaxConfigs, nc);
    if (!grid) return fail(FSPANN_E_ARG, "grid is null");
    const int T = c->cfg.tables, D = c->cfg.divisions;
    if (T > UINT16_MAX || D > UINT16_MAX) return fail(FSPANN_E_RANGE, "tables %d or divisions %d beyond %d", T, D, UINT16_MAX);
    CovArgs a{};
    a.nk = nk;
    a.nc = nc;
    for (int j = 0; j < nk; j++) {
        if (ks[j] < 1 || ks[j] > kg) return fail(FSPANN_E_ARG, "ks[%d] = %d: k must be in [1, kg = %d]", j, ks[j], kg);
        a.k[j] = static_cast<uint16_t>(ks[j]);
        a.kmax = std::max(a.kmax, ks[j]);
    }
    for (int i = 0; i < nc; i++) {
        const int32_t* g = grid + 3 * i;
        if (g[0] < 1 || g[0] > T) return fail(FSPANN_E_ARG, "grid[%d]: tables %d: 1 .. %d", i, g[0], T);
        if (g[1] < 1 || g[1] > D) return fail(FSPANN_E_ARG, "grid[%d]: divisions %d: 1 .. %d", i, g[1], D);
        if (g[2] < 1 || g[2] > reach_probes) return fail(FSPANN_E_ARG, "grid[%d]: probes %d: 1 .. reach_probes = %d", i, g[2], reach_probes);
        a.tables[i] = static_cast<uint16_t>(g[0]); a.divisions[i] = static_cast<uint16_t>(g[1]); a.probes[i] = static_cast<uint16_t>(g[2]);
    }
    if (nq > 0 && !reach_dev) return fail(FSPANN_E_ARG, "reach_dev is null");
    if (nq > 0 && !hits_dev) return fail(FSPANN_E_ARG, "hits_dev is null");
    if (exact)                                      // plan_route's need_cap, at the configuration's own tables, divisions and probes
        for (int i = 0; i < nc; i++)
            exact[i] = static_cast<int64_t>(grid[3 * i]) * grid[3 * i + 1] * grid[3 * i + 2] * c->cfg.block_size < c->hard_cap ? 1 : 0;
    if (nq == 0) return FSPANN_OK;
    hipLaunchKernelGGL(route_coverage_kernel, dim3(static_cast<unsigned>(nq)), dim3(kCovThreads), 0, c->stream, reach_dev, kg, c->TD, D, nq, a, hits_dev,
                       ceiling_dev, score_dev);
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

}  // extern "C"
