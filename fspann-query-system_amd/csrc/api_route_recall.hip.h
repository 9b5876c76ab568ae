// api_route_recall.hip.h — include/fspann_route_recall.h: the rank of every ground-truth id in a candidate list and the recall
// ceilings the ranks imply (fspann_gt_rank_dev / fspann_recall_ceiling_dev).  Kernels in route_recall.hip.h; semantics, the kernel
// and its LDS budget: DESIGN.md 3.6d.  Neither call allocates or synchronises: checks, one launch.
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_route_recall.h"

extern "C" {

int fspann_gt_rank_dev(fspann_ctx* c, int64_t nq, const int32_t* list_ids_dev, const int32_t* list_score_dev, int64_t list_stride,
                       const int32_t* list_count_dev, const int32_t* gt_ids_dev, int64_t gt_stride, int kg, int32_t* rank_dev, int32_t* gt_score_dev) {
    CHECK_CTX(c);
    if (nq < 0 || nq > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or nq > INT32_MAX");
    if (kg < 1 || kg > kRankMaxKg) return fail(FSPANN_E_ARG, "kg %d: 1 .. %d", kg, kRankMaxKg);
    if (gt_stride < kg) return fail(FSPANN_E_ARG, "gt_stride %lld is below kg %d", static_cast<long long>(gt_stride), kg);
    if (list_stride < 1 || list_stride > INT32_MAX) return fail(FSPANN_E_ARG, "list_stride %lld: 1 .. INT32_MAX", static_cast<long long>(list_stride));
    if ((list_score_dev == nullptr) != (gt_score_dev == nullptr))
        return fail(FSPANN_E_ARG, "list_score_dev and gt_score_dev go together: both or neither");
    if (nq == 0) return FSPANN_OK;
    if (!list_ids_dev) return fail(FSPANN_E_ARG, "list_ids_dev is null");
    if (!gt_ids_dev) return fail(FSPANN_E_ARG, "gt_ids_dev is null");
    if (!rank_dev) return fail(FSPANN_E_ARG, "rank_dev is null");
    if (reinterpret_cast<uintptr_t>(list_ids_dev) & 3) return fail(FSPANN_E_ARG, "list_ids_dev is not aligned to its element");
    const int slots = rank_table_slots(kg);
    hipLaunchKernelGGL(gt_rank_kernel, dim3(static_cast<unsigned>(nq)), dim3(kRankThreads), rank_lds_bytes(kg), c->stream, list_ids_dev, list_score_dev, list_stride,
                       list_count_dev, gt_ids_dev, gt_stride, kg, slots, 32 - __builtin_ctz(static_cast<unsigned>(slots)), rank_dev, gt_score_dev);
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

int fspann_recall_ceiling_dev(fspann_ctx* c, int64_t nq, const int32_t* rank_dev, int64_t rank_stride, const int32_t* ks, int nk, const int64_t* limits,
                              int nl, int32_t* hits_dev, double* ceiling_dev) {
    CHECK_CTX(c);
    if (nq < 0 || nq > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or nq > INT32_MAX");
    if (nk < 1 || nk > kCeilMaxK) return fail(FSPANN_E_ARG, "nk must be in [1, %d]: %d", kCeilMaxK, nk);
    if (!ks) return fail(FSPANN_E_ARG, "ks is null");
    if (nl < 0 || nl > kCeilMaxLimits) return fail(FSPANN_E_ARG, "nl %d: 0 .. %d limits", nl, kCeilMaxLimits);
    if (nl > 0 && !limits) return fail(FSPANN_E_ARG, "limits is null");
    if (rank_stride < 1) return fail(FSPANN_E_ARG, "rank_stride %lld < 1", static_cast<long long>(rank_stride));
    CeilArgs a{};
    a.nk = nk;
    a.nl = nl;
    for (int j = 0; j < nk; j++) {
        if (ks[j] < 1 || ks[j] > rank_stride) return fail(FSPANN_E_ARG, "ks[%d] = %d: k must be in [1, rank_stride = %lld]", j, ks[j], static_cast<long long>(rank_stride));
        a.k[j] = ks[j];
        a.kmax = std::max(a.kmax, ks[j]);
    }
    for (int j = 0; j < nl; j++) {
        if (limits[j] < 1 || limits[j] > INT32_MAX) return fail(FSPANN_E_ARG, "limits[%d] = %lld out of range (1 .. INT32_MAX)", j, static_cast<long long>(limits[j]));
        if (j > 0 && limits[j] <= limits[j - 1]) return fail(FSPANN_E_ARG, "limits must be strictly ascending (limits[%d] = %lld after %lld)", j,
                                                              static_cast<long long>(limits[j]), static_cast<long long>(limits[j - 1]));
        a.limit[j] = static_cast<int32_t>(limits[j]);
    }
    a.limit[nl] = INT32_MAX;
    if (nq == 0) return FSPANN_OK;
    if (!rank_dev) return fail(FSPANN_E_ARG, "rank_dev is null");
    if (!hits_dev) return fail(FSPANN_E_ARG, "hits_dev is null");
    hipLaunchKernelGGL(recall_ceiling_kernel, dim3(static_cast<unsigned>(nq)), dim3(kCeilThreads), 0, c->stream, rank_dev, rank_stride, nq, a, hits_dev, ceiling_dev);
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

}  // extern "C"
