// api_groundtruth_mfma.hip.h — the ground truth with the fp32 matrix-core pre-filter (include/fspann_groundtruth_mfma.h): the
// launches of groundtruth_mfma.hip.h over query chunks, the call's one read-back, and the two ways out to gt_rows_run.
// Part of the single translation unit fspann_api.hip (included there behind api_groundtruth.hip.h, whose checks and exact path it
// calls); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_groundtruth_mfma.h"

namespace {

// The ground truth of fp32 queries over rows of type TB (arguments checked by the caller).  ws_gt: GtmState and the survivor counts
// of all nq queries (what the call reads back), |x|^2 [n], then per chunk |q|^2, the thresholds, the survivor lists [chunk x kGtmCap]
// and the [chunk x ld] estimates, every part 256-byte aligned.  The chunk follows gt8_run's rule over the same budget, with the lists
// counted in.  Every kernel of every chunk is launched before anything is known on the host — a flagged call's kernels return at
// once, an overflowed query's finish returns — and ONE synchronisation reads the flag and the counts (gtm_read_back).
template <typename TB>
int gtm_read_back(fspann_ctx* c, const char* w, int64_t n, const TB* base, int64_t nq, const float* q, int dim, int k, int32_t* out_ids, double* out_d2,
                  fspann_gt_mfma_stats* stats);
template <typename TB>
int gtm_run(fspann_ctx* c, int64_t n, const TB* base, int64_t nq, const float* q, int dim, int k, int32_t* out_ids, double* out_d2, fspann_gt_mfma_stats* stats) {
    if (dim > kGtmMaxDim) {
        stats->whole_call_exact = 1;
        stats->queries_exact = nq;
        return gt_rows_run(c, n, base, nq, q, dim, k, out_ids, out_d2);
    }
    auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
    const int64_t ld = (n + 3) & ~int64_t(3);
    const int64_t nbt = (n + kGtmRows - 1) / kGtmRows;
    const int64_t per_q = ld * 4 + int64_t(kGtmCap) * 4;
    int64_t chunk = std::max<int64_t>(32, std::min<int64_t>((nq + 31) / 32 * 32, (c->gt_scratch_bytes / per_q) / 32 * 32));
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(kGtmQ, ((int64_t(1) << 31) - 1) / nbt / 2 * kGtmQ));      // the distance grid stays below 2^31 workgroups
    const size_t head_bytes = up(sizeof(GtmState) + static_cast<size_t>(nq) * 4), xn_bytes = up(static_cast<size_t>(n) * 4), qn_bytes = up(static_cast<size_t>(chunk) * 4);
    const size_t list_bytes = up(static_cast<size_t>(chunk) * kGtmCap * 4);
    int rc = ensure(c, c->ws_gt, head_bytes + xn_bytes + 2 * qn_bytes + list_bytes + static_cast<size_t>(chunk) * ld * 4);
    if (rc) return rc;
    char* w = static_cast<char*>(c->ws_gt.p);
    GtmState* st = reinterpret_cast<GtmState*>(w);
    int32_t* counts = reinterpret_cast<int32_t*>(w + sizeof(GtmState));
    float* xn = reinterpret_cast<float*>(w + head_bytes);
    float* qn = reinterpret_cast<float*>(w + head_bytes + xn_bytes);
    unsigned* thr = reinterpret_cast<unsigned*>(w + head_bytes + xn_bytes + qn_bytes);
    int32_t* lists = reinterpret_cast<int32_t*>(w + head_bytes + xn_bytes + 2 * qn_bytes);
    unsigned* dist = reinterpret_cast<unsigned*>(w + head_bytes + xn_bytes + 2 * qn_bytes + list_bytes);
    // 16 bytes at a time when both matrices allow it (dim % 4 == 0 then, so every chunk of the queries starts aligned as well)
    const bool vec = rows_vec16<TB>(base, dim) && rows_vec16<float>(q, dim);
    hipLaunchKernelGGL(gtm_init_kernel, dim3(1), dim3(1), 0, c->stream, st);
    hipLaunchKernelGGL((vec ? gtm_norm_kernel<TB, true> : gtm_norm_kernel<TB, false>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, c->stream, base, n, dim,
                       xn, st, &st->xmax_bits);
    FSP_HIP(hipGetLastError());
    for (int64_t s = 0; s < nq; s += chunk) {
        const int64_t cq = std::min(chunk, nq - s);
        const float* qs = q + s * dim;
        const int nqb = static_cast<int>((cq + kGtmQ - 1) / kGtmQ);
        hipLaunchKernelGGL((vec ? gtm_norm_kernel<float, true> : gtm_norm_kernel<float, false>), dim3(static_cast<unsigned>((cq + 255) / 256)), dim3(256), 0, c->stream, qs,
                           cq, dim, qn, st, static_cast<unsigned long long*>(nullptr));
        hipLaunchKernelGGL((vec ? gtm_dist_kernel<TB, true> : gtm_dist_kernel<TB, false>), dim3(static_cast<unsigned>(nbt * nqb)), dim3(256), 0, c->stream, base, n, qs, cq,
                           dim, xn, qn, st, dist, ld, nqb);
        FSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(gtm_kth_kernel, dim3(static_cast<unsigned>(cq)), dim3(kGtmSelThreads), 0, c->stream, dist, ld, n, k, dim, qn, st, thr);
        hipLaunchKernelGGL(gtm_collect_kernel, dim3(static_cast<unsigned>(cq)), dim3(kGtmColThreads), 0, c->stream, dist, ld, n, thr, st, lists, counts + s);
        FSP_HIP(hipGetLastError());
        hipLaunchKernelGGL((vec ? gtm_finish_kernel<TB, true> : gtm_finish_kernel<TB, false>), dim3(static_cast<unsigned>(cq)), dim3(kGtmFinThreads), 0, c->stream, base, n,
                           qs, dim, k, lists, counts + s, st, out_ids + s * k, out_d2 ? out_d2 + s * k : nullptr);
        FSP_HIP(hipGetLastError());
    }
    return gtm_read_back(c, w, n, base, nq, q, dim, k, out_ids, out_d2, stats);
}

// The end of a pre-filtered call (this one's and gtm16_run's), behind the launches of all its chunks: the ONE synchronisation, which
// reads the head of ws_gt `w` — GtmState and the nq survivor counts —, and the two ways out to gt_rows_run.
template <typename TB>
int gtm_read_back(fspann_ctx* c, const char* w, int64_t n, const TB* base, int64_t nq, const float* q, int dim, int k, int32_t* out_ids, double* out_d2,
                  fspann_gt_mfma_stats* stats) {
    std::vector<int32_t> host(sizeof(GtmState) / 4 + static_cast<size_t>(nq));
    FSP_HIP(hipMemcpyAsync(host.data(), w, host.size() * 4, hipMemcpyDeviceToHost, c->stream));
    FSP_HIP(hipStreamSynchronize(c->stream));
    GtmState hs;
    std::memcpy(&hs, host.data(), sizeof(hs));
    if (hs.flag) {
        stats->whole_call_exact = 1;
        stats->queries_exact = nq;
        return gt_rows_run(c, n, base, nq, q, dim, k, out_ids, out_d2);
    }
    const int32_t* hc = host.data() + sizeof(GtmState) / 4;
    std::vector<int32_t> over;
    for (int64_t i = 0; i < nq; i++) {
        stats->survivors_total += hc[i];
        stats->survivors_max = std::max<int64_t>(stats->survivors_max, hc[i]);
        if (hc[i] > kGtmCap) over.push_back(static_cast<int32_t>(i));
    }
    stats->queries_exact = static_cast<int64_t>(over.size());
    stats->queries_fast = nq - stats->queries_exact;
    if (over.empty()) return FSPANN_OK;
    // the overflowed queries, contiguous for gt_rows_run (which takes ws_gt: the blocks here are the call's own), and back
    const int64_t m = static_cast<int64_t>(over.size());
    DevPtr<int32_t> idx, tids;
    DevPtr<float> tq;
    DevPtr<double> td2;
    FSP_HIP(dev_alloc(idx, static_cast<size_t>(m) * 4));
    FSP_HIP(dev_alloc(tq, static_cast<size_t>(m) * dim * 4));
    FSP_HIP(dev_alloc(tids, static_cast<size_t>(m) * k * 4));
    FSP_HIP(dev_alloc(td2, static_cast<size_t>(m) * k * 8));
    FSP_HIP(hipMemcpyAsync(idx.get(), over.data(), static_cast<size_t>(m) * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(gtm_gather_kernel, dim3(static_cast<unsigned>(m)), dim3(256), 0, c->stream, q, idx.get(), dim, tq.get());
    FSP_HIP(hipGetLastError());
    int rc = gt_rows_run(c, n, base, m, tq.get(), dim, k, tids.get(), td2.get());
    if (rc == FSPANN_OK) {
        hipLaunchKernelGGL(gtm_scatter_kernel, dim3(static_cast<unsigned>(m)), dim3(256), 0, c->stream, idx.get(), k, tids.get(), td2.get(), out_ids, out_d2);
        rc = hipGetLastError() == hipSuccess ? FSPANN_OK : fail(FSPANN_E_DEVICE, "gtm_scatter_kernel failed to launch");
    }
    const hipError_t e = hipStreamSynchronize(c->stream);      // the blocks above go with this scope
    if (rc == FSPANN_OK && e != hipSuccess) return fail(FSPANN_E_DEVICE, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    return rc;
}

}  // namespace

extern "C" {

int fspann_groundtruth_mfma_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const float* q_dev, int dim, int k,
                                int32_t* out_ids_dev, double* out_d2_dev, fspann_gt_mfma_stats* stats) {
    CHECK_CTX(c);
    fspann_gt_mfma_stats local{};
    if (!stats) stats = &local;
    *stats = fspann_gt_mfma_stats{};
    if (!base_dev || !q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    if (!is_row_dtype(base_dtype) || base_dtype == FSPANN_F64)      // (the words of fspann_groundtruth_rows_dev)
        return fail(FSPANN_E_ARG, "ground truth rows are FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3 (the reference's ground truth reads floats): base %s (%d)",
                    dtype_name(base_dtype), base_dtype);
    int rc = check_gt_shape(n, nq, dim, k);
    if (rc || nq == 0) return rc;
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        if constexpr (DtypeOf<TB>::id != FSPANN_F64) rc = gtm_run(c, n, static_cast<const TB*>(base_dev), nq, q_dev, dim, k, out_ids_dev, out_d2_dev, stats);
    });
    return rc;
}

// The same with the context's resident store as the base.
int fspann_groundtruth_mfma_store_dev(fspann_ctx* c, int64_t nq, const float* q_dev, int k, int32_t* out_ids_dev, double* out_d2_dev, fspann_gt_mfma_stats* stats) {
    CHECK_CTX(c);
    if (stats) *stats = fspann_gt_mfma_stats{};
    if (!q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    return with_store_rows(c, "no ground truth over an FSPANN_F64 store: the reference's ground truth reads floats", [&](int64_t n, const void* rows, int dtype, int dim) {
        return fspann_groundtruth_mfma_dev(c, n, rows, dtype, nq, q_dev, dim, k, out_ids_dev, out_d2_dev, stats);
    });
}

}  // extern "C"
