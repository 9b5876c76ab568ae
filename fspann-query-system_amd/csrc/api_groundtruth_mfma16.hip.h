// api_groundtruth_mfma16.hip.h — the ground truth with the pre-filter on the 16-bit matrix cores
// (include/fspann_groundtruth_mfma16.h): the launches of groundtruth_mfma16.hip.h over query chunks.  The base norms, the
// collection, the exact finish, the call's one read-back and the two ways out are api_groundtruth_mfma.hip.h's.
// Part of the single translation unit fspann_api.hip (included there behind api_groundtruth_mfma.hip.h); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_groundtruth_mfma16.h"

namespace {

// gtm_run for rows of a type TB whose elements are halves or bfloat16s.  ws_gt as there, and per chunk also the epilogue factors
// [chunk] and the queries' term planes [T][chunk][kpad] of 16-bit values, kpad = dim rounded up to kGtm16KPad; the chunk follows the
// same rule with the planes counted in.
template <typename TB>
int gtm16_run(fspann_ctx* c, int64_t n, const TB* base, int64_t nq, const float* q, int dim, int k, int32_t* out_ids, double* out_d2, fspann_gt_mfma_stats* stats) {
    if (dim > kGtmMaxDim) {
        stats->whole_call_exact = 1;
        stats->queries_exact = nq;
        return gt_rows_run(c, n, base, nq, q, dim, k, out_ids, out_d2);
    }
    constexpr int T = Gtm16Op<TB>::T;
    constexpr bool bf = std::is_same<TB, fsp_bf16>::value;
    auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
    const int kpad = (dim + kGtm16KPad - 1) / kGtm16KPad * kGtm16KPad;
    const int64_t ld = (n + 3) & ~int64_t(3);
    const int64_t nbt = (n + kGtm16Rows - 1) / kGtm16Rows;
    const int64_t per_q = ld * 4 + int64_t(kGtmCap) * 4 + int64_t(T) * kpad * 2;
    int64_t chunk = std::max<int64_t>(32, std::min<int64_t>((nq + 31) / 32 * 32, (c->gt_scratch_bytes / per_q) / 32 * 32));
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(kGtmQ, ((int64_t(1) << 31) - 1) / nbt / 2 * kGtmQ));      // the distance grid stays below 2^31 workgroups
    const size_t head_bytes = up(sizeof(GtmState) + static_cast<size_t>(nq) * 4), xn_bytes = up(static_cast<size_t>(n) * 4), qn_bytes = up(static_cast<size_t>(chunk) * 4);
    const size_t list_bytes = up(static_cast<size_t>(chunk) * kGtmCap * 4), plane_bytes = up(static_cast<size_t>(T) * chunk * kpad * 2);
    const int64_t plane_stride = chunk * kpad;
    int rc = ensure(c, c->ws_gt, head_bytes + xn_bytes + 3 * qn_bytes + list_bytes + plane_bytes + static_cast<size_t>(chunk) * ld * 4);
    if (rc) return rc;
    char* w = static_cast<char*>(c->ws_gt.p);
    GtmState* st = reinterpret_cast<GtmState*>(w);
    int32_t* counts = reinterpret_cast<int32_t*>(w + sizeof(GtmState));
    char* at = w + head_bytes;
    auto take = [&](size_t bytes) { char* p = at; at += bytes; return p; };
    float* xn = reinterpret_cast<float*>(take(xn_bytes));
    float* qn = reinterpret_cast<float*>(take(qn_bytes));
    float* qsc = reinterpret_cast<float*>(take(qn_bytes));
    unsigned* thr = reinterpret_cast<unsigned*>(take(qn_bytes));
    int32_t* lists = reinterpret_cast<int32_t*>(take(list_bytes));
    uint16_t* planes = reinterpret_cast<uint16_t*>(take(plane_bytes));
    unsigned* dist = reinterpret_cast<unsigned*>(at);
    const bool vec = rows_vec16<TB>(base, dim);           // (the queries are read by element once, in the split; the planes are always aligned)
    hipLaunchKernelGGL(gtm_init_kernel, dim3(1), dim3(1), 0, c->stream, st);
    hipLaunchKernelGGL((vec ? gtm_norm_kernel<TB, true> : gtm_norm_kernel<TB, false>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, c->stream, base, n, dim,
                       xn, st, &st->xmax_bits);
    FSP_HIP(hipGetLastError());
    for (int64_t s = 0; s < nq; s += chunk) {
        const int64_t cq = std::min(chunk, nq - s);
        const float* qs = q + s * dim;
        const int nqb = static_cast<int>((cq + kGtmQ - 1) / kGtmQ);
        hipLaunchKernelGGL(gtm16_split_kernel<bf>, dim3(static_cast<unsigned>((cq + 3) / 4)), dim3(256), 0, c->stream, qs, cq, dim, kpad, qn, qsc, planes, plane_stride, st);
        hipLaunchKernelGGL((vec ? gtm16_dist_kernel<TB, true> : gtm16_dist_kernel<TB, false>), dim3(static_cast<unsigned>(nbt * nqb)), dim3(256), 0, c->stream, base, n,
                           planes, plane_stride, kpad, cq, dim, xn, qn, qsc, st, dist, ld, nqb);
        FSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(gtm16_kth_kernel, dim3(static_cast<unsigned>(cq)), dim3(kGtmSelThreads), 0, c->stream, dist, ld, n, k, dim, T, qn, qsc, st, thr);
        hipLaunchKernelGGL(gtm_collect_kernel, dim3(static_cast<unsigned>(cq)), dim3(kGtmColThreads), 0, c->stream, dist, ld, n, thr, st, lists, counts + s);
        FSP_HIP(hipGetLastError());
        hipLaunchKernelGGL((vec ? gtm_finish_kernel<TB, true> : gtm_finish_kernel<TB, false>), dim3(static_cast<unsigned>(cq)), dim3(kGtmFinThreads), 0, c->stream, base, n,
                           qs, dim, k, lists, counts + s, st, out_ids + s * k, out_d2 ? out_d2 + s * k : nullptr);
        FSP_HIP(hipGetLastError());
    }
    return gtm_read_back(c, w, n, base, nq, q, dim, k, out_ids, out_d2, stats);
}

}  // namespace

extern "C" {

int fspann_groundtruth_mfma16_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const float* q_dev, int dim, int k,
                                  int32_t* out_ids_dev, double* out_d2_dev, fspann_gt_mfma_stats* stats) {
    CHECK_CTX(c);
    fspann_gt_mfma_stats local{};
    if (!stats) stats = &local;
    *stats = fspann_gt_mfma_stats{};
    if (!base_dev || !q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    if (base_dtype == FSPANN_F32)
        return fail(FSPANN_E_ARG, "an FSPANN_F32 row is no operand of the 16-bit matrix cores: fspann_groundtruth_mfma_dev takes fp32 rows (this call: FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16, FSPANN_F8E4M3)");
    if (!is_row_dtype(base_dtype) || base_dtype == FSPANN_F64)      // (the words of fspann_groundtruth_rows_dev)
        return fail(FSPANN_E_ARG, "ground truth rows are FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3 (the reference's ground truth reads floats): base %s (%d)",
                    dtype_name(base_dtype), base_dtype);
    int rc = check_gt_shape(n, nq, dim, k);
    if (rc || nq == 0) return rc;
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        if constexpr (sizeof(TB) <= 2) rc = gtm16_run(c, n, static_cast<const TB*>(base_dev), nq, q_dev, dim, k, out_ids_dev, out_d2_dev, stats);
    });
    return rc;
}

// The same with the context's resident store as the base.
int fspann_groundtruth_mfma16_store_dev(fspann_ctx* c, int64_t nq, const float* q_dev, int k, int32_t* out_ids_dev, double* out_d2_dev, fspann_gt_mfma_stats* stats) {
    CHECK_CTX(c);
    if (stats) *stats = fspann_gt_mfma_stats{};
    if (!q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    return with_store_rows(c, "no ground truth over an FSPANN_F64 store: the reference's ground truth reads floats", [&](int64_t n, const void* rows, int dtype, int dim) {
        return fspann_groundtruth_mfma16_dev(c, n, rows, dtype, nq, q_dev, dim, k, out_ids_dev, out_d2_dev, stats);
    });
}

}  // extern "C"
