// api_groundtruth.hip.h — the exact-scan calls over rows given by pointer or the resident store: ground truth, recall and distance
// ratio at one k and at every k of a list, their argument checks and the one rule for the (row, query) dtype pairs the metrics take.
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_groundtruth_rows.h"     // the two ground-truth calls over typed rows (not part of fspann.h's counted set)
#include "../../include/fspann_eval.h"

namespace {

// A lane reads its row of TB 16 bytes at a time when every row starts on a 16-byte boundary and ends on one.
template <typename TB> bool rows_vec16(const void* base, int dim) { return (static_cast<int64_t>(dim) * sizeof(TB)) % 16 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0; }

// The context's resident store as the rows of an exact scan: body(n, rows, dtype, dim).  `no_f64`: the caller's sentence for an FSPANN_F64 store.
template <class F> int with_store_rows(fspann_ctx* c, const char* no_f64, F&& body) {
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    if (c->store->dtype == FSPANN_F64) return fail(FSPANN_E_ARG, "%s", no_f64);
    return body(c->store->n, c->store->rows, c->store->dtype, c->cfg.dim);
}

// The pairs the metrics take: fp32 queries (what searches are made with) over every row type but FSPANN_F64, and a byte type over
// itself.  f(DtypeTag<TB>{}, DtypeTag<TQ>{}) for such a pair; false: any other pair, f was not called (the caller words the error).
template <class F> bool with_metric_pair(int base_dtype, int q_dtype, F&& f) {
    bool taken = false;
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        if constexpr (DtypeOf<TB>::finite) if (q_dtype == base_dtype) { f(tb, tb); taken = true; }
        if constexpr (DtypeOf<TB>::id != FSPANN_F64) if (q_dtype == FSPANN_F32) { f(tb, DtypeTag<float>{}); taken = true; }
    });
    return taken;
}

// n, nq, dim and k of a ground-truth call.  `byte_rows`: the dtype's name on the integer path, whose distances must fit 32 bits.
int check_gt_shape(int64_t n, int64_t nq, int dim, int k, const char* byte_rows = nullptr) {
    if (n <= 0 || n >= (1LL << 31) || nq < 0 || dim <= 0) return fail(FSPANN_E_ARG, "Empty or malformed vector files (zero records).");
    if (byte_rows && dim > kGt8MaxDim) return fail(FSPANN_E_ARG, "dim %d > %d: %s distances would not fit 32 bits", dim, kGt8MaxDim, byte_rows);
    if (k <= 0 || k > kGtMaxK) return fail(FSPANN_E_ARG, "k must be in [1, %d]", kGtMaxK);
    return FSPANN_OK;
}

// The arguments of a metrics call, at one k or at the largest of several: the buffers, the dtype pair (refused by name), the shape.
int check_metrics_args(int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim, int k, const int32_t* ann_ids_dev,
                       int64_t ann_stride, const int32_t* gt_ids_dev, int64_t gt_stride, const double* recall_dev, const double* ratio_dev) {
    if (!base_dev || !q_dev || !ann_ids_dev || !gt_ids_dev || !recall_dev || !ratio_dev) return fail(FSPANN_E_NULL, "metrics buffer is null");
    if (!with_metric_pair(base_dtype, q_dtype, [](auto, auto) {})) {
        for (const DtypeInfo& r : kDtypes) {       // the row-only types that are refused by name, in the table's order
            if (!r.words || (base_dtype != r.id && q_dtype != r.id)) continue;
            if (r.finite)
                return fail(FSPANN_E_ARG, "metrics take %s rows with %s / FSPANN_F32 queries only (a signed byte pairs with nothing else): base %s, query %s", r.name, r.name,
                            dtype_name(base_dtype), dtype_name(q_dtype));
            return fail(FSPANN_E_ARG, "metrics take %s rows with FSPANN_F32 queries only (a query is never %s): base %s, query %s", r.name, r.name, dtype_name(base_dtype),
                        dtype_name(q_dtype));
        }
        return fail(FSPANN_E_ARG, "metrics take FSPANN_F32 rows with FSPANN_F32 queries, or FSPANN_U8 rows with FSPANN_U8 / FSPANN_F32 queries: base %s, query %s",
                    dtype_name(base_dtype), dtype_name(q_dtype));
    }
    if (n <= 0 || nq < 0 || dim <= 0 || k <= 0 || k > kGtMaxK || gt_stride < k || ann_stride <= 0) return fail(FSPANN_E_ARG, "k must be in [1, %d] and gt must hold >= k ids per query", kGtMaxK);
    return FSPANN_OK;
}

// The ground truth of fp32 queries over rows of type TB (arguments checked by the caller): gt_dist_kernel fills a [chunk x n] fp64
// distance matrix in scratch, at most the context's budget at a time (FSPANN_GT_SCRATCH_MB, 8 GiB) and a grid whose y dimension
// stays within 65535 query tiles, and gt_select_kernel picks every query's k.
template <typename TB>
int gt_rows_run(fspann_ctx* c, int64_t n, const TB* base, int64_t nq, const float* q, int dim, int k, int32_t* out_ids, double* out_d2) {
    int64_t chunk = std::max<int64_t>(kGtQT, std::min<int64_t>(nq, (c->gt_scratch_bytes / (n * 8)) / kGtQT * kGtQT));
    chunk = std::min<int64_t>(chunk, int64_t(65535) * kGtQT);
    int rc = ensure(c, c->ws_gt, static_cast<size_t>(chunk) * n * 8);
    if (rc) return rc;
    double* dist = static_cast<double*>(c->ws_gt.p);
    auto dist_kernel = gt_dist_kernel<TB, false>;      // fp32 rows: element loads
    if constexpr (DtypeOf<TB>::id != FSPANN_F32)
        if (rows_vec16<TB>(base, dim)) dist_kernel = gt_dist_kernel<TB, true>;
    for (int64_t s = 0; s < nq; s += chunk) {
        const int64_t cq = std::min(chunk, nq - s);
        dim3 grid(static_cast<unsigned>((n + kGtRows - 1) / kGtRows), static_cast<unsigned>((cq + kGtQT - 1) / kGtQT));
        hipLaunchKernelGGL(dist_kernel, grid, dim3(kGtRows), 0, c->stream, base, n, q + s * dim, cq, dim, dist);
        FSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(gt_select_kernel, dim3(static_cast<unsigned>(cq)), dim3(kGtSelThreads), 0, c->stream, dist, n, k, out_ids + s * k,
                           out_d2 ? out_d2 + s * k : nullptr);
        FSP_HIP(hipGetLastError());
    }
    return FSPANN_OK;
}

int gt8_digits(uint64_t v) {      // 8-bit digits that hold v
    int nd = 1;
    while (nd < 4 && (v >> (8 * nd)) != 0) nd++;
    return nd;
}

// The ground truth of byte queries over byte rows of the same type TB (uint8_t or int8_t; arguments checked by the caller):
// integer distances on the int8 matrix cores (groundtruth_u8.hip.h).
template <typename TB>
int gt8_run(fspann_ctx* c, int64_t n, const TB* base, int64_t nq, const TB* q, int dim, int k, int32_t* out_ids, double* out_d2) {
    // scratch: |x'|^2 [n], |q'|^2 [chunk], then the [chunk x ld] uint32 distances, every part 256-byte aligned, rows 16-byte aligned
    const int64_t ld = (n + 3) & ~int64_t(3);
    const int64_t nbt = (n + kGt8Rows - 1) / kGt8Rows;
    int64_t chunk = std::max<int64_t>(32, std::min<int64_t>((nq + 31) / 32 * 32, (c->gt_scratch_bytes / (ld * 4)) / 32 * 32));
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(kGt8Q, ((int64_t(1) << 31) - 1) / nbt / 2 * kGt8Q));      // the distance grid stays below 2^31 workgroups
    const size_t xn_bytes = (static_cast<size_t>(n) * 4 + 255) & ~size_t(255);
    const size_t qn_bytes = (static_cast<size_t>(chunk) * 4 + 255) & ~size_t(255);
    int rc = ensure(c, c->ws_gt, xn_bytes + qn_bytes + static_cast<size_t>(chunk) * ld * 4);
    if (rc) return rc;
    unsigned* xn = static_cast<unsigned*>(c->ws_gt.p);
    unsigned* qn = reinterpret_cast<unsigned*>(static_cast<char*>(c->ws_gt.p) + xn_bytes);
    unsigned* dist = reinterpret_cast<unsigned*>(static_cast<char*>(c->ws_gt.p) + xn_bytes + qn_bytes);
    // rows that start at odd addresses (dim % 16, or either matrix off a 16-byte boundary) take the byte-load instantiation
    const bool aligned = rows_vec16<TB>(base, dim) && rows_vec16<TB>(q, dim);
    const int ndd = gt8_digits(static_cast<uint64_t>(dim) * 255 * 255), ndi = gt8_digits(static_cast<uint64_t>(n - 1));
    auto xnorm_kernel = aligned ? gt8_norm_kernel<TB, true> : gt8_norm_kernel<TB, false>;
    hipLaunchKernelGGL(xnorm_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, c->stream, base, n, dim, xn);
    FSP_HIP(hipGetLastError());
    for (int64_t s = 0; s < nq; s += chunk) {
        const int64_t cq = std::min(chunk, nq - s);
        const TB* qs = q + s * dim;
        const bool qal = aligned && rows_vec16<TB>(qs, dim);      // (dim % 16 == 0: every chunk starts aligned)
        const int nqb = static_cast<int>((cq + kGt8Q - 1) / kGt8Q);
        auto qnorm_kernel = qal ? gt8_norm_kernel<TB, true> : gt8_norm_kernel<TB, false>;
        auto dist_kernel = qal ? gt8_dist_kernel<TB, true> : gt8_dist_kernel<TB, false>;
        hipLaunchKernelGGL(qnorm_kernel, dim3(static_cast<unsigned>((cq + 255) / 256)), dim3(256), 0, c->stream, qs, cq, dim, qn);
        hipLaunchKernelGGL(dist_kernel, dim3(static_cast<unsigned>(nbt * nqb)), dim3(256), 0, c->stream, base, n, qs, cq, dim, xn, qn, dist, ld, nqb);
        FSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(gt8_select_kernel, dim3(static_cast<unsigned>(cq)), dim3(kGt8SelThreads), 0, c->stream, dist, ld, n, k, ndd, ndi, out_ids + s * k,
                           out_d2 ? out_d2 + s * k : nullptr);
        FSP_HIP(hipGetLastError());
    }
    return FSPANN_OK;
}

}  // namespace

extern "C" {

// ---- exact ground truth (groundtruth.hip.h, groundtruth_u8.hip.h) -------------------------------------------------------------
// Ground truth of fp32 queries over typed rows: the element widened exactly, then one arithmetic and one select for every row type.
int fspann_groundtruth_rows_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const float* q_dev, int dim, int k,
                                int32_t* out_ids_dev, double* out_d2_dev) {
    CHECK_CTX(c);
    if (!base_dev || !q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    if (!is_row_dtype(base_dtype) || base_dtype == FSPANN_F64)      // (FSPANN_F64, or no dtype at all)
        return fail(FSPANN_E_ARG, "ground truth rows are FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3 (the reference's ground truth reads floats): base %s (%d)",
                    dtype_name(base_dtype), base_dtype);
    int rc = check_gt_shape(n, nq, dim, k);
    if (rc || nq == 0) return rc;
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        if constexpr (DtypeOf<TB>::id != FSPANN_F64) rc = gt_rows_run(c, n, static_cast<const TB*>(base_dev), nq, q_dev, dim, k, out_ids_dev, out_d2_dev);
    });
    return rc;
}

int fspann_groundtruth_dev(fspann_ctx* c, int64_t n, const float* base_dev, int64_t nq, const float* q_dev, int dim, int k, int32_t* out_ids_dev,
                           double* out_d2_dev) {
    return fspann_groundtruth_rows_dev(c, n, base_dev, FSPANN_F32, nq, q_dev, dim, k, out_ids_dev, out_d2_dev);
}

// The same with the context's resident store as the base.
int fspann_groundtruth_store_dev(fspann_ctx* c, int64_t nq, const float* q_dev, int k, int32_t* out_ids_dev, double* out_d2_dev) {
    CHECK_CTX(c);
    if (!q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    return with_store_rows(c, "no ground truth over an FSPANN_F64 store: the reference's ground truth reads floats", [&](int64_t n, const void* rows, int dtype, int dim) {
        return fspann_groundtruth_rows_dev(c, n, rows, dtype, nq, q_dev, dim, k, out_ids_dev, out_d2_dev);
    });
}

// Base and query of one type, as the reference reads them from files.  (U8, U8) and (I8, I8): integer distances on the int8 matrix cores.
int fspann_groundtruth_typed_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim, int k,
                                 int32_t* out_ids_dev, double* out_d2_dev) {
    CHECK_CTX(c);
    if (!base_dev || !q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    for (const DtypeInfo& r : kDtypes)     // the reference reads base and query from files of one type, floats or bytes: and a query is never a half, a bfloat16 or an fp8
        if (!r.query && !r.finite && (base_dtype == r.id || q_dtype == r.id))
            return fail(FSPANN_E_ARG, "no ground truth over %s (base and query are both FSPANN_F32 or both FSPANN_U8): base %s, query %s", r.name, dtype_name(base_dtype),
                        dtype_name(q_dtype));
    // (FSPANN_I8 pairs with FSPANN_I8 only: signed with unsigned bytes, or with floats, is a pair that does not match)
    if (base_dtype != q_dtype || (base_dtype != FSPANN_F32 && base_dtype != FSPANN_U8 && base_dtype != FSPANN_I8))
        return fail(FSPANN_E_ARG, "Base and query types must match (both fvecs or both bvecs): base %s, query %s", dtype_name(base_dtype), dtype_name(q_dtype));
    if (base_dtype == FSPANN_F32) return fspann_groundtruth_rows_dev(c, n, base_dev, FSPANN_F32, nq, static_cast<const float*>(q_dev), dim, k, out_ids_dev, out_d2_dev);
    int rc = check_gt_shape(n, nq, dim, k, dtype_name(base_dtype));
    if (rc || nq == 0) return rc;
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        if constexpr (DtypeOf<TB>::finite) rc = gt8_run(c, n, static_cast<const TB*>(base_dev), nq, static_cast<const TB*>(q_dev), dim, k, out_ids_dev, out_d2_dev);
    });
    return rc;
}

// ---- evaluation metrics (groundtruth.hip.h, eval_sweep.hip.h) -------------------------------------------------------------------
// Recall and distance ratio at k over a resident typed store, without an fp32 copy (every element is exact in fp64).
int fspann_eval_metrics_typed_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim, int k,
                                  const int32_t* ann_ids_dev, int64_t ann_stride, const int32_t* ann_count_dev, const int32_t* gt_ids_dev,
                                  int64_t gt_stride, double* recall_dev, double* ratio_dev) {
    CHECK_CTX(c);
    int rc = check_metrics_args(n, base_dev, base_dtype, nq, q_dev, q_dtype, dim, k, ann_ids_dev, ann_stride, gt_ids_dev, gt_stride, recall_dev, ratio_dev);
    if (rc || nq == 0) return rc;
    with_metric_pair(base_dtype, q_dtype, [&](auto tb, auto tq) {
        using TB = typename decltype(tb)::type;
        using TQ = typename decltype(tq)::type;
        hipLaunchKernelGGL((gt_metrics_kernel<TB, TQ>), dim3(static_cast<unsigned>(nq)), dim3(64), 0, c->stream, static_cast<const TB*>(base_dev), n,
                           static_cast<const TQ*>(q_dev), dim, k, ann_ids_dev, ann_stride, ann_count_dev, gt_ids_dev, gt_stride, recall_dev, ratio_dev);
    });
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

int fspann_eval_metrics_dev(fspann_ctx* c, int64_t n, const float* base_dev, int64_t nq, const float* q_dev, int dim, int k, const int32_t* ann_ids_dev,
                            int64_t ann_stride, const int32_t* ann_count_dev, const int32_t* gt_ids_dev, int64_t gt_stride, double* recall_dev,
                            double* ratio_dev) {
    return fspann_eval_metrics_typed_dev(c, n, base_dev, FSPANN_F32, nq, q_dev, FSPANN_F32, dim, k, ann_ids_dev, ann_stride, ann_count_dev, gt_ids_dev, gt_stride,
                                         recall_dev, ratio_dev);
}

// computeMetricsAtK for every k of ks from one result list, in one launch (include/fspann_eval.h).
int fspann_eval_kvariants_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim,
                              const int32_t* ks, int nk, const int32_t* ann_ids_dev, int64_t ann_stride, const int32_t* ann_count_dev,
                              const int32_t* gt_ids_dev, int64_t gt_stride, const int32_t* unique_dev, double* recall_dev, double* ratio_dev,
                              double* cand_ratio_dev) {
    CHECK_CTX(c);
    if (!ks) return fail(FSPANN_E_NULL, "ks is null");
    if (nk < 1 || nk > kEvalMaxK) return fail(FSPANN_E_ARG, "nk must be in [1, %d]: %d", kEvalMaxK, nk);
    EvalKs kv{};
    int kmax = 0;
    for (int j = 0; j < nk; j++) {
        if (ks[j] <= 0 || ks[j] > kGtMaxK) return fail(FSPANN_E_ARG, "ks[%d] = %d: k must be in [1, %d]", j, ks[j], kGtMaxK);
        kv.k[j] = ks[j];
        kmax = std::max(kmax, ks[j]);
    }
    if ((unique_dev == nullptr) != (cand_ratio_dev == nullptr))
        return fail(FSPANN_E_ARG, "unique_dev and cand_ratio_dev go together: both or neither");
    // (a bad nq is refused below, in this call's own words and behind every other refusal: the shared check is given none to judge)
    if (int rc = check_metrics_args(n, base_dev, base_dtype, 0, q_dev, q_dtype, dim, kmax, ann_ids_dev, ann_stride, gt_ids_dev, gt_stride, recall_dev, ratio_dev)) return rc;
    if (nq < 0 || nq > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or nq > INT32_MAX");
    if (nq == 0) return FSPANN_OK;
    const size_t lds = eval_lds_bytes(dim, kmax);      // at most 32 KB of query + 24 KB at kmax = 1024
    with_metric_pair(base_dtype, q_dtype, [&](auto tb, auto tq) {
        using TB = typename decltype(tb)::type;
        using TQ = typename decltype(tq)::type;
        // 16 bytes at a time when the rows allow it and the query is in LDS
        auto kernel = rows_vec16<TB>(base_dev, dim) && dim <= kEvalQLdsMax ? eval_kvariants_kernel<TB, TQ, true> : eval_kvariants_kernel<TB, TQ, false>;
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(nq)), dim3(kEvalThreads), lds, c->stream, static_cast<const TB*>(base_dev), n,
                           static_cast<const TQ*>(q_dev), dim, nq, kv, nk, kmax, ann_ids_dev, ann_stride, ann_count_dev, gt_ids_dev, gt_stride, unique_dev,
                           recall_dev, ratio_dev, cand_ratio_dev);
    });
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

}  // extern "C"
