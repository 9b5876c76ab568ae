// api_gt_validate.hip.h — GroundtruthValidator on the device (include/fspann_gt_validate.h): the validator's sample, the exact
// top-1 of a list of queries (gt_validate.hip.h) over rows given by pointer or the resident store, and validate itself.
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_gt_validate.h"
#include "../host/java_random.hpp"

namespace {

// the launch along the rows: every workgroup walks the same number of 256-row tiles (but for the last few), at most kNn1MaxGrid of them
int nn1_grid_x(int64_t n) {
    const int64_t tiles = (n + kGtRows - 1) / kGtRows;
    const int64_t per = (tiles + kNn1MaxGrid - 1) / kNn1MaxGrid;
    return static_cast<int>((tiles + per - 1) / per);
}
// scratch per query of a chunk: its row widened to fp64, and one (sum, row) partial per workgroup
size_t nn1_query_bytes(int64_t n, int dim) { return static_cast<size_t>(dim) * 8 + static_cast<size_t>(nn1_grid_x(n)) * 12; }
// queries per chunk under the context's budget (FSPANN_GT_SCRATCH_MB), whole query tiles, and a grid whose y stays within 65535
int64_t nn1_chunk(const fspann_ctx* c, int64_t n, int dim, int64_t nsel) {
    const int64_t fit = static_cast<int64_t>(static_cast<size_t>(c->gt_scratch_bytes) / nn1_query_bytes(n, dim)) / kGtQT * kGtQT;
    const int64_t all = (nsel + kGtQT - 1) / kGtQT * kGtQT;
    return std::min<int64_t>(std::max<int64_t>(kGtQT, std::min(all, fit)), int64_t(65535) * kGtQT);
}
size_t nn1_scratch_bytes(const fspann_ctx* c, int64_t n, int dim, int64_t nsel) {
    return (static_cast<size_t>(nn1_chunk(c, n, dim, nsel)) * nn1_query_bytes(n, dim) + 255) & ~size_t(255);
}

// The arguments both exact top-1 calls and both validate calls share (every refusal, in one place)
int nn1_check(int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim) {
    if (!base_dev || !q_dev) return fail(FSPANN_E_NULL, "exact top-1 buffer is null");
    if (!is_row_dtype(base_dtype) || base_dtype == FSPANN_F64)      // (FSPANN_F64, or no dtype at all)
        return fail(FSPANN_E_ARG, "exact top-1 rows are FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3 (the reference's validator reads floats or bytes): base %s (%d)",
                    dtype_name(base_dtype), base_dtype);
    if (!is_query_dtype(q_dtype))
        return fail(FSPANN_E_ARG, "exact top-1 queries are FSPANN_F64 (the reference's double[]) or FSPANN_F32: query %s (%d)", dtype_name(q_dtype), q_dtype);
    if (n <= 0 || n >= (1LL << 31) || nq < 0 || dim <= 0) return fail(FSPANN_E_ARG, "Empty or malformed vector files (zero records).");
    return FSPANN_OK;
}

// The launches of fspann_nn1_exact_dev (arguments checked by the caller).  The scratch is ws_gt from byte `head` on; the caller
// that keeps something in front of it has sized ws_gt for head + nn1_scratch_bytes already, so nothing moves here.
template <typename TB>
int nn1_run(fspann_ctx* c, int64_t n, const TB* base, int64_t nq, const void* q, int q_dtype, int dim, const int64_t* qsel, int64_t nsel, int32_t* out_idx,
            double* out_d2, size_t head) {
    const int gx = nn1_grid_x(n);
    const int64_t chunk = nn1_chunk(c, n, dim, nsel);
    int rc = ensure(c, c->ws_gt, head + nn1_scratch_bytes(c, n, dim, nsel));
    if (rc) return rc;
    char* w = static_cast<char*>(c->ws_gt.p) + head;
    double* qd = reinterpret_cast<double*>(w);
    unsigned long long* pkey = reinterpret_cast<unsigned long long*>(w + static_cast<size_t>(chunk) * dim * 8);
    int32_t* pidx = reinterpret_cast<int32_t*>(w + static_cast<size_t>(chunk) * dim * 8 + static_cast<size_t>(chunk) * gx * 8);
    // a lane reads its row 16 bytes at a time when every row starts on a 16-byte boundary and ends on one
    const bool vec = (static_cast<int64_t>(dim) * static_cast<int64_t>(sizeof(TB))) % 16 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
    for (int64_t s = 0; s < nsel; s += chunk) {
        const int64_t cq = std::min(chunk, nsel - s);
        const dim3 wgrid(static_cast<unsigned>(std::min<int64_t>((cq * dim + 255) / 256, 1024)));
        if (q_dtype == FSPANN_F64) hipLaunchKernelGGL(nn1_widen_q_kernel<double>, wgrid, dim3(256), 0, c->stream, static_cast<const double*>(q), nq, dim, qsel, s, cq, qd);
        else hipLaunchKernelGGL(nn1_widen_q_kernel<float>, wgrid, dim3(256), 0, c->stream, static_cast<const float*>(q), nq, dim, qsel, s, cq, qd);
        FSP_HIP(hipGetLastError());
        const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>((cq + kGtQT - 1) / kGtQT));
        if (vec) hipLaunchKernelGGL((nn1_exact_kernel<TB, true>), grid, dim3(kGtRows), 0, c->stream, base, n, qd, cq, dim, pkey, pidx);
        else hipLaunchKernelGGL((nn1_exact_kernel<TB, false>), grid, dim3(kGtRows), 0, c->stream, base, n, qd, cq, dim, pkey, pidx);
        FSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(nn1_reduce_kernel, dim3(static_cast<unsigned>(cq)), dim3(64), 0, c->stream, pkey, pidx, gx, out_idx + s, out_d2 ? out_d2 + s : nullptr);
        FSP_HIP(hipGetLastError());
    }
    return FSPANN_OK;
}

int nn1_dispatch(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim, const int64_t* qsel,
                 int64_t nsel, int32_t* out_idx, double* out_d2, size_t head) {
    int rc = FSPANN_OK;
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        if constexpr (DtypeOf<TB>::id != FSPANN_F64)
            rc = nn1_run(c, n, static_cast<const TB*>(base_dev), nq, q_dev, q_dtype, dim, qsel, nsel, out_idx, out_d2, head);
    });
    return rc;
}

int nn1_exact(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim, const int64_t* qsel_dev,
              int64_t nsel, int32_t* out_idx_dev, double* out_d2_dev) {
    int rc = nn1_check(n, base_dev, base_dtype, nq, q_dev, q_dtype, dim);
    if (rc) return rc;
    if (nsel < 0 || (!qsel_dev && nsel > nq)) return fail(FSPANN_E_ARG, "nsel must be >= 0, and <= nq without a selection list");
    if (nsel == 0) return FSPANN_OK;
    if (!out_idx_dev) return fail(FSPANN_E_NULL, "exact top-1 buffer is null");
    return nn1_dispatch(c, n, base_dev, base_dtype, nq, q_dev, q_dtype, dim, qsel_dev, nsel, out_idx_dev, out_d2_dev, 0);
}

// validate (GroundtruthValidator.java:81-184) with the arguments checked
int gt_validate(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim, const int32_t* gt_ids_dev,
                int64_t gt_rows, int64_t gt_stride, int64_t sample_size, double tolerance, fspann_gt_validation* out) {
    if (!out) return fail(FSPANN_E_NULL, "out is null");
    int rc = nn1_check(n, base_dev, base_dtype, nq, q_dev, q_dtype, dim);
    if (rc) return rc;
    if (nq >= (1LL << 31)) return fail(FSPANN_E_ARG, "nq %lld is no Java int: the validator's sample is Random.nextInt(nq)", static_cast<long long>(nq));
    if (gt_rows < 0 || (gt_rows > 0 && (gt_stride < 1 || !gt_ids_dev))) return fail(FSPANN_E_ARG, "gt_ids must be [gt_rows][gt_stride >= 1]");
    fspann_gt_validation v{};
    const bool run = nq > 0 && gt_rows > 0;      // neither early return (:94-101)
    std::vector<int64_t> sel;
    if (run) sel = jdk::gt_validator_sample(nq, sample_size);
    const int64_t ns = static_cast<int64_t>(sel.size());
    // ws_gt: the result block | the sample | its nearest rows | the scratch of the exact top-1
    const size_t sel_bytes = (static_cast<size_t>(ns) * 8 + 255) & ~size_t(255), nn_bytes = (static_cast<size_t>(ns) * 4 + 255) & ~size_t(255);
    const size_t head = 256 + sel_bytes + nn_bytes;
    rc = ensure(c, c->ws_gt, head + (ns > 0 ? nn1_scratch_bytes(c, n, dim, ns) : 0));
    if (rc) return rc;
    char* w = static_cast<char*>(c->ws_gt.p);
    GtCompareOut* res = reinterpret_cast<GtCompareOut*>(w);
    int64_t* sel_dev = reinterpret_cast<int64_t*>(w + 256);
    int32_t* nn_dev = reinterpret_cast<int32_t*>(w + 256 + sel_bytes);
    if (ns > 0) {
        FSP_HIP(hipMemcpyAsync(sel_dev, sel.data(), static_cast<size_t>(ns) * 8, hipMemcpyHostToDevice, c->stream));
        rc = nn1_dispatch(c, n, base_dev, base_dtype, nq, q_dev, q_dtype, dim, sel_dev, ns, nn_dev, nullptr, head);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(gt_compare_kernel, dim3(1), dim3(64), 0, c->stream, sel_dev, ns, nn_dev, gt_ids_dev, gt_rows, gt_stride, res);
    FSP_HIP(hipGetLastError());
    const int64_t count = gt_rows * gt_stride;
    if (count > 0) {
        hipLaunchKernelGGL(gt_id_range_kernel, dim3(static_cast<unsigned>(std::min<int64_t>((count + 255) / 256, 1024))), dim3(256), 0, c->stream, gt_ids_dev, count, res);
        FSP_HIP(hipGetLastError());
    }
    GtCompareOut h{};
    FSP_HIP(hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    FSP_HIP(hipStreamSynchronize(c->stream));
    v.gt_min_id = h.min_id;
    v.gt_max_id = h.max_id;
    v.consistent = (n > 0 && h.max_id < n && h.min_id >= 0) ? 1 : 0;      // GroundtruthManager.java:222-243
    if (nq == 0) {
        v.valid = 1;                                                      // "No queries to validate"
    } else if (gt_rows == 0) {
        v.valid = 0;                                                      // "Groundtruth is empty"
        v.mismatch_rate = 1.0;
    } else {
        const int64_t effective = std::min(sample_size, nq);              // (as given: 0 makes the rate 0 / 0 = NaN, which is valid)
        v.sample_size = effective;
        v.mismatches = h.mismatches;
        v.n_mismatched = h.n_mismatched;
        for (int i = 0; i < h.n_mismatched && i < 10; i++) v.mismatched[i] = h.mismatched[i];
        v.mismatch_rate = static_cast<double>(h.mismatches) / static_cast<double>(effective);
        v.valid = (v.mismatch_rate > tolerance) ? 0 : 1;
    }
    *out = v;
    return FSPANN_OK;
}

}  // namespace

extern "C" {

int fspann_gt_validator_sample(int64_t nq, int64_t sample_size, int64_t* out_idx, int64_t* out_n) {
    return guarded([&]() -> int {
        if (!out_n) return fail(FSPANN_E_NULL, "out_n is null");
        *out_n = 0;
        if (nq <= 0 || sample_size <= 0) return FSPANN_OK;
        if (nq >= (1LL << 31)) return fail(FSPANN_E_ARG, "nq %lld is no Java int: the validator's sample is Random.nextInt(nq)", static_cast<long long>(nq));
        if (!out_idx) return fail(FSPANN_E_NULL, "out_idx is null");
        const std::vector<int64_t> sel = jdk::gt_validator_sample(nq, sample_size);
        std::copy(sel.begin(), sel.end(), out_idx);
        *out_n = static_cast<int64_t>(sel.size());
        return FSPANN_OK;
    });
}

int fspann_nn1_exact_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim,
                         const int64_t* qsel_dev, int64_t nsel, int32_t* out_idx_dev, double* out_d2_dev) {
    return guarded([&]() -> int {
        CHECK_CTX(c);
        return nn1_exact(c, n, base_dev, base_dtype, nq, q_dev, q_dtype, dim, qsel_dev, nsel, out_idx_dev, out_d2_dev);
    });
}

int fspann_nn1_exact_store_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, const int64_t* qsel_dev, int64_t nsel, int32_t* out_idx_dev,
                               double* out_d2_dev) {
    return guarded([&]() -> int {
        CHECK_CTX(c);
        if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
        if (c->store->dtype == FSPANN_F64) return fail(FSPANN_E_ARG, "no exact top-1 over an FSPANN_F64 store: the reference's validator reads floats or bytes");
        return nn1_exact(c, c->store->n, c->store->rows, c->store->dtype, nq, q_dev, q_dtype, c->cfg.dim, qsel_dev, nsel, out_idx_dev, out_d2_dev);
    });
}

int fspann_gt_validate_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim,
                           const int32_t* gt_ids_dev, int64_t gt_rows, int64_t gt_stride, int64_t sample_size, double tolerance, fspann_gt_validation* out) {
    return guarded([&]() -> int {
        CHECK_CTX(c);
        return gt_validate(c, n, base_dev, base_dtype, nq, q_dev, q_dtype, dim, gt_ids_dev, gt_rows, gt_stride, sample_size, tolerance, out);
    });
}

int fspann_gt_validate_store_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, const int32_t* gt_ids_dev, int64_t gt_rows, int64_t gt_stride,
                                 int64_t sample_size, double tolerance, fspann_gt_validation* out) {
    return guarded([&]() -> int {
        CHECK_CTX(c);
        if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
        if (c->store->dtype == FSPANN_F64) return fail(FSPANN_E_ARG, "no exact top-1 over an FSPANN_F64 store: the reference's validator reads floats or bytes");
        return gt_validate(c, c->store->n, c->store->rows, c->store->dtype, nq, q_dev, q_dtype, c->cfg.dim, gt_ids_dev, gt_rows, gt_stride, sample_size, tolerance, out);
    });
}

}  // extern "C"
