// api_misc.hip.h — ground truth + metrics, the multi-GPU top-k merge, HBM read-peak probes, device memory helpers
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_groundtruth_rows.h"     // the two ground-truth calls over typed rows (not part of fspann.h's counted set)

namespace {
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
    // a lane reads its typed row 16 bytes at a time when every row starts on a 16-byte boundary and ends on one; fp32 rows: element loads
    auto dist_kernel = gt_dist_kernel<TB, false>;
    if constexpr (DtypeOf<TB>::id != FSPANN_F32)
        if ((static_cast<int64_t>(dim) * static_cast<int64_t>(sizeof(TB))) % 16 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0) dist_kernel = gt_dist_kernel<TB, true>;
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
}  // namespace
extern "C" {

// ---- exact ground truth + evaluation metrics (groundtruth.hip.h) -------------------------------------------------------------
int fspann_groundtruth_dev(fspann_ctx* c, int64_t n, const float* base_dev, int64_t nq, const float* q_dev, int dim, int k, int32_t* out_ids_dev,
                           double* out_d2_dev) {
    CHECK_CTX(c);
    if (!base_dev || !q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    if (n <= 0 || n >= (1LL << 31) || nq < 0 || dim <= 0) return fail(FSPANN_E_ARG, "Empty or malformed vector files (zero records).");
    if (k <= 0 || k > kGtMaxK) return fail(FSPANN_E_ARG, "k must be in [1, %d]", kGtMaxK);
    if (nq == 0) return FSPANN_OK;
    return gt_rows_run(c, n, base_dev, nq, q_dev, dim, k, out_ids_dev, out_d2_dev);
}

// (Every check stands before the `nq == 0` return, and nq == 0 launches nothing: fspann_eval_kvariants_dev, api_eval.hip.h, runs
// fspann_eval_metrics_typed_dev with nq = 0 as ITS argument check.  Keep that order here and there.)
int fspann_eval_metrics_dev(fspann_ctx* c, int64_t n, const float* base_dev, int64_t nq, const float* q_dev, int dim, int k, const int32_t* ann_ids_dev,
                            int64_t ann_stride, const int32_t* ann_count_dev, const int32_t* gt_ids_dev, int64_t gt_stride, double* recall_dev,
                            double* ratio_dev) {
    CHECK_CTX(c);
    if (!base_dev || !q_dev || !ann_ids_dev || !gt_ids_dev || !recall_dev || !ratio_dev) return fail(FSPANN_E_NULL, "metrics buffer is null");
    if (n <= 0 || nq < 0 || dim <= 0 || k <= 0 || k > kGtMaxK || gt_stride < k || ann_stride <= 0) return fail(FSPANN_E_ARG, "k must be in [1, %d] and gt must hold >= k ids per query", kGtMaxK);
    if (nq == 0) return FSPANN_OK;
    hipLaunchKernelGGL((gt_metrics_kernel<float, float>), dim3(static_cast<unsigned>(nq)), dim3(64), 0, c->stream, base_dev, n, q_dev, dim, k, ann_ids_dev, ann_stride,
                       ann_count_dev, gt_ids_dev, gt_stride, recall_dev, ratio_dev);
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

}  // extern "C"
namespace {
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
    // rows that start at odd addresses (dim % 16, or a matrix off a 16-byte boundary) take the byte-load instantiation
    const bool aligned = (dim % 16 == 0) && ((reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(q)) & 15) == 0;
    const int ndd = gt8_digits(static_cast<uint64_t>(dim) * 255 * 255), ndi = gt8_digits(static_cast<uint64_t>(n - 1));
    auto xnorm_kernel = aligned ? gt8_norm_kernel<TB, true> : gt8_norm_kernel<TB, false>;
    hipLaunchKernelGGL(xnorm_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, c->stream, base, n, dim, xn);
    FSP_HIP(hipGetLastError());
    for (int64_t s = 0; s < nq; s += chunk) {
        const int64_t cq = std::min(chunk, nq - s);
        const TB* qs = q + s * dim;
        const bool qal = aligned && (reinterpret_cast<uintptr_t>(qs) & 15) == 0;      // (dim % 16 == 0: every chunk starts aligned)
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

// Ground truth over typed rows.  (U8, U8) and (I8, I8): integer distances on the int8 matrix cores (groundtruth_u8.hip.h).
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
    if (base_dtype == FSPANN_F32)
        return fspann_groundtruth_dev(c, n, static_cast<const float*>(base_dev), nq, static_cast<const float*>(q_dev), dim, k, out_ids_dev, out_d2_dev);
    if (n <= 0 || n >= (1LL << 31) || nq < 0 || dim <= 0) return fail(FSPANN_E_ARG, "Empty or malformed vector files (zero records).");
    if (dim > kGt8MaxDim) return fail(FSPANN_E_ARG, "dim %d > %d: %s distances would not fit 32 bits", dim, kGt8MaxDim, dtype_name(base_dtype));
    if (k <= 0 || k > kGtMaxK) return fail(FSPANN_E_ARG, "k must be in [1, %d]", kGtMaxK);
    if (nq == 0) return FSPANN_OK;
    int rc = FSPANN_OK;
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        if constexpr (DtypeOf<TB>::finite) rc = gt8_run(c, n, static_cast<const TB*>(base_dev), nq, static_cast<const TB*>(q_dev), dim, k, out_ids_dev, out_d2_dev);
    });
    return rc;
}

// This function is also the argument check of fspann_eval_kvariants_dev (api_eval.hip.h), which calls it with nq = 0 and relies on
// two things: every refusal below (null buffers, the dtype pair, n, dim, k, the strides) is decided BEFORE the `nq == 0` return,
// on both branches (the FSPANN_F32 one forwards to fspann_eval_metrics_dev), and nq == 0 launches nothing.  A check added or
// moved behind that return is a check the one-launch call loses; tests/test_gpu_eval_kvariants.py::test_refusals holds both
// calls to the same refusals.
int fspann_eval_metrics_typed_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const void* q_dev, int q_dtype, int dim, int k,
                                  const int32_t* ann_ids_dev, int64_t ann_stride, const int32_t* ann_count_dev, const int32_t* gt_ids_dev,
                                  int64_t gt_stride, double* recall_dev, double* ratio_dev) {
    CHECK_CTX(c);
    if (!base_dev || !q_dev || !ann_ids_dev || !gt_ids_dev || !recall_dev || !ratio_dev) return fail(FSPANN_E_NULL, "metrics buffer is null");
    // The pairs: fp32 queries (what searches are made with) over every row type but FSPANN_F64, and a byte type over itself.
    const DtypeInfo* bi = dtype_info(base_dtype);
    const bool same_bytes = bi && bi->finite && q_dtype == base_dtype;
    if (!(same_bytes || (bi && q_dtype == FSPANN_F32 && base_dtype != FSPANN_F64))) {
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
    if (base_dtype == FSPANN_F32)
        return fspann_eval_metrics_dev(c, n, static_cast<const float*>(base_dev), nq, static_cast<const float*>(q_dev), dim, k, ann_ids_dev, ann_stride,
                                       ann_count_dev, gt_ids_dev, gt_stride, recall_dev, ratio_dev);
    if (n <= 0 || nq < 0 || dim <= 0 || k <= 0 || k > kGtMaxK || gt_stride < k || ann_stride <= 0) return fail(FSPANN_E_ARG, "k must be in [1, %d] and gt must hold >= k ids per query", kGtMaxK);
    if (nq == 0) return FSPANN_OK;
    // a resident typed store: recall and ratio without an fp32 copy (every element is exact in fp64)
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        auto go = [&](auto tq) {
            using TQ = typename decltype(tq)::type;
            hipLaunchKernelGGL((gt_metrics_kernel<TB, TQ>), dim3(static_cast<unsigned>(nq)), dim3(64), 0, c->stream, static_cast<const TB*>(base_dev), n,
                               static_cast<const TQ*>(q_dev), dim, k, ann_ids_dev, ann_stride, ann_count_dev, gt_ids_dev, gt_stride, recall_dev, ratio_dev);
        };
        if constexpr (DtypeOf<TB>::finite) { if (same_bytes) go(tb); else go(DtypeTag<float>{}); }
        else if constexpr (!DtypeOf<TB>::query) go(DtypeTag<float>{});
    });
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

// Ground truth of fp32 queries over typed rows: the element widened exactly, then fspann_groundtruth_dev's arithmetic and select.
int fspann_groundtruth_rows_dev(fspann_ctx* c, int64_t n, const void* base_dev, int base_dtype, int64_t nq, const float* q_dev, int dim, int k,
                                int32_t* out_ids_dev, double* out_d2_dev) {
    CHECK_CTX(c);
    if (!base_dev || !q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    if (base_dtype == FSPANN_F32) return fspann_groundtruth_dev(c, n, static_cast<const float*>(base_dev), nq, q_dev, dim, k, out_ids_dev, out_d2_dev);
    if (!is_row_dtype(base_dtype) || is_query_dtype(base_dtype))      // (FSPANN_F64, or no dtype at all)
        return fail(FSPANN_E_ARG, "ground truth rows are FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3 (the reference's ground truth reads floats): base %s (%d)",
                    dtype_name(base_dtype), base_dtype);
    if (n <= 0 || n >= (1LL << 31) || nq < 0 || dim <= 0) return fail(FSPANN_E_ARG, "Empty or malformed vector files (zero records).");
    if (k <= 0 || k > kGtMaxK) return fail(FSPANN_E_ARG, "k must be in [1, %d]", kGtMaxK);
    if (nq == 0) return FSPANN_OK;
    int rc = FSPANN_OK;
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        if constexpr (!DtypeOf<TB>::query) rc = gt_rows_run(c, n, static_cast<const TB*>(base_dev), nq, q_dev, dim, k, out_ids_dev, out_d2_dev);
    });
    return rc;
}

// The same with the context's resident store as the base (fspann_store_set or fspann_store_attach_dev; its n, dtype and cfg.dim).
int fspann_groundtruth_store_dev(fspann_ctx* c, int64_t nq, const float* q_dev, int k, int32_t* out_ids_dev, double* out_d2_dev) {
    CHECK_CTX(c);
    if (!q_dev || !out_ids_dev) return fail(FSPANN_E_NULL, "ground truth buffer is null");
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    if (c->store->dtype == FSPANN_F64) return fail(FSPANN_E_ARG, "no ground truth over an FSPANN_F64 store: the reference's ground truth reads floats");
    return fspann_groundtruth_rows_dev(c, c->store->n, c->store->rows, c->store->dtype, nq, q_dev, c->cfg.dim, k, out_ids_dev, out_d2_dev);
}

// ---- multi-GPU merge: one RCCL all-gather of the packed per-rank top-k -------------------------------
size_t fspann_topk_bytes(int64_t nq, int k) {
    if (nq < 0 || k <= 0) return 0;
    const size_t idb = (static_cast<size_t>(nq) * k * 4 + 7) & ~size_t(7);     // keeps the fp64 part 8-byte aligned
    return idb + static_cast<size_t>(nq) * k * 8;
}
size_t fspann_topk_dist_offset(int64_t nq, int k) {
    if (nq < 0 || k <= 0) return 0;
    return (static_cast<size_t>(nq) * k * 4 + 7) & ~size_t(7);
}

int fspann_comm_available(void) { return rccl_api() ? 1 : 0; }

int fspann_comm_unique_id(void* id_out) {
    if (!id_out) return fail(FSPANN_E_NULL, "id_out is null");
    RcclApi* a = rccl_api();
    if (!a) return fail(FSPANN_E_STATE, "librccl not found (set FSPANN_RCCL_LIB): %s", dlerror() ? dlerror() : "no candidate loaded");
    RcclApi::UniqueId id;
    const int rc = a->GetUniqueId(&id);
    if (rc != 0) return fail(FSPANN_E_DEVICE, "ncclGetUniqueId: %s", rccl_err(a, rc));
    std::memcpy(id_out, &id, sizeof(id));
    return FSPANN_OK;
}

int fspann_comm_create(fspann_ctx* c, const void* unique_id, int world, int rank, fspann_comm** out) {
    CHECK_CTX(c);
    if (!unique_id || !out) return fail(FSPANN_E_NULL, "unique_id/out is null");
    *out = nullptr;
    if (world <= 0 || rank < 0 || rank >= world) return fail(FSPANN_E_ARG, "bad world %d / rank %d", world, rank);
    RcclApi* a = rccl_api();
    if (!a) return fail(FSPANN_E_STATE, "librccl not found (set FSPANN_RCCL_LIB)");
    RcclApi::UniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    fspann_comm* m = new (std::nothrow) fspann_comm();
    if (!m) return fail(FSPANN_E_NOMEM, "out of host memory");
    const int rc = a->CommInitRank(&m->nccl, world, id, rank);     // on the context's device (CHECK_CTX made it current)
    if (rc != 0) {
        delete m;
        return fail(FSPANN_E_DEVICE, "ncclCommInitRank(world %d, rank %d): %s", world, rank, rccl_err(a, rc));
    }
    m->ctx = c; m->world = world; m->rank = rank;
    c->comm_refs.fetch_add(1);
    *out = m;
    return FSPANN_OK;
}

int fspann_comm_destroy(fspann_comm* m) {
    if (!m) return FSPANN_OK;
    RcclApi* a = rccl_api();
    if (a && m->nccl) {
        if (m->ctx) { (void)hipSetDevice(m->ctx->device); (void)hipStreamSynchronize(m->ctx->stream); }
        (void)a->CommDestroy(m->nccl);
    }
    fspann_ctx* c = m->ctx;
    delete m;
    // the context was destroyed while this communicator held it: the last holder finishes that destroy
    if (c && c->comm_refs.fetch_sub(1) == 1 && c->destroy_deferred.exchange(false)) fspann_ctx_destroy(c);
    return FSPANN_OK;
}

int fspann_comm_info(fspann_comm* m, int* world, int* rank, const char** library) {
    if (!m) return fail(FSPANN_E_NULL, "comm is null");
    if (world) *world = m->world;
    if (rank) *rank = m->rank;
    if (library) { RcclApi* a = rccl_api(); *library = a ? a->path.c_str() : ""; }
    return FSPANN_OK;
}

// gathered_dev = world x fspann_topk_bytes(nq_local, k), in rank order = global query order when the batch was cut into
// contiguous equal shards (the last one padded with id -1 / +inf, which Refine writes for missing results anyway).
int fspann_allgather_topk_dev(fspann_comm* m, int64_t nq_local, int k, const void* local_packed_dev, void* gathered_dev) {
    if (!m || !m->ctx) return fail(FSPANN_E_NULL, "comm is null");
    CHECK_CTX(m->ctx);
    if (!local_packed_dev || !gathered_dev) return fail(FSPANN_E_NULL, "top-k buffer is null");
    const size_t nb = fspann_topk_bytes(nq_local, k);
    if (nb == 0) return fail(FSPANN_E_ARG, "nq_local < 0 or k <= 0");
    RcclApi* a = rccl_api();
    if (!a) return fail(FSPANN_E_STATE, "librccl not found");
    const int rc = a->AllGather(local_packed_dev, gathered_dev, nb, 0 /* ncclInt8 */, m->nccl, m->ctx->stream);
    if (rc != 0) return fail(FSPANN_E_DEVICE, "ncclAllGather: %s", rccl_err(a, rc));
    return FSPANN_OK;
}

// Measurement aid (bench.py `roofline.peak_measured`): the rate at which THIS device streams `bytes` of HBM through a
// pure 16-byte-load kernel (buffer owned by the library, larger than the 256 MiB Infinity Cache when bytes says so).
}  // extern "C"
namespace {
typedef unsigned int hbm_u32x4 __attribute__((ext_vector_type(4)));
template <bool kNT>   // kNT: the loads carry the nt policy (read-once data, as the refinement scan's row stream)
__global__ __launch_bounds__(256) void hbm_read_kernel(const hbm_u32x4* __restrict__ p, size_t n16, unsigned long long* __restrict__ sink) {
    hbm_u32x4 acc = {0, 0, 0, 0};
    const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const hbm_u32x4 v = kNT ? __builtin_nontemporal_load(p + i) : p[i];
        acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w;
    }
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9E3779B9u) atomicAdd(sink, 1ull);   // keeps the loads alive; practically never taken
}
}  // namespace
extern "C" {
int fspann_hbm_read_peak(fspann_ctx* c, size_t bytes, int reps, double* gb_per_s) {
    CHECK_CTX(c);
    if (!gb_per_s || reps <= 0 || bytes < (1u << 20)) return fail(FSPANN_E_ARG, "bytes < 1 MiB, reps <= 0 or null output");
    void* buf = nullptr;
    unsigned long long* sink = nullptr;
    FSP_HIP(hipMalloc(&buf, bytes));
    if (hipMalloc(&sink, 8) != hipSuccess) { (void)hipFree(buf); return fail(FSPANN_E_NOMEM, "hipMalloc failed"); }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = FSPANN_OK;
    do {
        if (hipMemsetAsync(buf, 0x5A, bytes, c->stream) != hipSuccess || hipMemsetAsync(sink, 0, 8, c->stream) != hipSuccess ||
            hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { rc = fail(FSPANN_E_DEVICE, "setup failed"); break; }
        const unsigned grid = static_cast<unsigned>(c->num_cus) * 8;
        const hbm_u32x4* src = static_cast<const hbm_u32x4*>(buf);
        double best = 0.0;
        for (int nt = 0; nt < 2 && rc == FSPANN_OK; nt++) {      // default cache policy and nt: the ceiling is the better of the two
            for (int r = -1; r < reps; r++) {                    // r = -1: warm-up
                (void)hipEventRecord(e0, c->stream);
                if (nt) hipLaunchKernelGGL(hbm_read_kernel<true>, dim3(grid), dim3(256), 0, c->stream, src, bytes / 16, sink);
                else hipLaunchKernelGGL(hbm_read_kernel<false>, dim3(grid), dim3(256), 0, c->stream, src, bytes / 16, sink);
                (void)hipEventRecord(e1, c->stream);
                if (hipEventSynchronize(e1) != hipSuccess) { rc = fail(FSPANN_E_DEVICE, "hbm_read_kernel failed"); break; }
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, e0, e1);
                if (r >= 0 && ms > 0.f) best = std::max(best, static_cast<double>(bytes) / (ms * 1e-3) / 1e9);
            }
        }
        *gb_per_s = best;
    } while (0);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(buf);
    (void)hipFree(sink);
    return rc;
}

int fspann_hbm_read_window(fspann_ctx* c, size_t bytes, size_t window, int reps, double* gb_per_s) {
    CHECK_CTX(c);
    if (!gb_per_s || reps <= 0 || window < (1u << 20) || bytes < 2 * window || (window & 15))
        return fail(FSPANN_E_ARG, "window < 1 MiB or not a multiple of 16, bytes < 2 windows, reps <= 0 or null output");
    void* buf = nullptr;
    unsigned long long* sink = nullptr;
    FSP_HIP(hipMalloc(&buf, bytes));
    if (hipMalloc(&sink, 8) != hipSuccess) { (void)hipFree(buf); return fail(FSPANN_E_NOMEM, "hipMalloc failed"); }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = FSPANN_OK;
    do {
        if (hipMemsetAsync(buf, 0x5A, bytes, c->stream) != hipSuccess || hipMemsetAsync(sink, 0, 8, c->stream) != hipSuccess ||
            hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { rc = fail(FSPANN_E_DEVICE, "setup failed"); break; }
        const unsigned grid = static_cast<unsigned>(c->num_cus) * 8;
        const size_t nwin = bytes / window;
        double best = 0.0;
        size_t wi = 0;
        for (int nt = 0; nt < 2 && rc == FSPANN_OK; nt++) {      // default cache policy and nt: the ceiling is the better of the two
            double total_ms = 0.0;
            int done = 0;
            for (int r = -1; r < reps; r++) {                    // r = -1: warm-up
                const hbm_u32x4* w = reinterpret_cast<const hbm_u32x4*>(static_cast<const char*>(buf) + (++wi % nwin) * window);
                if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(FSPANN_E_DEVICE, "hbm_read_kernel failed"); break; }
                if (nt) hipExtLaunchKernelGGL(hbm_read_kernel<true>, dim3(grid), dim3(256), 0, c->stream, e0, e1, 0, w, window / 16, sink);
                else hipExtLaunchKernelGGL(hbm_read_kernel<false>, dim3(grid), dim3(256), 0, c->stream, e0, e1, 0, w, window / 16, sink);
                if (hipEventSynchronize(e1) != hipSuccess) { rc = fail(FSPANN_E_DEVICE, "hbm_read_kernel failed"); break; }
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, e0, e1);
                if (r >= 0) { total_ms += ms; done++; }
            }
            if (rc == FSPANN_OK && total_ms > 0.0) best = std::max(best, static_cast<double>(window) * done / (total_ms * 1e-3) / 1e9);
        }
        if (rc == FSPANN_OK) *gb_per_s = best;
    } while (0);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(buf);
    (void)hipFree(sink);
    return rc;
}

// ---- device memory helpers -----------------------------------------------------------------
int fspann_dev_alloc(fspann_ctx* c, size_t bytes, void** out) {
    CHECK_CTX(c);
    if (!out) return fail(FSPANN_E_NULL, "out is null");
    FSP_HIP(hipMalloc(out, bytes ? bytes : 1));
    return FSPANN_OK;
}
int fspann_dev_free(fspann_ctx* c, void* p) {
    CHECK_CTX(c);
    if (p) {
        FSP_HIP(hipStreamSynchronize(c->stream));
        FSP_HIP(hipFree(p));
    }
    return FSPANN_OK;
}
int fspann_h2d(fspann_ctx* c, void* dst_dev, const void* src, size_t bytes) {
    CHECK_CTX(c);
    FSP_HIP(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, c->stream));
    FSP_HIP(hipStreamSynchronize(c->stream));
    return FSPANN_OK;
}
int fspann_d2h(fspann_ctx* c, void* dst, const void* src_dev, size_t bytes) {
    CHECK_CTX(c);
    FSP_HIP(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    FSP_HIP(hipStreamSynchronize(c->stream));
    return FSPANN_OK;
}


}  // extern "C"
