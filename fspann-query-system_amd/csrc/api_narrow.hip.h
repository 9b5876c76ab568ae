// api_narrow.hip.h — include/fspann_narrow.h: which row types hold a block of fp32 or fp64 rows exactly, the rows re-packed, and a
// resident store narrowed in place (fspann_rows_fit_dev / fspann_rows_narrow_dev / fspann_store_fit / fspann_store_narrow).
// Kernels in narrow.hip.h, the rule per type in row_codec.hip.h (RowCodec<T>::fits / narrow); design and measurements: DESIGN.md 3.3k.
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_narrow.h"

namespace {

// "narrowest": fewest bytes per element; U8, I8, F8E4M3 among the one-byte types, F16 before BF16; then F32; then the source itself
constexpr int kNarrowOrder[] = {FSPANN_U8, FSPANN_I8, FSPANN_F8E4M3, FSPANN_F16, FSPANN_BF16, FSPANN_F32};

// the source dtype of a fit or narrow call: FSPANN_F32 or FSPANN_F64, anything else refused by name
int narrow_check_src(int dtype, const char* what) {
    if (dtype == FSPANN_F32 || dtype == FSPANN_F64) return FSPANN_OK;
    if (!is_row_dtype(dtype)) return fail(FSPANN_E_ARG, "%s: unknown dtype %d", what, dtype);
    return fail(FSPANN_E_ARG, "%s %s: rows are narrowed from FSPANN_F32 or FSPANN_F64", what, dtype_name(dtype));
}

int narrow_check_shape(int64_t n, int dim) {
    if (n <= 0) return fail(FSPANN_E_ARG, "n <= 0");
    if (dim <= 0) return fail(FSPANN_E_ARG, "dim <= 0");
    if (n > INT64_MAX / dim) return fail(FSPANN_E_ARG, "n * dim overflows");
    return FSPANN_OK;
}

// The fit pass over rows [n][dim] of TS on the context's stream, its result brought to the host (synchronises).
template <typename TS> int rows_fit_run(fspann_ctx* c, int64_t n, const TS* rows, int dim, uint8_t* row_fits, FitResult& r) {
    if (int rc = ensure(c, c->ws_narrow, sizeof(FitResult))) return rc;
    FitResult* out = static_cast<FitResult*>(c->ws_narrow.p);
    FSP_HIP(hipMemsetAsync(out->first, 0xff, sizeof(out->first), c->stream));
    FSP_HIP(hipMemsetAsync(&out->nonfinite, 0, sizeof(out->nonfinite), c->stream));
    const int rows_per_wg = std::max(1, kNarrowTile / dim);
    const int64_t grid = std::min<int64_t>((n + rows_per_wg - 1) / rows_per_wg, static_cast<int64_t>(c->num_cus) * 8);     // (a workgroup strides over the tiles)
    if (row_fits) hipLaunchKernelGGL((rows_fit_kernel<TS, true>), dim3(static_cast<unsigned>(grid)), dim3(kNarrowThreads), 0, c->stream, rows, n, dim, rows_per_wg, row_fits, out);
    else hipLaunchKernelGGL((rows_fit_kernel<TS, false>), dim3(static_cast<unsigned>(grid)), dim3(kNarrowThreads), 0, c->stream, rows, n, dim, rows_per_wg, row_fits, out);
    FSP_HIP(hipGetLastError());
    FSP_HIP(hipMemcpyAsync(&r, out, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    FSP_HIP(hipStreamSynchronize(c->stream));
    return FSPANN_OK;
}

// fspann_rows_fit_dev behind its context check (fspann_store_fit and fspann_store_narrow come here with the store)
int rows_fit(fspann_ctx* c, int64_t n, const void* rows_dev, int dtype, int dim, uint32_t allowed, uint8_t* row_fits_dev, fspann_fit* out) {
    if (!rows_dev || !out) return fail(FSPANN_E_NULL, "rows_dev or out is null");
    if (int rc = narrow_check_src(dtype, "dtype")) return rc;
    if (int rc = narrow_check_shape(n, dim)) return rc;
    if (allowed & ~kAllDtypes) return fail(FSPANN_E_ARG, "allowed 0x%x: a mask of (1u << FSPANN_x)", allowed);
    FitResult r;
    int rc = dtype == FSPANN_F32 ? rows_fit_run(c, n, static_cast<const float*>(rows_dev), dim, row_fits_dev, r)
                                 : rows_fit_run(c, n, static_cast<const double*>(rows_dev), dim, row_fits_dev, r);
    if (rc) return rc;
    out->fits = 0;
    for (const DtypeInfo& t : kDtypes) {       // (a type that is not narrower than the source was not tested: its first[] stayed "none")
        out->first_misfit[t.id] = r.first[t.id] == kNoMisfit ? -1 : static_cast<int64_t>(r.first[t.id]);
        if (r.first[t.id] == kNoMisfit) out->fits |= 1u << t.id;
    }
    out->first_misfit[7] = -1;
    out->nonfinite = static_cast<int64_t>(r.nonfinite);
    out->narrowest = dtype;
    const size_t own = dtype_size(dtype);
    for (int i = static_cast<int>(sizeof(kNarrowOrder) / sizeof(kNarrowOrder[0])) - 1; i >= 0; i--) {
        const int t = kNarrowOrder[i];
        if (dtype_size(t) < own && (out->fits >> t & 1u) && (allowed == 0 || (allowed >> t & 1u))) out->narrowest = t;
    }
    return FSPANN_OK;
}

// The narrow pass TS -> TD over ne elements, its counts brought to the host (synchronises).
template <typename TS, typename TD> int rows_narrow_run(fspann_ctx* c, int64_t ne, const TS* src, TD* dst, NarrowResult& r) {
    if (int rc = ensure(c, c->ws_narrow, sizeof(FitResult))) return rc;       // (one block serves both passes)
    NarrowResult* out = static_cast<NarrowResult*>(c->ws_narrow.p);
    FSP_HIP(hipMemsetAsync(&out->first, 0xff, sizeof(out->first), c->stream));
    FSP_HIP(hipMemsetAsync(&out->misfits, 0, sizeof(out->misfits), c->stream));
    constexpr int64_t per_slot = 16 / static_cast<int64_t>(sizeof(TD)), per_wg = kNarrowThreads * kNarrowSlots;
    const int64_t slots = (ne + per_slot - 1) / per_slot + 1;                 // (one more than packed rows need: a dst off its 16-byte grid)
    const int64_t grid = (slots + per_wg - 1) / per_wg;
    if (grid > INT32_MAX) return fail(FSPANN_E_ARG, "%lld elements: too many for one narrow pass", static_cast<long long>(ne));
    hipLaunchKernelGGL((rows_narrow_kernel<TS, TD>), dim3(static_cast<unsigned>(grid)), dim3(kNarrowThreads), 0, c->stream, src, ne, dst, out);
    FSP_HIP(hipGetLastError());
    FSP_HIP(hipMemcpyAsync(&r, out, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    FSP_HIP(hipStreamSynchronize(c->stream));
    return FSPANN_OK;
}

// fspann_rows_narrow_dev behind its context check
int rows_narrow(fspann_ctx* c, int64_t n, const void* src_dev, int src_dtype, int dim, void* dst_dev, int dst_dtype, int64_t* misfits) {
    if (misfits) *misfits = 0;
    if (!src_dev || !dst_dev) return fail(FSPANN_E_NULL, "src_dev or dst_dev is null");
    if (int rc = narrow_check_src(src_dtype, "src_dtype")) return rc;
    if (!is_row_dtype(dst_dtype)) return fail(FSPANN_E_ARG, "dst_dtype: unknown dtype %d", dst_dtype);
    if (dtype_size(dst_dtype) >= dtype_size(src_dtype))
        return fail(FSPANN_E_ARG, "dst_dtype %s is not narrower than src_dtype %s", dtype_name(dst_dtype), dtype_name(src_dtype));
    if (int rc = narrow_check_shape(n, dim)) return rc;
    if (reinterpret_cast<uintptr_t>(dst_dev) % dtype_size(dst_dtype)) return fail(FSPANN_E_ARG, "dst_dev is not aligned to its element");
    NarrowResult r{};
    int rc = FSPANN_OK;
    with_query_type(src_dtype, [&](auto ts) {          // (the query dtypes are the source dtypes: FSPANN_F32 and FSPANN_F64)
        using TS = typename decltype(ts)::type;
        with_row_type(dst_dtype, [&](auto td) {
            using TD = typename decltype(td)::type;
            if constexpr (sizeof(TD) < sizeof(TS)) rc = rows_narrow_run(c, n * dim, static_cast<const TS*>(src_dev), static_cast<TD*>(dst_dev), r);
        });
    });
    if (rc) return rc;
    if (misfits) *misfits = static_cast<int64_t>(r.misfits);
    if (r.misfits)
        return fail(FSPANN_E_ARG, "%llu element(s) are not %s values, the first at index %llu (row %llu, column %llu): the library never rounds", r.misfits,
                    dtype_name(dst_dtype), r.first, r.first / dim, r.first % dim);
    return FSPANN_OK;
}

}  // namespace

extern "C" {

int fspann_rows_fit_dev(fspann_ctx* c, int64_t n, const void* rows_dev, int dtype, int dim, uint32_t allowed, uint8_t* row_fits_dev, fspann_fit* out) {
    CHECK_CTX(c);
    return rows_fit(c, n, rows_dev, dtype, dim, allowed, row_fits_dev, out);
}

int fspann_rows_narrow_dev(fspann_ctx* c, int64_t n, const void* src_dev, int src_dtype, int dim, void* dst_dev, int dst_dtype, int64_t* misfits) {
    CHECK_CTX(c);
    return rows_narrow(c, n, src_dev, src_dtype, dim, dst_dev, dst_dtype, misfits);
}

int fspann_store_fit(fspann_ctx* c, uint32_t allowed, fspann_fit* out) {
    CHECK_CTX(c);
    if (!out) return fail(FSPANN_E_NULL, "out is null");
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    if (!is_query_dtype(c->store->dtype)) {         // a row-only type: nothing is narrower in the order, nothing is scanned
        *out = fspann_fit{};
        out->fits = 1u << c->store->dtype;
        out->narrowest = c->store->dtype;
        for (int64_t& f : out->first_misfit) f = -1;
        out->nonfinite = -1;
        return FSPANN_OK;
    }
    return rows_fit(c, c->store->n, c->store->rows, c->store->dtype, c->cfg.dim, allowed, nullptr, out);
}

int fspann_store_narrow(fspann_ctx* c, uint32_t allowed, int* dtype_out) {
    CHECK_CTX(c);
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    if (!may_change_shared(c)) return refuse_shared(c, "store");      // (in place: the one call that changes a RowStore others may hold)
    if (!c->store->owned)
        return fail(FSPANN_E_STATE, "the store is attached, caller-owned memory: narrow into a buffer of your own with fspann_rows_narrow_dev and attach that");
    if (dtype_out) *dtype_out = c->store->dtype;
    if (!is_query_dtype(c->store->dtype)) return FSPANN_OK;
    fspann_fit fit;
    if (int rc = rows_fit(c, c->store->n, c->store->rows, c->store->dtype, c->cfg.dim, allowed, nullptr, &fit)) return rc;
    if (fit.narrowest == c->store->dtype) return FSPANN_OK;
    void* rows = nullptr;
    FSP_HIP(hipMalloc(&rows, static_cast<size_t>(c->store->n) * c->cfg.dim * dtype_size(fit.narrowest)));
    int64_t misfits = 0;
    int rc = rows_narrow(c, c->store->n, c->store->rows, c->store->dtype, c->cfg.dim, rows, fit.narrowest, &misfits);      // (synchronises: nothing reads the old rows any more)
    if (rc) { (void)hipFree(rows); return rc; }
    (void)hipFree(c->store->rows);
    c->store->rows = rows;
    c->store->dtype = fit.narrowest;
    c->store->gen++;
    if (dtype_out) *dtype_out = c->store->dtype;
    return FSPANN_OK;
}

}  // extern "C"
