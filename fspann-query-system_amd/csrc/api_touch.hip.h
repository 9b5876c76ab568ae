// api_touch.hip.h — the touched-record set of selective re-encryption: fspann_touch_enable / _count / _drain, and the mark that
// every Refine launch enqueues behind itself while tracking is on (QSI:120,263,348-349; ReencryptionTracker.java:23-45;
// FSA:1739-1804).  Kernels in touch.hip.h.
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once

namespace {

// (Re)allocate the family's set for its current n_ids, cleared.  Under the family's touch_mu.  The new set is zeroed (on c's stream,
// waited for) before it is published, and an old set is released only after that: a failure leaves the old set in place, still
// bounded by its own touch_n.  Replacing a set needs no clone alive (the rule of every call that changes n_ids): then c is the
// owner, only it marks into the old set, and the wait on its stream is also the wait for those marks.
int touch_alloc(fspann_ctx* c) {
    const int64_t n = c->fam->n_ids;
    if (n <= 0) return fail(FSPANN_E_STATE, "set id metadata first: the touched set has one entry per handle");
    uint8_t* old = c->fam->d_touch.load(std::memory_order_acquire);
    if (old && !may_change_shared(c)) return refuse_shared(c, "touched set");
    const size_t bytes = static_cast<size_t>((n + kTouchTile - 1) / kTouchTile * kTouchTile);
    uint8_t* p = nullptr;
    FSP_HIP(hipMalloc(&p, bytes));
    if (hipMemsetAsync(p, 0, bytes, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(p);
        return fail(FSPANN_E_DEVICE, "allocating the touched set failed: the previous set is kept");
    }
    c->fam->touch_n = n;
    c->fam->touch_bytes = bytes;
    c->fam->d_touch.store(p, std::memory_order_release);
    if (old) (void)hipFree(old);
    return FSPANN_OK;
}

// The store validity bytes of c's store, computed once per store (stream order: the first mark behind a store_set pays for it).
int touch_store_ok(fspann_ctx* c) {
    if (c->store_ok_gen == c->store->gen && c->store_ok.p) return FSPANN_OK;
    int rc = ensure(c, c->store_ok, static_cast<size_t>(c->store->n));
    if (rc) return rc;
    const int d = c->cfg.dim;
    const unsigned grid = static_cast<unsigned>((c->store->n + kTouchThreads / 64 - 1) / (kTouchThreads / 64));
    hipError_t set = hipSuccess;
    with_row_type(c->store->dtype, [&](auto tr) {
        using T = typename decltype(tr)::type;
        if constexpr (DtypeOf<T>::finite)     // a byte, unsigned or signed, is always finite: every row is valid
            set = hipMemsetAsync(c->store_ok.p, 1, static_cast<size_t>(c->store->n), c->stream);
        else                                  // a float, a double, a half and a bfloat16 can be +-inf or NaN; an fp8 has no infinity but two NaN patterns
            hipLaunchKernelGGL(touch_store_valid_kernel<T>, dim3(grid), dim3(kTouchThreads), 0, c->stream, static_cast<const T*>(c->store->rows), c->store->n, d,
                               static_cast<uint8_t*>(c->store_ok.p));
    });
    FSP_HIP(set);
    FSP_HIP(hipGetLastError());
    c->store_ok_gen = c->store->gen;
    return FSPANN_OK;
}

// Marks the rows a Refine job scores (GATHER: rows from the resident store by id, else the job's rows), enqueued behind it on c's
// stream.  Tracking off: nothing is launched.
template <typename TC, typename TQ, bool GATHER>
int touch_mark(fspann_ctx* c, const RefineJob& j) {
    const int64_t nq = j.nq, B = j.B;
    const TQ* q = static_cast<const TQ*>(j.q);
    const int32_t *ids = j.cand_ids, *cnt = j.cand_count, *qlist = j.qlist, *qcount = j.qcount;
    IndexFamily& fam = *c->fam;
    if (!fam.touch_on.load(std::memory_order_acquire) || nq <= 0) return FSPANN_OK;
    uint8_t* set = fam.d_touch.load(std::memory_order_acquire);
    const int64_t n_set = fam.touch_n;
    if (!set) return FSPANN_OK;
    const int d = c->cfg.dim;
    const unsigned grid = static_cast<unsigned>(nq);
    if constexpr (GATHER) {
        int rc = touch_store_ok(c);
        if (rc) return rc;
        hipLaunchKernelGGL(touch_mark_store_kernel<TQ>, dim3(grid), dim3(kTouchThreads), 0, c->stream, q, d, ids, cnt, B, qlist, qcount,
                           static_cast<const uint8_t*>(c->store_ok.p), c->store->n, set, n_set);
    } else {
        hipLaunchKernelGGL((touch_mark_rows_kernel<TQ, TC>), dim3(grid), dim3(kTouchThreads), 0, c->stream, q, d, static_cast<const TC*>(j.rows), ids, cnt, B, qlist, qcount,
                           set, n_set);
    }
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

// Tile counts + their scan on c's stream; *total (host) = touched handles.  Under the family's touch_mu.
int touch_scan(fspann_ctx* c, int64_t out_cap, int64_t* total, int32_t** tile_cnt, int32_t** tile_off, int32_t** out) {
    const int64_t ntiles = static_cast<int64_t>(c->fam->touch_bytes) / kTouchTile;
    const size_t tb = (static_cast<size_t>(ntiles) * 4 + 255) & ~size_t(255);
    int rc = ensure(c, c->ws_touch, 2 * tb + 256 + static_cast<size_t>(out_cap) * 4);
    if (rc) return rc;
    char* w = static_cast<char*>(c->ws_touch.p);
    *tile_cnt = reinterpret_cast<int32_t*>(w);
    *tile_off = reinterpret_cast<int32_t*>(w + tb);
    int64_t* tot_dev = reinterpret_cast<int64_t*>(w + 2 * tb);
    *out = reinterpret_cast<int32_t*>(w + 2 * tb + 256);
    hipLaunchKernelGGL(touch_tile_count_kernel, dim3(static_cast<unsigned>(ntiles)), dim3(kTouchThreads), 0, c->stream,
                       static_cast<const uint8_t*>(c->fam->d_touch.load(std::memory_order_acquire)), *tile_cnt);
    FSP_HIP(hipGetLastError());
    hipLaunchKernelGGL(touch_tile_scan_kernel, dim3(1), dim3(kTouchScanThreads), 0, c->stream, *tile_cnt, ntiles, *tile_off, tot_dev);
    FSP_HIP(hipGetLastError());
    FSP_HIP(hipMemcpyAsync(total, tot_dev, 8, hipMemcpyDeviceToHost, c->stream));
    FSP_HIP(hipStreamSynchronize(c->stream));
    return FSPANN_OK;
}

}  // namespace

extern "C" {

int fspann_touch_enable(fspann_ctx* c, int on) {
    CHECK_CTX(c);
    std::lock_guard<std::mutex> tl(c->fam->touch_mu);
    if (!on) {
        c->fam->touch_on.store(false, std::memory_order_release);
        return FSPANN_OK;
    }
    if (!c->fam->d_touch.load(std::memory_order_acquire) || c->fam->touch_n != c->fam->n_ids) {
        int rc = touch_alloc(c);
        if (rc) return rc;
    }
    c->fam->touch_on.store(true, std::memory_order_release);
    return FSPANN_OK;
}

int fspann_touch_count(fspann_ctx* c, int64_t* unique) {
    CHECK_CTX(c);
    if (!unique) return fail(FSPANN_E_NULL, "unique is null");
    std::lock_guard<std::mutex> tl(c->fam->touch_mu);
    if (!c->fam->d_touch.load(std::memory_order_acquire)) return fail(FSPANN_E_STATE, "touch tracking was never enabled (fspann_touch_enable)");
    FSP_HIP(hipStreamSynchronize(c->stream));      // this context's marks first
    int32_t *tc, *to, *out;
    return touch_scan(c, 0, unique, &tc, &to, &out);
}

int fspann_touch_drain(fspann_ctx* c, int32_t* handles, int64_t cap, int64_t* n, int reset) {
    CHECK_CTX(c);
    if (!n) return fail(FSPANN_E_NULL, "n is null");
    if (cap < 0) return fail(FSPANN_E_ARG, "cap < 0");
    if (cap > 0 && !handles) return fail(FSPANN_E_NULL, "handles is null");
    std::lock_guard<std::mutex> tl(c->fam->touch_mu);
    uint8_t* set = c->fam->d_touch.load(std::memory_order_acquire);
    if (!set) return fail(FSPANN_E_STATE, "touch tracking was never enabled (fspann_touch_enable)");
    const int64_t cap_eff = std::min<int64_t>(cap, c->fam->touch_n);
    FSP_HIP(hipStreamSynchronize(c->stream));
    int32_t *tile_cnt, *tile_off, *out;
    int64_t total = 0;
    int rc = touch_scan(c, cap_eff, &total, &tile_cnt, &tile_off, &out);
    if (rc) return rc;
    *n = total;
    const int64_t w = std::min(total, cap_eff);
    if (w <= 0) return FSPANN_OK;
    const int64_t ntiles = static_cast<int64_t>(c->fam->touch_bytes) / kTouchTile;
    hipLaunchKernelGGL(touch_compact_kernel, dim3(static_cast<unsigned>(ntiles)), dim3(kTouchThreads), 0, c->stream, set, tile_cnt, tile_off, out,
                       w, reset ? 1 : 0);
    FSP_HIP(hipGetLastError());
    FSP_HIP(hipMemcpyAsync(handles, out, static_cast<size_t>(w) * 4, hipMemcpyDeviceToHost, c->stream));
    FSP_HIP(hipStreamSynchronize(c->stream));
    return FSPANN_OK;
}

}  // extern "C"
