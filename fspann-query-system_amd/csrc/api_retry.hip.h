// api_retry.hip.h — QueryServiceImpl.search with its adaptive retry (QSI:101-352, 327-337, 444-447) in one call on the device:
// fspann_search_retry_dev / fspann_search_retry_finish_dev.  Pass 1 is fspann_search_store_dev; retry_pick_kernel lists the
// short queries; pass 2 runs the list-mode Route (probe, bounded select, full select) and the list-mode refine over that list
// only, with 10 probes, and overwrites those queries' rows in place.
// Part of the single translation unit fspann_api.hip (included there, last); product code, no CPU fallback.
#pragma once

namespace {

constexpr int kPickThreads = 1024;

// QSI's retry predicate per query (QSI:159, 293, 444-447): not rejected (bad), its Route not flagged (count -1), at least one
// row scored, and fewer than k results or fewer than 10 k rows scored.
__device__ __forceinline__ bool retry_wanted(const int32_t* __restrict__ bad, const int32_t* __restrict__ route_cnt,
                                             const int32_t* __restrict__ out_count, const int32_t* __restrict__ scored, int64_t i, int k) {
    const int32_t sc = scored[i];
    return bad[i] == 0 && route_cnt[i] >= 0 && sc > 0 && (out_count[i] < k || static_cast<int64_t>(sc) < 10 * static_cast<int64_t>(k));
}

// One workgroup: wave w owns the contiguous slice [w * seg, (w + 1) * seg) of the batch.  Pass 1 writes retried[] and counts per
// wave, the wave counts are scanned, pass 2 writes each picked index at its rank.  The list is ascending whatever nq is.
__global__ __launch_bounds__(kPickThreads) void retry_pick_kernel(int64_t nq, int k, const int32_t* __restrict__ bad,
                                                                  const int32_t* __restrict__ route_cnt, const int32_t* __restrict__ out_count,
                                                                  const int32_t* __restrict__ scored, int32_t* __restrict__ retried,
                                                                  int32_t* __restrict__ list, int32_t* __restrict__ count) {
    constexpr int nwv = kPickThreads / 64;
    __shared__ int s_base[nwv + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t seg = ((nq + nwv - 1) / nwv + 63) & ~int64_t(63);
    const int64_t lo = min(nq, wave * seg), hi = min(nq, lo + seg);
    int n = 0;
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool p = i < hi && retry_wanted(bad, route_cnt, out_count, scored, i, k);
        if (i < hi) retried[i] = p ? 1 : 0;
        n += __popcll(__ballot(p));
    }
    if (lane == 0) s_base[wave] = n;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int w = 0; w < nwv; w++) { const int x = s_base[w]; s_base[w] = acc; acc += x; }
        s_base[nwv] = acc;
        *count = acc;
    }
    __syncthreads();
    int at = s_base[wave];
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int64_t i0 = lo; i0 < hi && at < s_base[wave + 1]; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool p = i < hi && retried[i] != 0;
        const unsigned long long m = __ballot(p);
        if (p) list[at + __popcll(m & lt)] = static_cast<int32_t>(i);
        at += __popcll(m);
    }
}

// Route with limit = cap = B over the queries qlist[0 .. *qcount) only (launches sized for nq; the count is read on the device).
int route_list_dev(fspann_ctx* c, int64_t nq, const uint64_t* codes_dev, int probe_override, int64_t B, int32_t* sel, int32_t* cnt,
                   const int32_t* qlist, const int32_t* qcount) {
    RoutePlan pl;
    RouteParams p{};
    bool fused = false;
    int rc = prepare_route(c, nq, codes_dev, probe_override, static_cast<int32_t>(B), B, sel, nullptr, cnt, nullptr, nullptr, &pl, &p, &fused);
    if (rc) return rc;
    p.qlist = qlist; p.qcount = qcount;
    if (!fused) {
        int G = 64;
        while (G > 2 && G / 2 >= 2 * pl.P - 1 && G / 2 >= 16) G >>= 1;     // (as launch_route_probe)
        const int gpb = kProbeThreads / G;
        const unsigned grid1 = static_cast<unsigned>((nq * c->TD + gpb - 1) / gpb);
        const size_t lds1 = static_cast<size_t>(gpb) * (2 * pl.P - 1) * 12;
        hipLaunchKernelGGL(route_probe_list_kernel, dim3(grid1), dim3(kProbeThreads), lds1, c->stream, p, p.probe_g, p.nprobe_g, G);
        FSP_HIP(hipGetLastError());
    }
    c->last_route_lazy = pl.lazy;
    if (pl.lazy) {
        auto go = [&](auto lk, bool big) -> int {      // big: the size class plans with more than the default 64 KB of LDS
            if (big) if (int r = raise_lds_ceiling(c, lk, 159 * 1024)) return r;
            hipLaunchKernelGGL(lk, dim3(pl.lz_grid), dim3(kLzThreads), pl.lz_lds_bytes, c->stream, p);
            FSP_HIP(hipGetLastError());
            return FSPANN_OK;
        };
        if (pl.lz_entries == 512) rc = go(route_select_lazy_list_kernel<kLzThreads, 512, false>, false);
        else if (pl.lz_entries == 2048) rc = go(route_select_lazy_list_kernel<kLzThreads, 2048, true>, true);
        else rc = go(route_select_lazy_list_kernel<kLzThreads, kLzEntriesMax, true>, true);
        if (rc) return rc;
        // the queries the bounded select handed over (none, normally): the full select over its overflow list, as fspann_route_dev
        p.qcount = p.ovf_count; p.qlist = p.ovf_list;
        pl.grid = std::min(pl.grid, 32);
    }
    return launch_full_select(c, pl, p);
}

// Work area of a retry call behind fspann_search_store_dev's: the pick list [nq], its count, retried [nq] (when the caller passes
// none) and scored [nq] (when the caller passes none).
struct RetryArea {
    int32_t* list;
    int32_t* count;
    int32_t* retried;
    int32_t* scored;
};

int retry_area(fspann_ctx* c, int64_t nq, RetryArea& r) {
    const size_t nb = (static_cast<size_t>(nq) * 4 + 255) & ~size_t(255);
    int rc = ensure(c, c->ws_retry, 3 * nb + 256);
    if (rc) return rc;
    char* w = static_cast<char*>(c->ws_retry.p);
    r.list = reinterpret_cast<int32_t*>(w);
    r.retried = reinterpret_cast<int32_t*>(w + nb);
    r.scored = reinterpret_cast<int32_t*>(w + 2 * nb);
    r.count = reinterpret_cast<int32_t*>(w + 3 * nb);
    return FSPANN_OK;
}

// Stage C of the native pipeline with the retry on (fspann_pipeline_set_retry), behind pass 1's refine and under the context's
// GPU lock: the pick kernel, its count read back; list-mode Route with 10 probes for the listed queries (flagged ones finished
// by the host model with 10 probes); only their F_q opened on the host; their rows copied up; list-mode refine in place.
int pipeline_retry(fspann_pipeline* p, fspann_pipeline::Slot& s) {
    fspann_ctx* c = p->ctx;
    const int d = c->cfg.dim;
    const int64_t nq = s.nq, B = p->B;
    const double t0 = now_ms();
    int32_t* list_h = s.list_pin;
    int32_t* cnt_h = s.cnt_pin;
    hipLaunchKernelGGL(retry_pick_kernel, dim3(1), dim3(kPickThreads), 0, c->stream, nq, p->k, static_cast<const int32_t*>(s.bad_dev),
                       static_cast<const int32_t*>(s.cnt_dev), static_cast<const int32_t*>(s.oc_dev), static_cast<const int32_t*>(s.sc_dev),
                       static_cast<int32_t*>(s.ret_dev), static_cast<int32_t*>(s.list_dev), static_cast<int32_t*>(s.lcnt_dev));
    FSP_HIP(hipGetLastError());
    FSP_HIP(hipMemcpyAsync(list_h + nq, s.lcnt_dev, 4, hipMemcpyDeviceToHost, c->stream));
    FSP_HIP(hipStreamSynchronize(c->stream));
    const int32_t n = list_h[nq];
    s.retried = n;
    // (pass 1 at 10 effective probes: pass 2 would reproduce it)
    if (n == 0 || effective_probes(c, -1) == effective_probes(c, 10)) { s.t_retry_ms = now_ms() - t0; return FSPANN_OK; }
    const uint64_t* codes = static_cast<const uint64_t*>(s.codes_dev);
    int32_t* sel = static_cast<int32_t*>(s.sel_dev);
    int32_t* cnt = static_cast<int32_t*>(s.cnt_dev);
    int rc = route_list_dev(c, nq, codes, 10, B, sel, cnt, static_cast<const int32_t*>(s.list_dev), static_cast<const int32_t*>(s.lcnt_dev));
    if (rc) return rc;
    auto fetch = [&]() -> int {
        FSP_HIP(hipMemcpyAsync(s.sel_pin, sel, static_cast<size_t>(nq) * B * 4, hipMemcpyDeviceToHost, c->stream));
        FSP_HIP(hipMemcpyAsync(cnt_h, cnt, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost, c->stream));
        FSP_HIP(hipStreamSynchronize(c->stream));
        return FSPANN_OK;
    };
    FSP_HIP(hipMemcpyAsync(list_h, s.list_dev, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, c->stream));
    if ((rc = fetch())) return rc;
    std::vector<int64_t> flagged;
    for (int32_t j = 0; j < n; j++)
        if (cnt_h[list_h[j]] == kRouteUnmodelled) flagged.push_back(list_h[j]);
    if (!flagged.empty()) {
        int64_t done = 0, left = 0;
        if ((rc = resolve_queries(c, flagged, codes, 10, static_cast<int32_t>(B), B, sel, nullptr, cnt, nullptr, nullptr, &done, &left))) return rc;
        s.unmodelled += left;
        if ((rc = fetch())) return rc;
    }
    // F_q of the listed queries, compact, opened on the host (PIS:717-724 + AES-GCM) ...
    for (int32_t j = 0; j < n; j++) {
        const int64_t qi = list_h[j];
        std::memcpy(s.rsel_pin + static_cast<size_t>(j) * B, s.sel_pin + qi * B, static_cast<size_t>(B) * 4);
        s.rselc_pin[j] = cnt_h[qi];
    }
    pointstore_open_batch<float>(p->ps, n, B, s.rsel_pin, s.rselc_pin, s.rcand_pin, s.rids_pin, s.rkcnt_pin, p->threads);
    // ... put back at their queries' places in the batch layout; only their rows go up
    float* cand_dev = static_cast<float*>(s.cand_dev);
    for (int32_t j = 0; j < n; j++) {
        const int64_t qi = list_h[j];
        const int32_t kc = s.rkcnt_pin[j];
        std::memcpy(s.ids_pin + qi * B, s.rids_pin + static_cast<size_t>(j) * B, static_cast<size_t>(B) * 4);
        s.kcnt_pin[qi] = kc;
        if (kc > 0) {
            std::memcpy(s.cand_pin + static_cast<size_t>(qi) * B * d, s.rcand_pin + static_cast<size_t>(j) * B * d, static_cast<size_t>(kc) * d * 4);
            FSP_HIP(hipMemcpyAsync(cand_dev + static_cast<size_t>(qi) * B * d, s.cand_pin + static_cast<size_t>(qi) * B * d, static_cast<size_t>(kc) * d * 4,
                                   hipMemcpyHostToDevice, c->stream));
        }
    }
    FSP_HIP(hipMemcpyAsync(s.ids_dev, s.ids_pin, static_cast<size_t>(nq) * B * 4, hipMemcpyHostToDevice, c->stream));
    FSP_HIP(hipMemcpyAsync(s.kcnt_dev, s.kcnt_pin, static_cast<size_t>(nq) * 4, hipMemcpyHostToDevice, c->stream));
    rc = launch_refine_t<float, float, false>(c, nq, static_cast<const float*>(s.q_dev), cand_dev, B, static_cast<const int32_t*>(s.ids_dev),
                                              static_cast<const int32_t*>(s.kcnt_dev), p->k, static_cast<int32_t*>(s.oi_dev), static_cast<double*>(s.od_dev),
                                              static_cast<int32_t*>(s.oc_dev), static_cast<int32_t*>(s.sc_dev), static_cast<const int32_t*>(s.list_dev),
                                              static_cast<const int32_t*>(s.lcnt_dev));
    s.t_retry_ms = now_ms() - t0;
    return rc;
}

int check_retry_args(fspann_ctx* c, int64_t nq, const void* q_dev, int64_t B, int k, int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev) {
    if (!c->frozen) return fail(FSPANN_E_STATE, "Index not finalized");
    if (!c->d_store) return fail(FSPANN_E_STATE, "plaintext store not set");
    if (nq < 0 || B <= 0 || B > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or B out of range");
    if (k <= 0) return fail(FSPANN_E_ARG, "topK must be > 0");  // QueryTokenFactory.java:65
    if (nq > INT32_MAX) return fail(FSPANN_E_ARG, "nq > INT32_MAX");
    if ((!q_dev || !out_ids_dev || !out_dist_dev || !out_count_dev)) return fail(FSPANN_E_NULL, "search buffer is null");
    return FSPANN_OK;
}

}  // namespace

extern "C" {

int fspann_search_retry_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int probe_override, int64_t B, int k,
                            int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev,
                            int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, int32_t* retried_dev) {
    CHECK_CTX(c);
    int rc = check_retry_args(c, nq, q_dev, B, k, out_ids_dev, out_dist_dev, out_count_dev);
    if (rc || nq == 0) return rc;
    RetryArea ra;
    if ((rc = retry_area(c, nq, ra))) return rc;
    int32_t* scored = scored_dev ? scored_dev : ra.scored;
    int32_t* retried = retried_dev ? retried_dev : ra.retried;
    // pass 1: fspann_search_store_dev with the caller's probes
    if ((rc = fspann_search_store_dev(c, nq, q_dev, q_dtype, probe_override, B, k, out_ids_dev, out_dist_dev, out_count_dev, scored,
                                      sel_ids_dev, sel_count_dev, bad_dev))) return rc;
    SearchArea sa;
    if (!search_area(c, nq, B, sel_ids_dev, sel_count_dev, bad_dev, sa)) return fail(FSPANN_E_STATE, "search work area missing");
    hipLaunchKernelGGL(retry_pick_kernel, dim3(1), dim3(kPickThreads), 0, c->stream, nq, k, sa.bad, sa.cnt, out_count_dev, scored, retried, ra.list, ra.count);
    FSP_HIP(hipGetLastError());
    // pass 2 with 10 probes (QSI:333) over the listed queries only.  Pass 1 at 10 effective probes already is what pass 2 would
    // compute (same codes, same Route, same store): retried says 1 and nothing runs again.
    if (effective_probes(c, probe_override) == effective_probes(c, 10)) return FSPANN_OK;
    if ((rc = route_list_dev(c, nq, sa.codes, 10, B, sa.sel, sa.cnt, ra.list, ra.count))) return rc;
    return refine_store_list(c, nq, q_dev, q_dtype, B, sa.sel, sa.cnt, k, out_ids_dev, out_dist_dev, out_count_dev, scored, ra.list, ra.count);
}

int fspann_search_retry_finish_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int probe_override, int64_t B, int k,
                                   int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev,
                                   int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, int32_t* retried_dev, int64_t* resolved) {
    CHECK_CTX(c);
    if (resolved) *resolved = 0;
    if (int rc = refuse_row_only(q_dtype, "q_dtype")) return rc;     // (whether or not a query is left to finish)
    int rc = check_retry_args(c, nq, q_dev, B, k, out_ids_dev, out_dist_dev, out_count_dev);
    if (rc || nq == 0) return rc;
    SearchArea sa;
    if (!search_area(c, nq, B, sel_ids_dev, sel_count_dev, bad_dev, sa) || !c->ws_retry.p ||
        c->ws_retry.bytes < 3 * ((static_cast<size_t>(nq) * 4 + 255) & ~size_t(255)) + 256)
        return fail(FSPANN_E_STATE, "no fspann_search_retry_dev call of this size precedes");
    RetryArea ra;
    if ((rc = retry_area(c, nq, ra))) return rc;
    int32_t* scored = scored_dev ? scored_dev : ra.scored;
    int32_t* retried = retried_dev ? retried_dev : ra.retried;
    return guarded([&]() -> int {
        const size_t n4 = static_cast<size_t>(nq) * 4;
        FSP_HIP(hipStreamSynchronize(c->stream));
        std::vector<int32_t> cnt(static_cast<size_t>(nq));
        FSP_HIP(hipMemcpy(cnt.data(), sa.cnt, n4, hipMemcpyDeviceToHost));
        bool any = false;
        for (int64_t i = 0; i < nq && !any; i++) any = cnt[i] == kRouteUnmodelled;
        if (!any) return FSPANN_OK;
        std::vector<int32_t> ret(static_cast<size_t>(nq));
        FSP_HIP(hipMemcpy(ret.data(), retried, n4, hipMemcpyDeviceToHost));
        std::vector<int64_t> g1, g2;                 // flagged in pass 1 (never picked), flagged in pass 2
        for (int64_t i = 0; i < nq; i++)
            if (cnt[i] == kRouteUnmodelled) (ret[i] ? g2 : g1).push_back(i);
        const bool same = effective_probes(c, probe_override) == effective_probes(c, 10);
        int64_t done = 0, left = 0, d1 = 0;
        auto rescore = [&](const std::vector<int64_t>& qs) -> int {
            if (qs.empty()) return FSPANN_OK;
            std::vector<int32_t> l(qs.begin(), qs.end());
            const int32_t n = static_cast<int32_t>(l.size());
            FSP_HIP(hipMemcpy(ra.list, l.data(), l.size() * 4, hipMemcpyHostToDevice));
            FSP_HIP(hipMemcpy(ra.count, &n, 4, hipMemcpyHostToDevice));
            int r = refine_store_list(c, nq, q_dev, q_dtype, B, sa.sel, sa.cnt, k, out_ids_dev, out_dist_dev, out_count_dev, scored, ra.list, ra.count);
            if (r) return r;
            FSP_HIP(hipStreamSynchronize(c->stream));
            return FSPANN_OK;
        };
        // pass 1's flagged queries: finished with pass 1's probes and scored; the short ones go on to their pass 2
        int r = resolve_queries(c, g1, sa.codes, probe_override, static_cast<int32_t>(B), B, sa.sel, nullptr, sa.cnt, nullptr, nullptr, &d1, &left);
        if (r) return r;
        done += d1;
        if ((r = rescore(g1))) return r;
        std::vector<int64_t> again;
        if (!g1.empty()) {
            std::vector<int32_t> bad(n4 / 4), oc(n4 / 4), sc(n4 / 4);
            FSP_HIP(hipMemcpy(bad.data(), sa.bad, n4, hipMemcpyDeviceToHost));
            FSP_HIP(hipMemcpy(oc.data(), out_count_dev, n4, hipMemcpyDeviceToHost));
            FSP_HIP(hipMemcpy(sc.data(), scored, n4, hipMemcpyDeviceToHost));
            FSP_HIP(hipMemcpy(cnt.data(), sa.cnt, n4, hipMemcpyDeviceToHost));
            for (int64_t i : g1)
                if (bad[i] == 0 && cnt[i] >= 0 && sc[i] > 0 && (oc[i] < k || static_cast<int64_t>(sc[i]) < 10 * static_cast<int64_t>(k))) {
                    again.push_back(i);
                    const int32_t one = 1;
                    FSP_HIP(hipMemcpy(retried + i, &one, 4, hipMemcpyHostToDevice));
                }
        }
        std::vector<int64_t> s2 = g2;
        if (!again.empty() && !same) {
            // their pass 2 on the device: Route with 10 probes over them; what it flags joins pass 2's flagged queries
            std::vector<int32_t> l(again.begin(), again.end());
            const int32_t n = static_cast<int32_t>(l.size());
            FSP_HIP(hipMemcpy(ra.list, l.data(), l.size() * 4, hipMemcpyHostToDevice));
            FSP_HIP(hipMemcpy(ra.count, &n, 4, hipMemcpyHostToDevice));
            if ((r = route_list_dev(c, nq, sa.codes, 10, B, sa.sel, sa.cnt, ra.list, ra.count))) return r;
            FSP_HIP(hipStreamSynchronize(c->stream));
            FSP_HIP(hipMemcpy(cnt.data(), sa.cnt, n4, hipMemcpyDeviceToHost));
            for (int64_t i : again)
                if (cnt[i] == kRouteUnmodelled) g2.push_back(i);
            std::sort(g2.begin(), g2.end());
            s2.insert(s2.end(), again.begin(), again.end());
            std::sort(s2.begin(), s2.end());
        }
        // pass 2's flagged queries: finished with 10 probes, then every query of a host-side pass 2 is scored
        int64_t d2 = 0, left2 = 0;
        if ((r = resolve_queries(c, g2, sa.codes, 10, static_cast<int32_t>(B), B, sa.sel, nullptr, sa.cnt, nullptr, nullptr, &d2, &left2))) return r;
        done += d2;
        if ((r = rescore(s2))) return r;
        if (resolved) *resolved = done;
        return FSPANN_OK;
    });
}

// QSI's adaptive retry in the native pipeline (stage C, see pipeline_retry).  Refused while batches are in flight.
int fspann_pipeline_set_retry(fspann_pipeline* p, int on) {
    if (!p) return fail(FSPANN_E_NULL, "pipeline is null");
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->free_q.size() != static_cast<size_t>(fspann_pipeline::kSlots))
        return fail(FSPANN_E_STATE, "%d batch(es) in flight: collect them before switching the retry", fspann_pipeline::kSlots - static_cast<int>(p->free_q.size()));
    if (on && !p->slot[0].rcand_pin) {
        const size_t d = p->ctx->cfg.dim, rows = static_cast<size_t>(p->nq_max) * p->B;
        bool ok = true;
        auto pin = [&](auto** ptr, size_t bytes) { if (ok && hipHostMalloc(reinterpret_cast<void**>(ptr), bytes, hipHostMallocDefault) != hipSuccess) ok = false; };
        for (auto& s : p->slot) {
            pin(&s.rsel_pin, rows * 4); pin(&s.rselc_pin, p->nq_max * 4); pin(&s.rids_pin, rows * 4); pin(&s.rkcnt_pin, p->nq_max * 4);
            pin(&s.rcand_pin, rows * d * 4);
        }
        if (!ok) {
            (void)hipGetLastError();
            for (auto& s : p->slot) {
                void* pins[] = {s.rsel_pin, s.rselc_pin, s.rids_pin, s.rkcnt_pin, s.rcand_pin};
                for (void* x : pins) if (x) (void)hipHostFree(x);
                s.rsel_pin = s.rselc_pin = s.rids_pin = s.rkcnt_pin = nullptr; s.rcand_pin = nullptr;
            }
            return fail(FSPANN_E_NOMEM, "pinned retry buffers: allocation failed");
        }
    }
    p->retry = on != 0;
    return FSPANN_OK;
}

// Queries the retry took through its second pass, and the mean time per batch spent in retry passes.
int fspann_pipeline_retry_stats(fspann_pipeline* p, int64_t* retried, double* retry_ms) {
    if (!p) return fail(FSPANN_E_NULL, "pipeline is null");
    std::lock_guard<std::mutex> lk(p->mu);
    if (retried) *retried = p->sum_retried;
    if (retry_ms) *retry_ms = p->sum_retry_ms / std::max<long long>(1, p->batches);
    return FSPANN_OK;
}

}  // extern "C"
