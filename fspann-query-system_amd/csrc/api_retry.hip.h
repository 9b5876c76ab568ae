// api_retry.hip.h — QueryServiceImpl.search with its adaptive retry (QSI:101-352, 327-337, 444-447) in one call on the device:
// fspann_search_retry_dev / fspann_search_retry_finish_dev.  Pass 1 is fspann_search_store_dev; the pick kernel (search_pick.hip.h,
// RetryRule) lists the short queries; pass 2 runs Route (probe, bounded select, full select) and the refine over that list only,
// with 10 probes, and overwrites those queries' rows in place.  Also what the fallback and the sweep calls build on: the buffers of
// a search call (SearchBufs) and the host's half of a search, finish_flagged.
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once

namespace {

// Work area of a retry call behind fspann_search_store_dev's: the pick list [nq], retried [nq] and scored [nq] (for the caller that
// passes none), the list's count.
struct RetryArea {
    int32_t *list, *retried, *scored, *count;
    size_t lay(void* base, int64_t nq) {
        Carver w(base);
        list = w.take<int32_t>(static_cast<size_t>(nq) * 4);
        retried = w.take<int32_t>(static_cast<size_t>(nq) * 4);
        scored = w.take<int32_t>(static_cast<size_t>(nq) * 4);
        count = w.take<int32_t>(4);
        return w.off;
    }
};

// The buffers of one search call, the caller's or the work areas': what the passes and the host finish of every search family work
// on.  In a sweep B is the largest limit and out_count / scored / retried are [nl][nq] planes.
struct SearchBufs {
    int64_t nq, B;
    const void* q;
    int q_dtype, k;
    int32_t* out_ids;
    double* out_dist;
    int32_t* out_count;
    int32_t *scored, *retried;
    int32_t *list, *count;         // the pick list
    SearchArea sa;
};

// ... with the area's (RetryArea, SweepArea) scored / retried where the caller passed none.
template <class Area>
SearchBufs search_bufs(int64_t nq, const void* q_dev, int q_dtype, int64_t B, int k, int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev,
                       int32_t* scored_dev, int32_t* retried_dev, const SearchArea& sa, const Area& a) {
    return {nq, B, q_dev, q_dtype, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev ? scored_dev : a.scored, retried_dev ? retried_dev : a.retried, a.list, a.count, sa};
}

// The buffers of a retry call.  precedes (a call's name): the work areas must be as that call left them, nothing is allocated.
int retry_bufs(fspann_ctx* c, const char* precedes, int64_t nq, const void* q_dev, int q_dtype, int64_t B, int k, int32_t* out_ids_dev, double* out_dist_dev,
               int32_t* out_count_dev, int32_t* scored_dev, int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, int32_t* retried_dev, SearchBufs& s) {
    SearchArea sa;
    RetryArea ra;
    if (precedes) {
        if (!search_area(c, nq, B, sel_ids_dev, sel_count_dev, bad_dev, sa) || !area_held(c->ws_retry, ra, nq))
            return fail(FSPANN_E_STATE, "no %s call of this size precedes", precedes);
    } else {
        int rc;
        if ((rc = search_area_grow(c, nq, B, sel_ids_dev, sel_count_dev, bad_dev, sa)) || (rc = area_grow(c, c->ws_retry, ra, nq))) return rc;
    }
    s = search_bufs(nq, q_dev, q_dtype, B, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, retried_dev, sa, ra);
    return FSPANN_OK;
}

PickIn pick_in(const SearchBufs& s) { return {s.sa.bad, s.sa.cnt, s.out_count, s.scored, s.k}; }
// the list-mode Refine of a search over the store: the queries list[0 .. *count) only, in place
int refine_store_list(fspann_ctx* c, const SearchBufs& s, const int32_t* list, const int32_t* count) {
    return refine_run(c, store_job(c, s.q, s.q_dtype, s.nq, s.B, s.sa.sel, s.sa.cnt, s.k, s.out_ids, s.out_dist, s.out_count, s.scored, list, count));
}

// QSI.search with its adaptive retry, in stream order: pass 1 is fspann_search_store_dev with the caller's probes; the pick; pass 2
// with 10 probes (QSI:333) over the listed queries only, in place.  Pass 1 at 10 effective probes already is what pass 2 would
// compute (same codes, same Route, same store): retried says 1 and nothing runs again.  Pass 1 receives the buffers s already
// resolved (the caller's, or the search area's): it finds the area grown and hands the same pointers back.
int search_retry_passes(fspann_ctx* c, const SearchBufs& s, int probe_override) {
    int rc;
    if ((rc = fspann_search_store_dev(c, s.nq, s.q, s.q_dtype, probe_override, s.B, s.k, s.out_ids, s.out_dist, s.out_count, s.scored, s.sa.sel, s.sa.cnt, s.sa.bad))) return rc;
    if ((rc = launch_pick(c, s.nq, RetryRule{pick_in(s), s.retried}, s.list, s.count))) return rc;
    if (effective_probes(c, probe_override) == effective_probes(c, 10)) return FSPANN_OK;
    if ((rc = route_list_dev(c, s.nq, s.sa.codes, 10, s.B, s.sa.sel, s.sa.cnt, s.list, s.count))) return rc;
    return refine_store_list(c, s, s.list, s.count);
}

// First step of a finish call: the stream synchronised, the Route counts on the host; *any = one of them is flagged.
int flagged_counts(fspann_ctx* c, const SearchBufs& s, std::vector<int32_t>& cnt, bool* any) {
    FSP_HIP(hipStreamSynchronize(c->stream));
    cnt.resize(static_cast<size_t>(s.nq));
    FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, cnt.size() * 4, hipMemcpyDeviceToHost));
    *any = std::find(cnt.begin(), cnt.end(), kRouteUnmodelled) != cnt.end();
    return FSPANN_OK;
}

// The host's half of one QSI.search over nl planes of (out_count, scored, retried) (the stream is synchronised): g1 = the queries
// Route flagged in the pass at `probe_override` probes, g2 = those it flagged in the retry pass.  g1 is finished by the host model
// and scored on every plane; the retry rule is applied to it again; the queries it sends on are routed with 10 probes on the device,
// and what that flags joins g2; g2 is finished with 10 probes, and every query of a host-side pass 2 is scored on its retried planes.
// score(masked) scores the queries of s.list / s.count in stream order (masked: their retried planes only; with one plane every such
// query is retried, so both coincide).  requalified(i, count, last) follows the rule's verdict on query i: the Route count pass 1 ended
// on and the largest retried plane (-1: none).
template <class Score, class Requalified>
int finish_flagged(fspann_ctx* c, const SearchBufs& s, int nl, int probe_override, std::vector<int64_t> g1, std::vector<int64_t> g2, int64_t* done, Score&& score,
                   Requalified&& requalified) {
    if (g1.empty() && g2.empty()) return FSPANN_OK;
    const int64_t nq = s.nq;
    const size_t n4 = static_cast<size_t>(nq) * 4;
    const int32_t B32 = static_cast<int32_t>(s.B);
    const bool same = effective_probes(c, probe_override) == effective_probes(c, 10);
    auto put_list = [&](const std::vector<int64_t>& qs) -> int {
        std::vector<int32_t> l(qs.begin(), qs.end());
        const int32_t n = static_cast<int32_t>(l.size());
        FSP_HIP(hipMemcpy(s.list, l.data(), l.size() * 4, hipMemcpyHostToDevice));
        FSP_HIP(hipMemcpy(s.count, &n, 4, hipMemcpyHostToDevice));
        return FSPANN_OK;
    };
    auto rescore = [&](const std::vector<int64_t>& qs, bool masked) -> int {
        if (qs.empty()) return FSPANN_OK;
        int r = put_list(qs);
        if (r || (r = score(masked))) return r;
        FSP_HIP(hipStreamSynchronize(c->stream));
        return FSPANN_OK;
    };
    int64_t d1 = 0, d2 = 0, left = 0;
    int r = resolve_queries(c, g1, s.sa.codes, probe_override, B32, s.B, s.sa.sel, nullptr, s.sa.cnt, nullptr, nullptr, &d1, &left);
    if (r) return r;
    if ((r = rescore(g1, false))) return r;
    std::vector<int32_t> cnt(n4 / 4);
    std::vector<int64_t> again;
    if (!g1.empty()) {
        std::vector<int32_t> bad(n4 / 4), oc(n4 / 4 * nl), sc(n4 / 4 * nl);
        FSP_HIP(hipMemcpy(bad.data(), s.sa.bad, n4, hipMemcpyDeviceToHost));
        FSP_HIP(hipMemcpy(oc.data(), s.out_count, n4 * nl, hipMemcpyDeviceToHost));
        FSP_HIP(hipMemcpy(sc.data(), s.scored, n4 * nl, hipMemcpyDeviceToHost));
        FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
        for (int64_t i : g1) {
            int last = -1;
            for (int j = 0; j < nl; j++) {
                const size_t pl = static_cast<size_t>(j) * nq + i;
                if (!retry_wanted(bad[i], cnt[i], oc[pl], sc[pl], s.k)) continue;
                const int32_t one = 1;
                FSP_HIP(hipMemcpy(s.retried + pl, &one, 4, hipMemcpyHostToDevice));
                last = j;
            }
            if ((r = requalified(i, cnt[i], last))) return r;
            if (last >= 0) again.push_back(i);
        }
    }
    std::vector<int64_t> s2 = g2;
    if (!again.empty() && !same) {
        if ((r = put_list(again))) return r;
        if ((r = route_list_dev(c, nq, s.sa.codes, 10, s.B, s.sa.sel, s.sa.cnt, s.list, s.count))) return r;
        FSP_HIP(hipStreamSynchronize(c->stream));
        FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
        for (int64_t i : again)
            if (cnt[i] == kRouteUnmodelled) g2.push_back(i);
        std::sort(g2.begin(), g2.end());
        s2.insert(s2.end(), again.begin(), again.end());
        std::sort(s2.begin(), s2.end());
    }
    if ((r = resolve_queries(c, g2, s.sa.codes, 10, B32, s.B, s.sa.sel, nullptr, s.sa.cnt, nullptr, nullptr, &d2, &left))) return r;
    if ((r = rescore(s2, true))) return r;
    *done += d1 + d2;
    return FSPANN_OK;
}

// ... of a single-limit search: one plane, scored by the list-mode refine over the store.
int finish_flagged(fspann_ctx* c, const SearchBufs& s, int probe_override, std::vector<int64_t> g1, std::vector<int64_t> g2, int64_t* done) {
    return finish_flagged(
        c, s, 1, probe_override, std::move(g1), std::move(g2), done,
        [&](bool) { return refine_store_list(c, s, s.list, s.count); },
        [](int64_t, int32_t, int) { return FSPANN_OK; });
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
    const PickIn in{static_cast<const int32_t*>(s.bad_dev), static_cast<const int32_t*>(s.cnt_dev), static_cast<const int32_t*>(s.oc_dev),
                    static_cast<const int32_t*>(s.sc_dev), p->k};
    if (int rc = launch_pick(c, nq, RetryRule{in, static_cast<int32_t*>(s.ret_dev)}, static_cast<int32_t*>(s.list_dev), static_cast<int32_t*>(s.lcnt_dev))) return rc;
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
    rc = refine_run(c, {s.q_dev, FSPANN_F32, cand_dev, FSPANN_F32, false, nq, B, static_cast<const int32_t*>(s.ids_dev), static_cast<const int32_t*>(s.kcnt_dev), p->k,
                        static_cast<int32_t*>(s.oi_dev), static_cast<double*>(s.od_dev), static_cast<int32_t*>(s.oc_dev), static_cast<int32_t*>(s.sc_dev),
                        static_cast<const int32_t*>(s.list_dev), static_cast<const int32_t*>(s.lcnt_dev)});
    s.t_retry_ms = now_ms() - t0;
    return rc;
}

int check_retry_args(fspann_ctx* c, int64_t nq, const void* q_dev, int64_t B, int k, int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev) {
    if (!c->frozen) return fail(FSPANN_E_STATE, "Index not finalized");
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
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
    SearchBufs s;
    if ((rc = retry_bufs(c, nullptr, nq, q_dev, q_dtype, B, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, sel_ids_dev, sel_count_dev, bad_dev, retried_dev, s)))
        return rc;
    return search_retry_passes(c, s, probe_override);
}

int fspann_search_retry_finish_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int probe_override, int64_t B, int k,
                                   int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev,
                                   int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, int32_t* retried_dev, int64_t* resolved) {
    CHECK_CTX(c);
    if (resolved) *resolved = 0;
    if (int rc = refuse_row_only(q_dtype, "q_dtype")) return rc;     // (whether or not a query is left to finish)
    int rc = check_retry_args(c, nq, q_dev, B, k, out_ids_dev, out_dist_dev, out_count_dev);
    if (rc || nq == 0) return rc;
    SearchBufs s;
    if ((rc = retry_bufs(c, "fspann_search_retry_dev", nq, q_dev, q_dtype, B, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, sel_ids_dev, sel_count_dev, bad_dev,
                         retried_dev, s))) return rc;
    return guarded([&]() -> int {
        std::vector<int32_t> cnt;
        bool any = false;
        if (int r = flagged_counts(c, s, cnt, &any)) return r;
        if (!any) return FSPANN_OK;
        std::vector<int32_t> ret(static_cast<size_t>(nq));
        FSP_HIP(hipMemcpy(ret.data(), s.retried, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToHost));
        std::vector<int64_t> g1, g2;                 // flagged in pass 1 (never picked), flagged in pass 2
        for (int64_t i = 0; i < nq; i++)
            if (cnt[i] == kRouteUnmodelled) (ret[i] ? g2 : g1).push_back(i);
        int64_t done = 0;
        if (int r = finish_flagged(c, s, probe_override, g1, g2, &done)) return r;
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
