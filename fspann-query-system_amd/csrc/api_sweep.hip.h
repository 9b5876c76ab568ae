// api_sweep.hip.h — include/fspann_sweep.h: Refine and QueryServiceImpl.search at several refinement limits in one pass
// (fspann_refine_sweep_dev / fspann_refine_store_sweep_dev / fspann_search_sweep_dev / fspann_search_sweep_finish_dev).
// Kernels in refine_sweep.hip.h; the argument why one pass is exact, the design and the measurements: DESIGN.md 3.3i.
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_sweep.h"

namespace {

// Work area of a sweep call: the keys [nq][kpitch], the clipped counts, pass 1's Route counts, each query's largest retried limit,
// the pick list and its count, and retried / scored [nl][nq] for the outputs the caller does not ask for.
struct SweepArea {
    uint64_t* keys;
    int64_t kpitch;
    int32_t *clip, *cnt1, *cap_q, *list, *count, *retried, *scored;
    size_t lay(void* base, int64_t nq, int nchunks, int nl) {
        Carver w(base);
        kpitch = static_cast<int64_t>(nchunks) * kRefRows;
        keys = w.take<uint64_t>(static_cast<size_t>(nq) * kpitch * 8);
        for (int32_t** p : {&clip, &cnt1, &cap_q, &list}) *p = w.take<int32_t>(static_cast<size_t>(nq) * 4);
        count = w.take<int32_t>(4);
        retried = w.take<int32_t>(static_cast<size_t>(nq) * nl * 4);
        scored = w.take<int32_t>(static_cast<size_t>(nq) * nl * 4);
        return w.off;
    }
};

// limits / nl / k of every sweep call (include/fspann_sweep.h): the checked copy travels in kernel arguments.
int sweep_check(const int64_t* limits, int nl, int k, SweepLimits& lim) {
    if (nl < 1 || nl > kSweepMaxLimits) return fail(FSPANN_E_ARG, "nl %d: 1 .. %d limits", nl, kSweepMaxLimits);
    if (!limits) return fail(FSPANN_E_NULL, "limits is null");
    if (k < 1 || k > kSweepMaxK) return fail(FSPANN_E_ARG, "k %d: 1 .. %d", k, kSweepMaxK);
    lim = SweepLimits{};
    lim.n = nl;
    for (int j = 0; j < nl; j++) {
        if (limits[j] < 1 || limits[j] > INT32_MAX) return fail(FSPANN_E_ARG, "limits[%d] = %lld out of range (1 .. INT32_MAX)", j, static_cast<long long>(limits[j]));
        if (j > 0 && limits[j] <= limits[j - 1]) return fail(FSPANN_E_ARG, "limits must be strictly ascending (limits[%d] = %lld after %lld)", j,
                                                              static_cast<long long>(limits[j]), static_cast<long long>(limits[j - 1]));
        lim.v[j] = static_cast<int32_t>(limits[j]);
    }
    return FSPANN_OK;
}

// The scan of job j (counts: the clipped counts; no outputs) with the key epilogue under launch_refine_dc's plan (scan_plan), without
// partial lists, hand-over or kernel-attached timing, and the touched-record set behind it: the rows this scan scores.  j.B = the
// row pitch (stride); nchunks covers the largest limit only.
template <typename TC, typename TQ, bool GATHER>
int launch_refine_keys_t(fspann_ctx* c, const RefineJob& j, int nchunks, uint64_t* keys) {
    int rc = with_tile_width<TC>(c, [&](auto dc) -> int {
        constexpr int DC = decltype(dc)::value;
        const ScanPlan sp = scan_plan<TC, DC, GATHER>(c, j.nq, static_cast<const TC*>(j.rows), nchunks);
        const RefineArgs<TC, TQ> ra{static_cast<const TQ*>(j.q), static_cast<const TC*>(j.rows), GATHER ? c->store->n : 0, j.B, c->cfg.dim, j.cand_ids, j.cand_count, 0, nchunks,
                                    nullptr, nullptr, nullptr, nullptr, reinterpret_cast<RefinePartial*>(keys), nullptr, 0, 0, c->dbg_route};
        int r = FSPANN_OK;
        bool streamed = false;
        if constexpr (DC * sizeof(TC) == 128) if (sp.stream) {
            const unsigned sgrid = sp.sgrid(j.nq * nchunks);
            r = j.qlist ? launch_refine_kernel(c, false, refine_stream_keys_kernel<TC, TQ, DC, GATHER, true>, sgrid, sp.lds, ra, j.nq, j.qlist, j.qcount)
                        : launch_refine_kernel(c, false, refine_stream_keys_kernel<TC, TQ, DC, GATHER, false>, sgrid, sp.lds, ra, j.nq, j.qlist, j.qcount);
            streamed = true;
        }
        if (!streamed)
            r = sp.vec ? launch_refine_kernel_lds(c, false, refine_scan_keys_kernel<TC, TQ, DC, true, GATHER>, sp.grid, sp.lds, sp.lds, ra, j.qlist, j.qcount)
                       : launch_refine_kernel_lds(c, false, refine_scan_keys_kernel<TC, TQ, DC, false, GATHER>, sp.grid, sp.lds, sp.lds, ra, j.qlist, j.qcount);
        if (r) return r;
        FSP_HIP(hipGetLastError());
        return FSPANN_OK;
    });
    return rc ? rc : touch_mark<TC, TQ, GATHER>(c, j);
}

// One sweep refine: the key scan of job j (rows dense, or the resident store; its counts are replaced by the clipped counts
// sw.clip, j.B is the stride), then the prefix top-k with its snapshots into j's outputs.  take (device, [nl][nq]): only the planes
// it marks are written.
int sweep_refine(fspann_ctx* c, const SweepArea& sw, int nchunks, RefineJob j, const SweepLimits& lim, const int32_t* take) {
    j.cand_count = sw.clip;
    int rc = with_refine_types(j.q_dtype, j.row_dtype, [&](auto tq, auto tc) -> int {
        using TQ = typename decltype(tq)::type;
        using TC = typename decltype(tc)::type;
        return j.gather ? launch_refine_keys_t<TC, TQ, true>(c, j, nchunks, sw.keys) : launch_refine_keys_t<TC, TQ, false>(c, j, nchunks, sw.keys);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(refine_prefix_topk_kernel, dim3(static_cast<unsigned>(j.nq)), dim3(kSweepThreads), static_cast<size_t>(j.k) * 32, c->stream, sw.keys, sw.kpitch,
                       j.cand_ids, j.B, sw.clip, lim, j.k, j.nq, j.out_ids, j.out_dist, j.out_count, j.scored, take, j.qlist, j.qcount);
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

int sweep_clip(fspann_ctx* c, int64_t nq, const int32_t* count, int32_t bmax, const int32_t* cap_q, int32_t* clip) {
    hipLaunchKernelGGL(sweep_clip_kernel, dim3(static_cast<unsigned>((nq + 255) / 256)), dim3(256), 0, c->stream, nq, count, bmax, cap_q, clip);
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

template <bool GATHER>
int refine_sweep_call(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, const void* rows, int row_dtype, int64_t stride, const int32_t* cand_ids_dev,
                      const int32_t* cand_count_dev, const int64_t* limits, int nl, int k, int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev,
                      int32_t* scored_dev) {
    if (nq < 0) return fail(FSPANN_E_ARG, "nq < 0");
    SweepLimits lim;
    int rc = sweep_check(limits, nl, k, lim);
    if (rc) return rc;
    const int64_t bmax = lim.v[nl - 1];
    if (stride < bmax) return fail(FSPANN_E_ARG, "stride %lld is below the largest limit %lld", static_cast<long long>(stride), static_cast<long long>(bmax));
    if (nq == 0) return FSPANN_OK;
    if (!q_dev || !rows || !cand_ids_dev || !cand_count_dev || !out_ids_dev || !out_dist_dev || !out_count_dev) return fail(FSPANN_E_NULL, "refine buffer is null");
    const int nchunks = static_cast<int>((bmax + kRefRows - 1) / kRefRows);
    if (nq * nchunks >= (int64_t(1) << 31)) return fail(FSPANN_E_ARG, "nq x limit too large for one sweep");
    SweepArea sw;
    if ((rc = area_grow(c, c->ws_sweep, sw, nq, nchunks, nl))) return rc;
    if ((rc = sweep_clip(c, nq, cand_count_dev, static_cast<int32_t>(bmax), nullptr, sw.clip))) return rc;
    return sweep_refine(c, sw, nchunks, {q_dev, q_dtype, rows, row_dtype, GATHER, nq, stride, cand_ids_dev, cand_count_dev, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev},
                        lim, nullptr);
}

// What a search sweep call and its finish call share: the checked arguments, the sweep's work area, and the buffers of the search
// (Route's work area in fspann_search_store_dev's layout at Bmax; the sweep area's pick list and planes where the caller passed none).
struct SweepCall {
    SweepLimits lim;
    int64_t bmax;
    int nchunks;
    SweepArea sw;
    SearchBufs b;
};

int sweep_search_args(fspann_ctx* c, int64_t nq, const void* q_dev, const int64_t* limits, int nl, int k, int32_t* out_ids_dev, double* out_dist_dev,
                      int32_t* out_count_dev, SweepCall& s) {
    if (!c->frozen) return fail(FSPANN_E_STATE, "Index not finalized");
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    if (nq < 0 || nq > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or nq > INT32_MAX");
    int rc = sweep_check(limits, nl, k, s.lim);
    if (rc) return rc;
    s.bmax = s.lim.v[nl - 1];
    s.nchunks = static_cast<int>((s.bmax + kRefRows - 1) / kRefRows);
    if (nq * s.nchunks >= (int64_t(1) << 31)) return fail(FSPANN_E_ARG, "nq x limit too large for one sweep");
    if (nq > 0 && (!q_dev || !out_ids_dev || !out_dist_dev || !out_count_dev)) return fail(FSPANN_E_NULL, "search buffer is null");
    return FSPANN_OK;
}

// The work areas of a checked call, grown to size or (held) as the preceding fspann_search_sweep_dev left them, and its buffers.
int sweep_bufs(fspann_ctx* c, bool held, int64_t nq, const void* q_dev, int q_dtype, int nl, int k, int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev,
               int32_t* scored_dev, int32_t* bad_dev, int32_t* retried_dev, SweepCall& s) {
    SearchArea sa;
    if (held) {
        if (!area_held(c->ws_sweep, s.sw, nq, s.nchunks, nl) || !search_area(c, nq, s.bmax, nullptr, nullptr, bad_dev, sa))
            return fail(FSPANN_E_STATE, "no fspann_search_sweep_dev call of this size precedes");
    } else {
        int rc;
        if ((rc = search_area_grow(c, nq, s.bmax, nullptr, nullptr, bad_dev, sa)) || (rc = area_grow(c, c->ws_sweep, s.sw, nq, s.nchunks, nl))) return rc;
    }
    s.b = search_bufs(nq, q_dev, q_dtype, s.bmax, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, retried_dev, sa, s.sw);
    return FSPANN_OK;
}

// Scores the queries of the pick list through the sweep, in place: on every plane, or (masked) on their retried planes only and up
// to their largest retried limit — the rows nobody asked for are neither read nor marked.
int sweep_score_list(fspann_ctx* c, const SweepCall& s, bool masked) {
    const SearchBufs& b = s.b;
    if (int rc = sweep_clip(c, b.nq, b.sa.cnt, static_cast<int32_t>(s.bmax), masked ? s.sw.cap_q : nullptr, s.sw.clip)) return rc;
    return sweep_refine(c, s.sw, s.nchunks, store_job(c, b.q, b.q_dtype, b.nq, s.bmax, b.sa.sel, b.sa.cnt, b.k, b.out_ids, b.out_dist, b.out_count, b.scored, b.list, b.count),
                        s.lim, masked ? b.retried : nullptr);
}

int sweep_unique(fspann_ctx* c, int64_t nq, const SweepCall& s, bool pass2, int32_t* unique_dev) {
    if (!unique_dev) return FSPANN_OK;
    hipLaunchKernelGGL(sweep_unique_kernel, dim3(static_cast<unsigned>((nq + 255) / 256)), dim3(256), 0, c->stream, nq, s.lim, s.sw.cnt1, s.b.sa.cnt, s.b.retried,
                       pass2 ? 1 : 0, unique_dev);
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

}  // namespace

extern "C" {

int fspann_refine_sweep_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, const void* cand_dev, int cand_dtype, int64_t stride,
                            const int32_t* cand_ids_dev, const int32_t* cand_count_dev, const int64_t* limits, int nl, int k, int32_t* out_ids_dev,
                            double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev) {
    CHECK_CTX(c);
    return refine_sweep_call<false>(c, nq, q_dev, q_dtype, cand_dev, cand_dtype, stride, cand_ids_dev, cand_count_dev, limits, nl, k, out_ids_dev, out_dist_dev,
                                    out_count_dev, scored_dev);
}

int fspann_refine_store_sweep_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int64_t stride, const int32_t* cand_ids_dev,
                                  const int32_t* cand_count_dev, const int64_t* limits, int nl, int k, int32_t* out_ids_dev, double* out_dist_dev,
                                  int32_t* out_count_dev, int32_t* scored_dev) {
    CHECK_CTX(c);
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    return refine_sweep_call<true>(c, nq, q_dev, q_dtype, c->store->rows, c->store->dtype, stride, cand_ids_dev, cand_count_dev, limits, nl, k, out_ids_dev, out_dist_dev,
                                   out_count_dev, scored_dev);
}

int fspann_search_sweep_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int probe_override, const int64_t* limits, int nl, int k,
                            int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev, int32_t* unique_dev, int32_t* bad_dev,
                            int32_t* retried_dev) {
    CHECK_CTX(c);
    SweepCall s;
    int rc = sweep_search_args(c, nq, q_dev, limits, nl, k, out_ids_dev, out_dist_dev, out_count_dev, s);
    if (rc || nq == 0) return rc;
    c->sweep_nq = 0;                                   // (no finish call may follow a call that failed half-way)
    if ((rc = sweep_bufs(c, false, nq, q_dev, q_dtype, nl, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, bad_dev, retried_dev, s))) return rc;
    const SearchBufs& b = s.b;
    const int32_t bmax32 = static_cast<int32_t>(s.bmax);
    // pass 1: one encode, one Route at the largest limit with the caller's probes, one sweep refine over the store
    if ((rc = fspann_encode_dev(c, nq, q_dev, q_dtype, const_cast<uint64_t*>(b.sa.codes), nullptr, b.sa.bad))) return rc;
    if ((rc = fspann_route_dev(c, nq, b.sa.codes, probe_override, bmax32, s.bmax, b.sa.sel, nullptr, b.sa.cnt, nullptr, nullptr))) return rc;
    FSP_HIP(hipMemcpyAsync(s.sw.cnt1, b.sa.cnt, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = sweep_clip(c, nq, b.sa.cnt, bmax32, nullptr, s.sw.clip))) return rc;
    if ((rc = sweep_refine(c, s.sw, s.nchunks, store_job(c, q_dev, q_dtype, nq, s.bmax, b.sa.sel, b.sa.cnt, k, out_ids_dev, out_dist_dev, out_count_dev, b.scored), s.lim,
                           nullptr))) return rc;
    // QSI's retry predicate per (query, limit); the queries with any retried limit are listed
    if ((rc = launch_pick(c, nq, SweepRule{pick_in(b), s.lim, nq, b.retried, s.sw.cap_q}, b.list, b.count))) return rc;
    c->sweep_nq = nq; c->sweep_bmax = s.bmax; c->sweep_nl = nl; c->sweep_k = k;
    // pass 2 with 10 probes (QSI:333) over the listed queries; pass 1 at 10 effective probes already is what it would compute
    const bool same = effective_probes(c, probe_override) == effective_probes(c, 10);
    if (!same) {
        if ((rc = route_list_dev(c, nq, b.sa.codes, 10, s.bmax, b.sa.sel, b.sa.cnt, b.list, b.count))) return rc;
        if ((rc = sweep_score_list(c, s, true))) return rc;
    }
    return sweep_unique(c, nq, s, !same, unique_dev);
}

int fspann_search_sweep_finish_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int probe_override, const int64_t* limits, int nl, int k,
                                   int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev, int32_t* unique_dev,
                                   int32_t* bad_dev, int32_t* retried_dev, int64_t* resolved) {
    CHECK_CTX(c);
    if (resolved) *resolved = 0;
    if (int rc = refuse_row_only(q_dtype, "q_dtype")) return rc;
    SweepCall s;
    int rc = sweep_search_args(c, nq, q_dev, limits, nl, k, out_ids_dev, out_dist_dev, out_count_dev, s);
    if (rc || nq == 0) return rc;
    const bool held = c->sweep_nq == nq && c->sweep_bmax == s.bmax && c->sweep_nl == nl && c->sweep_k == k;
    if (!held) return fail(FSPANN_E_STATE, "no fspann_search_sweep_dev call of this size precedes");
    if ((rc = sweep_bufs(c, true, nq, q_dev, q_dtype, nl, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, bad_dev, retried_dev, s))) return rc;
    const SearchBufs& b = s.b;
    return guarded([&]() -> int {
        std::vector<int32_t> cnt;
        bool any = false;
        if (int r = flagged_counts(c, b, cnt, &any)) return r;
        if (!any) return FSPANN_OK;
        std::vector<int32_t> ret(static_cast<size_t>(nq) * nl);
        FSP_HIP(hipMemcpy(ret.data(), b.retried, ret.size() * 4, hipMemcpyDeviceToHost));
        auto picked = [&](int64_t i) { for (int j = 0; j < nl; j++) if (ret[static_cast<size_t>(j) * nq + i]) return true; return false; };
        std::vector<int64_t> g1, g2;                 // flagged in pass 1 (never picked), flagged in pass 2
        for (int64_t i = 0; i < nq; i++)
            if (cnt[i] == kRouteUnmodelled) (picked(i) ? g2 : g1).push_back(i);
        // pass 1's flagged queries are finished at Bmax and scored at every limit; the short planes go on to pass 2, whose queries are
        // scored on their retried planes
        int64_t done = 0;
        int r = finish_flagged(
            c, b, nl, probe_override, g1, g2, &done, [&](bool masked) { return sweep_score_list(c, s, masked); },
            [&](int64_t i, int32_t count, int last) -> int {
                const int32_t cap = last >= 0 ? s.lim.v[last] : 0;
                FSP_HIP(hipMemcpy(s.sw.cnt1 + i, &count, 4, hipMemcpyHostToDevice));      // (the count pass 1 ended on)
                FSP_HIP(hipMemcpy(s.sw.cap_q + i, &cap, 4, hipMemcpyHostToDevice));
                return FSPANN_OK;
            });
        if (r) return r;
        const bool same = effective_probes(c, probe_override) == effective_probes(c, 10);
        if ((r = sweep_unique(c, nq, s, !same, unique_dev))) return r;
        FSP_HIP(hipStreamSynchronize(c->stream));
        if (resolved) *resolved = done;
        return FSPANN_OK;
    });
}

}  // extern "C"
