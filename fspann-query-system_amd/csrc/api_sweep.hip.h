// api_sweep.hip.h — include/fspann_sweep.h: Refine and QueryServiceImpl.search at several refinement limits in one pass
// (fspann_refine_sweep_dev / fspann_refine_store_sweep_dev / fspann_search_sweep_dev / fspann_search_sweep_finish_dev).
// Kernels in refine_sweep.hip.h; the argument why one pass is exact, the design and the measurements: DESIGN.md 3.3i.
// Part of the single translation unit fspann_api.hip (included there, last); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_sweep.h"

namespace {

// Work area of a sweep call: the keys [nq][kpitch], the clipped counts, pass 1's Route counts, each query's largest retried limit,
// the pick list and its count, and retried / scored / unique [nl][nq] for the outputs the caller does not ask for.
struct SweepArea {
    uint64_t* keys;
    int64_t kpitch;
    int32_t *clip, *cnt1, *cap_q, *list, *count, *retried, *scored;
};

size_t sweep_area_bytes(int64_t nq, int nchunks, int nl) {
    const size_t kb = (static_cast<size_t>(nq) * nchunks * kRefRows * 8 + 255) & ~size_t(255);
    const size_t nb = (static_cast<size_t>(nq) * 4 + 255) & ~size_t(255);
    const size_t pb = (static_cast<size_t>(nq) * nl * 4 + 255) & ~size_t(255);
    return kb + 4 * nb + 256 + 2 * pb;
}

int sweep_area(fspann_ctx* c, int64_t nq, int nchunks, int nl, SweepArea& s) {
    const size_t kb = (static_cast<size_t>(nq) * nchunks * kRefRows * 8 + 255) & ~size_t(255);
    const size_t nb = (static_cast<size_t>(nq) * 4 + 255) & ~size_t(255);
    const size_t pb = (static_cast<size_t>(nq) * nl * 4 + 255) & ~size_t(255);
    int rc = ensure(c, c->ws_sweep, sweep_area_bytes(nq, nchunks, nl));
    if (rc) return rc;
    char* w = static_cast<char*>(c->ws_sweep.p);
    s.keys = reinterpret_cast<uint64_t*>(w);
    s.kpitch = static_cast<int64_t>(nchunks) * kRefRows;
    s.clip = reinterpret_cast<int32_t*>(w + kb);
    s.cnt1 = reinterpret_cast<int32_t*>(w + kb + nb);
    s.cap_q = reinterpret_cast<int32_t*>(w + kb + 2 * nb);
    s.list = reinterpret_cast<int32_t*>(w + kb + 3 * nb);
    s.count = reinterpret_cast<int32_t*>(w + kb + 4 * nb);
    s.retried = reinterpret_cast<int32_t*>(w + kb + 4 * nb + 256);
    s.scored = reinterpret_cast<int32_t*>(w + kb + 4 * nb + 256 + pb);
    return FSPANN_OK;
}

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

// The scan with the key epilogue: launch_refine_dc's choice between the stream and one workgroup per chunk, without partial lists,
// hand-over or kernel-attached timing.  B = the row pitch (stride); nchunks covers the largest limit only.
template <typename TC, typename TQ, int DC, bool GATHER>
int launch_refine_keys_dc(fspann_ctx* c, int64_t nq, const TQ* q, const TC* cand, int64_t B, const int32_t* cand_ids, const int32_t* cand_count, int nchunks,
                          uint64_t* keys, const int32_t* qlist, const int32_t* qcount) {
    constexpr int VN = VecOf<TC>::N;
    const int d = c->cfg.dim;
    const bool vec = (d % VN == 0) && ((reinterpret_cast<uintptr_t>(cand) & 15) == 0);
    const size_t lds = std::max<size_t>(static_cast<size_t>(kRefRows) * (vec ? DC + VN : DC + 1) * sizeof(TC), static_cast<size_t>(kRefRows) * 16);
    const unsigned grid = static_cast<unsigned>(nq * nchunks);
    const RefineArgs<TC, TQ> ra{q, cand, GATHER ? c->store_n : 0, B, d, cand_ids, cand_count, 0, nchunks, nullptr, nullptr, nullptr, nullptr,
                                reinterpret_cast<RefinePartial*>(keys), nullptr, 0, 0, c->dbg_route};
    const int stream_wgs = (c->knob_refine_stream >= 0) ? std::min(c->knob_refine_stream, GATHER ? 3 : 4) : (GATHER ? 3 : 4);
    bool done = false;
    if constexpr (DC * sizeof(TC) == 128) if (vec && stream_wgs > 0) {
        const unsigned sgrid = static_cast<unsigned>(std::min<int64_t>(nq * nchunks, static_cast<int64_t>(c->num_cus) * stream_wgs));
        if (qlist) hipLaunchKernelGGL((refine_stream_keys_kernel<TC, TQ, DC, GATHER, true>), dim3(sgrid), dim3(kRefRows), lds, c->stream, ra, nq, qlist, qcount);
        else hipLaunchKernelGGL((refine_stream_keys_kernel<TC, TQ, DC, GATHER, false>), dim3(sgrid), dim3(kRefRows), lds, c->stream, ra, nq, qlist, qcount);
        done = true;
    }
    if (!done) {
        auto kern = vec ? refine_scan_keys_kernel<TC, TQ, DC, true, GATHER> : refine_scan_keys_kernel<TC, TQ, DC, false, GATHER>;
        if (lds > 64 * 1024) if (int rc = raise_lds_ceiling(c, kern, lds)) return rc;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kRefRows), lds, c->stream, ra, qlist, qcount);
    }
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

template <typename TC, typename TQ, bool GATHER>
int launch_refine_keys_t(fspann_ctx* c, int64_t nq, const TQ* q, const TC* cand, int64_t B, const int32_t* cand_ids, const int32_t* cand_count, int nchunks,
                         uint64_t* keys, const int32_t* qlist, const int32_t* qcount) {
    auto run = [&](auto dc) {
        return launch_refine_keys_dc<TC, TQ, decltype(dc)::value, GATHER>(c, nq, q, cand, B, cand_ids, cand_count, nchunks, keys, qlist, qcount);
    };
    constexpr int DC0 = 128 / static_cast<int>(sizeof(TC));     // dims per tile, as launch_refine_t
    const int dc_env = c->knob_refine_dc;
    int rc;
    if constexpr (sizeof(TC) < 4) rc = run(std::integral_constant<int, DC0>{});
    else if (dc_env == DC0 * 2) rc = run(std::integral_constant<int, DC0 * 2>{});
    else if (dc_env == DC0 * 4) rc = run(std::integral_constant<int, DC0 * 4>{});
    else rc = run(std::integral_constant<int, DC0>{});
    if (rc) return rc;
    // the touched-record set: the rows this scan scores (the clipped counts), marked behind it
    return touch_mark<TC, TQ, GATHER>(c, nq, q, cand, B, cand_ids, cand_count, qlist, qcount);
}

// One sweep refine: the key scan over the rows at `rows` (dense blocks, or GATHER: the resident store) with the clipped counts
// `clip`, then the prefix top-k with its snapshots.  qlist / qcount (device): over the queries qlist[0 .. *qcount) only; take
// (device, [nl][nq]): only the planes it marks are written.
template <bool GATHER>
int sweep_refine(fspann_ctx* c, const SweepArea& sw, int nchunks, int row_dtype, int q_dtype, int64_t nq, const void* q_dev, const void* rows, int64_t stride,
                 const int32_t* cand_ids_dev, const SweepLimits& lim, int k, int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev,
                 int32_t* scored_dev, const int32_t* take, const int32_t* qlist, const int32_t* qcount) {
    int rc = FSPANN_OK;
    bool launched = false;
    with_query_type(q_dtype, [&](auto tq) {
        launched = with_row_type(row_dtype, [&](auto tc) {
            using TQ = typename decltype(tq)::type;
            using TC = typename decltype(tc)::type;
            rc = launch_refine_keys_t<TC, TQ, GATHER>(c, nq, static_cast<const TQ*>(q_dev), static_cast<const TC*>(rows), stride, cand_ids_dev, sw.clip, nchunks,
                                                      sw.keys, qlist, qcount);
        });
    });
    if (!launched) {
        if ((rc = refuse_row_only(q_dtype, "q_dtype"))) return rc;
        if (!is_query_dtype(q_dtype)) return fail(FSPANN_E_ARG, "q_dtype %d: a query is FSPANN_F32 or FSPANN_F64", q_dtype);
        return fail(FSPANN_E_ARG, "unknown dtype");
    }
    if (rc) return rc;
    hipLaunchKernelGGL(refine_prefix_topk_kernel, dim3(static_cast<unsigned>(nq)), dim3(kSweepThreads), static_cast<size_t>(k) * 32, c->stream, sw.keys, sw.kpitch,
                       cand_ids_dev, stride, sw.clip, lim, k, nq, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, take, qlist, qcount);
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
    if ((rc = sweep_area(c, nq, nchunks, nl, sw))) return rc;
    if ((rc = sweep_clip(c, nq, cand_count_dev, static_cast<int32_t>(bmax), nullptr, sw.clip))) return rc;
    return sweep_refine<GATHER>(c, sw, nchunks, row_dtype, q_dtype, nq, q_dev, rows, stride, cand_ids_dev, lim, k, out_ids_dev, out_dist_dev, out_count_dev,
                                scored_dev, nullptr, nullptr, nullptr);
}

// What a search sweep call and its finish call share: the checked arguments, Route's work area (fspann_search_store_dev's layout at
// Bmax), the sweep's own, and the outputs with the area's buffers where the caller passed none.
struct SweepCall {
    SweepLimits lim;
    int64_t bmax;
    int nchunks;
    SearchArea sa;
    SweepArea sw;
    int32_t *scored, *retried;
};

int sweep_search_args(fspann_ctx* c, int64_t nq, const void* q_dev, const int64_t* limits, int nl, int k, int32_t* out_ids_dev, double* out_dist_dev,
                      int32_t* out_count_dev, SweepCall& s) {
    if (!c->frozen) return fail(FSPANN_E_STATE, "Index not finalized");
    if (!c->d_store) return fail(FSPANN_E_STATE, "plaintext store not set");
    if (nq < 0 || nq > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or nq > INT32_MAX");
    int rc = sweep_check(limits, nl, k, s.lim);
    if (rc) return rc;
    s.bmax = s.lim.v[nl - 1];
    s.nchunks = static_cast<int>((s.bmax + kRefRows - 1) / kRefRows);
    if (nq * s.nchunks >= (int64_t(1) << 31)) return fail(FSPANN_E_ARG, "nq x limit too large for one sweep");
    if (nq > 0 && (!q_dev || !out_ids_dev || !out_dist_dev || !out_count_dev)) return fail(FSPANN_E_NULL, "search buffer is null");
    return FSPANN_OK;
}

int sweep_unique(fspann_ctx* c, int64_t nq, const SweepCall& s, bool pass2, int32_t* unique_dev) {
    if (!unique_dev) return FSPANN_OK;
    hipLaunchKernelGGL(sweep_unique_kernel, dim3(static_cast<unsigned>((nq + 255) / 256)), dim3(256), 0, c->stream, nq, s.lim, s.sw.cnt1, s.sa.cnt, s.retried,
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
    if (!c->d_store) return fail(FSPANN_E_STATE, "plaintext store not set");
    return refine_sweep_call<true>(c, nq, q_dev, q_dtype, c->d_store, c->store_dtype, stride, cand_ids_dev, cand_count_dev, limits, nl, k, out_ids_dev, out_dist_dev,
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
    if ((rc = ensure(c, c->ws_search, search_area_bytes(c, nq, s.bmax)))) return rc;
    (void)search_area(c, nq, s.bmax, nullptr, nullptr, bad_dev, s.sa);
    if ((rc = sweep_area(c, nq, s.nchunks, nl, s.sw))) return rc;
    s.scored = scored_dev ? scored_dev : s.sw.scored;
    s.retried = retried_dev ? retried_dev : s.sw.retried;
    const int32_t bmax32 = static_cast<int32_t>(s.bmax);
    // pass 1: one encode, one Route at the largest limit with the caller's probes, one sweep refine over the store
    if ((rc = fspann_encode_dev(c, nq, q_dev, q_dtype, const_cast<uint64_t*>(s.sa.codes), nullptr, s.sa.bad))) return rc;
    if ((rc = fspann_route_dev(c, nq, s.sa.codes, probe_override, bmax32, s.bmax, s.sa.sel, nullptr, s.sa.cnt, nullptr, nullptr))) return rc;
    FSP_HIP(hipMemcpyAsync(s.sw.cnt1, s.sa.cnt, static_cast<size_t>(nq) * 4, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = sweep_clip(c, nq, s.sa.cnt, bmax32, nullptr, s.sw.clip))) return rc;
    if ((rc = sweep_refine<true>(c, s.sw, s.nchunks, c->store_dtype, q_dtype, nq, q_dev, c->d_store, s.bmax, s.sa.sel, s.lim, k, out_ids_dev, out_dist_dev,
                                 out_count_dev, s.scored, nullptr, nullptr, nullptr))) return rc;
    // QSI's retry predicate per (query, limit); the queries with any retried limit are listed
    hipLaunchKernelGGL(sweep_pick_kernel, dim3(1), dim3(kSweepPickThreads), 0, c->stream, nq, k, s.lim, s.sa.bad, s.sa.cnt, out_count_dev, s.scored, s.retried,
                       s.sw.cap_q, s.sw.list, s.sw.count);
    FSP_HIP(hipGetLastError());
    c->sweep_nq = nq; c->sweep_bmax = s.bmax; c->sweep_nl = nl; c->sweep_k = k;
    // pass 2 with 10 probes (QSI:333) over the listed queries; pass 1 at 10 effective probes already is what it would compute
    const bool same = effective_probes(c, probe_override) == effective_probes(c, 10);
    if (!same) {
        if ((rc = route_list_dev(c, nq, s.sa.codes, 10, s.bmax, s.sa.sel, s.sa.cnt, s.sw.list, s.sw.count))) return rc;
        // a query's pass 2 is scored up to its largest retried limit: the rows nobody asked for are neither read nor marked
        if ((rc = sweep_clip(c, nq, s.sa.cnt, bmax32, s.sw.cap_q, s.sw.clip))) return rc;
        if ((rc = sweep_refine<true>(c, s.sw, s.nchunks, c->store_dtype, q_dtype, nq, q_dev, c->d_store, s.bmax, s.sa.sel, s.lim, k, out_ids_dev, out_dist_dev,
                                     out_count_dev, s.scored, s.retried, s.sw.list, s.sw.count))) return rc;
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
    if (c->sweep_nq != nq || c->sweep_bmax != s.bmax || c->sweep_nl != nl || c->sweep_k != k || !c->ws_sweep.p ||
        c->ws_sweep.bytes < sweep_area_bytes(nq, s.nchunks, nl) || !search_area(c, nq, s.bmax, nullptr, nullptr, bad_dev, s.sa))
        return fail(FSPANN_E_STATE, "no fspann_search_sweep_dev call of this size precedes");
    if ((rc = sweep_area(c, nq, s.nchunks, nl, s.sw))) return rc;
    s.scored = scored_dev ? scored_dev : s.sw.scored;
    s.retried = retried_dev ? retried_dev : s.sw.retried;
    return guarded([&]() -> int {
        const size_t n4 = static_cast<size_t>(nq) * 4;
        const int32_t bmax32 = static_cast<int32_t>(s.bmax);
        FSP_HIP(hipStreamSynchronize(c->stream));
        std::vector<int32_t> cnt(static_cast<size_t>(nq));
        FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
        bool any = false;
        for (int64_t i = 0; i < nq && !any; i++) any = cnt[i] == kRouteUnmodelled;
        if (!any) return FSPANN_OK;
        std::vector<int32_t> ret(static_cast<size_t>(nq) * nl);
        FSP_HIP(hipMemcpy(ret.data(), s.retried, n4 * nl, hipMemcpyDeviceToHost));
        auto picked = [&](int64_t i) { for (int j = 0; j < nl; j++) if (ret[static_cast<size_t>(j) * nq + i]) return true; return false; };
        std::vector<int64_t> g1, g2;                 // flagged in pass 1 (never picked), flagged in pass 2
        for (int64_t i = 0; i < nq; i++)
            if (cnt[i] == kRouteUnmodelled) (picked(i) ? g2 : g1).push_back(i);
        const bool same = effective_probes(c, probe_override) == effective_probes(c, 10);
        int64_t done = 0, left = 0, d1 = 0;
        // scores the queries qs through the sweep: every plane (masked = false) or their retried planes up to their largest retried limit
        auto rescore = [&](const std::vector<int64_t>& qs, bool masked) -> int {
            if (qs.empty()) return FSPANN_OK;
            std::vector<int32_t> l(qs.begin(), qs.end());
            const int32_t n = static_cast<int32_t>(l.size());
            FSP_HIP(hipMemcpy(s.sw.list, l.data(), l.size() * 4, hipMemcpyHostToDevice));
            FSP_HIP(hipMemcpy(s.sw.count, &n, 4, hipMemcpyHostToDevice));
            int r = sweep_clip(c, nq, s.sa.cnt, bmax32, masked ? s.sw.cap_q : nullptr, s.sw.clip);
            if (r) return r;
            r = sweep_refine<true>(c, s.sw, s.nchunks, c->store_dtype, q_dtype, nq, q_dev, c->d_store, s.bmax, s.sa.sel, s.lim, k, out_ids_dev, out_dist_dev,
                                   out_count_dev, s.scored, masked ? s.retried : nullptr, s.sw.list, s.sw.count);
            if (r) return r;
            FSP_HIP(hipStreamSynchronize(c->stream));
            return FSPANN_OK;
        };
        // pass 1's flagged queries: finished at Bmax with pass 1's probes and scored at every limit; the short planes go on to pass 2
        int r = resolve_queries(c, g1, s.sa.codes, probe_override, bmax32, s.bmax, s.sa.sel, nullptr, s.sa.cnt, nullptr, nullptr, &d1, &left);
        if (r) return r;
        done += d1;
        if ((r = rescore(g1, false))) return r;
        std::vector<int64_t> again;
        if (!g1.empty()) {
            std::vector<int32_t> bad(static_cast<size_t>(nq)), oc(static_cast<size_t>(nq) * nl), sc(static_cast<size_t>(nq) * nl);
            FSP_HIP(hipMemcpy(bad.data(), s.sa.bad, n4, hipMemcpyDeviceToHost));
            FSP_HIP(hipMemcpy(oc.data(), out_count_dev, n4 * nl, hipMemcpyDeviceToHost));
            FSP_HIP(hipMemcpy(sc.data(), s.scored, n4 * nl, hipMemcpyDeviceToHost));
            FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
            for (int64_t i : g1) {
                FSP_HIP(hipMemcpy(s.sw.cnt1 + i, &cnt[i], 4, hipMemcpyHostToDevice));      // (the count pass 1 ended on)
                int32_t cap = 0;
                for (int j = 0; j < nl; j++) {
                    const size_t pl = static_cast<size_t>(j) * nq + i;
                    const int32_t one = (bad[i] == 0 && cnt[i] >= 0 && sc[pl] > 0 && (oc[pl] < k || static_cast<int64_t>(sc[pl]) < 10 * static_cast<int64_t>(k))) ? 1 : 0;
                    if (one) {
                        cap = s.lim.v[j];
                        FSP_HIP(hipMemcpy(s.retried + pl, &one, 4, hipMemcpyHostToDevice));
                    }
                }
                FSP_HIP(hipMemcpy(s.sw.cap_q + i, &cap, 4, hipMemcpyHostToDevice));
                if (cap > 0) again.push_back(i);
            }
        }
        std::vector<int64_t> s2 = g2;
        if (!again.empty() && !same) {
            // their pass 2 on the device: Route with 10 probes over them; what it flags joins pass 2's flagged queries
            std::vector<int32_t> l(again.begin(), again.end());
            const int32_t n = static_cast<int32_t>(l.size());
            FSP_HIP(hipMemcpy(s.sw.list, l.data(), l.size() * 4, hipMemcpyHostToDevice));
            FSP_HIP(hipMemcpy(s.sw.count, &n, 4, hipMemcpyHostToDevice));
            if ((r = route_list_dev(c, nq, s.sa.codes, 10, s.bmax, s.sa.sel, s.sa.cnt, s.sw.list, s.sw.count))) return r;
            FSP_HIP(hipStreamSynchronize(c->stream));
            FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
            for (int64_t i : again)
                if (cnt[i] == kRouteUnmodelled) g2.push_back(i);
            std::sort(g2.begin(), g2.end());
            s2.insert(s2.end(), again.begin(), again.end());
            std::sort(s2.begin(), s2.end());
        }
        // pass 2's flagged queries: finished with 10 probes, then every query of a host-side pass 2 is scored on its retried planes
        int64_t d2 = 0, left2 = 0;
        if ((r = resolve_queries(c, g2, s.sa.codes, 10, bmax32, s.bmax, s.sa.sel, nullptr, s.sa.cnt, nullptr, nullptr, &d2, &left2))) return r;
        done += d2;
        if ((r = rescore(s2, true))) return r;
        if ((r = sweep_unique(c, nq, s, !same, unique_dev))) return r;
        FSP_HIP(hipStreamSynchronize(c->stream));
        if (resolved) *resolved = done;
        return FSPANN_OK;
    });
}

}  // extern "C"
