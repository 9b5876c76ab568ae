// api_eval.hip.h — ForwardSecureANNSystem.runQueries' loop (FSA:622-748) over a resident store, include/fspann_eval.h:
//   * fspann_eval_kvariants_dev: computeMetricsAtK for every k of kVariants from one result list (eval_sweep.hip.h);
//   * fspann_search_fallback_dev / _finish_dev: QSI.search, then the empty-result fallback (FSA:667-678): the empty queries are
//     searched again, a whole QSI.search with its adaptive retry, at max(2 base, 4) probes, in list mode, in place.
// Part of the single translation unit fspann_api.hip (included there, last); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_eval.h"

namespace {

// runQueries' fallback predicate per query (FSA:667): searched (not bad, Route not flagged) and nothing returned.
__device__ __forceinline__ bool fallback_wanted(const int32_t* __restrict__ bad, const int32_t* __restrict__ route_cnt,
                                                const int32_t* __restrict__ out_count, int64_t i) {
    return bad[i] == 0 && route_cnt[i] >= 0 && out_count[i] == 0;
}

// retry_pick_kernel's ascending list for the two picks of the fallback.  kRetry false: the queries that fall back; member[] and
// fellback[] (optional) receive the flag.  kRetry true: the adaptive retry INSIDE search 2, retry_wanted among the queries of
// member[] only, whose retried[] is rewritten (search 2's); the others keep theirs.  The predicate reads nothing this kernel
// writes, so the second pass evaluates it again.
template <bool kRetry>
__global__ __launch_bounds__(kPickThreads) void fallback_pick_kernel(int64_t nq, int k, const int32_t* __restrict__ bad, const int32_t* __restrict__ route_cnt,
                                                                     const int32_t* __restrict__ out_count, const int32_t* __restrict__ scored,
                                                                     int32_t* __restrict__ member, int32_t* __restrict__ flag_out,
                                                                     int32_t* __restrict__ list, int32_t* __restrict__ count) {
    constexpr int nwv = kPickThreads / 64;
    __shared__ int s_base[nwv + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t seg = ((nq + nwv - 1) / nwv + 63) & ~int64_t(63);
    const int64_t lo = min(nq, wave * seg), hi = min(nq, lo + seg);
    auto wanted = [&](int64_t i) -> bool {
        if constexpr (kRetry) return member[i] != 0 && retry_wanted(bad, route_cnt, out_count, scored, i, k);
        else return fallback_wanted(bad, route_cnt, out_count, i);
    };
    int n = 0;
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool p = i < hi && wanted(i);
        if (i < hi) {
            if constexpr (kRetry) { if (member[i] != 0) flag_out[i] = p ? 1 : 0; }
            else { if (flag_out) flag_out[i] = p ? 1 : 0; }
        }
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
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool p = i < hi && wanted(i);
        const unsigned long long m = __ballot(p);
        if (p) list[at + __popcll(m & lt)] = static_cast<int32_t>(i);
        if constexpr (!kRetry) { if (i < hi) member[i] = p ? 1 : 0; }
        at += __popcll(m);
    }
}

// Work area of a fallback call behind fspann_search_retry_dev's: the fallback list [nq], member [nq] (the queries search 2 runs
// over), fellback [nq] (when the caller passes none), the list's count.
struct FallbackArea {
    int32_t* list;
    int32_t* member;
    int32_t* fellback;
    int32_t* count;
};

size_t fallback_area_bytes(int64_t nq) { return 3 * ((static_cast<size_t>(nq) * 4 + 255) & ~size_t(255)) + 256; }

int fallback_area(fspann_ctx* c, int64_t nq, FallbackArea& f) {
    const size_t nb = (static_cast<size_t>(nq) * 4 + 255) & ~size_t(255);
    int rc = ensure(c, c->ws_fallback, fallback_area_bytes(nq));
    if (rc) return rc;
    char* w = static_cast<char*>(c->ws_fallback.p);
    f.list = reinterpret_cast<int32_t*>(w);
    f.member = reinterpret_cast<int32_t*>(w + nb);
    f.fellback = reinterpret_cast<int32_t*>(w + 2 * nb);
    f.count = reinterpret_cast<int32_t*>(w + 3 * nb);
    return FSPANN_OK;
}

// FSA:640, 668-673: the probes of the fallback search
int fallback_probes(const fspann_ctx* c, int probe_override) {
    const int po = probe_override >= 0 ? probe_override : c->cfg.probe_override;
    const int base = po >= 0 ? po : c->cfg.default_probes;
    return static_cast<int>(std::min<int64_t>(std::max<int64_t>(2 * static_cast<int64_t>(base), 4), INT32_MAX));
}

// The buffers of one search call, the caller's or the work areas'.
struct SearchBufs {
    int64_t nq, B;
    const void* q;
    int q_dtype, k;
    int32_t* out_ids;
    double* out_dist;
    int32_t* out_count;
    int32_t* scored;
    int32_t* retried;
    SearchArea sa;
    RetryArea ra;
};

// QSI.search over the queries list[0 .. *count) (device, ascending; member[] flags them) at `probes` probes, in stream order, with
// search 1's codes and in place: list-mode Route and refine, the retry pick among them (into the retry area's list), and, unless
// `probes` already is what 10 gives, list-mode Route with 10 probes and refine over the picked.
int search_list_dev(fspann_ctx* c, const SearchBufs& s, int probes, const int32_t* list, const int32_t* count, int32_t* member) {
    int rc;
    if ((rc = route_list_dev(c, s.nq, s.sa.codes, probes, s.B, s.sa.sel, s.sa.cnt, list, count))) return rc;
    if ((rc = refine_store_list(c, s.nq, s.q, s.q_dtype, s.B, s.sa.sel, s.sa.cnt, s.k, s.out_ids, s.out_dist, s.out_count, s.scored, list, count))) return rc;
    hipLaunchKernelGGL(fallback_pick_kernel<true>, dim3(1), dim3(kPickThreads), 0, c->stream, s.nq, s.k, s.sa.bad, s.sa.cnt, s.out_count, s.scored, member,
                       s.retried, s.ra.list, s.ra.count);
    FSP_HIP(hipGetLastError());
    if (effective_probes(c, probes) == effective_probes(c, 10)) return FSPANN_OK;
    if ((rc = route_list_dev(c, s.nq, s.sa.codes, 10, s.B, s.sa.sel, s.sa.cnt, s.ra.list, s.ra.count))) return rc;
    return refine_store_list(c, s.nq, s.q, s.q_dtype, s.B, s.sa.sel, s.sa.cnt, s.k, s.out_ids, s.out_dist, s.out_count, s.scored, s.ra.list, s.ra.count);
}

// The host's half of one QSI.search (the stream is synchronised): g1 = queries Route flagged in the pass at `probe_override`
// probes, g2 = queries it flagged in the retry pass.  The body of fspann_search_retry_finish_dev for any first-pass probes.
int finish_flagged(fspann_ctx* c, const SearchBufs& s, int probe_override, std::vector<int64_t> g1, std::vector<int64_t> g2, int64_t* done) {
    if (g1.empty() && g2.empty()) return FSPANN_OK;
    const int64_t nq = s.nq, B = s.B;
    const int k = s.k;
    const size_t n4 = static_cast<size_t>(nq) * 4;
    const bool same = effective_probes(c, probe_override) == effective_probes(c, 10);
    auto put_list = [&](const std::vector<int64_t>& qs) -> int {
        std::vector<int32_t> l(qs.begin(), qs.end());
        const int32_t n = static_cast<int32_t>(l.size());
        FSP_HIP(hipMemcpy(s.ra.list, l.data(), l.size() * 4, hipMemcpyHostToDevice));
        FSP_HIP(hipMemcpy(s.ra.count, &n, 4, hipMemcpyHostToDevice));
        return FSPANN_OK;
    };
    auto rescore = [&](const std::vector<int64_t>& qs) -> int {
        if (qs.empty()) return FSPANN_OK;
        int r = put_list(qs);
        if (r) return r;
        if ((r = refine_store_list(c, nq, s.q, s.q_dtype, B, s.sa.sel, s.sa.cnt, k, s.out_ids, s.out_dist, s.out_count, s.scored, s.ra.list, s.ra.count))) return r;
        FSP_HIP(hipStreamSynchronize(c->stream));
        return FSPANN_OK;
    };
    int64_t d1 = 0, d2 = 0, left = 0;
    int r = resolve_queries(c, g1, s.sa.codes, probe_override, static_cast<int32_t>(B), B, s.sa.sel, nullptr, s.sa.cnt, nullptr, nullptr, &d1, &left);
    if (r) return r;
    if ((r = rescore(g1))) return r;
    std::vector<int32_t> cnt(n4 / 4);
    std::vector<int64_t> again;
    if (!g1.empty()) {
        std::vector<int32_t> bad(n4 / 4), oc(n4 / 4), sc(n4 / 4);
        FSP_HIP(hipMemcpy(bad.data(), s.sa.bad, n4, hipMemcpyDeviceToHost));
        FSP_HIP(hipMemcpy(oc.data(), s.out_count, n4, hipMemcpyDeviceToHost));
        FSP_HIP(hipMemcpy(sc.data(), s.scored, n4, hipMemcpyDeviceToHost));
        FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
        for (int64_t i : g1)
            if (bad[i] == 0 && cnt[i] >= 0 && sc[i] > 0 && (oc[i] < k || static_cast<int64_t>(sc[i]) < 10 * static_cast<int64_t>(k))) {
                again.push_back(i);
                const int32_t one = 1;
                FSP_HIP(hipMemcpy(s.retried + i, &one, 4, hipMemcpyHostToDevice));
            }
    }
    std::vector<int64_t> s2 = g2;
    if (!again.empty() && !same) {
        if ((r = put_list(again))) return r;
        if ((r = route_list_dev(c, nq, s.sa.codes, 10, B, s.sa.sel, s.sa.cnt, s.ra.list, s.ra.count))) return r;
        FSP_HIP(hipStreamSynchronize(c->stream));
        FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
        for (int64_t i : again)
            if (cnt[i] == kRouteUnmodelled) g2.push_back(i);
        std::sort(g2.begin(), g2.end());
        s2.insert(s2.end(), again.begin(), again.end());
        std::sort(s2.begin(), s2.end());
    }
    if ((r = resolve_queries(c, g2, s.sa.codes, 10, static_cast<int32_t>(B), B, s.sa.sel, nullptr, s.sa.cnt, nullptr, nullptr, &d2, &left))) return r;
    if ((r = rescore(s2))) return r;
    *done += d1 + d2;
    return FSPANN_OK;
}

}  // namespace

extern "C" {

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
    // buffers, dtype pair (refused by name), n, dim and the strides: fspann_eval_metrics_typed_dev's checks at k = max(ks), no launch
    if (int rc = fspann_eval_metrics_typed_dev(c, n, base_dev, base_dtype, 0, q_dev, q_dtype, dim, kmax, ann_ids_dev, ann_stride, ann_count_dev, gt_ids_dev,
                                               gt_stride, recall_dev, ratio_dev)) return rc;
    if (nq < 0 || nq > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or nq > INT32_MAX");
    if (nq == 0) return FSPANN_OK;
    const size_t lds = eval_lds_bytes(dim, kmax);      // at most 32 KB of query + 24 KB at kmax = 1024
    const bool same_bytes = q_dtype == base_dtype && base_dtype != FSPANN_F32;
    with_row_type(base_dtype, [&](auto tb) {
        using TB = typename decltype(tb)::type;
        auto go = [&](auto tq) {
            using TQ = typename decltype(tq)::type;
            // 16 bytes at a time when every row starts on a 16-byte boundary and is whole pieces (and the query is in LDS)
            const bool vec = (static_cast<int64_t>(dim) * static_cast<int64_t>(sizeof(TB))) % 16 == 0 && (reinterpret_cast<uintptr_t>(base_dev) & 15) == 0 &&
                             dim <= kEvalQLdsMax;
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(nq)), dim3(kEvalThreads), lds, c->stream, static_cast<const TB*>(base_dev), n,
                                   static_cast<const TQ*>(q_dev), dim, nq, kv, nk, kmax, ann_ids_dev, ann_stride, ann_count_dev, gt_ids_dev, gt_stride, unique_dev,
                                   recall_dev, ratio_dev, cand_ratio_dev);
            };
            if (vec) launch(eval_kvariants_kernel<TB, TQ, true>);
            else launch(eval_kvariants_kernel<TB, TQ, false>);
        };
        if constexpr (DtypeOf<TB>::finite) { if (same_bytes) go(tb); else go(DtypeTag<float>{}); }
        else if constexpr (!std::is_same<TB, double>::value) go(DtypeTag<float>{});
    });
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

int fspann_search_fallback_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int probe_override, int64_t B, int k,
                               int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev,
                               int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, int32_t* retried_dev, int32_t* fellback_dev) {
    CHECK_CTX(c);
    int rc = check_retry_args(c, nq, q_dev, B, k, out_ids_dev, out_dist_dev, out_count_dev);
    if (rc || nq == 0) return rc;
    FallbackArea fa;
    if ((rc = fallback_area(c, nq, fa))) return rc;
    // search 1
    if ((rc = fspann_search_retry_dev(c, nq, q_dev, q_dtype, probe_override, B, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, sel_ids_dev,
                                      sel_count_dev, bad_dev, retried_dev))) return rc;
    SearchBufs s{nq, B, q_dev, q_dtype, k, out_ids_dev, out_dist_dev, out_count_dev, nullptr, nullptr, {}, {}};
    if (!search_area(c, nq, B, sel_ids_dev, sel_count_dev, bad_dev, s.sa)) return fail(FSPANN_E_STATE, "search work area missing");
    if ((rc = retry_area(c, nq, s.ra))) return rc;
    s.scored = scored_dev ? scored_dev : s.ra.scored;
    s.retried = retried_dev ? retried_dev : s.ra.retried;
    // the empty queries, ascending ...
    hipLaunchKernelGGL(fallback_pick_kernel<false>, dim3(1), dim3(kPickThreads), 0, c->stream, nq, k, s.sa.bad, s.sa.cnt, out_count_dev, s.scored, fa.member,
                       fellback_dev ? fellback_dev : fa.fellback, fa.list, fa.count);
    FSP_HIP(hipGetLastError());
    // ... and search 2 over them
    return search_list_dev(c, s, fallback_probes(c, probe_override), fa.list, fa.count, fa.member);
}

int fspann_search_fallback_finish_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int probe_override, int64_t B, int k,
                                      int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev,
                                      int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, int32_t* retried_dev,
                                      int32_t* fellback_dev, int64_t* resolved) {
    CHECK_CTX(c);
    if (resolved) *resolved = 0;
    if (int rc = refuse_row_only(q_dtype, "q_dtype")) return rc;
    int rc = check_retry_args(c, nq, q_dev, B, k, out_ids_dev, out_dist_dev, out_count_dev);
    if (rc || nq == 0) return rc;
    SearchBufs s{nq, B, q_dev, q_dtype, k, out_ids_dev, out_dist_dev, out_count_dev, nullptr, nullptr, {}, {}};
    if (!search_area(c, nq, B, sel_ids_dev, sel_count_dev, bad_dev, s.sa) || !c->ws_retry.p ||
        c->ws_retry.bytes < 3 * ((static_cast<size_t>(nq) * 4 + 255) & ~size_t(255)) + 256 || !c->ws_fallback.p || c->ws_fallback.bytes < fallback_area_bytes(nq))
        return fail(FSPANN_E_STATE, "no fspann_search_fallback_dev call of this size precedes");
    FallbackArea fa;
    if ((rc = retry_area(c, nq, s.ra)) || (rc = fallback_area(c, nq, fa))) return rc;
    s.scored = scored_dev ? scored_dev : s.ra.scored;
    s.retried = retried_dev ? retried_dev : s.ra.retried;
    int32_t* fellback = fellback_dev ? fellback_dev : fa.fellback;
    const int F = fallback_probes(c, probe_override);
    return guarded([&]() -> int {
        const size_t n4 = static_cast<size_t>(nq) * 4;
        FSP_HIP(hipStreamSynchronize(c->stream));
        std::vector<int32_t> cnt(static_cast<size_t>(nq));
        FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
        bool any = false;
        for (int64_t i = 0; i < nq && !any; i++) any = cnt[i] == kRouteUnmodelled;
        if (!any) return FSPANN_OK;
        std::vector<int32_t> ret(static_cast<size_t>(nq)), fb(static_cast<size_t>(nq));
        FSP_HIP(hipMemcpy(ret.data(), s.retried, n4, hipMemcpyDeviceToHost));
        FSP_HIP(hipMemcpy(fb.data(), fellback, n4, hipMemcpyDeviceToHost));
        // flagged by search 1 (never fallen back) in its pass 1 / its pass 2, flagged by search 2 in its pass 1 / its pass 2
        std::vector<int64_t> a1, a2, b1, b2;
        for (int64_t i = 0; i < nq; i++)
            if (cnt[i] == kRouteUnmodelled) (fb[i] ? (ret[i] ? b2 : b1) : (ret[i] ? a2 : a1)).push_back(i);
        int64_t done = 0;
        // search 1's flagged queries, as fspann_search_retry_finish_dev finishes them
        int r = finish_flagged(c, s, probe_override, a1, a2, &done);
        if (r) return r;
        // the fallback of those: rule and search 2 as in the _dev call, over them only
        std::vector<int64_t> fin(a1);
        fin.insert(fin.end(), a2.begin(), a2.end());
        std::sort(fin.begin(), fin.end());
        if (!fin.empty()) {
            std::vector<int32_t> bad(static_cast<size_t>(nq)), oc(static_cast<size_t>(nq)), member(static_cast<size_t>(nq), 0), l;
            FSP_HIP(hipMemcpy(bad.data(), s.sa.bad, n4, hipMemcpyDeviceToHost));
            FSP_HIP(hipMemcpy(oc.data(), out_count_dev, n4, hipMemcpyDeviceToHost));
            FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
            for (int64_t i : fin)
                if (bad[i] == 0 && cnt[i] >= 0 && oc[i] == 0) { l.push_back(static_cast<int32_t>(i)); member[i] = 1; }
            if (!l.empty()) {
                const int32_t n = static_cast<int32_t>(l.size()), one = 1;
                FSP_HIP(hipMemcpy(fa.list, l.data(), l.size() * 4, hipMemcpyHostToDevice));
                FSP_HIP(hipMemcpy(fa.count, &n, 4, hipMemcpyHostToDevice));
                FSP_HIP(hipMemcpy(fa.member, member.data(), n4, hipMemcpyHostToDevice));
                for (int32_t i : l) FSP_HIP(hipMemcpy(fellback + i, &one, 4, hipMemcpyHostToDevice));
                if ((r = search_list_dev(c, s, F, fa.list, fa.count, fa.member))) return r;
                FSP_HIP(hipStreamSynchronize(c->stream));
                FSP_HIP(hipMemcpy(cnt.data(), s.sa.cnt, n4, hipMemcpyDeviceToHost));
                FSP_HIP(hipMemcpy(ret.data(), s.retried, n4, hipMemcpyDeviceToHost));
                for (int32_t i : l)
                    if (cnt[i] == kRouteUnmodelled) (ret[i] ? b2 : b1).push_back(i);
                std::sort(b1.begin(), b1.end());
                std::sort(b2.begin(), b2.end());
            }
        }
        // search 2's flagged queries, with the probes of the pass that flagged them
        if ((r = finish_flagged(c, s, F, b1, b2, &done))) return r;
        if (resolved) *resolved = done;
        return FSPANN_OK;
    });
}

}  // extern "C"
