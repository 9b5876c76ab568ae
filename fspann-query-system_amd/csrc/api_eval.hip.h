// api_eval.hip.h — ForwardSecureANNSystem.runQueries' loop (FSA:622-748) over a resident store, include/fspann_eval.h:
//   * fspann_eval_kvariants_dev: computeMetricsAtK for every k of kVariants from one result list (eval_sweep.hip.h);
//   * fspann_search_fallback_dev / _finish_dev: QSI.search, then the empty-result fallback (FSA:667-678): the empty queries are
//     searched again, a whole QSI.search with its adaptive retry, at max(2 base, 4) probes, in list mode, in place.
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once
#include "../../include/fspann_eval.h"

namespace {

// Work area of a fallback call behind fspann_search_retry_dev's: the fallback list [nq], member [nq] (the queries search 2 runs
// over), fellback [nq] (for the caller that passes none), the list's count.
struct FallbackArea {
    int32_t *list, *member, *fellback, *count;
    size_t lay(void* base, int64_t nq) {
        Carver w(base);
        list = w.take<int32_t>(static_cast<size_t>(nq) * 4);
        member = w.take<int32_t>(static_cast<size_t>(nq) * 4);
        fellback = w.take<int32_t>(static_cast<size_t>(nq) * 4);
        count = w.take<int32_t>(4);
        return w.off;
    }
};

// FSA:640, 668-673: the probes of the fallback search
int fallback_probes(const fspann_ctx* c, int probe_override) {
    const int po = probe_override >= 0 ? probe_override : c->cfg.probe_override;
    const int base = po >= 0 ? po : c->cfg.default_probes;
    return static_cast<int>(std::min<int64_t>(std::max<int64_t>(2 * static_cast<int64_t>(base), 4), INT32_MAX));
}

// QSI.search over the queries list[0 .. *count) (device, ascending; member[] flags them) at `probes` probes, in stream order, with
// search 1's codes and in place: list-mode Route and refine, the retry pick among them (into the retry area's list), and, unless
// `probes` already is what 10 gives, list-mode Route with 10 probes and refine over the picked.
int search_list_dev(fspann_ctx* c, const SearchBufs& s, int probes, const int32_t* list, const int32_t* count, const int32_t* member) {
    int rc;
    if ((rc = route_list_dev(c, s.nq, s.sa.codes, probes, s.B, s.sa.sel, s.sa.cnt, list, count))) return rc;
    if ((rc = refine_store_list(c, s, list, count))) return rc;
    if ((rc = launch_pick(c, s.nq, MemberRetryRule{pick_in(s), member, s.retried}, s.list, s.count))) return rc;
    if (effective_probes(c, probes) == effective_probes(c, 10)) return FSPANN_OK;
    if ((rc = route_list_dev(c, s.nq, s.sa.codes, 10, s.B, s.sa.sel, s.sa.cnt, s.list, s.count))) return rc;
    return refine_store_list(c, s, s.list, s.count);
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
        else if constexpr (DtypeOf<TB>::id != FSPANN_F64) go(DtypeTag<float>{});
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
    SearchBufs s;
    if ((rc = area_grow(c, c->ws_fallback, fa, nq)) ||
        (rc = retry_bufs(c, nullptr, nq, q_dev, q_dtype, B, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, sel_ids_dev, sel_count_dev, bad_dev, retried_dev, s)))
        return rc;
    // search 1
    if ((rc = search_retry_passes(c, s, probe_override))) return rc;
    // the empty queries, ascending ...
    if ((rc = launch_pick(c, nq, FallbackRule{pick_in(s), fa.member, fellback_dev ? fellback_dev : fa.fellback}, fa.list, fa.count))) return rc;
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
    FallbackArea fa;
    SearchBufs s;
    if ((rc = retry_bufs(c, "fspann_search_fallback_dev", nq, q_dev, q_dtype, B, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev, sel_ids_dev, sel_count_dev,
                         bad_dev, retried_dev, s))) return rc;
    if (!area_held(c->ws_fallback, fa, nq)) return fail(FSPANN_E_STATE, "no fspann_search_fallback_dev call of this size precedes");
    int32_t* fellback = fellback_dev ? fellback_dev : fa.fellback;
    const int F = fallback_probes(c, probe_override);
    return guarded([&]() -> int {
        const size_t n4 = static_cast<size_t>(nq) * 4;
        std::vector<int32_t> cnt;
        bool any = false;
        if (int r = flagged_counts(c, s, cnt, &any)) return r;
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
                if (fallback_wanted(bad[i], cnt[i], oc[i])) { l.push_back(static_cast<int32_t>(i)); member[i] = 1; }
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
