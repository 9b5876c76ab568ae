// search_pick.hip.h — what the search passes share on the device: the two rules that send a query through another pass (QSI's
// adaptive retry, runQueries' empty-result fallback), written once for host and device, and the ONE kernel that applies a rule to a
// batch and lists the queries it picks, ascending (api_retry.hip.h, api_eval.hip.h, api_sweep.hip.h).
// Part of the single translation unit fspann_api.hip; product code, no CPU fallback.
#pragma once
#include "refine_sweep.hip.h"

namespace fspann {

// QSI's retry predicate (QSI:159, 293, 444-447): not rejected (bad), its Route not flagged (count -1), at least one row scored, and
// fewer than k results or fewer than 10 k rows scored.
__host__ __device__ inline bool retry_wanted(int32_t bad, int32_t route_cnt, int32_t out_count, int32_t scored, int k) {
    return bad == 0 && route_cnt >= 0 && scored > 0 && (out_count < k || static_cast<int64_t>(scored) < 10 * static_cast<int64_t>(k));
}

// runQueries' fallback predicate (FSA:667): searched (not bad, Route not flagged) and nothing returned.
__host__ __device__ inline bool fallback_wanted(int32_t bad, int32_t route_cnt, int32_t out_count) {
    return bad == 0 && route_cnt >= 0 && out_count == 0;
}

// A rule travels by value in the kernel arguments.  mark(i) evaluates the predicate for query i, writes the rule's flags and says
// whether i is listed; listed(i) reads back what mark(i) stored.
struct PickIn {                      // what the rules read, [nq] each ([nl][nq] planes of out_count / scored in a sweep)
    const int32_t *bad, *route_cnt, *out_count, *scored;
    int k;
};

struct RetryRule {                   // the adaptive retry: retried[i]
    PickIn in;
    int32_t* retried;
    __device__ bool mark(int64_t i) const {
        const bool p = retry_wanted(in.bad[i], in.route_cnt[i], in.out_count[i], in.scored[i], in.k);
        retried[i] = p ? 1 : 0;
        return p;
    }
    __device__ bool listed(int64_t i) const { return retried[i] != 0; }
};

struct FallbackRule {                // the queries that fall back: member[i] and (optional) fellback[i]
    PickIn in;
    int32_t *member, *fellback;
    __device__ bool mark(int64_t i) const {
        const bool p = fallback_wanted(in.bad[i], in.route_cnt[i], in.out_count[i]);
        member[i] = p ? 1 : 0;
        if (fellback) fellback[i] = p ? 1 : 0;
        return p;
    }
    __device__ bool listed(int64_t i) const { return member[i] != 0; }
};

struct MemberRetryRule {             // the adaptive retry INSIDE search 2: among the queries of member[] only; the others keep their retried[]
    PickIn in;
    const int32_t* member;
    int32_t* retried;
    __device__ bool mark(int64_t i) const { return member[i] != 0 && RetryRule{in, retried}.mark(i); }
    __device__ bool listed(int64_t i) const { return member[i] != 0 && retried[i] != 0; }
};

struct SweepRule {                   // the retry per (query, limit): retried [nl][nq]; cap_q[i] = the query's largest retried limit (0: none)
    PickIn in;
    SweepLimits lim;
    int64_t nq;
    int32_t *retried, *cap_q;
    __device__ bool mark(int64_t i) const {
        const int32_t bad = in.bad[i], route_cnt = in.route_cnt[i];
        int32_t cap = 0;
        for (int j = 0; j < lim.n; j++) {
            const int64_t pl = static_cast<int64_t>(j) * nq + i;
            const bool p = retry_wanted(bad, route_cnt, in.out_count[pl], in.scored[pl], in.k);
            retried[pl] = p ? 1 : 0;
            if (p) cap = lim.v[j];
        }
        cap_q[i] = cap;
        return cap > 0;
    }
    __device__ bool listed(int64_t i) const { return cap_q[i] > 0; }
};

constexpr int kPickThreads = 1024;

// One workgroup: wave w owns the contiguous, 64-aligned slice [w * seg, (w + 1) * seg) of the batch.  Pass 1 marks and counts per
// wave, the wave counts are scanned, pass 2 writes each listed index at its rank: the list is ascending whatever nq is.  The same
// lane handles index i in both passes, so listed(i) reads that lane's own stores of mark(i).
template <class Rule>
__global__ __launch_bounds__(kPickThreads) void retry_pick_kernel(int64_t nq, Rule rule, int32_t* __restrict__ list, int32_t* __restrict__ count) {
    constexpr int nwv = kPickThreads / 64;
    __shared__ int s_base[nwv + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t seg = ((nq + nwv - 1) / nwv + 63) & ~int64_t(63);
    const int64_t lo = min(nq, wave * seg), hi = min(nq, lo + seg);
    int n = 0;
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        n += __popcll(__ballot(i < hi && rule.mark(i)));
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
        const bool p = i < hi && rule.listed(i);
        const unsigned long long m = __ballot(p);
        if (p) list[at + __popcll(m & lt)] = static_cast<int32_t>(i);
        at += __popcll(m);
    }
}

// The four instantiations, made here and not where the drivers launch them: the compiler emits an explicit instantiation where it
// stands, and every implicit one behind all other code of the translation unit.  A pick is one workgroup and a few microseconds
// long, so where its code lies shows in its time (profiles/notes/search_passes_fold.txt): these lie right behind the kernels that
// are no templates, the sweep's prefix top-k among them, which runs just before the sweep's pick.
template __global__ void retry_pick_kernel<SweepRule>(int64_t, SweepRule, int32_t*, int32_t*);
template __global__ void retry_pick_kernel<RetryRule>(int64_t, RetryRule, int32_t*, int32_t*);
template __global__ void retry_pick_kernel<FallbackRule>(int64_t, FallbackRule, int32_t*, int32_t*);
template __global__ void retry_pick_kernel<MemberRetryRule>(int64_t, MemberRetryRule, int32_t*, int32_t*);

template <class Rule>
int launch_pick(fspann_ctx* c, int64_t nq, const Rule& rule, int32_t* list, int32_t* count) {
    hipLaunchKernelGGL(retry_pick_kernel<Rule>, dim3(1), dim3(kPickThreads), 0, c->stream, nq, rule, list, count);
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

}  // namespace fspann
