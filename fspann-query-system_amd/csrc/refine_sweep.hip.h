// refine_sweep.hip.h — Refine at several refinement limits in one scan (include/fspann_sweep.h, api_sweep.hip.h).
//
// The top-K of QueryServiceImpl.search at limit B is the top-K of the FIRST B entries of the score-ordered candidate list, ties broken
// by candidate position (QSI:177-214, 238-316): the results at the limits B_0 < B_1 < ... are snapshots of ONE walk over the list.
// Two steps.  (a) The scan of refine.hip.h runs once, at the largest limit, with its key epilogue (refine_keys_emit): the row walk —
// the one part whose arithmetic order is the result — is the code of every other Refine call, for every row dtype, query dtype and
// layout.  (b) refine_prefix_topk_kernel walks each query's keys in candidate order, keeps the best k so far sorted by (key, candidate
// position) in LDS, and writes a snapshot behind every limit.
// Part of the single translation unit fspann_api.hip; product code, no CPU fallback.
#pragma once
#include "refine.hip.h"

namespace fspann {

constexpr int kSweepMaxLimits = 16;
constexpr int kSweepMaxK = 1024;
constexpr int kSweepThreads = 256;

struct SweepLimits {               // travels in the kernel arguments
    int32_t v[kSweepMaxLimits];    // strictly ascending
    int32_t n;
};

// The scan with the key epilogue as a stream (refine_stream_run; the layouts it takes), over the batch or (kList) over the queries
// qlist[0 .. *qcount), launched with the grid of the whole batch.
template <typename TC, typename TQ, int DC, bool GATHER, bool kList>
__global__ __launch_bounds__(kRefRows, (GATHER ? 2 : 4)) void refine_stream_keys_kernel(RefineArgs<TC, TQ> a, int64_t nq, const int32_t* __restrict__ qlist,
                                                                                      const int32_t* __restrict__ qcount) {
    extern __shared__ __align__(16) unsigned char smem[];
    if constexpr (kList) {
        const int64_t nsel = *qcount;
        if (static_cast<int64_t>(blockIdx.x) >= nsel * a.nchunks) return;
        refine_stream_run<TC, TQ, DC, GATHER, RefineNoFix, false, true, true>(a, smem, static_cast<int64_t>(blockIdx.x), static_cast<int64_t>(gridDim.x), nsel, false,
                                                                              RefineNoFix(), qlist);
    } else {
        refine_stream_run<TC, TQ, DC, GATHER, RefineNoFix, false, false, true>(a, smem, static_cast<int64_t>(blockIdx.x), static_cast<int64_t>(gridDim.x), nq, false);
    }
}

// The same with one workgroup per chunk (layouts the stream does not take): block = (query or list slot, chunk).
template <typename TC, typename TQ, int DC, bool VEC, bool GATHER>
__global__ __launch_bounds__(kRefRows, (DC * sizeof(TC) <= 128 ? 4 : (DC * sizeof(TC) <= 256 ? 2 : 1))) void refine_scan_keys_kernel(
        RefineArgs<TC, TQ> a, const int32_t* __restrict__ qlist, const int32_t* __restrict__ qcount) {
    extern __shared__ __align__(16) unsigned char smem[];
    int64_t bidx = static_cast<int64_t>(blockIdx.x);
    if (qlist) {                                                   // (uniform: a kernel argument)
        const int64_t slot = bidx / a.nchunks;
        if (slot >= static_cast<int64_t>(*qcount)) return;
        bidx = static_cast<int64_t>(qlist[slot]) * a.nchunks + (bidx - slot * a.nchunks);
    }
    refine_scan_block<TC, TQ, DC, VEC, GATHER, true>(a, smem, bidx);
}

// Counts as a sweep scan takes them: clip[q] = min(max(count[q], 0), cap) with cap = bmax, or (cap_q given: pass 2 of the search
// sweep) the query's own largest retried limit.  Route's -1 / PENDING markers and a query nobody retried score nothing.
__global__ __launch_bounds__(256) void sweep_clip_kernel(int64_t nq, const int32_t* __restrict__ count, int32_t bmax, const int32_t* __restrict__ cap_q,
                                                         int32_t* __restrict__ clip) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= nq) return;
    const int32_t cap = cap_q ? min(cap_q[i], bmax) : bmax;
    clip[i] = min(max(count[i], 0), max(cap, 0));
}

// One workgroup per query (list mode: per list slot, leaving at once past *qcount).  keys [.][kpitch]: the scan's keys in candidate
// order; count: the clipped counts (0 <= count <= limits[n - 1] <= kpitch).  The walk goes in pieces of at most 256 keys that never
// straddle a limit.  The best k so far live in LDS sorted by (key, candidate position), 16 bytes per entry (key lo, key hi,
// position, -), in one of two buffers: a piece contributes only the keys strictly below the current k-th (later positions lose
// ties), and when it contributes any, every old entry and every newcomer is written at its new rank into the other buffer — an old
// entry moves up by the newcomers in front of it, a newcomer stands behind the old entries with key <= its own and the newcomers in
// front of it (refine_topk_running's scheme; nothing is held in registers across the barrier, so k = 1024 costs no register array).
// Behind the piece that ends at limit j (or at the end of the list) snapshot j is written: ids (read from cand_ids by position) and
// distances of the first min(k, scored so far), padded with -1 / +inf, out_count and scored; take [nl][nq] (optional) = 0 suppresses
// that write.  Planes are [nl][nq][k] / [nl][nq] with nq the whole batch.  A non-finite query has no valid key (the scan scored
// nothing for it): empty rows, scored = 0.
// Every loop bound derives from the kernel arguments, the query's count and the survivor count S, each made a scalar
// (readfirstlane) where it comes from memory, so every loop exit and every barrier is wave-uniform.
__global__ __launch_bounds__(kSweepThreads) void refine_prefix_topk_kernel(const uint64_t* __restrict__ keys, int64_t kpitch, const int32_t* __restrict__ cand_ids,
                                                                           int64_t stride, const int32_t* __restrict__ count, SweepLimits lim, int k, int64_t nq,
                                                                           int32_t* __restrict__ out_ids, double* __restrict__ out_dist,
                                                                           int32_t* __restrict__ out_count, int32_t* __restrict__ scored,
                                                                           const int32_t* __restrict__ take, const int32_t* __restrict__ qlist,
                                                                           const int32_t* __restrict__ qcount) {
    extern __shared__ __align__(16) unsigned char sweep_smem[];
    uint4* s_best = reinterpret_cast<uint4*>(sweep_smem);          // [2][k]
    __shared__ uint4 s_new[kSweepThreads];                         // survivors of a piece, in candidate order
    __shared__ int s_wcnt[kSweepThreads / 64], s_wval[kSweepThreads / 64];
    int64_t qi = blockIdx.x;
    if (qlist) {
        if (qi >= static_cast<int64_t>(*qcount)) return;
        qi = qlist[qi];
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cnt = __builtin_amdgcn_readfirstlane(count[qi]);
    const uint64_t* __restrict__ qkeys = keys + qi * kpitch;
    const int32_t* __restrict__ qids = cand_ids + qi * stride;
    auto key_of = [](const uint4 e) { return static_cast<uint64_t>(e.x) | (static_cast<uint64_t>(e.y) << 32); };
    int cur = 0, L = 0, nvalid = 0, pos = 0;                       // scalars: list buffer, its length, valid keys and keys walked so far
    for (int j = 0; j < lim.n; j++) {
        const int end = min(cnt, lim.v[j]);
        while (pos < end) {
            const int n = min(kSweepThreads, end - pos);
            const uint4* best = s_best + cur * k;
            uint4* next = s_best + (cur ^ 1) * k;
            const uint64_t key = (tid < n) ? qkeys[pos + tid] : kInvalidKey;
            const bool valid = key != kInvalidKey;                 // (a valid key is a finite double's bits)
            uint64_t thr = kInvalidKey;                            // list not full: every valid key enters
            if (L == k) thr = key_of(best[k - 1]);
            const bool sv = valid && key < thr;                    // strictly: an equal key at a later position ranks behind the k-th
            const unsigned long long bm = __ballot(sv), bv = __ballot(valid);
            if (lane == 0) { s_wcnt[wave] = __popcll(bm); s_wval[wave] = __popcll(bv); }
            __syncthreads();   // (1) counts of all waves
            static_assert(kSweepThreads / 64 == 4, "four waves");
            const int c0 = s_wcnt[0], c1 = s_wcnt[1], c2 = s_wcnt[2], c3 = s_wcnt[3];
            const int S = __builtin_amdgcn_readfirstlane(c0 + c1 + c2 + c3);
            nvalid += __builtin_amdgcn_readfirstlane(s_wval[0] + s_wval[1] + s_wval[2] + s_wval[3]);
            if (S > 0) {
                if (sv) {
                    const int base = (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
                    const int at = base + static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(bm >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(bm), 0u)));
                    s_new[at] = make_uint4(static_cast<uint32_t>(key), static_cast<uint32_t>(key >> 32), static_cast<uint32_t>(pos + tid), 0u);
                }
                __syncthreads();   // (2) the survivor list
                for (int t = tid; t < L + S; t += kSweepThreads) {
                    uint4 me;
                    int r;
                    if (t < L) {
                        me = best[t];
                        const uint64_t mk = key_of(me);
                        r = t;
                        for (int i = 0; i < S; i++) r += key_of(s_new[i]) < mk;       // an old entry wins ties (earlier position)
                    } else {
                        const int mi = t - L;
                        me = s_new[mi];
                        const uint64_t mk = key_of(me);
                        int lo = 0, hi = L;                                           // old entries with key <= mine
                        while (lo < hi) { const int mid = (lo + hi) >> 1; if (key_of(best[mid]) <= mk) lo = mid + 1; else hi = mid; }
                        r = lo;
                        for (int i = 0; i < S; i++) {
                            const uint64_t ok_ = key_of(s_new[i]);
                            r += (ok_ < mk) || (ok_ == mk && i < mi);                 // (the list is in candidate order)
                        }
                    }
                    if (r < k) next[r] = me;
                }
                L = min(k, L + S);
                cur ^= 1;
            }
            pos += n;
            __syncthreads();   // (3) the list is complete; s_new and the counts may be written again
        }
        // snapshot j (the barrier above, or nothing walked since the last snapshot: the list is as it was)
        const int64_t plane = static_cast<int64_t>(j) * nq + qi;
        if (take && take[plane] == 0) continue;                    // (uniform: one word per workgroup)
        const uint4* best = s_best + cur * k;
        for (int i = tid; i < k; i += kSweepThreads) {
            if (i < L) {
                const uint4 e = best[i];
                out_ids[plane * k + i] = qids[e.z];
                out_dist[plane * k + i] = __longlong_as_double(static_cast<long long>(key_of(e)));
            } else {
                out_ids[plane * k + i] = -1;
                out_dist[plane * k + i] = __longlong_as_double(0x7FF0000000000000LL);
            }
        }
        if (tid == 0) {
            out_count[plane] = L;
            if (scored) scored[plane] = nvalid;
        }
    }
}

// ---- the search sweep (fspann_search_sweep_dev) ----------------------------------------------------------------------------
// (QSI's retry predicate per (query, limit) and the list of the queries with any retried limit: SweepRule, search_pick.hip.h)

// unique [nl][nq] = |F_q| of the pass plane j ended on, as the search at limits[j] reports it: min(count, limits[j]); a count still
// flagged (-1) is passed on.  pass2: the retried planes ended on pass 2 (cnt2), the others — and all of them when pass 2 did not
// run — on pass 1 (cnt1).
__global__ __launch_bounds__(256) void sweep_unique_kernel(int64_t nq, SweepLimits lim, const int32_t* __restrict__ cnt1, const int32_t* __restrict__ cnt2,
                                                           const int32_t* __restrict__ retried, int pass2, int32_t* __restrict__ unique) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= nq) return;
    for (int j = 0; j < lim.n; j++) {
        const int64_t pl = static_cast<int64_t>(j) * nq + i;
        const int32_t c = (pass2 && retried[pl]) ? cnt2[i] : cnt1[i];
        unique[pl] = c < 0 ? c : min(c, lim.v[j]);
    }
}

}  // namespace fspann
