// route_recall.hip.h — recall attribution (include/fspann_route_recall.h, api_route_recall.hip.h): the rank of every
// ground-truth id in a candidate list, and the recall ceilings those ranks imply.  The rank of an id in Route's full list
// (fspann_route_dev at limit = INT32_MAX) is the refinement limit at which the search starts to score it, so one pass over the list
// says whether a lost neighbour was never offered (probes, tables) or was cut by stage A.5 (refinementLimit).  No candidate row is read.
#pragma once
#include "fspann_common.h"

namespace fspann {

constexpr int kRankThreads = 256;
constexpr int kRankMaxKg = 1024;           // ground-truth ids per query
constexpr int kRankMinSlots = 64;          // smallest LDS table
constexpr int kRankMaxSlots = 4096;        // largest: 32 KB, a quarter full at kg = 1024
constexpr int kRankUnroll = 4;             // 16-byte loads a lane has in flight per step of the list walk
constexpr int32_t kRankNone = -1;          // rank: the id is not among the live entries of the list
constexpr int32_t kRankUnknown = -2;       // rank: the list itself is unknown (list_count -1: flagged by Route, not resolved)
constexpr int32_t kRankEmptyKey = -1;      // table: a free slot (a negative ground-truth id is padding and never enters the table)
constexpr int32_t kRankNoPos = INT32_MAX;  // table: the slot's id has not been met in the list

// Slots of the table for kg ids: a power of two, an eighth full where 32 KB allow it (kg <= 512), a quarter full at most.  Nearly
// every list entry misses the table, and a wave walks until the longest chain of its 64 lanes ends, so what the list walk costs is
// the tail of the chain lengths: short chains are worth more here than a small table (DESIGN.md 3.6d has the measurements).
inline int rank_table_slots(int kg) {
    int s = kRankMinSlots;
    while (s < 8 * kg && s < kRankMaxSlots) s <<= 1;
    return s;
}
inline size_t rank_lds_bytes(int kg) { return static_cast<size_t>(rank_table_slots(kg)) * 8; }      // keys | positions

typedef int32_t rank_i4 __attribute__((ext_vector_type(4)));      // one 16-byte load of the list walk

// Double hashing: the first slot of an id, and the stride of its walk — odd, so that the walk visits every slot of a power-of-two
// table; ids that collide in one slot part ways at the next, so no clusters build up as they do under linear probing.
__device__ __forceinline__ uint32_t rank_hash(int32_t id, int shift) { return (static_cast<uint32_t>(id) * 2654435761u) >> shift; }
__device__ __forceinline__ uint32_t rank_step(int32_t id) { return ((static_cast<uint32_t>(id) * 0x85EBCA6Bu) >> 15) | 1u; }

// One list entry against the table: a slot that holds its id takes the minimum of the positions.  The walk ends at the id or at a
// free slot; the table is never more than a quarter full, so there always is one.  Per-lane exits, nothing shared but the LDS atomic.
__device__ __forceinline__ void rank_probe(const int32_t* keys, int32_t* pos, uint32_t mask, int shift, int32_t id, int32_t j) {
    if (id < 0) return;
    uint32_t h = rank_hash(id, shift);
    const uint32_t st = rank_step(id);
    for (;;) {
        const int32_t k = keys[h];
        if (k == id) { atomicMin(&pos[h], j); return; }
        if (k == kRankEmptyKey) return;
        h = (h + st) & mask;
    }
}

// One workgroup per query.  (1) the kg ground-truth ids go into an open-addressed LDS table (identical ids share a slot);
// (2) the c live entries of the list are streamed once — the row starts at q * list_stride * 4 bytes, which for an odd stride is
// not 16-byte aligned, so up to three head entries go one by one, the aligned middle as 16-byte loads, kRankUnroll of them in flight
// per lane, and up to three tail entries one by one — every entry probes the table, a hit takes an LDS atomicMin on its position;
// (3) every ground-truth slot reads its id's entry and writes rank and score.  Every trip count comes from c, read once per
// workgroup, so all loops and barriers are workgroup-uniform.  Which slot an id lands in depends on the order of the waves, the
// minimum it ends with does not.
__global__ __launch_bounds__(kRankThreads) void gt_rank_kernel(const int32_t* __restrict__ list_ids, const int32_t* __restrict__ list_score, int64_t list_stride,
                                                               const int32_t* __restrict__ list_count, const int32_t* __restrict__ gt_ids, int64_t gt_stride, int kg,
                                                               int slots, int shift, int32_t* __restrict__ rank, int32_t* __restrict__ gt_score) {
    extern __shared__ __align__(16) unsigned char rank_smem[];
    int32_t* keys = reinterpret_cast<int32_t*>(rank_smem);
    int32_t* pos = keys + slots;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int32_t* gt = gt_ids + q * gt_stride;
    int32_t* out_rank = rank + q * kg;
    int32_t* out_score = gt_score ? gt_score + q * kg : nullptr;

    const int32_t cnt = list_count ? list_count[q] : INT32_MAX;
    const int32_t c = static_cast<int32_t>(cnt < list_stride ? cnt : list_stride);
    if (c <= 0) {                                  // nothing live: not seen, or (count -1) a list nobody knows
        const int32_t r = cnt == -1 ? kRankUnknown : kRankNone;
        for (int i = tid; i < kg; i += kRankThreads) {
            out_rank[i] = r;
            if (out_score) out_score[i] = -1;
        }
        return;
    }

    const uint32_t mask = static_cast<uint32_t>(slots) - 1;
    for (int i = tid; i < slots; i += kRankThreads) { keys[i] = kRankEmptyKey; pos[i] = kRankNoPos; }
    __syncthreads();
    for (int i = tid; i < kg; i += kRankThreads) {
        const int32_t id = gt[i];
        if (id < 0) continue;
        uint32_t h = rank_hash(id, shift);
        for (;;) {
            const int32_t prev = atomicCAS(&keys[h], kRankEmptyKey, id);
            if (prev == kRankEmptyKey || prev == id) break;
            h = (h + rank_step(id)) & mask;
        }
    }
    __syncthreads();

    const int32_t* row = list_ids + q * list_stride;
    const int32_t mis = static_cast<int32_t>((reinterpret_cast<uintptr_t>(row) >> 2) & 3);      // (entries are 4-byte aligned)
    const int32_t head = ((4 - mis) & 3) < c ? ((4 - mis) & 3) : c;
    const int32_t nvec = (c - head) >> 2;
    const int32_t tail0 = head + (nvec << 2);
    if (tid < head) rank_probe(keys, pos, mask, shift, row[tid], tid);
    if (tid < c - tail0) rank_probe(keys, pos, mask, shift, row[tail0 + tid], tail0 + tid);
    const rank_i4* vrow = reinterpret_cast<const rank_i4*>(row + head);
    for (int32_t v0 = 0; v0 < nvec; v0 += kRankThreads * kRankUnroll) {
        rank_i4 x[kRankUnroll];
#pragma unroll
        for (int u = 0; u < kRankUnroll; u++) {
            const int32_t v = v0 + u * kRankThreads + tid;
            x[u] = v < nvec ? __builtin_nontemporal_load(vrow + v) : rank_i4{-1, -1, -1, -1};
        }
#pragma unroll
        for (int u = 0; u < kRankUnroll; u++) {
            const int32_t v = v0 + u * kRankThreads + tid;
            if (v >= nvec) continue;               // (its words are -1; and past nvec the position below could leave int32)
            const int32_t j = head + (v << 2);
            rank_probe(keys, pos, mask, shift, x[u].x, j);
            rank_probe(keys, pos, mask, shift, x[u].y, j + 1);
            rank_probe(keys, pos, mask, shift, x[u].z, j + 2);
            rank_probe(keys, pos, mask, shift, x[u].w, j + 3);
        }
    }
    __syncthreads();

    for (int i = tid; i < kg; i += kRankThreads) {
        const int32_t id = gt[i];
        int32_t r = kRankNone;
        if (id >= 0) {
            uint32_t h = rank_hash(id, shift);
            while (keys[h] != id) h = (h + rank_step(id)) & mask;      // (step 1 put it there)
            if (pos[h] != kRankNoPos) r = pos[h];
        }
        out_rank[i] = r;
        if (out_score) out_score[i] = r >= 0 ? list_score[q * list_stride + r] : -1;
    }
}

constexpr int kCeilMaxK = 64;              // k values per call: one lane each (fspann_eval_kvariants_dev's bound)
constexpr int kCeilMaxLimits = 16;
constexpr int kCeilThreads = 256;

struct CeilArgs {                          // travels in the kernel arguments
    int32_t k[kCeilMaxK];
    int32_t limit[kCeilMaxLimits + 1];     // limit[nl] = INT32_MAX: Route's own ceiling
    int32_t nk, nl, kmax;
};

// hits / ceiling [nl + 1][nk][nq] from rank [nq][rank_stride].  One workgroup per query, its waves take the planes in turn: a wave
// walks the first kmax ranks 64 at a time, one ballot per step, and lane j counts the bits below ks[j].  A rank of -2 among the first
// ks[j] makes that k's answer "unknown": hits -1, ceiling NaN.
__global__ __launch_bounds__(kCeilThreads) void recall_ceiling_kernel(const int32_t* __restrict__ rank, int64_t rank_stride, int64_t nq, CeilArgs a,
                                                                      int32_t* __restrict__ hits, double* __restrict__ ceiling) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = blockIdx.x;
    const int32_t* r = rank + q * rank_stride;
    const int32_t kj = lane < a.nk ? a.k[lane] : 0;
    for (int l = wave; l <= a.nl; l += kCeilThreads / 64) {
        const int32_t lim = a.limit[l];
        int32_t n = 0, unknown = 0;
        for (int32_t i0 = 0; i0 < a.kmax; i0 += 64) {
            const int32_t x = i0 + lane < a.kmax ? r[i0 + lane] : kRankNone;
            const unsigned long long hit = __ballot(x >= 0 && x < lim), unk = __ballot(x == kRankUnknown);
            const int32_t below = kj - i0;             // this lane's k covers the step's first `below` lanes
            const unsigned long long m = below >= 64 ? ~0ull : below <= 0 ? 0ull : (1ull << below) - 1;
            n += __popcll(hit & m);
            unknown += __popcll(unk & m);
        }
        if (lane < a.nk) {
            const int64_t o = (static_cast<int64_t>(l) * a.nk + lane) * nq + q;
            hits[o] = unknown ? -1 : n;
            if (ceiling) ceiling[o] = unknown ? __builtin_nan("") : static_cast<double>(n) / static_cast<double>(kj);
        }
    }
}

}  // namespace fspann
