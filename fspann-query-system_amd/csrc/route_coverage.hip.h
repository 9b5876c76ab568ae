// route_coverage.hip.h — the Route coverage map (include/fspann_route_coverage.h, api_route_coverage.hip.h): per
// (query, ground-truth id, table) the probe step at which Route reaches the id's partition and that partition's Hamming score, and
// from those records the recall ceiling of every (tables, divisions, probes) below the index's own.  The probe order of a table does
// not depend on the probe count and a smaller index is a sub-grid of tables, so one pass over the ids Route's staging reads answers
// the whole cube.  No candidate row is read.
#pragma once
#include "route.hip.h"
#include "route_recall.hip.h"

namespace fspann {

constexpr int kReachThreads = 256;
constexpr int kReachG = 16;                                  // lanes per table
constexpr int kReachGroups = kReachThreads / kReachG;        // tables per round
constexpr int kReachMaxProbes = 32;
constexpr int kReachU = 4;                                   // id loads a lane has in flight
constexpr int32_t kReachNone = -1;
constexpr int32_t kReachNoFirst = INT32_MAX;

// LDS of gt_reach_kernel: keys | first positions of the table, then per lane group the probe window [2P-1][3] and the probe list
// [P] int4.  kg = 1024, P = 32: 32 768 + 16 * 63 * 12 + 16 * 32 * 16 = 53 056 bytes, under the default 64 KB.
inline size_t reach_lds_bytes(int kg, int P) {
    return static_cast<size_t>(rank_table_slots(kg)) * 8 + static_cast<size_t>(kReachGroups) * ((2 * P - 1) * 12 + P * 16);
}

// The slot of a live ground-truth id, -1 when the table does not hold it.  Per-lane exits, nothing shared.
__device__ __forceinline__ int reach_find(const int32_t* keys, uint32_t mask, int shift, int32_t id) {
    if (id < 0) return -1;
    uint32_t h = rank_hash(id, shift);
    const uint32_t st = rank_step(id);
    for (;;) {
        const int32_t k = keys[h];
        if (k == id) return static_cast<int>(h);
        if (k == kRankEmptyKey) return -1;
        h = (h + st) & mask;
    }
}

// One workgroup per query.  (1) the output rows of the query are set to -1 and the live ground-truth ids (in range, not deleted) go
// into an open-addressed LDS table that keeps the first position i0 of every id; (2) the 16 lane groups take the tables in rounds,
// td = round * 16 + group: the group runs Route's probe (route_probe_table, P = probes_max) into its own LDS scratch, then streams
// the ids of the partitions it polled, in polling order; every id probes the table, and a hit takes a global atomicMin of
// (step << 16) | hamming on reach[q][i0][td] — as unsigned words, so that -1 is the largest; (3) the rows of repeated ids are
// copied from their first position.  The round count comes from TD, so the probe's ballots are met by every lane of every wave; the
// streaming loops have per-group trip counts and no cross-lane operation inside.  prm: tables, recs, rec_words, dir, dir_bits, ids,
// deleted_bits, codes, TD, W, P (= probes_max), S and n_ids are read, nothing else.
__global__ __launch_bounds__(kReachThreads) void gt_reach_kernel(RouteParams prm, const int32_t* __restrict__ gt_ids, int64_t gt_stride, int kg, int slots,
                                                                 int shift, int32_t* __restrict__ reach) {
    extern __shared__ __align__(16) unsigned char reach_smem[];
    int32_t* keys = reinterpret_cast<int32_t*>(reach_smem);
    int32_t* first = keys + slots;
    const int tid = threadIdx.x, lane = tid & 63;
    const int grp = tid / kReachG, gl = tid & (kReachG - 1), grp_in_wave = lane / kReachG;
    const int TD = prm.TD, W = prm.W, P = prm.P, S = prm.S;
    const int nd = 2 * P - 1;
    int4* plist = reinterpret_cast<int4*>(first + slots) + grp * P;                                   // (16-byte aligned: slots * 8 is)
    int32_t* w3 = reinterpret_cast<int32_t*>(reinterpret_cast<int4*>(first + slots) + kReachGroups * P) + grp * nd * 3;
    const int64_t q = blockIdx.x;
    const int32_t* gt = gt_ids + q * gt_stride;
    int32_t* out = reach + q * kg * TD;
    const uint32_t mask = static_cast<uint32_t>(slots) - 1;

    for (int i = tid; i < slots; i += kReachThreads) { keys[i] = kRankEmptyKey; first[i] = kReachNoFirst; }
    for (int64_t i = tid; i < static_cast<int64_t>(kg) * TD; i += kReachThreads) out[i] = kReachNone;
    __syncthreads();
    for (int i = tid; i < kg; i += kReachThreads) {
        const int32_t id = gt[i];
        if (id < 0 || id >= prm.n_ids) continue;
        if (prm.deleted_bits && ((prm.deleted_bits[id >> 5] >> (id & 31)) & 1u)) continue;
        uint32_t h = rank_hash(id, shift);
        for (;;) {
            const int32_t prev = atomicCAS(&keys[h], kRankEmptyKey, id);
            if (prev == kRankEmptyKey || prev == id) break;
            h = (h + rank_step(id)) & mask;
        }
        atomicMin(&first[h], i);
    }
    __syncthreads();                               // (its workgroup-scope release: the -1 rows are in L2 before an atomic of this workgroup meets them)

    const int rounds = (TD + kReachGroups - 1) / kReachGroups;
    for (int r = 0; r < rounds; r++) {
        const int td = r * kReachGroups + grp;
        const bool act = td < TD;
        const RouteTable tb = prm.tables[act ? td : 0];
        const uint64_t* qc = prm.codes + (q * TD + (act ? td : 0)) * W;
        const int np = route_probe_table(prm, act, qc, tb, kReachG, gl, grp_in_wave, w3, plist);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // lane 0 of the group wrote the list
        __builtin_amdgcn_wave_barrier();
        for (int s = 0; s < np; s++) {
            const int4 pr = plist[s];              // {partition, Hamming, id offset, size}
            const int32_t* ids = prm.ids + tb.ids_base + pr.z;
            const int sz = pr.w < S ? pr.w : S;
            const uint32_t rec = (static_cast<uint32_t>(s) << 16) | static_cast<uint32_t>(pr.y);
            for (int p0 = 0; p0 < sz; p0 += kReachG * kReachU) {
                int32_t idv[kReachU];
#pragma unroll
                for (int u = 0; u < kReachU; u++) {
                    const int pos = p0 + u * kReachG + gl;
                    idv[u] = pos < sz ? ids[pos] : -1;
                }
#pragma unroll
                for (int u = 0; u < kReachU; u++) {
                    const int h = reach_find(keys, mask, shift, idv[u]);
                    if (h >= 0) atomicMin(reinterpret_cast<uint32_t*>(out) + static_cast<int64_t>(first[h]) * TD + td, rec);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the list is read before the next round overwrites it
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();

    for (int i = tid; i < kg; i += kReachThreads) {
        const int h = reach_find(keys, mask, shift, gt[i]);
        if (h < 0) continue;                       // (padding, out of range, deleted: never entered, the row stays -1)
        const int i0 = first[h];
        if (i0 == i) continue;
        for (int td = 0; td < TD; td++)            // (the minima were taken in L2: read them there)
            out[static_cast<int64_t>(i) * TD + td] = __hip_atomic_load(out + static_cast<int64_t>(i0) * TD + td, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

constexpr int kCovMaxK = 64;               // k values per call: one lane each
constexpr int kCovMaxConfigs = 64;
constexpr int kCovThreads = 256;

struct CovArgs {                           // travels in the kernel arguments: 524 bytes
    uint16_t k[kCovMaxK];
    uint16_t tables[kCovMaxConfigs], divisions[kCovMaxConfigs], probes[kCovMaxConfigs];
    int32_t nk, nc, kmax;                  // kmax: the largest k
};

// hits / ceiling [nc][nk][nq] and score [nc][nq][kg] from reach [nq][kg][TD].  One workgroup per query, its waves take the
// configurations in turn: a wave walks the ground-truth positions 64 at a time (the first kmax, or all kg when the scores are
// wanted), every lane scans its position's records over the sub-grid t < tables, d < divisions — a wave-uniform trip count — then
// one ballot per step, and lane j counts the bits below ks[j] (as recall_ceiling_kernel does).
__global__ __launch_bounds__(kCovThreads) void route_coverage_kernel(const int32_t* __restrict__ reach, int kg, int TD, int D, int64_t nq, CovArgs a,
                                                                     int32_t* __restrict__ hits, double* __restrict__ ceiling, int32_t* __restrict__ score) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = blockIdx.x;
    const int32_t* rq = reach + q * kg * TD;
    const int32_t kj = lane < a.nk ? a.k[lane] : 0;
    const int32_t upto = score ? kg : a.kmax;
    for (int c = wave; c < a.nc; c += kCovThreads / 64) {
        const int Tc = a.tables[c], Dc = a.divisions[c], Pc = a.probes[c];
        int32_t n = 0;
        for (int32_t i0 = 0; i0 < upto; i0 += 64) {
            const int32_t i = i0 + lane;
            int32_t best = -1;
            if (i < upto) {
                const int32_t* row = rq + static_cast<int64_t>(i) * TD;
                for (int t = 0; t < Tc; t++)
                    for (int d = 0; d < Dc; d++) {
                        const int32_t rec = row[t * D + d];
                        const int32_t ham = rec & 0xFFFF;
                        if (rec >= 0 && (rec >> 16) < Pc && (best < 0 || ham < best)) best = ham;
                    }
                if (score) score[(static_cast<int64_t>(c) * nq + q) * kg + i] = best;
            }
            const unsigned long long hit = __ballot(best >= 0);
            const int32_t below = kj - i0;             // this lane's k covers the step's first `below` lanes
            const unsigned long long m = below >= 64 ? ~0ull : below <= 0 ? 0ull : (1ull << below) - 1;
            n += __popcll(hit & m);
        }
        if (lane < a.nk) {
            const int64_t o = (static_cast<int64_t>(c) * a.nk + lane) * nq + q;
            hits[o] = n;
            if (ceiling) ceiling[o] = static_cast<double>(n) / static_cast<double>(kj);
        }
    }
}

}  // namespace fspann
