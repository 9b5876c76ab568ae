// touch.hip.h — kernels of the touched-record set (fspann_touch_*, api_touch.hip.h): which records a search has loaded, decrypted
// and scored, for selective re-encryption (QSI:120,263,348-349 -> ReencryptionTracker.record; FSA:1739-1804 drains it).
//
// The set is one byte per handle.  A mark is a plain byte store of 1: idempotent, so no atomic and no read-modify-write; the line
// stays in the XCD's L2 and only the dirtied bytes are written back, so marks of different XCDs (or of different contexts' kernels)
// into one line do not overwrite each other.  A drain reads the bytes with 16-byte loads, counts them per tile, scans the tile
// counts and writes the ascending handles at their ranks (optionally clearing exactly the bytes it wrote out).
// Part of the single translation unit fspann_api.hip; product code, no CPU fallback.
#pragma once

namespace fspann {

constexpr int kTouchThreads = 256;
constexpr int64_t kTouchTile = int64_t(kTouchThreads) * 16;   // handles per tile: one 16-byte load per thread
constexpr int kTouchScanThreads = 1024;

// 1 per store row whose dim values are all finite — Refine's `ok` for a store row (QSI.isValid, QSI:407-413).  One wave per row.
template <typename T>
__global__ __launch_bounds__(kTouchThreads) void touch_store_valid_kernel(const T* __restrict__ store, int64_t n, int d, uint8_t* __restrict__ ok) {
    const int lane = threadIdx.x & 63;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * (kTouchThreads / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const T* r = store + row * d;
    bool bad = false;
    for (int i = lane; i < d; i += 64) bad = bad || !RowCodec<T>::finite(r[i]);
    const bool any_bad = __any(bad);
    if (lane == 0) ok[row] = any_bad ? 0 : 1;
}

// Query qi of a mark launch: workgroup w takes query w, or qlist[w] in list mode (workgroups past *qcount leave).  -1: none.
__device__ __forceinline__ int64_t touch_query(const int32_t* __restrict__ qlist, const int32_t* __restrict__ qcount) {
    const int64_t w = blockIdx.x;
    if (!qlist) return w;
    return (w < *qcount) ? static_cast<int64_t>(qlist[w]) : -1;
}

// Rows of F_q that the query's Refine scores: min(count, B) of them (count -1: a query flagged for the host, nothing), and none
// at all when the query holds NaN / Inf (QueryTokenFactory rejects it; Refine scores nothing for it either).
template <typename TQ>
__device__ __forceinline__ int64_t touch_rows(const TQ* __restrict__ q, int d, const int32_t* __restrict__ cnt, int64_t B, int64_t qi) {
    const int64_t n = min(static_cast<int64_t>(cnt[qi]), B);
    if (n <= 0) return 0;      // (uniform: every thread returns before the barrier below)
    bool nf = false;
    for (int i = threadIdx.x; i < d; i += kTouchThreads) nf = nf || !__builtin_isfinite(q[qi * d + i]);
    return __syncthreads_or(nf) ? 0 : n;
}

// Rows read from the resident store by id: row j counts when its id loaded (0 <= id < store_n) and the row is finite (store
// validity byte).  One workgroup per query, one thread per row.
template <typename TQ>
__global__ __launch_bounds__(kTouchThreads) void touch_mark_store_kernel(const TQ* __restrict__ q, int d, const int32_t* __restrict__ ids,
                                                                         const int32_t* __restrict__ cnt, int64_t B, const int32_t* __restrict__ qlist,
                                                                         const int32_t* __restrict__ qcount, const uint8_t* __restrict__ ok, int64_t store_n,
                                                                         uint8_t* __restrict__ set, int64_t n_set) {
    const int64_t qi = touch_query(qlist, qcount);
    if (qi < 0) return;
    const int64_t n = touch_rows(q, d, cnt, B, qi);
    for (int64_t j = threadIdx.x; j < n; j += kTouchThreads) {
        const int32_t id = ids[qi * B + j];
        if (id >= 0 && id < store_n && id < n_set && ok[id]) set[id] = 1;
    }
}

// Rows handed over by the caller ([nq][B][dim], present iff j < count): row j counts when all its values are finite.  The rows
// are read a second time (Refine read them first); the paths that hand rows over are host-bound (the JVM's decrypt loop, the
// native pipeline's AES-GCM stage), so that read is not on their critical path.  One wave per row.
template <typename TQ, typename TC>
__global__ __launch_bounds__(kTouchThreads) void touch_mark_rows_kernel(const TQ* __restrict__ q, int d, const TC* __restrict__ rows,
                                                                        const int32_t* __restrict__ ids, const int32_t* __restrict__ cnt, int64_t B,
                                                                        const int32_t* __restrict__ qlist, const int32_t* __restrict__ qcount,
                                                                        uint8_t* __restrict__ set, int64_t n_set) {
    const int64_t qi = touch_query(qlist, qcount);
    if (qi < 0) return;
    const int64_t n = touch_rows(q, d, cnt, B, qi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t j = wave; j < n; j += kTouchThreads / 64) {
        const int32_t id = ids[qi * B + j];
        if (id < 0 || id >= n_set) continue;          // (wave-uniform) not a handle of this index: nothing to mark
        const TC* r = rows + (qi * B + j) * d;
        bool bad = false;
        if constexpr (!RowCodec<TC>::always_finite)      // (a byte is never read a second time)
            for (int i = lane; i < d; i += 64) bad = bad || !RowCodec<TC>::finite(r[i]);
        const bool any_bad = __any(bad);
        if (lane == 0 && !any_bad) set[id] = 1;
    }
}

__device__ __forceinline__ int touch_nz_bytes(uint32_t x) {     // non-zero bytes of a word
    x |= x >> 4;
    x |= x >> 2;
    x |= x >> 1;
    return __popc(x & 0x01010101u);
}

__device__ __forceinline__ int touch_wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int touch_wave_incl_scan(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// Marked handles per tile of kTouchTile bytes (the set is allocated in whole tiles, its padding stays zero).
__global__ __launch_bounds__(kTouchThreads) void touch_tile_count_kernel(const uint8_t* __restrict__ set, int32_t* __restrict__ tile_cnt) {
    __shared__ int s_w[kTouchThreads / 64];
    const uint4 v = reinterpret_cast<const uint4*>(set + static_cast<int64_t>(blockIdx.x) * kTouchTile)[threadIdx.x];
    const int n = touch_wave_sum(touch_nz_bytes(v.x) + touch_nz_bytes(v.y) + touch_nz_bytes(v.z) + touch_nz_bytes(v.w));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kTouchThreads / 64; w++) t += s_w[w];
        tile_cnt[blockIdx.x] = t;
    }
}

// Exclusive scan of the tile counts (one workgroup; thread t owns a contiguous run of tiles) and their total.
__global__ __launch_bounds__(kTouchScanThreads) void touch_tile_scan_kernel(const int32_t* __restrict__ tile_cnt, int64_t ntiles,
                                                                            int32_t* __restrict__ tile_off, int64_t* __restrict__ total) {
    constexpr int nwv = kTouchScanThreads / 64;
    __shared__ int s_w[nwv + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t seg = (ntiles + kTouchScanThreads - 1) / kTouchScanThreads;
    const int64_t lo = min(ntiles, tid * seg), hi = min(ntiles, lo + seg);
    int s = 0;
    for (int64_t i = lo; i < hi; i++) s += tile_cnt[i];
    const int incl = touch_wave_incl_scan(s, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int w = 0; w < nwv; w++) { const int x = s_w[w]; s_w[w] = acc; acc += x; }
        s_w[nwv] = acc;
        *total = acc;
    }
    __syncthreads();
    int at = s_w[wave] + incl - s;
    for (int64_t i = lo; i < hi; i++) { tile_off[i] = at; at += tile_cnt[i]; }
}

// Ascending handles at their ranks: rank = tile offset + marked bytes in front within the tile.  Only ranks < cap are written, and
// at most the tile's counted entries (a mark that lands after the count is left for the next drain); reset clears exactly the
// bytes written out.
__global__ __launch_bounds__(kTouchThreads) void touch_compact_kernel(uint8_t* __restrict__ set, const int32_t* __restrict__ tile_cnt,
                                                                      const int32_t* __restrict__ tile_off, int32_t* __restrict__ out, int64_t cap,
                                                                      int reset) {
    __shared__ int s_w[kTouchThreads / 64];
    const int64_t base = tile_off[blockIdx.x];
    if (base >= cap) return;                          // (uniform) every rank of this tile is past the buffer
    const int64_t lim = min(cap, base + tile_cnt[blockIdx.x]);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t h0 = static_cast<int64_t>(blockIdx.x) * kTouchTile + static_cast<int64_t>(tid) * 16;
    const uint4 v = *reinterpret_cast<const uint4*>(set + h0);
    const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
    const int n = touch_nz_bytes(v.x) + touch_nz_bytes(v.y) + touch_nz_bytes(v.z) + touch_nz_bytes(v.w);
    const int incl = touch_wave_incl_scan(n, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int wbase = 0;
    for (int w = 0; w < wave; w++) wbase += s_w[w];
    int64_t r = base + wbase + incl - n;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if ((w4[i >> 2] >> ((i & 3) * 8)) & 0xFFu) {
            if (r < lim) {
                out[r] = static_cast<int32_t>(h0 + i);
                if (reset) set[h0 + i] = 0;
            }
            r++;
        }
    }
}

}  // namespace fspann
