// gt_validate.hip.h — GroundtruthValidator's exact top-1 (api/.../GroundtruthValidator.java:219-265) as one fused kernel, and
// the two small kernels of validate (:123-153) around it.
//
// BaseVectorReader.l2sq (:219-242): per dimension `double d = query[i] - v` with query a double[] — a DOUBLE subtraction, where
// GroundtruthPrecompute.l2sq (groundtruth.hip.h) subtracts in float — then `sum += d * d` from 0.0 in dimension order.
// bruteForceNN (:252-265): a strict `<` running minimum over ascending indices from +inf, i.e. the lexicographic minimum of
// (sum bits as uint64, index) among the rows whose sum is < +inf (sums are >= +0 or NaN, so the bits order as the values do and
// every NaN pattern lies above +inf's); no such row: -1.
//
// A lane owns a row and keeps kGtQT running sums (one per query of its tile), as gt_dist_kernel does, so every sum is
// bit-identical to the JVM's whatever the launch shape.  Nothing goes to a [Q x N] matrix: a workgroup walks row tiles with a
// grid stride, each lane carries its best (sum, index) per query across its tiles (its rows ascend: strict `<` keeps the first),
// and the epilogue reduces lane -> wave (shuffles) -> workgroup (LDS) to one partial per (query, workgroup).  nn1_reduce_kernel
// takes the minimum of a query's partials.  The queries are widened to fp64 once by nn1_widen_q_kernel (exact for fp32), which
// also resolves the selection list, so the main kernel has one query type and reads it through the constant address space.
#pragma once
#include "groundtruth.hip.h"

#pragma clang fp contract(off)

namespace fspann {

constexpr int kNn1MaxGrid = 1024;                               // workgroups along the rows (4 per CU at 256 CUs)
constexpr unsigned long long kNn1InfBits = 0x7FF0000000000000ull;

// (a, ai) < (b, bi) lexicographically; index -1 (no row) orders last among equal sums
__device__ __forceinline__ bool nn1_before(unsigned long long a, int32_t ai, unsigned long long b, int32_t bi) {
    return a < b || (a == b && static_cast<uint32_t>(ai) < static_cast<uint32_t>(bi));
}

// qd[j][i] = (double) q[qsel ? qsel[s0 + j] : s0 + j][i] for the cq queries of a chunk; a selection outside [0, nq) becomes a
// row of NaN (every sum NaN: no row wins, -1 / +inf)
template <typename TQ>
__global__ __launch_bounds__(256) void nn1_widen_q_kernel(const TQ* __restrict__ q, int64_t nq, int d, const int64_t* __restrict__ qsel, int64_t s0,
                                                          int64_t cq, double* __restrict__ qd) {
    const int64_t total = cq * d;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t j = e / d;
        const int64_t src = qsel ? qsel[s0 + j] : s0 + j;
        qd[e] = (src >= 0 && src < nq) ? static_cast<double>(q[src * d + (e - j * d)]) : __longlong_as_double(0x7FF8000000000000LL);
    }
}

// pkey / pidx [cq][gridDim.x]: per query of the chunk and workgroup, the best (sum bits, row) over the workgroup's row tiles.
// kVec: every row starts on a 16-byte boundary and is a whole number of 16-byte pieces (the caller checks both).
template <typename TB, bool kVec>
__global__ __launch_bounds__(kGtRows) void nn1_exact_kernel(const TB* __restrict__ base, int64_t n, const double* __restrict__ qd, int64_t cq, int d,
                                                            unsigned long long* __restrict__ pkey, int32_t* __restrict__ pidx) {
    const int tid = threadIdx.x;
    const int64_t q0 = static_cast<int64_t>(blockIdx.y) * kGtQT;
    typedef const double __attribute__((address_space(4)))* const_row_t;     // uniform loads -> scalar loads
    const_row_t qt[kGtQT];
#pragma unroll
    for (int t = 0; t < kGtQT; t++) qt[t] = (const_row_t)(qd + min(q0 + t, cq - 1) * d);
    unsigned long long bk[kGtQT];
    int32_t bi[kGtQT];
#pragma unroll
    for (int t = 0; t < kGtQT; t++) { bk[t] = kNn1InfBits; bi[t] = -1; }
    const int64_t tiles = (n + kGtRows - 1) / kGtRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r = tile * kGtRows + tid;
        if (r < n) {
            double acc[kGtQT];
#pragma unroll
            for (int t = 0; t < kGtQT; t++) acc[t] = 0.0;
            const TB* row = base + r * d;
            if constexpr (kVec) {
                constexpr int kPer = 16 / static_cast<int>(sizeof(TB));
                constexpr int kSub = kPer < 8 ? kPer : 8;          // one query's kSub doubles are one scalar load (at most 16 dwords)
                const fsp_u32x4* pieces = reinterpret_cast<const fsp_u32x4*>(row);
                for (int i0 = 0; i0 < d; i0 += kPer) {
                    const fsp_u32x4 piece = pieces[i0 / kPer];
#pragma unroll
                    for (int s = 0; s < kPer; s += kSub) {
                        double v[kSub];
#pragma unroll
                        for (int e = 0; e < kSub; e++) v[e] = static_cast<double>(RowCodec<TB>::piece_f32(piece, s + e));
                        // query by query, the load of query t issued one query ahead and no earlier (gt_dist_kernel says why)
#pragma unroll
                        for (int t = 0; t < kGtQT; t++) {
                            const_row_t p = qt[t] + (i0 + s);
                            asm volatile("" : "+s"(p) : "v"(acc[(t + kGtQT - 2) % kGtQT]));
#pragma unroll
                            for (int e = 0; e < kSub; e++) {
                                const double dd = p[e] - v[e];            // double - double (GroundtruthValidator.java:230, 236)
                                const double sq = dd * dd;
                                acc[t] = acc[t] + sq;
                            }
                        }
                    }
                }
            } else {
                for (int i = 0; i < d; i++) {
                    const double v = static_cast<double>(static_cast<float>(row[i]));      // the element widened exactly
#pragma unroll
                    for (int t = 0; t < kGtQT; t++) {
                        const double dd = qt[t][i] - v;
                        const double sq = dd * dd;
                        acc[t] = acc[t] + sq;
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < kGtQT; t++) {
                const unsigned long long key = static_cast<unsigned long long>(__double_as_longlong(acc[t]));
                if (key < bk[t]) { bk[t] = key; bi[t] = static_cast<int32_t>(r); }      // strict: a lane's rows ascend, the first stays
            }
        }
    }
    // lane -> wave -> workgroup
    __shared__ unsigned long long s_k[kGtRows / 64][kGtQT];
    __shared__ int32_t s_i[kGtRows / 64][kGtQT];
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int t = 0; t < kGtQT; t++) {
        unsigned long long k = bk[t];
        int32_t i = bi[t];
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long ok = __shfl_xor(k, off);
            const int32_t oi = __shfl_xor(i, off);
            if (nn1_before(ok, oi, k, i)) { k = ok; i = oi; }
        }
        if (lane == 0) { s_k[wave][t] = k; s_i[wave][t] = i; }
    }
    __syncthreads();
    if (tid < kGtQT && q0 + tid < cq) {
        unsigned long long k = s_k[0][tid];
        int32_t i = s_i[0][tid];
        for (int w = 1; w < kGtRows / 64; w++)
            if (nn1_before(s_k[w][tid], s_i[w][tid], k, i)) { k = s_k[w][tid]; i = s_i[w][tid]; }
        pkey[(q0 + tid) * gridDim.x + blockIdx.x] = k;
        pidx[(q0 + tid) * gridDim.x + blockIdx.x] = i;
    }
}

// One wave per query: the minimum of its gx partials.  out_d2 may be null.
__global__ __launch_bounds__(64) void nn1_reduce_kernel(const unsigned long long* __restrict__ pkey, const int32_t* __restrict__ pidx, int gx,
                                                        int32_t* __restrict__ out_idx, double* __restrict__ out_d2) {
    const int64_t j = blockIdx.x;
    const int lane = threadIdx.x;
    unsigned long long k = kNn1InfBits;
    int32_t i = -1;
    for (int b = lane; b < gx; b += 64) {
        const unsigned long long ok = pkey[j * gx + b];
        const int32_t oi = pidx[j * gx + b];
        if (nn1_before(ok, oi, k, i)) { k = ok; i = oi; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ok = __shfl_xor(k, off);
        const int32_t oi = __shfl_xor(i, off);
        if (nn1_before(ok, oi, k, i)) { k = ok; i = oi; }
    }
    if (lane == 0) {
        out_idx[j] = i;
        if (out_d2) out_d2[j] = __longlong_as_double(static_cast<long long>(i < 0 ? kNn1InfBits : k));
    }
}

// What validate's loop leaves behind, and GroundtruthManager's id range
struct GtCompareOut {
    int64_t mismatches;
    int32_t n_mismatched, min_id, max_id, pad;
    int64_t mismatched[10];
};

// validate's loop (:123-153) by one wave, the sample in its iteration order: sampled query sel[j] with nearest row nn1[j] is
// skipped when it has no ground-truth row (sel[j] >= gt_rows), else a mismatch iff gt[sel[j]][0] != nn1[j]; the count, and the
// first 10 mismatching queries in order (retry_pick_kernel's ballot scan).  Also starts the id range at (INT32_MAX, -1).
__global__ __launch_bounds__(64) void gt_compare_kernel(const int64_t* __restrict__ sel, int64_t ns, const int32_t* __restrict__ nn1,
                                                        const int32_t* __restrict__ gt, int64_t gt_rows, int64_t gt_stride, GtCompareOut* __restrict__ out) {
    const int lane = threadIdx.x;
    const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    int64_t total = 0;
    for (int64_t j0 = 0; j0 < ns; j0 += 64) {
        const int64_t j = j0 + lane;
        const int64_t qi = j < ns ? sel[j] : -1;
        const bool p = qi >= 0 && qi < gt_rows && gt[qi * gt_stride] != nn1[j];
        const unsigned long long m = __ballot(p);
        const int64_t at = total + __popcll(m & lt);
        if (p && at < 10) out->mismatched[at] = qi;
        total += __popcll(m);
    }
    if (lane == 0) {
        out->mismatches = total;
        out->n_mismatched = static_cast<int32_t>(min(total, static_cast<int64_t>(10)));
        out->min_id = 0x7FFFFFFF;
        out->max_id = -1;
        out->pad = 0;
    }
}

// minId / maxId over all `count` ids (GroundtruthManager.java:121-122), into the range gt_compare_kernel started
__global__ __launch_bounds__(256) void gt_id_range_kernel(const int32_t* __restrict__ ids, int64_t count, GtCompareOut* __restrict__ out) {
    int32_t lo = 0x7FFFFFFF, hi = -1;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; e < count; e += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int32_t v = ids[e];
        lo = min(lo, v);
        hi = max(hi, v);
    }
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&out->min_id, lo);
        atomicMax(&out->max_id, hi);
    }
}

}  // namespace fspann
