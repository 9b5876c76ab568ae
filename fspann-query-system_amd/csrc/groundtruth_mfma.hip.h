// groundtruth_mfma.hip.h — the exact ground truth of fp32 queries over typed rows with an fp32 pre-filter on the matrix cores
// (fspann_groundtruth_mfma_dev / _store_dev, include/fspann_groundtruth_mfma.h; DESIGN.md 3.6f has the proof and the measurements).
//
// gt_dist_kernel pays the reference's fp64 chain for every (query, row, element), although only about k of a query's n distances
// are ever needed exactly.  Here every pair gets an fp32 estimate
//     a = max(0, |q|^2 + |x|^2 - 2 q.x)        norms: fp64 sums rounded once to fp32; q.x: v_mfma_f32_32x32x2_f32; the rest fp32
// with |a - D_ref| <= eps_q for every row x of the base (D_ref: the reference's value, eps_q below), so with a_k the k-th smallest
// estimate of a query every member of its true top-k has a <= a_k + 2 eps_q.  Those rows, the survivors, are listed, the reference's
// chain (the statements of gt_dist_kernel) runs on them alone, and the k smallest (distance bits, id) among them are the answer:
// bit-identical to fspann_groundtruth_rows_dev by construction.  What the bound does not cover never takes this path: a non-finite
// element, a squared norm above kGtmNormLimit or dim > kGtmMaxDim hands the whole call to gt_rows_run, and so does a query with more
// than kGtmCap survivors for itself (api_groundtruth_mfma.hip.h).
#pragma once
#include "fspann_common.h"

#pragma clang fp contract(off)

namespace fspann {

typedef float gtm_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kGtmRows = 128;           // base rows per workgroup of gtm_dist_kernel: 4 waves x 32 (the MFMA tile's lane dimension)
constexpr int kGtmQ = 128;              // queries per workgroup: 4 tiles of 32, one accumulator each
constexpr int kGtmCap = 4096;           // survivors one query may list; more: the query is finished by gt_rows_run
constexpr int kGtmSelThreads = 1024;
constexpr int kGtmColThreads = 256;
constexpr int kGtmFinThreads = 256;
constexpr int kGtmMaxDim = 65536;       // (dim + 4) 2^-24 <= 2^-8: the first-order rounding bound holds with the 1.01 of eps_q
constexpr double kGtmNormLimit = 0x1p120;      // |x|^2, |q|^2 above it: no fast path (below it no fp32 product, sum or difference overflows)
static_assert(kGtmCap >= kGtMaxK, "every member of a top-k must fit the survivor list");

// What the norm passes leave for the call: the largest |x|^2 of the base (fp64 bits: monotone for non-negative values), and whether
// any row or query is off the fast path.
struct GtmState {
    unsigned long long xmax_bits;
    int flag;
    int pad;
};

// Elements [k0, k0 + N) of one row, N = 16 / sizeof(T), in flight as they were loaded and widened exactly to fp32 on use; elements at
// k >= d read as zeros.  kVec (every row a whole number of 16-byte pieces on 16-byte boundaries): one 16-byte load at a clamped
// address, so the loop that issues it holds no branch; otherwise N element loads of any alignment.
template <typename T, bool kVec> struct GtmFrag;
template <typename T> struct GtmFrag<T, true> {
    static constexpr int N = RowCodec<T>::N;
    fsp_u32x4 p;
    bool live;
    __device__ __forceinline__ void load(const T* __restrict__ row, int k0, int d) {
        p = *reinterpret_cast<const fsp_u32x4*>(row + min(k0, d - N));      // (d >= N: d is a multiple of N)
        live = k0 < d;
    }
    __device__ __forceinline__ float get(int e) const { return live ? RowCodec<T>::piece_f32(p, e) : 0.0f; }
};
template <typename T> struct GtmFrag<T, false> {
    static constexpr int N = RowCodec<T>::N;
    float v[N];
    __device__ __forceinline__ void load(const T* __restrict__ row, int k0, int d) {
#pragma unroll
        for (int e = 0; e < N; e++) {
            const float x = static_cast<float>(row[min(k0 + e, d - 1)]);
            v[e] = (k0 + e < d) ? x : 0.0f;
        }
    }
    __device__ __forceinline__ float get(int e) const { return v[e]; }
};

__global__ void gtm_init_kernel(GtmState* __restrict__ st) {
    st->xmax_bits = 0ull;
    st->flag = 0;
    st->pad = 0;
}

// out[r] = |rows[r]|^2, summed in fp64 and rounded once to fp32; one lane per row.  A row with a non-finite element or a squared
// norm above kGtmNormLimit raises st->flag (an infinite or NaN element makes the fp64 sum infinite or NaN, so one comparison sees all
// three).  xmax_bits != nullptr (the base): the largest fp64 sum, by atomicMax on its bits.  The same kernel takes the queries of a
// chunk (T = float).
template <typename T, bool kVec>
__global__ __launch_bounds__(256) void gtm_norm_kernel(const T* __restrict__ rows, int64_t n, int d, float* __restrict__ out, GtmState* __restrict__ st,
                                                       unsigned long long* __restrict__ xmax_bits) {
    constexpr int N = RowCodec<T>::N;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    double s = 0.0;
    if (r < n) {
        const T* row = rows + r * d;
        for (int k0 = 0; k0 < d; k0 += N) {
            GtmFrag<T, kVec> f;
            f.load(row, k0, d);
#pragma unroll
            for (int e = 0; e < N; e++) {
                const double v = static_cast<double>(f.get(e));
                const double sq = v * v;
                s = s + sq;
            }
        }
        out[r] = static_cast<float>(s);
    }
    const bool bad = !(s <= kGtmNormLimit);
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(&st->flag, 1);
    if (xmax_bits) {
        double m = bad ? 0.0 : s;
        for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off));
        if ((threadIdx.x & 63) == 0) atomicMax(xmax_bits, static_cast<unsigned long long>(__double_as_longlong(m)));
    }
}

// dist[q][r] = bits of a = max(0, |q|^2 + |x_r|^2 - 2 q.x_r) for the kGtmQ queries x kGtmRows base rows of this workgroup
// (workgroup id = base tile * nqb + query block, as in gt8_dist_kernel: neighbours share the base tile, which so comes from HBM once).
//
// v_mfma_f32_32x32x2_f32: lane l gives A[l & 31][l >> 5] and B[l >> 5][l & 31]; with A = queries and B = base rows the result has
// the base row on the lane (l & 31) and the query on the register, query (reg & 3) + 8 (reg >> 2) + 4 (l >> 5), so the 32 lanes of a
// half store 128 contiguous bytes of one query's row of `dist`.  A wave owns 32 base rows and four accumulators, one per 32-query
// tile.  A K step is 2 N elements (N = elements per 16 bytes of TB): lane half h = l >> 5 reads the 16 bytes [k0 + h N, k0 + (h + 1) N)
// of ITS OWN row, widened in registers by the codec, and instruction j of the step multiplies element j of both halves — the K pair
// (k0 + j, k0 + N + j).  The queries follow the same permutation, so a dot product is the same set of products in another order
// (the bound of eps_q does not depend on the order) and nothing is transposed.
// The workgroup's query slab of a step, [2 N][kGtmQ] floats, goes through LDS once for the four waves: thread t loads the N floats
// [k0 + (t >> 7) N, + N) of query t & 127 and writes them k-major (a wave writes and reads 64 consecutive floats: no bank
// conflict).  Two slabs: while step s is multiplied from one, the loads of step s + 1 — issued before the MFMAs, base piece and query
// pieces — land in registers and are written to the other; one lds_barrier per step, which waits for LDS only and leaves the global
// loads in flight.  Every load is unconditional (clamped address, zeros at k >= d on both operands); rows >= n and queries >= nq
// are computed on a clamped index and never stored.  No fp64 in the loop.
template <typename TB, bool kVec>
__global__ __launch_bounds__(256) void gtm_dist_kernel(const TB* __restrict__ base, int64_t n, const float* __restrict__ q, int64_t nq, int d,
                                                       const float* __restrict__ xn, const float* __restrict__ qn, const GtmState* __restrict__ st,
                                                       unsigned* __restrict__ dist, int64_t ld, int nqb) {
    constexpr int N = RowCodec<TB>::N, kStep = 2 * N, kQP = N / 4;
    __shared__ float Qs[2][kStep][kGtmQ];
    if (st->flag) return;                                 // (uniform; the call goes to gt_rows_run)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int64_t bt = blockIdx.x / static_cast<unsigned>(nqb);
    const int64_t qb = blockIdx.x % static_cast<unsigned>(nqb);
    const int64_t r = bt * kGtmRows + wave * 32 + col;
    const TB* brow = base + min(r, n - 1) * d;
    const int sq = tid & (kGtmQ - 1), sh = tid >> 7;      // this thread's query and half of the slab
    const float* qrow = q + min(qb * kGtmQ + sq, nq - 1) * d;
    gtm_f32x16 acc[4];
#pragma unroll
    for (int g = 0; g < 4; g++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[g][i] = 0.0f;

    GtmFrag<TB, kVec> bcur, bnxt;
    GtmFrag<float, kVec> qf[kQP];
    auto q_load = [&](int k0) {
#pragma unroll
        for (int p = 0; p < kQP; p++) qf[p].load(qrow, k0 + sh * N + 4 * p, d);
    };
    auto q_store = [&](int buf) {
#pragma unroll
        for (int p = 0; p < kQP; p++)
#pragma unroll
            for (int e = 0; e < 4; e++) Qs[buf][sh * N + 4 * p + e][sq] = qf[p].get(e);
    };
    bcur.load(brow, h * N, d);
    q_load(0);
    q_store(0);
    lds_barrier();
    int buf = 0;
    for (int k0 = 0; k0 < d; k0 += kStep) {
        bnxt.load(brow, k0 + kStep + h * N, d);           // the next step's loads, in flight behind this step's MFMAs
        q_load(k0 + kStep);
#pragma unroll
        for (int j = 0; j < N; j++) {
            const float b = bcur.get(j);
#pragma unroll
            for (int g = 0; g < 4; g++) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[buf][h * N + j][32 * g + col], b, acc[g], 0, 0, 0);
        }
        q_store(buf ^ 1);
        lds_barrier();
        bcur = bnxt;
        buf ^= 1;
    }
    if (r >= n) return;
    const float nx = xn[r];
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int64_t qa = qb * kGtmQ + 32 * g + 4 * h;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int64_t qi = qa + (reg & 3) + 8 * (reg >> 2);
            if (qi < nq) {
                const float s = qn[qi] + nx;
                const float t = s - 2.0f * acc[g][reg];
                dist[qi * ld + r] = __float_as_uint(t > 0.0f ? t : 0.0f);       // (+0 for -0, and bits of non-negative floats are monotone)
            }
        }
    }
}

// The narrow select: the kk-th smallest key of a query's row of `dist` (kk = min(k, n)) by an MSB radix select over its four 8-bit
// digits, four keys per 16-byte load — gt8_select_kernel without the id digits, the collection and the ordering (its histogram
// helper gt8_hist_add is called as it is).  Then the query's threshold, thr = a_k + 2 eps_q rounded UP in fp32, as bits:
//     eps_q = 1.01 [ 2 (d + 4) 2^-24 |q| X + 2^-21 (|q| + X)^2 ] + d 2^-120          X = the largest |x| of the base
// from the fp32 |q|^2 inflated by its own rounding and the fp64 X^2, in fp64.
// (gtm_kth_body: the kernel but for eps_q, which eps(qi) gives; gtm16_kth_kernel of groundtruth_mfma16.hip.h is the other caller)
template <class Eps>
__device__ __forceinline__ void gtm_kth_body(const unsigned* __restrict__ dist, int64_t ld, int64_t n, int k, const GtmState* __restrict__ st,
                                             unsigned* __restrict__ thr, Eps eps_of) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_pk, s_need;
    if (st->flag) return;
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const fsp_u32x4* keys4 = reinterpret_cast<const fsp_u32x4*>(dist + qi * ld);
    const int64_t n4 = (n + 3) >> 2;
    if (tid == 0) { s_pk = 0u; s_need = static_cast<unsigned>(min(static_cast<int64_t>(k), n)); }
    __syncthreads();
    for (int p = 0; p < 4; p++) {
        for (int i = tid; i < 256; i += kGtmSelThreads) hist[i] = 0u;
        __syncthreads();
        const unsigned pk = s_pk;
        const int sh = 24 - 8 * p;
        for (int64_t i4 = tid; i4 < n4; i4 += kGtmSelThreads) {      // (lanes past the end have left: the ballots count the rest)
            const fsp_u32x4 v = keys4[i4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned key = v[j];
                const bool match = (p == 0) || ((key >> (sh + 8)) == (pk >> (sh + 8)));
                gt8_hist_add(hist, (key >> sh) & 255u, match && 4 * i4 + j < n);
            }
        }
        __syncthreads();
        if (tid == 0) {       // the digit bucket holding the need-th smallest of the matching keys
            unsigned cum = 0, dsel = 255;
            const unsigned need = s_need;
            for (unsigned b = 0; b < 256; b++) {
                if (cum + hist[b] >= need) { dsel = b; break; }
                cum += hist[b];
            }
            s_need = need - cum;
            s_pk = pk | (dsel << sh);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double ak = static_cast<double>(__uint_as_float(s_pk));
        const double eps = eps_of(qi);
        const double t64 = ak + 2.0 * eps;
        float t = static_cast<float>(t64);
        if (static_cast<double>(t) < t64) t = __uint_as_float(__float_as_uint(t) + 1u);      // (t >= 0 and far below FLT_MAX: the next float up)
        thr[qi] = __float_as_uint(t);
    }
}
__global__ __launch_bounds__(kGtmSelThreads) void gtm_kth_kernel(const unsigned* __restrict__ dist, int64_t ld, int64_t n, int k, int d,
                                                                 const float* __restrict__ qn, const GtmState* __restrict__ st, unsigned* __restrict__ thr) {
    gtm_kth_body(dist, ld, n, k, st, thr, [&](int64_t qi) {
        const double nq1 = sqrt(static_cast<double>(qn[qi]) * (1.0 + 0x1p-23));
        const double X = sqrt(__longlong_as_double(static_cast<long long>(st->xmax_bits)));
        return 1.01 * (2.0 * static_cast<double>(d + 4) * 0x1p-24 * nq1 * X + 0x1p-21 * (nq1 + X) * (nq1 + X)) + static_cast<double>(d) * 0x1p-120;
    });
}

// The ids of a query's survivors, key <= thr, appended to its list [kGtmCap] in any order: a wave's hits take their places with one
// add to the LDS counter.  counts[q] = how many there were, also when that is more than the list holds (the call reads it).
__global__ __launch_bounds__(kGtmColThreads) void gtm_collect_kernel(const unsigned* __restrict__ dist, int64_t ld, int64_t n, const unsigned* __restrict__ thr,
                                                                     const GtmState* __restrict__ st, int32_t* __restrict__ lists, int32_t* __restrict__ counts) {
    __shared__ unsigned s_cnt;
    if (st->flag) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t qi = blockIdx.x;
    const fsp_u32x4* keys4 = reinterpret_cast<const fsp_u32x4*>(dist + qi * ld);
    const int64_t n4 = (n + 3) >> 2;
    int32_t* list = lists + qi * kGtmCap;
    const unsigned t = thr[qi];
    if (tid == 0) s_cnt = 0u;
    __syncthreads();
    for (int64_t i4 = tid; i4 < n4; i4 += kGtmColThreads) {
        const fsp_u32x4 v = keys4[i4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t i = 4 * i4 + j;
            const bool hit = i < n && v[j] <= t;
            const unsigned long long m = __ballot(hit);
            if (m == 0ull) continue;
            const int lead = __ffsll(static_cast<long long>(m)) - 1;
            unsigned at = 0u;
            if (lane == lead) at = atomicAdd(&s_cnt, static_cast<unsigned>(__popcll(m)));
            at = static_cast<unsigned>(__shfl(static_cast<int>(at), lead)) + static_cast<unsigned>(__popcll(m & ((1ull << lane) - 1ull)));
            if (hit && at < static_cast<unsigned>(kGtmCap)) list[at] = static_cast<int32_t>(i);
        }
    }
    __syncthreads();
    if (tid == 0) counts[qi] = static_cast<int32_t>(s_cnt);
}

// One workgroup per query: a lane per survivor runs the reference's chain (the statements of gt_dist_kernel: float subtraction,
// widened, sum = sum + df * df in dimension order), then the composites (distance bits, id) are ranked in LDS by counting — a
// composite is unique, so the count of smaller ones IS its place; no padding to a power of two, every comparison reads a broadcast
// LDS word, and the survivors of ordinary data number little more than k — and the first min(k, n) are written with the padding
// behind them.  A query whose list overflowed is left to the call.
template <typename TB, bool kVec>
__global__ __launch_bounds__(kGtmFinThreads) void gtm_finish_kernel(const TB* __restrict__ base, int64_t n, const float* __restrict__ q, int d, int k,
                                                                    const int32_t* __restrict__ lists, const int32_t* __restrict__ counts,
                                                                    const GtmState* __restrict__ st, int32_t* __restrict__ out_ids, double* __restrict__ out_d2) {
    constexpr int N = RowCodec<TB>::N;
    __shared__ unsigned long long s_key[kGtmCap];
    __shared__ unsigned s_id[kGtmCap];
    if (st->flag) return;
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const int cnt = counts[qi];
    if (cnt > kGtmCap) return;
    const float* qr = q + qi * d;
    const int32_t* list = lists + qi * kGtmCap;
    for (int s = tid; s < cnt; s += kGtmFinThreads) {
        const int32_t id = list[s];
        const TB* row = base + static_cast<int64_t>(id) * d;
        double sum = 0.0;
        for (int k0 = 0; k0 < d; k0 += N) {
            GtmFrag<TB, kVec> f;
            f.load(row, k0, d);
#pragma unroll
            for (int e = 0; e < N; e++) {
                if (kVec || k0 + e < d) {
                    const float df = qr[kVec ? k0 + e : min(k0 + e, d - 1)] - f.get(e);       // float - float (GroundtruthPrecompute.java:150)
                    const double dd = static_cast<double>(df);
                    const double sq = dd * dd;
                    sum = sum + sq;
                }
            }
        }
        s_key[s] = static_cast<unsigned long long>(__double_as_longlong(sum));
        s_id[s] = static_cast<unsigned>(id);
    }
    __syncthreads();
    const int kk = static_cast<int>(min(static_cast<int64_t>(min(k, cnt)), n));
    for (int e = tid; e < cnt; e += kGtmFinThreads) {
        const unsigned long long mk = s_key[e];
        const unsigned mi = s_id[e];
        int rank = 0;
        for (int j = 0; j < cnt; j++) rank += (s_key[j] < mk) || (s_key[j] == mk && s_id[j] < mi);
        if (rank < kk) {
            out_ids[qi * k + rank] = static_cast<int32_t>(mi);
            if (out_d2) out_d2[qi * k + rank] = __longlong_as_double(static_cast<long long>(mk));
        }
    }
    for (int e = kk + tid; e < k; e += kGtmFinThreads) {
        out_ids[qi * k + e] = -1;
        if (out_d2) out_d2[qi * k + e] = __longlong_as_double(0x7FF0000000000000LL);
    }
}

// The overflowed queries of a call, gathered for gt_rows_run and their results put back: out[j] = q[idx[j]] and back.
__global__ __launch_bounds__(256) void gtm_gather_kernel(const float* __restrict__ q, const int32_t* __restrict__ idx, int d, float* __restrict__ out) {
    const float* src = q + static_cast<int64_t>(idx[blockIdx.x]) * d;
    for (int i = threadIdx.x; i < d; i += 256) out[static_cast<int64_t>(blockIdx.x) * d + i] = src[i];
}
__global__ __launch_bounds__(256) void gtm_scatter_kernel(const int32_t* __restrict__ idx, int k, const int32_t* __restrict__ ids, const double* __restrict__ d2,
                                                          int32_t* __restrict__ out_ids, double* __restrict__ out_d2) {
    const int64_t to = static_cast<int64_t>(idx[blockIdx.x]) * k, from = static_cast<int64_t>(blockIdx.x) * k;
    for (int i = threadIdx.x; i < k; i += 256) {
        out_ids[to + i] = ids[from + i];
        if (out_d2) out_d2[to + i] = d2[from + i];
    }
}

}  // namespace fspann
