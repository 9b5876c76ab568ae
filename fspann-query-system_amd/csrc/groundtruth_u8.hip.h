// groundtruth_u8.hip.h — exact ground truth over BYTE vectors (FSPANN_U8 base and queries: .bvecs data) on the int8 matrix cores.
//
// The reference (GroundtruthPrecompute.java:142-163 with BvecsLoader's `buf[i] & 0xFF`) sums `d*d` in fp64 in dimension order.
// Over bytes every term and every partial sum is an integer below 2^53, so that sum is exact in ANY order and equals the
// integer
//     sum (q_i - x_i)^2  =  sum q'_i^2 + sum x'_i^2 - 2 sum q'_i x'_i        q' = q - 128, x' = x - 128 (signed bytes)
// which for dim <= 32768 fits 32 bits (32768 * 255^2 < 2^31).  The cross term is a matrix product, [queries] x [base rows]^T,
// and runs on v_mfma_i32_32x32x32_i8; the two norms come from a small kernel of their own (v_dot4_i32_i8).  The [Q x N]
// distances go to a scratch matrix of uint32 (half the bytes of the fp32 path's fp64 matrix) and the same exact selection as
// gt_select_kernel runs over them: an MSB radix select of the k-th smallest composite key (distance, id).
// Signed bytes (FSPANN_I8 base and queries) are the int8_t instantiations of the same kernels: the same product without the flip.
#pragma once
#include "fspann_common.h"

namespace fspann {

typedef int gt8_i32x4 __attribute__((ext_vector_type(4)));
typedef int gt8_i32x16 __attribute__((ext_vector_type(16)));

constexpr int kGt8Rows = 128;        // base rows per workgroup: 4 waves x 32 (one MFMA tile column each)
constexpr int kGt8Q = 128;           // queries per workgroup: 4 tiles of 32, walked in turn against the wave's 32 rows
constexpr int kGt8MaxDim = 32768;    // 32768 * 255^2 < 2^31
constexpr int kGt8SelThreads = 1024;

// Bytes [k0, k0 + 16) of one row as four words of SIGNED bytes, which is what the matrix cores take.  TB = uint8_t: every byte
// flipped (x ^ 0x80 = x - 128); bytes at k >= d are signed zeros, put there AFTER the flip (a raw 0 would count as -128).
// TB = int8_t: the bytes as they are, and a raw 0 is the right pad.  kAligned: d % 16 == 0 and a 16-byte aligned matrix, one
// 16-byte load.
//
// The distances are formed in uint32 arithmetic from the norms and the product of these signed bytes (q', x' below: q - 128 and
// x - 128 for uint8_t, q and x themselves for int8_t).  Why that lands on the exact distance: |q'|^2 and |x'|^2 are at most
// 16384 d <= 2^29 each, q'.x' lies in [-16256 d, 16384 d], so 2 q'.x' as an unsigned wraps when the product is negative, and
// |q'|^2 + |x'|^2 - 2 q'.x' may pass through values >= 2^32 or "below 0" on the way.  Addition, subtraction and the
// multiplication by 2 are those of the ring Z / 2^32, where the result depends on the operands' residues only; the true value
// sum (q_i - x_i)^2 lies in [0, d * 255^2] with d * 255^2 < 2^31 for d <= 32768, and a residue in that range is the integer
// itself.  (The accumulator of the MFMA is the exact q'.x': |q'.x'| <= 2^29.)  gt8_select_kernel serves both types: a distance
// is an integer in 0 .. d * 255^2 either way.
template <typename TB, bool kAligned>
__device__ __forceinline__ gt8_i32x4 gt8_frag(const TB* __restrict__ row, int k0, int d) {
    constexpr unsigned kFlip = RowCodec<TB>::kToSigned;      // per byte; only the byte types (uint8_t, int8_t) have it
    fsp_u32x4 w = {0u, 0u, 0u, 0u};
    if constexpr (kAligned) {       // (d >= 16 here; the load is made at a clamped address so that the K loop holds no branch)
        w = *reinterpret_cast<const fsp_u32x4*>(row + min(k0, d - 16));
        w ^= kFlip * 0x01010101u;
        if (k0 >= d) w = fsp_u32x4{0u, 0u, 0u, 0u};
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const int k = k0 + j;
            const unsigned b = (k < d) ? ((static_cast<unsigned>(row[k]) & 0xFFu) ^ kFlip) : 0u;
            w[j >> 2] |= b << (8 * (j & 3));
        }
    }
    return __builtin_bit_cast(gt8_i32x4, w);
}

// out[r] = |x'|^2 = sum_i (rows[r][i] - 128)^2 (uint8_t) or sum_i rows[r][i]^2 (int8_t), at most 16384 d; one lane per row.
template <typename TB, bool kAligned>
__global__ __launch_bounds__(256) void gt8_norm_kernel(const TB* __restrict__ rows, int64_t n, int d, unsigned* __restrict__ out) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r >= n) return;
    const TB* row = rows + r * d;
    int s = 0;
    for (int k0 = 0; k0 < d; k0 += 16) {
        const gt8_i32x4 v = gt8_frag<TB, kAligned>(row, k0, d);
#pragma unroll
        for (int j = 0; j < 4; j++) s = __builtin_amdgcn_sdot4(v[j], v[j], s, false);
    }
    out[r] = static_cast<unsigned>(s);
}

// dist[q][r] = |q'|^2 + |x'|^2 - 2 q'.x' for the kGt8Q queries x kGt8Rows base rows of this workgroup (workgroup id = base tile *
// nqb + query block: neighbours in the grid share the base tile, so it comes from cache after its first read).
// v_mfma_i32_32x32x32_i8: lane l holds bytes 16 (l >> 5) .. +15 of the K step of ONE row for both operands (A: query l & 31,
// B: base row l & 31), i.e. 16-byte pieces of row-major data, nothing transposed; the result has the base row on the lane
// (l & 31) and the query on the register: query (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  So one register's 32 lanes store 32
// consecutive base rows of one query.  No barrier: a wave whose 32 rows lie beyond n leaves at once.
template <typename TB, bool kAligned>
__global__ __launch_bounds__(256) void gt8_dist_kernel(const TB* __restrict__ base, int64_t n, const TB* __restrict__ q, int64_t nq, int d,
                                                       const unsigned* __restrict__ xn, const unsigned* __restrict__ qn,
                                                       unsigned* __restrict__ dist, int64_t ld, int nqb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t bt = blockIdx.x / static_cast<unsigned>(nqb);
    const int64_t qb = blockIdx.x % static_cast<unsigned>(nqb);
    const int64_t r0 = bt * kGt8Rows + wave * 32;
    if (r0 >= n) return;
    const int64_t r = r0 + (lane & 31);
    const TB* brow = base + min(r, n - 1) * d;           // rows >= n of an edge tile: computed on a copy, never stored
    const int kh = 16 * (lane >> 5);
    const unsigned nx = xn[min(r, n - 1)];
    for (int g = 0; g < kGt8Q / 32; g++) {
        const int64_t q0 = qb * kGt8Q + g * 32;
        if (q0 >= nq) break;
        const TB* qrow = q + min(q0 + (lane & 31), nq - 1) * d;
        // |q'|^2 of this lane's 16 queries, four 16-byte loads (qn holds whole tiles of 32: entries >= nq are never used for a store)
        const fsp_u32x4* qn4 = reinterpret_cast<const fsp_u32x4*>(qn + q0 + 4 * (lane >> 5));
        fsp_u32x4 nqv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) nqv[j] = qn4[2 * j];
        gt8_i32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k0 = 0; k0 < d; k0 += 64) {      // two K steps per turn, their four loads in flight together (a step past d is zeros)
            const gt8_i32x4 a0 = gt8_frag<TB, kAligned>(qrow, k0 + kh, d);
            const gt8_i32x4 b0 = gt8_frag<TB, kAligned>(brow, k0 + kh, d);
            const gt8_i32x4 a1 = gt8_frag<TB, kAligned>(qrow, k0 + 32 + kh, d);
            const gt8_i32x4 b1 = gt8_frag<TB, kAligned>(brow, k0 + 32 + kh, d);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc, 0, 0, 0);
        }
        if (r < n) {
            const int64_t qa = q0 + 4 * (lane >> 5);
            unsigned* o = dist + qa * ld + r;
            if (q0 + 32 <= nq) {
#pragma unroll
                for (int reg = 0; reg < 16; reg++)
                    o[((reg & 3) + 8 * (reg >> 2)) * ld] = nqv[reg >> 2][reg & 3] + nx - 2u * static_cast<unsigned>(acc[reg]);
            } else {
#pragma unroll
                for (int reg = 0; reg < 16; reg++) {
                    const int qo = (reg & 3) + 8 * (reg >> 2);
                    if (qa + qo < nq) o[qo * ld] = nqv[reg >> 2][reg & 3] + nx - 2u * static_cast<unsigned>(acc[reg]);
                }
            }
        }
    }
}

// One matching key into the digit histogram.  Top digits are often the same for every lane of a wave (a distance of 23
// significant bits has few distinct top bytes); then one lane adds the wave's count instead of 64 adds to one LDS address.
__device__ __forceinline__ void gt8_hist_add(unsigned* hist, unsigned digit, bool match) {
    const unsigned long long m = __ballot(match);
    if (m == 0ull) return;
    const int lead = __ffsll(static_cast<long long>(m)) - 1;
    const unsigned d0 = static_cast<unsigned>(__shfl(static_cast<int>(digit), lead));
    if (__ballot(match && digit != d0) == 0ull) {
        if ((threadIdx.x & 63) == lead) atomicAdd(&hist[d0], static_cast<unsigned>(__popcll(m)));
    } else if (match) {
        atomicAdd(&hist[digit], 1u);
    }
}

// gt_select_kernel over uint32 keys: one workgroup per query, ids of the k smallest (distance, id), ascending.  The query's
// row of `dist` starts 16-byte aligned (ld % 4 == 0) and is read four keys per load.  ndd distance digits (the host knows how
// many bytes dim * 255^2 needs) and ndi id digits (bytes of n - 1), most significant first; the id digits matter only among
// keys equal to the k-th distance, and are skipped when all of those belong to the result.
__global__ __launch_bounds__(kGt8SelThreads) void gt8_select_kernel(const unsigned* __restrict__ dist, int64_t ld, int64_t n, int k, int ndd, int ndi,
                                                                    int32_t* __restrict__ out_ids, double* __restrict__ out_d2) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_pk, s_pi, s_need, s_cnt, s_done;
    __shared__ unsigned sel_key[kGtMaxK];
    __shared__ unsigned sel_id[kGtMaxK];
    const int tid = threadIdx.x;
    const int64_t qi = blockIdx.x;
    const fsp_u32x4* keys4 = reinterpret_cast<const fsp_u32x4*>(dist + qi * ld);
    const int64_t n4 = (n + 3) >> 2;
    const int kk = static_cast<int>(min(static_cast<int64_t>(k), n));
    if (tid == 0) { s_pk = 0u; s_pi = 0u; s_need = static_cast<unsigned>(kk); s_cnt = 0u; s_done = 0u; }
    __syncthreads();
    for (int p = 0; p < ndd + ndi; p++) {
        if (p >= ndd && s_done) break;
        for (int i = tid; i < 256; i += kGt8SelThreads) hist[i] = 0u;
        __syncthreads();
        const unsigned pk = s_pk, pi = s_pi;
        const bool on_dist = p < ndd;
        const int sh = on_dist ? 8 * (ndd - 1 - p) : 8 * (ndd + ndi - 1 - p);
        const bool first = (p == 0) || (p == ndd);                 // no digit of this part chosen yet
        const int hs = first ? 0 : sh + 8;                         // (first: the prefix test is not made; keeps the shift below 32)
        for (int64_t i4 = tid; i4 < n4; i4 += kGt8SelThreads) {    // (lanes past the end have left: the ballots count the rest)
            const fsp_u32x4 v = keys4[i4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int64_t i = 4 * i4 + j;
                const unsigned key = v[j];
                const unsigned id = static_cast<unsigned>(i);
                bool match;
                unsigned digit;
                if (on_dist) {
                    match = first || ((key >> hs) == (pk >> hs));
                    digit = (key >> sh) & 255u;
                } else {
                    match = (key == pk) && (first || ((id >> hs) == (pi >> hs)));
                    digit = (id >> sh) & 255u;
                }
                gt8_hist_add(hist, digit, match && i < n);
            }
        }
        __syncthreads();
        if (tid == 0) {       // the digit bucket holding the need-th smallest of the matching elements
            unsigned cum = 0, dsel = 255;
            const unsigned need = s_need;
            for (unsigned b = 0; b < 256; b++) {
                if (cum + hist[b] >= need) { dsel = b; break; }
                cum += hist[b];
            }
            s_need = need - cum;
            if (on_dist) {
                s_pk = pk | (dsel << sh);
                // last distance digit: hist[dsel] keys equal the k-th distance; if the result takes them all, ids do not decide
                if (p == ndd - 1 && hist[dsel] == need - cum) { s_pi = 0xFFFFFFFFu; s_done = 1u; }
            } else {
                s_pi = pi | (dsel << sh);
            }
        }
        __syncthreads();
    }
    // (s_pk, s_pi) is the kk-th smallest composite: collect everything at or below it (exactly kk elements), then order them
    const unsigned tk = s_pk, ti = s_pi;
    for (int64_t i4 = tid; i4 < n4; i4 += kGt8SelThreads) {
        const fsp_u32x4 v = keys4[i4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int64_t i = 4 * i4 + j;
            const unsigned key = v[j];
            if (i < n && (key < tk || (key == tk && static_cast<unsigned>(i) <= ti))) {
                const unsigned at = atomicAdd(&s_cnt, 1u);
                if (at < static_cast<unsigned>(kGtMaxK)) { sel_key[at] = key; sel_id[at] = static_cast<unsigned>(i); }
            }
        }
    }
    __syncthreads();
    const int cnt = static_cast<int>(min(s_cnt, static_cast<unsigned>(kk)));
    for (int e = tid; e < cnt; e += kGt8SelThreads) {
        const unsigned mk = sel_key[e], mi = sel_id[e];
        int rank = 0;
        for (int j = 0; j < cnt; j++) rank += (sel_key[j] < mk) || (sel_key[j] == mk && sel_id[j] < mi);
        out_ids[qi * k + rank] = static_cast<int32_t>(mi);
        if (out_d2) out_d2[qi * k + rank] = __uint2double_rn(mk);
    }
    for (int e = cnt + tid; e < k; e += kGt8SelThreads) {
        out_ids[qi * k + e] = -1;
        if (out_d2) out_d2[qi * k + e] = __longlong_as_double(0x7FF0000000000000LL);
    }
}

}  // namespace fspann
