// groundtruth_mfma16.hip.h — the pre-filter of groundtruth_mfma.hip.h on the 16-bit matrix cores, for the rows whose every element
// is a half (FSPANN_F16, FSPANN_U8, FSPANN_I8, FSPANN_F8E4M3: v_mfma_f32_32x32x16_f16) or a bfloat16 (FSPANN_BF16:
// v_mfma_f32_32x32x16_bf16) (fspann_groundtruth_mfma16_dev / _store_dev, include/fspann_groundtruth_mfma16.h; DESIGN.md 3.6g has
// the proof, the layout and the measurements).
//
// A 16-byte piece of such a row IS one operand of those instructions (a piece of a one-byte type: two, after an exact conversion in
// registers); only the fp32 query is not narrow, and it is split once per chunk into T terms of the rows' format,
//     q = 2^e (h_1 + h_2 [+ h_3]) + residual,       T = 2 halves (|residual| <= 2^-22 |q_i| + 2^(e-24)) or 3 bfloat16s (2^-24 |q_i|, e = 0)
// by gtm16_split_kernel.  gtm16_dist_kernel multiplies every term into the same fp32 accumulator — the products of two halves or
// two bfloat16s are exact in fp32 — and leaves the estimate a = max(0, |q|^2 + |x|^2 - 2 2^e acc) where gtm_dist_kernel leaves its
// own.  gtm16_kth_kernel is gtm_kth_kernel with the error interval of THIS estimate.  The base norms, the collection, the exact
// finish and the two ways out are those of groundtruth_mfma.hip.h, unchanged.
#pragma once
#include "groundtruth_mfma.hip.h"

#pragma clang fp contract(off)

namespace fspann {

typedef __bf16 gtm16_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kGtm16Rows = 256;         // base rows per workgroup of gtm16_dist_kernel: 4 waves x 2 tiles of 32
constexpr int kGtm16KPad = 32;          // the term planes' row length is d rounded up to this: the longest K step (one-byte rows)
constexpr int kGtm16ScaleMin = -100;    // e is kept above this, so that 2^(e+1) is a normal float (a query that small sits lower in the half range)

// What the matrix instruction of a row type takes.  T: the terms of a query.  bits(x): one row element as the 16 bits of its operand
// element (the element-load path); piece(p, u): operand u of a 16-byte piece.
template <typename TB> struct Gtm16Op {        // the halves
    static constexpr int T = 2;
    static __device__ __forceinline__ uint16_t bits(TB x) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(static_cast<float>(x))); }
    static __device__ __forceinline__ fsp_u32x4 piece(fsp_u32x4 p, int u) { return __builtin_bit_cast(fsp_u32x4, RowCodec<TB>::piece_f16x8(p, u)); }
    static __device__ __forceinline__ gtm_f32x16 mfma(fsp_u32x4 a, fsp_u32x4 b, gtm_f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(fsp_f16x8, a), __builtin_bit_cast(fsp_f16x8, b), c, 0, 0, 0);
    }
};
template <> struct Gtm16Op<fsp_bf16> {
    static constexpr int T = 3;
    static __device__ __forceinline__ uint16_t bits(fsp_bf16 x) { return x.b; }
    static __device__ __forceinline__ fsp_u32x4 piece(fsp_u32x4 p, int) { return p; }
    static __device__ __forceinline__ gtm_f32x16 mfma(fsp_u32x4 a, fsp_u32x4 b, gtm_f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(gtm16_bf16x8, a), __builtin_bit_cast(gtm16_bf16x8, b), c, 0, 0, 0);
    }
};

// The operands of the row elements [k0, k0 + N) of one row, N = 16 / sizeof(TB), U = N / 8 of them; elements at k >= d are zeros.
// kVec: the 16-byte piece as it was loaded from a clamped address, converted on use; otherwise N element loads of any alignment,
// packed at once.
template <typename TB, bool kVec> struct Gtm16Frag;
template <typename TB> struct Gtm16Frag<TB, true> {
    static constexpr int N = RowCodec<TB>::N;
    fsp_u32x4 p;
    bool live;
    __device__ __forceinline__ void load(const TB* __restrict__ row, int k0, int d) {
        p = *reinterpret_cast<const fsp_u32x4*>(row + min(k0, d - N));      // (d >= N: d is a multiple of N)
        live = k0 < d;
    }
    __device__ __forceinline__ fsp_u32x4 op(int u) const {
        const fsp_u32x4 o = Gtm16Op<TB>::piece(p, u);
        return live ? o : fsp_u32x4{0u, 0u, 0u, 0u};
    }
};
template <typename TB> struct Gtm16Frag<TB, false> {
    static constexpr int N = RowCodec<TB>::N, U = N / 8;
    fsp_u32x4 v[U];
    __device__ __forceinline__ void load(const TB* __restrict__ row, int k0, int d) {
#pragma unroll
        for (int e = 0; e < N; e += 2) {
            const uint32_t lo = Gtm16Op<TB>::bits(row[min(k0 + e, d - 1)]), hi = Gtm16Op<TB>::bits(row[min(k0 + e + 1, d - 1)]);
            v[e >> 3][(e & 7) >> 1] = (k0 + e < d ? lo : 0u) | (k0 + e + 1 < d ? hi << 16 : 0u);
        }
    }
    __device__ __forceinline__ fsp_u32x4 op(int u) const { return v[u]; }
};

// One wave per query of a chunk (four to a workgroup).  Leaves |q|^2 (the fp64 sum rounded once to fp32, and the flag of
// gtm_norm_kernel<float> for a non-finite or over-limit query), the factor 2^(e+1) of the epilogue, and the term planes
// planes[t][query][kpad] (16-bit, zeros at k >= d):
//     q' = q 2^-e;  h_1 = round16(q'), h_2 = round16(q' - h_1), h_3 = round16(q' - h_1 - h_2), differences in fp32 (exact)
// kBf16 = false: two halves, e = floor(log2 max|q_i|) - 14, so the largest |q'_i| lies in [2^14, 2^15) (e = 0 for an all-zero
// query); true: three bfloat16s (round to nearest even on the bits), e = 0.
template <bool kBf16>
__global__ __launch_bounds__(256) void gtm16_split_kernel(const float* __restrict__ q, int64_t nq, int d, int kpad, float* __restrict__ qn, float* __restrict__ qsc,
                                                          uint16_t* __restrict__ planes, int64_t plane_stride, GtmState* __restrict__ st) {
    const int lane = threadIdx.x & 63;
    const int64_t qi = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (qi >= nq) return;                                 // (a whole wave)
    const float* row = q + qi * d;
    double s = 0.0;
    float m = 0.0f;
    for (int i = lane; i < d; i += 64) {
        const float v = row[i];
        const double w = static_cast<double>(v);
        const double sq = w * w;
        s = s + sq;
        m = fmaxf(m, fabsf(v));
    }
    for (int off = 32; off > 0; off >>= 1) {
        s = s + __shfl_xor(s, off);
        m = fmaxf(m, __shfl_xor(m, off));
    }
    const bool bad = !(s <= kGtmNormLimit);
    int e = 0;
    if (!kBf16 && !bad && m > 0.0f) {
        int ex;
        frexpf(m, &ex);                                    // m = f 2^ex, f in [0.5, 1): also for a subnormal m
        e = max(ex - 15, kGtm16ScaleMin);
    }
    if (lane == 0) {
        qn[qi] = static_cast<float>(s);
        qsc[qi] = ldexpf(2.0f, e);
        if (bad) atomicOr(&st->flag, 1);
    }
    uint16_t* out = planes + qi * kpad;
    for (int i = lane; i < kpad; i += 64) {
        float r = i < d ? ldexpf(row[min(i, d - 1)], -e) : 0.0f;
#pragma unroll
        for (int t = 0; t < (kBf16 ? 3 : 2); t++) {
            uint16_t hb;
            float h;
            if (kBf16) {
                const uint32_t b = __float_as_uint(r);
                hb = static_cast<uint16_t>((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
                h = __uint_as_float(static_cast<uint32_t>(hb) << 16);
            } else {
                const _Float16 hh = static_cast<_Float16>(r);
                hb = __builtin_bit_cast(uint16_t, hh);
                h = static_cast<float>(hh);
            }
            out[t * plane_stride + i] = hb;
            r = r - h;
        }
    }
}

// dist[q][r] = bits of a = max(0, |q|^2 + |x_r|^2 - 2^(e_q + 1) acc) for the kGtmQ queries x kGtm16Rows base rows of this workgroup
// (workgroup id = base tile * nqb + query block, as in gtm_dist_kernel).
//
// v_mfma_f32_32x32x16_{f16,bf16}: lane l gives the 8 consecutive K values 8 (l >> 5) .. + 7 of A row l & 31 and of B column l & 31;
// with A = queries and B = base rows the result lies as in gtm_dist_kernel: the base row on the lane, the query on the register
// ((reg & 3) + 8 (reg >> 2) + 4 (l >> 5)).  A wave owns 64 base rows — two tiles of 32 — and eight accumulators, one per row tile
// and 32-query tile, so every query operand it reads from LDS feeds two MFMAs: with one row tile per wave the four waves' operand
// reads (4 tiles x T terms x 1 KB per 8 K values) and not the matrix pipe would set the pace.
// A K step is 2 N elements (N = elements per 16 bytes of TB): lane half h = l >> 5 reads the 16 bytes [k0 + h N, + N) of ITS OWN
// two rows.  For the two-byte types that piece is the operand; for the one-byte types it gives U = 2 operands, elements [0, 8) and
// [8, 16) of the piece, after an exact conversion (RowCodec::piece_f16x8).  Operand u of the step so holds K = k0 + h N + 8 u .. + 7,
// and the queries follow the same permutation: nothing is transposed.
// The query block's terms of a step, T U 2 planes of kGtmQ 16-byte operands, go through LDS once for the four waves: thread t loads
// the operands of query t & 127 for lane half t >> 7 with 16-byte loads from the term planes (always aligned and zero-padded: the
// planes are the call's own) and writes them operand-major, Qs[buf][(t U + u) 2 + h][query] — a wave writes 64 consecutive 16-byte
// words and a lane half reads 32 consecutive ones with one ds_read_b128, so neither has a bank conflict.  Two buffers: the loads of
// step s + 1, base pieces and query operands, are issued before the MFMAs of step s and written to the other buffer behind them;
// one lds_barrier per step.  Every load is unconditional (clamped address; zeros at k >= d on both sides); rows >= n and queries
// >= nq are computed on a clamped index and never stored.  No fp64, no conversion of the query side in the loop.
template <typename TB, bool kVec>
__global__ __launch_bounds__(256, 2) void gtm16_dist_kernel(const TB* __restrict__ base, int64_t n, const uint16_t* __restrict__ planes, int64_t plane_stride, int kpad,
                                                         int64_t nq, int d, const float* __restrict__ xn, const float* __restrict__ qn, const float* __restrict__ qsc,
                                                         const GtmState* __restrict__ st, unsigned* __restrict__ dist, int64_t ld, int nqb) {
    constexpr int N = RowCodec<TB>::N, kStep = 2 * N, U = N / 8, T = Gtm16Op<TB>::T;
    __shared__ fsp_u32x4 Qs[2][T * U * 2][kGtmQ];
    if (st->flag) return;                                 // (uniform; the call goes to gt_rows_run)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, h = lane >> 5;
    const int64_t bt = blockIdx.x / static_cast<unsigned>(nqb);
    const int64_t qb = blockIdx.x % static_cast<unsigned>(nqb);
    const int64_t r0 = bt * kGtm16Rows + wave * 64 + col;
    const TB* brow[2] = {base + min(r0, n - 1) * d, base + min(r0 + 32, n - 1) * d};
    const int sq = tid & (kGtmQ - 1), sh = tid >> 7;      // this thread's query and lane half of the operands it stages
    const uint16_t* qrow = planes + min(qb * kGtmQ + sq, nq - 1) * kpad;
    gtm_f32x16 acc[2][4];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[s][g][i] = 0.0f;

    Gtm16Frag<TB, kVec> bcur[2], bnxt[2];
    fsp_u32x4 qf[T * U];
    auto q_load = [&](int k0) {
#pragma unroll
        for (int t = 0; t < T; t++)
#pragma unroll
            for (int u = 0; u < U; u++) qf[t * U + u] = *reinterpret_cast<const fsp_u32x4*>(qrow + t * plane_stride + min(k0 + sh * N + 8 * u, kpad - 8));
    };
    auto q_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < T * U; i++) Qs[buf][2 * i + sh][sq] = qf[i];
    };
    bcur[0].load(brow[0], h * N, d);
    bcur[1].load(brow[1], h * N, d);
    q_load(0);
    q_store(0);
    lds_barrier();
    int buf = 0;
    for (int k0 = 0; k0 < d; k0 += kStep) {
        bnxt[0].load(brow[0], k0 + kStep + h * N, d);     // the next step's loads, in flight behind this step's MFMAs
        bnxt[1].load(brow[1], k0 + kStep + h * N, d);
        q_load(k0 + kStep);
#pragma unroll
        for (int u = 0; u < U; u++) {
            const fsp_u32x4 b0 = bcur[0].op(u), b1 = bcur[1].op(u);
#pragma unroll
            for (int t = 0; t < T; t++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const fsp_u32x4 a = Qs[buf][(t * U + u) * 2 + h][32 * g + col];
                    acc[0][g] = Gtm16Op<TB>::mfma(a, b0, acc[0][g]);
                    acc[1][g] = Gtm16Op<TB>::mfma(a, b1, acc[1][g]);
                }
        }
        q_store(buf ^ 1);
        lds_barrier();
        bcur[0] = bnxt[0];
        bcur[1] = bnxt[1];
        buf ^= 1;
    }
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int64_t r = r0 + 32 * s;
        if (r >= n) continue;
        const float nx = xn[r];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int64_t qa = qb * kGtmQ + 32 * g + 4 * h;
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int64_t qi = qa + (reg & 3) + 8 * (reg >> 2);
                if (qi < nq) {
                    const float sum = qn[qi] + nx;
                    const float t = sum - qsc[qi] * acc[s][g][reg];                 // (the product with 2^(e+1) is exact)
                    dist[qi * ld + r] = __float_as_uint(t > 0.0f ? t : 0.0f);       // (+0 for -0, and bits of non-negative floats are monotone)
                }
            }
        }
    }
}

// gtm_kth_kernel for the estimates of gtm16_dist_kernel: the same select, and thr = a_k + 2 eps_q rounded up with
//     eps_q = 1.01 [ 2 (1.005 g_m + c_T) |q| X + 2 s_q sqrt(d) X + 2^-21 (|q| + X)^2 ] + d 2^-120
//     m = T d + 1, g_m = m 2^-23 / (1 - m 2^-23)       the accumulation of the T d exact products, ONE UNIT OF 2^-23 PER ADDITION
//     c_2 = 2^-22, c_3 = 2^-24                          what the terms leave of q
//     s_q = 2^(e-24) for halves, 0 for bfloat16s        a term rounded in the halves' subnormal range
__global__ __launch_bounds__(kGtmSelThreads) void gtm16_kth_kernel(const unsigned* __restrict__ dist, int64_t ld, int64_t n, int k, int d, int terms,
                                                                   const float* __restrict__ qn, const float* __restrict__ qsc, const GtmState* __restrict__ st,
                                                                   unsigned* __restrict__ thr) {
    gtm_kth_body(dist, ld, n, k, st, thr, [&](int64_t qi) {
        const double nq1 = sqrt(static_cast<double>(qn[qi]) * (1.0 + 0x1p-23));
        const double X = sqrt(__longlong_as_double(static_cast<long long>(st->xmax_bits)));
        const double mu = (static_cast<double>(terms) * d + 1.0) * 0x1p-23;
        const double gm = mu / (1.0 - mu);
        const double cT = terms == 2 ? 0x1p-22 : 0x1p-24;
        const double sub = terms == 2 ? static_cast<double>(qsc[qi]) * 0x1p-25 * sqrt(static_cast<double>(d)) * X : 0.0;
        return 1.01 * (2.0 * (1.005 * gm + cT) * nq1 * X + 2.0 * sub + 0x1p-21 * (nq1 + X) * (nq1 + X)) + static_cast<double>(d) * 0x1p-120;
    });
}

}  // namespace fspann
