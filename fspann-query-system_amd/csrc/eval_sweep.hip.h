// eval_sweep.hip.h — computeMetricsAtK (FSA:770-835) for EVERY k of kVariants from one result list, one launch
// (fspann_eval_kvariants_dev, include/fspann_eval.h): runQueries' metric loop (FSA:684-692).  Row j of the outputs is what
// gt_metrics_kernel (groundtruth.hip.h) writes for k = ks[j], bit for bit.
// Included from fspann_api.hip behind groundtruth.hip.h (kGtMaxK).
#pragma once

namespace fspann {

constexpr int kEvalThreads = 256;
constexpr int kEvalMaxK = 64;          // k values per call: one lane of the folding wave each
constexpr int kEvalQLdsMax = 4096;     // queries of more dimensions are read from global memory (element path only)

// the k values of a call, in the kernel arguments (nothing the caller must keep alive)
struct EvalKs {
    int32_t k[kEvalMaxK];
};

// LDS of one launch: the query as fp64 | dAnn [kmax] | dGt [kmax] | gt ids [kmax] | hit histogram [kmax]; every part 16-byte aligned
__host__ __device__ inline size_t eval_q_slots(int d) { return d <= kEvalQLdsMax ? static_cast<size_t>((d + 1) & ~1) : 0; }
__host__ __device__ inline size_t eval_k_slots(int kmax) { return static_cast<size_t>((kmax + 3) & ~3); }
inline size_t eval_lds_bytes(int d, int kmax) { return eval_q_slots(d) * 8 + eval_k_slots(kmax) * (8 + 8 + 4 + 4); }

// One workgroup per query.
//   1. the query goes to LDS as fp64, the first kmax gt ids too;
//   2. lane r owns ONE row: ann[i] (r = 2 i) or gt[i] (r = 2 i + 1) of a place i < min(kmax, na) whose two ids are rows of the base,
//      and sums BaseVectorReader.l2 over it in dimension order (the statements of gt_metrics_kernel; d is split over lanes
//      nowhere), 16 bytes at a time when kVec (every row starts on a 16-byte boundary and is whole pieces: the caller checks);
//      the lanes r = 2 i also find m(i) = max(i, first place of ann[i] in gt[0..kmax)) and count it in the histogram;
//   3. wave 0 folds the terms dAnn_i / dGt_i in index order (rounds of 64, sequential inside a round: the fold of the existing
//      kernel), lane j reading the running sum off behind term ks[j] - 1: the fold for k is a prefix of the fold for kmax.
//      hits(k) = #{i : m(i) < k}: the ann place counts for k iff it is among the first k and its id among the first k of gt.
template <typename TB, typename TQ, bool kVec>
__global__ __launch_bounds__(kEvalThreads) void eval_kvariants_kernel(const TB* __restrict__ base, int64_t n, const TQ* __restrict__ q, int d, int64_t nq,
                                                                      EvalKs ks, int nk, int kmax, const int32_t* __restrict__ ann, int64_t ann_stride,
                                                                      const int32_t* __restrict__ ann_count, const int32_t* __restrict__ gt, int64_t gt_stride,
                                                                      const int32_t* __restrict__ unique, double* __restrict__ recall,
                                                                      double* __restrict__ ratio, double* __restrict__ cand_ratio) {
    extern __shared__ __attribute__((aligned(16))) char eval_smem[];
    const size_t qs = eval_q_slots(d), kslots = eval_k_slots(kmax);
    double* s_q = reinterpret_cast<double*>(eval_smem);
    double* s_da = s_q + qs;
    double* s_dg = s_da + kslots;
    int32_t* s_gt = reinterpret_cast<int32_t*>(s_dg + kslots);
    int32_t* s_hist = s_gt + kslots;

    const int64_t qi = blockIdx.x;
    const int tid = threadIdx.x;
    const int na = ann_count ? max(0, min(ann_count[qi], static_cast<int>(ann_stride))) : static_cast<int>(ann_stride);
    const int lim = min(kmax, na);                         // places of ann that any k reads
    const int32_t* a = ann + qi * ann_stride;
    const int32_t* g = gt + qi * gt_stride;
    const TQ* qr = q + qi * d;
    const bool q_lds = qs != 0;
    if (q_lds)
        for (int t = tid; t < d; t += kEvalThreads) s_q[t] = static_cast<double>(qr[t]);
    for (int i = tid; i < kmax; i += kEvalThreads) { s_gt[i] = g[i]; s_hist[i] = 0; }
    __syncthreads();

    for (int r = tid; r < 2 * lim; r += kEvalThreads) {
        const int i = r >> 1;
        const int32_t ai = a[i], gi = s_gt[i];
        if ((r & 1) == 0) {
            // recall: the first place of ann[i] among gt[0..kmax) (plain equality, as the existing loop compares)
            int p = kmax;
            for (int j = kmax - 1; j >= 0; j--) p = (s_gt[j] == ai) ? j : p;
            const int m = max(i, p);
            if (m < kmax) atomicAdd(&s_hist[m], 1);
        }
        const bool ok = !(ai < 0 || ai >= n || gi < 0 || gi >= n);
        double s = 0.0;
        if (ok) {
            const TB* row = base + static_cast<int64_t>((r & 1) ? gi : ai) * d;
            if constexpr (kVec) {
                constexpr int kPer = 16 / static_cast<int>(sizeof(TB));
                const fsp_u32x4* pieces = reinterpret_cast<const fsp_u32x4*>(row);
                for (int t0 = 0; t0 < d; t0 += kPer) {
                    const fsp_u32x4 piece = pieces[t0 / kPer];
#pragma unroll
                    for (int e = 0; e < kPer; e++) {
                        const double qv = s_q[t0 + e];
                        const double dg = qv - static_cast<double>(RowCodec<TB>::piece_f32(piece, e));
                        const double pg = dg * dg;
                        s = s + pg;
                    }
                }
            } else {
                for (int t = 0; t < d; t++) {
                    const double qv = q_lds ? s_q[t] : static_cast<double>(qr[t]);
                    const double dg = qv - static_cast<double>(row[t]);
                    const double pg = dg * dg;
                    s = s + pg;
                }
            }
        }
        // a place with an id that is no row: dGt = 0, which the fold skips like the reference's `continue`
        if (r & 1) s_dg[i] = ok ? sqrt(s) : 0.0;
        else s_da[i] = ok ? sqrt(s) : 0.0;
    }
    __syncthreads();
    if (tid >= 64) return;

    const int lane = tid;
    const int myk = lane < nk ? ks.k[lane] : 0;
    double tot = 0.0, snap_tot = 0.0;
    int usedt = 0, snap_used = -1;
    for (int i0 = 0; i0 < lim; i0 += 64) {
        const int i = i0 + lane;
        double term = 0.0;
        int used = 0;
        if (i < lim) {
            const double dGt = s_dg[i];
            if (dGt > 0) { term = s_da[i] / dGt; used = 1; }
        }
        for (int l = 0; l < 64; l++) {
            const double v = __shfl(term, l);
            const int u = __shfl(used, l);
            if (u) { tot = tot + v; usedt += u; }
            if (myk == i0 + l + 1) { snap_tot = tot; snap_used = usedt; }
        }
    }
    if (lane < nk) {
        int hits = 0;
        for (int m = 0; m < myk; m++) hits += s_hist[m];
        const double kd = static_cast<double>(myk);
        const double nan = __longlong_as_double(0x7FF8000000000000LL);
        const int64_t o = static_cast<int64_t>(lane) * nq + qi;
        recall[o] = static_cast<double>(hits) / kd;
        ratio[o] = (na >= myk && snap_used == myk) ? snap_tot / kd : nan;
        if (cand_ratio) {
            const int32_t u = unique[qi];
            cand_ratio[o] = u > 0 ? static_cast<double>(u) / kd : nan;      // FSA:824-828
        }
    }
}

}  // namespace fspann
