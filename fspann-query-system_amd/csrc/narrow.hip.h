// narrow.hip.h — lossless row narrowing on the device (include/fspann_narrow.h, api_narrow.hip.h): which row types
// hold a block of fp32 or fp64 rows EXACTLY, and the rows re-packed as one of them.  The inverse direction of RowCodec<T>::wide:
// RowCodec<T>::fits / narrow (row_codec.hip.h) say what an element of T is, the two kernels here stream the rows through them.
// Nothing is rounded, shifted or scaled: a type is taken only when every element already is a value of it.
//
// Both kernels walk the rows as one flat array of n * dim elements in 16-byte SLOTS of the side that is accessed 16 bytes at a
// time (the source for the fit pass, the destination for the narrow pass); slot s holds the elements s * N - mis .. + N - 1, `mis`
// being the base pointer's distance from a 16-byte boundary in elements.  A slot inside the range moves as one 16-byte access, a slot
// on an edge element by element — any alignment and any dim go through the same loop.
#pragma once
#include "fspann_common.h"

namespace fspann {

constexpr int kNarrowThreads = 256;
constexpr int kNarrowTile = 4096;                 // elements of a rows_fit_kernel tile: as many WHOLE rows as fit (one row when dim is larger)
constexpr int kNarrowSlots = 4;                   // 16-byte output slots per thread of rows_narrow_kernel
constexpr unsigned long long kNoMisfit = ~0ull;   // first[]: every element fits
constexpr uint32_t kAllDtypes = 0x7fu;            // bit (1u << FSPANN_x) of every row of FSPANN_DTYPE_TABLE

// What the fit pass leaves in device memory (set to kNoMisfit / 0 before the launch).
struct FitResult {
    unsigned long long first[8];      // per dtype id: flat index row * dim + col of the first element that is not a value of it
    unsigned long long nonfinite;     // elements that are NaN or +-inf
};
// ... and the narrow pass.
struct NarrowResult {
    unsigned long long first, misfits;
};

template <typename TS> struct NarrowSrc {
    static constexpr int N = 16 / static_cast<int>(sizeof(TS));
    typedef TS vec __attribute__((ext_vector_type(N)));
    // the types a block of TS can be narrowed to: every strictly smaller one
    template <typename T> static constexpr bool takes = sizeof(T) < sizeof(TS);
};

// One source element.  The rows may start at ANY byte (fp64 rows 4 bytes off an 8-byte boundary included): an element load assumes
// no alignment; only the 16-byte loads do, and they are taken where the address allows.
template <typename TS> __device__ __forceinline__ TS narrow_load(const TS* src, int64_t e) {
    TS v;
    __builtin_memcpy(&v, reinterpret_cast<const char*>(src) + e * static_cast<int64_t>(sizeof(TS)), sizeof(TS));
    return v;
}

// RowCodec<T>::fits where T is narrower than the source (nothing else is ever asked; double has no fits)
template <typename T, typename TS> __device__ __forceinline__ bool fits_narrower(TS x) {
    if constexpr (NarrowSrc<TS>::template takes<T>) return RowCodec<T>::fits(x);
    else return true;
}

// The exact flat index of type T's first misfit in the slot a wave has just found one in: its lanes 0 .. N - 1 read the slot's
// elements again (cache hits), once per wave and type.  Wave-uniform.
template <typename T, typename TS>
__device__ __forceinline__ int64_t fit_first_in_slot(const TS* __restrict__ src, int64_t slot, int mis, int64_t e0, int64_t e1) {
    constexpr int N = NarrowSrc<TS>::N;
    const int lane = threadIdx.x & 63;
    const int64_t e = slot * N - mis + lane;
    const bool bad = lane < N && e >= e0 && e < e1 && !RowCodec<T>::fits(narrow_load(src, e));
    return slot * N - mis + __builtin_ctzll(__ballot(bad) | (1ull << (N - 1)));      // (the slot was recorded because it holds a misfit)
}

// One streaming pass over [n][dim] packed rows of TS (float or double).  A TILE is `rows_per_wg` whole rows, i.e. the elements
// [e0, e1); a workgroup takes the tiles blockIdx.x, + gridDim.x, ... in ascending order, in 16-byte source slots: per step a wave
// loads kFitUnroll groups of 64 consecutive slots, then tests them.  Per candidate type T the wave keeps, in scalar registers, the
// index of its first element that is not a value of T: ballot + find-first-set, no vector work and no atomic in the loop.  Misfits
// are the common case (random floats fit nothing), so
//   * a type whose first misfit is known — in this wave, or globally in front of the wave's first tile when it starts (ONE 64-byte
//     read of the result block per wave) — is not tested again (without a row mask nothing else depends on it): a block that fits
//     nothing costs the loads and the finite test;
//   * at its end a WORKGROUP issues one read of the result block and at most one atomicMin per type, none for a type whose global
//     value already lies below its own.
// kMask: row_fits[r] receives bit id for every type the whole row r fits.  The workgroup keeps its tile's bytes in LDS (rows are
// never shared between workgroups), and only a slot holding a misfit touches them.
constexpr int kFitUnroll = 4;
template <typename TS, bool kMask>
__global__ __launch_bounds__(kNarrowThreads) void rows_fit_kernel(const TS* __restrict__ src, int64_t n, int dim, int rows_per_wg, uint8_t* __restrict__ row_fits,
                                                                  FitResult* __restrict__ out) {
    using S = NarrowSrc<TS>;
    constexpr int N = S::N;
    __shared__ uint32_t rowm[kMask ? kNarrowTile / 4 : 1];
    __shared__ unsigned long long wgfirst[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mis = static_cast<int>((reinterpret_cast<uintptr_t>(src) / sizeof(TS)) % N);
    const bool vec_ok = reinterpret_cast<uintptr_t>(src) % sizeof(TS) == 0;      // (else no slot is 16-byte aligned)
    const int64_t ntiles = (n + rows_per_wg - 1) / rows_per_wg;

    // the types still tested by this wave (wave-uniform), and the index of the wave's first misfit of each
    uint32_t live = 0;
    int64_t wfirst[8];
#define FSPANN_FIT_INIT(ID, T, QUERY, FINITE, WORDS, USES, NOUN) \
    wfirst[ID] = -1;                                             \
    if constexpr (S::template takes<T>) live |= 1u << ID;
    FSPANN_DTYPE_TABLE(FSPANN_FIT_INIT)
#undef FSPANN_FIT_INIT
    if constexpr (!kMask) {
        const unsigned long long g = lane < 8 ? __atomic_load_n(&out->first[lane], __ATOMIC_RELAXED) : kNoMisfit;
        live &= static_cast<uint32_t>(__ballot(g >= static_cast<unsigned long long>(blockIdx.x) * rows_per_wg * dim));
    }
    unsigned long long nonfinite = 0;

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t r0 = tile * rows_per_wg;
        const int64_t r1 = r0 + rows_per_wg < n ? r0 + rows_per_wg : n;
        const int64_t e0 = r0 * dim, e1 = r1 * dim;
        const int64_t s0 = (e0 + mis) / N, s1 = (e1 + mis + N - 1) / N;
        if constexpr (kMask) {
            for (int i = tid; i < kNarrowTile / 4; i += kNarrowThreads) rowm[i] = kAllDtypes * 0x01010101u;
            __syncthreads();
        }
        for (int64_t sb0 = s0 + wave * 64; sb0 < s1; sb0 += kNarrowThreads * kFitUnroll) {
            TS x[kFitUnroll][N];
#pragma unroll
            for (int u = 0; u < kFitUnroll; u++) {
                const int64_t s = sb0 + u * kNarrowThreads + lane;
                const int64_t ef = s * N - mis;                   // the slot's first element
                if (vec_ok && s < s1 && ef >= e0 && ef + N <= e1) {
                    const typename S::vec v = __builtin_nontemporal_load(reinterpret_cast<const typename S::vec*>(src + ef));
#pragma unroll
                    for (int j = 0; j < N; j++) x[u][j] = v[j];
                } else {                                          // an edge of the tile: what lies outside counts as 0, which fits every type
#pragma unroll
                    for (int j = 0; j < N; j++) x[u][j] = (s < s1 && ef + j >= e0 && ef + j < e1) ? narrow_load(src, ef + j) : static_cast<TS>(0);
                }
            }
#pragma unroll
            for (int u = 0; u < kFitUnroll; u++) {
                const int64_t sb = sb0 + u * kNarrowThreads;
                const int64_t ef = (sb + lane) * N - mis;
                bool fin = true;
#pragma unroll
                for (int j = 0; j < N; j++) fin = fin && __builtin_isfinite(x[u][j]);
                if (__ballot(!fin)) {                             // (counted per element only where a wave's slots hold one)
#pragma unroll
                    for (int j = 0; j < N; j++) nonfinite += __popcll(__ballot(!__builtin_isfinite(x[u][j])));
                }
                uint32_t vbad = 0;                                // kMask: the types this lane's slot does not fit
#define FSPANN_FIT_TEST(ID, T, QUERY, FINITE, WORDS, USES, NOUN)                                                         \
    if constexpr (S::template takes<T>) {                                                                                \
        if (live & (1u << ID)) {                                                                                         \
            bool ok = true;                                                                                              \
            _Pragma("unroll") for (int j = 0; j < N; j++) ok = ok && fits_narrower<T>(x[u][j]);                          \
            const unsigned long long bad = __ballot(!ok);                                                                \
            if (bad != 0 && wfirst[ID] < 0) {                                                                            \
                wfirst[ID] = fit_first_in_slot<T, TS>(src, sb + __builtin_ctzll(bad), mis, e0, e1);                      \
                if (!kMask) live &= ~(1u << ID);                                                                         \
            }                                                                                                            \
            if (kMask && !ok) vbad |= 1u << ID;                                                                          \
        }                                                                                                                \
    }
                FSPANN_DTYPE_TABLE(FSPANN_FIT_TEST)
#undef FSPANN_FIT_TEST
                if constexpr (kMask) {
                    if (vbad) {                                   // which of the slot's elements, hence which rows, lose which bits
#pragma unroll
                        for (int j = 0; j < N; j++) {
                            if (ef + j < e0 || ef + j >= e1) continue;
                            uint32_t ebad = 0;
#define FSPANN_FIT_ELEM(ID, T, QUERY, FINITE, WORDS, USES, NOUN) \
    if constexpr (S::template takes<T>) ebad |= fits_narrower<T>(x[u][j]) ? 0u : 1u << ID;
                            FSPANN_DTYPE_TABLE(FSPANN_FIT_ELEM)
#undef FSPANN_FIT_ELEM
                            const uint32_t r = static_cast<uint32_t>(ef + j - e0) / static_cast<uint32_t>(dim);
                            if (ebad) atomicAnd(&rowm[r >> 2], ~(ebad << (8 * (r & 3))));
                        }
                    }
                }
            }
        }
        if constexpr (kMask) {
            __syncthreads();
            for (int64_t i = tid; i < r1 - r0; i += kNarrowThreads) row_fits[r0 + i] = static_cast<uint8_t>(rowm[i >> 2] >> (8 * (i & 3)));
            __syncthreads();
        }
    }

    // The workgroup's waves fold their first misfits in LDS, and lanes 0..7 of its first wave publish them: ONE read of the result
    // block and at most one atomic instruction per workgroup.  Every wave reading and lowering the same 64 bytes at the end of the
    // launch is a queue on one L2 line (measured: a "nothing fits" pass 50 us behind an "everything fits" one).
    if (tid < 8) wgfirst[tid] = kNoMisfit;
    __syncthreads();
    if (lane == 0) {
#define FSPANN_FIT_PUBLISH(ID, T, QUERY, FINITE, WORDS, USES, NOUN) \
    if (wfirst[ID] >= 0) atomicMin(&wgfirst[ID], static_cast<unsigned long long>(wfirst[ID]));
        FSPANN_DTYPE_TABLE(FSPANN_FIT_PUBLISH)
#undef FSPANN_FIT_PUBLISH
        if (nonfinite != 0) atomicAdd(&out->nonfinite, nonfinite);
    }
    __syncthreads();
    if (tid < 8) {
        const unsigned long long mine = wgfirst[tid];
        if (mine != kNoMisfit && mine < __atomic_load_n(&out->first[tid], __ATOMIC_RELAXED)) atomicMin(&out->first[tid], mine);
    }
}

// an element's bits, at the bottom of a dword
template <typename TD> __device__ __forceinline__ uint32_t narrow_bits(TD y) {
    if constexpr (sizeof(TD) == 1) return __builtin_bit_cast(uint8_t, y);
    else if constexpr (sizeof(TD) == 2) return __builtin_bit_cast(uint16_t, y);
    else return __builtin_bit_cast(uint32_t, y);
}

// One pass: packed [n][dim] rows of TS re-packed as rows of the smaller TD.  A thread fills kNarrowSlots 16-byte destination slots
// (consecutive lanes consecutive slots), each from N = 16 / sizeof(TD) source elements — 16-byte loads when the source of a slot is
// 16-byte aligned too (src_vec, the same for every slot), else element loads.  An element that is not a value of TD is counted and
// the first such index kept (the caller ran the fit pass, so this is the error path: a slot without one costs the `&&` chain);
// what is stored for it is unspecified.
template <typename TS, typename TD>
__global__ __launch_bounds__(kNarrowThreads) void rows_narrow_kernel(const TS* __restrict__ src, int64_t ne, TD* __restrict__ dst, NarrowResult* __restrict__ out) {
    static_assert(sizeof(TD) < sizeof(TS), "a target is narrower than its source");
    using S = NarrowSrc<TS>;
    constexpr int N = 16 / static_cast<int>(sizeof(TD)), NV = N / S::N;
    const int lane = threadIdx.x & 63;
    const int mis = static_cast<int>((reinterpret_cast<uintptr_t>(dst) / sizeof(TD)) % N);
    const bool src_vec = ((reinterpret_cast<uintptr_t>(src) - mis * sizeof(TS)) & 15) == 0;      // (N * sizeof(TS) is a multiple of 16)
    const int64_t s1 = (ne + mis + N - 1) / N;
    unsigned long long first = kNoMisfit;
    uint32_t misfits = 0;

    for (int it = 0; it < kNarrowSlots; it++) {
        const int64_t s = (static_cast<int64_t>(blockIdx.x) * kNarrowSlots + it) * kNarrowThreads + threadIdx.x;
        if (s >= s1) break;
        const int64_t ef = s * N - mis;
        const bool whole = ef >= 0 && ef + N <= ne;
        TS x[N];
        if (whole && src_vec) {
#pragma unroll
            for (int v = 0; v < NV; v++) {
                const typename S::vec w = __builtin_nontemporal_load(reinterpret_cast<const typename S::vec*>(src + ef) + v);
#pragma unroll
                for (int j = 0; j < S::N; j++) x[v * S::N + j] = w[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < N; j++) x[j] = (ef + j >= 0 && ef + j < ne) ? narrow_load(src, ef + j) : static_cast<TS>(0);
        }
        bool ok = true;
#pragma unroll
        for (int j = 0; j < N; j++) ok = ok && RowCodec<TD>::fits(x[j]);
        if (!ok) {
#pragma unroll
            for (int j = 0; j < N; j++)
                if (!RowCodec<TD>::fits(x[j])) {
                    misfits++;
                    if (first == kNoMisfit) first = static_cast<unsigned long long>(ef + j);
                }
        }
        if (whole) {
            fsp_u32x4 o = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < N; j++) o[j * static_cast<int>(sizeof(TD)) / 4] |= narrow_bits(RowCodec<TD>::narrow(x[j])) << (8 * ((j * static_cast<int>(sizeof(TD))) & 3));
            *reinterpret_cast<fsp_u32x4*>(dst + ef) = o;
        } else {
#pragma unroll
            for (int j = 0; j < N; j++)
                if (ef + j >= 0 && ef + j < ne) dst[ef + j] = RowCodec<TD>::narrow(x[j]);
        }
    }
    // the error path: one add and at most one min per wave (a thread's slots ascend, so `first` is its lowest misfit)
    if (__ballot(misfits != 0) == 0) return;
    for (int off = 32; off > 0; off >>= 1) {
        misfits += __shfl_down(misfits, off);
        const unsigned long long o = __shfl_down(first, off);
        first = o < first ? o : first;
    }
    if (lane == 0) {
        atomicAdd(&out->misfits, static_cast<unsigned long long>(misfits));
        if (first < __atomic_load_n(&out->first, __ATOMIC_RELAXED)) atomicMin(&out->first, first);
    }
}

}  // namespace fspann
