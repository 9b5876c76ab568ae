// fspann_common.h — context, error plumbing and small helpers shared by the
// gfx950 kernels and the C ABI (include/fspann.h).  Product code: never includes
// or links anything under oracle/.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fspann.h"

namespace fspann {

// ---- thread-local error message ------------------------------------------------
inline std::string& last_error_ref() {
    static thread_local std::string s;
    return s;
}
inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error_ref() = buf;
    return code;
}

#define FSP_HIP(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return ::fspann::fail(_e == hipErrorOutOfMemory ? FSPANN_E_NOMEM : FSPANN_E_DEVICE,    \
                                  "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                                  __LINE__);                                                       \
    } while (0)

// One FSPANN_BF16 row element: 16 bits b, value = the fp32 whose bit pattern is b << 16 (every bfloat16, subnormals, +-0, +-inf and
// NaN included).  A type of its own, so that a bf16 row is never taken for a half or for a uint16_t id.  Widening is a shift: exact,
// no conversion instruction that could round or flush.
struct fsp_bf16 {
    uint16_t b;
    __host__ __device__ __forceinline__ explicit operator float() const { return __builtin_bit_cast(float, static_cast<uint32_t>(b) << 16); }
    __host__ __device__ __forceinline__ explicit operator double() const { return static_cast<double>(static_cast<float>(*this)); }
};
static_assert(sizeof(fsp_bf16) == 2 && alignof(fsp_bf16) == 2, "a bf16 row element is two bytes");

// One FSPANN_F8E4M3 row element: the OCP fp8 e4m3fn byte b = S EEEE MMM, bias 7 (E = 0: +-M/8 * 2^-6; else +-(1 + M/8) * 2^(E-7);
// 0x7F / 0xFF NaN, no infinity, |x| <= 448).  A type of its own, so that an fp8 row is never taken for a uint8_t row or a flag
// byte.  On the device the widening is the hardware's v_cvt_f32_fp8 (gfx950 converts the OCP format): exact, every e4m3 value is
// a float; the host spells the definition out.
struct fsp_f8e4m3 {
    uint8_t b;
    __host__ __device__ __forceinline__ explicit operator float() const {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(b), 0);
#else
        const int e = (b >> 3) & 15, m = b & 7;
        const float mag = (e == 15 && m == 7) ? __builtin_nanf("") : e == 0 ? __builtin_ldexpf(static_cast<float>(m), -9)
                                                                         : __builtin_ldexpf(static_cast<float>(8 + m), e - 10);
        return (b & 0x80) ? -mag : mag;
#endif
    }
    __host__ __device__ __forceinline__ explicit operator double() const { return static_cast<double>(static_cast<float>(*this)); }
};
static_assert(sizeof(fsp_f8e4m3) == 1 && alignof(fsp_f8e4m3) == 1, "an fp8 row element is one byte");

}  // namespace fspann
#include "dtypes.h"     // the table of the dtypes, their dispatchers and the refusal by name
#include "row_codec.hip.h"   // one RowCodec per row of the table: what the kernels know about an element type
namespace fspann {

// ---- order-key bit budget (DESIGN.md "Java order key") ----------------------------
// key = score(10) | bucket(20) | seq(22); seq = (td*P + step)*S + pos is unique per tuple.
constexpr int kSeqBits = 22;
constexpr int kBucketBits = 20;
constexpr int kScoreBits = 10;
constexpr uint32_t kSeqMask = (1u << kSeqBits) - 1;
constexpr uint32_t kEmptyKey = 0xFFFFFFFFu;

// One (t,d) table inside the concatenated device arrays.
struct RouteTable {
    int64_t part_base;  // first partition of this table in keys2 / rep
    int64_t off_base;   // first entry of this table in id_off (nparts+1 entries per table)
    int64_t ids_base;   // first id of this table in ids
    int32_t nparts;
    int32_t dir_base;   // first entry pair of this table in the radix directory (RouteParams::dir), in pairs
};

// Members that free themselves: a device block, a pinned host block, a grown-on-demand work area.  Whoever destroys their holder has
// set the device and drained the streams that may still read them (fspann_ctx_destroy, ~IndexFamily).
struct HipFree { void operator()(void* p) const { (void)hipFree(p); } };
struct HipHostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
template <class T> using DevPtr = std::unique_ptr<T, HipFree>;
using PinPtr = std::unique_ptr<void, HipHostFree>;
// p = a fresh device block of `bytes`; what it held goes first
template <class T> hipError_t dev_alloc(DevPtr<T>& p, size_t bytes) {
    p.reset();
    void* raw = nullptr;
    const hipError_t e = hipMalloc(&raw, bytes);
    p.reset(static_cast<T*>(raw));
    return e;
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    unsigned gen = 0;   // bumped by every (re)allocation: "same address" does not mean "same contents"
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// fspann_ctx::ws_io by what each host-pointer call keeps in a slot on its Direct transport (host_staging.h lays the calls out; a Block
// call sends its way up through its first slot and fetches its way down from the slot marked so)
enum IoSlot : int {
    kIoEncQ = 0, kIoEncCodes = 1, kIoEncBad = 2, kIoEncHashes = 3,
    kIoRouteCodes = 0, kIoRouteIds = 1 /* Block: down */, kIoRouteScores = 2, kIoRouteCounts = 3,
    kIoRefQ = 0, kIoRefRows = 1, kIoRefIds = 2, kIoRefCounts = 3 /* in | count | scored */, kIoRefOutIds = 4 /* Block: down */, kIoRefOutDist = 5,
    kIoHandles = 6      // fspann_set_deleted's handles (api_ext.hip.h)
};

// What fspann_ctx_clone shares: GFunctions, frozen index, id metadata and touched set of ONE index in HBM, held by shared_ptr from
// its owner (the context that built or imported it) and from every clone, freed with the last of them.  Read-only while a clone is
// alive (may_change_shared, api_common.hip.h), except the deleted bits and the touched set: own locks, published as atomics.  The
// clone count changes only while nothing here can be mutated: a clone is made under its source's lock (an owner mutates under its
// own lock and at count 0; a clone as source keeps the count above 0) and leaves the count after synchronising its own stream.
struct IndexFamily {
    int device = 0;
    std::atomic<int> clones{0};               // clones alive
    std::atomic<bool> owner_gone{false};      // the owner was destroyed: the family takes no new clone

    // GFunctions: alphaT[dim][P_total] fp64 (transposed for coalescing), r/omega[P_total]
    DevPtr<double> d_alphaT;
    DevPtr<double> d_alpha_rows;               // alpha as the JVM hands it over, [P][d]: the re-check of the MFMA path reads a projection's row 64 dimensions at a time
    DevPtr<double> d_r, d_omega;
    std::vector<double> h_alpha, h_r, h_omega;  // host copies (export)
    DevPtr<float> d_alphaT32;                  // fp32 copy of alphaT for the MFMA fast path
    double alpha_norm_max = 1.0;               // max_j ||alpha_j||_2 (error bound of the fast path)
    bool have_g = false;

    // frozen index (concatenated over td)
    std::vector<RouteTable> h_tables;
    std::vector<std::vector<int64_t>> h_min, h_max, h_off;  // host mirror per td (export / rebuild / the host's replay of a query)
    std::vector<std::vector<uint64_t>> h_rep;
    std::vector<std::vector<int32_t>> h_ids;
    std::vector<char> h_table_set;
    bool dev_index_dirty = true;
    DevPtr<RouteTable> d_tables;
    DevPtr<int64_t> d_recs;       // [total_parts][rec_words] partition records {minKey, maxKey, rep[W], id offset | size << 32}
    int rec_words = 0;
    DevPtr<int2> d_dir;           // radix directory of the probe: [TD][2^dir_bits + 1] {first maxKey >= bound, first minKey >= bound}
    int dir_bits = 0;
    DevPtr<int32_t> d_ids;
    DevPtr<int32_t> d_inv;        // [TD][n_ids] inverse id map for the bounded select (null: a table holds an id twice)
    DevPtr<uint64_t> d_ids_bk;    // per partition: (id << 32 | bucket field) sorted by bucket, for the bounded select
    DevPtr<uint16_t> d_bin16;     // [total_parts][1 << bin16_shift] HashMap bin (at cap0) of every id, partition order, padded per partition:
    int bin16_shift = 0;          //   what the bounded select's exact treeify check reads (one 128-byte line per 64-id partition)
    int meta_epoch = 0, bk_epoch = -1;  // d_ids_bk / d_inv are valid for the id metadata of bk_epoch
    int64_t total_parts = 0, total_ids = 0;

    // id metadata
    int64_t n_ids = 0;
    DevPtr<int32_t> d_java_hash;
    std::vector<int32_t> h_java_hash;
    bool decimal_ids = false;  // ids are Long.toString(handle): String.hashCode computed in-kernel
    // mirror of metadata.isDeleted (PIS:739), one bit per handle; nullptr => nothing deleted so far.  fspann_set_deleted may allocate
    // it on any context of the family while the others serve: published with release, read with acquire at every call.
    std::atomic<uint32_t*> d_deleted_bits{nullptr};
    std::vector<uint32_t> h_deleted_bits;   // host mirror (guarded by deleted_mu): the host replay of a query reads it
    std::mutex deleted_mu;
    // touched-record set of selective re-encryption (api_touch.hip.h): one byte per handle, whole kTouchTile tiles (padding zero).
    // Every context of the family marks into it.  Allocated / reallocated under touch_mu, and published before touch_on: a context
    // that sees touch_on sees the set.  Count and drain hold touch_mu.
    std::mutex touch_mu;
    std::atomic<uint8_t*> d_touch{nullptr};
    int64_t touch_n = 0;             // handles the set covers (n_ids when it was allocated)
    size_t touch_bytes = 0;
    std::atomic<bool> touch_on{false};

    ~IndexFamily() {
        (void)hipSetDevice(device);
        if (uint32_t* db = d_deleted_bits.load()) (void)hipFree(db);
        if (uint8_t* ts = d_touch.load()) (void)hipFree(ts);
    }
};

// The plaintext store (test / bench harness) a context refines from.  A clone starts on its source's store and may install one of
// its own (fspann_store_set / fspann_store_attach_dev install a NEW RowStore; the rows go with the last context that refers to them).
struct RowStore {
    void* rows = nullptr;
    bool owned = false;              // false: rows attached from caller-owned device memory (fspann_store_attach_dev)
    int dtype = FSPANN_F32;
    int64_t n = 0;
    unsigned gen = 1;                // one more than the store it replaced (fspann_ctx::store_ok_gen keys on it)
    RowStore() = default;
    RowStore(const RowStore&) = delete; RowStore& operator=(const RowStore&) = delete;
    ~RowStore() { if (owned && rows) (void)hipFree(rows); }
};

}  // namespace fspann

// The opaque context of include/fspann.h.
constexpr int kDirBitsAuto = 99;   // knob_dir_extra_bits: size the probe's radix directory by a memory budget (fspann_api.hip)
struct fspann_ctx {
    // Calls on one context are serialised INSIDE the library: every entry point that takes a context holds this
    // lock for its duration (recursive: entry points call each other).  Different contexts — e.g. the clones of one index —
    // run concurrently.
    std::recursive_mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    fspann_cfg cfg{};
    int TD = 0, W = 0, bits = 0, P_total = 0;  // P_total = TD*m projections
    int hard_cap = 0;                          // max(maxGlobalCandidates, refinementLimit), PIS:612-615
    int cap0 = 0;                              // tableSizeFor(min(HARD_CAP, 1<<16)), PIS:619
    int num_cus = 256;
    int lds_limit = 160 * 1024;
    bool frozen = false;
    // a clone reads its source's family and store in place; its stream, knobs and work areas are its own and go when IT is destroyed
    std::shared_ptr<fspann::IndexFamily> fam;
    std::shared_ptr<fspann::RowStore> store;   // never null; rows == nullptr: no store set
    bool is_clone = false;           // made by fspann_ctx_clone: counted in fam->clones, may not change what the family shares
    long long* dbg_route = nullptr;  // per-block phase stamps, caller-owned; only reachable in FSPANN_DEBUG_STAMPS builds (tools/)
    // tuning / test knobs, read from the environment ONCE at fspann_ctx_create (never per call)
    int knob_ht_x4 = 0;              // FSPANN_ROUTE_HT_X4=1: hash load factor <= 0.5 instead of <= 0.8
    int knob_threads = 0;            // FSPANN_ROUTE_THREADS: 512 / 1024 force the full select's workgroup size (0: by list length)
    int knob_lazy_cap = 0;           // FSPANN_ROUTE_LAZY_CAP: entries one query may hold in the bounded select (tests)
    int knob_fused_probe = 1;        // FSPANN_ROUTE_FUSED_PROBE=0: separate probe kernel in front of the bounded select
    int knob_refine_dc = 0;          // FSPANN_REFINE_DC: dims per LDS tile of the refinement scan (tools/refine_bench.py)
    int knob_dir_extra_bits = kDirBitsAuto;   // FSPANN_ROUTE_DIR_EXTRA_BITS: finer (+) or coarser (-) radix directory than four partitions per entry; unset: auto
    bool knob_lazy_small = true;     // FSPANN_ROUTE_LAZY_SMALL: 512-entry size class of the bounded select for limit <= 256 (0: always 1024)
    bool knob_probe_dir = true;      // FSPANN_ROUTE_DIR: radix directory + one-round window in the probe (0: plain G-ary search)
    int knob_refine_stream = -1;     // FSPANN_REFINE_STREAM: workgroups per CU of the streaming refinement scan (-1: 4 dense / 3 gather, 0: one workgroup per query)
    int knob_tick_refine = 1;        // FSPANN_TICK_REFINE: refine workgroups per CU inside a tick (each streams several queries)
    int knob_gpu_cut = 1;            // FSPANN_GPU_CUT=0: fspann_build_index cuts the partitions on host threads (std::sort) instead of the GPU radix sort
    int knob_wave_sort = 1;          // FSPANN_ROUTE_WAVE_SORT=0: long lists' groups are sorted by the whole workgroup one by one (dev A/B)
    int knob_tick_fuse = 1;          // FSPANN_TICK_FUSE=0: fspann_tick_dev always uses the stand-alone kernels
    int knob_front_encode = 1;       // FSPANN_FRONT_ENCODE: encode role of the front launch, mfma (1, default) or exact (0: encode_exact_block; dev A/B)
    int knob_tick_front = 100;       // FSPANN_TICK_FRONT: percent of a tick's Route workgroups that head the grid
    int64_t gt_scratch_bytes = int64_t(8192) << 20;   // FSPANN_GT_SCRATCH_MB: budget of the ground truth's [query chunk x n] distance matrix
    int knob_bincheck = -1;          // FSPANN_ROUTE_BINCHECK: the bounded select's exact treeify check (-1: on for opaque ids, off for decimal ordinals; 0 / 1 force)
    bool knob_shape_spec = true;     // FSPANN_ROUTE_SHAPE_SPEC=0: the bounded select's build with run-time tables x probes also for 16 x 5 (dev A/B)
    int knob_mfma_tile = 0;          // FSPANN_ENCODE_MFMA_TILE=1: the 32 x 128 block tile of the MFMA encode for every batch size (dev A/B)
    int knob_encode_qb = 0;          // FSPANN_ENCODE_QB: query rows per workgroup of the exact encode (0 = by batch size; dev A/B)
    bool knob_zero_copy = true;      // FSPANN_ZERO_COPY=0: tiny host-pointer calls go through copy commands like larger ones (dev A/B)
    int knob_route_lds_kb = 0;       // FSPANN_ROUTE_LDS_KB: LDS the full select may plan with (0 = all of it); less leaves room for scan workgroups beside it
    int knob_route_wgs = 0;          // FSPANN_ROUTE_WGS: workgroups per CU of the full select's grid (0 = what fits, at most 4)
    int knob_devflags = 0;           // FSPANN_ROUTE_DEVFLAGS: dev A/B switches of the full select (route.hip.h)
    bool knob_refine_run = true;     // FSPANN_REFINE_RUN=0: long lists keep one partial top-k list per 256-row chunk (dev A/B)
    bool knob_slice = true;          // FSPANN_ROUTE_SLICE=0: the full select's global-arena mode builds its hash in the arena (dev A/B)
    int last_tick_fused = 0;
    int last_front_encode_mfma = 0;  // the last fspann_tick_dev coded its batch with front_kernel's MFMA role (encode_mfma_block)

    int encode_mode = 0;                       // 0 auto, 1 exact fp64, 2 MFMA fp32 + exact re-check
    unsigned long long fix_cap_last = 0;       // capacity of the re-check list of the last MFMA-path call
    bool mfma_last = false;                    // the last encode took the MFMA path
    fspann::DevBuf ws_fix;                     // fix list + counter + int32 hashes of the MFMA path
    int route_mode = 0;              // 0 auto, 1 always route_select_kernel, 2 bounded select whenever its preconditions hold
    fspann::DevBuf ws_ovf;
    // kernel-attached HIP events of the refinement scan (fspann_refine_timing_begin / _end)
    std::vector<hipEvent_t> rt_events;   // pairs: start, stop
    size_t rt_used = 0;
    int rt_every = 1, rt_seen = 0;       // events go on every rt_every-th dispatch
    bool rt_on = false;
    // work areas of the search calls, each laid out once by its struct's lay() (Carver, api_common.hip.h)
    fspann::DevBuf ws_search;        // SearchArea: codes / F_q ids / counts / bad of fspann_search_store_dev (api_common.hip.h)
    fspann::DevBuf ws_retry;         // RetryArea: pick list, retried / scored, the list's count of fspann_search_retry_dev (api_retry.hip.h)
    fspann::DevBuf ws_fallback;      // FallbackArea: fallback list, member / fellback flags, the list's count of fspann_search_fallback_dev (api_eval.hip.h)
    fspann::DevBuf ws_sweep;         // SweepArea: keys, clipped counts, pass 1's counts, caps, pick list and planes of the sweep calls (api_sweep.hip.h)
    int64_t sweep_nq = 0, sweep_bmax = 0;   // the last fspann_search_sweep_dev: what its finish call must repeat (0: none)
    int sweep_nl = 0, sweep_k = 0;
    struct LdsCeiling { const void* kernel; size_t bytes; };
    static constexpr int kLdsCeilings = 64;
    LdsCeiling lds_ceilings[kLdsCeilings] = {};   // kernels whose dynamic-LDS ceiling this context has raised on its device, and to what (raise_lds_ceiling)
    int n_lds_ceilings = 0;
    int ovf_flip = 0;                // which of the two overflow counters the last bounded select used
    unsigned ovf_gen_seen = 0;       // ws_ovf.gen whose counters have been zeroed (0 = never)
    int last_route_lazy = 0;         // 1 if the last fspann_route[_dev] ran the bounded select
    fspann::DevPtr<int32_t> d_unmodelled;   // device counter: queries flagged "HashMap bin treeified" (out_count = -1) since the last reset

    unsigned store_ok_gen = 0;       // store->gen that store_ok was computed for (0: none)
    fspann::DevBuf store_ok;         // per store row: 1 = all dim values finite (api_touch.hip.h, computed at the first mark)
    fspann::DevBuf ws_touch;         // tile counts / offsets / total / handles of fspann_touch_count / _drain
    fspann::DevBuf ws_narrow;        // FitResult / NarrowResult of the fit and narrow passes (api_narrow.hip.h)

    // scratch arenas (grown on demand, reused across calls)
    fspann::DevBuf ws_route;   // global hash/sort fallback for the route kernel
    fspann::DevBuf ws_probe;   // probe lists handed from route_probe_kernel to route_select_kernel
    fspann::DevBuf ws_refine;  // per-chunk partial top-k
    fspann::DevBuf ws_gt;      // [query chunk][n] distance matrix of fspann_groundtruth_dev (fp64) / _typed_dev over bytes (uint32, + the norms)
    fspann::DevBuf ws_tickfix; // arenas of the full select run by the refine role of a tick for PENDING queries
    static constexpr int kFixSlots = 8;
    fspann::DevPtr<void> d_fixparams;    // kFixSlots RouteParams blocks in device memory (parameters of that redo) ...
    std::vector<unsigned char> h_fixparams;   // ... and what each slot holds
    unsigned fix_valid = 0;
    int fix_next = 0;
    fspann::DevBuf ws_io[8];   // staging for the host-pointer entry points (IoSlot)
    fspann::PinPtr h_pin;      // pinned host block (kPinBytes) for the small transfers of the host-pointer entry points: one H2D and one D2H
    void* d_pin = nullptr;     // the same block as the device sees it (mapped host memory): kernels of the tiniest calls read and write it directly
    fspann::PinPtr h_rows;     // fspann_host_buffer: pinned host memory the adapter packs decrypted rows into (grown on demand)
    size_t h_rows_bytes = 0;
                               //   per call instead of one synchronous pageable copy per argument (a per-query caller pays each of them)
    // transient, set by fspann_tick_dev around a refine-only tick: device-resident RouteParams of the batch's hand-over buffer
    // (the streaming scan then finishes PENDING queries itself), the LDS its full select needs, and whether a launch took it
    const void* refine_fix_dev = nullptr;
    size_t refine_fix_lds = 0;
    bool refine_fix_used = false;

    std::atomic<int> comm_refs{0};      // fspann_comm objects that hold this context (it must outlive them)
    std::atomic<bool> destroy_deferred{false};   // fspann_ctx_destroy came while a communicator still held the context: the last fspann_comm_destroy finishes it
    // incremental Setup (fspann_build_begin / _append / _finish): codes of the rows appended so far stay in HBM
    int64_t bld_n = 0, bld_done = -1;    // bld_done < 0: no build in progress
    fspann::DevBuf bld_codes;
};

namespace fspann {

inline int ensure(fspann_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return FSPANN_OK;
    if (b.p) {
        FSP_HIP(hipStreamSynchronize(c->stream));
        FSP_HIP(hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
    }
    size_t want = bytes + bytes / 4 + 256;
    FSP_HIP(hipMalloc(&b.p, want));
    b.bytes = want;
    b.gen++;
    return FSPANN_OK;
}

// Launches that need more than the default 64 KB of dynamic LDS: hipFuncAttributeMaxDynamicSharedMemorySize of `kernel` is raised to
// `bytes` unless this context has already raised it that far (the attribute is a ceiling, not the launch size; a clone keeps its
// own record).  A few dozen kernels at most: a flat array scanned linearly, nothing allocated on the launch path.
template <class K> int raise_lds_ceiling(fspann_ctx* c, K kernel, size_t bytes) {
    const void* key = reinterpret_cast<const void*>(kernel);
    fspann_ctx::LdsCeiling* e = c->lds_ceilings;
    fspann_ctx::LdsCeiling* const end = e + c->n_lds_ceilings;
    while (e != end && e->kernel != key) e++;
    if (e != end && e->bytes >= bytes) return FSPANN_OK;
    FSP_HIP(hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)));
    if (e == end) {
        if (c->n_lds_ceilings == fspann_ctx::kLdsCeilings) return FSPANN_OK;     // (a full record: this kernel is raised at every launch)
        c->n_lds_ceilings++;
        e->kernel = key;
    }
    e->bytes = bytes;
    return FSPANN_OK;
}

// java.util.HashMap.tableSizeFor
inline int table_size_for(int cap) {
    uint32_t c = static_cast<uint32_t>(cap - 1);
    int nlz = (c == 0) ? 32 : __builtin_clz(c);
    int32_t n = static_cast<int32_t>(0xFFFFFFFFu >> (nlz & 31));
    if (n < 0) return 1;
    if (n >= (1 << 30)) return 1 << 30;
    return n + 1;
}

// String.hashCode of Long.toString(v) (ids are decimal ordinals, ForwardSecureANNSystem.java:515)
inline int32_t decimal_string_hash(int64_t v) {
    char buf[24];
    int n = snprintf(buf, sizeof(buf), "%lld", static_cast<long long>(v));
    uint32_t h = 0;
    for (int i = 0; i < n; i++) h = 31u * h + static_cast<unsigned char>(buf[i]);
    return static_cast<int32_t>(h);
}

}  // namespace fspann
