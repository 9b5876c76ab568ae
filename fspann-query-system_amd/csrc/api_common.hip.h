// api_common.hip.h — helpers shared by every entry point of include/fspann.h: sizes, guarded(), the context checks, the work areas
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once

using namespace fspann;

namespace {

int next_pow2(int64_t v) {
    int64_t p = 1;
    while (p < v) p <<= 1;
    return static_cast<int>(p);
}

int effective_probes(const fspann_ctx* c, int override_) {  // PIS:880-888
    if (override_ > 0) return override_;
    if (c->cfg.probe_override > 0) return c->cfg.probe_override;
    return c->cfg.default_probes;
}

int java_final_cap_host(int cap0, int64_t n) {
    int cap = cap0;
    int64_t thr = static_cast<int64_t>(static_cast<float>(cap) * 0.75f);
    while (n > thr && cap < (1 << 30)) {
        const int oldCap = cap;
        cap <<= 1;
        thr = (oldCap >= 16) ? (thr << 1) : static_cast<int64_t>(static_cast<float>(cap) * 0.75f);
    }
    return cap;
}

int resolve_unmodelled(fspann_ctx* c, int64_t nq, const uint64_t* codes_dev, int probe_override, int32_t limit, int64_t cap, int32_t* ids_dev,
                       int32_t* score_dev, int32_t* count_dev, int32_t* kept_dev, int32_t* raw_dev, int64_t* resolved_out, int64_t* left_out);   // api_ext.hip.h

// No C++ exception crosses the C ABI (include/fspann.h): every entry point that allocates host memory or starts
// threads runs its body through guarded(); worker threads catch on their own and report through a flag.
template <class F> int guarded(F&& f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(FSPANN_E_NOMEM, "out of host memory");
    } catch (const std::exception& e) {
        return fail(FSPANN_E_ARG, "C++ exception: %s", e.what());
    } catch (...) {
        return fail(FSPANN_E_ARG, "unknown C++ exception");
    }
}

#define CHECK_CTX_NOLOCK(c)                                               \
    do {                                                                  \
        if (!(c)) return fail(FSPANN_E_NULL, "ctx is null");              \
        hipError_t _e = hipSetDevice((c)->device);                        \
        if (_e != hipSuccess) return fail(FSPANN_E_DEVICE, "hipSetDevice(%d): %s", (c)->device, hipGetErrorString(_e)); \
    } while (0)
// ... and the context's lock for the rest of the entry point (calls on one context are serialised inside the library)
#define CHECK_CTX(c)         \
    CHECK_CTX_NOLOCK(c);     \
    std::lock_guard<std::recursive_mutex> _ctx_lock((c)->mu)

// State shared through fspann_ctx_clone is read-only: a clone cannot change it, its owner cannot while clones are alive.
inline bool may_change_shared(const fspann_ctx* c) { return !c->is_clone && c->fam->clones.load() == 0; }
// ... and the refusal of a call that would change `what` ("index", "store", "touched set")
inline int refuse_shared(const fspann_ctx* c, const char* what) {
    if (c->is_clone) return fail(FSPANN_E_STATE, "a clone reads its parent's %s: it cannot be changed here", what);
    return fail(FSPANN_E_STATE, "the %s is shared with %d clone(s): destroy them first", what, c->fam->clones.load());
}
#define CHECK_UNSHARED(c) do { if (!may_change_shared(c)) return refuse_shared(c, "index"); } while (0)

// One Refine job on the device: what the entry point or internal caller builds once and every layer down to the launch and the
// touched-record mark reads.  gather: the rows are the resident store's, row j of query qi is rows[cand_ids[qi * B + j]]; else
// dense blocks [nq][B][dim].  qlist / qcount (device, optional): over the queries qlist[0 .. *qcount) only, each at its own index.
struct RefineJob {
    const void* q; int q_dtype;
    const void* rows; int row_dtype; bool gather;
    int64_t nq, B;
    const int32_t *cand_ids, *cand_count;
    int k;
    int32_t* out_ids; double* out_dist; int32_t *out_count, *scored;
    const int32_t *qlist = nullptr, *qcount = nullptr;
};
// ... over the context's resident store
RefineJob store_job(const fspann_ctx* c, const void* q, int q_dtype, int64_t nq, int64_t B, const int32_t* cand_ids, const int32_t* cand_count, int k, int32_t* out_ids,
                    double* out_dist, int32_t* out_count, int32_t* scored, const int32_t* qlist = nullptr, const int32_t* qcount = nullptr) {
    return {q, q_dtype, c->store->rows, c->store->dtype, true, nq, B, cand_ids, cand_count, k, out_ids, out_dist, out_count, scored, qlist, qcount};
}

// The one dispatch over (query dtype, row dtype) of a scan: f(query type tag, row type tag) -> int, or the refusal.
template <class F> int with_refine_types(int q_dtype, int row_dtype, F&& f) {
    int rc = FSPANN_OK;
    bool launched = false;
    with_query_type(q_dtype, [&](auto tq) { launched = with_row_type(row_dtype, [&](auto tc) { rc = f(tq, tc); }); });
    if (launched) return rc;
    if ((rc = refuse_row_only(q_dtype, "q_dtype"))) return rc;
    if (!is_query_dtype(q_dtype)) return fail(FSPANN_E_ARG, "q_dtype %d: a query is FSPANN_F32 or FSPANN_F64", q_dtype);
    return fail(FSPANN_E_ARG, "unknown dtype");
}

// Work areas.  A Carver hands out 256-byte-rounded pieces of a buffer in order; over a null base it only adds up the size.  An area
// is a struct of pointers with ONE description of its layout, lay(base, dims...), which carves its pieces and returns its size.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base(static_cast<char*>(b)) {}
    template <typename T> T* take(size_t bytes) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (bytes + 255) & ~size_t(255);
        return p;
    }
};
// The area in buffer b, grown to the area's size first ...
template <class A, class... D> int area_grow(fspann_ctx* c, DevBuf& b, A& a, D... dims) {
    if (int rc = ensure(c, b, a.lay(nullptr, dims...))) return rc;
    a.lay(b.p, dims...);
    return FSPANN_OK;
}
// ... or as a call of this size left it; false when none precedes.
template <class A, class... D> bool area_held(const DevBuf& b, A& a, D... dims) {
    if (!b.p || b.bytes < a.lay(nullptr, dims...)) return false;
    a.lay(b.p, dims...);
    return true;
}

// The work area of fspann_search_store_dev (codes | F_q ids | counts | bad), shared with the calls that complete or extend it
// (fspann_search_store_finish_dev, the retry, fallback and sweep calls).
struct SearchArea {
    const uint64_t* codes;
    int32_t* sel;
    int32_t* cnt;
    int32_t* bad;
    size_t lay(void* base, const fspann_ctx* c, int64_t nq, int64_t B) {
        Carver w(base);
        codes = w.take<uint64_t>(static_cast<size_t>(nq) * c->TD * c->W * 8);
        sel = w.take<int32_t>(static_cast<size_t>(nq) * B * 4);
        cnt = w.take<int32_t>(static_cast<size_t>(nq) * 4);
        bad = w.take<int32_t>(static_cast<size_t>(nq) * 4);
        return w.off;
    }
    void prefer(int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev) {     // the caller's buffers where it passed them
        if (sel_ids_dev) sel = sel_ids_dev;
        if (sel_count_dev) cnt = sel_count_dev;
        if (bad_dev) bad = bad_dev;
    }
};
int search_area_grow(fspann_ctx* c, int64_t nq, int64_t B, int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, SearchArea& s) {
    if (int rc = area_grow(c, c->ws_search, s, c, nq, B)) return rc;
    s.prefer(sel_ids_dev, sel_count_dev, bad_dev);
    return FSPANN_OK;
}
bool search_area(fspann_ctx* c, int64_t nq, int64_t B, int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev, SearchArea& s) {
    if (!area_held(c->ws_search, s, c, nq, B)) return false;
    s.prefer(sel_ids_dev, sel_count_dev, bad_dev);
    return true;
}

}  // namespace
