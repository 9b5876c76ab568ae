// api_refine.hip.h — Refine entry points: fspann_refine[_dev], the resident plaintext store, the one-call search, scan timing (QSI:238-316,364-372)
// Part of the single translation unit fspann_api.hip (included there, in order); product code, no CPU fallback.
#pragma once

namespace {

// Dims per tile, DC, as a constant for f.  One- and two-byte rows: a tile is 128 bytes (128 / 64 dims), FSPANN_REFINE_DC is an fp32 /
// fp64 notion and is ignored; FSPANN_F32 / FSPANN_F64 rows: 128 bytes unless FSPANN_REFINE_DC asks for twice or four times that.
template <typename TC, class F>
int with_tile_width(const fspann_ctx* c, F&& f) {
    constexpr int DC0 = 128 / static_cast<int>(sizeof(TC));
    if constexpr (sizeof(TC) >= 4) {
        if (c->knob_refine_dc == DC0 * 2) return f(std::integral_constant<int, DC0 * 2>{});
        if (c->knob_refine_dc == DC0 * 4) return f(std::integral_constant<int, DC0 * 4>{});
    }
    return f(std::integral_constant<int, DC0>{});
}

// How the scan of one launch runs (every Refine call, the list mode and the sweep's key scan): 16 bytes at a time or not, its LDS,
// and the one decision between the stream and one workgroup per (query, chunk).
struct ScanPlan {
    bool vec;
    size_t lds;
    int nchunks;
    unsigned grid;       // one workgroup per (query, chunk)
    int stream_wgs;      // workgroups per CU of the streaming scan: dense blocks run at 128 registers (4 per CU: a 1024-query batch is
                         // exactly one unit per workgroup on 256 CUs), the store gather at 3 per CU; FSPANN_REFINE_STREAM overrides, 0 = off
    int64_t slots;       // ... on the whole device
    bool stream;         // the scan runs as a stream (a kernel built for 128-byte tiles only)
    unsigned sgrid(int64_t units) const { return static_cast<unsigned>(std::min<int64_t>(units, slots)); }
};
template <typename TC, int DC, bool GATHER>
ScanPlan scan_plan(const fspann_ctx* c, int64_t nq, const TC* cand, int nchunks) {
    constexpr int VN = RowCodec<TC>::N;
    ScanPlan s{};
    s.vec = (c->cfg.dim % VN == 0) && ((reinterpret_cast<uintptr_t>(cand) & 15) == 0);
    s.lds = std::max<size_t>(static_cast<size_t>(kRefRows) * (s.vec ? DC + VN : DC + 1) * sizeof(TC), static_cast<size_t>(kRefRows) * 16);
    s.nchunks = nchunks;
    s.grid = static_cast<unsigned>(nq * nchunks);
    s.stream_wgs = (c->knob_refine_stream >= 0) ? std::min(c->knob_refine_stream, GATHER ? 3 : 4) : (GATHER ? 3 : 4);
    s.slots = static_cast<int64_t>(c->num_cus) * s.stream_wgs;
    s.stream = DC * sizeof(TC) == 128 && s.vec && s.stream_wgs > 0 && nq * nchunks < (int64_t(1) << 31);
    return s;
}

// One way to launch a scan or merge kernel of kRefRows threads.  may_time — the non-listed scan and stream dispatches, the hand-over
// and the running top-k among them; never a listed dispatch or a merge: start/stop events attached to this very dispatch when it
// is the rt_every-th one seen while scan timing is on and events are left (fspann_refine_timing_begin).
template <class K, class... A>
int launch_refine_kernel(fspann_ctx* c, bool may_time, K kern, unsigned grid, size_t lds, A... args) {
    if (may_time && c->rt_on && (c->rt_seen++ % c->rt_every) == 0 && c->rt_used + 2 <= c->rt_events.size()) {
        hipExtLaunchKernelGGL(kern, dim3(grid), dim3(kRefRows), lds, c->stream, c->rt_events[c->rt_used], c->rt_events[c->rt_used + 1], 0, args...);
        c->rt_used += 2;
    } else {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kRefRows), lds, c->stream, args...);
    }
    return FSPANN_OK;
}
// ... of a kernel whose launch can need more than the default 64 KB of LDS: its ceiling raised to `ceiling` first where that is beyond
// them (the stream kernels never do: a 128-byte tile plus its 16-byte pad over kRefRows rows is 36 KB)
template <class K, class... A>
int launch_refine_kernel_lds(fspann_ctx* c, bool may_time, K kern, unsigned grid, size_t lds, size_t ceiling, A... args) {
    if (ceiling > 64 * 1024) if (int rc = raise_lds_ceiling(c, kern, ceiling)) return rc;
    return launch_refine_kernel(c, may_time, kern, grid, lds, args...);
}

template <typename TC, typename TQ, int DC, bool GATHER>
int launch_refine_dc(fspann_ctx* c, const RefineJob& j) {
    constexpr bool kStreamTile = DC * sizeof(TC) == 128;
    // fp32 queries over rows of at most four bytes at the default tile width (128 bytes; no hand-over kernel reads FSPANN_F64 rows)
    constexpr bool kHandOver = DtypeOf<TQ>::id == FSPANN_F32 && sizeof(TC) <= 4 && kStreamTile;
    // qlist / qcount (device, the retry pass of fspann_search_retry_dev): only the queries qlist[0 .. *qcount) are scored, each at its
    // own index; the launches are sized for nq and their workgroups past the count leave at once.  One partial list per chunk
    // (no running top-k), no hand-over, no kernel-attached timing.
    const bool listed = j.qlist != nullptr;
    const int64_t nq = j.nq;
    const int k = j.k;
    const int nchunks = static_cast<int>((j.B + kRefRows - 1) / kRefRows);
    const ScanPlan sp = scan_plan<TC, DC, GATHER>(c, nq, static_cast<const TC*>(j.rows), nchunks);
    const size_t lds = sp.lds;
    RefinePartial* partial = nullptr;
    int32_t* pcnt = nullptr;
    // Long candidate lists (B in the thousands, k = 100: the reference's shipped profiles): a workgroup walks a RUN of consecutive
    // chunks of one query and keeps its best k in LDS (refine_topk_running) — one list per run instead of one per chunk.  With at
    // least half a grid of queries a run is the whole query (no merge kernel at all); fewer queries are cut into as many runs as
    // fill the grid (one query: one chunk per workgroup, as before).
    int npieces = 0, cpp = 0;
    if (!listed && !GATHER && nchunks > 1 && k > kRefFilterMaxK && k <= kRunMaxK && c->knob_refine_run && sp.stream) {
        int np = (nq * 2 >= sp.slots) ? 1 : static_cast<int>(std::min<int64_t>(nchunks, (sp.slots + nq - 1) / std::max<int64_t>(nq, 1)));
        cpp = (nchunks + np - 1) / np;
        npieces = (nchunks + cpp - 1) / cpp;
        if (nq * npieces >= (int64_t(1) << 31)) { npieces = 0; cpp = 0; }
    }
    const int nlists = npieces > 0 ? npieces : nchunks;      // partial lists per query (runs of chunks, or chunks)
    if (nlists > 1) {
        const size_t pb = static_cast<size_t>(nq) * nlists * k * sizeof(RefinePartial);
        const size_t cb = static_cast<size_t>(nq) * nlists * 2 * 4;
        int rc = ensure(c, c->ws_refine, pb + cb + 64);
        if (rc) return rc;
        partial = static_cast<RefinePartial*>(c->ws_refine.p);
        pcnt = reinterpret_cast<int32_t*>(static_cast<char*>(c->ws_refine.p) + ((pb + 15) & ~size_t(15)));
    }
    const RefineArgs<TC, TQ> ra{static_cast<const TQ*>(j.q), static_cast<const TC*>(j.rows), GATHER ? c->store->n : 0, j.B, c->cfg.dim, j.cand_ids, j.cand_count, k, nchunks,
                                j.out_ids, j.out_dist, j.out_count, j.scored, partial, pcnt, npieces, cpp, c->dbg_route};
    // The kernel of this scan.  As a stream: stream_wgs workgroups per CU, each walking several (query, chunk) units with the loads
    // of the next tile in flight across unit boundaries (refine_stream_run); else one workgroup per (query, chunk).  Hand-over: the
    // batch's Route ran with a hand-over buffer, the scan's workgroups finish its PENDING queries first (tick.hip.h).
    enum class Scan { ListStream, ListChunks, HandOver, Runs, Stream, Chunks };
    const bool stream = kStreamTile && sp.stream;
    const Scan scan = listed ? (stream ? Scan::ListStream : Scan::ListChunks)
                      : !stream ? Scan::Chunks
                      : (kHandOver && c->refine_fix_dev && nchunks == 1) ? Scan::HandOver
                      : npieces > 0 ? Scan::Runs : Scan::Stream;
    const unsigned sgrid = sp.sgrid(nq * nlists);
    int rc = FSPANN_OK;
    if (scan == Scan::ListStream) {
        if constexpr (kStreamTile) rc = launch_refine_kernel(c, false, refine_stream_list_kernel<TC, TQ, DC, GATHER>, sgrid, lds, ra, j.qlist, j.qcount);
    } else if (scan == Scan::ListChunks) {
        rc = sp.vec ? launch_refine_kernel_lds(c, false, refine_scan_list_kernel<TC, TQ, DC, true, GATHER>, sp.grid, lds, lds, ra, j.qlist, j.qcount)
                    : launch_refine_kernel_lds(c, false, refine_scan_list_kernel<TC, TQ, DC, false, GATHER>, sp.grid, lds, lds, ra, j.qlist, j.qcount);
    } else if (scan == Scan::HandOver) {
        if constexpr (kHandOver) {
            rc = launch_refine_kernel_lds(c, true, refine_stream_fix_kernel<TC, GATHER>, sgrid, std::max(lds, c->refine_fix_lds), 159 * 1024, ra, nq,
                                          static_cast<const RouteParams*>(c->refine_fix_dev));
            if (!rc) c->refine_fix_used = true;
        }
    } else if (scan == Scan::Runs) {
        if constexpr (kStreamTile && !GATHER) rc = launch_refine_kernel(c, true, refine_stream_kernel<TC, TQ, DC, false, true>, sgrid, lds, ra, nq);
    } else if (scan == Scan::Stream) {
        if constexpr (kStreamTile) rc = launch_refine_kernel(c, true, refine_stream_kernel<TC, TQ, DC, GATHER>, sgrid, lds, ra, nq);
    } else {
        rc = sp.vec ? launch_refine_kernel_lds(c, true, refine_scan_kernel<TC, TQ, DC, true, GATHER>, sp.grid, lds, lds, ra)
                    : launch_refine_kernel_lds(c, true, refine_scan_kernel<TC, TQ, DC, false, GATHER>, sp.grid, lds, lds, ra);
    }
    if (rc) return rc;
    FSP_HIP(hipGetLastError());
    if (npieces > 0 && !stream) return fail(FSPANN_E_STATE, "refine: the running top-k was planned but the streaming scan did not run");
    if (nlists > 1) {
        // the merge of a query's partial lists (one per run, or per chunk), all their keys in LDS when they fit (two workgroups per CU
        // at least); over the listed queries when there is a list
        const size_t mlds = static_cast<size_t>(nlists) * k * 8 + static_cast<size_t>(nlists) * 4 + 16;
        const bool in_lds = mlds <= 72 * 1024;
        auto merge = [&](auto mk, auto... list) {
            return launch_refine_kernel_lds(c, false, mk, static_cast<unsigned>(nq), in_lds ? mlds : static_cast<size_t>(nlists) * 4 + 16, in_lds ? 72 * 1024 : 0, partial, pcnt,
                                            nlists, k, j.out_ids, j.out_dist, j.out_count, j.scored, list...);
        };
        if (listed) rc = in_lds ? merge(refine_merge_list_kernel<true>, j.qlist, j.qcount) : merge(refine_merge_list_kernel<false>, j.qlist, j.qcount);
        else rc = in_lds ? merge(refine_merge_kernel<true>) : merge(refine_merge_kernel<false>);
        if (rc) return rc;
        FSP_HIP(hipGetLastError());
    }
    return FSPANN_OK;
}

// The one way from a job to its scan: (query dtype, row dtype, gather or dense) -> the tile width -> the launch, and the
// touched-record set (api_touch.hip.h) behind it: the rows this launch scores (nothing while tracking is off).
int refine_run(fspann_ctx* c, const RefineJob& j) {
    return with_refine_types(j.q_dtype, j.row_dtype, [&](auto tq, auto tc) -> int {
        using TQ = typename decltype(tq)::type;
        using TC = typename decltype(tc)::type;
        auto run = [&](auto gather) -> int {
            constexpr bool GATHER = decltype(gather)::value;
            int rc = with_tile_width<TC>(c, [&](auto dc) { return launch_refine_dc<TC, TQ, decltype(dc)::value, GATHER>(c, j); });
            return rc ? rc : touch_mark<TC, TQ, GATHER>(c, j);
        };
        return j.gather ? run(std::true_type{}) : run(std::false_type{});
    });
}

// The argument checks of the four Refine calls (ok: every buffer the call needs is there); the caller returns on rc or nq == 0.
int check_refine_args(int64_t nq, int64_t B, int k, bool ok) {
    if (nq < 0 || B <= 0) return fail(FSPANN_E_ARG, "nq < 0 or B <= 0");
    if (k <= 0) return fail(FSPANN_E_ARG, "topK must be > 0");  // QueryTokenFactory.java:65
    if (nq > 0 && !ok) return fail(FSPANN_E_NULL, "refine buffer is null");
    return FSPANN_OK;
}

// fspann_refine / fspann_refine_store behind their checks: j holds the caller's HOST pointers (gather: no rows); staged, then the
// _dev twin over the device addresses, then every output handed back.
// Small calls: query, ids and counts go up in ONE pinned block and every output comes down in one (the candidate rows keep
// their own copy straight from the caller's buffer): three transfers and one synchronisation instead of eight and one.  A handful
// of queries: query, ids and counts are read from the mapped pinned block and the results written into it by the kernel itself.
int refine_staged(fspann_ctx* c, const RefineJob& j, StagePolicy policy) {
    const size_t nq = static_cast<size_t>(j.nq), d = c->cfg.dim, nb = nq * 4, ob_i = nq * j.k * 4, ob_d = nq * j.k * 8;
    RefineIo io(j.q, nq * d * dtype_size(j.q_dtype), j.rows, j.gather ? 0 : nq * j.B * d * dtype_size(j.row_dtype), j.cand_ids, nq * j.B * 4, j.cand_count, nb, ob_d, ob_i);
    io.choose(c, j.nq, policy);
    io.outputs(j.out_ids, ob_i, j.out_dist, ob_d, j.out_count, j.scored, nb);
    int rc;
    if ((rc = io.begin(c)) || (rc = io.send(c))) return rc;
    const void* q_d = io.dev_up<void>(c, RefineIo::Q);
    const int32_t *ids_d = io.dev_up<int32_t>(c, RefineIo::CandIds), *cnt_d = io.dev_up<int32_t>(c, RefineIo::CandCount);
    int32_t *oi = io.dev_down<int32_t>(c, RefineIo::Ids), *oc = io.dev_down<int32_t>(c, RefineIo::Counts);
    double* od = io.dev_down<double>(c, RefineIo::Dist);
    rc = j.gather ? fspann_refine_store_dev(c, j.nq, q_d, j.q_dtype, j.B, ids_d, cnt_d, j.k, oi, od, oc, oc + nq)
                  : fspann_refine_dev(c, j.nq, q_d, j.q_dtype, io.dev_up<void>(c, RefineIo::Rows), j.row_dtype, j.B, ids_d, cnt_d, j.k, oi, od, oc, oc + nq);
    if (rc || (rc = io.fetch(c))) return rc;
    FSP_HIP(hipStreamSynchronize(c->stream));
    io.unpack(c);
    return FSPANN_OK;
}

}  // namespace

extern "C" {

// ---- refine ---------------------------------------------------------------------------
int fspann_refine_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, const void* cand_dev, int cand_dtype,
                      int64_t B, const int32_t* cand_ids_dev, const int32_t* cand_count_dev, int k, int32_t* out_ids_dev,
                      double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev) {
    CHECK_CTX(c);
    int rc = check_refine_args(nq, B, k, q_dev && cand_dev && cand_ids_dev && cand_count_dev && out_ids_dev && out_dist_dev && out_count_dev);
    if (rc || nq == 0) return rc;
    return refine_run(c, {q_dev, q_dtype, cand_dev, cand_dtype, false, nq, B, cand_ids_dev, cand_count_dev, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev});
}

int fspann_refine(fspann_ctx* c, int64_t nq, const void* q, const void* cand, int dtype, int64_t B,
                  const int32_t* cand_ids, const int32_t* cand_count, int k, int32_t* out_ids, double* out_dist,
                  int32_t* out_count, int32_t* scored) {
    CHECK_CTX(c);
    int rc = check_refine_args(nq, B, k, q && cand && cand_ids && cand_count && out_ids && out_dist && out_count);
    if (rc || nq == 0) return rc;
    if (const DtypeInfo* di = dtype_info(dtype); di && di->rows_noun)
        return fail(FSPANN_E_ARG, "dtype %s: fspann_refine has one dtype for query and rows, and a query is FSPANN_F32 or FSPANN_F64 (%s: fspann_refine_dev)", di->name, di->rows_noun);
    if (!is_query_dtype(dtype)) return fail(FSPANN_E_ARG, "unknown dtype %d", dtype);
    return refine_staged(c, {q, dtype, cand, dtype, false, nq, B, cand_ids, cand_count, k, out_ids, out_dist, out_count, scored}, RefineIo::policy);
}

void* fspann_host_buffer(fspann_ctx* c, size_t bytes) {
    if (!c) { fail(FSPANN_E_NULL, "ctx is null"); return nullptr; }
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) { (void)hipGetLastError(); fail(FSPANN_E_DEVICE, "hipSetDevice(%d) failed", c->device); return nullptr; }
    if (bytes == 0) bytes = 16;
    if (bytes > c->h_rows_bytes) {
        if (hipStreamSynchronize(c->stream) != hipSuccess) (void)hipGetLastError();      // nothing in flight may still read the old block
        c->h_rows.reset(); c->h_rows_bytes = 0;
        const size_t want = (bytes + 4095) & ~size_t(4095);
        void* block = nullptr;
        if (hipHostMalloc(&block, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            fail(FSPANN_E_NOMEM, "cannot pin %zu bytes of host memory", want);
            return nullptr;
        }
        c->h_rows.reset(block);
        c->h_rows_bytes = want;
    }
    return c->h_rows.get();
}

// ---- plaintext store (test / bench harness) ----------------------------------------------
// A fresh, empty RowStore in place of the one c refers to, the stream drained first: nothing in flight reads the old rows when the
// last reference to them goes, and a context never holds two stores of its own in HBM.
static int store_renew(fspann_ctx* c) {
    FSP_HIP(hipStreamSynchronize(c->stream));
    return guarded([&]() -> int {
        auto s = std::make_shared<RowStore>();
        s->gen = c->store->gen + 1;
        c->store = std::move(s);
        return FSPANN_OK;
    });
}

// (a clone lets go of its source's rows and refers to its own from here on; an owner may not replace rows that clones read)
int fspann_store_set(fspann_ctx* c, int64_t n, const void* vectors, int dtype) {
    CHECK_CTX(c);
    if (!c->is_clone && !may_change_shared(c)) return refuse_shared(c, "store");
    if (!vectors) return fail(FSPANN_E_NULL, "vectors is null");
    if (n <= 0) return fail(FSPANN_E_ARG, "n <= 0");
    if (!is_row_dtype(dtype)) return fail(FSPANN_E_ARG, "unknown dtype %d", dtype);
    const size_t bytes = static_cast<size_t>(n) * c->cfg.dim * dtype_size(dtype);
    if (int rc = store_renew(c)) return rc;
    RowStore& s = *c->store;
    FSP_HIP(hipMalloc(&s.rows, bytes));
    s.owned = true;
    FSP_HIP(hipMemcpy(s.rows, vectors, bytes, hipMemcpyHostToDevice));
    s.dtype = dtype;
    s.n = n;
    return FSPANN_OK;
}

// The same store over rows that already live in HBM (caller-owned, e.g. a tensor): no copy; the caller keeps the
// memory alive and unchanged while the context refers to it (until the next store_set / store_attach / ctx_destroy).
int fspann_store_attach_dev(fspann_ctx* c, int64_t n, const void* vectors_dev, int dtype) {
    CHECK_CTX(c);
    if (!c->is_clone && !may_change_shared(c)) return refuse_shared(c, "store");
    if (!vectors_dev) return fail(FSPANN_E_NULL, "vectors is null");
    if (n <= 0) return fail(FSPANN_E_ARG, "n <= 0");
    if (!is_row_dtype(dtype)) return fail(FSPANN_E_ARG, "unknown dtype %d", dtype);
    if (reinterpret_cast<uintptr_t>(vectors_dev) & 15) return fail(FSPANN_E_ARG, "store rows must be 16-byte aligned");
    if (int rc = store_renew(c)) return rc;
    RowStore& s = *c->store;
    s.rows = const_cast<void*>(vectors_dev);
    s.dtype = dtype;
    s.n = n;
    return FSPANN_OK;
}

// Refine straight from the resident store: row j of query qi is store[cand_ids[qi*B + j]].  Same kernel as
// fspann_refine_dev with the row address taken from the id (no [nq][B][dim] staging copy).
int fspann_refine_store_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int64_t B,
                            const int32_t* cand_ids_dev, const int32_t* cand_count_dev, int k, int32_t* out_ids_dev,
                            double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev) {
    CHECK_CTX(c);
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    int rc = check_refine_args(nq, B, k, q_dev && cand_ids_dev && cand_count_dev && out_ids_dev && out_dist_dev && out_count_dev);
    if (rc || nq == 0) return rc;
    return refine_run(c, store_job(c, q_dev, q_dtype, nq, B, cand_ids_dev, cand_count_dev, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev));
}

// (no pinned or mapped transport: one copy command per argument)
int fspann_refine_store(fspann_ctx* c, int64_t nq, const void* q, int q_dtype, int64_t B, const int32_t* cand_ids,
                        const int32_t* cand_count, int k, int32_t* out_ids, double* out_dist, int32_t* out_count,
                        int32_t* scored) {
    CHECK_CTX(c);
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    int rc = check_refine_args(nq, B, k, q && cand_ids && cand_count && out_ids && out_dist && out_count);
    if (rc || nq == 0) return rc;
    if ((rc = refuse_row_only(q_dtype, "q_dtype"))) return rc;
    if (!is_query_dtype(q_dtype)) return fail(FSPANN_E_ARG, "q_dtype %d: a query is FSPANN_F32 or FSPANN_F64", q_dtype);
    return refine_staged(c, {q, q_dtype, nullptr, c->store->dtype, true, nq, B, cand_ids, cand_count, k, out_ids, out_dist, out_count, scored}, RefineIo::store_policy);
}

// QueryServiceImpl.search for a batch, all three stages in stream order with one call: TokenGen codes (encode),
// Route with limit = B (stage A.5; counters not produced, so the bounded select may run), Refine from the resident store.
// The adaptive retry (QSI:327-337) stays with the caller: out_count / scored tell it when to call again with
// probe_override = 10.  sel_ids_dev / sel_count_dev (optional) receive F_q.
int fspann_search_store_dev(fspann_ctx* c, int64_t nq, const void* q_dev, int q_dtype, int probe_override, int64_t B, int k,
                            int32_t* out_ids_dev, double* out_dist_dev, int32_t* out_count_dev, int32_t* scored_dev,
                            int32_t* sel_ids_dev, int32_t* sel_count_dev, int32_t* bad_dev) {
    CHECK_CTX(c);
    if (!c->frozen) return fail(FSPANN_E_STATE, "Index not finalized");
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    if (nq < 0 || B <= 0 || B > INT32_MAX) return fail(FSPANN_E_ARG, "nq < 0 or B out of range");
    if (k <= 0) return fail(FSPANN_E_ARG, "topK must be > 0");
    if (nq == 0) return FSPANN_OK;
    int rc;
    SearchArea sa;
    if ((rc = search_area_grow(c, nq, B, sel_ids_dev, sel_count_dev, bad_dev, sa))) return rc;
    uint64_t* codes = const_cast<uint64_t*>(sa.codes);
    int32_t* sel = sa.sel;
    int32_t* cnt = sa.cnt;
    int32_t* bad = sa.bad;
    if ((rc = fspann_encode_dev(c, nq, q_dev, q_dtype, codes, nullptr, bad))) return rc;
    if ((rc = fspann_route_dev(c, nq, codes, probe_override, static_cast<int32_t>(B), B, sel, nullptr, cnt, nullptr, nullptr))) return rc;
    return fspann_refine_store_dev(c, nq, q_dev, q_dtype, B, sel, cnt, k, out_ids_dev, out_dist_dev, out_count_dev, scored_dev);
}

const void* fspann_store_dev_ptr(fspann_ctx* c, int* dtype) {
    if (!c) return nullptr;
    if (dtype) *dtype = c->store->dtype;
    return c->store->rows;
}

int fspann_store_gather_dev(fspann_ctx* c, int64_t nq, const int32_t* sel_ids_dev, const int32_t* sel_count_dev, int64_t B,
                            void* cand_dev) {
    CHECK_CTX(c);
    if (!c->store->rows) return fail(FSPANN_E_STATE, "plaintext store not set");
    if (!sel_ids_dev || !sel_count_dev || !cand_dev) return fail(FSPANN_E_NULL, "gather buffer is null");
    if (nq <= 0 || B <= 0) return FSPANN_OK;
    const int d = c->cfg.dim;
    const int64_t rows = nq * B;
    const unsigned grid = static_cast<unsigned>((rows + 7) / 8);
    with_row_type(c->store->dtype, [&](auto tc) {      // (a store has a row dtype: fspann_store_set / _attach_dev)
        using T = typename decltype(tc)::type;
        const int vec_ok = (d % RowCodec<T>::N == 0) && ((reinterpret_cast<uintptr_t>(cand_dev) & 15) == 0);
        hipLaunchKernelGGL(store_gather_kernel<T>, dim3(grid), dim3(256), 0, c->stream, static_cast<const T*>(c->store->rows), d, sel_ids_dev, sel_count_dev, B, nq,
                           static_cast<T*>(cand_dev), vec_ok);
    });
    FSP_HIP(hipGetLastError());
    return FSPANN_OK;
}

// Kernel-attached timing of the refinement scan: between _begin and _end every refine_scan_kernel dispatch of this
// context carries its own start/stop HIP events (hipExtLaunchKernel), i.e. the duration of the kernel itself on the
// context's stream — what a rocprofv3 kernel trace reports — without the gaps a record-before / record-after bracket adds.
// A dispatch with attached events costs a few microseconds of extra stream time, hence `every`: only every n-th one is timed.
int fspann_refine_timing_begin(fspann_ctx* c, int max_launches, int every) {
    CHECK_CTX(c);
    if (max_launches <= 0 || every <= 0) return fail(FSPANN_E_ARG, "max_launches <= 0 or every <= 0");
    c->rt_every = every;
    c->rt_seen = 0;
    while (c->rt_events.size() < static_cast<size_t>(max_launches) * 2) {
        hipEvent_t e;
        FSP_HIP(hipEventCreate(&e));
        c->rt_events.push_back(e);
    }
    c->rt_used = 0;
    c->rt_on = true;
    return FSPANN_OK;
}
int fspann_refine_timing_end(fspann_ctx* c, int* launches, double* total_ms) {
    CHECK_CTX(c);
    c->rt_on = false;
    FSP_HIP(hipStreamSynchronize(c->stream));
    double tot = 0.0;
    for (size_t i = 0; i + 1 < c->rt_used; i += 2) {
        float ms = 0.f;
        FSP_HIP(hipEventElapsedTime(&ms, c->rt_events[i], c->rt_events[i + 1]));
        tot += ms;
    }
    if (launches) *launches = static_cast<int>(c->rt_used / 2);
    if (total_ms) *total_ms = tot;
    c->rt_used = 0;
    return FSPANN_OK;
}

}  // extern "C"
