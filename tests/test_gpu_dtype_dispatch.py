"""GPU: the way from a dtype given at run time to the code that runs, over the C ABI itself (ctypes, no package-side checks).

1. The refusal matrix: every entry point that takes a dtype, with every dtype id of DTYPES (pairs where there are two), on one tiny
   context.  A valid value returns FSPANN_OK; every other value returns FSPANN_E_ARG and the WHOLE fspann_last_error() string
   written out below (the strings are the library's contract with its callers: they are not derived from the library).
2. Which template ran: the same bytes mean different numbers as FSPANN_U8 / _I8 / _F8E4M3 (and the same 16-bit patterns as
   FSPANN_F16 / _BF16), so a branch that pairs a dtype with another type's kernel returns other neighbours.  Every row type is
   refined against fp32 and fp64 queries through fspann_refine_dev, fspann_refine_store_dev and the retry's listed pass, and
   ids, fp64 distances, counts and scored must EQUAL numpy's fp64 over the test's own decoding of the bytes.  All values are
   chosen so that every difference, square and sum is exact in fp64 (_rows), so the order of the sum does not matter and nothing
   has a tolerance.  The gathered rows must be the store's bytes, and the index built from typed rows the F32 build's."""
import ctypes as C
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, E_ARG = 0, -2
F32, F64, U8, F16, BF16, F8, I8 = range(7)
DTYPES = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 77)
NAMES = {0: "FSPANN_F32", 1: "FSPANN_F64", 2: "FSPANN_U8", 3: "FSPANN_F16", 4: "FSPANN_BF16", 5: "FSPANN_F8E4M3", 6: "FSPANN_I8"}
ROW_ONLY = {
    3: "%s FSPANN_F16: half precision is a row dtype only (store, refine rows, Setup input, metrics base); this one is FSPANN_F32 or FSPANN_F64",
    4: "%s FSPANN_BF16: bfloat16 is a row dtype only (store, refine rows, Setup input, metrics base); this one is FSPANN_F32 or FSPANN_F64",
    5: "%s FSPANN_F8E4M3: fp8 e4m3fn is a row dtype only (store, refine rows, Setup input, metrics base); this one is FSPANN_F32 or FSPANN_F64",
    6: "%s FSPANN_I8: signed int8 is a row dtype only (store, refine rows, Setup input, metrics and ground truth over int8 pairs); this one is FSPANN_F32 or FSPANN_F64",
}
REFINE_ONE_DTYPE = {
    2: "dtype FSPANN_U8: fspann_refine has one dtype for query and rows, and a query is FSPANN_F32 or FSPANN_F64 (byte rows: fspann_refine_dev)",
    3: "dtype FSPANN_F16: fspann_refine has one dtype for query and rows, and a query is FSPANN_F32 or FSPANN_F64 (half rows: fspann_refine_dev)",
    4: "dtype FSPANN_BF16: fspann_refine has one dtype for query and rows, and a query is FSPANN_F32 or FSPANN_F64 (bfloat16 rows: fspann_refine_dev)",
    5: "dtype FSPANN_F8E4M3: fspann_refine has one dtype for query and rows, and a query is FSPANN_F32 or FSPANN_F64 (fp8 rows: fspann_refine_dev)",
    6: "dtype FSPANN_I8: fspann_refine has one dtype for query and rows, and a query is FSPANN_F32 or FSPANN_F64 (signed byte rows: fspann_refine_dev)",
}


def _name(t):
    return NAMES.get(t, "unknown dtype")


# ---- what each entry point answers: (return code, message) ------------------------------------------------------------------------
def want_query(t, what="dtype"):
    """an entry point with one query dtype, named `what` in its refusals"""
    if t in (F32, F64):
        return OK, None
    if t in ROW_ONLY:
        return E_ARG, ROW_ONLY[t] % what
    return E_ARG, "unknown dtype %d" % t


def want_store_query(t):
    """fspann_refine_store / _store_dev: the store has a row dtype, q_dtype is the caller's"""
    if t in (F32, F64):
        return OK, None
    if t in ROW_ONLY:
        return E_ARG, ROW_ONLY[t] % "q_dtype"
    return E_ARG, "q_dtype %d: a query is FSPANN_F32 or FSPANN_F64" % t


def want_refine_dev(q, rows):
    if q in (F32, F64) and rows in NAMES:
        return OK, None
    if q in (F32, F64):
        return E_ARG, "unknown dtype"
    return want_store_query(q)


def want_refine(t):
    if t in (F32, F64):
        return OK, None
    if t in REFINE_ONE_DTYPE:
        return E_ARG, REFINE_ONE_DTYPE[t]
    return E_ARG, "unknown dtype %d" % t


def want_finish(t):
    """fspann_search_store_finish_dev / fspann_search_retry_finish_dev behind a call that left no query to finish: the row-only
    dtypes are refused by name, nothing else looks at q_dtype"""
    if t in ROW_ONLY:
        return E_ARG, ROW_ONLY[t] % "q_dtype"
    return OK, None


def want_rows(t):
    if t in NAMES:
        return OK, None
    return E_ARG, "unknown dtype %d" % t


def want_gt_typed(b, q):
    for t in (F16, BF16, F8):
        if t in (b, q):
            return E_ARG, "no ground truth over %s (base and query are both FSPANN_F32 or both FSPANN_U8): base %s, query %s" % (NAMES[t], _name(b), _name(q))
    if b != q or b not in (F32, U8, I8):
        return E_ARG, "Base and query types must match (both fvecs or both bvecs): base %s, query %s" % (_name(b), _name(q))
    return OK, None


def want_gt_rows(b):
    if b in (F32, U8, I8, F16, BF16, F8):
        return OK, None
    return E_ARG, ("ground truth rows are FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3 (the reference's ground truth reads floats): "
                   "base %s (%d)" % (_name(b), b))


def want_metrics_typed(b, q):
    tail = ": base %s, query %s" % (_name(b), _name(q))
    for t in (F16, BF16, F8):
        if t in (b, q) and not (b == t and q == F32):
            return E_ARG, "metrics take %s rows with FSPANN_F32 queries only (a query is never %s)" % (NAMES[t], NAMES[t]) + tail
    if I8 in (b, q) and not (b == I8 and q in (I8, F32)):
        return E_ARG, "metrics take FSPANN_I8 rows with FSPANN_I8 / FSPANN_F32 queries only (a signed byte pairs with nothing else)" + tail
    if (b, q) in ((F32, F32), (U8, U8), (U8, F32), (I8, I8), (I8, F32), (F16, F32), (BF16, F32), (F8, F32)):
        return OK, None
    return E_ARG, "metrics take FSPANN_F32 rows with FSPANN_F32 queries, or FSPANN_U8 rows with FSPANN_U8 / FSPANN_F32 queries" + tail


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _check(L, what, rc, want):
    err = (L.fspann_last_error() or b"").decode()
    if want[0] == OK:
        assert rc == OK, (what, rc, err)
    else:
        assert (rc, err) == want, (what, rc, err, want)


def test_refusal_matrix(pkg):
    import torch
    L = pkg._native.lib()
    d, n, nq, B, k = 16, 4, 2, 4, 2
    rng = np.random.default_rng(5)
    X = rng.integers(-8, 9, (n, d)).astype(np.float32)
    cfg = pkg.PaperRuntimeConfig(tables=2, divisions=1, m=4, lambda_=2, dim=d, refinement_limit=B, block_size=2, default_probes=1)
    # zeros are a finite value of every dtype: one zeroed block serves as queries, rows and ground-truth base of every type
    Zh = np.zeros(4096, np.uint8)
    Zd = _dev(Zh)
    z = Zd.data_ptr()
    ids_h = np.tile(np.arange(B, dtype=np.int32), (nq, 1))
    cnt_h = np.full(nq, B, np.int32)
    ids_d, cnt_d = _dev(ids_h), _dev(cnt_h)
    dev = torch.device("cuda", 0)
    o_ids = torch.zeros((nq, B), dtype=torch.int32, device=dev)
    o_dist = torch.zeros((nq, B), dtype=torch.float64, device=dev)
    o_cnt, o_sc, o_bad, o_ret, o_selc = (torch.zeros(nq, dtype=torch.int32, device=dev) for _ in range(5))
    o_sel = torch.zeros((nq, B), dtype=torch.int32, device=dev)
    o_codes = torch.zeros(nq * 64, dtype=torch.int64, device=dev)
    o_f64 = torch.zeros((2, nq), dtype=torch.float64, device=dev)
    h_ids, h_dist, h_cnt, h_sc = np.zeros((nq, k), np.int32), np.zeros((nq, k), np.float64), np.zeros(nq, np.int32), np.zeros(nq, np.int32)
    h_codes = np.zeros(nq * 64, np.uint64)
    outs = (o_ids.data_ptr(), o_dist.data_ptr(), o_cnt.data_ptr(), o_sc.data_ptr())
    with pkg.FspannContext(cfg, 0) as ctx:
        h = ctx.handle
        ctx.registry_initialize(X.astype(np.float64))
        ctx.set_id_meta(n)
        ctx.build_index(X)
        ctx.store_set(X)
        torch.cuda.synchronize()

        def run(what, want, fn, *args):
            rc = fn(h, *args)
            _check(L, what, rc, want)
            ctx.sync()

        for t in DTYPES:
            run(("encode", t), want_query(t), L.fspann_encode, nq, _hp(Zh), t, _hp(h_codes), None)
            run(("encode_dev", t), want_query(t), L.fspann_encode_dev, nq, z, t, o_codes.data_ptr(), None, o_bad.data_ptr())
            run(("refine", t), want_refine(t), L.fspann_refine, nq, _hp(Zh), _hp(Zh), t, B, _hp(ids_h), _hp(cnt_h), k, _hp(h_ids), _hp(h_dist), _hp(h_cnt), _hp(h_sc))
            run(("refine_store", t), want_store_query(t), L.fspann_refine_store, nq, _hp(Zh), t, B, _hp(ids_h), _hp(cnt_h), k, _hp(h_ids), _hp(h_dist), _hp(h_cnt),
                _hp(h_sc))
            run(("refine_store_dev", t), want_store_query(t), L.fspann_refine_store_dev, nq, z, t, B, ids_d.data_ptr(), cnt_d.data_ptr(), k, *outs)
            # the one-call search codes its queries first: its refusals are the encode's ("dtype")
            run(("search_store_dev", t), want_query(t), L.fspann_search_store_dev, nq, z, t, -1, B, k, *outs, o_sel.data_ptr(), o_selc.data_ptr(), o_bad.data_ptr())
            run(("search_retry_dev", t), want_query(t), L.fspann_search_retry_dev, nq, z, t, -1, B, k, *outs, o_sel.data_ptr(), o_selc.data_ptr(), o_bad.data_ptr(),
                o_ret.data_ptr())
            run(("groundtruth_rows_dev", t), want_gt_rows(t), L.fspann_groundtruth_rows_dev, n, z, t, nq, z, d, k, o_ids.data_ptr(), o_dist.data_ptr())
        for q, r in itertools.product(DTYPES, DTYPES):
            run(("refine_dev", q, r), want_refine_dev(q, r), L.fspann_refine_dev, nq, z, q, z, r, B, ids_d.data_ptr(), cnt_d.data_ptr(), k, *outs)
            run(("groundtruth_typed_dev", r, q), want_gt_typed(r, q), L.fspann_groundtruth_typed_dev, n, z, r, nq, z, q, d, k, o_ids.data_ptr(), o_dist.data_ptr())
            run(("eval_metrics_typed_dev", r, q), want_metrics_typed(r, q), L.fspann_eval_metrics_typed_dev, n, z, r, nq, z, q, d, k, ids_d.data_ptr(), B,
                cnt_d.data_ptr(), ids_d.data_ptr(), B, o_f64[0].data_ptr(), o_f64[1].data_ptr())
        # the finish calls, behind a search of this size that left nothing to finish
        res = C.c_int64(-1)
        run("search_store_dev", (OK, None), L.fspann_search_store_dev, nq, z, F32, -1, B, k, *outs, o_sel.data_ptr(), o_selc.data_ptr(), o_bad.data_ptr())
        run("search_retry_dev", (OK, None), L.fspann_search_retry_dev, nq, z, F32, -1, B, k, *outs, o_sel.data_ptr(), o_selc.data_ptr(), o_bad.data_ptr(), o_ret.data_ptr())
        assert (o_selc.cpu().numpy() >= 0).all()
        for t in DTYPES:
            run(("search_store_finish_dev", t), want_finish(t), L.fspann_search_store_finish_dev, nq, z, t, -1, B, k, *outs, o_sel.data_ptr(), o_selc.data_ptr(),
                C.byref(res))
            run(("search_retry_finish_dev", t), want_finish(t), L.fspann_search_retry_finish_dev, nq, z, t, -1, B, k, *outs, o_sel.data_ptr(), o_selc.data_ptr(),
                o_bad.data_ptr(), o_ret.data_ptr(), C.byref(res))
        # the calls that replace the store or the index, last
        for t in DTYPES:
            run(("store_set", t), want_rows(t), L.fspann_store_set, n, _hp(Zh), t)
            run(("store_attach_dev", t), want_rows(t), L.fspann_store_attach_dev, n, z, t)
            run(("build_index", t), want_rows(t), L.fspann_build_index, n, _hp(Zh), t, None)
            assert L.fspann_build_begin(h, n) == OK
            run(("build_append", t), want_rows(t), L.fspann_build_append, n, _hp(Zh), t)
    from fspann_amd import hostpipe
    ps = hostpipe.PointStore(n, d, bytes(range(32)))
    try:
        p_ids, p_cnt = np.zeros((nq, B), np.int32), np.zeros(nq, np.int32)
        for t in DTYPES:
            _check(L, ("pointstore_encrypt", t), L.fspann_pointstore_encrypt(ps.handle, 0, n, _hp(Zh), t, 1), want_query(t))
            _check(L, ("pointstore_open_batch", t),
                   L.fspann_pointstore_open_batch(ps.handle, nq, B, _hp(ids_h), _hp(cnt_h), _hp(Zh), t, _hp(p_ids), _hp(p_cnt), 1), want_query(t, "dst_dtype"))
    finally:
        ps.close()


# ---- which template ran -----------------------------------------------------------------------------------------------------------
def _f8_table():
    """the 256 values of OCP fp8 e4m3fn: S EEEE MMM, bias 7; E = 0: +-M/8 * 2^-6; 0x7F / 0xFF NaN"""
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    mag[(e == 15) & (m == 7)] = np.nan
    return np.where(b & 0x80, -mag, mag)


N_STORE = 320


def _rows(rng, d):
    """{dtype: (array as the library takes it, float64 values)}.  One byte buffer read three ways and one 16-bit buffer read two ways.
    Bytes: every value but 0x7F / 0xFF (NaN as fp8), so bytes at and above 0x80 are there: 128..254 as U8, -128..-2 as I8, negative as
    fp8.  16-bit patterns: any sign, bits 14..7 in 120..133, any low seven bits: as bfloat16 2^-7 <= |x| < 2^7 in multiples of 2^-14,
    as a half 1 <= |x| < 4 in multiples of 2^-10.  With queries in multiples of 1/8 below 8 every difference has at most 22
    significant bits, every square at most 44, and a sum of 24 of them fits the 53 of a double: all exact, in any order."""
    by = rng.integers(0, 254, (N_STORE, d)).astype(np.uint8)
    by[by >= 0x7F] += 1                      # 0..126, 128..254
    by[0, :4] = (0x80, 0xFE, 0x7E, 0x00)
    assert (by >= 0x80).any() and not np.isin(by, (0x7F, 0xFF)).any()
    hw = ((rng.integers(0, 2, (N_STORE, d)) << 15) | (rng.integers(120, 134, (N_STORE, d)) << 7) | rng.integers(0, 128, (N_STORE, d))).astype(np.uint16)
    f32 = (rng.integers(-32, 33, (N_STORE, d)) / 4.0).astype(np.float32)
    f64 = rng.integers(-64, 65, (N_STORE, d)) / 8.0
    bf = (hw.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    hf = hw.view(np.float16).astype(np.float64)
    assert np.isfinite(bf).all() and np.isfinite(hf).all()
    return {U8: (by, by.astype(np.float64)), I8: (by.view(np.int8), by.view(np.int8).astype(np.float64)), F8: (by, _f8_table()[by]),
            F16: (hw, hf), BF16: (hw, bf), F32: (f32, f32.astype(np.float64)), F64: (f64, f64)}


def _reference(Q64, V64, ids, cnt, k):
    """QueryServiceImpl's refinement in numpy fp64: the first cnt[i] candidates by (distance, position)"""
    nq = len(Q64)
    oi, od, oc = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf), np.zeros(nq, np.int32)
    for i in range(nq):
        c = max(int(cnt[i]), 0)
        dist = np.sqrt(((Q64[i][None] - V64[ids[i, :c]]) ** 2).sum(1))
        o = np.argsort(dist, kind="stable")[:k]
        oc[i] = len(o)
        oi[i, :len(o)], od[i, :len(o)] = ids[i, :c][o], dist[o]
    return oi, od, oc


def _same(t, ref, scored, what):
    got = (t["ids"].cpu().numpy(), t["dist"].cpu().numpy(), t["count"].cpu().numpy())
    for g, r, name in zip(got, ref, ("ids", "dist", "count")):
        assert np.array_equal(g, r), (what, name, g, r)
    assert np.array_equal(t["scored"].cpu().numpy(), scored), (what, "scored")


def _bufs(nq, B, k):
    import torch
    dev = torch.device("cuda", 0)
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)   # noqa: E731
    return dict(ids=i32(nq, k), dist=torch.zeros((nq, k), dtype=torch.float64, device=dev), count=i32(nq), scored=i32(nq), sel=i32(nq, B), selc=i32(nq), bad=i32(nq),
                ret=i32(nq))


@pytest.mark.parametrize("d", [16, 24, 17], ids=["d16", "d24", "d17"])
@pytest.mark.parametrize("row_dtype", [F32, F64, U8, F16, BF16, F8, I8], ids=["f32", "f64", "u8", "f16", "bf16", "f8", "i8"])
def test_rows_reach_their_own_template(pkg, row_dtype, d):
    """d = 16: 16-byte slots for every type; d = 24: slots for the two-byte types only; d = 17: element-wise everywhere.
    B = 300: two chunks of 256 rows and a merge; k = 33: one above the filter's k, the running top-k."""
    import torch
    L = pkg._native.lib()
    nq = 3
    rng = np.random.default_rng(100 * d + row_dtype)
    raw, V64 = _rows(rng, d)[row_dtype]
    raw = np.ascontiguousarray(raw)
    cfg = pkg.PaperRuntimeConfig(tables=2, divisions=1, m=4, lambda_=2, dim=d, refinement_limit=300, block_size=8, default_probes=1)
    queries = {F32: (rng.integers(-32, 33, (nq, d)) / 4.0).astype(np.float32), F64: rng.integers(-63, 64, (nq, d)) / 8.0}
    with pkg.FspannContext(cfg, 0) as ctx, pkg.FspannContext(cfg, 0) as c32:
        h = ctx.handle
        ctx.registry_initialize(V64)
        for c in (ctx, c32):
            c.set_gfunctions(*ctx.get_gfunctions())
            c.set_id_meta(N_STORE)
        # Setup from the typed rows: the tables of the F32 build of the same values
        assert L.fspann_build_index(h, N_STORE, _hp(raw), row_dtype, None) == OK, L.fspann_last_error()
        c32.build_index(V64.astype(np.float32))
        assert np.array_equal(V64.astype(np.float32).astype(np.float64), V64)
        for td in range(ctx.TD):
            a, b = ctx.get_index(td), c32.get_index(td)
            assert sorted(a) == sorted(b) and all(np.array_equal(a[key], b[key]) for key in a), td
        assert L.fspann_store_set(h, N_STORE, _hp(raw), row_dtype) == OK, L.fspann_last_error()
        raw_bytes = raw.view(np.uint8).reshape(N_STORE, -1)
        for (B, k), (qdt, Q) in itertools.product(((5, 3), (300, 3), (300, 33)), queries.items()):
            what = (row_dtype, d, B, k, qdt)
            Q64, qd = Q.astype(np.float64), _dev(Q)
            ids = rng.integers(0, N_STORE, (nq, B)).astype(np.int32)
            cnt = np.array([B, B - 1, max(1, B // 2)], np.int32)
            ref = _reference(Q64, V64, ids, cnt, k)
            ids_d, cnt_d = _dev(ids), _dev(cnt)
            # the resident store by id
            t = _bufs(nq, B, k)
            torch.cuda.synchronize()
            assert L.fspann_refine_store_dev(h, nq, qd.data_ptr(), qdt, B, ids_d.data_ptr(), cnt_d.data_ptr(), k, t["ids"].data_ptr(), t["dist"].data_ptr(),
                                             t["count"].data_ptr(), t["scored"].data_ptr()) == OK, L.fspann_last_error()
            ctx.sync()
            _same(t, ref, cnt, ("store",) + what)
            # the gathered block holds the store's bytes; dense rows
            cand = torch.zeros((nq, B, raw_bytes.shape[1]), dtype=torch.uint8, device=qd.device)
            t = _bufs(nq, B, k)
            torch.cuda.synchronize()
            assert L.fspann_store_gather_dev(h, nq, ids_d.data_ptr(), cnt_d.data_ptr(), B, cand.data_ptr()) == OK, L.fspann_last_error()
            assert L.fspann_refine_dev(h, nq, qd.data_ptr(), qdt, cand.data_ptr(), row_dtype, B, ids_d.data_ptr(), cnt_d.data_ptr(), k, t["ids"].data_ptr(),
                                       t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr()) == OK, L.fspann_last_error()
            ctx.sync()
            live = np.arange(B)[None] < cnt[:, None]
            assert np.array_equal(cand.cpu().numpy()[live], raw_bytes[ids][live]), ("gather",) + what
            _same(t, ref, cnt, ("dense",) + what)
            # the retry: one probe first, then ten probes over the listed queries (fewer than 10 k rows scored: every query with
            # candidates is listed) and their refinement from the store, the listed scan
            t = _bufs(nq, B, k)
            torch.cuda.synchronize()
            args = (nq, qd.data_ptr(), qdt, -1, B, k, t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr(), t["sel"].data_ptr(),
                    t["selc"].data_ptr(), t["bad"].data_ptr(), t["ret"].data_ptr())
            assert L.fspann_search_retry_dev(h, *args) == OK, L.fspann_last_error()
            assert L.fspann_search_retry_finish_dev(h, *args, None) == OK, L.fspann_last_error()
            ctx.sync()
            sel, selc = t["sel"].cpu().numpy(), t["selc"].cpu().numpy()
            assert (t["bad"].cpu().numpy() == 0).all() and (selc >= 0).all() and t["ret"].cpu().numpy().any(), ("retry",) + what
            _same(t, _reference(Q64, V64, sel, selc, k), np.minimum(selc, B), ("retry",) + what)
