"""GPU: FSPANN_U8 rows (unsigned bytes, value = the integer 0..255) in the resident store, in dense candidate blocks, in the
refine role of a tick and as Setup input.  For such data a byte holds exactly what the reference's double[] holds, so every
result must EQUAL (np.array_equal: ids, fp64 distances, counts, scored, F_q) what the oracle computes from the same values as
float64, and what a second context computes from the same rows held as FSPANN_F32.  No query is left out of a comparison; a
non-finite query has no F_q in the reference (QSI:137-140: it is never routed), so its `sel` is the one thing not compared."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def siftlike(rng, n, d, r=16, noise=6.0):
    """bench.py's SIFT-like generator (integers 0..255 of intrinsic dimension r), as tests/test_gpu_shipped_profiles.py has it."""
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)
    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        return np.clip(np.rint(np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)), 0, 255).astype(np.float32)
    return draw


def _scene(oracle, n=20000, d=128, T=4, D=4, m=16, lam=2, B=256, seed=3, hard_cap=20000, probes=-1):
    rng = np.random.default_rng(seed)
    draw = siftlike(rng, n, d)
    X = draw(n)
    X8 = X.astype(np.uint8)
    assert np.array_equal(X8.astype(np.float32), X)
    X64 = X.astype(np.float64)
    alpha, r, w = oracle.registry_init(X64[:1000], m, 13, T, D)
    o = oracle.Oracle(T, D, m, lam, d, max_global_candidates=hard_cap, refinement_limit=B, probe_override=probes)
    o.set_gfunctions(alpha, r, w)
    o.set_id_meta(n)
    o.set_store(X64)
    o.build_index(X64)
    return dict(X=X, X8=X8, X64=X64, draw=draw, rng=rng, alpha=alpha, r=r, w=w, o=o,
                p=dict(n=n, d=d, T=T, D=D, m=m, lam=lam, B=B, hard_cap=hard_cap, probes=probes))


def _ctx(pkg, sc, rows, store=True, build=True):
    """rows 'u8': index built from bytes, U8 store; 'f32': both from the same values as fp32."""
    p = sc["p"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 max_global_candidates=p["hard_cap"], probe_override=p["probes"])
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["w"])
    ctx.set_id_meta(p["n"])
    if build:
        ctx.build_index(sc["X8"] if rows == "u8" else sc["X"])
    if store:
        if rows == "u8":
            ctx.store_set(sc["X8"], dtype=np.uint8)
        else:
            ctx.store_set(sc["X"])
    return ctx


def _store_dtype(ctx):
    dt = C.c_int(-1)
    ctx.L.fspann_store_dev_ptr.restype = C.c_void_p
    ctx.L.fspann_store_dev_ptr(ctx.handle, C.byref(dt))
    return dt.value


def _bufs(nq, B, K):
    import torch
    dev = torch.device("cuda", 0)
    return dict(ids=torch.full((nq, K), -7, dtype=torch.int32, device=dev), dist=torch.zeros((nq, K), dtype=torch.float64, device=dev),
                count=torch.full((nq,), -7, dtype=torch.int32, device=dev), scored=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                sel=torch.full((nq, B), -1, dtype=torch.int32, device=dev), selc=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                bad=torch.full((nq,), -7, dtype=torch.int32, device=dev), ret=torch.full((nq,), -7, dtype=torch.int32, device=dev))


def _qdt(pkg, Q):
    return pkg._native.F64 if Q.dtype == np.float64 else pkg._native.F32


def _search(pkg, ctx, Q, B, K, call="store", po=-1):
    """fspann_search_store_dev / fspann_search_retry_dev, each followed by its _finish_dev call (flagged queries are answered there)."""
    import torch
    nq = len(Q)
    qd = torch.from_numpy(np.ascontiguousarray(Q)).to(torch.device("cuda", 0))
    t = _bufs(nq, B, K)
    torch.cuda.synchronize()
    args = (nq, qd.data_ptr(), _qdt(pkg, Q), po, B, K, t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr(),
            t["sel"].data_ptr(), t["selc"].data_ptr())
    if call == "retry":
        ctx.search_retry_dev(*args, t["bad"].data_ptr(), t["ret"].data_ptr())
        ctx.search_retry_finish_dev(*args, t["bad"].data_ptr(), t["ret"].data_ptr())
    else:
        ctx.search_store_dev(*args, t["bad"].data_ptr())
        ctx.search_store_finish_dev(*args)
    ctx.sync()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    c = np.maximum(out["selc"], 0)
    out["sel"] = np.where(np.arange(B)[None] < c[:, None], out["sel"], -1)
    if call != "retry":
        del out["ret"]
    return out


def _same_as_oracle(got, ref, B, finite=None):
    nq = len(got["count"])
    finite = np.ones(nq, bool) if finite is None else finite
    assert np.array_equal(got["ids"], ref["ids"]), np.flatnonzero((got["ids"] != ref["ids"]).any(1))[:8]
    assert np.array_equal(got["dist"], ref["dist"]), np.flatnonzero((got["dist"] != ref["dist"]).any(1))[:8]
    assert np.array_equal(got["count"], ref["count"])
    assert np.array_equal(got["scored"], ref["metrics"][:, 2])
    if "ret" in got:
        assert np.array_equal(got["ret"], ref["metrics"][:, 4])
    if "sel" in got:
        assert np.array_equal(got["selc"][finite], ref["sel_count"][finite])
        assert np.array_equal(got["sel"][finite], ref["sel"][finite][:, :B])


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _queries(sc, nq, dtype):
    """SIFT-like queries with a fractional part (a query is not byte data): quarters in fp32, arbitrary fractions in fp64."""
    Q = sc["draw"](nq)
    if dtype == np.float32:
        return (Q + sc["rng"].integers(0, 4, Q.shape).astype(np.float32) / np.float32(4)).astype(np.float32)
    return Q.astype(np.float64) + sc["rng"].random(Q.shape)


# ---- 1. store paths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qdtype", [np.float32, np.float64], ids=["q32", "q64"])
def test_store_paths(pkg, oracle, qdtype):
    import torch
    N = pkg._native
    B, K, nq = 256, 10, 256
    sc = _scene(oracle, B=B)
    o = sc["o"]
    Q = _queries(sc, nq, qdtype)
    Q64 = Q.astype(np.float64)
    ref = o.search(Q64, K)
    assert not ref["metrics"][:, 4].any() and not o.unmodelled      # 256 scored >= 10 K: the reference does not retry here
    ref100 = o.search(Q64, 100)
    assert ref100["metrics"][:, 4].sum() > 0                         # scored <= 256 < 10 K: every scored query takes the second pass
    with _ctx(pkg, sc, "u8") as c8, _ctx(pkg, sc, "f32") as c32:
        assert _store_dtype(c8) == N.U8 and _store_dtype(c32) == N.F32
        # refine_store (host pointers) over F_q of the library's own Route
        codes = c8.encode(Q)
        assert np.array_equal(codes, o.encode(Q64))
        rt = c8.route(codes, limit=B, counters=False)
        a = c8.refine_store(Q, rt["ids"][:, :B], rt["count"], K)
        b = c32.refine_store(Q, rt["ids"][:, :B], rt["count"], K)
        _same(a, b)
        _same_as_oracle(a, ref, B)
        # a dense uint8 block gathered from the store: refine_dev(cand_dtype = U8) on it equals refine_store
        dev = torch.device("cuda", 0)
        seld, cntd = torch.from_numpy(np.ascontiguousarray(rt["ids"][:, :B])).to(dev), torch.from_numpy(rt["count"]).to(dev)
        qd = torch.from_numpy(Q).to(dev)
        cand = torch.zeros((nq, B, sc["p"]["d"]), dtype=torch.uint8, device=dev)
        t = _bufs(nq, B, K)
        torch.cuda.synchronize()
        c8.store_gather_dev(nq, seld.data_ptr(), cntd.data_ptr(), B, cand.data_ptr())
        c8.refine_dev(nq, qd.data_ptr(), _qdt(pkg, Q), cand.data_ptr(), N.U8, B, seld.data_ptr(), cntd.data_ptr(), K, t["ids"].data_ptr(),
                      t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
        c8.sync()
        _same({k: t[k].cpu().numpy() for k in ("ids", "dist", "count", "scored")}, a)
        del cand
        # the one-call search: U8 store, a clone of it, the F32 store
        g8 = _search(pkg, c8, Q, B, K)
        g32 = _search(pkg, c32, Q, B, K)
        _same(g8, g32)
        _same_as_oracle(g8, ref, B)
        with c8.clone() as cl:
            assert _store_dtype(cl) == N.U8
            _same(_search(pkg, cl, Q, B, K), g8)
        # the retry on the device: second pass through the list kernels
        r8 = _search(pkg, c8, Q, B, 100, call="retry")
        r32 = _search(pkg, c32, Q, B, 100, call="retry")
        assert r8["ret"].sum() > 0
        _same(r8, r32)
        _same_as_oracle(r8, ref100, B)
        assert c8.unmodelled_queries() == 0
    # rows that already live in HBM (a torch.uint8 tensor)
    with _ctx(pkg, sc, "u8", store=False) as ca:
        xt = torch.from_numpy(sc["X8"]).to(torch.device("cuda", 0))
        assert xt.dtype == torch.uint8
        ca.store_attach_dev(sc["p"]["n"], xt.data_ptr(), N.U8)
        assert _store_dtype(ca) == N.U8
        _same(_search(pkg, ca, Q, B, K), g8)
        _same(_search(pkg, ca, Q, B, 100, call="retry"), r8)
        ca.sync()
        del xt


# ---- 2. + 4. shapes, through the store and through dense blocks ----------------------------------------------------------------
@pytest.mark.parametrize("B,K", [(256, 10), (1024, 10), (8000, 100)])
@pytest.mark.parametrize("d", [128, 96, 960, 100])
def test_shapes_store_and_dense(pkg, oracle, d, B, K):
    """d: whole tile, partial tile, many tiles, element-wise path; B: one chunk, merge, runs of chunks (dense) / merge (store).
    Counts below B and 0, ids of -1 and past the store's end (skipped, QSI:252-256), half of the store duplicates of 40 rows so
    that equal distances are ordered by position.  Store path: refine_store; dense path: store_gather_dev into a uint8 block,
    then refine_dev(cand_dtype = U8).  Expected: the oracle's refine over the same rows as float64, and the F32 context."""
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 + d + B)
    n, store_n, nq = 6000, 5500, 5
    X = siftlike(rng, n, d)(n)
    X[n // 2:] = X[rng.integers(0, 40, n - n // 2)]
    X8, X64 = X.astype(np.uint8), X.astype(np.float64)
    ids = rng.integers(0, n, (nq, B)).astype(np.int32)
    ids[rng.random((nq, B)) < 0.03] = -1
    count = np.array([B, B - 1, 0, B // 2 + 3, 1], np.int32)
    gid = np.clip(ids, 0, store_n - 1).astype(np.int32)              # rows of the dense block (every row j < count is a row handed over)
    missing = (ids < 0) | (ids >= store_n)
    assert missing[:, :1].size and (ids >= store_n).any() and (ids < 0).any()
    live = np.arange(B)[None] < count[:, None]
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as c8, pkg.FspannContext(cfg, 0) as c32:
        c8.store_set(X8[:store_n], dtype=np.uint8)
        c32.store_set(X[:store_n])
        for qdtype in (np.float32, np.float64):
            Q = siftlike(rng, nq, d)(nq)
            Q = (Q + np.float32(0.25)) if qdtype == np.float32 else (Q.astype(np.float64) + rng.random(Q.shape))
            Q64 = Q.astype(np.float64)
            # ---- store
            rows = X64[np.clip(ids, 0, n - 1)]
            rows[missing] = np.nan
            ei, ed, ec = oracle.refine(Q64, rows, ids, count, K)
            a = c8.refine_store(Q, ids, count, K)
            b = c32.refine_store(Q, ids, count, K)
            _same(a, b)
            assert np.array_equal(a["ids"], ei) and np.array_equal(a["dist"], ed) and np.array_equal(a["count"], ec), (d, B, qdtype)
            assert np.array_equal(a["scored"], (live & ~missing).sum(1))
            del rows
            # ---- dense
            ei, ed, ec = oracle.refine(Q64, X64[gid], ids, count, K)
            qd = torch.from_numpy(Q).to(dev)
            idd, gidd, cntd = torch.from_numpy(ids).to(dev), torch.from_numpy(gid).to(dev), torch.from_numpy(count).to(dev)
            res = {}
            variants = [("u8", c8, torch.uint8, N.U8, 0), ("f32", c32, torch.float32, N.F32, 0)]
            if d == 128 and B == 256:
                variants.append(("u8_misaligned", c8, torch.uint8, N.U8, 1))      # a block that cannot take 16-byte slots
            for name, ctx, tdt, cdt, shift in variants:
                flat = torch.zeros(nq * B * d + 16, dtype=tdt, device=dev)
                cand = flat[shift:shift + nq * B * d]
                t = _bufs(nq, B, K)
                torch.cuda.synchronize()
                ctx.store_gather_dev(nq, gidd.data_ptr(), cntd.data_ptr(), B, cand.data_ptr())
                ctx.refine_dev(nq, qd.data_ptr(), _qdt(pkg, Q), cand.data_ptr(), cdt, B, idd.data_ptr(), cntd.data_ptr(), K, t["ids"].data_ptr(),
                               t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
                ctx.sync()
                if name == "u8":
                    got = cand.cpu().numpy().reshape(nq, B, d)
                    assert np.array_equal(got[live], X8[gid][live])                # the gathered block holds the store's bytes
                res[name] = {k: t[k].cpu().numpy() for k in ("ids", "dist", "count", "scored")}
                del flat, cand
            for name in res:
                _same(res[name], res["u8"])
            g = res["u8"]
            assert np.array_equal(g["ids"], ei) and np.array_equal(g["dist"], ed) and np.array_equal(g["count"], ec), (d, B, qdtype)
            assert np.array_equal(g["scored"], count)
            # the dense block of the routed rows equals the store path when every id loads
            if (~missing[live]).all():
                _same(g, a)


def _dense_case(pkg, oracle, rng, d, B, K, nq, n=6000):
    """A dense block of random store rows per query, U8 and F32, against the oracle's refine over the same rows as float64."""
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    X = siftlike(rng, n, d)(n)
    X[n // 2:] = X[rng.integers(0, 40, n - n // 2)]
    ids = rng.integers(0, n, (nq, B)).astype(np.int32)
    count = rng.integers(0, B + 1, nq).astype(np.int32)
    count[:3] = (B, 0, B - 1)
    Q = siftlike(rng, nq, d)(nq) + np.float32(0.25)
    ei, ed, ec = oracle.refine(Q.astype(np.float64), X.astype(np.float64)[ids], ids, count, K)
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B)
    res = {}
    for rows in ("u8", "f32"):
        with pkg.FspannContext(cfg, 0) as ctx:
            cand = torch.from_numpy(np.ascontiguousarray(X[ids].astype(np.uint8) if rows == "u8" else X[ids])).to(dev)
            qd, idd, cntd = torch.from_numpy(Q).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(count).to(dev)
            t = _bufs(nq, B, K)
            torch.cuda.synchronize()
            ctx.refine_dev(nq, qd.data_ptr(), N.F32, cand.data_ptr(), N.U8 if rows == "u8" else N.F32, B, idd.data_ptr(), cntd.data_ptr(), K,
                           t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
            ctx.sync()
            res[rows] = {k: t[k].cpu().numpy() for k in ("ids", "dist", "count", "scored")}
            del cand
    _same(res["u8"], res["f32"])
    g = res["u8"]
    assert np.array_equal(g["ids"], ei) and np.array_equal(g["dist"], ed) and np.array_equal(g["count"], ec)
    assert np.array_equal(g["scored"], count)


def test_dense_runs_of_chunks(pkg, oracle, monkeypatch):
    """B = 8 000, k = 100 over dense U8 blocks with enough queries that a workgroup walks a RUN of consecutive chunks and keeps the
    running top-k: 48 queries (runs of two chunks, then the merge), and, at one streaming workgroup per CU, 130 queries (a run is
    the whole query: 32 chunks, no merge kernel)."""
    rng = np.random.default_rng(77)
    _dense_case(pkg, oracle, rng, d=32, B=8000, K=100, nq=48)
    monkeypatch.setenv("FSPANN_REFINE_STREAM", "1")
    _dense_case(pkg, oracle, rng, d=32, B=8000, K=100, nq=130)


@pytest.mark.parametrize("knob,val", [("FSPANN_REFINE_STREAM", "0"), ("FSPANN_REFINE_DC", "64"), ("FSPANN_REFINE_DC", "128")])
def test_scan_knobs(pkg, oracle, knob, val, monkeypatch):
    """FSPANN_REFINE_STREAM=0: the one-workgroup-per-chunk scan with 16-byte slots; FSPANN_REFINE_DC is an fp32 notion that U8 rows
    ignore (one tile = 128 bytes = 128 dims)."""
    monkeypatch.setenv(knob, val)
    rng = np.random.default_rng(78)
    _dense_case(pkg, oracle, rng, d=128, B=1024, K=10, nq=20)
    _dense_case(pkg, oracle, rng, d=96, B=256, K=40, nq=20)


# ---- 3. queries that are not finite, and an fp64 query whose squares overflow ------------------------------------------------
@pytest.mark.parametrize("qdtype", [np.float32, np.float64], ids=["q32", "q64"])
def test_nonfinite_and_overflowing_queries(pkg, oracle, qdtype):
    B, K, nq = 256, 10, 64
    sc = _scene(oracle, n=20000, B=B, seed=9)
    o = sc["o"]
    Q = _queries(sc, nq, qdtype)
    Q[3, 7] = np.nan
    Q[10, 0] = np.inf
    Q[11, 127] = -np.inf
    Q[40, 5] = np.nan
    Q[40, 6] = np.inf
    if qdtype == np.float64:
        Q[20, 9] = 1e200            # finite, its square is not: the reference scores the rows with distance +inf
        Q[21, 100] = -1e200
    finite = np.isfinite(Q).all(1)
    Q64 = Q.astype(np.float64)
    codes = o.encode(np.where(np.isfinite(Q64), Q64, 0))      # (a non-finite query is never coded: QSI:137-140)
    ref = o.search(Q64, K, codes=codes)
    assert (ref["count"][~finite] == 0).all() and (ref["metrics"][~finite, 2] == 0).all()
    if qdtype == np.float64:
        assert np.isinf(ref["dist"][20]).all() and ref["count"][20] == K and ref["metrics"][20, 2] > 0
    with _ctx(pkg, sc, "u8") as c8, _ctx(pkg, sc, "f32") as c32:
        g8 = _search(pkg, c8, Q, B, K, call="retry")
        g32 = _search(pkg, c32, Q, B, K, call="retry")
        assert (g8["bad"][~finite] == 1).all() and (g8["scored"][~finite] == 0).all()
        for k in g8:
            if k in ("sel", "selc"):
                assert np.array_equal(g8[k][finite], g32[k][finite]), k
            else:
                assert np.array_equal(g8[k], g32[k]), k
        _same_as_oracle(g8, ref, B, finite)
        # the scan alone (refine_store: the per-query check of an fp64 query, the sum's of an fp32 one)
        rt = c8.route(codes, limit=B, counters=False)
        a = c8.refine_store(Q, rt["ids"][:, :B], rt["count"], K)
        _same(a, c32.refine_store(Q, rt["ids"][:, :B], rt["count"], K))
        nr = ref["metrics"][:, 4] == 0                                   # (a retried query's answer is its second pass')
        assert np.array_equal(a["ids"][nr], ref["ids"][nr]) and np.array_equal(a["dist"][nr], ref["dist"][nr])
        assert (a["count"][~finite] == 0).all() and (a["scored"][~finite] == 0).all()


# ---- 5. tick ---------------------------------------------------------------------------------------------------------------------
def _tick_bufs(ctx, nq, B, K, TD, W):
    import torch
    dev = torch.device("cuda", 0)
    return dict(codes=torch.zeros((nq, TD, W), dtype=torch.int64, device=dev), sel=torch.full((nq, B), -1, dtype=torch.int32, device=dev),
                selc=torch.zeros(nq, dtype=torch.int32, device=dev), hov=torch.zeros(ctx.route_handover_bytes(nq), dtype=torch.uint8, device=dev),
                ids=torch.full((nq, K), -7, dtype=torch.int32, device=dev), dist=torch.zeros((nq, K), dtype=torch.float64, device=dev),
                count=torch.full((nq,), -7, dtype=torch.int32, device=dev), scored=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                bad=torch.zeros(nq, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "gather"])
def test_refine_only_tick_finishes_handed_over_queries(pkg, oracle, dense, monkeypatch):
    """Route as a tick with a hand-over buffer (a tiny entry budget: queries stay PENDING), then a refine-only tick over U8 rows: the
    scan's own workgroups finish the PENDING queries first (refine_stream_fix_kernel<uint8_t, GATHER>: one launch, last_tick_fused)."""
    import torch
    monkeypatch.setenv("FSPANN_ROUTE_LAZY_CAP", "258")
    N = pkg._native
    dev = torch.device("cuda", 0)
    B, K, nq, d = 256, 10, 96, 16
    sc = _scene(oracle, n=40000, d=d, T=10, D=1, m=12, lam=2, B=B, seed=23)
    o, p = sc["o"], sc["p"]
    Q = _queries(sc, nq, np.float32)
    ref = o.search(Q.astype(np.float64), K)
    assert not ref["metrics"][:, 4].any()
    out = {}
    for rows in ("u8", "f32"):
        with _ctx(pkg, sc, rows) as ctx:
            t = _tick_bufs(ctx, nq, B, K, p["T"] * p["D"], 1)
            qd = torch.from_numpy(Q).to(dev)
            codes = ctx.encode(Q)
            t["codes"].copy_(torch.from_numpy(codes.view(np.int64)))
            torch.cuda.synchronize()
            ctx.tick_dev(None, dict(nq=nq, codes=t["codes"].data_ptr(), limit=B, ids=t["sel"].data_ptr(), count=t["selc"].data_ptr(),
                                    handover=t["hov"].data_ptr()), None)
            ctx.sync()
            assert ctx.last_route_info()["lazy"]
            cnt_h = t["selc"].cpu().numpy()
            assert (cnt_h == -2).any(), "no query was handed over"
            cand = None
            if dense:
                # the host's load of F_q; a PENDING query's F_q does not exist yet: its rows are packed from the stand-alone Route,
                # which is what the redo must reproduce (as tests/test_gpu_tick.py does)
                ids_h = t["sel"].cpu().numpy()
                rr = ctx.route(codes, limit=B, counters=False)
                ids_h = np.where((cnt_h == -2)[:, None], rr["ids"][:, :B], ids_h)
                X = sc["X8"] if rows == "u8" else sc["X"]
                cand = torch.from_numpy(np.ascontiguousarray(X[np.clip(ids_h, 0, p["n"] - 1)])).to(dev)
                torch.cuda.synchronize()
            ctx.tick_dev(None, None, dict(nq=nq, q=qd.data_ptr(), B=B, ids=t["sel"].data_ptr(), count=t["selc"].data_ptr(), k=K,
                                          out_ids=t["ids"].data_ptr(), out_dist=t["dist"].data_ptr(), out_count=t["count"].data_ptr(),
                                          scored=t["scored"].data_ptr(), cand=cand.data_ptr() if dense else None,
                                          cand_dtype=N.U8 if rows == "u8" else N.F32, codes=t["codes"].data_ptr(), handover=t["hov"].data_ptr()))
            ctx.sync()
            assert ctx.last_tick_fused()                                  # one launch: the scan finished the PENDING queries itself
            assert ctx.unmodelled_queries() == 0
            g = {k: t[k].cpu().numpy() for k in ("ids", "dist", "count", "scored", "sel", "selc")}
            g["sel"] = np.where(np.arange(B)[None] < g["selc"][:, None], g["sel"], -1)
            out[rows] = g
            del cand
    _same(out["u8"], out["f32"])
    _same_as_oracle(out["u8"], ref, B)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "gather"])
def test_three_role_tick_over_u8_rows_runs_unfused(pkg, oracle, dense):
    """tick_kernel is fp32-only: encode + Route + Refine over U8 rows in one tick_dev call run as stand-alone kernels in stream
    order (last_tick_fused() is False) and give the arrays each part gives alone; the same tick over F32 rows fuses."""
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    B, K, nq, d = 256, 10, 128, 64
    sc = _scene(oracle, n=30000, d=d, T=8, D=1, m=12, lam=2, B=B, seed=5)
    o, p = sc["o"], sc["p"]
    Qa, Qb, Qc = (_queries(sc, nq, np.float32) for _ in range(3))
    ref_a, ref_b = o.search(Qa.astype(np.float64), K), o.search(Qb.astype(np.float64), K)
    assert not ref_a["metrics"][:, 4].any()
    out = {}
    for rows in ("u8", "f32"):
        with _ctx(pkg, sc, rows) as ctx:
            ta, tb = _tick_bufs(ctx, nq, B, K, p["T"], 1), _tick_bufs(ctx, nq, B, K, p["T"], 1)
            tc = _tick_bufs(ctx, nq, B, K, p["T"], 1)
            qa, qc = torch.from_numpy(Qa).to(dev), torch.from_numpy(Qc).to(dev)
            ta["codes"].copy_(torch.from_numpy(ctx.encode(Qa).view(np.int64)))
            tb["codes"].copy_(torch.from_numpy(ctx.encode(Qb).view(np.int64)))
            torch.cuda.synchronize()
            ctx.tick_dev(None, dict(nq=nq, codes=ta["codes"].data_ptr(), limit=B, ids=ta["sel"].data_ptr(), count=ta["selc"].data_ptr()), None)
            ctx.sync()
            cand = None
            if dense:
                X = sc["X8"] if rows == "u8" else sc["X"]
                cand = torch.from_numpy(np.ascontiguousarray(X[np.clip(ta["sel"].cpu().numpy(), 0, p["n"] - 1)])).to(dev)
                torch.cuda.synchronize()
            ctx.tick_dev(dict(nq=nq, q=qc.data_ptr(), codes=tc["codes"].data_ptr(), bad=tc["bad"].data_ptr()),
                         dict(nq=nq, codes=tb["codes"].data_ptr(), limit=B, ids=tb["sel"].data_ptr(), count=tb["selc"].data_ptr()),
                         dict(nq=nq, q=qa.data_ptr(), B=B, ids=ta["sel"].data_ptr(), count=ta["selc"].data_ptr(), k=K, out_ids=ta["ids"].data_ptr(),
                              out_dist=ta["dist"].data_ptr(), out_count=ta["count"].data_ptr(), scored=ta["scored"].data_ptr(),
                              cand=cand.data_ptr() if dense else None, cand_dtype=N.U8 if rows == "u8" else N.F32))
            ctx.sync()
            assert ctx.last_tick_fused() == (rows == "f32")
            g = {k: ta[k].cpu().numpy() for k in ("ids", "dist", "count", "scored", "sel", "selc")}
            g["sel"] = np.where(np.arange(B)[None] < g["selc"][:, None], g["sel"], -1)
            g["codes_c"] = tc["codes"].cpu().numpy().view(np.uint64)
            g["bad_c"] = tc["bad"].cpu().numpy()
            g["selc_b"] = tb["selc"].cpu().numpy()
            g["sel_b"] = np.where(np.arange(B)[None] < g["selc_b"][:, None], tb["sel"].cpu().numpy(), -1)
            out[rows] = g
            del cand
    _same(out["u8"], out["f32"])
    g = out["u8"]
    _same_as_oracle({k: g[k] for k in ("ids", "dist", "count", "scored", "sel", "selc")}, ref_a, B)
    assert np.array_equal(g["codes_c"], o.encode(Qc.astype(np.float64))) and not g["bad_c"].any()
    assert np.array_equal(g["selc_b"], ref_b["sel_count"]) and np.array_equal(g["sel_b"], ref_b["sel"][:, :B])


# ---- 6. touch tracking ---------------------------------------------------------------------------------------------------------
def test_touched_set_equals_the_f32_contexts(pkg, oracle):
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    B, K, nq = 256, 100, 128
    sc = _scene(oracle, B=B, seed=4)
    Q = _queries(sc, nq, np.float32)
    Q[5, 3] = np.nan
    drained = {}
    for rows in ("u8", "f32"):
        with _ctx(pkg, sc, rows) as ctx:
            ctx.touch_enable()
            g = _search(pkg, ctx, Q, B, K, call="retry")
            s1 = ctx.drain_touched()
            # dense rows handed over by the caller (touch_mark over a block)
            X = sc["X8"] if rows == "u8" else sc["X"]
            sel = np.where(g["sel"] >= 0, g["sel"], 0)
            cand = torch.from_numpy(np.ascontiguousarray(X[sel])).to(dev)
            qd = torch.from_numpy(Q).to(dev)
            idd, cntd = torch.from_numpy(np.ascontiguousarray(g["sel"])).to(dev), torch.from_numpy(np.maximum(g["selc"], 0)).to(dev)
            t = _bufs(nq, B, K)
            torch.cuda.synchronize()
            ctx.refine_dev(nq, qd.data_ptr(), N.F32, cand.data_ptr(), N.U8 if rows == "u8" else N.F32, B, idd.data_ptr(), cntd.data_ptr(), K,
                           t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
            ctx.sync()
            s2 = ctx.drain_touched()
            drained[rows] = (s1, s2, g)
            del cand
    assert len(drained["u8"][0]) > 0 and len(drained["u8"][1]) > 0
    assert np.array_equal(drained["u8"][0], drained["f32"][0])
    assert np.array_equal(drained["u8"][1], drained["f32"][1])
    _same(drained["u8"][2], drained["f32"][2])
    # the last pass' F_q of every finite query is in the set of the search (every row of a byte store is valid)
    g = drained["u8"][2]
    fin = np.isfinite(Q).all(1)
    assert set(g["sel"][fin][g["sel"][fin] >= 0].tolist()) <= set(drained["u8"][0].tolist())


# ---- 7. Setup input --------------------------------------------------------------------------------------------------------------
def test_build_from_bytes_gives_the_same_tables(pkg, oracle):
    sc = _scene(oracle, n=30000, d=128, T=4, D=4, m=16, lam=2, seed=6)
    o, p = sc["o"], sc["p"]
    TD = p["T"] * p["D"]
    with _ctx(pkg, sc, "u8", store=False) as c8, _ctx(pkg, sc, "f32", store=False) as c32, _ctx(pkg, sc, "u8", store=False, build=False) as cc:
        cc.build_begin(p["n"])
        for lo, hi in ((0, 1), (1, 4097), (4097, 17000), (17000, p["n"])):      # chunks of uneven sizes
            cc.build_append(sc["X8"][lo:hi])
        cc.build_finish()
        for td in range(TD):
            want = o.get_index(td)
            for ctx in (c8, c32, cc):
                got = ctx.get_index(td)
                assert all(np.array_equal(got[k], want[k]) for k in want), td


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_u8_is_refused_where_a_query_dtype_is_given(pkg, oracle):
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    B, K, nq = 64, 5, 8
    sc = _scene(oracle, n=4000, d=32, T=2, D=2, m=8, lam=2, B=B, seed=8)
    p = sc["p"]
    Q8 = sc["X8"][:nq].copy()
    with _ctx(pkg, sc, "u8") as ctx:
        qd = torch.from_numpy(Q8).to(dev)
        t = _bufs(nq, B, K)
        codes = torch.zeros((nq, p["T"] * p["D"], 1), dtype=torch.int64, device=dev)
        cand = torch.zeros((nq, B, p["d"]), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        out = (t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
        with pytest.raises(pkg.FspannArgumentError, match="q_dtype"):
            ctx.refine_store_dev(nq, qd.data_ptr(), N.U8, B, t["sel"].data_ptr(), t["selc"].data_ptr(), K, *out)
        with pytest.raises(pkg.FspannArgumentError, match="q_dtype"):
            ctx.refine_dev(nq, qd.data_ptr(), N.U8, cand.data_ptr(), N.U8, B, t["sel"].data_ptr(), t["selc"].data_ptr(), K, *out)
        with pytest.raises(pkg.FspannArgumentError):
            ctx.search_store_dev(nq, qd.data_ptr(), N.U8, -1, B, K, *out, t["sel"].data_ptr(), t["selc"].data_ptr())
        with pytest.raises(pkg.FspannArgumentError):
            ctx.search_retry_dev(nq, qd.data_ptr(), N.U8, -1, B, K, *out, t["sel"].data_ptr(), t["selc"].data_ptr())
        with pytest.raises(pkg.FspannArgumentError):
            ctx.encode_dev(nq, qd.data_ptr(), N.U8, codes.data_ptr())
        with pytest.raises(pkg.FspannArgumentError):
            ctx.tick_dev(None, None, dict(nq=nq, q=qd.data_ptr(), q_dtype=N.U8, B=B, ids=t["sel"].data_ptr(), count=t["selc"].data_ptr(), k=K,
                                          out_ids=out[0], out_dist=out[1], out_count=out[2]))
        # host-pointer entry points, straight through the C ABI (the numpy wrapper widens a uint8 array before it gets there)
        L = ctx.L
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        hc = np.zeros((nq, p["T"] * p["D"], 1), np.uint64)
        assert L.fspann_encode(ctx.handle, nq, vp(Q8), N.U8, vp(hc), None) == N.E_ARG
        hcand = np.zeros((nq, B, p["d"]), np.uint8)
        hi, hn = np.zeros((nq, B), np.int32), np.zeros(nq, np.int32)
        oi, od, oc = np.zeros((nq, K), np.int32), np.zeros((nq, K), np.float64), np.zeros(nq, np.int32)
        assert L.fspann_refine(ctx.handle, nq, vp(Q8), vp(hcand), N.U8, B, vp(hi), vp(hn), K, vp(oi), vp(od), vp(oc), None) == N.E_ARG
        assert b"FSPANN_U8" in L.fspann_last_error()
        assert L.fspann_refine_store(ctx.handle, nq, vp(Q8), N.U8, B, vp(hi), vp(hn), K, vp(oi), vp(od), vp(oc), None) == N.E_ARG
        assert b"q_dtype" in L.fspann_last_error()
        ps = C.c_void_p()
        N.check(L.fspann_pointstore_create(100, p["d"], C.byref(ps)))
        try:
            assert L.fspann_pointstore_open_batch(ps, nq, B, vp(hi), vp(hn), vp(hcand), N.U8, vp(hi.copy()), vp(hn.copy()), 1) == N.E_ARG
        finally:
            L.fspann_pointstore_destroy(ps)
        # the numpy wrapper: only an explicit dtype=np.uint8 keeps bytes
        with pytest.raises(pkg.FspannArgumentError):
            ctx.store_set(sc["X"] + np.float32(0.5), dtype=np.uint8)
        with pytest.raises(pkg.FspannArgumentError):
            ctx.store_set(np.full((4, p["d"]), 256.0), dtype=np.uint8)
        ctx.store_set(sc["X"], dtype=np.uint8)                 # integers 0..255 held as fp32: packed
        assert _store_dtype(ctx) == N.U8 and ctx.store_dtype == np.uint8
        ctx.store_set(sc["X8"])                                # no dtype: widened to float64, as before
        assert _store_dtype(ctx) == N.F64 and ctx.store_dtype == np.float64
