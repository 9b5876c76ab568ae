"""GPU: FSPANN_I8 rows (signed bytes, value = the two's-complement integer -128..127) in the resident store, in dense candidate
blocks, in the refine role of a tick, as Setup input and as a metrics base.  Every value is exactly a float and a double, so every
result must EQUAL (np.array_equal: ids, fp64 distances, counts, scored, F_q, index tables) what the oracle computes from the same
values as float64 and what a second context computes from the same rows held as FSPANN_F32.  Nothing here has a tolerance.
Values are drawn over the whole range, and every scene holds rows of all -128, all 127 and all -1 (0xFF: read as unsigned it
would be 255)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def signed_clustered(rng, d, r=16, noise=6.0):
    """integers -128..127 of intrinsic dimension r around 0, standard deviation ~64: both ends of the range are reached (clipped)"""
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)

    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        return np.clip(np.rint(np.float32(64.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)), -128, 127).astype(np.float32)
    return draw


def _rows(rng, n, d, draw=None):
    X = (draw or signed_clustered(rng, d))(n)
    X[n // 3], X[n // 3 + 1], X[n // 3 + 2] = -128, 127, -1
    return X


def _scene(oracle, n=3000, d=128, T=4, D=2, m=12, lam=2, B=256, seed=3, hard_cap=20000, probes=-1):
    rng = np.random.default_rng(seed)
    draw = signed_clustered(rng, d)
    X = _rows(rng, n, d, draw)
    X8 = X.astype(np.int8)
    assert np.array_equal(X8.astype(np.float32), X) and X.min() == -128 and X.max() == 127
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
    """rows 'i8': index built from signed bytes, I8 store; 'f32': both from the same values as fp32."""
    p = sc["p"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 max_global_candidates=p["hard_cap"], probe_override=p["probes"])
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["w"])
    ctx.set_id_meta(p["n"])
    if build:
        ctx.build_index(sc["X8"] if rows == "i8" else sc["X"])
    if store:
        if rows == "i8":
            ctx.store_set(sc["X8"], dtype=np.int8)
        else:
            ctx.store_set(sc["X"])
    return ctx


def _store_dtype(ctx):
    dt = C.c_int(-1)
    ctx.L.fspann_store_dev_ptr(ctx.handle, C.byref(dt))
    return dt.value


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _bufs(nq, B, K):
    import torch
    dev = torch.device("cuda", 0)
    return dict(ids=torch.full((nq, K), -7, dtype=torch.int32, device=dev), dist=torch.zeros((nq, K), dtype=torch.float64, device=dev),
                count=torch.full((nq,), -7, dtype=torch.int32, device=dev), scored=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                sel=torch.full((nq, B), -1, dtype=torch.int32, device=dev), selc=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                bad=torch.full((nq,), -7, dtype=torch.int32, device=dev), ret=torch.full((nq,), -7, dtype=torch.int32, device=dev))


def _qdt(pkg, Q):
    return pkg._native.F64 if Q.dtype == np.float64 else pkg._native.F32


def _out(t):
    return {k: t[k].cpu().numpy() for k in ("ids", "dist", "count", "scored")}


def _search(pkg, ctx, Q, B, K, call="store", po=-1):
    """fspann_search_store_dev / fspann_search_retry_dev, each followed by its _finish_dev call (flagged queries are answered there)."""
    import torch
    nq = len(Q)
    qd = _dev(Q)
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


def _same_as_oracle(got, ref, B, rows=None):
    rows = np.ones(len(got["count"]), bool) if rows is None else rows
    assert np.array_equal(got["ids"][rows], ref["ids"][rows]), np.flatnonzero((got["ids"] != ref["ids"]).any(1))[:8]
    assert np.array_equal(got["dist"][rows], ref["dist"][rows]), np.flatnonzero((got["dist"] != ref["dist"]).any(1))[:8]
    assert np.array_equal(got["count"][rows], ref["count"][rows])
    assert np.array_equal(got["scored"][rows], ref["metrics"][rows, 2])
    if "ret" in got:
        assert np.array_equal(got["ret"][rows], ref["metrics"][rows, 4])
    if "sel" in got:
        assert np.array_equal(got["selc"][rows], ref["sel_count"][rows])
        assert np.array_equal(got["sel"][rows], ref["sel"][rows][:, :B])


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _queries(sc, nq, dtype):
    """queries with a fractional part (a query is not byte data): quarters in fp32, arbitrary fractions in fp64"""
    Q = sc["draw"](nq)
    if dtype == np.float32:
        return (Q + sc["rng"].integers(0, 4, Q.shape).astype(np.float32) / np.float32(4)).astype(np.float32)
    return Q.astype(np.float64) + sc["rng"].random(Q.shape)


# ---- 1. store and dense paths ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qdtype", [np.float32, np.float64], ids=["q32", "q64"])
@pytest.mark.parametrize("d", [128, 100], ids=["slots", "elementwise"])
def test_store_and_dense_paths(pkg, oracle, d, qdtype):
    """d = 128: 16-byte slots; d = 100: rows start off 16 bytes, the element-wise kernel."""
    import torch
    N = pkg._native
    B, K, nq = 256, 10, 37
    sc = _scene(oracle, d=d, B=B, seed=3 + d)
    o = sc["o"]
    Q = _queries(sc, nq, qdtype)
    Q64 = Q.astype(np.float64)
    ref = o.search(Q64, K)                       # (with the reference's adaptive retry: metrics[:, 4] says which queries took it)
    ref100 = o.search(Q64, 100)
    assert not o.unmodelled and ref100["metrics"][:, 4].sum() > 0
    with _ctx(pkg, sc, "i8") as c8, _ctx(pkg, sc, "f32") as c32:
        assert _store_dtype(c8) == N.I8 and _store_dtype(c32) == N.F32 and c8.store_dtype == np.int8
        codes = c8.encode(Q)
        assert np.array_equal(codes, o.encode(Q64))
        rt = c8.route(codes, limit=B, counters=False)
        ids, cnt = np.ascontiguousarray(rt["ids"][:, :B]), rt["count"]
        assert cnt.max() > K
        ei, ed, ec = oracle.refine(Q64, sc["X64"][np.clip(ids, 0, sc["p"]["n"] - 1)], ids, cnt, K)
        # refine_store (host pointers) and refine_store_dev over F_q of the library's own Route
        a = c8.refine_store(Q, ids, cnt, K)
        _same(a, c32.refine_store(Q, ids, cnt, K))
        assert np.array_equal(a["ids"], ei) and np.array_equal(a["dist"], ed) and np.array_equal(a["count"], ec)
        assert np.array_equal(a["scored"], np.minimum(cnt, B))
        seld, cntd, qd = _dev(ids), _dev(cnt), _dev(Q)
        t = _bufs(nq, B, K)
        torch.cuda.synchronize()
        c8.refine_store_dev(nq, qd.data_ptr(), _qdt(pkg, Q), B, seld.data_ptr(), cntd.data_ptr(), K, t["ids"].data_ptr(), t["dist"].data_ptr(),
                            t["count"].data_ptr(), t["scored"].data_ptr())
        c8.sync()
        _same(_out(t), a)
        # a dense int8 block gathered from the store: refine_dev(cand_dtype = I8) on it equals refine_store
        cand = torch.zeros((nq, B, d), dtype=torch.int8, device=torch.device("cuda", 0))
        t = _bufs(nq, B, K)
        torch.cuda.synchronize()
        c8.store_gather_dev(nq, seld.data_ptr(), cntd.data_ptr(), B, cand.data_ptr())
        c8.refine_dev(nq, qd.data_ptr(), _qdt(pkg, Q), cand.data_ptr(), N.I8, B, seld.data_ptr(), cntd.data_ptr(), K, t["ids"].data_ptr(),
                      t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
        c8.sync()
        live = np.arange(B)[None] < cnt[:, None]
        assert np.array_equal(cand.cpu().numpy()[live], sc["X8"][ids][live])         # the gathered block holds the store's bytes
        _same(_out(t), a)
        del cand
        # the one-call search: I8 store, a clone of it, the F32 store (the oracle's answer is its last pass: compare where it took one)
        g8 = _search(pkg, c8, Q, B, K)
        _same(g8, _search(pkg, c32, Q, B, K))
        once = ref["metrics"][:, 4] == 0
        assert once.any()
        _same_as_oracle(g8, ref, B, once)
        with c8.clone() as cl:
            assert _store_dtype(cl) == N.I8
            _same(_search(pkg, cl, Q, B, K), g8)
        # the retry on the device: second pass through the list kernels
        for k, rf in ((K, ref), (100, ref100)):
            r8 = _search(pkg, c8, Q, B, k, call="retry")
            _same(r8, _search(pkg, c32, Q, B, k, call="retry"))
            _same_as_oracle(r8, rf, B)
        assert r8["ret"].sum() > 0 and c8.unmodelled_queries() == 0
    # rows that already live in HBM (a torch.int8 tensor)
    with _ctx(pkg, sc, "i8", store=False) as ca:
        xt = _dev(sc["X8"])
        assert xt.dtype == torch.int8
        ca.store_attach_dev(sc["p"]["n"], xt.data_ptr(), N.I8)
        assert _store_dtype(ca) == N.I8
        _same(_search(pkg, ca, Q, B, K), g8)
        _same(_search(pkg, ca, Q, B, 100, call="retry"), r8)
        ca.sync()
        del xt


# ---- 2. sign -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 100, 16])
def test_bytes_are_read_signed(pkg, oracle, d):
    """Rows of -1 (0xFF) against a zero query score sqrt(d) (read as unsigned: 255 sqrt(d)); a row and its bitwise complement
    (~x = -x - 1) do not tie; -128 is -128.  Store path and dense path, fp32 and fp64 queries."""
    import torch
    N = pkg._native
    rng = np.random.default_rng(d)
    r = rng.integers(-128, 128, d).astype(np.int8)
    X8 = np.stack([np.full(d, -1, np.int8), r, ~r, np.full(d, -128, np.int8), np.full(d, 127, np.int8), np.zeros(d, np.int8)])
    assert X8.view(np.uint8)[0].min() == 255 and np.array_equal(~r, (-r.astype(np.int16) - 1).astype(np.int8))
    n, B, K = len(X8), 8, 6
    X64 = X8.astype(np.float64)
    ids = np.tile(np.array([0, 1, 2, 3, 4, 5, 0, 0], np.int32), (2, 1))
    cnt = np.array([6, 6], np.int32)
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as ctx:
        ctx.store_set(X8, dtype=np.int8)
        for qdtype in (np.float32, np.float64):
            Q = np.stack([np.zeros(d), r.astype(np.float64) + 0.25]).astype(qdtype)
            ei, ed, ec = oracle.refine(Q.astype(np.float64), X64[ids], ids, cnt, K)
            a = ctx.refine_store(Q, ids, cnt, K)
            assert np.array_equal(a["ids"], ei) and np.array_equal(a["dist"], ed) and np.array_equal(a["count"], ec)
            by_id = dict(zip(a["ids"][0].tolist(), a["dist"][0].tolist()))
            assert by_id[0] == np.sqrt(float(d)) and by_id[3] == np.sqrt(16384.0 * d) and by_id[4] == np.sqrt(16129.0 * d) and by_id[5] == 0.0
            assert by_id[0] != np.sqrt(65025.0 * d)                        # (what 0xFF read as 255 would score)
            assert by_id[1] == np.sqrt(float((X64[1] ** 2).sum())) and by_id[2] == np.sqrt(float((X64[2] ** 2).sum())) and by_id[1] != by_id[2]
            assert a["ids"][1, 0] == 1 and a["dist"][1, 0] == np.sqrt(d * 0.0625)
            cand, qd, idd, cntd = _dev(X8[ids]), _dev(Q), _dev(ids), _dev(cnt)
            t = _bufs(2, B, K)
            torch.cuda.synchronize()
            ctx.refine_dev(2, qd.data_ptr(), _qdt(pkg, Q), cand.data_ptr(), N.I8, B, idd.data_ptr(), cntd.data_ptr(), K, t["ids"].data_ptr(),
                           t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
            ctx.sync()
            _same(_out(t), a)


# ---- 3. long lists, duplicates, ids outside the store, a misaligned block ---------------------------------------------------------
@pytest.mark.parametrize("B,K", [(1100, 10), (1100, 100), (256, 10)])
@pytest.mark.parametrize("d", [128, 100])
def test_lists_store_and_dense(pkg, oracle, d, B, K):
    """B = 1100: several chunks and the running top-k / the merge.  Counts below B, 0 and -1 (a query Route flagged: nothing is
    scored), ids of -1 and past the store's end (skipped, QSI:252-256), half of the store duplicates of 40 rows so that equal
    distances are ordered by position.  Store path: refine_store; dense path: store_gather_dev into an int8 block, then
    refine_dev(cand_dtype = I8) — also on a block that starts one byte into its allocation (no 16-byte slots: the element-wise
    kernel).  Expected: the oracle's refine over the same rows as float64, and the F32 context."""
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 + d + B + K)
    n, store_n, nq = 3000, 2700, 6
    X = _rows(rng, n, d)
    X[n // 2:] = X[rng.integers(0, 40, n - n // 2)]
    X8, X64 = X.astype(np.int8), X.astype(np.float64)
    ids = rng.integers(0, n, (nq, B)).astype(np.int32)
    ids[rng.random((nq, B)) < 0.03] = -1
    count = np.array([B, B - 1, 0, B // 2 + 3, 1, -1], np.int32)
    gid = np.clip(ids, 0, store_n - 1).astype(np.int32)              # rows of the dense block (every row j < count is a row handed over)
    missing = (ids < 0) | (ids >= store_n)
    assert (ids >= store_n).any() and (ids < 0).any()
    live = np.arange(B)[None] < count[:, None]
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as c8, pkg.FspannContext(cfg, 0) as c32:
        c8.store_set(X8[:store_n], dtype=np.int8)
        c32.store_set(X[:store_n])
        for qdtype in (np.float32, np.float64):
            Q = signed_clustered(rng, d)(nq)
            Q = (Q + np.float32(0.25)) if qdtype == np.float32 else (Q.astype(np.float64) + rng.random(Q.shape))
            Q64 = Q.astype(np.float64)
            # ---- store
            rows = X64[np.clip(ids, 0, n - 1)]
            rows[missing] = np.nan
            ei, ed, ec = oracle.refine(Q64, rows, ids, np.maximum(count, 0), K)
            a = c8.refine_store(Q, ids, count, K)
            _same(a, c32.refine_store(Q, ids, count, K))
            assert np.array_equal(a["ids"], ei) and np.array_equal(a["dist"], ed) and np.array_equal(a["count"], ec), (d, B, qdtype)
            assert np.array_equal(a["scored"], (live & ~missing).sum(1)) and a["scored"][5] == 0 and a["count"][5] == 0
            del rows
            # ---- dense
            ei, ed, ec = oracle.refine(Q64, X64[gid], ids, np.maximum(count, 0), K)
            qd = _dev(Q)
            idd, gidd, cntd = _dev(ids), _dev(gid), _dev(count)
            res = {}
            for name, ctx, tdt, cdt, shift in (("i8", c8, torch.int8, N.I8, 0), ("f32", c32, torch.float32, N.F32, 0),
                                               ("i8_misaligned", c8, torch.int8, N.I8, 1)):
                flat = torch.zeros(nq * B * d + 16, dtype=tdt, device=dev)
                cand = flat[shift:shift + nq * B * d]
                t = _bufs(nq, B, K)
                torch.cuda.synchronize()
                ctx.store_gather_dev(nq, gidd.data_ptr(), cntd.data_ptr(), B, cand.data_ptr())
                ctx.refine_dev(nq, qd.data_ptr(), _qdt(pkg, Q), cand.data_ptr(), cdt, B, idd.data_ptr(), cntd.data_ptr(), K, t["ids"].data_ptr(),
                               t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
                ctx.sync()
                if name != "f32":
                    got = cand.cpu().numpy().reshape(nq, B, d)
                    assert np.array_equal(got[live], X8[gid][live])                # the gathered block holds the store's bytes
                res[name] = _out(t)
                del flat, cand
            for name in res:
                _same(res[name], res["i8"])
            g = res["i8"]
            assert np.array_equal(g["ids"], ei) and np.array_equal(g["dist"], ed) and np.array_equal(g["count"], ec), (d, B, qdtype)
            assert np.array_equal(g["scored"], np.maximum(count, 0))


def test_duplicate_rows_are_ordered_by_position(pkg, oracle):
    """every candidate row is one of three distinct rows: the top-k is decided by the position in F_q alone"""
    rng = np.random.default_rng(17)
    d, B, K, nq = 128, 256, 40, 4
    X = _rows(rng, 300, d)
    X[3:] = X[rng.integers(0, 3, 297)]
    ids = np.stack([rng.permutation(300)[:B] for _ in range(nq)]).astype(np.int32)
    count = np.full(nq, B, np.int32)
    Q = (signed_clustered(rng, d)(nq) + np.float32(0.5)).astype(np.float32)
    ei, ed, ec = oracle.refine(Q.astype(np.float64), X.astype(np.float64)[ids], ids, count, K)
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as ctx:
        ctx.store_set(X.astype(np.int8), dtype=np.int8)
        a = ctx.refine_store(Q, ids, count, K)
    assert np.array_equal(a["ids"], ei) and np.array_equal(a["dist"], ed) and np.array_equal(a["count"], ec)
    assert (np.diff(a["dist"], axis=1) == 0).any()                     # ties are in the answer


def test_a_deleted_id_is_skipped(pkg, oracle):
    """fspann_set_deleted on a served index over an I8 store: the next search leaves the id out, like the F32 context and the oracle"""
    B, K, nq = 256, 10, 37
    sc = _scene(oracle, d=128, B=B, seed=31)
    o, n = sc["o"], sc["p"]["n"]
    Q = _queries(sc, nq, np.float32)
    first = o.search(Q.astype(np.float64), K)
    victims = np.unique(first["ids"][first["ids"] >= 0][::3]).astype(np.int32)
    assert len(victims) > 5
    deleted = np.zeros(n, np.uint8)
    deleted[victims] = 1
    with _ctx(pkg, sc, "i8") as c8, _ctx(pkg, sc, "f32") as c32:
        before = _search(pkg, c8, Q, B, K, call="retry")
        _same_as_oracle(before, first, B)
        c8.set_deleted(victims)
        c32.set_deleted(victims)
        o.set_id_meta(n, None, deleted)
        ref = o.search(Q.astype(np.float64), K)
        g8 = _search(pkg, c8, Q, B, K, call="retry")
        _same(g8, _search(pkg, c32, Q, B, K, call="retry"))
        _same_as_oracle(g8, ref, B)
        assert not np.isin(g8["ids"], victims).any() and not np.isin(g8["sel"], victims).any()


# ---- 4. tick -------------------------------------------------------------------------------------------------------------------
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
    """Route as a tick with a hand-over buffer (a tiny entry budget: queries stay PENDING), then a refine-only tick over I8 rows: the
    scan's own workgroups finish the PENDING queries first (refine_stream_fix_kernel<int8_t, GATHER>: one launch, last_tick_fused).
    Run on two I8 contexts in turn: each raises the kernel's dynamic-LDS ceiling under its own attribute bit."""
    import torch
    monkeypatch.setenv("FSPANN_ROUTE_LAZY_CAP", "258")
    N = pkg._native
    B, K, nq, d = 256, 10, 96, 16
    sc = _scene(oracle, n=20000, d=d, T=10, D=1, m=12, lam=2, B=B, seed=23)
    o, p = sc["o"], sc["p"]
    Q = _queries(sc, nq, np.float32)
    ref = o.search(Q.astype(np.float64), K)
    assert not ref["metrics"][:, 4].any()
    out = {}
    for rows in ("i8", "f32", "i8_again"):
        with _ctx(pkg, sc, rows[:3].rstrip("_")) as ctx:
            i8 = rows != "f32"
            t = _tick_bufs(ctx, nq, B, K, p["T"] * p["D"], 1)
            qd = _dev(Q)
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
                X = sc["X8"] if i8 else sc["X"]
                cand = _dev(X[np.clip(ids_h, 0, p["n"] - 1)])
                torch.cuda.synchronize()
            ctx.tick_dev(None, None, dict(nq=nq, q=qd.data_ptr(), B=B, ids=t["sel"].data_ptr(), count=t["selc"].data_ptr(), k=K,
                                          out_ids=t["ids"].data_ptr(), out_dist=t["dist"].data_ptr(), out_count=t["count"].data_ptr(),
                                          scored=t["scored"].data_ptr(), cand=cand.data_ptr() if dense else None,
                                          cand_dtype=N.I8 if i8 else N.F32, codes=t["codes"].data_ptr(), handover=t["hov"].data_ptr()))
            ctx.sync()
            assert ctx.last_tick_fused()                                  # one launch: the scan finished the PENDING queries itself
            assert ctx.unmodelled_queries() == 0
            g = {k: t[k].cpu().numpy() for k in ("ids", "dist", "count", "scored", "sel", "selc")}
            g["sel"] = np.where(np.arange(B)[None] < g["selc"][:, None], g["sel"], -1)
            out[rows] = g
            del cand
    _same(out["i8"], out["f32"])
    _same(out["i8_again"], out["i8"])
    _same_as_oracle(out["i8"], ref, B)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "gather"])
def test_three_role_tick_over_i8_rows_runs_unfused(pkg, oracle, dense):
    """tick_kernel is fp32-only: encode + Route + Refine over I8 rows in one tick_dev call run as stand-alone kernels in stream
    order (last_tick_fused() is False) and give the arrays each part gives alone; the same tick over F32 rows fuses."""
    import torch
    N = pkg._native
    B, K, nq, d = 256, 10, 128, 64
    sc = _scene(oracle, n=20000, d=d, T=8, D=1, m=12, lam=2, B=B, seed=5)
    o, p = sc["o"], sc["p"]
    Qa, Qb, Qc = (_queries(sc, nq, np.float32) for _ in range(3))
    ref_a, ref_b = o.search(Qa.astype(np.float64), K), o.search(Qb.astype(np.float64), K)
    assert not ref_a["metrics"][:, 4].any()
    out = {}
    for rows in ("i8", "f32"):
        with _ctx(pkg, sc, rows) as ctx:
            ta, tb = _tick_bufs(ctx, nq, B, K, p["T"], 1), _tick_bufs(ctx, nq, B, K, p["T"], 1)
            tc = _tick_bufs(ctx, nq, B, K, p["T"], 1)
            qa, qc = _dev(Qa), _dev(Qc)
            ta["codes"].copy_(torch.from_numpy(ctx.encode(Qa).view(np.int64)))
            tb["codes"].copy_(torch.from_numpy(ctx.encode(Qb).view(np.int64)))
            torch.cuda.synchronize()
            ctx.tick_dev(None, dict(nq=nq, codes=ta["codes"].data_ptr(), limit=B, ids=ta["sel"].data_ptr(), count=ta["selc"].data_ptr()), None)
            ctx.sync()
            cand = None
            if dense:
                X = sc["X8"] if rows == "i8" else sc["X"]
                cand = _dev(X[np.clip(ta["sel"].cpu().numpy(), 0, p["n"] - 1)])
                torch.cuda.synchronize()
            ctx.tick_dev(dict(nq=nq, q=qc.data_ptr(), codes=tc["codes"].data_ptr(), bad=tc["bad"].data_ptr()),
                         dict(nq=nq, codes=tb["codes"].data_ptr(), limit=B, ids=tb["sel"].data_ptr(), count=tb["selc"].data_ptr()),
                         dict(nq=nq, q=qa.data_ptr(), B=B, ids=ta["sel"].data_ptr(), count=ta["selc"].data_ptr(), k=K, out_ids=ta["ids"].data_ptr(),
                              out_dist=ta["dist"].data_ptr(), out_count=ta["count"].data_ptr(), scored=ta["scored"].data_ptr(),
                              cand=cand.data_ptr() if dense else None, cand_dtype=N.I8 if rows == "i8" else N.F32))
            ctx.sync()
            assert ctx.last_tick_fused() == (rows == "f32")
            assert ctx.L.fspann_last_tick_fused(ctx.handle) == (0 if rows == "i8" else 1)
            g = {k: ta[k].cpu().numpy() for k in ("ids", "dist", "count", "scored", "sel", "selc")}
            g["sel"] = np.where(np.arange(B)[None] < g["selc"][:, None], g["sel"], -1)
            g["codes_c"] = tc["codes"].cpu().numpy().view(np.uint64)
            g["bad_c"] = tc["bad"].cpu().numpy()
            g["selc_b"] = tb["selc"].cpu().numpy()
            g["sel_b"] = np.where(np.arange(B)[None] < g["selc_b"][:, None], tb["sel"].cpu().numpy(), -1)
            out[rows] = g
            del cand
    _same(out["i8"], out["f32"])
    g = out["i8"]
    _same_as_oracle({k: g[k] for k in ("ids", "dist", "count", "scored", "sel", "selc")}, ref_a, B)
    assert np.array_equal(g["codes_c"], o.encode(Qc.astype(np.float64))) and not g["bad_c"].any()
    assert np.array_equal(g["selc_b"], ref_b["sel_count"]) and np.array_equal(g["sel_b"], ref_b["sel"][:, :B])


# ---- 5. touch tracking ---------------------------------------------------------------------------------------------------------
def test_touched_set_equals_the_f32_contexts(pkg, oracle):
    import torch
    N = pkg._native
    B, K, nq = 256, 100, 64
    sc = _scene(oracle, n=6000, B=B, seed=4)
    Q = _queries(sc, nq, np.float32)
    Q[5, 3] = np.nan
    drained = {}
    for rows in ("i8", "f32"):
        with _ctx(pkg, sc, rows) as ctx:
            ctx.touch_enable()
            g = _search(pkg, ctx, Q, B, K, call="retry")
            s1 = ctx.drain_touched()
            # dense rows handed over by the caller (touch_mark over a block)
            X = sc["X8"] if rows == "i8" else sc["X"]
            sel = np.where(g["sel"] >= 0, g["sel"], 0)
            cand, qd = _dev(X[sel]), _dev(Q)
            idd, cntd = _dev(g["sel"]), _dev(np.maximum(g["selc"], 0))
            t = _bufs(nq, B, K)
            torch.cuda.synchronize()
            ctx.refine_dev(nq, qd.data_ptr(), N.F32, cand.data_ptr(), N.I8 if rows == "i8" else N.F32, B, idd.data_ptr(), cntd.data_ptr(), K,
                           t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
            ctx.sync()
            s2 = ctx.drain_touched()
            drained[rows] = (s1, s2, g)
            del cand
    assert len(drained["i8"][0]) > 0 and len(drained["i8"][1]) > 0
    assert np.array_equal(drained["i8"][0], drained["f32"][0])
    assert np.array_equal(drained["i8"][1], drained["f32"][1])
    _same(drained["i8"][2], drained["f32"][2])
    # the last pass' F_q of every finite query is in the set of the search (every row of a signed byte store is valid)
    g = drained["i8"][2]
    fin = np.isfinite(Q).all(1)
    assert set(g["sel"][fin][g["sel"][fin] >= 0].tolist()) <= set(drained["i8"][0].tolist())


# ---- 6. Setup input --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2], ids=["exact_fp64", "mfma_prefilter"])
@pytest.mark.parametrize("d", [128, 100])
def test_build_from_signed_bytes_gives_the_same_tables(pkg, oracle, d, mode):
    """build_index(int8 rows) and build_begin / append / finish in two uneven chunks give the tables of the F32 build and of the
    oracle, under either encode mode (2: the MFMA pre-filter with the exact re-check, reached at this size because it is forced)."""
    sc = _scene(oracle, n=5000, d=d, T=4, D=2, m=16, lam=2, seed=6 + d)
    o, p = sc["o"], sc["p"]
    TD = p["T"] * p["D"]
    with _ctx(pkg, sc, "i8", store=False, build=False) as c8, _ctx(pkg, sc, "f32", store=False, build=False) as c32, \
            _ctx(pkg, sc, "i8", store=False, build=False) as cc:
        for ctx in (c8, c32, cc):
            ctx.set_encode_mode(mode)
        c8.build_index(sc["X8"])
        c32.build_index(sc["X"])
        cc.build_begin(p["n"])
        for lo, hi in ((0, 1237), (1237, p["n"])):                       # two chunks of uneven sizes (the first ends off a dword)
            cc.build_append(sc["X8"][lo:hi])
        cc.build_finish()
        for td in range(TD):
            want = o.get_index(td)
            f32 = c32.get_index(td)
            for ctx in (c8, cc):
                got = ctx.get_index(td)
                assert all(np.array_equal(got[k], want[k]) for k in want), td
                assert sorted(got) == sorted(f32) and all(np.array_equal(got[k], f32[k]) for k in f32), td


# ---- 7. metrics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q_as", ["i8", "f32"])
def test_metrics_i8_match_compute_metrics_at_k(pkg, oracle, q_as):
    """The scene of test_metrics_u8_match_compute_metrics_at_k on signed data, queries as signed bytes and as fp32."""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    rng = np.random.default_rng(3)
    n, d, nq, k = 4000, 24, 64, 10
    X8 = rng.integers(-128, 128, (n, d), dtype=np.int8)
    X8[100], X8[101], X8[102] = -128, 127, -1
    Q8 = rng.integers(-128, 128, (nq, d), dtype=np.int8)
    Q8[5] = X8[17]                                           # distance 0 to its nearest neighbour: ratio is NaN there
    X, Q = X8.astype(np.float32), Q8.astype(np.float32)
    gt, _ = oracle.groundtruth(X, Q, 20)
    ann = gt[:, :12].copy()
    for i in range(nq):                                      # an approximate answer: some true neighbours replaced
        m = rng.random(12) < 0.4
        ann[i, m] = rng.integers(0, n, int(m.sum()))
    cnt = np.full(nq, 12, np.int32)
    cnt[3], cnt[9] = 7, 0                                    # fewer than k results: ratio NaN, recall over what exists
    ann[11, 2] = -1                                          # an unparsable id
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=d), 0) as ctx:
        xd, ad, cd, gd = _dev(X8), _dev(ann), _dev(cnt), _dev(gt)
        qd, qdt = (_dev(Q8), N.I8) if q_as == "i8" else (_dev(Q), N.F32)
        rec = torch.zeros(nq, dtype=torch.float64, device=dev)
        rat = torch.zeros(nq, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.eval_metrics_typed_dev(n, xd.data_ptr(), N.I8, nq, qd.data_ptr(), qdt, d, k, ad.data_ptr(), 12, cd.data_ptr(), gd.data_ptr(), 20,
                                   rec.data_ptr(), rat.data_ptr())
        ctx.sync()
        rec, rat = rec.cpu().numpy(), rat.cpu().numpy()
    ref_rec, ref_rat = oracle.metrics(X, Q, k, ann, cnt, gt)
    assert np.array_equal(rec, ref_rec)
    assert np.array_equal(np.isnan(rat), np.isnan(ref_rat)) and np.isnan(rat[[3, 5, 9, 11]]).all()
    ok = ~np.isnan(rat)
    assert ok.sum() == nq - 4 and np.array_equal(rat[ok], ref_rat[ok])


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_i8_is_refused_where_it_cannot_stand(pkg, oracle):
    """every query dtype, the point store, ground truth over any pair but (I8, I8) and metrics with another query type:
    FSPANN_E_ARG, the message names FSPANN_I8; next to each refusal the same call with an accepted pair is taken"""
    import torch
    N = pkg._native
    I8 = N.I8
    dev = torch.device("cuda", 0)
    B, K, nq = 64, 5, 8
    sc = _scene(oracle, n=3000, d=32, T=2, D=2, m=8, lam=2, B=B, seed=8)
    p = sc["p"]
    Q8 = sc["X8"][:nq].copy()
    Q32 = sc["X"][:nq] + np.float32(0.25)
    with _ctx(pkg, sc, "i8") as ctx:
        L, h = ctx.L, ctx.handle
        err = lambda: L.fspann_last_error().decode()
        q8, q32 = _dev(Q8), _dev(Q32)
        t = _bufs(nq, B, K)
        codes = torch.zeros((nq, p["T"] * p["D"], 1), dtype=torch.int64, device=dev)
        cand = torch.zeros((nq, B, p["d"]), dtype=torch.int8, device=dev)
        t["selc"].zero_()
        torch.cuda.synchronize()
        out = (t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
        sel = (t["sel"].data_ptr(), t["selc"].data_ptr())
        calls = [
            lambda q, dt: ctx.refine_store_dev(nq, q, dt, B, *sel, K, *out),
            lambda q, dt: ctx.refine_dev(nq, q, dt, cand.data_ptr(), I8, B, *sel, K, *out),
            lambda q, dt: ctx.search_store_dev(nq, q, dt, -1, B, K, *out, *sel),
            lambda q, dt: ctx.search_store_finish_dev(nq, q, dt, -1, B, K, *out, *sel),
            lambda q, dt: ctx.search_retry_dev(nq, q, dt, -1, B, K, *out, *sel),
            lambda q, dt: ctx.search_retry_finish_dev(nq, q, dt, -1, B, K, *out, *sel),
            lambda q, dt: ctx.encode_dev(nq, q, dt, codes.data_ptr()),
            lambda q, dt: ctx.tick_dev(None, None, dict(nq=nq, q=q, q_dtype=dt, B=B, ids=sel[0], count=sel[1], k=K, out_ids=out[0], out_dist=out[1],
                                                        out_count=out[2])),
            lambda q, dt: ctx.tick_dev(None, None, dict(nq=nq, q=q, q_dtype=dt, B=B, ids=sel[0], count=sel[1], k=K, cand=cand.data_ptr(),
                                                        cand_dtype=I8, out_ids=out[0], out_dist=out[1], out_count=out[2])),
            lambda q, dt: ctx.tick_dev(dict(nq=nq, q=q, dtype=dt, codes=codes.data_ptr()), None, None),
        ]
        for call in calls:
            with pytest.raises(pkg.FspannArgumentError, match="FSPANN_I8"):
                call(q8.data_ptr(), I8)
            ctx.sync()
            call(q32.data_ptr(), N.F32)                                 # the same call with a query dtype the library takes
            ctx.sync()
        # host-pointer entry points, straight through the C ABI
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        hc = np.zeros((nq, p["T"] * p["D"], 1), np.uint64)
        assert L.fspann_encode(h, nq, vp(Q8), I8, vp(hc), None) == N.E_ARG and "FSPANN_I8" in err()
        assert L.fspann_encode(h, nq, vp(Q32), N.F32, vp(hc), None) == N.OK
        hcand = np.zeros((nq, B, p["d"]), np.int8)
        fcand = np.zeros((nq, B, p["d"]), np.float32)
        hi, hn = np.zeros((nq, B), np.int32), np.zeros(nq, np.int32)
        oi, od, oc = np.zeros((nq, K), np.int32), np.zeros((nq, K), np.float64), np.zeros(nq, np.int32)
        assert L.fspann_refine(h, nq, vp(Q8), vp(hcand), I8, B, vp(hi), vp(hn), K, vp(oi), vp(od), vp(oc), None) == N.E_ARG
        assert "FSPANN_I8" in err()
        assert L.fspann_refine(h, nq, vp(Q32), vp(fcand), N.F32, B, vp(hi), vp(hn), K, vp(oi), vp(od), vp(oc), None) == N.OK
        assert L.fspann_refine_store(h, nq, vp(Q8), I8, B, vp(hi), vp(hn), K, vp(oi), vp(od), vp(oc), None) == N.E_ARG
        assert "FSPANN_I8" in err() and "q_dtype" in err()
        assert L.fspann_refine_store(h, nq, vp(Q32), N.F32, B, vp(hi), vp(hn), K, vp(oi), vp(od), vp(oc), None) == N.OK
        ps = C.c_void_p()
        N.check(L.fspann_pointstore_create(100, p["d"], C.byref(ps)))
        try:
            key = np.arange(32, dtype=np.uint8)
            N.check(L.fspann_pointstore_set_master_key(ps, vp(key)))
            assert L.fspann_pointstore_encrypt(ps, 0, 4, vp(hcand), I8, 1) == N.E_ARG and "FSPANN_I8" in err()
            assert L.fspann_pointstore_encrypt(ps, 0, 4, vp(fcand), N.F32, 1) == N.OK
            assert L.fspann_pointstore_open_batch(ps, nq, B, vp(hi), vp(hn), vp(hcand), I8, vp(hi.copy()), vp(hn.copy()), 1) == N.E_ARG
            assert "FSPANN_I8" in err()
            assert L.fspann_pointstore_open_batch(ps, nq, B, vp(hi), vp(hn), vp(fcand), N.F32, vp(hi.copy()), vp(hn.copy()), 1) == N.OK
        finally:
            L.fspann_pointstore_destroy(ps)
        # ground truth: (I8, I8) only; any other pair with a signed byte in it is a pair that does not match, both names in the message
        buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        o64 = torch.zeros(4096, dtype=torch.float64, device=dev)
        b, o = buf.data_ptr(), o64.data_ptr()
        torch.cuda.synchronize()
        names = {N.F32: "FSPANN_F32", N.F64: "FSPANN_F64", N.U8: "FSPANN_U8", I8: "FSPANN_I8"}
        gt = lambda bdt, qdt: L.fspann_groundtruth_typed_dev(h, 10, b, bdt, 2, b, qdt, 16, 5, o, o + 16384)
        for bdt, qdt in ((I8, N.U8), (N.U8, I8), (I8, N.F32), (N.F32, I8), (I8, N.F64), (N.F64, I8)):
            assert gt(bdt, qdt) == N.E_ARG, (bdt, qdt)
            assert "Base and query types must match (both fvecs or both bvecs)" in err() and names[bdt] in err() and names[qdt] in err(), err()
        assert gt(I8, I8) == N.OK and gt(N.U8, N.U8) == N.OK
        assert L.fspann_groundtruth_typed_dev(h, 10, b, I8, 2, b, I8, 32769, 5, o, o + 16384) == N.E_ARG and "32768" in err() and "FSPANN_I8" in err()
        mt = lambda bdt, qdt: L.fspann_eval_metrics_typed_dev(h, 10, b, bdt, 2, b, qdt, 16, 5, o, 8, None, o, 8, o, o)
        for bdt, qdt in ((I8, N.U8), (I8, N.F64), (N.U8, I8), (N.F32, I8), (N.F64, I8)):
            assert mt(bdt, qdt) == N.E_ARG and "FSPANN_I8" in err(), (bdt, qdt)
        assert mt(I8, I8) == N.OK and mt(I8, N.F32) == N.OK and mt(N.U8, N.U8) == N.OK
        # a pair with a half, a bfloat16 or an fp8 in it keeps the name it had: the new checks stand behind the existing ones
        for other, name in ((N.F16, "FSPANN_F16"), (N.BF16, "FSPANN_BF16"), (N.F8E4M3, "FSPANN_F8E4M3")):
            for bdt, qdt in ((I8, other), (other, I8)):
                assert gt(bdt, qdt) == N.E_ARG and name in err() and "no ground truth over" in err(), (bdt, qdt)
                assert mt(bdt, qdt) == N.E_ARG and name in err() and "metrics take " + name in err(), (bdt, qdt)
        ctx.sync()
        # the numpy wrapper: only an explicit dtype=np.int8 keeps signed bytes, and never rounds or shifts
        with pytest.raises(pkg.FspannArgumentError):
            ctx.store_set(sc["X"] + np.float32(0.5), dtype=np.int8)
        with pytest.raises(pkg.FspannArgumentError):
            ctx.store_set(np.full((4, p["d"]), 128.0), dtype=np.int8)
        assert _store_dtype(ctx) == N.I8                       # refused before the store was touched
        ctx.store_set(sc["X"], dtype=np.int8)                  # integers -128..127 held as fp32: packed
        assert _store_dtype(ctx) == N.I8 and ctx.store_dtype == np.int8
        ctx.store_set(sc["X8"])                                # no dtype: widened to float64, as before
        assert _store_dtype(ctx) == N.F64 and ctx.store_dtype == np.float64
