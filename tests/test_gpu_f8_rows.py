"""GPU: FSPANN_F8E4M3 rows (OCP fp8 e4m3fn bytes: S EEEE MMM, bias 7, 0x7F / 0xFF NaN, no infinity) in the resident store, in dense
candidate blocks, in the refine role of a tick, as Setup input and as the base of the metrics.  Rows are float32 values rounded to
e4m3 ONCE, by the caller (torch's cast on the CPU), before anything else sees them; every finite e4m3 value is a half, a float and a
double, so every result must EQUAL (np.array_equal: ids, fp64 distance bits, counts, scored, F_q) three witnesses: the oracle fed
the rows widened by THIS file's 256-entry table (built from the format's definition, not from library code), a context holding the
same values as FSPANN_F32, and a context holding them as FSPANN_F16.  There are no tolerances.  A non-finite query has no F_q in
the reference (QSI:137-140: it is never routed), so its `sel` is the one thing not compared.
tests/test_gpu_bf16_rows.py, test for test, plus what only fp8 has: all 256 patterns through the public path, and ties."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def e4m3_table():
    """value of each of the 256 patterns, from the definition: E = 0: +-M/8 * 2^-6; E = 1..15: +-(1 + M/8) * 2^(E-7); 0x7F / 0xFF NaN"""
    t = np.empty(256, np.float64)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = (m / 8.0) * 2.0 ** -6
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if s else v
    return t


TABLE = e4m3_table()
FINITE = np.array([b for b in range(256) if (b & 0x7F) != 0x7F], np.uint8)
SCALE = np.float32(16.0)


def clustered(rng, n, d, r=16, noise=6.0):
    """bench.py's SIFT-like generator (intrinsic dimension r) without its rounding to integers: float32 draws in [0, 64].
    draw(cnt) -> float32; the rows of a test are f8_cast(draw(cnt)), the one rounding (|x| stays far below 448: no row turns NaN)."""
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)
    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        v = np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)
        return (np.clip(v, 0, 255) / np.float32(64.0) * SCALE).astype(np.float32)
    return draw


def f8_cast(a):
    """the caller's rounding: float32 values -> e4m3 bytes, torch's cast on the CPU"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()


def widen(b):
    """e4m3 bytes -> the float64 values they are, by this file's table"""
    return TABLE[np.ascontiguousarray(b, np.uint8)]


def _f8s(a):
    """the one rounding: float32 values -> e4m3 bytes, and the same values as float32 / float16 / float64 (all exact)"""
    b = f8_cast(a)
    x64 = widen(b)
    assert np.isfinite(x64).all()
    x32, x16 = x64.astype(np.float32), x64.astype(np.float16)
    assert np.array_equal(x32.astype(np.float64), x64) and np.array_equal(x16.astype(np.float64), x64)
    assert (np.abs(x64 - a) <= np.maximum(np.abs(a.astype(np.float64)) * 2.0 ** -4, 2.0 ** -10)).all()      # half an ulp of four bits
    return b, x32, x16, x64


ROWS = ("f8", "f32", "f16")


def _scene(oracle, n=20000, d=128, T=4, D=4, m=16, lam=2, B=256, seed=3, hard_cap=20000, probes=-1):
    rng = np.random.default_rng(seed)
    draw = clustered(rng, n, d)
    raw = draw(n)
    Xb, X, X16, X64 = _f8s(raw)
    assert not np.array_equal(X, raw)                                    # the rounding is a real one: these are not fp32 data
    alpha, r, w = oracle.registry_init(X64[:1000], m, 13, T, D)
    o = oracle.Oracle(T, D, m, lam, d, max_global_candidates=hard_cap, refinement_limit=B, probe_override=probes)
    o.set_gfunctions(alpha, r, w)
    o.set_id_meta(n)
    o.set_store(X64)
    o.build_index(X64)
    return dict(X=X, Xb=Xb, X16=X16, X64=X64, draw=draw, rng=rng, alpha=alpha, r=r, w=w, o=o,
                p=dict(n=n, d=d, T=T, D=D, m=m, lam=lam, B=B, hard_cap=hard_cap, probes=probes))


def _set_store(pkg, ctx, rows, Xb, X, X16):
    if rows == "f8":
        ctx.store_set(Xb, dtype=pkg.float8_e4m3fn)
    elif rows == "f16":
        ctx.store_set(X16, dtype=np.float16)
    else:
        ctx.store_set(X)


def _ctx(pkg, sc, rows, store=True, build=True):
    """rows 'f8': index built from e4m3 bytes, F8E4M3 store; 'f32' / 'f16': both from the same values as fp32 / halves."""
    p = sc["p"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 max_global_candidates=p["hard_cap"], probe_override=p["probes"])
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["w"])
    ctx.set_id_meta(p["n"])
    if build:
        if rows == "f8":
            ctx.build_index(sc["Xb"], dtype=pkg.float8_e4m3fn)
        elif rows == "f16":
            ctx.build_index(sc["X16"])
        else:
            ctx.build_index(sc["X"])
    if store:
        _set_store(pkg, ctx, rows, sc["Xb"], sc["X"], sc["X16"])
    return ctx


def _cdt(pkg, rows):
    N = pkg._native
    return dict(f8=N.F8E4M3, f32=N.F32, f16=N.F16)[rows]


def _src(rows, Xb, X, X16):
    return dict(f8=Xb, f32=X, f16=X16)[rows]


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


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_as_oracle(got, ref, B, finite=None):
    nq = len(got["count"])
    finite = np.ones(nq, bool) if finite is None else finite
    assert np.array_equal(got["ids"], ref["ids"]), np.flatnonzero((got["ids"] != ref["ids"]).any(1))[:8]
    assert np.array_equal(_bits(got["dist"]), _bits(ref["dist"])), np.flatnonzero((got["dist"] != ref["dist"]).any(1))[:8]
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
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _queries(sc, nq, dtype):
    """queries are not e4m3 values: fp32 draws as they come, fp64 ones with bits below fp32's"""
    Q = sc["draw"](nq)
    if dtype == np.float32:
        assert not np.array_equal(widen(f8_cast(Q)).astype(np.float32), Q)
        return Q
    return Q.astype(np.float64) + sc["rng"].random(Q.shape) * 2.0 ** -10


def _dev(a):
    """a numpy array on the device (e4m3 bytes as a uint8 tensor, bits unchanged)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _tdt(rows):
    import torch
    return dict(f8=torch.uint8, f32=torch.float32, f16=torch.float16)[rows]


def _refine_dev(pkg, ctx, rows, cand, qd, Q, B, idd, cntd, K):
    import torch
    nq = len(Q)
    t = _bufs(nq, B, K)
    torch.cuda.synchronize()
    ctx.refine_dev(nq, qd.data_ptr(), _qdt(pkg, Q), cand.data_ptr(), _cdt(pkg, rows), B, idd.data_ptr(), cntd.data_ptr(), K, t["ids"].data_ptr(),
                   t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
    ctx.sync()
    return {k: t[k].cpu().numpy() for k in ("ids", "dist", "count", "scored")}


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
    with _ctx(pkg, sc, "f8") as ch, _ctx(pkg, sc, "f32") as c32, _ctx(pkg, sc, "f16") as c16:
        assert _store_dtype(ch) == N.F8E4M3 and _store_dtype(c32) == N.F32 and _store_dtype(c16) == N.F16 and ch.store_dtype is pkg.float8_e4m3fn
        # refine_store (host pointers) over F_q of the library's own Route
        codes = ch.encode(Q)
        assert np.array_equal(codes, o.encode(Q64))
        rt = ch.route(codes, limit=B, counters=False)
        a = ch.refine_store(Q, rt["ids"][:, :B], rt["count"], K)
        _same(a, c32.refine_store(Q, rt["ids"][:, :B], rt["count"], K))
        _same(a, c16.refine_store(Q, rt["ids"][:, :B], rt["count"], K))
        _same_as_oracle(a, ref, B)
        # refine_store_dev, and a dense fp8 block gathered from the store: refine_dev(cand_dtype = F8E4M3) on it equals refine_store
        dev = torch.device("cuda", 0)
        seld, cntd = _dev(rt["ids"][:, :B]), _dev(rt["count"])
        qd = _dev(Q)
        t = _bufs(nq, B, K)
        torch.cuda.synchronize()
        ch.refine_store_dev(nq, qd.data_ptr(), _qdt(pkg, Q), B, seld.data_ptr(), cntd.data_ptr(), K, t["ids"].data_ptr(), t["dist"].data_ptr(),
                            t["count"].data_ptr(), t["scored"].data_ptr())
        ch.sync()
        _same({k: t[k].cpu().numpy() for k in ("ids", "dist", "count", "scored")}, a)
        cand = torch.zeros((nq, B, sc["p"]["d"]), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ch.store_gather_dev(nq, seld.data_ptr(), cntd.data_ptr(), B, cand.data_ptr())
        _same(_refine_dev(pkg, ch, "f8", cand, qd, Q, B, seld, cntd, K), a)
        del cand
        # the one-call search: F8E4M3 store, a clone of it, the F32 store, the F16 store
        gh = _search(pkg, ch, Q, B, K)
        _same(gh, _search(pkg, c32, Q, B, K))
        _same(gh, _search(pkg, c16, Q, B, K))
        _same_as_oracle(gh, ref, B)
        with ch.clone() as cl:
            assert _store_dtype(cl) == N.F8E4M3
            _same(_search(pkg, cl, Q, B, K), gh)
        # the retry on the device: second pass through the list kernels
        rh = _search(pkg, ch, Q, B, 100, call="retry")
        assert rh["ret"].sum() > 0
        _same(rh, _search(pkg, c32, Q, B, 100, call="retry"))
        _same(rh, _search(pkg, c16, Q, B, 100, call="retry"))
        _same_as_oracle(rh, ref100, B)
        assert ch.unmodelled_queries() == 0
    # rows that already live in HBM (a torch.float8_e4m3fn tensor)
    with _ctx(pkg, sc, "f8", store=False) as ca:
        xt = _dev(sc["Xb"]).view(torch.float8_e4m3fn)
        assert xt.element_size() == 1
        ca.store_attach_dev(sc["p"]["n"], xt.data_ptr(), N.F8E4M3)
        assert _store_dtype(ca) == N.F8E4M3
        _same(_search(pkg, ca, Q, B, K), gh)
        _same(_search(pkg, ca, Q, B, 100, call="retry"), rh)
        ca.sync()
        del xt


# ---- 2. shapes, through the store and through dense blocks ---------------------------------------------------------------------
SHAPE_B = (1, 64, 256, 1024, 5000)
SHAPE_K = (1, 10, 100)


def _counts(B):
    return np.array([B, B - 1, 0, B // 2 + (3 if B > 8 else 0), 1], np.int32)


@pytest.mark.parametrize("d", [16, 100, 128, 136, 144, 256, 768, 960])
def test_shapes_store_and_dense(pkg, oracle, d):
    """d: 16 (one slot), 128 (one tile), 100 and 136 (d % 16 != 0: the element-wise path), 144 (a partial last tile), 256 (two
    tiles), 768 / 960 (many tiles); every B of SHAPE_B (a single row, part of a chunk, one chunk, the merge, 20 chunks: runs of chunks
    when dense) with every K of SHAPE_K (also K > B).  Counts below B and 0, ids of -1 and past the store's end (skipped,
    QSI:252-256), half of the store duplicates of 40 rows so that equal distances are ordered by position.  Store path:
    refine_store; dense path: store_gather_dev into an fp8 block, then refine_dev(cand_dtype = F8E4M3); d = 128, B = 256 also with
    the block's base pointer offset by 1 byte.  Expected: the oracle's refine over the same rows as float64, the F32 context and the
    F16 context."""
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    n, store_n, nq = 6000, 5500, 5
    rng = np.random.default_rng(2000 + d)
    raw = clustered(rng, n, d)(n)
    raw[n // 2:] = raw[rng.integers(0, 40, n - n // 2)]
    Xb, X, X16, X64 = _f8s(raw)
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=max(SHAPE_B))
    with pkg.FspannContext(cfg, 0) as ch, pkg.FspannContext(cfg, 0) as c32, pkg.FspannContext(cfg, 0) as c16:
        ch.store_set(Xb[:store_n], dtype=pkg.float8_e4m3fn)
        c32.store_set(X[:store_n])
        c16.store_set(X16[:store_n], dtype=np.float16)
        assert _store_dtype(ch) == N.F8E4M3
        for B in SHAPE_B:
            ids = rng.integers(0, n, (nq, B)).astype(np.int32)
            ids[rng.random((nq, B)) < 0.03] = -1
            if B >= 64:
                ids[0, 5], ids[0, 6] = -1, n - 1
                assert (ids >= store_n).any() and (ids < 0).any()
            count = _counts(B)
            gid = np.clip(ids, 0, store_n - 1).astype(np.int32)          # rows of the dense block (every row j < count is a row handed over)
            missing = (ids < 0) | (ids >= store_n)
            live = np.arange(B)[None] < count[:, None]
            rows_store = X64[np.clip(ids, 0, n - 1)]
            rows_store[missing] = np.nan
            rows_dense = X64[gid]
            idd, gidd, cntd = _dev(ids), _dev(gid), _dev(count)
            for qdtype in (np.float32, np.float64):
                Qr = clustered(rng, nq, d)(nq)
                Q = Qr if qdtype == np.float32 else (Qr.astype(np.float64) + rng.random(Qr.shape) * 2.0 ** -10)
                Q64 = Q.astype(np.float64)
                qd = _dev(Q)
                for K in SHAPE_K:
                    tag = (d, B, K, qdtype.__name__)
                    # ---- store
                    ei, ed, ec = oracle.refine(Q64, rows_store, ids, count, K)
                    a = ch.refine_store(Q, ids, count, K)
                    _same(a, c32.refine_store(Q, ids, count, K))
                    _same(a, c16.refine_store(Q, ids, count, K))
                    assert np.array_equal(a["ids"], ei) and np.array_equal(_bits(a["dist"]), _bits(ed)) and np.array_equal(a["count"], ec), tag
                    assert np.array_equal(a["scored"], (live & ~missing).sum(1)), tag
                    # ---- dense
                    ei, ed, ec = oracle.refine(Q64, rows_dense, ids, count, K)
                    res = {}
                    variants = [("f8", ch, "f8", 0), ("f32", c32, "f32", 0), ("f16", c16, "f16", 0)]
                    if d == 128 and B == 256:
                        variants.append(("f8_misaligned", ch, "f8", 1))      # base pointer off by 1 byte: no 16-byte slots
                    for name, ctx, rows, shift in variants:
                        flat = torch.zeros(nq * B * d + 16, dtype=_tdt(rows), device=dev)
                        cand = flat[shift:shift + nq * B * d]
                        assert cand.data_ptr() == flat.data_ptr() + shift * flat.element_size()
                        torch.cuda.synchronize()
                        ctx.store_gather_dev(nq, gidd.data_ptr(), cntd.data_ptr(), B, cand.data_ptr())
                        res[name] = _refine_dev(pkg, ctx, rows, cand, qd, Q, B, idd, cntd, K)
                        if rows == "f8" and K == SHAPE_K[0]:
                            got = cand.cpu().numpy().reshape(nq, B, d)
                            assert np.array_equal(got[live], Xb[gid][live]), tag   # the store's bit patterns, unchanged
                        del flat, cand
                    for name in res:
                        _same(res[name], res["f8"])
                    g = res["f8"]
                    assert np.array_equal(g["ids"], ei) and np.array_equal(_bits(g["dist"]), _bits(ed)) and np.array_equal(g["count"], ec), tag
                    assert np.array_equal(g["scored"], count), tag
                    if (~missing[live]).all():
                        _same(g, a)
            del rows_store, rows_dense


def _dense_case(pkg, oracle, rng, d, B, K, nq, n=6000):
    """A dense block of random store rows per query, F8E4M3, F32 and F16, against the oracle's refine over the same rows as float64."""
    raw = clustered(rng, n, d)(n)
    raw[n // 2:] = raw[rng.integers(0, 40, n - n // 2)]
    Xb, X, X16, X64 = _f8s(raw)
    ids = rng.integers(0, n, (nq, B)).astype(np.int32)
    count = rng.integers(0, B + 1, nq).astype(np.int32)
    count[:3] = (B, 0, B - 1)
    Q = clustered(rng, nq, d)(nq)
    ei, ed, ec = oracle.refine(Q.astype(np.float64), X64[ids], ids, count, K)
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B)
    res = {}
    for rows in ROWS:
        with pkg.FspannContext(cfg, 0) as ctx:
            cand = _dev(_src(rows, Xb, X, X16)[ids])
            res[rows] = _refine_dev(pkg, ctx, rows, cand, _dev(Q), Q, B, _dev(ids), _dev(count), K)
            del cand
    _same(res["f8"], res["f32"])
    _same(res["f8"], res["f16"])
    g = res["f8"]
    assert np.array_equal(g["ids"], ei) and np.array_equal(_bits(g["dist"]), _bits(ed)) and np.array_equal(g["count"], ec)
    assert np.array_equal(g["scored"], count)


def test_dense_runs_of_chunks(pkg, oracle, monkeypatch):
    """B = 8 000, k = 100 over dense fp8 blocks with enough queries that a workgroup walks a RUN of consecutive chunks and keeps the
    running top-k: 48 queries (runs of two chunks, then the merge), and, at one streaming workgroup per CU, 130 queries (a run is
    the whole query: 32 chunks, no merge kernel)."""
    rng = np.random.default_rng(77)
    _dense_case(pkg, oracle, rng, d=64, B=8000, K=100, nq=48)
    monkeypatch.setenv("FSPANN_REFINE_STREAM", "1")
    _dense_case(pkg, oracle, rng, d=64, B=8000, K=100, nq=130)


@pytest.mark.parametrize("knob,val", [("FSPANN_REFINE_STREAM", "0"), ("FSPANN_REFINE_STREAM", "2"), ("FSPANN_REFINE_RUN", "0"),
                                      ("FSPANN_REFINE_DC", "64"), ("FSPANN_REFINE_DC", "128")])
def test_scan_knobs(pkg, oracle, knob, val, monkeypatch):
    """FSPANN_REFINE_STREAM=0: the one-workgroup-per-chunk scan with 16-byte slots, =2: fewer streaming workgroups;
    FSPANN_REFINE_RUN=0: one partial list per chunk and the merge instead of the running top-k; FSPANN_REFINE_DC is an fp32 notion
    that fp8 rows ignore (one tile = 128 bytes = 128 dims)."""
    monkeypatch.setenv(knob, val)
    rng = np.random.default_rng(78)
    _dense_case(pkg, oracle, rng, d=128, B=1024, K=10, nq=20)
    _dense_case(pkg, oracle, rng, d=72, B=256, K=40, nq=20)
    _dense_case(pkg, oracle, rng, d=64, B=2048, K=100, nq=24)         # k > 32, several chunks: where the running top-k applies


# ---- 3. all 256 patterns, special rows, ties -----------------------------------------------------------------------------------
def _refine_all_ways(pkg, ctxs, Xb, X, X16, Q, ids, count, K):
    """refine_store over the F8E4M3, F32 and F16 stores, and refine_dev over dense blocks of all three: all six equal; returns one"""
    nq, B = ids.shape
    a = ctxs["f8"].refine_store(Q, ids, count, K)
    for rows in ("f32", "f16"):
        _same(a, ctxs[rows].refine_store(Q, ids, count, K))
    for rows in ROWS:
        cand = _dev(_src(rows, Xb, X, X16)[ids])
        _same(_refine_dev(pkg, ctxs[rows], rows, cand, _dev(Q), Q, B, _dev(ids), _dev(count), K), a)
        del cand
    return a


@pytest.mark.parametrize("qdtype", [np.float32, np.float64], ids=["q32", "q64"])
@pytest.mark.parametrize("path", ["dense", "store"])
def test_all_256_patterns_through_the_public_path(pkg, path, qdtype):
    """A d = 16 block of 256 rows, row b holding pattern b at position b % 16 and zeros elsewhere, scored against the zero query and
    against a query of ones: the 254 finite rows come back with exactly sqrt(v^2) = |v| and sqrt((1 - v)^2 + 15) — the table's v —
    which fixes the magnitude and the sign of every widened value, subnormals and -0.0 included; rows 0x7F / 0xFF are skipped and
    `scored` says 254.  (For an e4m3 v, v^2 and (1 - v)^2 + 15 are exact in fp64, so the expected distances are the correctly rounded
    square roots numpy gives.)"""
    N = pkg._native
    d, B = 16, 256
    Xb = np.zeros((256, d), np.uint8)
    Xb[np.arange(256), np.arange(256) % d] = np.arange(256, dtype=np.uint8)
    v = TABLE
    fin = np.isfinite(v)
    assert fin.sum() == 254 and not fin[0x7F] and not fin[0xFF]
    Q = np.stack([np.zeros(d), np.ones(d)]).astype(qdtype)
    ids = np.tile(np.arange(256, dtype=np.int32), (2, 1))
    count = np.full(2, B, np.int32)
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as ctx:
        if path == "store":
            ctx.store_set(Xb, dtype=pkg.float8_e4m3fn)
            assert _store_dtype(ctx) == N.F8E4M3
            g = ctx.refine_store(Q, ids, count, B)
        else:
            cand = _dev(Xb[ids])
            g = _refine_dev(pkg, ctx, "f8", cand, _dev(Q), Q, B, _dev(ids), _dev(count), B)
    assert g["scored"].tolist() == [254, 254] and g["count"].tolist() == [254, 254]
    with np.errstate(invalid="ignore"):
        want = [np.sqrt(v * v), np.sqrt((1.0 - v) * (1.0 - v) + 15.0)]
    for qi in range(2):
        got_ids, got_d = g["ids"][qi, :254], g["dist"][qi, :254]
        assert sorted(got_ids.tolist()) == np.flatnonzero(fin).tolist()           # every finite row, neither NaN row
        assert np.array_equal(got_d.view(np.uint64), want[qi][got_ids].view(np.uint64)), (path, qdtype, qi)
        order = sorted(np.flatnonzero(fin).tolist(), key=lambda b: (want[qi][b], b))          # ties (+-v, +-0) by position
        assert got_ids.tolist() == order
    # the zero query tells magnitudes only; the ones query tells signs: v and -v are told apart unless v = 0
    assert want[1][0x38] == np.sqrt(15.0) and want[1][0xB8] == np.sqrt(19.0) and want[1][0x80] == want[1][0x00] == 4.0


@pytest.mark.parametrize("d", [64, 100, 101, 144])
def test_special_values_in_rows(pkg, oracle, d):
    """+-0, +-448 (the largest e4m3), subnormals (rows made of nothing else, such as 2^-9 in every element), every finite pattern
    somewhere, and rows holding a NaN (0x7F or 0xFF) in single elements — the last element of an odd-length row among them — which
    the reference skips (QSI.isValid): in the resident store (gather), in dense blocks, through the vector path (d = 64, 144) and the
    element-wise one (d = 100, 101), against fp32 and fp64 queries.  Against an fp64 query of 1e200 every row is scored with distance
    +inf, as the reference scores it."""
    rng = np.random.default_rng(500 + d)
    n, B, nq = 2048, 512, 8
    Xb = f8_cast(clustered(rng, n, d)(n))
    sub = np.arange(1, 8, dtype=np.uint8)                                # every positive subnormal: m * 2^-9
    Xb[0] = rng.choice(sub, d)                                           # rows made only of subnormals
    Xb[1] = rng.choice(sub, d) | np.uint8(0x80)
    Xb[2] = 0x01                                                         # the smallest one, 2^-9, in every element
    Xb[3] = 0x00
    Xb[4] = 0x80                                                         # -0.0
    Xb[5] = 0x7E                                                         # 448
    Xb[6] = 0xFE
    Xb[7, ::2], Xb[7, 1::2] = 0x00, 0x80
    Xb[8, d - 1] = 0x7F                                                  # NaN in the last element: skipped
    Xb[9, 0] = 0xFF                                                      # the negative NaN
    Xb[10, d // 2] = 0x7F
    Xb[11, 3] = 0xFF
    Xb[12, 1], Xb[12, 2] = 0x7F, 0xFF
    Xb[13, :3] = (0x7E, 0x01, 0x80)
    Xb[14] = rng.permutation(np.resize(FINITE, max(d, 254)))[:d]         # finite patterns of every kind in one row
    Xb[15] = rng.permutation(np.resize(FINITE, max(d, 254)))[:d]
    X64 = widen(Xb)
    X, X16 = X64.astype(np.float32), X64.astype(np.float16)
    bad = ~np.isfinite(X64).all(1)
    assert bad.sum() == 5 and np.array_equal(np.flatnonzero(bad), [8, 9, 10, 11, 12])
    assert np.array_equal(X64[2], np.full(d, 2.0 ** -9)) and X64[5, 0] == 448.0 and np.signbit(X64[4]).all()
    ids = np.stack([16 + rng.permutation(n - 16)[:B] for _ in range(nq)]).astype(np.int32)
    ids[:, :16] = rng.permuted(np.tile(np.arange(16, dtype=np.int32), (nq, 1)), axis=1)      # every query sees every special row
    count = np.full(nq, B, np.int32)
    count[7] = B - 5
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as ch, pkg.FspannContext(cfg, 0) as c32, pkg.FspannContext(cfg, 0) as c16:
        ctxs = dict(f8=ch, f32=c32, f16=c16)
        for rows in ROWS:
            _set_store(pkg, ctxs[rows], rows, Xb, X, X16)
        for qdtype in (np.float32, np.float64):
            Q = clustered(rng, nq, d)(nq).astype(qdtype)
            Q[0] = 0                                                     # at the origin: the subnormal rows and the zeros are its nearest
            Q[1] = qdtype(2.0 ** -9)                                     # distance exactly 0 to row 2
            Q[2] = qdtype(1e-3)
            Q[3] = 448.0                                                 # distance 0 to row 5, 896 sqrt(d) to row 6
            if qdtype == np.float64:
                Q[4] = widen(rng.choice(sub, d)) + 2.0 ** -60
                Q[5] = 1e200                                             # finite, its square is not: every row is scored with distance +inf
            Q64 = Q.astype(np.float64)
            for K in (1, 10, 100):
                ei, ed, ec = oracle.refine(Q64, X64[ids], ids, count, K)
                assert not np.isin(ei, np.flatnonzero(bad)).any()
                if K == 10:      # the origin: the three rows of zeros at distance 0, then the row of 2^-9 at a positive distance
                    assert set(ei[0, :3].tolist()) == {3, 4, 7} and (ed[0, :3] == 0).all() and ei[0, 3] == 2
                    assert ed[0, 3] == np.sqrt(d * 2.0 ** -18) > 0
                    assert ei[1, 0] == 2 and ed[1, 0] == 0.0 and ed[1, 1] > 0
                    assert ei[3, 0] == 5 and ed[3, 0] == 0.0 and np.isfinite(ed[3]).all()
                    if qdtype == np.float64:
                        assert np.isinf(ed[5]).all() and ec[5] == K
                a = _refine_all_ways(pkg, ctxs, Xb, X, X16, Q, ids, count, K)
                assert np.array_equal(a["ids"], ei) and np.array_equal(_bits(a["dist"]), _bits(ed)) and np.array_equal(a["count"], ec), (d, K, qdtype)
                assert np.array_equal(a["scored"], (~bad[ids] & (np.arange(B)[None] < count[:, None])).sum(1))


@pytest.mark.parametrize("active", [16, 4], ids=["d16", "d16_four_live_dims"])
def test_ties_keep_the_order_of_f_q(pkg, oracle, active):
    """With three mantissa bits equal distances are common.  e4m3-valued rows AND e4m3-valued queries (handed over as F32) at
    d = 16 — once with all sixteen dimensions drawn from N(0, 16^2), once with four of them and zeros in the other twelve (the
    vector path still, with the ties of a four-dimensional scene: dozens inside the returned top-k) — so the stable tie order
    (position in F_q) is exercised inside a chunk, across chunk boundaries (B = 1000: four chunks and the merge) and across runs of
    chunks (B = 4000, k = 100, dense), in the store and in dense blocks."""
    rng = np.random.default_rng(91)
    n, d, nq = 4000, 16, 50
    raw, rawq = np.zeros((n, d), np.float32), np.zeros((nq, d), np.float32)
    raw[:, :active] = rng.standard_normal((n, active)) * 16
    rawq[:, :active] = rng.standard_normal((nq, active)) * 16
    Xb, X, X16, X64 = _f8s(raw)
    _, Q, _, Q64 = _f8s(rawq)
    dd = np.sqrt(((Q64[:, None, :] - X64[None, :, :]) ** 2).sum(2))
    repeats = dd.size - sum(len(np.unique(r)) for r in dd)               # per query: distances that repeat an earlier one
    assert repeats > (300 if active == 16 else 8000), repeats
    ties = 0
    for B, K in ((256, 10), (1000, 100), (4000, 100)):
        ids = np.stack([rng.permutation(n)[:B] for _ in range(nq)]).astype(np.int32)
        count = np.full(nq, B, np.int32)
        count[1] = B - 7
        ei, ed, ec = oracle.refine(Q64, X64[ids], ids, count, K)
        ties += sum(len(r) - len(np.unique(r)) for r in ed)              # ties inside the returned top-k itself
        cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B)
        with pkg.FspannContext(cfg, 0) as ch, pkg.FspannContext(cfg, 0) as c32, pkg.FspannContext(cfg, 0) as c16:
            ctxs = dict(f8=ch, f32=c32, f16=c16)
            for rows in ROWS:
                _set_store(pkg, ctxs[rows], rows, Xb, X, X16)
            a = _refine_all_ways(pkg, ctxs, Xb, X, X16, Q, ids, count, K)
        assert np.array_equal(a["ids"], ei) and np.array_equal(_bits(a["dist"]), _bits(ed)) and np.array_equal(a["count"], ec), (B, K)
        assert np.array_equal(a["scored"], count)
    assert ties >= (1 if active == 16 else 50), ties


# ---- 4. queries that are not finite, and an fp64 query whose squares overflow --------------------------------------------------
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
    with _ctx(pkg, sc, "f8") as ch, _ctx(pkg, sc, "f32") as c32, _ctx(pkg, sc, "f16") as c16:
        gh = _search(pkg, ch, Q, B, K, call="retry")
        assert (gh["bad"][~finite] == 1).all() and (gh["scored"][~finite] == 0).all()
        for cw in (c32, c16):
            gw = _search(pkg, cw, Q, B, K, call="retry")
            for k in gh:
                if k in ("sel", "selc"):
                    assert np.array_equal(gh[k][finite], gw[k][finite]), k
                else:
                    assert np.array_equal(_bits(gh[k]), _bits(gw[k])), k
        _same_as_oracle(gh, ref, B, finite)
        # the scan alone (refine_store: the per-query check of an fp64 query, the sum's of an fp32 one)
        rt = ch.route(codes, limit=B, counters=False)
        a = ch.refine_store(Q, rt["ids"][:, :B], rt["count"], K)
        _same(a, c32.refine_store(Q, rt["ids"][:, :B], rt["count"], K))
        _same(a, c16.refine_store(Q, rt["ids"][:, :B], rt["count"], K))
        nr = ref["metrics"][:, 4] == 0                                   # (a retried query's answer is its second pass')
        assert np.array_equal(a["ids"][nr], ref["ids"][nr]) and np.array_equal(_bits(a["dist"][nr]), _bits(ref["dist"][nr]))
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
    """Route as a tick with a hand-over buffer (a tiny entry budget: queries stay PENDING), then a refine-only tick over fp8 rows: the
    scan's own workgroups finish the PENDING queries first (refine_stream_fix_kernel<fsp_f8e4m3, GATHER>: one launch, last_tick_fused)."""
    import torch
    monkeypatch.setenv("FSPANN_ROUTE_LAZY_CAP", "258")
    B, K, nq, d = 256, 10, 96, 16
    sc = _scene(oracle, n=40000, d=d, T=10, D=1, m=12, lam=2, B=B, seed=23)
    o, p = sc["o"], sc["p"]
    Q = _queries(sc, nq, np.float32)
    ref = o.search(Q.astype(np.float64), K)
    assert not ref["metrics"][:, 4].any()
    out = {}
    for rows in ROWS:
        with _ctx(pkg, sc, rows) as ctx:
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
                cand = _dev(_src(rows, sc["Xb"], sc["X"], sc["X16"])[np.clip(ids_h, 0, p["n"] - 1)])
                torch.cuda.synchronize()
            ctx.tick_dev(None, None, dict(nq=nq, q=qd.data_ptr(), B=B, ids=t["sel"].data_ptr(), count=t["selc"].data_ptr(), k=K,
                                          out_ids=t["ids"].data_ptr(), out_dist=t["dist"].data_ptr(), out_count=t["count"].data_ptr(),
                                          scored=t["scored"].data_ptr(), cand=cand.data_ptr() if dense else None,
                                          cand_dtype=_cdt(pkg, rows), codes=t["codes"].data_ptr(), handover=t["hov"].data_ptr()))
            ctx.sync()
            assert ctx.last_tick_fused()                                  # one launch: the scan finished the PENDING queries itself
            assert ctx.unmodelled_queries() == 0
            g = {k: t[k].cpu().numpy() for k in ("ids", "dist", "count", "scored", "sel", "selc")}
            g["sel"] = np.where(np.arange(B)[None] < g["selc"][:, None], g["sel"], -1)
            out[rows] = g
            del cand
    _same(out["f8"], out["f32"])
    _same(out["f8"], out["f16"])
    _same_as_oracle(out["f8"], ref, B)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "gather"])
def test_three_role_tick_over_f8_rows_runs_unfused(pkg, oracle, dense):
    """tick_kernel is fp32-only: encode + Route + Refine over fp8 rows in one tick_dev call run as stand-alone kernels in stream
    order (fspann_last_tick_fused() == 0) and give the arrays each part gives alone; the same tick over F32 rows fuses."""
    import torch
    B, K, nq, d = 256, 10, 128, 64
    sc = _scene(oracle, n=30000, d=d, T=8, D=1, m=12, lam=2, B=B, seed=5)
    o, p = sc["o"], sc["p"]
    Qa, Qb, Qc = (_queries(sc, nq, np.float32) for _ in range(3))
    ref_a, ref_b = o.search(Qa.astype(np.float64), K), o.search(Qb.astype(np.float64), K)
    assert not ref_a["metrics"][:, 4].any()
    out = {}
    for rows in ROWS:
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
                cand = _dev(_src(rows, sc["Xb"], sc["X"], sc["X16"])[np.clip(ta["sel"].cpu().numpy(), 0, p["n"] - 1)])
                torch.cuda.synchronize()
            ctx.tick_dev(dict(nq=nq, q=qc.data_ptr(), codes=tc["codes"].data_ptr(), bad=tc["bad"].data_ptr()),
                         dict(nq=nq, codes=tb["codes"].data_ptr(), limit=B, ids=tb["sel"].data_ptr(), count=tb["selc"].data_ptr()),
                         dict(nq=nq, q=qa.data_ptr(), B=B, ids=ta["sel"].data_ptr(), count=ta["selc"].data_ptr(), k=K, out_ids=ta["ids"].data_ptr(),
                              out_dist=ta["dist"].data_ptr(), out_count=ta["count"].data_ptr(), scored=ta["scored"].data_ptr(),
                              cand=cand.data_ptr() if dense else None, cand_dtype=_cdt(pkg, rows)))
            ctx.sync()
            assert ctx.L.fspann_last_tick_fused(ctx.handle) == (1 if rows == "f32" else 0)
            g = {k: ta[k].cpu().numpy() for k in ("ids", "dist", "count", "scored", "sel", "selc")}
            g["sel"] = np.where(np.arange(B)[None] < g["selc"][:, None], g["sel"], -1)
            g["codes_c"] = tc["codes"].cpu().numpy().view(np.uint64)
            g["bad_c"] = tc["bad"].cpu().numpy()
            g["selc_b"] = tb["selc"].cpu().numpy()
            g["sel_b"] = np.where(np.arange(B)[None] < g["selc_b"][:, None], tb["sel"].cpu().numpy(), -1)
            out[rows] = g
            del cand
    _same(out["f8"], out["f32"])
    _same(out["f8"], out["f16"])
    g = out["f8"]
    _same_as_oracle({k: g[k] for k in ("ids", "dist", "count", "scored", "sel", "selc")}, ref_a, B)
    assert np.array_equal(g["codes_c"], o.encode(Qc.astype(np.float64))) and not g["bad_c"].any()
    assert np.array_equal(g["selc_b"], ref_b["sel_count"]) and np.array_equal(g["sel_b"], ref_b["sel"][:, :B])


# ---- 6. touch tracking ---------------------------------------------------------------------------------------------------------
def test_touched_set_equals_the_f32_and_f16_contexts(pkg, oracle):
    """searches (both passes) and a dense block over a store in which some rows hold a NaN: the touched handles are those of the
    F32 and F16 contexts holding the same values, and no skipped row is among them (a one-byte row is NOT always finite)."""
    B, K, nq = 256, 100, 128
    sc = _scene(oracle, B=B, seed=4)
    n = sc["p"]["n"]
    # the index stays that of the clean rows; the STORE gets rows that cannot be scored
    Sb = sc["Xb"].copy()
    badrows = np.arange(0, n, 7)
    Sb[badrows[0::2], 5] = np.uint8(0x7F)
    Sb[badrows[1::2], 0] = np.uint8(0xFF)
    S64 = widen(Sb)
    S32, S16 = S64.astype(np.float32), S64.astype(np.float16)
    Q = _queries(sc, nq, np.float32)
    Q[5, 3] = np.nan
    drained = {}
    for rows in ROWS:
        with _ctx(pkg, sc, rows, store=False) as ctx:
            _set_store(pkg, ctx, rows, Sb, S32, S16)
            ctx.touch_enable()
            g = _search(pkg, ctx, Q, B, K, call="retry")
            s1 = ctx.drain_touched()
            # dense rows handed over by the caller (touch_mark over a block)
            sel = np.where(g["sel"] >= 0, g["sel"], 0)
            cand = _dev(_src(rows, Sb, S32, S16)[sel])
            _refine_dev(pkg, ctx, rows, cand, _dev(Q), Q, B, _dev(g["sel"]), _dev(np.maximum(g["selc"], 0)), K)
            s2 = ctx.drain_touched()
            drained[rows] = (s1, s2, g)
            del cand
    assert len(drained["f8"][0]) > 0 and len(drained["f8"][1]) > 0
    for rows in ("f32", "f16"):
        assert np.array_equal(drained["f8"][0], drained[rows][0])
        assert np.array_equal(drained["f8"][1], drained[rows][1])
        _same(drained["f8"][2], drained[rows][2])
    g = drained["f8"][2]
    fin = np.isfinite(Q).all(1)
    routed = set(g["sel"][fin][g["sel"][fin] >= 0].tolist())
    assert routed & set(badrows.tolist()), "no skipped row was routed: the test shows nothing"
    for s in drained["f8"][:2]:
        assert not set(s.tolist()) & set(badrows.tolist())
    # the last pass' F_q of every finite query, less the rows that cannot be scored, is in the set of the search
    assert routed - set(badrows.tolist()) <= set(drained["f8"][0].tolist())


# ---- 7. Setup input --------------------------------------------------------------------------------------------------------------
def test_build_from_f8_gives_the_same_tables(pkg, oracle):
    sc = _scene(oracle, n=30000, d=128, T=4, D=4, m=16, lam=2, seed=6)
    o, p = sc["o"], sc["p"]
    TD = p["T"] * p["D"]
    with _ctx(pkg, sc, "f8", store=False) as ch, _ctx(pkg, sc, "f32", store=False) as c32, _ctx(pkg, sc, "f16", store=False) as c16, \
            _ctx(pkg, sc, "f8", store=False, build=False) as cc:
        cc.build_begin(p["n"])
        for lo, hi in ((0, 1), (1, 4098), (4098, 17001), (17001, p["n"])):      # chunks of uneven sizes (odd element counts too)
            cc.build_append(sc["Xb"][lo:hi], dtype=pkg.float8_e4m3fn)
        cc.build_finish()
        for td in range(TD):
            want = o.get_index(td)
            for ctx in (ch, c32, c16, cc):
                got = ctx.get_index(td)
                assert all(np.array_equal(got[k], want[k]) for k in want), td


def test_build_from_f8_odd_dim(pkg, oracle):
    """d = 27: n * d is not a multiple of the four elements a thread widens, and rows start at every byte offset"""
    sc = _scene(oracle, n=5001, d=27, T=3, D=2, m=10, lam=2, seed=16)
    o, p = sc["o"], sc["p"]
    with _ctx(pkg, sc, "f8", store=False) as ch:
        for td in range(p["T"] * p["D"]):
            want, got = o.get_index(td), ch.get_index(td)
            assert all(np.array_equal(got[k], want[k]) for k in want), td


# ---- 8. metrics ------------------------------------------------------------------------------------------------------------------
def test_metrics_over_an_f8_base(pkg, oracle):
    """recall@k and ratio@k over an F8E4M3 base with F32 queries: the bits fspann_eval_metrics_dev gives over the same base widened to
    fp32, the bits the F16 base gives (and the reference's computeMetricsAtK), straight from a resident fp8 store."""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    rng = np.random.default_rng(3)
    n, d, nq, k = 4000, 24, 64, 10
    Xb, X, X16, _ = _f8s(clustered(rng, n, d)(n))
    Q = clustered(rng, nq, d)(nq)
    Q[5] = X[17]                                             # distance 0 to its nearest neighbour: ratio is NaN there
    gt, _ = oracle.groundtruth(X, Q, 20)
    ann = gt[:, :12].copy()
    for i in range(nq):                                      # an approximate answer: some true neighbours replaced
        m = rng.random(12) < 0.4
        ann[i, m] = rng.integers(0, n, int(m.sum()))
    cnt = np.full(nq, 12, np.int32)
    cnt[3], cnt[9] = 7, 0                                    # fewer than k results: ratio NaN, recall over what exists
    ann[11, 2] = -1                                          # an unparsable id
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=64)
    with pkg.FspannContext(cfg, 0) as ctx:
        ctx.store_set(Xb, dtype=pkg.float8_e4m3fn)
        dt = C.c_int(-1)
        ctx.L.fspann_store_dev_ptr.restype = C.c_void_p
        store_ptr = ctx.L.fspann_store_dev_ptr(ctx.handle, C.byref(dt))
        assert dt.value == N.F8E4M3
        xh, x32, x16, qd, ad, cd, gd = _dev(Xb), _dev(X), _dev(X16), _dev(Q), _dev(ann), _dev(cnt), _dev(gt)
        out = {}
        for name, base, bdt in (("store", store_ptr, N.F8E4M3), ("tensor", xh.data_ptr(), N.F8E4M3), ("typed_f32", x32.data_ptr(), N.F32),
                                ("typed_f16", x16.data_ptr(), N.F16), ("f32", x32.data_ptr(), None)):
            rec = torch.full((nq,), -1.0, dtype=torch.float64, device=dev)
            rat = torch.full((nq,), -1.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            if bdt is None:
                ctx.eval_metrics_dev(n, base, nq, qd.data_ptr(), d, k, ad.data_ptr(), 12, cd.data_ptr(), gd.data_ptr(), 20, rec.data_ptr(), rat.data_ptr())
            else:
                ctx.eval_metrics_typed_dev(n, base, bdt, nq, qd.data_ptr(), N.F32, d, k, ad.data_ptr(), 12, cd.data_ptr(), gd.data_ptr(), 20,
                                           rec.data_ptr(), rat.data_ptr())
            ctx.sync()
            out[name] = (rec.cpu().numpy(), rat.cpu().numpy())
    for name in ("store", "tensor", "typed_f32", "typed_f16"):
        assert np.array_equal(out[name][0].view(np.uint64), out["f32"][0].view(np.uint64)), name
        assert np.array_equal(out[name][1].view(np.uint64), out["f32"][1].view(np.uint64)), name       # NaN bits included
    rec, rat = out["store"]
    ref_rec, ref_rat = oracle.metrics(X, Q, k, ann, cnt, gt)
    assert np.array_equal(rec, ref_rec)
    assert np.array_equal(np.isnan(rat), np.isnan(ref_rat)) and np.isnan(rat[[3, 5, 9, 11]]).all()
    ok = ~np.isnan(rat)
    assert ok.sum() == nq - 4 and np.array_equal(rat[ok], ref_rat[ok])


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_f8_is_refused_where_it_cannot_stand(pkg, oracle):
    """every query dtype, the point store, the ground truth and metrics with another query type: FSPANN_E_ARG, the message names
    FSPANN_F8E4M3"""
    import torch
    N = pkg._native
    F8 = N.F8E4M3
    dev = torch.device("cuda", 0)
    B, K, nq = 64, 5, 8
    sc = _scene(oracle, n=4000, d=32, T=2, D=2, m=8, lam=2, B=B, seed=8)
    p = sc["p"]
    Qh = sc["Xb"][:nq].copy()
    with _ctx(pkg, sc, "f8") as ctx:
        L, h = ctx.L, ctx.handle
        err = lambda: L.fspann_last_error().decode()
        qd = _dev(Qh)
        t = _bufs(nq, B, K)
        codes = torch.zeros((nq, p["T"] * p["D"], 1), dtype=torch.int64, device=dev)
        cand = torch.zeros((nq, B, p["d"]), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        out = (t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr())
        sel = (t["sel"].data_ptr(), t["selc"].data_ptr())
        calls = [
            lambda: ctx.refine_store_dev(nq, qd.data_ptr(), F8, B, *sel, K, *out),
            lambda: ctx.refine_dev(nq, qd.data_ptr(), F8, cand.data_ptr(), F8, B, *sel, K, *out),
            lambda: ctx.refine_dev(nq, qd.data_ptr(), F8, cand.data_ptr(), N.F32, B, *sel, K, *out),
            lambda: ctx.search_store_dev(nq, qd.data_ptr(), F8, -1, B, K, *out, *sel),
            lambda: ctx.search_store_finish_dev(nq, qd.data_ptr(), F8, -1, B, K, *out, *sel),
            lambda: ctx.search_retry_dev(nq, qd.data_ptr(), F8, -1, B, K, *out, *sel),
            lambda: ctx.search_retry_finish_dev(nq, qd.data_ptr(), F8, -1, B, K, *out, *sel),
            lambda: ctx.encode_dev(nq, qd.data_ptr(), F8, codes.data_ptr()),
            lambda: ctx.tick_dev(None, None, dict(nq=nq, q=qd.data_ptr(), q_dtype=F8, B=B, ids=sel[0], count=sel[1], k=K,
                                                  out_ids=out[0], out_dist=out[1], out_count=out[2])),
            lambda: ctx.tick_dev(None, None, dict(nq=nq, q=qd.data_ptr(), q_dtype=F8, B=B, ids=sel[0], count=sel[1], k=K, cand=cand.data_ptr(),
                                                  cand_dtype=F8, out_ids=out[0], out_dist=out[1], out_count=out[2])),
            lambda: ctx.tick_dev(dict(nq=nq, q=qd.data_ptr(), dtype=F8, codes=codes.data_ptr()), None, None),
        ]
        for i, call in enumerate(calls):
            with pytest.raises(pkg.FspannArgumentError, match="FSPANN_F8E4M3"):
                call()
            ctx.sync()
        # host-pointer entry points, straight through the C ABI
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        hc = np.zeros((nq, p["T"] * p["D"], 1), np.uint64)
        assert L.fspann_encode(h, nq, vp(Qh), F8, vp(hc), None) == N.E_ARG and "FSPANN_F8E4M3" in err()
        hcand = np.zeros((nq, B, p["d"]), np.uint8)
        hi, hn = np.zeros((nq, B), np.int32), np.zeros(nq, np.int32)
        oi, od, oc = np.zeros((nq, K), np.int32), np.zeros((nq, K), np.float64), np.zeros(nq, np.int32)
        assert L.fspann_refine(h, nq, vp(Qh), vp(hcand), F8, B, vp(hi), vp(hn), K, vp(oi), vp(od), vp(oc), None) == N.E_ARG
        assert "FSPANN_F8E4M3" in err()
        assert L.fspann_refine_store(h, nq, vp(Qh), F8, B, vp(hi), vp(hn), K, vp(oi), vp(od), vp(oc), None) == N.E_ARG
        assert "FSPANN_F8E4M3" in err() and "q_dtype" in err()
        ps = C.c_void_p()
        N.check(L.fspann_pointstore_create(100, p["d"], C.byref(ps)))
        try:
            key = np.arange(32, dtype=np.uint8)
            N.check(L.fspann_pointstore_set_master_key(ps, vp(key)))
            assert L.fspann_pointstore_encrypt(ps, 0, 4, vp(hcand), F8, 1) == N.E_ARG and "FSPANN_F8E4M3" in err()
            assert L.fspann_pointstore_open_batch(ps, nq, B, vp(hi), vp(hn), vp(hcand), F8, vp(hi.copy()), vp(hn.copy()), 1) == N.E_ARG
            assert "FSPANN_F8E4M3" in err()
        finally:
            L.fspann_pointstore_destroy(ps)
        # ground truth: never over fp8; metrics: an F8E4M3 base only with F32 queries, an F8E4M3 query never
        buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        o64 = torch.zeros(4096, dtype=torch.float64, device=dev)
        b, o = buf.data_ptr(), o64.data_ptr()
        torch.cuda.synchronize()
        for bdt, qdt in ((F8, F8), (F8, N.F32), (N.F32, F8), (N.U8, F8), (F8, N.U8), (F8, N.F64)):
            assert L.fspann_groundtruth_typed_dev(h, 10, b, bdt, 2, b, qdt, 16, 5, o, o + 16384) == N.E_ARG and "FSPANN_F8E4M3" in err(), (bdt, qdt)
        mt = lambda bdt, qdt: L.fspann_eval_metrics_typed_dev(h, 10, b, bdt, 2, b, qdt, 16, 5, o, 8, None, o, 8, o, o)
        for bdt, qdt in ((F8, F8), (F8, N.F64), (F8, N.U8), (N.F32, F8), (N.U8, F8)):
            assert mt(bdt, qdt) == N.E_ARG and "FSPANN_F8E4M3" in err(), (bdt, qdt)
        # a pair with a half or a bfloat16 in it keeps the name it had: the new checks stand behind the existing ones
        for bdt, qdt, name in ((F8, N.F16, "FSPANN_F16"), (N.F16, F8, "FSPANN_F16"), (F8, N.BF16, "FSPANN_BF16"), (N.BF16, F8, "FSPANN_BF16")):
            assert L.fspann_groundtruth_typed_dev(h, 10, b, bdt, 2, b, qdt, 16, 5, o, o + 16384) == N.E_ARG and name in err(), (bdt, qdt)
            assert mt(bdt, qdt) == N.E_ARG and name in err(), (bdt, qdt)
        assert mt(F8, N.F32) == N.OK                                    # (the accepted pair, same buffers)
        ctx.sync()
        # accepted where a ROW dtype is given: the same calls with a query dtype the library takes
        ctx.refine_dev(nq, _dev(sc["X"][:nq]).data_ptr(), N.F32, cand.data_ptr(), F8, B, *sel, K, *out)
        ctx.sync()


def test_store_set_never_rounds(pkg, oracle):
    """store_set(x, dtype=pkg.float8_e4m3fn): a CPU torch.float8_e4m3fn tensor as it is, a uint8 array as bit patterns, a float array
    only if every value already is an e4m3 value; anything else raises and the store set before stays untouched.  The ways of handing
    over the same rows give the same store.  Without dtype a uint8 array is widened to float64, and dtype=np.uint8 is FSPANN_U8, as
    before."""
    import torch
    N = pkg._native
    d = 16
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=64)
    rng = np.random.default_rng(1)
    F8 = pkg.float8_e4m3fn
    with pkg.FspannContext(cfg, 0) as ctx:
        x = np.full((8, d), np.float32(0.5))
        ctx.store_set(x, dtype=F8)                                     # 0.5 is an e4m3 value
        assert _store_dtype(ctx) == N.F8E4M3 and ctx.store_dtype is F8
        for bad in (np.float32(0.1), np.float32(1.0 + 2.0 ** -4), np.float64(2.0 ** -10), np.float32(449.0), np.float64(1e6), np.float32(np.inf),
                    np.float64(-np.inf), np.float16(1.0 + 2.0 ** -10)):
            y = x.astype(np.asarray(bad).dtype).copy()
            y[3, 7] = bad
            with pytest.raises(pkg.FspannArgumentError, match="float8_e4m3fn"):
                ctx.store_set(y, dtype=F8)
            assert _store_dtype(ctx) == N.F8E4M3 and ctx.store_dtype is F8               # the store set before is untouched
        ctx.store_set(x)
        assert _store_dtype(ctx) == N.F32
        with pytest.raises(pkg.FspannArgumentError):
            ctx.store_set(np.full((8, d), np.float32(0.1)), dtype=F8)
        assert _store_dtype(ctx) == N.F32 and ctx.store_dtype == np.float32            # ... whatever its type
        with pytest.raises(pkg.FspannArgumentError):
            ctx.store_set(np.full((8, d), 3, np.int64), dtype=F8)                      # integers are neither bit patterns nor floats
        with pytest.raises(pkg.FspannArgumentError):
            ctx.store_set(torch.full((8, d), 0.5, dtype=torch.float32), dtype=F8)      # a float32 tensor is not fp8 rows
        assert _store_dtype(ctx) == N.F32
        y = x.copy()
        y[0, 0], y[3, 3], y[4, 4], y[5, 5], y[6, 6] = np.nan, np.float32(2.0 ** -9), np.float32(-0.0), np.float32(448.0), np.float32(-448.0)
        ctx.store_set(y, dtype=F8)                                     # NaN is NaN; subnormals and the top of the range are e4m3 values
        assert _store_dtype(ctx) == N.F8E4M3
        # the same rows as float32 / float64 / float16 values, as bit patterns and as a torch.float8_e4m3fn tensor: one store
        b = f8_cast((rng.standard_normal((64, d)) * 16).astype(np.float32))
        b[5, 3], b[6, 0], b[7, 1], b[8, 2] = 0x01, 0x7E, 0x80, 0x7F
        v = widen(b)
        Q = rng.standard_normal((4, d), dtype=np.float32)
        ids = np.tile(np.arange(64, dtype=np.int32), (4, 1))
        cnt = np.full(4, 64, np.int32)
        got = []
        for rows in (b, v.astype(np.float32), v, v.astype(np.float16), torch.from_numpy(b).view(torch.float8_e4m3fn),
                     torch.from_numpy(v.astype(np.float32)).to(torch.float8_e4m3fn)):
            ctx.store_set(rows, dtype=F8)
            assert _store_dtype(ctx) == N.F8E4M3 and ctx.store_dtype is F8
            got.append(ctx.refine_store(Q, ids, cnt, 10))
        ctx.store_set(v.astype(np.float32))
        want = ctx.refine_store(Q, ids, cnt, 10)
        assert (want["scored"] == 63).all()                            # row 8 holds a NaN
        for g in got:
            _same(g, want)
        ctx.store_set(b)                                               # no dtype: a uint8 array is widened to float64, as before
        assert _store_dtype(ctx) == N.F64 and ctx.store_dtype == np.float64
        ctx.store_set(b, dtype=np.uint8)                               # and dtype=np.uint8 is still FSPANN_U8: the integers 0..255
        assert _store_dtype(ctx) == N.U8 and ctx.store_dtype == np.uint8
