"""GPU: every transport of the four host-pointer calls (fspann_encode / fspann_route / fspann_refine / fspann_refine_store) against the
call's _dev twin over device copies of the same inputs, bit for bit; one case per call also against the oracle.

A host-pointer call moves its arguments one of three ways (csrc/host_staging.h): through the mapped pinned block (a handful of
queries, no copy command), through the pinned block with one copy command each way, or by one copy per argument straight from and
to the caller's memory.  Which one a call takes depends on its byte counts, nq and FSPANN_ZERO_COPY (read when the context is
created, so it is set before _ctx()).  The cases below are sized to land on each of them:

  encode        nq = 1 mapped | nq = 1, FSPANN_ZERO_COPY=0 direct | nq = 5 direct; with and without hashes
  route         nq = 1, limit = B mapped | nq = 1, FSPANN_ZERO_COPY=0 block | nq = 5 block | nq = 1, cap = 140 000 (two lists of
                560 000 bytes > 1 MiB) direct; counters on and off
  refine        nq = 1, B = 64 mapped | nq = 1, B = 2100 (ids 8400 bytes > 8192) block | nq = 1, B = 262 148 (ids > 1 MiB) direct
  refine_store  nq = 1 and nq = 5 (always direct)

and two cases of the kernel-attached scan timing: which dispatches count as "a scan that may be timed"."""
import numpy as np
import pytest

from conftest import make_scene

pytestmark = pytest.mark.gpu

K = 10


@pytest.fixture(scope="module")
def scene(oracle):
    return make_scene(oracle, n=2000, d=8, T=2, D=2, m=6, lam=2, B=64)


def _ctx(pkg, sc, store=False):
    p = sc["params"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 max_global_candidates=p["hard_cap"], probe_override=p["probe_override"])
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
    ctx.set_id_meta(p["n"])
    ctx.build_index(sc["X"])
    if store:
        ctx.store_set(sc["X"])
    return ctx


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _empty(shape, dtype):
    import torch
    t = torch.zeros(shape, dtype=dtype, device="cuda")
    torch.cuda.synchronize()          # (the library runs on the context's own stream: the fill has landed before it writes)
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _queries(sc, nq, dtype, seed):
    return np.random.default_rng(seed).standard_normal((nq, sc["params"]["d"])).astype(np.float32).astype(dtype)


# ---- encode ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zero_copy,nq", [("1", 1), ("0", 1), ("1", 5)])
@pytest.mark.parametrize("want_hashes", [False, True])
def test_encode_equals_encode_dev(pkg, scene, monkeypatch, zero_copy, nq, want_hashes):
    import torch
    monkeypatch.setenv("FSPANN_ZERO_COPY", zero_copy)
    sc, N = scene, pkg._native
    for dtype, code in ((np.float64, N.F64), (np.float32, N.F32)):
        Q = _queries(sc, nq, dtype, 11 + nq)
        with _ctx(pkg, sc) as ctx:
            got = ctx.encode(Q, want_hashes=want_hashes)
            codes, hs = got if want_hashes else (got, None)
            qd = _dev(Q)
            cd = _empty(codes.shape, torch.int64)
            hd = _empty((nq, ctx.TD, ctx.cfg.m), torch.int32)
            bd = _empty((nq,), torch.int32)
            ctx.encode_dev(nq, qd.data_ptr(), code, cd.data_ptr(), hd.data_ptr() if want_hashes else 0, bd.data_ptr())
            assert np.array_equal(codes, _host(cd).view(np.uint64))
            assert not _host(bd).any()
            if want_hashes:
                assert np.array_equal(hs, _host(hd))
                assert np.array_equal(hs, sc["oracle"].hashes(Q.astype(np.float64)))
            assert np.array_equal(codes, sc["oracle"].encode(Q.astype(np.float64)))
            # a NaN is refused on this transport too, and the call after it is answered
            bad = Q.copy()
            bad[nq - 1, 2] = np.nan
            with pytest.raises(ValueError):
                ctx.encode(bad, want_hashes=want_hashes)
            assert np.array_equal(ctx.encode(Q), codes)


# ---- route -------------------------------------------------------------------------------------------------------------------

def _route_dev(ctx, codes, limit, cap, counters):
    import torch
    nq = codes.shape[0]
    cd = _dev(codes.view(np.int64))
    ids, score = _empty((nq, cap), torch.int32), _empty((nq, cap), torch.int32)
    cnt, kept, raw = (_empty((nq,), torch.int32) for _ in range(3))
    ctx.route_dev(nq, cd.data_ptr(), -1, limit, cap, ids.data_ptr(), score.data_ptr(), cnt.data_ptr(), kept.data_ptr() if counters else 0,
                  raw.data_ptr() if counters else 0)
    out = dict(ids=_host(ids), score=_host(score), count=_host(cnt))
    if counters:
        out.update(kept=_host(kept), raw_seen=_host(raw))
    return out


@pytest.mark.parametrize("zero_copy,nq,cap", [("1", 1, None), ("0", 1, None), ("1", 5, None), ("1", 1, 140000)],
                         ids=["mapped", "block-zc-off", "block-nq5", "direct-cap140000"])
@pytest.mark.parametrize("counters", [True, False])
def test_route_equals_route_dev(pkg, scene, monkeypatch, zero_copy, nq, cap, counters):
    monkeypatch.setenv("FSPANN_ZERO_COPY", zero_copy)
    sc = scene
    B, o = sc["params"]["B"], sc["oracle"]
    codes = o.encode(_queries(sc, nq, np.float64, 21 + nq))
    ids_o, score_o, count_o, raw_o = o.route(codes)
    with _ctx(pkg, sc) as ctx:
        cap_eff = cap if cap else B
        got = ctx.route(codes, limit=B, cap=cap_eff, counters=counters)
        want = _route_dev(ctx, codes, B, cap_eff, counters)
        assert np.array_equal(got["count"], want["count"]) and (got["count"] >= 0).all()
        assert np.array_equal(got["count"], np.minimum(count_o, B))
        for j in range(nq):
            c = got["count"][j]
            assert np.array_equal(got["ids"][j, :c], want["ids"][j, :c]) and np.array_equal(got["ids"][j, :c], ids_o[j, :c])
            assert np.array_equal(got["score"][j, :c], want["score"][j, :c]) and np.array_equal(got["score"][j, :c], score_o[j, :c])
        if counters:
            assert np.array_equal(got["kept"], want["kept"]) and np.array_equal(got["raw_seen"], want["raw_seen"])
            assert np.array_equal(got["raw_seen"], raw_o)


# ---- refine ------------------------------------------------------------------------------------------------------------------

def _refine_dev(pkg, ctx, Q, rows, ids, cnt, k):
    import torch
    N = pkg._native
    nq, B, _ = rows.shape
    code = N.F64 if rows.dtype == np.float64 else N.F32
    qd, rd, idd, cd = _dev(Q), _dev(rows), _dev(ids), _dev(cnt)
    oi, od = _empty((nq, k), torch.int32), _empty((nq, k), torch.float64)
    oc, sc = _empty((nq,), torch.int32), _empty((nq,), torch.int32)
    ctx.refine_dev(nq, qd.data_ptr(), code, rd.data_ptr(), code, B, idd.data_ptr(), cd.data_ptr(), k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                   sc.data_ptr())
    return dict(ids=_host(oi), dist=_host(od), count=_host(oc), scored=_host(sc))


def _same(a, b):
    for key in ("ids", "dist", "count", "scored"):
        assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key


@pytest.mark.parametrize("B,count,dtype", [(64, 50, np.float64), (2100, 64, np.float64), (262148, 300, np.float32)],
                         ids=["mapped-B64", "block-B2100", "direct-B262148"])
def test_refine_equals_refine_dev(pkg, oracle, scene, B, count, dtype):
    sc = scene
    n, d = sc["params"]["n"], sc["params"]["d"]
    rng = np.random.default_rng(31 + B)
    Q = _queries(sc, 1, dtype, 32)
    ids = rng.integers(0, n, (1, B)).astype(np.int32)
    ids[0, :count] = rng.choice(n, count, replace=False)     # (distinct among the scored rows: no tie between equal ids)
    cnt = np.array([count], np.int32)
    rows = np.full((1, B, d), np.nan, dtype)          # rows beyond the count are NaN: they are never scored
    rows[0, :count] = sc["X"][ids[0, :count]].astype(dtype)
    with _ctx(pkg, sc) as ctx:
        got = ctx.refine(Q, rows, ids, cnt, K)
        _same(got, _refine_dev(pkg, ctx, Q, rows, ids, cnt, K))
    assert got["count"][0] == K and got["scored"][0] == count and np.isfinite(got["dist"]).all()
    o_ids, o_dist, o_count = oracle.refine(Q.astype(np.float64), np.nan_to_num(rows.astype(np.float64)), ids, cnt, K)
    assert np.array_equal(got["ids"], o_ids) and np.array_equal(got["dist"], o_dist) and np.array_equal(got["count"], o_count)


# ---- refine_store ------------------------------------------------------------------------------------------------------------

def _refine_store_dev(pkg, ctx, Q, ids, cnt, k, tensors=None):
    import torch
    N = pkg._native
    nq, B = ids.shape
    code = N.F64 if Q.dtype == np.float64 else N.F32
    t = tensors or dict(q=_dev(Q), ids=_dev(ids), cnt=_dev(cnt), oi=_empty((nq, k), torch.int32), od=_empty((nq, k), torch.float64),
                        oc=_empty((nq,), torch.int32), sc=_empty((nq,), torch.int32))
    ctx.refine_store_dev(nq, t["q"].data_ptr(), code, B, t["ids"].data_ptr(), t["cnt"].data_ptr(), k, t["oi"].data_ptr(), t["od"].data_ptr(),
                         t["oc"].data_ptr(), t["sc"].data_ptr())
    return t


@pytest.mark.parametrize("nq", [1, 5])
def test_refine_store_equals_refine_store_dev(pkg, oracle, scene, nq):
    sc = scene
    n, d, B = sc["params"]["n"], sc["params"]["d"], 100        # (B no multiple of 16)
    rng = np.random.default_rng(41 + nq)
    ids = np.stack([rng.permutation(n)[:B] for _ in range(nq)]).astype(np.int32)
    cnt = rng.integers(K, B + 1, nq).astype(np.int32)
    with _ctx(pkg, sc, store=True) as ctx:
        for dtype in (np.float64, np.float32):
            Q = _queries(sc, nq, dtype, 42)
            got = ctx.refine_store(Q, ids, cnt, K)
            t = _refine_store_dev(pkg, ctx, Q, ids, cnt, K)
            _same(got, dict(ids=_host(t["oi"]), dist=_host(t["od"]), count=_host(t["oc"]), scored=_host(t["sc"])))
            assert np.array_equal(got["scored"], cnt)
            rows = sc["X64"][ids]
            o_ids, o_dist, o_count = oracle.refine(Q.astype(np.float64), rows, ids, cnt, K)
            assert np.array_equal(got["ids"], o_ids) and np.array_equal(got["dist"], o_dist) and np.array_equal(got["count"], o_count)


# ---- kernel-attached timing: which dispatches may carry events ---------------------------------------------------------------
# The expected launch counts below were taken from the commit before the host-side staging / launch refactor by running this
# very test there; they are not derived from the code under test.

def test_timing_counts_every_second_plain_scan(pkg, scene):
    sc = scene
    n, B, nq = sc["params"]["n"], 100, 5
    rng = np.random.default_rng(51)
    ids = np.stack([rng.permutation(n)[:B] for _ in range(nq)]).astype(np.int32)
    cnt = np.full(nq, B, np.int32)
    Q = _queries(sc, nq, np.float32, 52)
    with _ctx(pkg, sc, store=True) as ctx:
        ctx.refine_timing_begin(8, every=2)
        t = None
        for _ in range(4):
            t = _refine_store_dev(pkg, ctx, Q, ids, cnt, K, t)
        launches, ms = ctx.refine_timing_end()
        assert launches == 2 and ms > 0.0, (launches, ms)


def test_timing_skips_the_listed_scan_of_a_retry_pass(pkg, scene):
    import torch
    sc, N = scene, pkg._native
    B, k, nq = 16, 5, 8
    Q = _queries(sc, nq, np.float32, 61)
    with _ctx(pkg, sc, store=True) as ctx:
        assert ctx.effective_probes(1) != ctx.effective_probes(10)
        qd = _dev(Q)
        oi, od = _empty((nq, k), torch.int32), _empty((nq, k), torch.float64)
        oc, scd, ret = (_empty((nq,), torch.int32) for _ in range(3))
        ctx.refine_timing_begin(8, every=2)
        for _ in range(4):
            # pass 1: one plain scan; the retry pass (every query is short of 10 * k scored rows) runs a listed Route and a listed scan
            ctx.search_retry_dev(nq, qd.data_ptr(), N.F32, 1, B, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), scd.data_ptr(), 0, 0, 0,
                                 ret.data_ptr())
        launches, ms = ctx.refine_timing_end()
        assert _host(ret).any(), "no query was retried: the listed scan did not do any work"
        # four plain scans seen, every second one timed; the four listed scans between them are not seen at all
        assert launches == 2 and ms > 0.0, (launches, ms)
