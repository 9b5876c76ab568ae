"""GPU: fspann_search_retry_dev (+ fspann_search_retry_finish_dev) is QueryServiceImpl.search WITH its adaptive retry
(QSI:327-337, 444-447): every query equals oracle.search — ids, fp64 distances, count, scored (metrics[:, 2]), F_q of the last
pass and retried (metrics[:, 4]) — with the short queries searched again on the device with 10 probes."""
import numpy as np
import pytest

from conftest import make_scene

pytestmark = pytest.mark.gpu


def _scene(oracle, n=20000, d=16, T=2, D=2, B=128, fail=0.0, seed=5, store_frac=1.0, m=10):
    """make_scene plus store rows that fail to load: non-finite rows (fraction `fail`) and ids past the GPU store's end
    (store_frac), mirrored in the oracle's store (QSI:252-260: skipped, not scored)."""
    sc = make_scene(oracle, n=n, d=d, T=T, D=D, m=m, lam=2, B=B, seed=seed)
    rng = np.random.default_rng(seed + 1)
    Xs = sc["X"].copy()
    Xs[rng.random(n) < fail] = np.nan
    ns = int(n * store_frac)
    sc["oracle"].set_store(Xs.astype(np.float64), (np.arange(n) < ns).astype(np.uint8))
    sc["Xs"] = np.ascontiguousarray(Xs[:ns])
    return sc


def _ctx(pkg, sc, jh=None, store=True):
    p = sc["params"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"])
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
    if jh is None:
        ctx.set_id_meta(p["n"])
        ctx.build_index(sc["X"])
    else:
        ctx.set_id_meta(p["n"], jh)
        o = sc["oracle"]
        for td in range(o.TD):
            ctx.set_index(td, **o.get_index(td))
        ctx.finalize()
    if store:
        ctx.store_set(sc["Xs"])
    return ctx


def _run(ctx, Q, B, K, po, call="retry", finish=False):
    import torch
    dev = torch.device("cuda", 0)
    nq = len(Q)
    qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    t = dict(ids=torch.full((nq, K), -7, dtype=torch.int32, device=dev), dist=torch.zeros((nq, K), dtype=torch.float64, device=dev),
             count=torch.full((nq,), -7, dtype=torch.int32, device=dev), scored=torch.full((nq,), -7, dtype=torch.int32, device=dev),
             sel=torch.full((nq, B), -1, dtype=torch.int32, device=dev), selc=torch.full((nq,), -7, dtype=torch.int32, device=dev),
             bad=torch.full((nq,), -7, dtype=torch.int32, device=dev), ret=torch.full((nq,), -7, dtype=torch.int32, device=dev))
    F32 = 0
    args = (nq, qd.data_ptr(), F32, po, B, K, t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr(),
            t["sel"].data_ptr(), t["selc"].data_ptr(), t["bad"].data_ptr())
    resolved = 0
    if call == "retry":
        ctx.search_retry_dev(*args, t["ret"].data_ptr())
        if finish:
            resolved = ctx.search_retry_finish_dev(*args, t["ret"].data_ptr())
    else:
        ctx.search_store_dev(*args)
    ctx.sync()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["resolved"] = resolved
    return out


def _check(got, ref, B, bad=None):
    nq = len(got["count"])
    bad = np.zeros(nq, bool) if bad is None else bad
    assert np.array_equal(got["count"], ref["count"]), np.flatnonzero(got["count"] != ref["count"])
    assert np.array_equal(got["ids"], ref["ids"]), np.flatnonzero((got["ids"] != ref["ids"]).any(1))
    assert np.array_equal(got["dist"], ref["dist"])
    assert np.array_equal(got["scored"], ref["metrics"][:, 2]), np.flatnonzero(got["scored"] != ref["metrics"][:, 2])
    assert np.array_equal(got["ret"], ref["metrics"][:, 4]), np.flatnonzero(got["ret"] != ref["metrics"][:, 4])
    for i in np.flatnonzero(~bad):
        c = ref["sel_count"][i]
        assert got["selc"][i] == c, i
        assert np.array_equal(got["sel"][i, :c], ref["sel"][i, :c]), i


@pytest.mark.parametrize("mode", [2, 1])
def test_every_query_retries(pkg, oracle, mode):
    """B < 10 K: every query with a scored row is short and takes pass 2; bounded select (2) and full select (1)."""
    B, K = 64, 10
    sc = _scene(oracle, T=4, D=2, B=B, seed=11)
    Q = sc["rng"].standard_normal((96, 16)).astype(np.float32)
    ref = sc["oracle"].search(Q.astype(np.float64), K)
    assert ref["metrics"][:, 4].all()
    with _ctx(pkg, sc) as ctx:
        ctx.set_route_mode(mode)
        got = _run(ctx, Q, B, K, -1)
        assert ctx.last_route_info()["lazy"] == (mode == 2)
    _check(got, ref, B)


def test_plain_search_call_differs_where_retry_matches(pkg, oracle):
    """The same batch through fspann_search_store_dev (no retry) is NOT oracle.search; through the new call it is."""
    B, K = 64, 10
    sc = _scene(oracle, T=4, D=2, B=B, seed=11)
    Q = sc["rng"].standard_normal((96, 16)).astype(np.float32)
    ref = sc["oracle"].search(Q.astype(np.float64), K)
    with _ctx(pkg, sc) as ctx:
        plain = _run(ctx, Q, B, K, -1, call="plain")
        got = _run(ctx, Q, B, K, -1)
    assert not (np.array_equal(plain["ids"], ref["ids"]) and np.array_equal(plain["selc"], ref["sel_count"]))
    _check(got, ref, B)


@pytest.mark.parametrize("B,K,T,D,fail,nq", [(128, 10, 2, 2, 0.15, 256), (512, 40, 2, 2, 0.15, 256), (2000, 100, 4, 4, 0.45, 64)])
def test_some_queries_retry(pkg, oracle, B, K, T, D, fail, nq):
    """B >= 10 K, two probes, failing store rows: some queries are short, the others keep pass 1's answer.  B = 512: the refine
    has two chunks per query (merge); B = 2000 (K = 100): the full select only."""
    sc = _scene(oracle, T=T, D=D, B=B, fail=fail, store_frac=0.95, seed=5 + B)
    Q = sc["rng"].standard_normal((nq, 16)).astype(np.float32)
    ref = sc["oracle"].search(Q.astype(np.float64), K, probe_override=2)
    r = ref["metrics"][:, 4]
    assert 0 < r.sum() < nq, r.sum()
    with _ctx(pkg, sc) as ctx:
        got = _run(ctx, Q, B, K, 2)
    _check(got, ref, B)


def test_nan_queries_and_ten_probes_already(pkg, oracle):
    """Non-finite queries are never retried (count 0, nothing scored); pass 1 at 10 probes: retried says 1, answer unchanged."""
    B, K = 128, 10
    sc = _scene(oracle, B=B, fail=0.15, store_frac=0.95, seed=21)
    Q = sc["rng"].standard_normal((200, 16)).astype(np.float32)
    nan_rows = np.array([0, 3, 77, 150, 199])
    Q[nan_rows, 5] = np.nan
    Q[150, 0] = np.inf
    bad = np.zeros(len(Q), bool)
    bad[nan_rows] = True
    o = sc["oracle"]
    with _ctx(pkg, sc) as ctx:
        for po in (2, 10):
            codes = o.encode(np.where(np.isfinite(Q), Q, 0).astype(np.float64))     # (a non-finite query is never coded: QSI:137-140)
            ref = o.search(Q.astype(np.float64), K, codes=codes, probe_override=po)
            r = ref["metrics"][:, 4]
            assert 0 < r.sum() < len(Q) and not r[bad].any()
            got = _run(ctx, Q, B, K, po)
            assert (got["count"][bad] == 0).all() and (got["ret"][bad] == 0).all() and (got["bad"][bad] == 1).all()
            _check(got, ref, B, bad)


def test_large_batch_scattered_short_queries(pkg, oracle):
    """nq = 20 000 with a few percent short queries spread over the batch: the pick list's order and the in-place write-back."""
    B, K = 128, 10
    sc = _scene(oracle, B=B, fail=0.05, store_frac=0.95, seed=8)
    Q = sc["rng"].standard_normal((20000, 16)).astype(np.float32)
    ref = sc["oracle"].search(Q.astype(np.float64), K, probe_override=2)
    r = ref["metrics"][:, 4]
    assert 0.01 * len(Q) < r.sum() < 0.2 * len(Q), r.sum()
    with _ctx(pkg, sc) as ctx:
        got = _run(ctx, Q, B, K, 2)
    _check(got, ref, B)


@pytest.fixture(scope="module")
def pick_scene(oracle):
    """One scene and one oracle search of 1 025 queries (a search is per query: a batch of the first nq is the first nq rows).
    Seed 10, chosen with the oracle: query 0 is retried, queries 64 and 1 024 are, and every prefix below holds both kinds."""
    sc = _scene(oracle, B=128, fail=0.15, store_frac=0.95, seed=10)
    Q = sc["rng"].standard_normal((1025, 16)).astype(np.float32)
    return sc, Q, sc["oracle"].search(Q.astype(np.float64), 10, probe_override=2)


@pytest.mark.parametrize("nq", [1, 63, 65, 1024, 1025])
def test_pick_list_at_the_slice_boundaries(pkg, pick_scene, nq):
    """The pick kernel gives each of its 16 waves a slice of roundup64(ceil(nq / 16)) queries: one query; one partial wave; one wave
    and one query of the next; 16 full slices of 64; slices of 128 with query 1 024 alone in the ninth."""
    sc, Q, full = pick_scene
    ref = {k: v[:nq] for k, v in full.items()}
    r = ref["metrics"][:, 4]
    assert r.all() if nq == 1 else 0 < r.sum() < nq, r.sum()
    with _ctx(pkg, sc) as ctx:
        got = _run(ctx, Q[:nq], 128, 10, 2)
    _check(got, ref, 128)


def _spread_inv(s):
    s = np.asarray(s).astype(np.uint32)
    return (s ^ (s >> 16)).view(np.int32)


@pytest.mark.parametrize("mode", [0, 1])
def test_flagged_in_either_pass_are_finished(pkg, oracle, mode):
    """Crafted bins (distinct hashCodes): query 0's map treeifies a bin in pass 1, query 1's only in pass 2 (twelve of the ids
    ten probes add).  The device leaves both flagged; the finish call resolves them on the host, in the right pass."""
    n, d, B, K = 8000, 16, 64, 10
    sc = _scene(oracle, n=n, d=d, T=4, D=1, B=B, seed=77)
    o = sc["oracle"]
    Q = sc["rng"].standard_normal((8, d)).astype(np.float32)
    codes = o.encode(Q.astype(np.float64))
    ids1, _, c1, _ = o.route(codes, cap=4096)
    ids2, _, c2, _ = o.route(codes, probe_override=10, cap=4096)
    jh = oracle.decimal_hashes(n).copy()
    jh[ids1[0, :12]] = _spread_inv(777 + 32768 * np.arange(1, 13))
    extra = np.setdiff1d(ids2[1, :c2[1]], ids1[1, :c1[1]])
    jh[extra[:12]] = _spread_inv(1777 + 32768 * np.arange(1, 13))
    o.set_id_meta(n, jh)
    o.build_index(sc["X64"])
    codes = o.encode(Q.astype(np.float64))
    f1, f2 = o.route_treeified(codes), o.route_treeified(codes, probe_override=10)
    assert f1[0] and not f1[1] and f2[1]
    ref = o.search(Q.astype(np.float64), K)
    assert ref["metrics"][:, 4].all() and not o.unmodelled
    with _ctx(pkg, sc, jh) as ctx:
        ctx.set_route_mode(mode)
        got = _run(ctx, Q, B, K, -1, finish=True)
        assert ctx.unmodelled_queries() == 0
    assert got["resolved"] >= 2
    _check(got, ref, B)


def test_argument_checks(pkg, oracle):
    import torch
    sc = _scene(oracle, n=4000, B=64, seed=3)
    p = sc["params"]
    dev = torch.device("cuda", 0)
    Q = torch.zeros((4, 16), dtype=torch.float32, device=dev)
    oi = torch.zeros((4, 10), dtype=torch.int32, device=dev)
    od = torch.zeros((4, 10), dtype=torch.float64, device=dev)
    oc = torch.zeros(4, dtype=torch.int32, device=dev)
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=64)
    with pkg.FspannContext(cfg, 0) as ctx:
        ctx.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
        ctx.set_id_meta(p["n"])
        with pytest.raises(pkg.FspannStateError):       # not finalized
            ctx.search_retry_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        ctx.build_index(sc["X"])
        with pytest.raises(pkg.FspannStateError):       # no store
            ctx.search_retry_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        ctx.store_set(sc["Xs"])
        with pytest.raises(pkg.FspannStateError):       # no retry call precedes the finish
            ctx.search_retry_finish_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        for k in (0, -3):
            with pytest.raises(pkg.FspannArgumentError):
                ctx.search_retry_dev(4, Q.data_ptr(), 0, -1, 64, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        for nulls in ((0, od, oc), (oi, 0, oc), (oi, od, 0)):
            ptrs = [x if isinstance(x, int) else x.data_ptr() for x in nulls]
            with pytest.raises(pkg.FspannNullError):
                ctx.search_retry_dev(4, Q.data_ptr(), 0, -1, 64, 10, *ptrs)
        with pytest.raises(pkg.FspannArgumentError):
            ctx.search_retry_dev(4, Q.data_ptr(), 0, -1, 0, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        ctx.search_retry_dev(0, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())     # empty batch: nothing to do


def test_list_mode_scan_and_merge_fallbacks(pkg, oracle, monkeypatch):
    """The list-mode paths the default scenes do not take: the one-workgroup-per-chunk scan (FSPANN_REFINE_STREAM=0) and the merge
    whose keys do not fit LDS (8 chunks x k = 1 200: 77 KB), with every query retried (10 k > B)."""
    B, K = 2000, 1200
    sc = _scene(oracle, T=4, D=4, B=B, fail=0.2, store_frac=0.95, seed=44)
    Q = sc["rng"].standard_normal((24, 16)).astype(np.float32)
    ref = sc["oracle"].search(Q.astype(np.float64), K, probe_override=2)
    assert ref["metrics"][:, 4].all()
    with _ctx(pkg, sc) as ctx:
        got = _run(ctx, Q, B, K, 2)
    _check(got, ref, B)
    B, K = 512, 40
    sc = _scene(oracle, B=B, fail=0.15, store_frac=0.95, seed=45)
    Q = sc["rng"].standard_normal((128, 16)).astype(np.float32)
    ref = sc["oracle"].search(Q.astype(np.float64), K, probe_override=2)
    assert 0 < ref["metrics"][:, 4].sum() < len(Q)
    monkeypatch.setenv("FSPANN_REFINE_STREAM", "0")
    with _ctx(pkg, sc) as ctx:
        got = _run(ctx, Q, B, K, 2)
    _check(got, ref, B)
