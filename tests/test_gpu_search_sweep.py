"""GPU: fspann_search_sweep_dev (+ fspann_search_sweep_finish_dev) is QueryServiceImpl.search with its adaptive retry at several
refinement limits from ONE encode, ONE Route and ONE scan of the candidate rows.  Two judges, plane by plane:

  the device  fspann_search_retry_dev + fspann_search_retry_finish_dev at B = limits[j]: ids, distances as uint64, count, scored,
              sel_count (= unique) and retried
  the oracle  oracle.search(q, k, refine_override = limits[j]) on an Oracle built with the same config: ids, distances, count,
              metrics candDecrypted / retried and sel_count

N = 20 000 x d = 32, T = 4, D = 1, default probes, k = 10; refinement_limit = 500 and max_global_candidates = 600, so HARD_CAP = 600
cuts every candidate list below the larger limits.  Limits [64, 256, 300, 1 024, 1 500, 4 000] stand on both sides of the bounded
select's 1 024 and of HARD_CAP.  Sixty per cent of the store rows fail to load (non-finite, or past the store's end), so that limit
256 scores about a hundred rows: limit 64 < 10 k retries whenever anything was scored, limit 256 retries for some queries only."""
import numpy as np
import pytest

from conftest import make_scene

pytestmark = pytest.mark.gpu

LIMITS = [64, 256, 300, 1024, 1500, 4000]
N, D_, K, NQ = 20000, 32, 10, 64
F32 = 0
CANARY = -77


def _scene(oracle, fail=0.6, n=N, d=D_, T=4, B=500, hard_cap=600, seed=31):
    sc = make_scene(oracle, n=n, d=d, T=T, D=1, m=10, lam=2, B=B, hard_cap=hard_cap, seed=seed)
    rng = np.random.default_rng(seed + 1)
    Xs = sc["X"].copy()
    ns = n
    if fail > 0:
        Xs[rng.random(n) < fail] = np.nan
        ns = int(n * 0.95)
    sc["oracle"].set_store(Xs.astype(np.float64), (np.arange(n) < ns).astype(np.uint8))
    sc["Xs"] = np.ascontiguousarray(Xs[:ns])
    return sc


def _ctx(pkg, sc, jh=None):
    p = sc["params"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 max_global_candidates=p["hard_cap"])
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
    ctx.store_set(sc["Xs"])
    return ctx


def _sweep(ctx, Q, limits, k, po, finish=True):
    import torch
    dev = torch.device("cuda", 0)
    nq, nl = len(Q), len(limits)
    qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    t = dict(ids=torch.full((nl + 1, nq, k), CANARY, dtype=torch.int32, device=dev), dist=torch.full((nl + 1, nq, k), -5.0, dtype=torch.float64, device=dev),
             bad=torch.full((2, nq), CANARY, dtype=torch.int32, device=dev))
    for key in ("count", "scored", "unique", "ret"):
        t[key] = torch.full((nl + 1, nq), CANARY, dtype=torch.int32, device=dev)
    args = (nq, qd.data_ptr(), F32, po, limits, k, t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr(),
            t["unique"].data_ptr(), t["bad"].data_ptr(), t["ret"].data_ptr())
    ctx.search_sweep_dev(*args)
    resolved = ctx.search_sweep_finish_dev(*args) if finish else 0
    ctx.sync()
    out = {key: v.cpu().numpy() for key, v in t.items()}
    for key, v in out.items():                        # the plane behind each output stays untouched
        assert (v[-1] == (CANARY if key != "dist" else -5.0)).all(), key
        out[key] = v[:-1]
    out["bad"] = out["bad"][0]
    out["resolved"] = resolved
    return out


def _separate(ctx, Q, B, k, po):
    import torch
    dev = torch.device("cuda", 0)
    nq = len(Q)
    qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    t = dict(ids=torch.full((nq, k), -7, dtype=torch.int32, device=dev), dist=torch.zeros((nq, k), dtype=torch.float64, device=dev))
    for key in ("count", "scored", "selc", "bad", "ret"):
        t[key] = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    args = (nq, qd.data_ptr(), F32, po, B, k, t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr(), 0,
            t["selc"].data_ptr(), t["bad"].data_ptr(), t["ret"].data_ptr())
    ctx.search_retry_dev(*args)
    resolved = ctx.search_retry_finish_dev(*args)
    ctx.sync()
    out = {key: v.cpu().numpy() for key, v in t.items()}
    out["resolved"] = resolved
    return out


def _check_device(got, j, one, what):
    assert np.array_equal(got["count"][j], one["count"]), (what, np.flatnonzero(got["count"][j] != one["count"]))
    assert np.array_equal(got["ids"][j], one["ids"]), (what, np.flatnonzero((got["ids"][j] != one["ids"]).any(1)))
    assert np.array_equal(got["dist"][j].view(np.uint64), one["dist"].view(np.uint64)), what
    assert np.array_equal(got["scored"][j], one["scored"]), (what, np.flatnonzero(got["scored"][j] != one["scored"]))
    assert np.array_equal(got["unique"][j], one["selc"]), (what, np.flatnonzero(got["unique"][j] != one["selc"]))
    assert np.array_equal(got["ret"][j], one["ret"]), (what, np.flatnonzero(got["ret"][j] != one["ret"]))
    assert np.array_equal(got["bad"], one["bad"]), what


def _check_oracle(got, j, ref, what, bad=None):
    ok = np.ones(len(ref["count"]), bool) if bad is None else ~bad
    assert np.array_equal(got["count"][j], ref["count"]), (what, np.flatnonzero(got["count"][j] != ref["count"]))
    assert np.array_equal(got["ids"][j], ref["ids"]), (what, np.flatnonzero((got["ids"][j] != ref["ids"]).any(1)))
    assert np.array_equal(got["dist"][j].view(np.uint64), ref["dist"].view(np.uint64)), what
    assert np.array_equal(got["scored"][j], ref["metrics"][:, 2]), (what, np.flatnonzero(got["scored"][j] != ref["metrics"][:, 2]))
    assert np.array_equal(got["ret"][j], ref["metrics"][:, 4]), (what, np.flatnonzero(got["ret"][j] != ref["metrics"][:, 4]))
    assert np.array_equal(got["unique"][j][ok], ref["sel_count"][ok]), (what, np.flatnonzero(got["unique"][j] != ref["sel_count"]))


def _queries(sc, nq=NQ, nan_row=None):
    Q = sc["rng"].standard_normal((nq, sc["params"]["d"])).astype(np.float32)
    bad = np.zeros(nq, bool)
    if nan_row is not None:
        Q[nan_row, 3] = np.nan
        bad[nan_row] = True
    return Q, bad


def _oracle_planes(sc, Q, limits, k, po=-1):
    o = sc["oracle"]
    codes = o.encode(np.where(np.isfinite(Q), Q, 0).astype(np.float64))       # (a non-finite query is never coded: QSI:137-140)
    return [o.search(Q.astype(np.float64), k, codes=codes, probe_override=po, refine_override=lim) for lim in limits]


def test_planes_equal_the_separate_searches_and_the_oracle(pkg, oracle):
    sc = _scene(oracle)
    o = sc["oracle"]
    Q, bad = _queries(sc, nan_row=17)
    # a few deleted ids: candidates of the first queries at the default probes
    codes = o.encode(np.where(np.isfinite(Q), Q, 0).astype(np.float64))
    ids, _, cnt, _ = o.route(codes, cap=1024)
    deleted = np.zeros(N, np.uint8)
    deleted[ids[0, 5:12]] = 1
    deleted[ids[3, :4]] = 1
    o.set_id_meta(N, None, deleted)
    refs = _oracle_planes(sc, Q, LIMITS, K)
    # the scene holds what it claims
    R = np.array([r["metrics"][:, 4] for r in refs])
    assert R.any() and not R.all()
    assert (R.min(0) != R.max(0)).any()                                       # a query whose planes differ in `retried`
    assert R[0][~bad].all() and 0 < R[1].sum() < NQ                           # limit 64 always, limit 256 for some
    assert (refs[-1]["sel_count"] < LIMITS[-1]).any() and (refs[-1]["sel_count"] > 512).any()
    assert not R[:, bad].any()
    with _ctx(pkg, sc) as ctx:
        ctx.set_deleted(np.flatnonzero(deleted).astype(np.int32))
        got = _sweep(ctx, Q, LIMITS, K, -1)
        assert got["resolved"] == 0
        assert (got["bad"][bad] == 1).all() and (got["bad"][~bad] == 0).all() and (got["count"][:, bad] == 0).all()
        for j, lim in enumerate(LIMITS):
            _check_oracle(got, j, refs[j], ("oracle", lim), bad)
            _check_device(got, j, _separate(ctx, Q, lim, K, -1), ("device", lim))
        # a single limit, and the optional outputs left out
        one = _sweep(ctx, Q, [300], K, -1)
        _check_oracle(one, 0, refs[2], ("oracle", "single"), bad)
        import torch
        dev = torch.device("cuda", 0)
        qd = torch.from_numpy(Q).to(dev)
        oi = torch.zeros((len(LIMITS), NQ, K), dtype=torch.int32, device=dev)
        od = torch.zeros((len(LIMITS), NQ, K), dtype=torch.float64, device=dev)
        oc = torch.zeros((len(LIMITS), NQ), dtype=torch.int32, device=dev)
        ctx.search_sweep_dev(NQ, qd.data_ptr(), F32, -1, LIMITS, K, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        assert ctx.search_sweep_finish_dev(NQ, qd.data_ptr(), F32, -1, LIMITS, K, oi.data_ptr(), od.data_ptr(), oc.data_ptr()) == 0
        ctx.sync()
        assert np.array_equal(oi.cpu().numpy(), got["ids"]) and np.array_equal(oc.cpu().numpy(), got["count"])
        assert np.array_equal(od.cpu().numpy().view(np.uint64), got["dist"].view(np.uint64))


@pytest.fixture(scope="module")
def pick_scene(oracle):
    """One scene and the oracle's two planes of 1 025 queries (a search is per query: a batch of the first nq is the first nq rows).
    Seed 32, chosen with the oracle: at limits 256 and 300 some queries retry on a plane and some on none, in either prefix below,
    queries 64 and 1 024 are listed, and hundreds of queries retry on one plane only."""
    limits = [256, 300]
    sc = _scene(oracle, seed=32)
    Q, _ = _queries(sc, nq=1025)
    return sc, Q, limits, _oracle_planes(sc, Q, limits, K)


@pytest.mark.parametrize("nq", [65, 1025])
def test_pick_list_at_the_slice_boundaries(pkg, pick_scene, nq):
    """The pick kernel's 16 waves own slices of roundup64(ceil(nq / 16)) queries: one wave and one query of the next; slices of 128
    with query 1 024 alone in the ninth.  Listed = retried on any plane."""
    sc, Q, limits, full = pick_scene
    refs = [{key: v[:nq] for key, v in r.items()} for r in full]
    R = np.array([r["metrics"][:, 4] for r in refs])
    assert 0 < R.max(0).sum() < nq and R.max(0)[-1] and (R[0] != R[1]).any()
    with _ctx(pkg, sc) as ctx:
        got = _sweep(ctx, Q[:nq], limits, K, -1)
    for j, lim in enumerate(limits):
        _check_oracle(got, j, refs[j], ("oracle", lim))


def test_ten_probes_already(pkg, oracle):
    """probe_override = 10: pass 2 is not run, the short planes are still reported retried"""
    sc = _scene(oracle)
    Q, bad = _queries(sc, nan_row=5)
    refs = _oracle_planes(sc, Q, LIMITS, K, po=10)
    R = np.array([r["metrics"][:, 4] for r in refs])
    assert R.any() and not R.all()
    with _ctx(pkg, sc) as ctx:
        got = _sweep(ctx, Q, LIMITS, K, 10)
        for j, lim in enumerate(LIMITS):
            _check_oracle(got, j, refs[j], ("oracle", lim), bad)
            _check_device(got, j, _separate(ctx, Q, lim, K, 10), ("device", lim))


def test_one_workgroup_per_chunk_scan_in_both_passes(pkg, oracle, monkeypatch):
    """FSPANN_REFINE_STREAM=0: the key scan the stream does not take, over the batch (pass 1) and over the pick list (pass 2)"""
    sc = _scene(oracle)
    Q, bad = _queries(sc, nan_row=40)
    refs = _oracle_planes(sc, Q, LIMITS, K)
    assert 0 < refs[1]["metrics"][:, 4].sum() < NQ
    monkeypatch.setenv("FSPANN_REFINE_STREAM", "0")
    with _ctx(pkg, sc) as ctx:
        got = _sweep(ctx, Q, LIMITS, K, -1)
    for j, lim in enumerate(LIMITS):
        _check_oracle(got, j, refs[j], ("oracle", lim), bad)


def _spread_inv(s):
    s = np.asarray(s).astype(np.uint32)
    return (s ^ (s >> 16)).view(np.int32)


def test_flagged_queries_are_finished_on_the_host(pkg, oracle):
    """Crafted hashCodes crowd one HashMap bin (distinct hashCodes in one bin, as tests/test_gpu_treeify.py builds them): query 0's
    map treeifies in pass 1, query 1's only among the ids ten probes add.  The device leaves both flagged; the finish call
    resolves them on the host in the right pass, scores them through the sweep and applies the retry rule per limit."""
    n, d = 8000, 16
    limits = [32, 64, 100, 200]
    sc = _scene(oracle, fail=0.0, n=n, d=d, B=64, hard_cap=20000, seed=77)
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
    refs = _oracle_planes(sc, Q, limits, K)
    assert not o.unmodelled
    R = np.array([r["metrics"][:, 4] for r in refs])
    assert R[0].all() and not R[-1].all()                # every query retries at limit 32; limit 200 scores 10 k rows for some
    with _ctx(pkg, sc, jh) as ctx:
        raw = _sweep(ctx, Q, limits, K, -1, finish=False)
        assert (raw["unique"][:, 0] == -1).all()         # query 0 is flagged in pass 1: nothing scored, nothing retried yet
        assert (raw["count"][:, 0] == 0).all() and (raw["ret"][:, 0] == 0).all()
        assert ctx.unmodelled_queries() >= 2             # (query 0 in pass 1, query 1 in pass 2; the counter is reset here)
        got = _sweep(ctx, Q, limits, K, -1)
        assert got["resolved"] >= 1 and ctx.unmodelled_queries() == 0
        for j, lim in enumerate(limits):
            _check_oracle(got, j, refs[j], ("oracle", lim))
            _check_device(got, j, _separate(ctx, Q, lim, K, -1), ("device", lim))


def test_touch_tracking_sees_the_union_of_the_separate_searches(pkg, oracle):
    sc = _scene(oracle)
    Q, _ = _queries(sc, nan_row=9)
    with _ctx(pkg, sc) as ctx:
        ctx.touch_enable(True)
        _sweep(ctx, Q, LIMITS, K, -1)
        swept = ctx.drain_touched(reset=True)
        assert ctx.touched_count() == 0
        for lim in LIMITS:
            _separate(ctx, Q, lim, K, -1)
        apart = ctx.drain_touched(reset=True)
        # pass 2 of a query stops at its largest retried limit: a sweep at the small limits alone marks fewer rows
        _sweep(ctx, Q, LIMITS[:1], K, -1)
        small = ctx.drain_touched(reset=True)
    assert len(swept) > 0 and np.array_equal(np.sort(swept), np.sort(apart))
    assert 0 < len(small) < len(swept) and np.isin(small, swept).all()


def test_limit_sweep(pkg, oracle):
    """recall / ratio / cand_ratio of plane j = eval_kvariants over the plane-j outputs of the separate search, as uint64"""
    ks = (1, 5, 10)
    limits = [64, 300, 4000]
    sc = _scene(oracle, fail=0.0)
    Q, _ = _queries(sc, nq=32)
    with _ctx(pkg, sc) as ctx:
        got = ctx.limit_sweep(Q, limits, ks)
        plain = ctx.search_sweep(Q, limits, max(ks))
        given = ctx.limit_sweep(Q, limits, ks, gt_ids=np.pad(got["gt_ids"], ((0, 0), (0, 2)), constant_values=-1))
        assert got["recall"].shape == (len(limits), len(ks), 32) and got["would_fall_back"].shape == (len(limits), 32)
        assert not got["would_fall_back"].any()
        for key in ("ids", "dist", "count", "scored", "unique", "retried", "bad"):
            assert plain[key].tobytes() == got[key].tobytes(), key
        for key in ("recall", "ratio", "cand_ratio"):
            assert np.array_equal(given[key].view(np.uint64), got[key].view(np.uint64)), key
        for j, lim in enumerate(limits):
            one = _separate(ctx, Q, lim, max(ks), -1)
            assert np.array_equal(got["ids"][j], one["ids"]) and np.array_equal(got["unique"][j], one["selc"])
            ev = ctx.eval_kvariants(sc["Xs"], Q, ks, one["ids"], one["count"], got["gt_ids"], unique=one["selc"])
            for key in ("recall", "ratio", "cand_ratio"):
                assert np.array_equal(got[key][j].view(np.uint64), ev[key].view(np.uint64)), (key, lim)
        assert (got["recall"][-1].mean(1) >= got["recall"][0].mean(1)).all() and got["recall"][-1].max() > 0
        ctx.store_set(sc["X64"])
        with pytest.raises(pkg.FspannArgumentError):
            ctx.limit_sweep(Q, limits, ks)                # an FSPANN_F64 store: the reference's ground truth reads floats


def test_state_and_argument_errors(pkg, oracle):
    import torch
    sc = _scene(oracle, fail=0.0, n=4000, d=16, B=64, hard_cap=20000, seed=3)
    dev = torch.device("cuda", 0)
    Q = torch.zeros((4, 16), dtype=torch.float32, device=dev)
    oi = torch.zeros((3, 4, 10), dtype=torch.int32, device=dev)
    od = torch.zeros((3, 4, 10), dtype=torch.float64, device=dev)
    oc = torch.zeros((3, 4), dtype=torch.int32, device=dev)
    outs = (oi.data_ptr(), od.data_ptr(), oc.data_ptr())
    with _ctx(pkg, sc) as ctx:
        with pytest.raises(pkg.FspannStateError, match="precedes"):
            ctx.search_sweep_finish_dev(4, Q.data_ptr(), F32, -1, [16, 64], 10, *outs)
        ctx.search_sweep_dev(4, Q.data_ptr(), F32, -1, [16, 64], 10, *outs)
        for limits, k in (([16, 32], 10), ([16, 64, 65], 10), ([16, 64], 9)):
            with pytest.raises(pkg.FspannStateError, match="precedes"):
                ctx.search_sweep_finish_dev(4, Q.data_ptr(), F32, -1, limits, k, *outs)
        assert ctx.search_sweep_finish_dev(4, Q.data_ptr(), F32, -1, [16, 64], 10, *outs) == 0
        for limits, k in (([64, 16], 10), ([], 10), (list(range(1, 18)), 10), ([16, 64], 1025), ([16, 64], 0)):
            with pytest.raises(pkg.FspannArgumentError):
                ctx.search_sweep_dev(4, Q.data_ptr(), F32, -1, limits, k, *outs)
        with pytest.raises(pkg.FspannNullError):
            ctx.search_sweep_dev(4, Q.data_ptr(), F32, -1, [16, 64], 10, 0, od.data_ptr(), oc.data_ptr())
        ctx.search_sweep_dev(0, Q.data_ptr(), F32, -1, [16, 64], 10, *outs)          # empty batch: nothing to do
