"""GPU: fspann_search_fallback_dev (+ fspann_search_fallback_finish_dev) is the search step of ForwardSecureANNSystem.runQueries
(FSA:660-678): QueryServiceImpl.search, and for a query that returned nothing a second whole search at max(2 * base probes, 4)
probes.  The reference is composed from oracle.search only: the batch at the caller's probes, then oracle.search of the empty rows
at F probes put in their places.  ids, fp64 distances, count, scored (metrics[:, 2]), F_q of the last pass and retried
(metrics[:, 4]) are compared with np.array_equal, fellback with the empty rows.  Every scene's preconditions (which queries are
empty, which retry inside the fallback, what F is) are asserted from the oracle before the device is asked."""
import numpy as np
import pytest

import fallback_ref as R
from conftest import make_scene

pytestmark = pytest.mark.gpu

def test_main_scene_empty_queries_fall_back(pkg, oracle):
    sc, Q, K, ref, fb, _, _ = R.main_scene(oracle)
    with R.context(pkg, sc) as ctx:
        got = R.run(ctx, Q, 256, K, -1)
        again = R.run(ctx, Q, 256, K, -1, finish=True)          # nothing is flagged: the finish call changes nothing
        assert ctx.unmodelled_queries() == 0
    R.check(got, ref, fb)
    R.check(again, ref, fb)
    assert again["resolved"] == 0


def test_no_empty_query_is_the_retry_call(pkg, oracle):
    """Every output equals fspann_search_retry_dev's, array for array, and nothing fell back."""
    B, K = 64, 10
    sc = make_scene(oracle, n=20000, d=16, T=4, D=2, m=10, lam=2, B=B, seed=11)
    sc["Xs"] = sc["X"]
    Q = sc["rng"].standard_normal((96, 16)).astype(np.float32)
    ref, fb, r1, _ = R.reference(sc["oracle"], Q, K, -1, R.fallback_probes(-1, -1))
    assert not fb.any() and r1["metrics"][:, 4].any()
    with R.context(pkg, sc) as ctx:
        want = R.run(ctx, Q, B, K, -1, call="retry")
        got = R.run(ctx, Q, B, K, -1)
    for k in ("ids", "dist", "count", "scored", "sel", "selc", "bad", "ret"):
        assert np.array_equal(got[k], want[k]), k
    assert (got["fb"] == 0).all()
    R.check(got, ref, fb)


PROBES = [
    # cfg.probe_override, the argument, F, what the oracle must show about the fallback's retry
    # (K = 30 with B = 256: 10 K > B, every query that scores a row is short)
    pytest.param(-1, -1, 10, "same", 30, id="default 5: F = 10, the retry pass is skipped"),
    pytest.param(-1, 6, 12, "down", 20, id="6: F = 12, the retry goes down to 10"),
    pytest.param(2, 0, 4, "any", 20, id="0: F = 4 although search 1 ran at cfg's 2"),
    pytest.param(3, -1, 6, "any", 20, id="cfg 3, argument -1: F = 6"),
]


def _probe_scene(oracle, cfg_po, arg_po, F, kind, K):
    sc, Q = R.empty_scene(oracle, cfg_po, arg_po, (0, 1, 2, 3, 9, 17))
    assert R.fallback_probes(arg_po, cfg_po) == F
    ref, fb, r1, r2 = R.reference(sc["oracle"], Q, K, arg_po, F)
    assert np.flatnonzero(fb).tolist() == [0, 1, 2, 3, 9, 17] and (r2["count"] > 0).any()
    if kind != "any":
        assert r2["metrics"][:, 4].any()                      # a fallen-back query is short at F probes: reported retried
    if kind == "down":                                        # and its second pass, at FEWER probes, is what it returns
        r12 = sc["oracle"].search(Q[fb == 1].astype(np.float64), K, probe_override=10)
        short = r2["metrics"][:, 4] == 1
        assert np.array_equal(r2["ids"][short], r12["ids"][short]) and (r2["sel_count"][short] == r12["sel_count"][short]).all()
    return sc, Q, K, ref, fb


@pytest.mark.parametrize("cfg_po,arg_po,F,kind,K", PROBES)
def test_fallback_probe_arithmetic(pkg, oracle, cfg_po, arg_po, F, kind, K):
    sc, Q, K, ref, fb = _probe_scene(oracle, cfg_po, arg_po, F, kind, K)
    with R.context(pkg, sc) as ctx:
        assert ctx.effective_probes(arg_po) == (arg_po if arg_po > 0 else cfg_po if cfg_po > 0 else 5)
        got = R.run(ctx, Q, 256, K, arg_po)
    R.check(got, ref, fb)


def _failed_loads_scene(oracle):
    K = 10
    sc = R.failing_scene(oracle)
    Q = sc["rng"].standard_normal((64, 16)).astype(np.float32)
    ref, fb, r1, r2 = R.reference(sc["oracle"], Q, K, -1, R.fallback_probes(-1, 1))
    m = r1["metrics"]
    assert ((m[:, 1] > 0) & (m[:, 2] == 0) & (fb == 1)).any(), "no query with kept > 0 and nothing scored"
    assert 0 < fb.sum() < len(Q) and (r2["count"] > 0).any()
    return sc, Q, K, ref, fb


def test_empty_by_failed_loads(pkg, oracle):
    """A store shorter than the index and non-finite rows: kept > 0 but nothing scored is empty too, and falls back."""
    sc, Q, K, ref, fb = _failed_loads_scene(oracle)
    with R.context(pkg, sc) as ctx:
        got = R.run(ctx, Q, 256, K, -1)
    R.check(got, ref, fb)


def test_non_finite_queries_never_fall_back(pkg, oracle):
    sc, Q, K, _, _, _, _ = R.main_scene(oracle)
    Q = Q.copy()
    Q[2, 5], Q[7, 0], Q[23, 15] = np.nan, np.inf, -np.inf
    bad = ~np.isfinite(Q).all(1)
    ref, fb, r1, _ = R.reference(sc["oracle"], Q, K, -1, 4)
    assert (r1["count"][bad] == 0).all() and fb.tolist() == [1, 1, 0, 1, 1] + [0] * 19
    with R.context(pkg, sc) as ctx:
        got = R.run(ctx, Q, 256, K, -1)
    assert (got["bad"] == bad).all() and (got["count"][bad] == 0).all() and (got["ret"][bad] == 0).all()
    R.check(got, ref, fb, bad)


def test_touched_set_is_the_union_of_both_searches(pkg, oracle):
    """The rows scored by search 1 (pass 1 and the last pass) and by search 2 (its pass 1 at F probes and its last pass)."""
    sc, Q, K, ref, fb, r1, r2 = R.main_scene(oracle)
    o, B = sc["oracle"], 256
    codes = o.encode(Q.astype(np.float64))
    ids1, _, c1, _ = o.route(codes, probe_override=-1)
    idsF, _, cF, _ = o.route(codes, probe_override=4)
    want = set()
    for i in range(len(Q)):
        want.update(ids1[i, :min(int(c1[i]), B)].tolist())
        want.update(r1["sel"][i, :r1["sel_count"][i]].tolist())
    for j, i in enumerate(np.flatnonzero(fb)):
        want.update(idsF[i, :min(int(cF[i]), B)].tolist())
        want.update(r2["sel"][j, :r2["sel_count"][j]].tolist())
    only2 = set(idsF[0, :min(int(cF[0]), B)].tolist()) - set(ids1.reshape(-1).tolist())
    assert only2, "search 2 scores no row that search 1 did not reach"
    with R.context(pkg, sc) as ctx:
        ctx.touch_enable(True)
        got = R.run(ctx, Q, B, K, -1)
        touched = set(ctx.drain_touched(reset=True).tolist())
    R.check(got, ref, fb)
    assert touched == want, (sorted(touched - want)[:10], sorted(want - touched)[:10])


def _spread_inv(s):
    s = np.asarray(s).astype(np.uint32)
    return (s ^ (s >> 16)).view(np.int32)


def _flagged_scene(oracle):
    """Query 0 is empty in search 1 (everything its pass reaches is deleted); twelve of the ids only the fallback's probes add carry
    crafted hashCodes (distinct, one bin): its HashMap treeifies a bin in search 2 only."""
    n, d, B, K = 8000, 16, 64, 10
    sc = make_scene(oracle, n=n, d=d, T=4, D=1, m=10, lam=2, B=B, seed=77, probe_override=2)
    sc["Xs"] = sc["X"]
    o = sc["oracle"]
    Q = sc["rng"].standard_normal((8, d)).astype(np.float32)
    codes = o.encode(Q.astype(np.float64))
    F = R.fallback_probes(-1, 2)
    ids1, _, c1, _ = o.route(codes, cap=4096)
    idsF, _, cF, _ = o.route(codes, probe_override=F, cap=4096)
    extra = np.setdiff1d(idsF[0, :cF[0]], ids1[0, :c1[0]])
    assert len(extra) >= 12
    jh = oracle.decimal_hashes(n).copy()
    jh[extra[:12]] = _spread_inv(1777 + 32768 * np.arange(1, 13))
    deleted = np.zeros(n, np.uint8)
    deleted[ids1[0, :c1[0]]] = 1
    o.set_id_meta(n, jh, deleted)
    o.build_index(sc["X64"])
    sc["deleted"] = deleted
    codes = o.encode(Q.astype(np.float64))
    f1, f10, fF = o.route_treeified(codes), o.route_treeified(codes, probe_override=10), o.route_treeified(codes, probe_override=F)
    assert not f1.any() and fF[0] and not fF[1:].any()
    ref, fb, r1, r2 = R.reference(o, Q, K, -1, F)
    assert fb[0] == 1 and r2["count"][0] > 0 and not o.unmodelled
    assert not f10[fb == 0].any()                             # (search 1's retry pass flags nothing)
    return sc, Q, B, K, jh, ref, fb


@pytest.mark.parametrize("mode", [0, 1])
def test_query_flagged_in_search_2_is_finished(pkg, oracle, mode):
    sc, Q, B, K, jh, ref, fb = _flagged_scene(oracle)
    with R.context(pkg, sc, jh) as ctx:
        ctx.set_route_mode(mode)
        got = R.run(ctx, Q, B, K, -1, finish=True)
        assert ctx.unmodelled_queries() == 0
    assert got["resolved"] >= 1
    R.check(got, ref, fb)


def _flagged_then_empty_scene(oracle):
    """Query 0 treeifies a bin in search 1's pass 1 (twelve crafted hashCodes among the ids it reaches) and every row that pass
    reaches fails to load (NaN): flagged, then, finished on the host, kept > 0 with nothing scored.  Its fallback belongs to the
    finish call, and at F probes its map treeifies again."""
    n, d, B, K = 8000, 16, 1024, 10
    sc = make_scene(oracle, n=n, d=d, T=4, D=1, m=10, lam=2, B=B, seed=77, probe_override=2)
    o = sc["oracle"]
    Q = sc["rng"].standard_normal((8, d)).astype(np.float32)
    codes = o.encode(Q.astype(np.float64))
    F = R.fallback_probes(-1, 2)
    ids1, _, c1, _ = o.route(codes, cap=4096)
    jh = oracle.decimal_hashes(n).copy()
    jh[ids1[0, :12]] = _spread_inv(777 + 32768 * np.arange(1, 13))
    Xs = sc["X"].copy()
    Xs[ids1[0, :c1[0]]] = np.nan
    o.set_id_meta(n, jh)
    o.build_index(sc["X64"])
    o.set_store(Xs.astype(np.float64))
    sc["Xs"] = Xs
    codes = o.encode(Q.astype(np.float64))
    f1, fF = o.route_treeified(codes), o.route_treeified(codes, probe_override=F)
    assert f1.tolist() == [True] + [False] * 7 and fF[0]
    ref, fb, r1, r2 = R.reference(o, Q, K, -1, F)
    assert fb.tolist() == [1] + [0] * 7 and r1["metrics"][0, 1] > 0 and r1["metrics"][0, 2] == 0 and not r1["metrics"][:, 4].any()
    assert r2["count"][0] == K and not o.unmodelled
    return sc, Q, B, K, jh, ref, fb


@pytest.mark.parametrize("mode", [0, 1])
def test_query_flagged_in_search_1_falls_back_in_the_finish_call(pkg, oracle, mode):
    sc, Q, B, K, jh, ref, fb = _flagged_then_empty_scene(oracle)
    with R.context(pkg, sc, jh) as ctx:
        ctx.set_route_mode(mode)
        got = R.run(ctx, Q, B, K, -1, finish=True)
        assert ctx.unmodelled_queries() == 0
    assert got["resolved"] >= 2                               # once in search 1, once in its fallback
    R.check(got, ref, fb)


def test_argument_checks(pkg, oracle):
    import torch
    sc = make_scene(oracle, n=4000, d=16, T=2, D=2, m=10, lam=2, B=64, seed=3)
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
            ctx.search_fallback_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        ctx.build_index(sc["X"])
        with pytest.raises(pkg.FspannStateError):       # no store
            ctx.search_fallback_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        ctx.store_set(sc["X"])
        with pytest.raises(pkg.FspannStateError):       # no fallback call precedes the finish
            ctx.search_fallback_finish_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        ctx.search_retry_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        with pytest.raises(pkg.FspannStateError):       # a retry call is not a fallback call
            ctx.search_fallback_finish_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        for k in (0, -3):
            with pytest.raises(pkg.FspannArgumentError):
                ctx.search_fallback_dev(4, Q.data_ptr(), 0, -1, 64, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        for nulls in ((0, od, oc), (oi, 0, oc), (oi, od, 0)):
            ptrs = [x if isinstance(x, int) else x.data_ptr() for x in nulls]
            with pytest.raises(pkg.FspannNullError):
                ctx.search_fallback_dev(4, Q.data_ptr(), 0, -1, 64, 10, *ptrs)
        with pytest.raises(pkg.FspannArgumentError):
            ctx.search_fallback_dev(4, Q.data_ptr(), 0, -1, 0, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        ctx.search_fallback_dev(0, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())     # empty batch: nothing to do
        ctx.search_fallback_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr())     # every optional buffer absent
        assert ctx.search_fallback_finish_dev(4, Q.data_ptr(), 0, -1, 64, 10, oi.data_ptr(), od.data_ptr(), oc.data_ptr()) == 0
        ctx.sync()
