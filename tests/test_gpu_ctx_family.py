"""GPU: what an owner and its clones share, and what each context keeps to itself (fspann_ctx_clone / fspann_ctx_destroy):

  * the owner closed first: the shared state lives on for the clones, which go on seeing each other's deletes and touched records;
  * a clone's private store: rows of its own behind store_set, the owner's rows untouched;
  * a Setup that fails half-way leaves a context that a correct Setup can still use.

Every result is compared with the CPU oracle; every refused call is a documented refusal."""
import threading

import numpy as np
import pytest

from conftest import make_scene

pytestmark = pytest.mark.gpu
SCENE = dict(n=4000, d=8, T=3, D=1, m=8, lam=2, B=64)
K = 5          # 10 K <= B: the oracle's adaptive retry (QSI:327-337) stays out of the comparison


def _ctx(pkg, sc):
    p = sc["params"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 max_global_candidates=p["hard_cap"])
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
    ctx.set_id_meta(p["n"])
    return ctx


def _route_equals_oracle(o, ctx, codes, B, note):
    ids, _, count, raw = o.route(codes)
    c = np.minimum(count, B)
    for counters in (True, False):                                         # full select (and the host's replay) / bounded select
        r = ctx.route(codes, limit=B, counters=counters)
        assert np.array_equal(r["count"], c), (note, counters)
        for i in range(len(codes)):
            assert np.array_equal(r["ids"][i, :c[i]], ids[i, :c[i]]), (note, i, counters)
        if counters:
            assert np.array_equal(r["kept"], count) and np.array_equal(r["raw_seen"], raw), note
    return ids, c


def _search_equals_oracle(o, ctx, Q, B, note):
    ref = o.search(Q.astype(np.float64), K)
    rt = ctx.route(ctx.encode(Q), limit=B, counters=False)
    rs = ctx.refine_store(Q, rt["ids"][:, :B], rt["count"], K)
    assert np.array_equal(rt["count"], ref["sel_count"]), note
    assert np.array_equal(rs["ids"], ref["ids"]) and np.array_equal(rs["dist"], ref["dist"]), note
    return rt


def test_owner_closed_first_the_clones_keep_one_shared_state(pkg, oracle):
    sc = make_scene(oracle, seed=81, **SCENE)
    o, n, B = sc["oracle"], SCENE["n"], SCENE["B"]
    Q = sc["rng"].standard_normal((12, SCENE["d"])).astype(np.float32)
    codes = o.encode(Q.astype(np.float64))
    owner = _ctx(pkg, sc)
    owner.build_index(sc["X"])
    owner.store_set(sc["X"])
    owner.touch_enable(True)
    tables = [owner.get_index(td) for td in range(o.TD)]
    a, b = owner.clone(), owner.clone()
    owner.close()
    try:
        b.set_route_mode(2)
        _route_equals_oracle(o, b, codes, B, "owner closed")
        # a delete through one clone shows in the other's next query, on the device and in the host's replay
        ids0, _, cnt0, _ = o.route(codes)
        victims = np.unique(np.concatenate([ids0[i, :min(cnt0[i], 10)] for i in range(0, len(Q), 3)])).astype(np.int32)
        a.set_deleted(victims, True)
        deleted = np.zeros(n, np.uint8)
        deleted[victims] = 1
        o.set_id_meta(n, None, deleted)
        _route_equals_oracle(o, b, codes, B, "deleted through the other clone")
        assert not np.isin(b.route(codes, limit=B)["ids"], victims).any()
        # a Refine on one clone marks the family's touched set: the other clone counts and drains it
        assert b.touched_count() == 0
        rt = _search_equals_oracle(o, a, Q, B, "search on a clone, owner closed")
        a.sync()
        want = np.unique(np.concatenate([rt["ids"][i, :rt["count"][i]] for i in range(len(Q))]))
        assert b.touched_count() == len(want)
        assert np.array_equal(b.drain_touched(), want)
        assert a.touched_count() == 0
        # the host mirror of the tables is the family's, not the owner's
        for td in range(o.TD):
            got = a.get_index(td)
            assert all(np.array_equal(got[k_], v_) for k_, v_ in tables[td].items()), td
        with pytest.raises(pkg.FspannStateError, match="was destroyed"):      # no new member once the owner is gone
            a.clone()
    finally:
        th = [threading.Thread(target=c_.close) for c_ in (a, b)]
        for t in th:
            t.start()
        for t in th:
            t.join()


def test_a_delete_through_one_clone_reaches_the_others_host_replay(pkg, oracle):
    """Twelve of query 0's candidates get different hashCodes of ONE HashMap bin: its bestScore map treeifies, the kernels flag the
    query and fspann_route finishes it on the host from the family's host mirror (tables, hashes, deleted bits).  The owner is
    closed; a delete through one clone must show in the other clone's replayed answer, which stays the oracle's."""
    from route_order_scenes import spread_inv
    sc = make_scene(oracle, seed=85, **SCENE)
    o, n, B = sc["oracle"], SCENE["n"], SCENE["B"]
    Q64 = sc["rng"].standard_normal((12, SCENE["d"]))
    ids0, _, cnt0, _ = o.route(o.encode(Q64))
    assert cnt0[0] >= 14
    crowd, others = ids0[0, :12].astype(np.int32), ids0[0, 12:14].astype(np.int32)
    jh = oracle.decimal_hashes(n).copy()
    jh[crowd] = spread_inv(777 + 32768 * np.arange(1, 13))
    o.set_id_meta(n, jh)
    o.build_index(sc["X64"])
    codes = o.encode(Q64)
    assert o.route_treeified(codes)[0]
    p = sc["params"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=B,
                                 max_global_candidates=p["hard_cap"])
    owner = pkg.FspannContext(cfg, 0)
    owner.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
    owner.set_id_meta(n, jh)
    for td in range(o.TD):
        owner.set_index(td, **o.get_index(td))
    owner.finalize()
    a, b = owner.clone(), owner.clone()
    owner.close()
    try:
        _route_equals_oracle(o, b, codes, B, "treeified, nothing deleted")
        victims = np.concatenate([crowd[:2], others])                       # ten of the twelve stay: the bin still treeifies
        a.set_deleted(victims, True)
        deleted = np.zeros(n, np.uint8)
        deleted[victims] = 1
        o.set_id_meta(n, jh, deleted)
        assert o.route_treeified(codes)[0] and not o.unmodelled
        _route_equals_oracle(o, b, codes, B, "treeified, deleted through the other clone")
        assert not np.isin(b.route(codes, limit=B)["ids"][0], victims).any()
        assert b.unmodelled_queries() == 0
    finally:
        a.close()
        b.close()


def test_a_clone_may_take_a_store_of_its_own(pkg, oracle):
    sc = make_scene(oracle, seed=82, **SCENE)
    o, B = sc["oracle"], SCENE["B"]
    X = sc["X"]
    Y = np.ascontiguousarray(X[::-1] * np.float32(0.5) + np.float32(0.25))      # other rows of the same shape
    Q = sc["rng"].standard_normal((12, SCENE["d"])).astype(np.float32)
    with _ctx(pkg, sc) as owner:
        owner.build_index(X)
        owner.store_set(X)
        k = owner.clone()
        try:
            _search_equals_oracle(o, k, Q, B, "the clone on the owner's rows")
            k.store_set(Y)
            o.set_store(Y.astype(np.float64))
            _search_equals_oracle(o, k, Q, B, "the clone on its own rows")
            o.set_store(sc["X64"])
            _search_equals_oracle(o, owner, Q, B, "the owner on its rows")
            with pytest.raises(pkg.FspannStateError, match=r"shared with 1 clone\(s\)"):
                owner.store_set(Y)
            with pytest.raises(pkg.FspannStateError, match="a clone reads its parent's"):
                k.store_narrow()
            _search_equals_oracle(o, owner, Q, B, "the owner after the refusals")
        finally:
            k.close()
        owner.store_set(Y)                                                    # the clone gone, the owner's store may change
        o.set_store(Y.astype(np.float64))
        _search_equals_oracle(o, owner, Q, B, "the owner on new rows")


def test_a_clone_of_a_clone_starts_on_its_sources_store(pkg, oracle):
    """fspann_ctx_clone copies its SOURCE's store reference (include/fspann.h): a clone made of a clone that took rows of its own
    refines over those rows, as the Python wrapper's bookkeeping (store_dtype, row count) has always assumed; the source may then
    replace its store again without touching what its clone reads."""
    sc = make_scene(oracle, seed=84, **SCENE)
    o, B = sc["oracle"], SCENE["B"]
    X = sc["X"]
    Y = np.ascontiguousarray(X[::-1] * np.float32(0.5) + np.float32(0.25))
    Q = sc["rng"].standard_normal((12, SCENE["d"])).astype(np.float32)
    with _ctx(pkg, sc) as owner:
        owner.build_index(X)
        owner.store_set(X)
        with owner.clone() as k:
            k.store_set(Y)
            with k.clone() as k2:
                o.set_store(Y.astype(np.float64))
                _search_equals_oracle(o, k2, Q, B, "the clone's clone on the clone's rows")
                k.store_set(X)                                                # k lets go of Y: k2 keeps it alive
                _search_equals_oracle(o, k2, Q, B, "the clone's clone after its source moved on")
                o.set_store(sc["X64"])
                _search_equals_oracle(o, k, Q, B, "the source on its new rows")
                _search_equals_oracle(o, owner, Q, B, "the owner on its rows")


def test_a_failed_finalize_leaves_a_context_that_a_correct_setup_can_use(pkg, oracle):
    sc = make_scene(oracle, seed=83, **SCENE)
    o, B = sc["oracle"], SCENE["B"]
    codes = o.encode(sc["rng"].standard_normal((12, SCENE["d"])))
    with _ctx(pkg, sc) as ctx:
        for td in range(o.TD):
            t = o.get_index(td)
            if td == 1:
                t["ids"] = t["ids"].copy()
                t["ids"][5] = t["ids"][4]                                      # a table that holds an id twice
            ctx.set_index(td, **t)
        with pytest.raises(pkg.FspannArgumentError, match="twice"):
            ctx.finalize()
        with pytest.raises(pkg.FspannStateError, match="not finalized"):
            ctx.route(codes, limit=B)
        ctx.build_index(sc["X"])
        _route_equals_oracle(o, ctx, codes, B, "built after the failed finalize")
