"""GPU: the touched-record set (fspann_touch_*, ReencryptionTracker): with tracking on, every Refine marks exactly the rows it
scores (QSI.lastCandDecrypted) — both retry passes, queries finished on the host, the tick's refine role, caller rows, clones of
one index — and every other output stays bit-identical.  Expected sets come from the oracle: pass 1's F_q is the first
min(count, B) entries of oracle.route with the caller's probes, the last pass's is oracle.search's `sel`, filtered by the test's
own store validity (ids past the store's end, non-finite rows) and by the query's finiteness."""
import threading

import numpy as np
import pytest

from conftest import make_scene

pytestmark = pytest.mark.gpu
F32 = 0


def _scene(oracle, n=20000, d=16, T=2, D=2, B=128, fail=0.15, store_frac=0.95, deleted_frac=0.05, seed=5):
    sc = make_scene(oracle, n=n, d=d, T=T, D=D, m=10, lam=2, B=B, seed=seed, deleted_frac=deleted_frac)
    rng = np.random.default_rng(seed + 1)
    Xs = sc["X"].copy()
    Xs[rng.random(n) < fail] = np.nan
    ns = int(n * store_frac)
    sc["oracle"].set_store(Xs.astype(np.float64), (np.arange(n) < ns).astype(np.uint8))
    sc["Xs"] = np.ascontiguousarray(Xs[:ns])
    sc["valid"] = (np.arange(n) < ns) & np.isfinite(Xs).all(1)
    return sc


def _ctx(pkg, sc, store=True, jh=None, probe_override=-1):
    """A context over the scene: index built on the GPU, or (jh given) the oracle's tables imported under those hashCodes."""
    p = sc["params"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 probe_override=probe_override)
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
    if jh is None:
        ctx.set_id_meta(p["n"], None, sc["deleted"])
        ctx.build_index(sc["X"])
    else:
        o = sc["oracle"]
        ctx.set_id_meta(p["n"], jh)
        for td in range(o.TD):
            ctx.set_index(td, **o.get_index(td))
        ctx.finalize()
    if store:
        ctx.store_set(sc["Xs"])
    return ctx


def _spread_inv(s):
    """String.hashCode values whose HashMap.hash() spread is `s` (h ^ h >>> 16 is an involution)."""
    s = np.asarray(s).astype(np.uint32)
    return (s ^ (s >> 16)).view(np.int32)


def _stream(pl, batches):
    """Every batch through the pipeline, kept full (submit ahead, collect in order)."""
    out = []
    for qb in batches:
        pl.submit(qb)
        if pl.in_flight == 4:
            out.append(pl.collect())
    while pl.in_flight:
        out.append(pl.collect())
    assert [o["ticket"] for o in out] == sorted(o["ticket"] for o in out)
    return out


def _codes(o, Q):
    return o.encode(np.where(np.isfinite(Q), Q, 0).astype(np.float64))      # (a non-finite query is never coded: QSI:137-140)


def _expected(o, Q, B, K, po, valid, retry=True):
    """Union over the finite queries of pass 1's F_q and (retry) the last pass's F_q, loaded and finite rows only."""
    codes = _codes(o, Q)
    ids1, _, cnt1, _ = o.route(codes, probe_override=po)
    ref = o.search(Q.astype(np.float64), K, codes=codes, probe_override=po)
    s = set()
    for i in np.flatnonzero(np.isfinite(Q).all(1)):
        rows = list(ids1[i, :min(int(cnt1[i]), B)])
        if retry:
            rows += list(ref["sel"][i, :ref["sel_count"][i]])
        s.update(int(h) for h in rows if valid[h])
    return s, ref


def _bufs(nq, B, K):
    import torch
    dev = torch.device("cuda", 0)
    return dict(ids=torch.full((nq, K), -7, dtype=torch.int32, device=dev), dist=torch.zeros((nq, K), dtype=torch.float64, device=dev),
                count=torch.full((nq,), -7, dtype=torch.int32, device=dev), scored=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                sel=torch.full((nq, B), -1, dtype=torch.int32, device=dev), selc=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                bad=torch.full((nq,), -7, dtype=torch.int32, device=dev), ret=torch.full((nq,), -7, dtype=torch.int32, device=dev))


def _search(ctx, Q, B, K, po, call="retry", finish=True, sync=True):
    import torch
    nq = len(Q)
    qd = torch.from_numpy(np.ascontiguousarray(Q)).to(torch.device("cuda", 0))
    t = _bufs(nq, B, K)
    torch.cuda.synchronize()
    args = (nq, qd.data_ptr(), F32, po, B, K, t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr(),
            t["sel"].data_ptr(), t["selc"].data_ptr())
    if call == "retry":
        ctx.search_retry_dev(*args, t["bad"].data_ptr(), t["ret"].data_ptr())
        if finish:
            ctx.search_retry_finish_dev(*args, t["bad"].data_ptr(), t["ret"].data_ptr())
    else:
        ctx.search_store_dev(*args, t["bad"].data_ptr())
        if finish:
            ctx.search_store_finish_dev(*args)
    if not sync:
        return t, qd
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in t.items()}


def _check_drain(ctx, want):
    n = ctx.touched_count()
    got = ctx.drain_touched(reset=True)
    assert n == len(got)
    assert np.all(np.diff(got) > 0), "handles not ascending"
    assert set(got.tolist()) == want, (sorted(set(got.tolist()) - want)[:10], sorted(want - set(got.tolist()))[:10])
    assert ctx.touched_count() == 0 and len(ctx.drain_touched()) == 0
    return got


def test_search_retry_touched_union_and_outputs_unchanged(pkg, oracle):
    B, K, po = 128, 10, 2
    sc = _scene(oracle, seed=5)
    o = sc["oracle"]
    Q = sc["rng"].standard_normal((256, 16)).astype(np.float32)
    Q[[0, 9, 100], 3] = np.nan
    Q[200, 0] = np.inf
    want, ref = _expected(o, Q, B, K, po, sc["valid"])
    r = ref["metrics"][:, 4]
    assert 0 < r.sum() < len(Q)
    assert sc["deleted"].any() and not (set(np.flatnonzero(sc["deleted"])) & want)
    with _ctx(pkg, sc) as ctx:
        with pytest.raises(pkg.FspannStateError):
            ctx.touched_count()
        off = _search(ctx, Q, B, K, po)
        ctx.touch_enable(True)
        assert ctx.touched_count() == 0
        on = _search(ctx, Q, B, K, po)
        for k in off:
            assert np.array_equal(off[k], on[k]), k
        assert np.array_equal(on["ids"], ref["ids"]) and np.array_equal(on["ret"], r)
        _check_drain(ctx, want)
        # off again: nothing is marked, the set is kept
        ctx.touch_enable(False)
        _search(ctx, Q, B, K, po)
        assert ctx.touched_count() == 0


def test_one_query_per_call_touches_its_scored_rows(pkg, oracle):
    B, K = 128, 10
    sc = _scene(oracle, seed=7)
    Q = sc["rng"].standard_normal((30, 16)).astype(np.float32)
    Q[4, 1] = np.nan
    with _ctx(pkg, sc) as ctx:
        ctx.touch_enable(True)
        for i in range(len(Q)):
            got = _search(ctx, Q[i:i + 1], B, K, 2, call="plain")
            h = ctx.drain_touched(reset=True)
            assert len(h) == got["scored"][0], i
            assert set(h.tolist()) <= set(got["sel"][0, :got["selc"][0]].tolist())
        assert ctx.touched_count() == 0


def test_queries_finished_on_the_host_are_touched(pkg, oracle):
    """Treeified bins (as tests/test_gpu_treeify.py): search_store_dev flags them, _finish_dev resolves and scores them."""
    n, d, B, K = 8000, 16, 64, 5
    sc = make_scene(oracle, n=n, d=d, T=4, D=1, m=10, lam=2, B=B, seed=77)
    o = sc["oracle"]
    Q = sc["rng"].standard_normal((8, d)).astype(np.float32)
    ids, _, count, _ = o.route(o.encode(Q.astype(np.float64)))
    jh = oracle.decimal_hashes(n).copy()
    jh[ids[0, :12]] = _spread_inv(777 + 32768 * np.arange(1, 13))
    o.set_id_meta(n, jh)
    o.build_index(sc["X64"])
    want_flag = o.route_treeified(o.encode(Q.astype(np.float64)))
    assert want_flag.any()
    ref = o.search(Q.astype(np.float64), K)
    assert not ref["metrics"][:, 4].any()
    want = set(int(h) for i in range(len(Q)) for h in ref["sel"][i, :ref["sel_count"][i]])
    with _ctx(pkg, dict(sc, Xs=sc["X"]), jh=jh) as ctx:
        ctx.touch_enable(True)
        t, qd = _search(ctx, Q, B, K, -1, call="plain", finish=False, sync=False)
        ctx.sync()
        flagged = set(int(h) for i in np.flatnonzero(want_flag) for h in ref["sel"][i, :ref["sel_count"][i]])
        assert ctx.touched_count() < len(want) and flagged - set(ctx.drain_touched(reset=False).tolist())
        args = (len(Q), qd.data_ptr(), F32, -1, B, K, t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr(),
                t["sel"].data_ptr(), t["selc"].data_ptr())
        assert ctx.search_store_finish_dev(*args) == int(want_flag.sum())
        ctx.sync()
        assert np.array_equal(t["ids"].cpu().numpy(), ref["ids"])
        _check_drain(ctx, want)


@pytest.mark.parametrize("dense", [False, True])
def test_tick_refine_role_touched(pkg, oracle, dense):
    """Three batches: route of batch t+1 and refine of batch t share a tick; rows from the store or handed over (dense)."""
    import torch
    B, K, d, Qn = 64, 5, 16, 96
    sc = _scene(oracle, B=B, fail=0.1, store_frac=1.0, deleted_frac=0.0, seed=13)
    o = sc["oracle"]
    dev = torch.device("cuda", 0)
    batches = [sc["rng"].standard_normal((Qn, d)).astype(np.float32) for _ in range(3)]
    batches[1][5, 2] = np.nan
    want = set()
    for qb in batches:
        w, _ = _expected(o, qb, B, K, -1, sc["valid"], retry=False)
        want |= w
    with _ctx(pkg, sc) as ctx:
        ctx.touch_enable(True)
        qd = [torch.from_numpy(qb).to(dev) for qb in batches]
        codes = [torch.zeros((Qn, ctx.TD * ctx.W), dtype=torch.int64, device=dev) for _ in batches]
        bad = [torch.zeros(Qn, dtype=torch.int32, device=dev) for _ in batches]
        sel = [torch.full((Qn, B), -1, dtype=torch.int32, device=dev) for _ in batches]
        selc = [torch.zeros(Qn, dtype=torch.int32, device=dev) for _ in batches]
        cand = torch.zeros((Qn, B, d), dtype=torch.float32, device=dev)
        oi = torch.zeros((Qn, K), dtype=torch.int32, device=dev)
        od = torch.zeros((Qn, K), dtype=torch.float64, device=dev)
        oc = torch.zeros(Qn, dtype=torch.int32, device=dev)
        scn = torch.zeros(Qn, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for b in range(3):
            ctx.encode_dev(Qn, qd[b].data_ptr(), F32, codes[b].data_ptr(), 0, bad[b].data_ptr())
        fused = []
        for t in range(4):
            rt = rf = None
            if t < 3:
                rt = dict(nq=Qn, codes=codes[t].data_ptr(), limit=B, ids=sel[t].data_ptr(), count=selc[t].data_ptr())
            if t >= 1:
                b = t - 1
                if dense:
                    ctx.sync()
                    ids_h, cnt_h = sel[b].cpu().numpy(), selc[b].cpu().numpy()
                    rows = np.zeros((Qn, B, d), np.float32)
                    rows[:] = np.where(np.isfinite(sc["Xs"]), sc["Xs"], np.nan)[np.clip(ids_h, 0, len(sc["Xs"]) - 1)]
                    assert (cnt_h >= 0).all()
                    cand.copy_(torch.from_numpy(rows))
                    torch.cuda.synchronize()
                rf = dict(nq=Qn, q=qd[b].data_ptr(), B=B, ids=sel[b].data_ptr(), count=selc[b].data_ptr(), k=K, out_ids=oi.data_ptr(),
                          out_dist=od.data_ptr(), out_count=oc.data_ptr(), scored=scn.data_ptr(), cand=cand.data_ptr() if dense else None)
            ctx.tick_dev(None, rt, rf)
            if rf is not None and rt is not None:
                fused.append(ctx.last_tick_fused())
        ctx.sync()
        assert any(fused)
        _check_drain(ctx, want)


def test_refine_with_caller_rows(pkg, oracle):
    """fspann_refine (host rows): NaN rows and a non-finite query mark nothing; ids outside the index are never marked."""
    n, d, B, K = 5000, 16, 32, 5
    sc = make_scene(oracle, n=n, d=d, T=2, D=2, m=10, lam=2, B=B, seed=3)
    rng = sc["rng"]
    nq = 40
    Q = rng.standard_normal((nq, d))
    Q[7, 0] = np.nan
    ids = rng.integers(0, n, (nq, B)).astype(np.int32)
    for i in range(nq):
        ids[i] = rng.choice(n, B, replace=False)
    ids[3, 1] = n + 5                              # no handle of this index
    ids[3, 2] = -1
    cnt = rng.integers(0, B + 1, nq).astype(np.int32)
    cnt[11] = -1                                   # flagged, unresolved: nothing
    cand = sc["X64"][np.clip(ids, 0, n - 1)].copy()
    nanrow = rng.random((nq, B)) < 0.2
    cand[nanrow, 4] = np.nan
    want = set()
    for i in range(nq):
        if i == 7 or cnt[i] <= 0:
            continue
        want.update(int(ids[i, j]) for j in range(cnt[i]) if not nanrow[i, j] and 0 <= ids[i, j] < n)
    with _ctx(pkg, dict(sc, Xs=sc["X"]), store=False) as ctx:
        before = ctx.refine(Q, cand, ids, cnt, K)
        ctx.touch_enable(True)
        res = ctx.refine(Q, cand, ids, cnt, K)
        for k in before:
            assert np.array_equal(before[k], res[k]), k
        _check_drain(ctx, want)


def test_clones_share_one_set(pkg, oracle):
    """Owner and two clones search on their own streams at once (overlapping and disjoint batches); enabling on a clone enables
    the family; a drain on a clone after syncing all three is the union."""
    B, K, po = 128, 10, 2
    sc = _scene(oracle, seed=19)
    o = sc["oracle"]
    rng = sc["rng"]
    A = rng.standard_normal((300, 16)).astype(np.float32)
    Ab = np.concatenate([A[150:], rng.standard_normal((100, 16)).astype(np.float32)])     # overlaps A
    C_ = rng.standard_normal((200, 16)).astype(np.float32) + 3.0                          # elsewhere
    want = set()
    for qb in (A, Ab, C_):
        want |= _expected(o, qb, B, K, po, sc["valid"])[0]
    with _ctx(pkg, sc) as owner:
        c1, c2 = owner.clone(), owner.clone()
        try:
            c1.touch_enable(True)
            out, errs = {}, []

            def run(name, ctx, qb):
                try:
                    for _ in range(2):
                        out[name] = _search(ctx, qb, B, K, po)
                except Exception as e:       # noqa: BLE001
                    errs.append(e)
            th = [threading.Thread(target=run, args=a) for a in (("a", owner, A), ("b", c1, Ab), ("c", c2, C_))]
            for x in th:
                x.start()
            for x in th:
                x.join()
            assert not errs, errs
            owner.sync(); c1.sync(); c2.sync()
            assert owner.touched_count() == len(want)
            _check_drain(c2, want)
        finally:
            c1.close(); c2.close()


def test_short_buffer_drains_the_smallest_first(pkg, oracle):
    B, K = 128, 10
    sc = _scene(oracle, seed=23)
    Q = sc["rng"].standard_normal((128, 16)).astype(np.float32)
    with _ctx(pkg, sc) as ctx:
        ctx.touch_enable(True)
        _search(ctx, Q, B, K, 2)
        n = ctx.touched_count()
        allh = ctx.drain_touched(reset=False)
        assert len(allh) == n > 100 and ctx.touched_count() == n
        cap = n // 3
        a = ctx.drain_touched(reset=True, cap=cap)
        assert np.array_equal(a, allh[:cap])
        assert ctx.touched_count() == n - cap
        b = ctx.drain_touched(reset=True)
        assert np.array_equal(b, allh[cap:])
        assert ctx.touched_count() == 0
        import ctypes as C
        L = pkg._native.lib()
        assert L.fspann_touch_count(ctx.handle, None) == pkg._native.E_NULL
        nn = C.c_int64(0)
        assert L.fspann_touch_drain(ctx.handle, None, 4, C.byref(nn), 1) == pkg._native.E_NULL
        assert L.fspann_touch_drain(ctx.handle, None, 0, None, 1) == pkg._native.E_NULL


def test_selective_reencryption_end_to_end(pkg, oracle):
    """Native pipeline with retry, some records deleted and some tampered with (they fail to open): after a rotation, every
    record is at version 2 iff it was touched; the others stay at version 1."""
    from fspann_amd import hostpipe
    K, B, n, gone_n = 10, 128, 20000, 4000
    sc = make_scene(oracle, n=n, d=16, T=2, D=2, m=10, lam=2, B=B, seed=31, probe_override=2)
    o, rng = sc["oracle"], sc["rng"]
    gone = rng.choice(n, gone_n, replace=False)
    valid = np.ones(n, bool)
    valid[gone] = False
    o.set_store(sc["X64"], valid.astype(np.uint8))                   # loadPointIfActive() == null / decrypt failure for those
    batches = [rng.standard_normal((nq, 16)).astype(np.float32) for nq in (200, 128, 7, 200, 200, 33)]
    refs = [o.search(qb.astype(np.float64), K) for qb in batches]
    assert any(r["metrics"][:, 4].any() for r in refs)
    want = set()
    for qb in batches:
        want |= _expected(o, qb, B, K, -1, valid)[0]
    with _ctx(pkg, sc, store=False, probe_override=2) as ctx, hostpipe.PointStore(n, 16) as ps:
        ps.encrypt(sc["X"], threads=8)
        for h in gone[:gone_n // 2]:
            ps.delete(int(h))                                        # no record
        for h in gone[gone_n // 2:]:
            ver, iv, ct = ps.get_record(int(h))
            ps.put_record(int(h), ver, iv, ct[:-1] + bytes([ct[-1] ^ 0x80]))   # tag mismatch
        ctx.touch_enable(True)
        with hostpipe.Pipeline(ctx, ps, 200, B, K, host_threads=8, retry=True) as pl:
            out = _stream(pl, batches)
            failed1 = ps.stats()["failed"]
        for res, ref in zip(out, refs):
            assert np.array_equal(res["ids"], ref["ids"]) and np.array_equal(res["dist"], ref["dist"])
        assert ctx.touched_count() == len(want)
        assert ps.rotate() == 2
        touched, done, already = hostpipe.reencrypt_touched(ctx, ps, threads=4)
        assert touched == len(want) and done + already == touched and done == touched
        ver = np.array([ps.get_record(h)[0] if valid[h] else -1 for h in range(n)])
        t = np.zeros(n, bool)
        t[list(want)] = True
        assert (ver[t] == 2).all() and (ver[valid & ~t] == 1).all()
        with hostpipe.Pipeline(ctx, ps, 200, B, K, host_threads=8, retry=True) as pl:
            again = _stream(pl, batches)
            failed2 = ps.stats()["failed"]
        assert failed1 > 0 and failed2 - failed1 == failed1      # only the gone records fail, as in the first run
        for res, ref in zip(again, refs):
            assert np.array_equal(res["ids"], ref["ids"]) and np.array_equal(res["dist"], ref["dist"])
        assert hostpipe.reencrypt_touched(ctx, ps, threads=4) == (len(want), 0, len(want))


@pytest.mark.fullsize
def test_config5_selective_reencryption_while_queries_stream(pkg):
    """BASELINE config #5 at its stated size (1 M x 128, 16 x 32 bits, B = 256, 1 024-query batches) with SELECTIVE
    re-encryption: queries stream through the pipeline on the owner's stream while another thread, on a clone, drains the
    touched set (resetting) and re-encrypts what it drained — drains race the marks of batches in flight.  Results stay
    bit-identical to the quiet run; the union of every drain is exactly the set of rows the batches scored (no mark lost);
    after a final drain, a record is at version 2 iff its handle was drained."""
    from fspann_amd import hostpipe
    n, d, T, m, B, Q, K = 1_000_000, 128, 16, 16, 256, 1024, 10
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, d), dtype=np.float32)
    batches = [rng.standard_normal((Q, d), dtype=np.float32) for _ in range(6)]
    cfg = pkg.PaperRuntimeConfig(tables=T, divisions=1, m=m, lambda_=2, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as ctx, hostpipe.PointStore(n, d) as ps:
        ctx.registry_initialize(X[:1000].astype(np.float64))
        ctx.set_id_meta(n)
        ctx.build_index(X)
        ps.encrypt(X)
        # what the batches score: every routed row (all records open, all rows and queries finite)
        want = np.zeros(n, bool)
        for qb in batches:
            rt = ctx.route(ctx.encode(qb), limit=B, counters=False)
            assert (rt["count"] >= 0).all()
            for i in range(Q):
                want[rt["ids"][i, :rt["count"][i]]] = True
        with hostpipe.Pipeline(ctx, ps, Q, B, K) as pl:
            quiet = _stream(pl, batches)                              # tracking off: the reference run
            assert ps.rotate() == 2
            ctx.touch_enable(True)
            drained = np.zeros(n, bool)
            drains, moved, stop, errs = [0], [0], [False], []
            drainer = ctx.clone()

            def reencrypt_loop():
                try:
                    while True:
                        last = stop[0]
                        h = drainer.drain_touched(reset=True)
                        drained[h] = True
                        drains[0] += 1
                        if len(h):
                            moved[0] += ps.reencrypt(h, threads=8)
                        if last:
                            return
                except Exception as e:                           # noqa: BLE001
                    errs.append(e)

            th = threading.Thread(target=reencrypt_loop)
            th.start()
            try:
                live = [_stream(pl, batches) for _ in range(4)]
            finally:
                ctx.sync()
                stop[0] = True
                th.join()
                drainer.close()
            assert not errs, errs
            assert drains[0] >= 2
            # the loop's last drain came after every mark had landed: nothing is left
            assert ctx.touched_count() == 0 and len(ctx.drain_touched(reset=True)) == 0
            after = _stream(pl, batches)                              # every touched record now opens under version 2
        for run in live + [after]:
            for a, b in zip(run, quiet):
                assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["dist"], b["dist"]) and np.array_equal(a["count"], b["count"])
        assert ps.stats()["failed"] == 0
        assert np.array_equal(drained, want), (int(drained.sum()), int(want.sum()))
        assert moved[0] == int(want.sum())                            # each touched record moved exactly once
        sample = np.concatenate([rng.integers(0, n, 3000), rng.choice(np.flatnonzero(want), 1000, replace=False)])
        ver = np.array([ps.get_record(int(h))[0] for h in sample])
        assert np.array_equal(ver == 2, drained[sample]) and set(ver.tolist()) == {1, 2}
