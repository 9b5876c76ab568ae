"""What the GPU tests of runQueries' search step share (tests/test_gpu_search_fallback.py, tests/test_gpu_run_queries.py): the
reference composed from oracle.search — the batch at the caller's probes, then oracle.search of the empty rows at F probes put in
their places —, the scenes whose preconditions are asserted from the oracle, a context over a scene, one device call and its
comparison.  A helper module (no test, no fixture), like gt_ref.py."""
import numpy as np

from conftest import make_scene

F32 = 0


def fallback_probes(arg_po, cfg_po, default=5):
    """FSA:640, 668-673"""
    po = arg_po if arg_po >= 0 else cfg_po
    base = po if po >= 0 else default
    return max(2 * base, 4)


def codes_of(o, Q):
    return o.encode(np.where(np.isfinite(Q), Q, 0).astype(np.float64))      # (a non-finite query is never coded: QSI:137-140)


def reference(o, Q, K, arg_po, F):
    """runQueries' search step from oracle.search: (merged result, fellback [nq], search 1's result, the fallback's result)"""
    Q64 = Q.astype(np.float64)
    codes = codes_of(o, Q)
    ref = o.search(Q64, K, codes=codes, probe_override=arg_po)
    fb = (ref["count"] == 0) & np.isfinite(Q).all(1)
    out = {k: v.copy() for k, v in ref.items()}
    r2 = None
    if fb.any():
        r2 = o.search(Q64[fb], K, codes=codes[fb], probe_override=F)
        for k in out:
            out[k][fb] = r2[k]
    return out, fb.astype(np.int32), ref, r2


def empty_scene(oracle, cfg_po, arg_po, empty, n=6000, B=256, seed=7, nq=24, also10=()):
    """make_scene with every id deleted that search 1's pass 1 reaches for the queries `empty` (and every id 10 probes reach for
    the queries `also10`): those queries return nothing (kept == 0), with no QSI retry."""
    sc = make_scene(oracle, n=n, d=16, T=2, D=2, m=8, lam=2, seed=seed, B=B, probe_override=cfg_po)
    Q = sc["rng"].standard_normal((nq, 16)).astype(np.float32)
    o = sc["oracle"]
    codes = o.encode(Q.astype(np.float64))
    ids1, _, c1, _ = o.route(codes, probe_override=arg_po, cap=8192)
    ids10, _, c10, _ = o.route(codes, probe_override=10, cap=8192)
    deleted = np.zeros(n, np.uint8)
    for q in empty:
        deleted[ids1[q, :c1[q]]] = 1
    for q in also10:
        deleted[ids10[q, :c10[q]]] = 1
    o.set_id_meta(n, None, deleted)
    sc["deleted"] = deleted
    sc["Xs"] = sc["X"]
    return sc, Q


def failing_scene(oracle, n=6000, B=256, seed=5, fail=0.97, store_frac=0.2, cfg_po=1):
    """make_scene plus store rows that fail to load: non-finite rows (fraction `fail`) and ids past the GPU store's end
    (store_frac), mirrored in the oracle's store (QSI:252-260: skipped, not scored)."""
    sc = make_scene(oracle, n=n, d=16, T=2, D=2, m=10, lam=2, seed=seed, B=B, probe_override=cfg_po)
    rng = np.random.default_rng(seed + 1)
    Xs = sc["X"].copy()
    Xs[rng.random(n) < fail] = np.nan
    ns = int(n * store_frac)
    sc["oracle"].set_store(Xs.astype(np.float64), (np.arange(n) < ns).astype(np.uint8))
    sc["Xs"] = np.ascontiguousarray(Xs[:ns])
    sc["valid"] = (np.arange(n) < ns) & np.isfinite(Xs).all(1)
    return sc


def context(pkg, sc, jh=None):
    p = sc["params"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 probe_override=p["probe_override"])
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
    if jh is None:
        ctx.set_id_meta(p["n"], None, sc.get("deleted"))
        ctx.build_index(sc["X"])
    else:
        o = sc["oracle"]
        ctx.set_id_meta(p["n"], jh, sc.get("deleted"))
        for td in range(o.TD):
            ctx.set_index(td, **o.get_index(td))
        ctx.finalize()
    ctx.store_set(sc["Xs"])
    return ctx


def run(ctx, Q, B, K, po, call="fallback", finish=False):
    import torch
    dev = torch.device("cuda", 0)
    nq = len(Q)
    qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    t = dict(ids=torch.full((nq, K), -7, dtype=torch.int32, device=dev), dist=torch.zeros((nq, K), dtype=torch.float64, device=dev),
             count=torch.full((nq,), -7, dtype=torch.int32, device=dev), scored=torch.full((nq,), -7, dtype=torch.int32, device=dev),
             sel=torch.full((nq, B), -1, dtype=torch.int32, device=dev), selc=torch.full((nq,), -7, dtype=torch.int32, device=dev),
             bad=torch.full((nq,), -7, dtype=torch.int32, device=dev), ret=torch.full((nq,), -7, dtype=torch.int32, device=dev),
             fb=torch.full((nq,), -7, dtype=torch.int32, device=dev))
    args = (nq, qd.data_ptr(), F32, po, B, K, t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr(),
            t["sel"].data_ptr(), t["selc"].data_ptr(), t["bad"].data_ptr(), t["ret"].data_ptr())
    resolved = 0
    if call == "fallback":
        ctx.search_fallback_dev(*args, t["fb"].data_ptr())
        if finish:
            resolved = ctx.search_fallback_finish_dev(*args, t["fb"].data_ptr())
    else:
        ctx.search_retry_dev(*args)
    ctx.sync()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out["resolved"] = resolved
    return out


def check(got, ref, fb, bad=None):
    nq = len(got["count"])
    bad = np.zeros(nq, bool) if bad is None else bad
    assert np.array_equal(got["fb"], fb), (got["fb"].tolist(), fb.tolist())
    assert np.array_equal(got["count"], ref["count"]), np.flatnonzero(got["count"] != ref["count"])
    assert np.array_equal(got["ids"], ref["ids"]), np.flatnonzero((got["ids"] != ref["ids"]).any(1))
    assert np.array_equal(got["dist"], ref["dist"])
    assert np.array_equal(got["scored"], ref["metrics"][:, 2]), np.flatnonzero(got["scored"] != ref["metrics"][:, 2])
    assert np.array_equal(got["ret"], ref["metrics"][:, 4]), np.flatnonzero(got["ret"] != ref["metrics"][:, 4])
    for i in np.flatnonzero(~bad):
        c = ref["sel_count"][i]
        assert got["selc"][i] == c, i
        assert np.array_equal(got["sel"][i, :c], ref["sel"][i, :c]), i


def main_scene(oracle):
    """cfg.probe_override = 2, K = 20: F = 4.  Queries 0-4 are empty (kept == 0); 0-3 return 20 results at 4 probes, 1 and 2 through
    the retry inside the fallback; 4 stays empty (everything 10 probes reach is deleted); 5-23 keep search 1's answer."""
    K = 20
    sc, Q = empty_scene(oracle, 2, -1, (0, 1, 2, 3), also10=(4,))
    assert int(sc["deleted"].sum()) == 3084
    F = fallback_probes(-1, 2)
    assert F == 4
    ref, fb, r1, r2 = reference(sc["oracle"], Q, K, -1, F)
    assert np.flatnonzero(r1["count"] == 0).tolist() == [0, 1, 2, 3, 4] and (r1["metrics"][:5, 1] == 0).all() and not r1["metrics"][:5, 4].any()
    assert r2["count"].tolist() == [20, 20, 20, 20, 0] and r2["metrics"][:, 4].tolist() == [0, 1, 1, 0, 0]
    assert (r1["count"][5:] == 20).all() and fb.tolist() == [1] * 5 + [0] * 19
    return sc, Q, K, ref, fb, r1, r2
