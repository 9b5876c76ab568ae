"""GPU: FspannContext.run_queries is ForwardSecureANNSystem.runQueries (FSA:622-748) for a batch over the resident store — the
search with its empty-result fallback, then recall, distance ratio and candidate ratio at every k of kVariants from the one result
list.  The expected results are composed from oracle.search (tests/fallback_ref.py), the expected metrics are
oracle.metrics per k over those results and oracle.groundtruth; a number is compared in its bits, a NaN by its place."""
import numpy as np
import pytest

import fallback_ref as F

pytestmark = pytest.mark.gpu

KS = (1, 10, 20)


def _bits_equal(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got.tolist(), want.tolist())
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64)), (what, got.tolist(), want.tolist())


def _check(oracle, got, ref, fb, X32, Q, ks, kinds=("nan", "num", "hit")):
    K = max(ks)
    assert np.array_equal(got["fellback"], fb)
    assert np.array_equal(got["ids"], ref["ids"]) and np.array_equal(got["dist"], ref["dist"]) and np.array_equal(got["count"], ref["count"])
    assert np.array_equal(got["scored"], ref["metrics"][:, 2]) and np.array_equal(got["retried"], ref["metrics"][:, 4])
    assert np.array_equal(got["sel_count"], ref["sel_count"]) and got["resolved"] == 0
    gt, _ = oracle.groundtruth(X32, Q, K)
    assert np.array_equal(got["gt_ids"], gt)
    seen = set()
    for j, k in enumerate(ks):
        rec, rat = oracle.metrics(X32, Q, k, ref["ids"], ref["count"], gt)
        _bits_equal(got["recall"][j], rec, "recall@%d" % k)
        _bits_equal(got["ratio"][j], rat, "ratio@%d" % k)
        u = ref["sel_count"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            cr = np.where(ref["sel_count"] > 0, u / k, np.nan)
        _bits_equal(got["cand_ratio"][j], cr, "cand_ratio@%d" % k)
        seen.update(["nan"] * int(np.isnan(rat).any()) + ["num"] * int((~np.isnan(rat)).any()) + ["hit"] * int((rec > 0).any()))
    assert seen == set(kinds)          # the scene shows each kind of value it was built to show


def test_run_queries_on_the_main_scene(pkg, oracle):
    sc, Q, K, ref, fb, _, _ = F.main_scene(oracle)
    assert K == max(KS)
    with F.context(pkg, sc) as ctx:
        got = ctx.run_queries(Q, KS, B=256)
        given = ctx.run_queries(Q, KS, gt_ids=np.pad(got["gt_ids"], ((0, 0), (0, 3)), constant_values=-1), B=256)     # gt_stride > K
        ctx.store_set(sc["X64"])
        with pytest.raises(pkg.FspannArgumentError):
            ctx.run_queries(Q, KS, B=256)                     # an FSPANN_F64 store: the reference's ground truth reads floats
    _check(oracle, got, ref, fb, sc["X"], Q, KS)
    for k in ("recall", "ratio", "cand_ratio"):
        assert np.array_equal(given[k].view(np.uint64), got[k].view(np.uint64)), k


def test_run_queries_on_a_clone(pkg, oracle):
    """A clone reads its parent's store in place (one resident store served from several contexts): the same answer from it."""
    sc, Q, K, ref, fb, _, _ = F.main_scene(oracle)
    with F.context(pkg, sc) as ctx:
        want = ctx.run_queries(Q, KS, B=256)
        with ctx.clone() as twin:
            got = twin.run_queries(Q, KS, B=256)
            with twin.clone() as third:                       # (a clone of a clone shares the same owner)
                got3 = third.run_queries(Q, KS, B=256)
    _check(oracle, got, ref, fb, sc["X"], Q, KS)
    for k in want:
        for g in (got, got3):
            a, b = np.asarray(want[k]), np.asarray(g[k])
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_run_queries_over_a_byte_store(pkg, oracle):
    """FSPANN_U8 rows (index built from the bytes, store kept as bytes): what the oracle gives over the same values as floats."""
    n, d, T, D, m, lam, B = 4000, 16, 2, 2, 8, 2, 256
    rng = np.random.default_rng(19)
    Xu = np.clip(np.rint(128 + 40 * rng.standard_normal((n, d))), 0, 255).astype(np.uint8)
    X32, X64 = Xu.astype(np.float32), Xu.astype(np.float64)
    Q = (X32[rng.integers(0, n, 16)] + 8 * rng.standard_normal((16, d))).astype(np.float32)
    alpha, r, w = oracle.registry_init(X64[:1000], m, 13, T, D)
    o = oracle.Oracle(T, D, m, lam, d, refinement_limit=B, probe_override=1)
    o.set_gfunctions(alpha, r, w)
    o.set_store(X64)
    codes = o.encode(Q.astype(np.float64))
    o.set_id_meta(n)
    o.build_index(X64)
    ids1, _, c1, _ = o.route(codes, cap=8192)
    deleted = np.zeros(n, np.uint8)
    for q in (0, 5):
        deleted[ids1[q, :c1[q]]] = 1
    o.set_id_meta(n, None, deleted)
    ref, fb, r1, r2 = F.reference(o, Q, max(KS), -1, F.fallback_probes(-1, 1))
    assert np.flatnonzero(fb).tolist() == [0, 5] and (r2["count"] > 0).any() and (r1["count"][fb == 0] > 0).all()
    cfg = pkg.PaperRuntimeConfig(tables=T, divisions=D, m=m, lambda_=lam, dim=d, refinement_limit=B, probe_override=1)
    with pkg.FspannContext(cfg, 0) as ctx:
        ctx.set_gfunctions(alpha, r, w)
        ctx.set_id_meta(n, None, deleted)
        ctx.build_index(Xu)
        ctx.store_set(Xu, dtype=np.uint8)
        assert ctx.store_dtype == np.uint8
        got = ctx.run_queries(Q, KS)
    _check(oracle, got, ref, fb, X32, Q, KS, kinds=("num", "hit"))          # (every query returns 20 results here: no NaN ratio)
