"""CPU: what can be asked of include/fspann_eval.h without a device — the header declares the three entry points and nothing else,
the library exports them, the binding holds them in a table of its own (fspann.h's counted set and the rows header's two stay as
they are), a null context is FSPANN_E_NULL — and the argument fspann_eval_kvariants_dev rests on, restated in numpy: the ratio fold
for k is a prefix of the fold for max(ks), and result i is a hit for k iff max(i, first place of its id in gt) < k.  Both are held
against gt_ref.metrics called once per k, over the data sets with invalid ids, dGt = 0, short counts and repeated ids planted."""
import os
import re

import numpy as np
import pytest

import gt_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EVAL = ("fspann_eval_kvariants_dev", "fspann_search_fallback_dev", "fspann_search_fallback_finish_dev")


def test_eval_entry_points_are_exported_and_wrapped(pkg):
    pkg._native.build()
    L = pkg._native.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fspann_eval.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fspann_[a-z0-9_]+)\s*\(", txt))) == sorted(EVAL)
    assert pkg._native.eval_symbols() == sorted(EVAL)
    for s in EVAL:
        assert hasattr(L, s), s
        assert s not in pkg._native.exported_symbols(), s
        assert s not in pkg._native.rows_symbols(), s
    for m in ("search_fallback_dev", "search_fallback_finish_dev", "eval_kvariants_dev", "eval_kvariants", "run_queries"):
        assert hasattr(pkg.FspannContext, m), m


def test_null_context_without_gpu(pkg):
    N = pkg._native
    L = N.lib()
    assert L.fspann_eval_kvariants_dev(None, 10, None, N.F32, 2, None, N.F32, 16, None, 1, None, 5, None, None, 5, None, None, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
    assert L.fspann_search_fallback_dev(None, 2, None, N.F32, -1, 64, 5, None, None, None, None, None, None, None, None, None) == N.E_NULL
    assert L.fspann_search_fallback_finish_dev(None, 2, None, N.F32, -1, 64, 5, None, None, None, None, None, None, None, None, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()


def sweep(base64, q64, ks, ann, ann_count, gt):
    """(recall [nk][nq], ratio [nk][nq]) the way the one-launch kernel computes them: each distance once, one running fold over
    i < min(kmax, na) read off behind term k - 1, hits(k) = #{i : max(i, p(i)) < k}"""
    n, kmax = len(base64), max(ks)
    nq, stride = ann.shape
    rec, rat = np.empty((len(ks), nq)), np.full((len(ks), nq), np.nan)
    for qi in range(nq):
        na = stride if ann_count is None else max(0, min(int(ann_count[qi]), stride))
        lim = min(kmax, na)
        a, g = ann[qi, :lim].astype(np.int64), gt[qi, :kmax].astype(np.int64)
        ok = (a >= 0) & (a < n) & (g[:lim] >= 0) & (g[:lim] < n)
        d_ann, d_gt = np.zeros(lim), np.zeros(lim)
        d_ann[ok] = gt_ref.l2(q64[qi], base64[a[ok]])
        d_gt[ok] = gt_ref.l2(q64[qi], base64[g[:lim][ok]])
        tot, used, snap = 0.0, 0, {}
        for i in range(lim):
            if d_gt[i] > 0:
                tot += float(d_ann[i]) / float(d_gt[i])
                used += 1
            snap[i + 1] = (tot, used)
        m = np.full(lim, kmax, np.int64)
        for i in range(lim):
            hit = np.flatnonzero(g == a[i])
            m[i] = max(i, int(hit[0])) if len(hit) else kmax
        for j, k in enumerate(ks):
            rec[j, qi] = int((m < k).sum()) / float(k)
            if na >= k and snap[k][1] == k:
                rat[j, qi] = snap[k][0] / k
    return rec, rat


@pytest.mark.parametrize("bdt,qdt,d,kmax", [("f32", "f32", 24, 100), ("u8", "u8", 24, 65), ("i8", "f32", 7, 64), ("f16", "f32", 24, 129)])
def test_prefix_fold_and_first_place_restate_the_metrics(bdt, qdt, d, kmax):
    sc = gt_ref.metrics_scene(bdt, qdt, d, kmax)
    ks = sorted({kmax, 1, min(10, kmax), kmax - 1, min(64, kmax), min(65, kmax)} - {0})
    X64, Q64 = sc["X"].astype(np.float64), sc["Q"].astype(np.float64)
    told = 0
    for stride, cnt in ((kmax, True), (kmax + 5, True), (kmax, False)):
        ann, c, g = gt_ref.metrics_call(sc, stride, kmax + 7)
        c = c if cnt else None
        rec, rat = sweep(X64, Q64, ks, ann, c, g)
        for j, k in enumerate(ks):
            r0, t0 = gt_ref.metrics(X64, Q64, k, ann, c, g)
            assert np.array_equal(rec[j], r0), (k, stride)
            assert np.array_equal(rat[j].view(np.uint64), t0.view(np.uint64)), (k, stride)
            told += int(np.isnan(t0).any()) + int((~np.isnan(t0)).any())
    assert told >= 2 * len(ks)          # every k saw a NaN ratio and a number
