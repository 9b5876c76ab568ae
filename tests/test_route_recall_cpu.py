"""CPU: what can be asked of include/fspann_route_recall.h without a device — the header declares the two attribution entry points
and nothing else, the library exports them, the binding holds them in a table of its own (fspann.h's counted set stays exactly that
header's set, the JNI shim does not bind them), a null context is FSPANN_E_NULL — and the numpy model of both calls (rank, score,
ceiling) that tests/test_gpu_route_recall.py compares the device against, checked here on hand-made cases."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUTE_RECALL = ("fspann_gt_rank_dev", "fspann_recall_ceiling_dev")
INT32_MAX = 2**31 - 1


# ---- the model ---------------------------------------------------------------------------------------------------------------
def rank_model(list_ids, list_score, list_count, gt_ids, kg):
    """fspann_gt_rank_dev: (rank [nq][kg], gt_score [nq][kg] or None).  list_ids [nq][stride], list_score the same or None,
    list_count [nq] or None, gt_ids [nq][>= kg]."""
    nq, stride = list_ids.shape
    rank = np.full((nq, kg), -1, np.int32)
    score = None if list_score is None else np.full((nq, kg), -1, np.int32)
    for q in range(nq):
        cnt = stride if list_count is None else int(list_count[q])
        c = min(cnt, stride)
        if c <= 0:
            if cnt == -1:
                rank[q] = -2
            continue
        first = {}
        for j in range(c - 1, -1, -1):
            first[int(list_ids[q, j])] = j          # (descending: the smallest position wins)
        for i in range(kg):
            g = int(gt_ids[q, i])
            if g >= 0 and g in first:
                rank[q, i] = first[g]
                if score is not None:
                    score[q, i] = list_score[q, first[g]]
    return rank, score


def ceiling_model(rank, ks, limits):
    """fspann_recall_ceiling_dev: (hits int32, ceiling float64) [nl + 1][nk][nq] from rank [nq][>= max(ks)]"""
    nq, nk, nl = rank.shape[0], len(ks), len(limits)
    hits = np.zeros((nl + 1, nk, nq), np.int32)
    ceil = np.zeros((nl + 1, nk, nq), np.float64)
    for l, lim in enumerate(list(limits) + [None]):
        for j, k in enumerate(ks):
            r = rank[:, :k]
            h = ((r >= 0) & (r < (INT32_MAX if lim is None else lim))).sum(1).astype(np.int32)
            unknown = (r == -2).any(1)
            hits[l, j] = np.where(unknown, -1, h)
            ceil[l, j] = np.where(unknown, np.nan, h / float(k))
    return hits, ceil


# ---- the model on cases small enough to read -----------------------------------------------------------------------------------
def test_rank_model_by_hand():
    ids = np.array([[7, 3, 9, 3, 5, 11], [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6], [8, 8, 8, 8, 8, 8]], np.int32)
    sc = np.array([[0, 1, 1, 2, 4, 9]] * 4, np.int32)
    cnt = np.array([5, -1, 0, 9], np.int32)
    gt = np.array([[3, 11, 7, -1, 3, 99, 5], [1, 2, 3, 4, 5, 6, 0], [1, 2, 3, 4, 5, 6, 0], [8, 1, -1, 8, 8, 8, 8]], np.int32)
    rank, score = rank_model(ids, sc, cnt, gt, 6)
    assert rank.tolist() == [[1, -1, 0, -1, 1, -1], [-2] * 6, [-1] * 6, [0, -1, -1, 0, 0, 0]]      # (11 sits at position 5 >= c = 5)
    assert score.tolist() == [[1, -1, 0, -1, 1, -1], [-1] * 6, [-1] * 6, [0, -1, -1, 0, 0, 0]]
    rank, score = rank_model(ids, None, None, gt, 2)
    assert score is None and rank.tolist() == [[1, 5], [0, 1], [0, 1], [0, -1]]


def test_ceiling_model_by_hand():
    rank = np.array([[0, 70, -1, 5], [-2, -2, -2, -2], [300, 2, 64, 63]], np.int32)
    hits, ceil = ceiling_model(rank, (4, 1, 2), (64, 256))
    assert hits[0].tolist() == [[2, -1, 2], [1, -1, 0], [1, -1, 1]]
    assert hits[1].tolist() == [[3, -1, 3], [1, -1, 0], [2, -1, 1]]
    assert hits[2].tolist() == [[3, -1, 4], [1, -1, 1], [2, -1, 2]]
    assert ceil[0, 0, 0] == 0.5 and ceil[2, 0, 2] == 1.0 and ceil[1, 2, 2] == 0.5 and np.isnan(ceil[:, :, 1]).all()
    hits, ceil = ceiling_model(rank, (4,), ())
    assert hits.shape == (1, 1, 3) and hits[0, 0].tolist() == [3, -1, 4]


# ---- header, library, binding --------------------------------------------------------------------------------------------------
def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fspann_[a-z0-9_]+)\s*\(", txt)))


def test_route_recall_entry_points_are_exported_and_bound(pkg):
    pkg._native.build()
    L = pkg._native.lib()
    assert _declared("fspann_route_recall.h") == sorted(ROUTE_RECALL)
    assert pkg._native.route_recall_symbols() == sorted(ROUTE_RECALL)
    for s in ROUTE_RECALL:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
        for other in ("exported_symbols", "rows_symbols", "eval_symbols", "validate_symbols", "plan_symbols", "sweep_symbols", "narrow_symbols"):
            assert s not in getattr(pkg._native, other)(), (s, other)
    for m in ("gt_rank_dev", "recall_ceiling_dev", "route_recall"):
        assert hasattr(pkg.FspannContext, m), m
    import inspect
    assert "attribution" in inspect.signature(pkg.FspannContext.run_queries).parameters


def test_exported_symbols_are_still_fspann_h_and_the_jni_shim_is_untouched(pkg):
    assert pkg._native.exported_symbols() == _declared("fspann.h")
    assert len(pkg._native.exported_symbols()) == 94
    bound = open(os.path.join(ROOT, "jni", "bound_symbols.txt")).read().split()
    assert sorted(bound) == _declared("fspann.h")
    for f in ("jni/fspann_jni.cpp", "java/com/fspann/gpu/FspannNative.java"):
        txt = open(os.path.join(ROOT, f)).read()
        for s in ROUTE_RECALL:
            assert s not in txt, (f, s)


def test_header_is_a_build_input(pkg):
    """a change of the header rebuilds the library"""
    import inspect
    assert "fspann_route_recall.h" in inspect.getsource(pkg._native.needs_build)


def test_null_context_without_gpu(pkg):
    import ctypes as C
    N = pkg._native
    L = N.lib()
    ks = (C.c_int32 * 1)(1)
    assert L.fspann_gt_rank_dev(None, 1, None, None, 4, None, None, 4, 1, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
    assert L.fspann_recall_ceiling_dev(None, 1, None, 4, ks, 1, None, 0, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()


def test_operator_twin_defaults_are_the_reference_s(pkg):
    """QSI:63-65: with no id set the twin reports what the reference always reports"""
    from fspann_amd import operators as ops
    host = ops.InMemoryHost()
    cfg = ops.SystemConfig(m=8, lambda_=2, divisions=1, tables=2)
    qs = ops.QueryServiceImpl(ops.PartitionedIndexService(host, cfg, host, host), host, host, None, cfg)
    assert qs.getLastTrueNNRank() == -1 and qs.wasLastTrueNNSeen() is False
    qs.setTrueNearestId("12")
    assert qs.search(None) == [] and qs.getLastTrueNNRank() == -1 and qs.wasLastTrueNNSeen() is False
    qs.lastTrueNNRank, qs.lastTrueNNSeen = 3, True
    qs.clearLastMetrics()
    assert qs.getLastTrueNNRank() == -1 and qs.wasLastTrueNNSeen() is False
