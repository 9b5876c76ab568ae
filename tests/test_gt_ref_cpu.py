"""CPU: tests/gt_ref.py, the plain numpy restatement of GroundtruthPrecompute and computeMetricsAtK that the GPU tests
test_gpu_metrics_fold.py and test_gpu_gt_select_ties.py take their expected values from, against the oracle: bit for bit (ids, and
the raw fp64 of distances, recall and ratio) on every finite data set those tests use but the one of n > 2^24, each made by the
generator in gt_ref.py that the GPU test calls.  And a condition on the data, not a measurement: every metrics data set with k > 64
can tell the ratio's index-order fold from three wrong ones, and the recall over k places from the recall over the first 64."""
import numpy as np
import pytest

import gt_ref as R


def _same_knn(oracle, V, Q, k):
    ids, d2, nan0 = R.knn(V, Q, k)
    oid, od2 = oracle.groundtruth(V, Q, k)
    assert np.array_equal(ids, oid) and np.array_equal(d2, od2)
    assert (nan0 == min(k, len(V))).all()
    return ids, d2


def test_d2_is_the_sequential_java_sum():
    """one row, one query, by hand: float subtraction, widened, squared and added in dimension order"""
    rng = np.random.default_rng(1)
    v, q = rng.standard_normal(37).astype(np.float32), rng.standard_normal(37).astype(np.float32)
    s = 0.0
    for i in range(37):
        df = np.float32(q[i] - v[i])
        s += float(df) * float(df)
    assert R.d2(v[None], q[None])[0, 0] == s
    assert R.l2(q.astype(np.float64), v.astype(np.float64)[None])[0] == np.sqrt(
        R.fold_index([(float(q[i]) - float(v[i])) ** 2 for i in range(37)]))


@pytest.mark.parametrize("n", R.S_IDENT_N)
def test_knn_all_rows_identical(oracle, n):
    V, Q = R.sel_identical(n)
    for k in R.S_IDENT_K:
        ids, d2 = _same_knn(oracle, V, Q, k)
        kk = min(k, n)
        assert (ids[:, :kk] == np.arange(kk)).all() and (ids[:, kk:] == -1).all() and np.isposinf(d2[:, kk:]).all()


def test_knn_tie_group_across_the_two_byte_id_boundary(oracle):
    V, Q = R.sel_boundary()
    assert R.sel_boundary_ids(136, False)[-1] == 65535 and R.sel_boundary_ids(137, False)[-1] == 65536
    for k in R.S_BOUND_K:
        ids, d2 = _same_knn(oracle, V, Q, k)
        for i in range(len(Q)):
            assert np.array_equal(ids[i], R.sel_boundary_ids(k, i == R.S_BOUND_FARQ)), (k, i)
    assert len(set(d2[0])) == 2 and d2[0, 0] == 0               # k = 1000: the group and the lowest far ids


def test_knn_keys_that_differ_in_the_low_mantissa_bytes(oracle):
    V, Q = R.sel_mantissa()
    D = R.d2(V, Q)[0]
    j = np.rint(V[:, 1].astype(np.float64) * 2.0 ** 26)
    grid = (V[:, 0] == 1) & (V[:, 1] >= 2.0 ** -26)
    assert grid.sum() > 2990 and np.array_equal(D[grid], 1 + j[grid] ** 2 * 2.0 ** -52)
    assert len(set((D[grid].view(np.uint64) >> 24).tolist())) == 1       # the top five bytes of those keys are one value
    assert D[17] == 0 and D[400] == 1 and 0 < D[2501] < D[2500] < 1e-80
    for k in R.S_MANT_K:
        _same_knn(oracle, V, Q, k)


@pytest.mark.parametrize("kind", ("normal", "ints"))
def test_knn_k_1024(oracle, kind):
    for n in R.S_K1024_N:
        _same_knn(oracle, *R.sel_k1024(n, kind), 1024)
    for n in (1, 300):
        ids, _ = _same_knn(oracle, *R.sel_k1024(n, kind), 1024)
        assert (ids[:, n:] == -1).all()


def test_knn_tile_edges(oracle):
    for nq in R.S_TILE_NQ:
        for n in R.S_TILE_N:
            for d in R.S_TILE_D:
                _same_knn(oracle, *R.sel_tiles(nq, n, d), 4)


def test_knn_nonfinite_rows_sort_as_the_contract_says():
    """(no oracle here: the data set is not finite.)  +inf distances tie by id, NaN distances come last, in id order"""
    V, Q = R.sel_nonfinite()
    ids, d2, nan0 = R.knn(V, Q, len(V))
    D = R.d2(V, Q)
    for i in range(len(Q)):
        assert nan0[i] == (~np.isnan(D[i])).sum() and 0 < nan0[i] < len(V)
        assert not np.isnan(d2[i, :nan0[i]]).any() and np.isnan(d2[i, nan0[i]:]).all()
        key = list(zip(d2[i, :nan0[i]], ids[i, :nan0[i]]))
        assert key == sorted(key)
    assert np.isposinf(d2[1]).sum() >= 10 and np.isposinf(d2[2]).sum() >= 9


@pytest.mark.parametrize("d,k", R.M_SHAPES)
@pytest.mark.parametrize("bdt,qdt", R.M_PAIRS)
def test_metrics_equal_the_oracle_and_the_data_tell_the_folds_apart(oracle, bdt, qdt, d, k):
    sc = R.metrics_scene(bdt, qdt, d, k)
    X, Q, n = sc["X"], sc["Q"], sc["n"]
    gt, gd2 = _same_knn(oracle, X, Q, k + 7)
    # the planted edges are where the GPU test's docstring says
    assert np.array_equal(gd2, sc["gd2"]) and (gt[R.Q_PLAIN] == sc["gt"][R.Q_PLAIN]).all()
    assert sc["ann"][R.Q_TAIL, k // 2] in gt[R.Q_TAIL, k:] and sc["ann"][R.Q_TAIL, k // 2] not in gt[R.Q_TAIL, :k]
    bad = [int(sc["ann"][R.Q_BAD0 + j, p]) for j in range(3) for p in R.bad_places(k)]
    assert {-1, n, R.I32_MAX} <= set(bad)
    assert (sc["gt"][[R.Q_BAD0, R.Q_BAD0 + 1, R.Q_BAD0 + 2]] >= 0).all()
    if k > 64:
        hole = np.flatnonzero(sc["gt"][R.Q_GTHOLE, :k] == -1)
        assert len(hole) == 1 and hole[0] >= 64 and (sc["ann"][R.Q_GTHOLE] >= 0).all()
    if k > 70 and d == 24:
        assert gd2[R.Q_ROW70, 0] == 0 and gd2[R.Q_ROW70, 1] > 0 and sc["gt"][R.Q_ROW70, 70] == gt[R.Q_ROW70, 0]
    X64, Q64 = X.astype(np.float64), Q.astype(np.float64)
    for ann_stride in (k, k + 5):
        ann, cnt, g = R.metrics_call(sc, ann_stride, k + 7)
        for counts in (cnt, None):
            rec, rat = R.metrics(X64, Q64, k, ann, counts, g)
            orec, orat = oracle.metrics(X, Q, k, ann, counts, g)
            assert np.array_equal(rec, orec)
            assert np.array_equal(np.isnan(rat), np.isnan(orat)) and np.array_equal(rat[~np.isnan(rat)], orat[~np.isnan(orat)])
            defined = [R.Q_PLAIN, R.Q_TAIL, R.Q_CLAMP] + ([R.Q_SHORT, R.Q_NONE, R.Q_NEG] if counts is None else [])
            defined += ([R.Q_GTHOLE] if k <= 64 else []) + ([R.Q_ROW70] if k <= 70 else [])
            assert np.array_equal(np.flatnonzero(~np.isnan(rat)), sorted(defined)), np.flatnonzero(~np.isnan(rat))
    if k <= 64:
        return
    # the condition: a fold in the wrong order, a dropped round or a recall over the first round only gives other bits somewhere
    assert R.folds_not_told_apart(sc) == []


def test_metrics_tiny_case(oracle):
    sc = R.tiny_scene()
    X64, Q64 = sc["X"].astype(np.float64), sc["Q"].astype(np.float64)
    rec, rat = R.metrics(X64, Q64, 5, sc["ann"], sc["cnt"], sc["gt"])
    orec, orat = oracle.metrics(sc["X"], sc["Q"], 5, sc["ann"], sc["cnt"], sc["gt"])
    assert np.array_equal(rec, orec) and np.array_equal(np.isnan(rat), np.isnan(orat)) and rat[0] == orat[0]
    assert np.array_equal(rec, [1.0, 0.8, 0.8]) and np.isnan(rat[1:]).all() and rat[0] > 1
