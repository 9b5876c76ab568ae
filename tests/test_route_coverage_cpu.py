"""CPU: what can be asked of include/fspann_route_coverage.h without a device — the numpy models of both calls (reach_model: the
probe step and Hamming score at which Route reaches a ground-truth id, per table; coverage_model: offered, score, hits, ceiling and
exact of every (tables, divisions, probes)) that tests/test_gpu_route_coverage.py compares the device against, and the two claims the
header rests on, checked against the oracle: the record equals what one-table oracles report when they route at 1 .. P probes, and
the prediction for (T', D', P) equals the list of an oracle that holds only the sub-grid's tables."""
import os
import re

import numpy as np
import pytest

import index_shapes as ish

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERAGE = ("fspann_gt_reach_dev", "fspann_route_coverage_dev")


# ---- the models ----------------------------------------------------------------------------------------------------------------
def _hamming_to(rep, code):
    """popcount(rep[p] ^ code) of every partition p"""
    x = np.ascontiguousarray(rep ^ code[None, :])
    return np.unpackbits(x.view(np.uint8).reshape(len(rep), -1), axis=1).sum(1).astype(np.int64)


def _nearest(mn, mx, key):
    """GreedyPartitioner.findNearestPartition (:101-124) over the key ranges it is given"""
    lo, hi = 0, len(mn) - 1
    while lo <= hi:
        mid = (lo + hi) >> 1
        if key < mn[mid]:
            hi = mid - 1
        elif key > mx[mid]:
            lo = mid + 1
        else:
            return mid
    if lo <= 0:
        return 0
    if lo >= len(mn):
        return len(mn) - 1

    def dist(p):
        return mn[p] - key if key < mn[p] else key - mx[p] if key > mx[p] else 0
    return lo - 1 if dist(lo - 1) <= dist(lo) else lo


def probe_list(ix, code, P):
    """[(partition, hamming)] in the order lookupCandidatesWithScores polls one table for one query code [W] (PIS:638-685): the
    nearest partition first, then best-first over the neighbours of what was polled, through a java.util.PriorityQueue that never
    holds more than two entries — a newcomer becomes the head only if strictly smaller."""
    npart = len(ix["min_key"])
    if npart == 0:
        return []
    ham = _hamming_to(ix["rep"], np.asarray(code, np.uint64))
    center = _nearest(ix["min_key"].tolist(), ix["max_key"].tolist(), int(ish.keys_of(np.asarray(code[:1], np.uint64))[0]))
    heap, lo, hi, out = [center], center, center, []
    while heap and len(out) < P:
        cur = heap.pop(0)
        out.append((cur, int(ham[cur])))
        for nb in (cur - 1, cur + 1):
            if 0 <= nb < npart and (nb < lo or nb > hi):
                lo, hi = min(lo, nb), max(hi, nb)
                assert len(heap) < 2
                if heap and ham[nb] < ham[heap[0]]:
                    heap.insert(0, nb)
                else:
                    heap.append(nb)
    return out


def probe_lists(tables, qcodes, P):
    """probe_list of every (query, table): [nq][TD] lists"""
    return [[probe_list(ix, qcodes[q, td], P) for td, ix in enumerate(tables)] for q in range(qcodes.shape[0])]


def reach_from_lists(tables, lists, gt, kg, probes_max, n_ids, deleted=None):
    """fspann_gt_reach_dev from probe lists of at least probes_max entries: reach [nq][kg][TD] = (step << 16) | hamming or -1"""
    nq, TD = len(lists), len(tables)
    reach = np.full((nq, kg, TD), -1, np.int32)
    for q in range(nq):
        row = np.asarray(gt[q, :kg]).astype(np.int64)
        live = (row >= 0) & (row < n_ids)
        if deleted is not None:
            live &= ~np.asarray(deleted, bool)[np.where(live, row, 0)]
        where = {}
        for i in np.flatnonzero(live):
            where.setdefault(int(row[i]), []).append(int(i))
        if not where:
            continue
        wanted = np.fromiter(where, np.int64)
        for td, ix in enumerate(tables):
            for s, (part, ham) in enumerate(lists[q][td][:probes_max]):
                ids = ix["ids"][ix["id_off"][part]:ix["id_off"][part + 1]]
                for id_ in ids[np.isin(ids, wanted)].tolist():
                    for i in where[id_]:
                        if reach[q, i, td] < 0:                    # (the earlier step wins, with that step's Hamming)
                            reach[q, i, td] = (s << 16) | ham
    return reach


def reach_model(tables, qcodes, gt, kg, probes_max, n_ids, deleted=None):
    return reach_from_lists(tables, probe_lists(tables, qcodes, probes_max), gt, kg, probes_max, n_ids, deleted)


def coverage_model(reach, T, D, ks, grid, block_size, hard_cap):
    """fspann_route_coverage_dev: dict(offered bool [nc][nq][kg], score int32 [nc][nq][kg], hits int32 / ceiling float64
    [nc][nk][nq], exact bool [nc]) from reach [nq][kg][T * D]"""
    nq, kg, TD = reach.shape
    assert TD == T * D
    r = reach.reshape(nq, kg, T, D).astype(np.int64)
    step, ham = np.where(r >= 0, r >> 16, -1), r & 0xFFFF
    nc, nk = len(grid), len(ks)
    offered = np.zeros((nc, nq, kg), bool)
    score = np.full((nc, nq, kg), -1, np.int32)
    hits = np.zeros((nc, nk, nq), np.int32)
    ceil = np.zeros((nc, nk, nq), np.float64)
    exact = np.zeros(nc, bool)
    for c, (tc, dc, pc) in enumerate(np.asarray(grid).tolist()):
        m = (step[:, :, :tc, :dc] >= 0) & (step[:, :, :tc, :dc] < pc)
        offered[c] = m.any((2, 3))
        score[c] = np.where(offered[c], np.where(m, ham[:, :, :tc, :dc], 1 << 20).min((2, 3)), -1)
        for j, k in enumerate(ks):
            hits[c, j] = offered[c][:, :k].sum(1)
            ceil[c, j] = hits[c, j] / float(k)
        exact[c] = tc * dc * pc * block_size < hard_cap
    return dict(offered=offered, score=score, hits=hits, ceiling=ceil, exact=exact)


# ---- the models on cases small enough to read -----------------------------------------------------------------------------------
def _toy_table():
    """five partitions of two ids over keys 0 .. 9 of a 4-bit code (the key reverses the bits under bit 62): codes are chosen by key"""
    def code_of(key):
        return np.array([int("{:063b}".format(key)[::-1], 2)], np.uint64)
    keys = np.arange(10)
    codes = np.stack([code_of(int(k) << 59) for k in keys])              # the key's top four bits: code bits 0 .. 3
    return ish.cut(np.arange(10, dtype=np.int32), codes, [2, 2, 2, 2, 2]), codes


def test_probe_list_by_hand():
    ix, codes = _toy_table()
    assert ish.ascends(ix) and ix["min_key"].tolist() == [k << 59 for k in (0, 2, 4, 6, 8)]
    # the query has id 5's code: partition 2 (keys 4, 5; rep = id 4's code, one bit away); then the neighbours by Hamming to their reps
    lst = probe_list(ix, codes[5], 5)
    ham = _hamming_to(ix["rep"], codes[5]).tolist()
    assert lst[0] == (2, ham[2]) and {p for p, _ in lst} == {0, 1, 2, 3, 4} and all(h == ham[p] for p, h in lst)
    assert [p for p, _ in lst[:3]] == ([2, 1, 3] if ham[1] <= ham[3] else [2, 3, 1])[:3]
    for P in (1, 2, 3, 4):
        assert probe_list(ix, codes[5], P) == lst[:P]                     # the order at P probes is a prefix
    assert probe_list(ish.empty_table(1), codes[5], 3) == []


def test_reach_and_coverage_models_by_hand():
    ix, codes = _toy_table()
    other = ish.cut(np.array([9, 8, 7, 6], np.int32), codes, [4])         # one partition, four ids: the list is shorter than P
    tables = [ix, other, ish.empty_table(1), ix]                          # T = 2, D = 2
    q = np.stack([codes[5]] * 4)[None]
    gt = np.array([[5, 4, 9, -1, 5, 12, 0, 3]], np.int32)
    lst = probe_list(ix, codes[5], 5)
    step = {p: s for s, (p, _) in enumerate(lst)}
    ham = {p: h for p, h in lst}
    deleted = np.zeros(10, bool)
    deleted[3] = True
    reach = reach_model(tables, q, gt, 8, 2, 10, deleted)

    def rec(id_):
        p = id_ // 2
        return (step[p] << 16) | ham[p] if step[p] < 2 else -1
    h_other = int(_hamming_to(other["rep"], codes[5])[0])
    want = [[rec(5), -1, -1, rec(5)], [rec(4), -1, -1, rec(4)], [rec(9), h_other, -1, rec(9)], [-1] * 4, [rec(5), -1, -1, rec(5)], [-1] * 4,
            [rec(0), -1, -1, rec(0)], [-1] * 4]
    assert reach[0].tolist() == want and rec(5) == ham[2] and rec(0) == -1
    cov = coverage_model(reach, 2, 2, (1, 8), [(1, 1, 1), (1, 2, 1), (2, 2, 2)], 2, 6)
    assert cov["offered"][0, 0].tolist() == [True, True, False, False, True, False, False, False]
    assert cov["offered"][1, 0].tolist() == [True, True, True, False, True, False, False, False]
    assert cov["score"][1, 0].tolist() == [ham[2], ham[2], h_other, -1, ham[2], -1, -1, -1]
    assert cov["hits"][:, :, 0].tolist() == [[1, 3], [1, 4], [1, 4]] and cov["ceiling"][1, 1, 0] == 0.5
    assert cov["exact"].tolist() == [True, True, False]


# ---- the two claims, against the oracle -------------------------------------------------------------------------------------------
class CoverageScene:
    """n = 3 000 points of dimension 16, T = 3, D = 2, m = 8, lambda = 2, the oracle's tables cut again in blocks of 16, 24 queries,
    K = 20, records at up to 6 probes, HARD_CAP 200: configurations of up to 12 probed partitions cannot meet it."""
    n, d, T, D, m, lam, S, nq, K, P, hard_cap = 3000, 16, 3, 2, 8, 2, 16, 24, 20, 6, 200

    def __init__(self, O, tables=None):
        self.O = O
        sc = ish.scene(O, nq=self.nq, n=self.n, d=self.d, T=self.T, D=self.D, m=self.m, lam=self.lam, B=64, hard_cap=self.hard_cap, seed=61)
        self.sc = sc
        self.tables = ish.uniform_tables(sc, self.S) if tables is None else tables(sc)
        self.Q, self.qcodes = sc["Q"], sc["qcodes"]
        self.gt = O.groundtruth(sc["X"], self.Q, self.K)[0]
        self.deleted = None

    def one_table_records(self, gt, P):
        """reach [nq][K][TD] as the reference reports it: table td alone in an Oracle(1, 1), routed at 1 .. P probes; the step of an
        id is the smallest probe count at which it is in the list, less one, its Hamming the score it has there"""
        nq, kg = gt.shape
        reach = np.full((nq, kg, self.T * self.D), -1, np.int32)
        for td, ix in enumerate(self.tables):
            o1 = self.O.Oracle(1, 1, self.m, self.lam, self.d, max_global_candidates=20000, refinement_limit=64)
            o1.set_gfunctions(self.sc["alpha"][td:td + 1], self.sc["r"][td:td + 1], self.sc["omega"][td:td + 1])
            o1.set_id_meta(self.n, None, self.deleted)
            o1.set_index(0, **ix)
            for p in range(1, P + 1):
                ids, score, count, _ = o1.route(self.qcodes[:, td:td + 1], probe_override=p)
                for q in range(nq):
                    at = {int(i): int(s) for i, s in zip(ids[q, :count[q]], score[q, :count[q]])}
                    for i in range(kg):
                        if reach[q, i, td] < 0 and int(gt[q, i]) in at:
                            reach[q, i, td] = ((p - 1) << 16) | at[int(gt[q, i])]
        return reach

    def subgrid_lists(self, tc, dc, pc):
        """per query {id: score} of lookupCandidatesWithScores in an Oracle(tc, dc) that holds the tables t < tc, d < dc, at pc probes"""
        tds = [t * self.D + d for t in range(tc) for d in range(dc)]
        o2 = self.O.Oracle(tc, dc, self.m, self.lam, self.d, max_global_candidates=self.hard_cap, refinement_limit=64)
        o2.set_gfunctions(self.sc["alpha"][tds], self.sc["r"][tds], self.sc["omega"][tds])
        o2.set_id_meta(self.n, None, self.deleted)
        for j, td in enumerate(tds):
            o2.set_index(j, **self.tables[td])
        ids, score, count, _ = o2.route(self.qcodes[:, tds], probe_override=pc)
        return [{int(i): int(s) for i, s in zip(ids[q, :count[q]], score[q, :count[q]])} for q in range(self.nq)]

    def check_prediction(self, gt, cov, grid):
        """exact configurations: the ground-truth ids in the sub-grid oracle's list and their scores are offered and score; the
        others: the oracle's set is a subset of offered"""
        for c, (tc, dc, pc) in enumerate(np.asarray(grid).tolist()):
            lists = self.subgrid_lists(tc, dc, pc)
            for q in range(self.nq):
                inlist = np.array([int(g) in lists[q] for g in gt[q]])
                if cov["exact"][c]:
                    assert np.array_equal(inlist, cov["offered"][c, q]), (tc, dc, pc, q)
                    want = [lists[q][int(g)] if ok else -1 for g, ok in zip(gt[q], inlist)]
                    assert cov["score"][c, q].tolist() == want, (tc, dc, pc, q)
                else:
                    assert not (inlist & ~cov["offered"][c, q]).any(), (tc, dc, pc, q)


def full_grid(T, D, P):
    return [(t, d, p) for t in range(1, T + 1) for d in range(1, D + 1) for p in range(1, P + 1)]


@pytest.fixture(scope="module")
def cscene(oracle):
    return CoverageScene(oracle)


def test_the_record_is_what_one_table_oracles_report(cscene):
    s = cscene
    want = s.one_table_records(s.gt, s.P)
    got = reach_model(s.tables, s.qcodes, s.gt, s.K, s.P, s.n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    for P in (1, 3):                                 # fewer probes cut the same order off
        assert np.array_equal(reach_model(s.tables, s.qcodes, s.gt, s.K, P, s.n), np.where((want >> 16) < P, want, -1))
    assert_not_trivial(want)


def assert_not_trivial(records):
    """some true neighbours are not reached at all, some are reached first at a step >= 1, some in one table only"""
    step = np.where(records >= 0, records >> 16, -1)
    first = np.where(step >= 0, step, 99).min(2)
    assert (step.max(2) < 0).any() and ((first >= 1) & (first < 99)).any() and ((step >= 0).sum(2) == 1).any()


def test_the_record_on_imported_shapes_and_deleted_ids(oracle):
    """ragged partitions with empties, a table with one partition, a table with none, a table that holds every second id; ground-truth
    rows with deleted ids, padding, a repeat and an id >= n_ids"""
    def tables(sc):
        tb = ish.ragged_tables(sc, 16, seed=5)
        tb[1] = ish.cut(tb[1]["ids"][:11], sc["codes_h"][:, 1], [11])
        tb[2] = ish.empty_table(1)
        tb[3] = ish.subset(tb[3], np.arange(sc["params"]["n"]) % 2 == 0, sc["codes_h"][:, 3], 16)
        return tb
    s = CoverageScene(oracle, tables)
    gt = s.gt.copy()
    s.deleted = np.zeros(s.n, np.uint8)
    s.deleted[gt[:, 2]] = 1
    want = s.one_table_records(gt, s.P)
    assert (want[:, 2] == -1).all() and (want[:, :, 2] == -1).all() and (want[:, :, 1] >= 0).sum() < (want[:, :, 0] >= 0).sum()
    gt[:, 5], gt[:, 6], gt[:, 7] = -1, gt[:, 0], s.n + 3
    want[:, 5], want[:, 6], want[:, 7] = -1, want[:, 0], -1
    got = reach_model(s.tables, s.qcodes, gt, s.K, s.P, s.n, s.deleted)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_the_prediction_is_the_sub_grid_oracle_s_list(cscene):
    s = cscene
    grid = [(1, 1, 1), (1, 2, 3), (2, 1, 6), (3, 1, 4), (2, 2, 3), (3, 2, 2), (2, 2, 5), (3, 2, 6)]
    reach = reach_model(s.tables, s.qcodes, s.gt, s.K, s.P, s.n)
    cov = coverage_model(reach, s.T, s.D, (1, 10, 20), grid, s.S, s.hard_cap)
    assert cov["exact"].tolist() == [True, True, True, True, True, True, False, False]
    s.check_prediction(s.gt, cov, grid)
    assert len({round(float(x), 6) for x in cov["ceiling"][:, 2].mean(1)}) >= 3


# ---- header, library, binding --------------------------------------------------------------------------------------------------
def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fspann_[a-z0-9_]+)\s*\(", txt)))


def test_coverage_entry_points_are_exported_and_bound(pkg):
    pkg._native.build()
    L = pkg._native.lib()
    assert _declared("fspann_route_coverage.h") == sorted(COVERAGE)
    assert pkg._native.coverage_symbols() == sorted(COVERAGE)
    for s in COVERAGE:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
        for other in ("exported_symbols", "rows_symbols", "eval_symbols", "validate_symbols", "plan_symbols", "sweep_symbols", "narrow_symbols",
                      "route_recall_symbols"):
            assert s not in getattr(pkg._native, other)(), (s, other)
    for m in ("gt_reach_dev", "route_coverage_dev", "route_coverage"):
        assert hasattr(pkg.FspannContext, m), m
    assert pkg.coverage_grid((1, 2), (3,), (4, 5)).tolist() == [[1, 3, 4], [1, 3, 5], [2, 3, 4], [2, 3, 5]]
    import inspect
    assert "fspann_route_coverage.h" in inspect.getsource(pkg._native.needs_build)


def test_fspann_h_and_the_jni_shim_are_untouched(pkg):
    assert pkg._native.exported_symbols() == _declared("fspann.h") and len(pkg._native.exported_symbols()) == 94
    for f in ("jni/fspann_jni.cpp", "java/com/fspann/gpu/FspannNative.java", "jni/bound_symbols.txt"):
        txt = open(os.path.join(ROOT, f)).read()
        for s in COVERAGE:
            assert s not in txt, (f, s)


def test_null_context_without_gpu(pkg):
    import ctypes as C
    N = pkg._native
    L = N.lib()
    ks, grid = (C.c_int32 * 1)(1), (C.c_int32 * 3)(1, 1, 1)
    assert L.fspann_gt_reach_dev(None, 1, None, 1, None, 1, 1, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
    assert L.fspann_route_coverage_dev(None, 1, None, 1, 1, ks, 1, grid, 1, None, None, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
