"""GPU: the Route coverage map (include/fspann_route_coverage.h).  The raw calls against the numpy models of
tests/test_route_coverage_cpu.py, bit for bit and with canaries behind every output, over imported tables of many shapes; route_coverage
on a scene whose answer is not trivial (asserted from the oracle as preconditions) against one-table oracles (the records), sub-grid
oracles (the prediction) and route_recall (the ceiling at the index's own tables and divisions); the argument guards; a clone."""
import ctypes as C

import numpy as np
import pytest

import index_shapes as ish
from test_route_coverage_cpu import CoverageScene, assert_not_trivial, coverage_model, full_grid, probe_lists, reach_from_lists

pytestmark = pytest.mark.gpu

CANARY = -77
NQ = 10
KGS = (1, 7, 1024)
PROBES = (1, 2, 32)


# ---- device calls with canaries ------------------------------------------------------------------------------------------------
def _reach(ctx, qcodes, gt, kg, P):
    """fspann_gt_reach_dev over device copies; (reach [nq][kg][TD], the canaries behind it)"""
    import torch
    dev = torch.device("cuda", 0)
    nq, TD = qcodes.shape[0], qcodes.shape[1]
    cd = torch.from_numpy(np.ascontiguousarray(qcodes).view(np.int64)).to(dev)
    gd = torch.from_numpy(np.ascontiguousarray(gt, np.int32)).to(dev)
    out = torch.full((nq * kg * TD + 16,), CANARY, dtype=torch.int32, device=dev)
    ctx.gt_reach_dev(nq, cd.data_ptr(), P, gd.data_ptr(), gt.shape[1], kg, out.data_ptr())
    ctx.sync()
    o = out.cpu().numpy()
    return o[:nq * kg * TD].reshape(nq, kg, TD), o[nq * kg * TD:]


def _coverage(ctx, reach, rp, ks, grid, want_ceiling=True, want_score=True):
    import torch
    dev = torch.device("cuda", 0)
    nq, kg, _ = reach.shape
    nc, nk = len(grid), len(ks)
    rd = torch.from_numpy(np.ascontiguousarray(reach)).to(dev)
    hits = torch.full((nc * nk * nq + 16,), CANARY, dtype=torch.int32, device=dev)
    ceil = torch.full((nc * nk * nq + 16,), -7.0, dtype=torch.float64, device=dev)
    score = torch.full((nc * nq * kg + 16,), CANARY, dtype=torch.int32, device=dev)
    exact = ctx.route_coverage_dev(nq, rd.data_ptr(), kg, rp, ks, grid, hits.data_ptr(), ceil.data_ptr() if want_ceiling else 0,
                                   score.data_ptr() if want_score else 0)
    ctx.sync()
    return hits.cpu().numpy(), ceil.cpu().numpy(), score.cpu().numpy(), exact


def _check_coverage(ctx, reach, rp, ks, grid, T, D, S, hard_cap):
    nq, kg, _ = reach.shape
    want = coverage_model(reach, T, D, ks, grid, S, hard_cap)
    hits, ceil, score, exact = _coverage(ctx, reach, rp, ks, grid)
    n, ns = want["hits"].size, want["score"].size
    assert np.array_equal(hits[:n].reshape(want["hits"].shape), want["hits"]) and (hits[n:] == CANARY).all()
    assert np.array_equal(ceil[:n].reshape(want["ceiling"].shape).view(np.uint64), want["ceiling"].view(np.uint64)) and (ceil[n:] == -7.0).all()
    assert np.array_equal(score[:ns].reshape(want["score"].shape), want["score"]) and (score[ns:] == CANARY).all()
    assert np.array_equal(exact, want["exact"])
    hits2, ceil2, score2, exact2 = _coverage(ctx, reach, rp, ks, grid, want_ceiling=False, want_score=False)
    assert np.array_equal(hits2, hits) and (ceil2 == -7.0).all() and (score2 == CANARY).all() and np.array_equal(exact2, exact)
    return want


# ---- a. the raw calls over imported tables of many shapes -----------------------------------------------------------------------
def _ragged(S):
    def tables(sc):
        """ragged partitions with empties; table 1: one partition of 11 ids (its probe list is shorter than P); table 2: no partitions;
        table 3: every second id only"""
        tb = ish.ragged_tables(sc, S, seed=5)
        tb[1] = ish.cut(tb[1]["ids"][:11], sc["codes_h"][:, 1], [11])
        tb[2] = ish.empty_table(1)
        tb[3] = ish.subset(tb[3], np.arange(sc["params"]["n"]) % 2 == 0, sc["codes_h"][:, 3], S)
        return tb
    return tables


SHAPES = {
    "ragged 16": (dict(), 16, _ragged(16)),                                        # T x D = 6 x 1
    "ragged 100": (dict(), 100, _ragged(100)),
    "ragged 128": (dict(), 128, _ragged(128)),
    "17 tables": (dict(T=17, n=2000, seed=62), 64, None),                          # more tables than lane groups: two rounds
    "one table": (dict(T=1, n=2000, seed=63), 64, None),
    "two words": (dict(d=20, T=2, D=2, m=40, lam=3, seed=14), 64, None),           # m * lambda = 120 bits
}


def _second_id_at_step_0(tables, lists_q):
    """the second id of the first partition of two or more ids that the query polls first in its table"""
    for td, lst in enumerate(lists_q):
        if lst:
            ids = tables[td]["ids"][tables[td]["id_off"][lst[0][0]]:tables[td]["id_off"][lst[0][0] + 1]]
            if len(ids) >= 2:
                return int(ids[1])
    raise AssertionError("no query-first partition of two ids")


def _gt_rows(rng, lists, tables, kg, stride, n_ids, dead):
    """per query: an id polled at step 0, -1, the same id again, an id >= n_ids, the query's deleted id, an id polled at the last step
    of some table — rotated by the query's index, so that kg = 1 meets each of them — then polled ids and random ids, half and half;
    the columns past kg hold polled ids (never read)"""
    nq = len(lists)
    gt = np.empty((nq, stride), np.int32)
    for q in range(nq):
        polled, at0, last = [], None, None
        for td, ix in enumerate(tables):
            for s, (part, _) in enumerate(lists[q][td]):
                ids = ix["ids"][ix["id_off"][part]:ix["id_off"][part + 1]]
                polled.append(ids)
                if s == 0 and at0 is None:
                    alive = ids[~np.isin(ids, dead)]
                    at0 = int(alive[0]) if len(alive) else None
                if len(ids) and s == len(lists[q][td]) - 1:
                    last = int(ids[-1])
        polled = np.concatenate(polled)
        special = np.roll(np.array([at0, -1, at0, n_ids + 5, dead[q], last], np.int32), q)
        body = np.where(rng.random(kg + stride) < 0.5, rng.choice(polled, kg + stride), rng.integers(0, n_ids, kg + stride)).astype(np.int32)
        gt[q] = np.concatenate([special, body])[:stride] if kg >= 6 else np.concatenate([special[:kg], rng.choice(polled, stride - kg)])
    return gt


@pytest.mark.parametrize("shape", list(SHAPES))
def test_raw_calls_against_the_models(pkg, oracle, shape):
    over, S, tables_of = SHAPES[shape]
    sc = ish.scene(oracle, **over)
    p = sc["params"]
    tables = ish.uniform_tables(sc, S) if tables_of is None else tables_of(sc)
    qcodes = np.ascontiguousarray(sc["qcodes"][:NQ])
    lists = probe_lists(tables, qcodes, max(PROBES))
    rng = np.random.default_rng(77)
    dead = np.array([_second_id_at_step_0(tables, lists[q]) for q in range(NQ)], np.int32)      # one deleted id per query
    deleted = np.zeros(p["n"], bool)
    deleted[dead] = True
    with ish.make_ctx(pkg, sc, block_size=S) as ctx:
        ish.import_tables(ctx, tables)
        ctx.set_deleted(dead)
        for kg in KGS:
            gt = _gt_rows(rng, lists, tables, kg, kg + 5, p["n"], dead)
            for P in PROBES:
                want = reach_from_lists(tables, lists, gt, kg, P, p["n"], deleted)
                got, tail = _reach(ctx, qcodes, gt, kg, P)
                assert np.array_equal(got, want), (kg, P, np.argwhere(got != want)[:8])
                assert (tail == CANARY).all()
                if kg == 1024:                     # the cases the rows were made for are there
                    rows = np.arange(NQ)
                    assert (want[gt[:, :kg] == dead[:, None]] == -1).all() and (want[gt[:, :kg] < 0] == -1).all() and (want[gt[:, :kg] >= p["n"]] == -1).all()
                    sp = [int(np.flatnonzero(np.roll(np.arange(6), q) == 0)[0]) for q in range(NQ)]          # where the step-0 id sits
                    again = [int(np.flatnonzero(np.roll(np.arange(6), q) == 2)[0]) for q in range(NQ)]
                    assert np.array_equal(want[rows, sp], want[rows, again]) and (want[rows, sp].max(1) >= 0).all()
                    assert ((want >= 0) & ((want >> 16) == P - 1)).any() or P == 32
                T, D = p["T"], p["D"]
                grid = [(T, D, P), (1, 1, 1), (T, 1, max(1, P // 2)), (1, D, P)] + [(int(rng.integers(1, T + 1)), int(rng.integers(1, D + 1)),
                                                                                       int(rng.integers(1, P + 1))) for _ in range(60 if kg == 7 else 3)]
                ks = sorted({kg, 1, min(kg, 10), min(kg, 100), max(1, kg - 1)}, reverse=True)
                cov = _check_coverage(ctx, got, P, ks, grid, T, D, S, max(p["hard_cap"], p["B"]))
                if kg == 1024:
                    assert 0 < cov["hits"][0, 0].min()
        # an empty batch: nothing is read or written
        ctx.gt_reach_dev(0, 0, 3, 0, 4, 4, 0)
        assert np.array_equal(ctx.route_coverage_dev(0, 0, 4, 3, (1,), [(1, 1, 3)], 0), [3 * S < max(p["hard_cap"], p["B"])])


def test_64_ks_and_64_configs(pkg, oracle):
    """the largest argument block: 64 k values and 64 configurations over synthetic records"""
    sc = ish.scene(oracle, T=17, n=2000, seed=62)
    rng = np.random.default_rng(78)
    kg, TD, nq = 130, 17, 5
    reach = np.where(rng.random((nq, kg, TD)) < 0.7, -1, (rng.integers(0, 32, (nq, kg, TD)) << 16) | rng.integers(0, 25, (nq, kg, TD))).astype(np.int32)
    grid = [(int(rng.integers(1, 18)), 1, int(rng.integers(1, 33))) for _ in range(64)]
    ks = [int(x) for x in rng.integers(1, kg + 1, 64)]
    with ish.make_ctx(pkg, sc, block_size=64) as ctx:
        ish.import_tables(ctx, ish.uniform_tables(sc, 64))
        _check_coverage(ctx, reach, 32, ks, grid, 17, 1, 64, max(sc["params"]["hard_cap"], sc["params"]["B"]))


# ---- b. the scene, through route_coverage ----------------------------------------------------------------------------------------
KS = (1, 10, 20)


@pytest.fixture(scope="module")
def cscene(oracle):
    return CoverageScene(oracle)


def _scene_ctx(pkg, s):
    ctx = ish.make_ctx(pkg, s.sc, block_size=s.S)
    ish.import_tables(ctx, s.tables)
    ctx.store_set(s.sc["X"])
    return ctx


def test_route_coverage_against_the_oracle(pkg, cscene):
    s = cscene
    cube = full_grid(s.T, s.D, s.P)
    grid = cube + cube[::-1]                         # 72 configurations: two groups
    records = s.one_table_records(s.gt, s.P)
    # preconditions, from the oracle alone: the answer is not trivial
    assert_not_trivial(records)
    model = coverage_model(records, s.T, s.D, KS, cube, s.S, s.hard_cap)
    assert len({round(float(x), 9) for x in model["ceiling"][:, 2].mean(1)}) >= 3
    assert model["exact"].any() and not model["exact"].all()
    with _scene_ctx(pkg, s) as ctx:
        got = ctx.route_coverage(s.Q, KS, grid)
        given = ctx.route_coverage(s.Q, KS, pkg.coverage_grid(range(1, s.T + 1), range(1, s.D + 1), range(1, s.P + 1)),
                                   gt_ids=np.pad(s.gt, ((0, 0), (0, 3)), constant_values=-1), probes_max=s.P)
        recall = {P: ctx.route_recall(s.Q, KS, probe_override=P, gt_ids=s.gt)["route_ceiling"] for P in range(1, s.P + 1)
                  if s.T * s.D * P * s.S < s.hard_cap}
    assert np.array_equal(got["gt_ids"], s.gt)
    want = records.reshape(s.nq, s.K, s.T, s.D)
    assert np.array_equal(got["step"], np.where(want >= 0, want >> 16, -1)) and np.array_equal(got["hamming"], np.where(want >= 0, want & 0xFFFF, -1))
    assert got["hits"].shape == (72, len(KS), s.nq) and got["score"].shape == (72, s.nq, s.K) and np.array_equal(got["grid"], np.array(grid))
    assert np.array_equal(got["exact"], [t * d * p * s.S < s.hard_cap for t, d, p in grid])
    for key in ("hits", "ceiling", "score", "exact"):
        assert np.array_equal(got[key][:36], given[key]) and np.array_equal(got[key][36:], given[key][::-1]), key
    for key in ("gt_ids", "step", "hamming"):
        assert np.array_equal(got[key], given[key]), key
    offered = got["score"] >= 0
    for j, k in enumerate(KS):
        assert np.array_equal(got["hits"][:, j], offered[:, :, :k].sum(2))
        assert np.array_equal(got["ceiling"][:, j].view(np.uint64), (got["hits"][:, j] / float(k)).view(np.uint64))
    # exact configurations are the sub-grid oracles' lists, as ids and as scores; capped ones are supersets
    s.check_prediction(s.gt, dict(exact=given["exact"], offered=given["score"] >= 0, score=given["score"]), cube)
    # at the index's own tables and divisions the ceiling is route_recall's, as doubles, where the cap cannot bind
    compared = 0
    for c, (t, d, p) in enumerate(cube):
        if (t, d) == (s.T, s.D) and given["exact"][c]:
            assert np.array_equal(given["ceiling"][c].view(np.uint64), recall[p].view(np.uint64)), p
            compared += 1
    assert compared >= 2


def test_a_clone_gives_the_same_records(pkg, cscene):
    s = cscene
    gt = np.ascontiguousarray(s.gt)
    with _scene_ctx(pkg, s) as ctx:
        mine, _ = _reach(ctx, s.qcodes, gt, s.K, s.P)
        with ctx.clone() as twin:
            theirs, tail = _reach(twin, s.qcodes, gt, s.K, s.P)
            cov = twin.route_coverage(s.Q, KS, [(s.T, s.D, s.P)], gt_ids=gt)
    assert np.array_equal(mine, theirs) and (tail == CANARY).all() and (mine >= 0).any()
    assert np.array_equal(cov["step"].reshape(mine.shape), np.where(mine >= 0, mine >> 16, -1))


# ---- c. argument guards ----------------------------------------------------------------------------------------------------------
def test_argument_errors(pkg, cscene):
    import torch
    s = cscene
    dev = torch.device("cuda", 0)
    inp = torch.zeros(1 << 16, dtype=torch.int32, device=dev)               # every input: codes, ground truth and records of zeros
    outs = [torch.zeros(1 << 16, dtype=torch.int32, device=dev) for _ in range(3)]
    dbl = torch.zeros(4096, dtype=torch.float64, device=dev)
    p, (o1, o2, o3), d = inp.data_ptr(), (t.data_ptr() for t in outs), dbl.data_ptr()
    with _scene_ctx(pkg, s) as ctx:
        def reach(nq=2, codes=p, P=3, gt=p, gs=8, kg=4, out=o1):
            ctx.gt_reach_dev(nq, codes, P, gt, gs, kg, out)

        def cover(nq=2, r=p, kg=4, rp=3, ks=(4, 1), grid=((3, 2, 3), (1, 1, 1)), hits=o2, c=d, sc=o3):
            return ctx.route_coverage_dev(nq, r, kg, rp, ks, grid, hits, c, sc)
        reach(), cover()                             # the defaults are a legal call each
        for kw, name in ((dict(P=0), "probes_max"), (dict(P=33), "probes_max"), (dict(kg=0), "kg"), (dict(kg=1025, gs=2000), "kg"),
                         (dict(gs=3), "gt_stride"), (dict(codes=0), "codes_dev"), (dict(gt=0), "gt_ids_dev"), (dict(out=0), "reach_dev"),
                         (dict(nq=-1), "nq")):
            with pytest.raises(pkg.FspannArgumentError, match=name):
                reach(**kw)
        for kw, name in ((dict(grid=((4, 1, 1),)), "tables"), (dict(grid=((1, 3, 1),)), "divisions"), (dict(grid=((1, 1, 4),)), "probes"),
                         (dict(grid=((1, 1, 1), (0, 1, 1))), r"grid\[1\]"), (dict(grid=((1, 0, 1),)), "divisions"), (dict(grid=((1, 1, 0),)), "probes"),
                         (dict(ks=(1,) * 65), "nk"), (dict(ks=()), "nk"), (dict(grid=((1, 1, 1),) * 65), "nc"), (dict(grid=()), "nc"),
                         (dict(ks=(4, 5)), r"ks\[1\]"), (dict(ks=(0,)), r"ks\[0\]"), (dict(kg=0), "kg"), (dict(kg=1025), "kg"),
                         (dict(rp=0), "reach_probes"), (dict(rp=33), "reach_probes"), (dict(r=0), "reach_dev"), (dict(hits=0), "hits_dev"),
                         (dict(nq=-1), "nq")):
            with pytest.raises(pkg.FspannArgumentError, match=name):
                cover(**kw)
        one, three = (C.c_int32 * 1)(1), (C.c_int32 * 3)(1, 1, 1)
        for ks_, grid_, name in ((None, three, "ks is null"), (one, None, "grid is null")):
            assert ctx.L.fspann_route_coverage_dev(ctx.handle, 2, p, 4, 3, ks_, 1, grid_, 1, o2, None, None, None) == pkg._native.E_ARG
            assert name.encode() in ctx.L.fspann_last_error()
        cover(c=0, sc=0)                             # the optional pointers
        reach(nq=0, codes=0, gt=0, out=0), cover(nq=0, r=0, hits=0, c=0, sc=0)      # an empty batch: nothing to do
        ctx.sync()
    assert not inp.any()
    cfg = pkg.PaperRuntimeConfig(tables=2, divisions=1, m=8, lambda_=2, dim=16)
    with pkg.FspannContext(cfg, 0) as bare:          # no index yet
        with pytest.raises(pkg.FspannStateError, match="not finalized"):
            bare.gt_reach_dev(2, p, 3, p, 8, 4, o1)
        with pytest.raises(pkg.FspannStateError, match="not finalized"):
            bare.route_coverage_dev(2, p, 4, 3, (1,), ((1, 1, 1),), o2)
