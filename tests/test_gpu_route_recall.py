"""GPU: recall attribution (include/fspann_route_recall.h) — the rank of the ground truth in a candidate list and the recall ceilings
it implies.  The raw calls on synthetic lists against the numpy model of tests/test_route_recall_cpu.py, word for word; route_recall
and run_queries(attribution=True) against the oracle's lookupCandidatesWithScores lists on a scene whose answer is not trivial (its
figures are asserted from the oracle as preconditions); the prediction itself — the ceiling at limit B equals the recall limit_sweep
measures at B wherever no distance tie sits on the k boundary; a host-resolved (treeified) query; the operator twin."""
import numpy as np
import pytest

import fallback_ref as FR
from test_route_recall_cpu import ceiling_model, rank_model

pytestmark = pytest.mark.gpu

CANARY = -77
INT32_MAX = 2**31 - 1
KS = (1, 10, 20)
LIMITS = (64, 256, 1024)


# ---- a. the rank call, raw -----------------------------------------------------------------------------------------------------
COUNTS = (0, -1, 1, 3, 255, 256, 257, 1030, 1031)
STRIDE = 1031


def _lists(nq, stride, seed, dup_row=None):
    """nq lists of different ids below 8 * stride (one id twice in dup_row) and their scores"""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(8 * stride)[:stride] for _ in range(nq)]).astype(np.int32)
    if dup_row is not None:
        ids[dup_row, 700] = ids[dup_row, 10]
    score = rng.integers(0, 48, (nq, stride)).astype(np.int32)
    return ids, score, rng


def _gt_rows(ids, counts, kg, gt_stride, rng):
    """per query: the id at position 0, the id at position c - 1, an id found only at a position >= c, a repeated id, -1 padding, an
    id larger than any in the list, the list's doubled id — rotated by the query's index so that kg = 1 meets each of them — then
    ids of which about one in eight is in the list; the columns past kg hold ids of the list (never read)"""
    nq, stride = ids.shape
    gt = np.empty((nq, gt_stride), np.int32)
    for q in range(nq):
        c = min(stride if counts is None else int(counts[q]), stride)
        special = [ids[q, 0], ids[q, max(c, 1) - 1], ids[q, min(max(c, 0), stride - 1)], ids[q, 0], -1, 10**6, ids[q, 10]]
        row = np.concatenate([np.roll(np.array(special, np.int32), q), rng.integers(0, 8 * stride, kg).astype(np.int32)])[:kg]
        gt[q, :kg] = row
        gt[q, kg:] = ids[q, 1:1 + gt_stride - kg]
    return gt


def _gt_rank(ctx, ids, score, counts, gt, kg, lead=0):
    """fspann_gt_rank_dev over device copies (the lists start `lead` entries into their allocation); rank and gt_score come back with
    the canaries behind them"""
    import torch
    dev = torch.device("cuda", 0)
    nq, stride = ids.shape

    def up(a):
        t = torch.full((a.size + lead,), CANARY, dtype=torch.int32, device=dev)
        t[lead:] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev)
        return t
    li, gd = up(ids), torch.from_numpy(gt).to(dev)
    ls = up(score) if score is not None else None
    lc = torch.from_numpy(np.asarray(counts, np.int32)).to(dev) if counts is not None else None
    rank = torch.full((nq * kg + 16,), CANARY, dtype=torch.int32, device=dev)
    gs = torch.full((nq * kg + 16,), CANARY, dtype=torch.int32, device=dev)
    ctx.gt_rank_dev(nq, li.data_ptr() + 4 * lead, ls.data_ptr() + 4 * lead if ls is not None else 0, stride, lc.data_ptr() if lc is not None else 0,
                    gd.data_ptr(), gt.shape[1], kg, rank.data_ptr(), gs.data_ptr() if ls is not None else 0)
    ctx.sync()
    return rank.cpu().numpy(), gs.cpu().numpy()


def _bare_ctx(pkg):
    return pkg.FspannContext(pkg.PaperRuntimeConfig(tables=2, divisions=1, m=8, lambda_=2, dim=16), 0)


@pytest.mark.parametrize("kg", [1, 7, 1024])
@pytest.mark.parametrize("variant", ["counts+scores", "no counts", "no scores", "base off the 16-byte grid"])
def test_gt_rank_on_synthetic_lists(pkg, kg, variant):
    nq = len(COUNTS)
    ids, score, rng = _lists(nq, STRIDE, 11, dup_row=COUNTS.index(1030))
    counts = None if variant == "no counts" else np.array(COUNTS, np.int32)
    sc = None if variant == "no scores" else score
    gt = _gt_rows(ids, counts, kg, kg + 5, rng)
    want_rank, want_score = rank_model(ids, sc, counts, gt, kg)
    with _bare_ctx(pkg) as ctx:
        rank, gs = _gt_rank(ctx, ids, sc, counts, gt, kg, lead=3 if variant.startswith("base") else 0)
    assert np.array_equal(rank[:nq * kg].reshape(nq, kg), want_rank), np.argwhere(rank[:nq * kg].reshape(nq, kg) != want_rank)[:8]
    assert (rank[nq * kg:] == CANARY).all()
    if sc is None:
        assert (gs == CANARY).all()              # gt_score is not written
    else:
        assert np.array_equal(gs[:nq * kg].reshape(nq, kg), want_score) and (gs[nq * kg:] == CANARY).all()
    if counts is not None and kg >= 7:           # the cases the rows were made for are there
        assert (want_rank[COUNTS.index(-1)] == -2).all() and (want_rank[COUNTS.index(0)] == -1).all()
        q = COUNTS.index(1030)
        assert 10 in want_rank[q] and 1029 in want_rank[q] and 0 in want_rank[q] and 700 not in want_rank[q]
        assert (want_rank[COUNTS.index(1031)] == 1030).any() and (want_rank[COUNTS.index(257)] == 256).any()


def test_gt_rank_on_the_longest_list_route_writes(pkg):
    """HARD_CAP + block_size - 1 = 20 063 entries: an odd stride, so the three rows start 0, 12 and 8 bytes off the 16-byte grid"""
    nq, stride, kg = 3, 20063, 100
    ids, score, rng = _lists(nq, stride, 12)
    counts = np.full(nq, stride, np.int32)
    gt = _gt_rows(ids, counts, kg, kg, rng)
    gt[:, 7:40] = ids[:, -33:]                   # the tail of each list, its last entry included
    gt[:, 40:60] = ids[:, 1:21]
    want_rank, want_score = rank_model(ids, score, counts, gt, kg)
    assert (want_rank == stride - 1).any() and (want_rank >= 0).sum() > 50 * nq
    with _bare_ctx(pkg) as ctx:
        rank, gs = _gt_rank(ctx, ids, score, counts, gt, kg)
    assert np.array_equal(rank[:nq * kg].reshape(nq, kg), want_rank) and np.array_equal(gs[:nq * kg].reshape(nq, kg), want_score)
    assert (rank[nq * kg:] == CANARY).all() and (gs[nq * kg:] == CANARY).all()


# ---- b. the ceiling call, raw --------------------------------------------------------------------------------------------------
def _ceiling(ctx, rank, ks, limits, want_ceiling=True):
    import torch
    dev = torch.device("cuda", 0)
    nq, planes = rank.shape[0], (len(limits) + 1) * len(ks)
    rd = torch.from_numpy(rank).to(dev)
    hits = torch.full((planes * nq + 16,), CANARY, dtype=torch.int32, device=dev)
    ceil = torch.full((planes * nq + 16,), -7.0, dtype=torch.float64, device=dev)
    ctx.recall_ceiling_dev(nq, rd.data_ptr(), rank.shape[1], ks, limits, hits.data_ptr(), ceil.data_ptr() if want_ceiling else 0)
    ctx.sync()
    return hits.cpu().numpy(), ceil.cpu().numpy()


@pytest.mark.parametrize("limits", [(), (256,), (1, 2, 3, 5, 8, 13, 64, 100, 256, 257, 500, 1000, 1030, 1031, 5000, INT32_MAX)])
def test_recall_ceiling_raw(pkg, limits):
    ks = (20, 1, 10, 10)
    nq = len(COUNTS) + 2
    rng = np.random.default_rng(21)
    rank = np.where(rng.random((nq, 25)) < 0.3, -1, rng.integers(0, 1031, (nq, 25))).astype(np.int32)
    rank[1] = -2                                 # a flagged query nobody resolved
    rank[2] = -1
    rank[3, :20] = np.arange(20)
    rank[4, 20:] = -2                            # beyond every k: not looked at
    want_hits, want_ceil = ceiling_model(rank, ks, limits)
    assert (want_hits[:, :, 1] == -1).all() and (want_hits[:, :, 4] >= 0).all() and want_hits[-1, 0, 3] == 20
    n = want_hits.size
    with _bare_ctx(pkg) as ctx:
        hits, ceil = _ceiling(ctx, rank, ks, limits)
        hits2, ceil2 = _ceiling(ctx, rank, ks, limits, want_ceiling=False)
    assert np.array_equal(hits[:n].reshape(want_hits.shape), want_hits) and (hits[n:] == CANARY).all()
    got = ceil[:n].reshape(want_ceil.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want_ceil)) and np.isnan(got[:, :, 1]).all()
    assert np.array_equal(np.nan_to_num(got, nan=-1.0).view(np.uint64), np.nan_to_num(want_ceil, nan=-1.0).view(np.uint64))
    assert (ceil[n:] == -7.0).all()
    assert np.array_equal(hits2, hits) and (ceil2 == -7.0).all()


# ---- c. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors(pkg):
    import torch
    dev = torch.device("cuda", 0)
    inp = torch.zeros(4096, dtype=torch.int32, device=dev)                  # every input: lists, counts, ground truth and ranks of zeros
    outs = [torch.zeros(4096, dtype=torch.int32, device=dev) for _ in range(3)]
    dbl = torch.zeros(4096, dtype=torch.float64, device=dev)
    p, (o1, o2, o3), d = inp.data_ptr(), (t.data_ptr() for t in outs), dbl.data_ptr()
    with _bare_ctx(pkg) as ctx:
        def rank(nq=2, li=p, ls=p, stride=8, lc=p, gt=p, gs=8, kg=4, out=o1, osc=o2):
            ctx.gt_rank_dev(nq, li, ls, stride, lc, gt, gs, kg, out, osc)

        def ceil(nq=2, r=p, rs=8, ks=(4, 1), limits=(2, 4), hits=o3, c=d):
            ctx.recall_ceiling_dev(nq, r, rs, ks, limits, hits, c)
        rank(), ceil()                           # the defaults are a legal call each
        for kw, name in ((dict(kg=0), "kg"), (dict(kg=1025, gs=2000), "kg"), (dict(gs=3), "gt_stride"), (dict(stride=0), "list_stride"),
                         (dict(li=0), "list_ids_dev"), (dict(gt=0), "gt_ids_dev"), (dict(out=0), "rank_dev"), (dict(ls=0), "list_score_dev"),
                         (dict(osc=0), "gt_score_dev"), (dict(nq=-1), "nq")):
            with pytest.raises(pkg.FspannArgumentError, match=name):
                rank(**kw)
        for kw, name in ((dict(ks=()), "nk"), (dict(ks=(1,) * 65), "nk"), (dict(ks=(4, 9)), r"ks\[1\]"), (dict(ks=(0,)), r"ks\[0\]"),
                         (dict(limits=(4, 4)), "ascending"), (dict(limits=(4, 2)), "ascending"), (dict(limits=(0, 2)), r"limits\[0\]"),
                         (dict(limits=(1, 2**31)), r"limits\[1\]"), (dict(limits=tuple(range(1, 18))), "nl"), (dict(r=0), "rank_dev"),
                         (dict(hits=0), "hits_dev"), (dict(nq=-1), "nq")):
            with pytest.raises(pkg.FspannArgumentError, match=name):
                ceil(**kw)
        rank(ls=0, osc=0), ceil(c=0), ceil(limits=())                # the optional pointers, no limits
        rank(nq=0, li=0, gt=0, out=0), ceil(nq=0, r=0, hits=0)         # an empty batch: nothing to do
        ctx.sync()
    assert not inp.any()


# ---- d - f. a scene where the answer is not trivial ----------------------------------------------------------------------------
class Scene:
    """Integer-valued data (exact distances: no rounding can reorder true neighbours) on a low-rank cloud, built as make_scene
    builds its scenes: registry_init(X64[:1000], m, 13, T, D), the oracle's own index, hard_cap 20 000."""
    n, d, T, D, m, lam, nq, B = 20000, 32, 6, 2, 12, 2, 64, 256

    def __init__(self, O):
        rng = np.random.default_rng(5)
        r, noise = 8, 6.0
        U = (rng.standard_normal((r, self.d)) / np.sqrt(r)).astype(np.float32)

        def draw(cnt):
            y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
            y = 64.0 + 48.0 * y + noise * rng.standard_normal((cnt, self.d), dtype=np.float32)
            return np.clip(np.rint(y), 0, 255).astype(np.float32)
        self.X, self.Q = draw(self.n), draw(self.nq)
        X64 = self.X.astype(np.float64)
        self.g = O.registry_init(X64[:1000], self.m, 13, self.T, self.D)
        o = O.Oracle(self.T, self.D, self.m, self.lam, self.d, max_global_candidates=20000, refinement_limit=self.B, probe_override=-1, hamming_threshold=0)
        o.set_gfunctions(*self.g)
        o.set_id_meta(self.n, None, None)
        o.set_store(X64)
        o.build_index(X64)
        self.o = o
        self.codes = o.encode(self.Q.astype(np.float64))
        # exact integer k-NN ordered by (d, id), one more than K: the (k + 1)-th distance says whether a tie sits on the k boundary
        Qi, Xi = self.Q.astype(np.int64), self.X.astype(np.int64)
        d2 = (Qi * Qi).sum(1)[:, None] + (Xi * Xi).sum(1)[None, :] - 2 * (Qi @ Xi.T)
        order = np.argsort(d2, axis=1, kind="stable")[:, :max(KS) + 1]           # (stable over ascending ids: ordered by (d, id))
        self.gt = order[:, :max(KS)].astype(np.int32)
        dk = np.take_along_axis(d2, order, 1)
        self.qualifies = np.stack([dk[:, k - 1] != dk[:, k] for k in KS])              # [nk][nq]
        self.lists = {}
        for po, probes in ((-1, 5), (10, 10)):
            ids, score, count, _ = o.route(self.codes, probe_override=po)
            self.lists[probes] = (ids, score, count, o.route_treeified(self.codes, probe_override=po))

    def ranks(self, probes_per_query, gt=None):
        """rank, gt_score [nq][K] of the ground truth in the oracle's list at each query's probes (numpy)"""
        gt = self.gt if gt is None else gt
        rank = np.full(gt.shape, -1, np.int32)
        score = np.full(gt.shape, -1, np.int32)
        for q, p in enumerate(probes_per_query):
            ids, sc, count, _ = self.lists[int(p)]
            r, s = rank_model(ids[q:q + 1], sc[q:q + 1], count[q:q + 1], gt[q:q + 1], gt.shape[1])
            rank[q], score[q] = r[0], s[0]
        return rank, score

    def context(self, pkg):
        cfg = pkg.PaperRuntimeConfig(tables=self.T, divisions=self.D, m=self.m, lambda_=self.lam, dim=self.d, refinement_limit=self.B,
                                     max_global_candidates=20000)
        ctx = pkg.FspannContext(cfg, 0)
        ctx.set_gfunctions(*self.g)
        ctx.set_id_meta(self.n)
        ctx.build_index(self.X)
        ctx.store_set(self.X)
        return ctx


@pytest.fixture(scope="module")
def scene(oracle):
    return Scene(oracle)


def _pct(x):
    return round(100.0 * float(x), 1)


def test_the_scene_is_not_trivial(scene):
    """the figures of the scene, from the oracle alone: what the other tests rest on"""
    K = max(KS)
    for probes, kept, found, first in ((5, (2621, 3242), 96.9, (8.0, 27.9, 76.7)), (10, (4640, 6090), 99.5, (7.2, 27.3, 72.6))):
        ids, score, count, tree = scene.lists[probes]
        assert (int(count.min()), int(count.max())) == kept and not tree.any()
        rank, _ = scene.ranks([probes] * scene.nq)
        assert _pct((rank >= 0).mean()) == found
        assert tuple(_pct(((rank >= 0) & (rank < b)).mean()) for b in LIMITS) == first
        if probes == 5:
            assert int(((rank < 0).any(1)).sum()) == 27
    assert scene.qualifies.shape == (len(KS), scene.nq) and int(scene.qualifies.sum()) == 191


@pytest.mark.parametrize("po,probes", [(-1, 5), (10, 10)])
def test_route_recall_against_the_oracle(pkg, scene, po, probes):
    ids, score, count, _ = scene.lists[probes]
    want_rank, want_score = scene.ranks([probes] * scene.nq)
    want_hits, want_ceil = ceiling_model(want_rank, KS, LIMITS)
    with scene.context(pkg) as ctx:
        got = ctx.route_recall(scene.Q, KS, limits=LIMITS, probe_override=po)
        given = ctx.route_recall(scene.Q, KS, limits=LIMITS, gt_ids=np.pad(scene.gt, ((0, 0), (0, 3)), constant_values=-1), probe_override=po)
    assert np.array_equal(got["gt_ids"], scene.gt)                   # exact integer k-NN ordered by (d, id)
    assert np.array_equal(got["rank"], want_rank) and np.array_equal(got["gt_score"], want_score)
    assert np.array_equal(got["kept"], count) and got["resolved"] == 0
    assert got["hits"].shape == (len(LIMITS) + 1, len(KS), scene.nq) and np.array_equal(got["hits"], want_hits)
    assert np.array_equal(got["ceiling"].view(np.uint64), want_ceil.view(np.uint64))
    assert np.array_equal(got["route_ceiling"], want_ceil[-1])
    assert np.array_equal(got["true_nn_rank"], want_rank[:, 0]) and np.array_equal(got["true_nn_seen"], want_rank[:, 0] >= 0)
    for key in got:
        assert np.array_equal(np.asarray(given[key]), np.asarray(got[key])), key


def _qualifying(scene):
    assert (~scene.qualifies).sum() <= 0.1 * scene.qualifies.size      # a condition that keeps the test honest, not a measurement
    return scene.qualifies


def test_the_ceiling_predicts_what_limit_sweep_measures(pkg, scene):
    """At 10 probes pass 2 of the retry would reproduce pass 1, so every plane of limit_sweep is at 10 probes.  With distinct k-th and
    (k + 1)-th exact distances a true neighbour inside the first B candidates is one of the k nearest of those B: recall at limit B is
    the ceiling at B, as doubles."""
    with scene.context(pkg) as ctx:
        swept = ctx.limit_sweep(scene.Q, LIMITS, KS, probe_override=10)
        pred = ctx.route_recall(scene.Q, KS, limits=LIMITS, probe_override=10)
    ok = _qualifying(scene)
    for l in range(len(LIMITS)):
        a, b = swept["recall"][l][ok], pred["ceiling"][l][ok]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (LIMITS[l], np.argwhere(swept["recall"][l] != pred["ceiling"][l])[:8])
    assert 0 < pred["ceiling"][0].mean() < pred["ceiling"][2].mean() < pred["route_ceiling"].mean() < 1


TODAY = {"ids", "dist", "count", "scored", "sel_count", "bad", "retried", "fellback", "resolved", "gt_ids", "recall", "ratio", "cand_ratio"}
EXTRA = {"last_probes", "gt_rank", "route_ceiling", "limit_ceiling", "true_nn_rank", "true_nn_seen"}


@pytest.mark.parametrize("B,probes", [(256, 5), (64, 10)])
def test_run_queries_attribution(pkg, scene, B, probes):
    """B = 256: scored = 256 >= 10 K, nobody retries, the last pass is at the default probes; B = 64: everybody retries"""
    want_rank, _ = scene.ranks([probes] * scene.nq)
    _, want_ceil = ceiling_model(want_rank, KS, (B,))
    with scene.context(pkg) as ctx:
        plain = ctx.run_queries(scene.Q, KS, B=B)
        got = ctx.run_queries(scene.Q, KS, B=B, attribution=True)
    assert set(plain) == TODAY and set(got) == TODAY | EXTRA
    for key in TODAY:
        assert np.array_equal(np.asarray(plain[key]), np.asarray(got[key])), key
    assert (got["retried"] != 0).all() == (probes == 10) and not got["fellback"].any()
    assert np.array_equal(got["last_probes"], np.full(scene.nq, probes, np.int32))
    assert np.array_equal(got["gt_rank"], want_rank)
    assert np.array_equal(got["route_ceiling"].view(np.uint64), want_ceil[1].view(np.uint64))
    assert np.array_equal(got["limit_ceiling"].view(np.uint64), want_ceil[0].view(np.uint64))
    ok = _qualifying(scene)
    assert np.array_equal(got["limit_ceiling"][ok].view(np.uint64), got["recall"][ok].view(np.uint64))
    assert np.array_equal(got["true_nn_rank"], got["gt_rank"][:, 0]) and np.array_equal(got["true_nn_seen"], got["gt_rank"][:, 0] >= 0)


def test_run_queries_attribution_follows_the_fallback_rule(pkg, oracle):
    """fallback_ref.main_scene: queries 0-3 fall back at F = 4, 1 and 2 retry inside the fallback, 4 stays empty, 5-23 keep search 1
    (cfg.probe_override = 2) — of which 11, 12 and 23 retried inside search 1 (the oracle's own metrics, asserted here), so their
    last pass ran at 10 probes and the others' at 2.  The ranks are taken in the oracle's lists at those probes, the scene's deleted
    ids in place: a deleted true neighbour is never offered."""
    sc, Q, K, ref, fb, r1, r2 = FR.main_scene(oracle)
    o = sc["oracle"]
    codes = FR.codes_of(o, Q)
    assert np.flatnonzero(r1["metrics"][:, 4]).tolist() == [11, 12, 23]
    want_last = np.array([4, 10, 10, 4, 4] + [10 if q in (11, 12, 23) else 2 for q in range(5, 24)], np.int32)
    assert np.array_equal(want_last, np.where(ref["metrics"][:, 4] != 0, 10, np.where(fb != 0, 4, 2)))      # 10 if retried, else F if fell back
    lists = {p: o.route(codes, probe_override=p) for p in (2, 4, 10)}
    for q in (11, 12, 23):                       # the rows these three keep are pass 2's: F_q is the head of the list at 10 probes, not at 2
        n = int(r1["sel_count"][q])
        assert n > 0 and np.array_equal(r1["sel"][q, :n], lists[10][0][q, :n]) and not np.array_equal(r1["sel"][q, :n], lists[2][0][q, :n])
    with FR.context(pkg, sc) as ctx:
        got = ctx.run_queries(Q, (1, K), attribution=True)
    assert got["last_probes"].tolist() == want_last.tolist()
    gt = got["gt_ids"]
    want = np.empty((len(Q), K), np.int32)
    for p in (2, 4, 10):
        ids, score, count, _ = lists[p]
        sel = np.flatnonzero(want_last == p)
        want[sel] = rank_model(ids[sel], None, count[sel], gt[sel], K)[0]
    assert np.array_equal(got["gt_rank"], want)
    dead = sc["deleted"][gt].astype(bool)
    assert dead.any() and (got["gt_rank"][dead] == -1).all() and (got["gt_rank"][4] == -1).all() and (got["gt_rank"][5:] >= 0).any()
    assert np.array_equal(got["true_nn_rank"], want[:, 0])


def test_non_finite_queries_are_left_out(pkg, scene):
    """a bad query is never coded or searched: run_queries leaves its ranks at -1 and its ceilings at 0, route_recall refuses it
    as encode() does; the other queries' answers do not move"""
    Q = scene.Q[:8].copy()
    Q[3, 5] = np.nan
    Q[6, 0] = np.inf
    want_rank, _ = scene.ranks([5] * scene.nq)
    with scene.context(pkg) as ctx:
        got = ctx.run_queries(Q, KS, attribution=True)
        with pytest.raises(pkg.FspannArgumentError, match="NaN/Inf"):
            ctx.route_recall(Q, KS)
    bad = np.array([0, 0, 0, 1, 0, 0, 1, 0], bool)
    assert np.array_equal(got["bad"] != 0, bad)
    assert (got["gt_rank"][bad] == -1).all() and not got["true_nn_seen"][bad].any()
    assert (got["route_ceiling"][:, bad] == 0).all() and (got["limit_ceiling"][:, bad] == 0).all()
    assert np.array_equal(got["gt_rank"][~bad], want_rank[:8][~bad])


# ---- g. a host-resolved query --------------------------------------------------------------------------------------------------
def test_route_recall_over_a_treeified_query(pkg, oracle):
    """hashCodes that crowd three bins (the scene builder of tests/test_gpu_treeify.py): the flagged queries are finished by the host
    model, so no rank is -2 and every rank is the position in the oracle's list"""
    from conftest import make_scene
    from test_gpu_treeify import _crowded_distinct_hashes, _ctx, _import
    rng = np.random.default_rng(900)
    n = int(rng.integers(1500, 6000))
    sc = make_scene(oracle, n=n, d=12, T=4, D=2, m=8, lam=2, B=64, hard_cap=20000, seed=40)
    o = sc["oracle"]
    jh = _crowded_distinct_hashes(rng, n, 3, oracle.table_size_for(20000))
    o.set_id_meta(n, jh)
    o.build_index(sc["X64"])
    Q = rng.standard_normal((32, 12)).astype(np.float32)
    codes = o.encode(Q.astype(np.float64))
    flagged = o.route_treeified(codes)
    ids, score, count, _ = o.route(codes)
    assert flagged.any() and not o.unmodelled
    with _ctx(pkg, sc, jh) as ctx:
        _import(ctx, o)
        ctx.store_set(sc["X"])
        got = ctx.route_recall(Q, (1, 10), limits=(64,))
    want_rank, want_score = rank_model(ids, score, count, got["gt_ids"], 10)
    assert got["resolved"] == int(flagged.sum()) >= 1
    assert (got["rank"] != -2).all() and (got["hits"] >= 0).all()
    assert np.array_equal(got["rank"], want_rank) and np.array_equal(got["gt_score"], want_score) and np.array_equal(got["kept"], count)
    assert (want_rank[flagged] >= 0).any()


# ---- h. the operator twin ------------------------------------------------------------------------------------------------------
def test_operator_twin_true_nearest_rank(pkg):
    """QueryServiceImpl.setTrueNearestId / getLastTrueNNRank / wasLastTrueNNSeen over the golden scene it_unified: the rank is the
    position in the lookupCandidatesWithScores list of the search's last pass — 5 probes, or 10 once the adaptive retry ran"""
    from fspann_amd import operators as ops
    from golden_util import load_scene_inputs
    g, X = load_scene_inputs("it_unified")
    T, D, m, lam, d, B, K, n = (int(g[k]) for k in ("T", "D", "m", "lam", "d", "B", "K", "n"))
    cfg = ops.SystemConfig(m=m, lambda_=lam, divisions=D, tables=T, seed=int(g["seed"]), refinementLimit=B, maxGlobalCandidates=int(g["hard_cap"]),
                           kVariants=(K,))
    host = ops.InMemoryHost()
    ops.GFunctionRegistry.reset()
    index = ops.PartitionedIndexService(host, cfg, host, host)

    def where(probes, qi, id):
        lst = g[f"route{probes}_ids"][qi, :int(g[f"route{probes}_count"][qi])]
        at = np.flatnonzero(lst == id)
        return (int(at[0]), True) if at.size else (-1, False)
    try:
        for i in range(n):
            index.insert(str(i), X[i])
        index.finalizeForSearch()
        tf = ops.QueryTokenFactory(host, host, cfg)
        qs = ops.QueryServiceImpl(index, host, host, tf, cfg)
        toks = tf.createBatch(list(g["Q"]), K)
        assert not g["search_metrics"][:, 4].any()                                  # nobody retries at B = 128
        res = qs.search(toks[0])
        assert [int(r.id) for r in res] == list(g["search_ids"][0, :K])
        assert (qs.getLastTrueNNRank(), qs.wasLastTrueNNSeen()) == (-1, False)       # no id set: the reference's answer
        for qi in range(len(toks)):
            nn = int(g["search_ids"][qi, 0])
            qs.setTrueNearestId(str(nn))
            assert [int(r.id) for r in qs.search(toks[qi])] == list(g["search_ids"][qi, :K])
            assert (qs.getLastTrueNNRank(), qs.wasLastTrueNNSeen()) == where(5, qi, nn) and qs.wasLastTrueNNSeen()
        absent = int(np.setdiff1d(np.arange(n), g["route5_ids"][0, :int(g["route5_count"][0])])[0])
        qs.setTrueNearestId(str(absent))
        qs.search(toks[0])
        assert (qs.getLastTrueNNRank(), qs.wasLastTrueNNSeen()) == (-1, False)
        # a refinement limit below 10 K makes the search retry with 10 probes: the rank is taken in that pass's list
        nn = int(g["search_ids"][1, 0])
        qs.setTrueNearestId(str(nn))
        qs.setRefinementLimit(50)
        qs.search(toks[1])
        assert (qs.getLastTrueNNRank(), qs.wasLastTrueNNSeen()) == where(10, 1, nn)
        qs.clearRefinementLimit()
        # the batched mirror describes the last token
        nn = int(g["search_ids"][len(toks) - 1, 0])
        qs.setTrueNearestId(str(nn))
        qs.searchBatch(toks)
        assert (qs.getLastTrueNNRank(), qs.wasLastTrueNNSeen()) == where(5, len(toks) - 1, nn)
        qs.clearLastMetrics()
        assert (qs.getLastTrueNNRank(), qs.wasLastTrueNNSeen()) == (-1, False)
    finally:
        if index.ctx is not None:
            index.ctx.close()
