"""GPU parity of the full select's ORDERING under crowded bins and at its size limits (route_select_kernel, phase C).

Which of the ordering paths a candidate list takes depends on the data: the all-pairs rank (nsel <= 896), the group path with
per-wave sorts, its whole-workgroup sorts for a group above a wave's slice, its redo by the general sort when such a group does
not fit the LDS region, and the general bitonic sort in LDS or in global memory.  Ids may be opaque (the caller supplies
String.hashCode): they need not spread evenly over the HashMap's bins, and a list whose ids crowd one range of bins with a few ids
per bin is legal — no tree bin, answered on the GPU.  Every scene here is built for one tier or one limit of a tier;
tests/route_order_model.py (a restatement of the kernel's path choice, fed with FspannContext.route_plan_info) PROVES the scene
reaches it before the lists are compared.  The expected lists come from the oracle alone: ids, score, count, kept and raw_seen equal
it entry for entry, no query is flagged, no bin holds more than eight ids.

Tier tallies, confirmed once on an MI355X against a scratch build of the kernel that counts, per Route call, the queries entering
each path and the groups each loop sorts: 79 calls (every scene below, with the counters, without them, and the hand-backs), the
model's prediction equal to the kernel's count in every one.  Per scene and limit: the target query's tiers -> all queries of the
call (identical with and without the counters):
  lds oversize half        limit none  q0: wave -> 8 on the group path: 821 wave groups, 18 workgroup groups, 0 redone
  lds oversize wcap-1      limit none  q0: wave -> 8 on the group path: 821 wave groups, 18 workgroup groups, 0 redone
  lds oversize wcap        limit none  q0: wave -> 8 on the group path: 821 wave groups, 18 workgroup groups, 0 redone
  lds oversize wcap+1      limit none  q0: wave+workgroup -> 8 on the group path: 820 wave groups, 19 workgroup groups, 0 redone
  lds oversize 5 wcap      limit none  q0: wave+workgroup -> 8 on the group path: 814 wave groups, 25 workgroup groups, 0 redone
  lds redo untrimmed       limit none  q1: redo+wave -> 4 on the group path: 528 wave groups, 93 workgroup groups, 1 redone
  lds room 5120            limit none  q1: wave+workgroup -> 4 on the group path: 538 wave groups, 93 workgroup groups, 0 redone
  lds room 5121            limit none  q1: redo+wave -> 4 on the group path: 527 wave groups, 93 workgroup groups, 1 redone
  lds three crowds         limit none  q0: wave+workgroup -> 8 on the group path: 802 wave groups, 29 workgroup groups, 0 redone
  lds three crowds         limit 4000  q0: wave+workgroup -> 8 on the group path: 525 wave groups, 29 workgroup groups, 0 redone
  lds limits in group      limit 2470  q0: wave -> 8 on the group path: 270 wave groups, 0 workgroup groups, 0 redone
  lds limits in group      limit 2471  q0: wave -> 8 on the group path: 271 wave groups, 0 workgroup groups, 0 redone
  lds limits in group      limit 2689  q0: wave -> 8 on the group path: 294 wave groups, 0 workgroup groups, 0 redone
  lds limits in group      limit 2876  q0: wave+workgroup -> 8 on the group path: 311 wave groups, 1 workgroup groups, 0 redone
  lds limits in group      limit 2908  q0: wave+workgroup -> 8 on the group path: 311 wave groups, 5 workgroup groups, 0 redone
  lds limits in group      limit 2909  q0: wave+workgroup -> 8 on the group path: 312 wave groups, 5 workgroup groups, 0 redone
  lds limits in group      limit 3132  q0: wave+workgroup -> 8 on the group path: 325 wave groups, 21 workgroup groups, 0 redone
  lds hard cap 4000        limit none  q0: wave+workgroup -> 8 on the group path: 839 wave groups, 2 workgroup groups, 0 redone
  lds hard cap 4000        limit 2000  q0: wave+workgroup -> 8 on the group path: 234 wave groups, 1 workgroup groups, 0 redone
  lds hard cap 3000        limit none  q0: wave+workgroup -> 8 on the group path: 640 wave groups, 1 workgroup groups, 0 redone
  lds hard cap 3000        limit 2000  q0: wave+workgroup -> 8 on the group path: 277 wave groups, 1 workgroup groups, 0 redone
  lds hand-back 1000       limit 1000  q0: wave+workgroup -> 8 on the group path: 126 wave groups, 1 workgroup groups, 0 redone
  lds hand-back 600        limit 600   q0: rank -> 8 ranked
  lds hand-back two groups limit 1000  q0: wave+workgroup -> 8 on the group path: 120 wave groups, 2 workgroup groups, 0 redone
  global oversize half     limit none  q0: wave -> 4 on the group path: 1491 wave groups, 0 workgroup groups, 0 redone
  global oversize wcap-1   limit none  q0: wave -> 4 on the group path: 1491 wave groups, 0 workgroup groups, 0 redone
  global oversize wcap     limit none  q0: wave -> 4 on the group path: 1491 wave groups, 0 workgroup groups, 0 redone
  global oversize wcap+1   limit none  q0: wave+workgroup -> 4 on the group path: 1490 wave groups, 1 workgroup groups, 0 redone
  global oversize 4 wcap   limit none  q0: wave+workgroup -> 4 on the group path: 1489 wave groups, 3 workgroup groups, 0 redone
  global g_sub             limit none  q0: wave+workgroup -> 4 on the group path: 1576 wave groups, 1 workgroup groups, 0 redone
  global redo              limit none  q0: redo+wave -> 4 on the group path: 1523 wave groups, 12 workgroup groups, 1 redone
  rank limit 895           limit none  q0: rank -> 1 ranked; 3 on the group path: 68 wave groups, 24 workgroup groups, 0 redone
  rank limit 895           limit 896   q0: rank -> 1 ranked; 3 general sort in the buffer
  rank limit 896           limit none  q0: rank -> 1 ranked; 3 on the group path: 68 wave groups, 24 workgroup groups, 0 redone
  rank limit 896           limit 896   q0: rank -> 1 ranked; 3 general sort in the buffer
  rank limit 897           limit none  q0: wave+workgroup -> 4 on the group path: 87 wave groups, 25 workgroup groups, 0 redone
  rank limit 897           limit 896   q0: bitonic_lds -> 4 general sort in the buffer
  general 17+16 bits       limit none  q0: bitonic_global -> 4 general sort in global memory
  general 17+16 bits       limit 950   q0: bitonic_lds -> 4 general sort in the buffer
  general small table      limit none  q0: bitonic_lds -> 6 general sort in the buffer
  general small table      limit 1000  q0: bitonic_global -> 6 general sort in global memory
"""
import numpy as np
import pytest

from conftest import make_scene
from route_order_model import TIERS
from route_order_scenes import crowd_levels, crowded_ids, max_bin_load, predict, trim_group, trim_list
from test_gpu_route_edges import ctx_for

pytestmark = pytest.mark.gpu

BIG = 2**31 - 1
PREDICTED = []      # (scene, limit, mode, lds_mode, target query, [tiers of every query]) of every Route call compared


def base_scene(oracle, nq, **kw):
    sc = make_scene(oracle, **kw)
    codes = sc["oracle"].encode(sc["rng"].standard_normal((nq, kw["d"])))
    return sc, codes


def planner_for(pkg, sc):
    """plan(limit, counters, mode) of this scene's configuration (the plan does not depend on the index)."""
    def plan(limit, probes, counters=True, mode=0):
        with ctx_for(pkg, sc) as ctx:
            ctx.set_route_mode(mode)
            return ctx.route_plan_info(probes, limit, counters)
    return plan


def _import(ctx, o):
    for td in range(o.TD):
        ctx.set_index(td, **o.get_index(td))
    ctx.finalize()


def _same(res, ref, lim, tag, counters):
    ids, score, count, raw = ref
    if counters:
        assert np.array_equal(res["kept"], count), tag
        assert np.array_equal(res["raw_seen"], raw), tag
    assert np.array_equal(res["count"], np.minimum(count, lim)), tag
    for i in range(len(count)):
        c = min(int(count[i]), lim)
        assert np.array_equal(res["ids"][i, :c], ids[i, :c]), (tag, i)
        assert np.array_equal(res["score"][i, :c], score[i, :c]), (tag, i)


def _brief(t):
    """The model's numbers without its per-entry arrays (for assertion messages)."""
    top = np.sort(t.info["group_sizes"])[::-1][:4].tolist() if "group_sizes" in t.info else None
    return sorted(t), {k: v for k, v in t.info.items() if np.ndim(v) == 0}, top


def _expect(tiers, q, expect, absent, tag):
    assert set(expect) <= tiers[q] and not (set(absent) & tiers[q]), (tag, _brief(tiers[q]))


def run_scene(pkg, name, sc, codes, probes, jh, deleted, cases, q=0):
    """cases = [(limit or None, tiers query q must take, tiers it must not take), ...]: one context, every limit with the counters
    requested and with counters=False under set_route_mode(1)."""
    o, n = sc["oracle"], sc["params"]["n"]
    o.set_id_meta(n, jh, deleted)
    ref = o.route(codes, probe_override=probes)
    ids, score, count, raw = ref
    assert not o.unmodelled, name
    assert not o.route_treeified(codes, probe_override=probes).any(), name
    sc["deleted"] = deleted
    with ctx_for(pkg, sc, java_hash=jh) as ctx:
        _import(ctx, o)
        for limit, expect, absent in cases:
            lim = limit or BIG
            plan = ctx.route_plan_info(probes, lim, True)
            assert max_bin_load(jh, ids, count, plan["cap0"]).max() <= 8, name
            tiers = [predict(plan, jh, ids, score, count, i, lim) for i in range(len(count))]
            _expect(tiers, q, expect, absent, (name, limit))
            PREDICTED.append((name, lim, "counters", plan["lds_mode"], q, tiers))
            _same(ctx.route(codes, probe_override=probes, limit=lim), ref, lim, (name, limit, "counters"), True)
            ctx.set_route_mode(1)
            plan1 = ctx.route_plan_info(probes, lim, False)
            assert not plan1["lazy"] and {k: v for k, v in plan1.items() if k != "lazy_cap"} == {k: v for k, v in plan.items() if k != "lazy_cap"}
            PREDICTED.append((name, lim, "no counters", plan["lds_mode"], q, tiers))
            _same(ctx.route(codes, probe_override=probes, limit=lim, counters=False), ref, lim, (name, limit, "no counters"), False)
            ctx.set_route_mode(0)
        assert ctx.unmodelled_queries() == 0, name
    return ref


def run_hand_back(pkg, monkeypatch, name, sc, codes, probes, jh, deleted, limit, expect, absent=(), q=0, check=None):
    """The same lists through the bounded select's hand-back: set_route_mode(2), no counters, and an entry budget small enough that
    every query overflows and is redone by the full select."""
    o, n = sc["oracle"], sc["params"]["n"]
    o.set_id_meta(n, jh, deleted)
    ref = o.route(codes, probe_override=probes)
    ids, score, count, raw = ref
    assert not o.unmodelled and not o.route_treeified(codes, probe_override=probes).any(), name
    sc["deleted"] = deleted
    monkeypatch.setenv("FSPANN_ROUTE_LAZY_CAP", "64")
    with ctx_for(pkg, sc, java_hash=jh) as ctx:
        _import(ctx, o)
        ctx.set_route_mode(2)
        plan = ctx.route_plan_info(probes, limit, False)
        assert plan["lazy"] and plan["lazy_cap"] == 64, plan
        tiers = [predict(plan, jh, ids, score, count, i, limit) for i in range(len(count))]
        _expect(tiers, q, expect, absent, (name, limit, "hand-back"))
        assert check is None or check(tiers[q].info), (name, _brief(tiers[q]))
        res = ctx.route(codes, probe_override=probes, limit=limit, counters=False)
        info = ctx.last_route_info()
        assert info["lazy"] and info["overflowed"] == len(count), info
        PREDICTED.append((name, limit, "hand-back", plan["lds_mode"], q, tiers))
        _same(res, ref, limit, (name, limit, "hand-back"), False)
        assert ctx.unmodelled_queries() == 0, name
    monkeypatch.delenv("FSPANN_ROUTE_LAZY_CAP")


# ---- LDS mode: 8 tables x 10 probes x 64 = 5 120 tuple slots, an 8 192-word hash table whose space the group path reuses -----------

LDS_KW = dict(n=20000, d=16, T=8, D=1, m=12, lam=2, B=4000, seed=51)      # the scene of test_long_lists_sorted_in_lds_and_global


@pytest.mark.parametrize("aim", ["half", "wcap-1", "wcap", "wcap+1", "5 wcap"])
def test_oversize_group_in_lds_mode(pkg, oracle, aim):
    """Query 0's most populated level (~660 ids) crowded into 2 048 bins, one id per bin: ONE group of the ordering.  Trimmed with
    deleted flags (deleted ids INSIDE the crowd, never put: PIS:739) to a wave's slice minus one, the slice, the slice plus one —
    the first size the whole workgroup sorts — and five slices."""
    sc, codes = base_scene(oracle, 8, **LDS_KW)
    plan = planner_for(pkg, sc)(BIG, 10)
    jh = crowd_levels(oracle, sc, codes, 10, 0, [(-1, 0, 4000, 0, 2048)])
    target = {"half": lambda i: i["wcap"] // 2, "wcap-1": lambda i: i["wcap"] - 1, "wcap": lambda i: i["wcap"],
              "wcap+1": lambda i: i["wcap"] + 1, "5 wcap": lambda i: 5 * i["wcap"]}[aim]
    deleted, t, c = trim_group(sc, codes, 10, 0, plan, BIG, jh, target, crowded_ids(oracle, jh))
    big = aim in ("wcap+1", "5 wcap")
    assert c == target(t.info) and (c == t.info["group_sizes"].max() or aim == "half") and t.info["wcap"] == 128 and deleted.sum() > 0
    # (the OTHER queries keep whatever their lists hold; only query 0 is aimed)
    run_scene(pkg, "lds oversize " + aim, sc, codes, 10, jh, deleted, [(None, {"workgroup"} if big else {"wave"}, () if big else {"workgroup", "redo"})])


def test_padded_group_at_the_room_limit_and_redo_in_lds_mode(pkg, oracle):
    """10 tables x 10 probes = 6 400 slots over the same 8 192-word region: a list of 5 120 entries leaves room for 2 048 words in
    front of the sub-keys.  A level of > 1 024 ids crowded into one group pads to 2 048: it fits at nsel = 5 120 (sorted by the
    workgroup) and no longer at 5 121 (room 2 044: too_big, the whole list is redone by the general sort) — the list trimmed to
    both lengths with deleted flags OUTSIDE the group.  Then untrimmed (~5 500 entries): redo."""
    sc, codes = base_scene(oracle, 4, n=30000, d=16, T=10, D=1, m=12, lam=2, B=6000, seed=151)
    plan = planner_for(pkg, sc)(BIG, 10)
    jh = crowd_levels(oracle, sc, codes, 10, 1, [(-1, 0, 1800, 0, 1024)])          # query 1: 1 800 ids of a level of ~2 600, two per bin
    o, n = sc["oracle"], sc["params"]["n"]
    ids, score, count, _ = o.route(codes, probe_override=10)
    t = predict(plan, jh, ids, score, count, 1, BIG)
    g = int(np.argmax(t.info["group_sizes"]))
    assert 1024 < t.info["group_sizes"][g] <= 2048 and t.info["nsel"] > 5121, _brief(t)
    run_scene(pkg, "lds redo untrimmed", sc, codes, 10, jh, None, [(None, {"redo"}, ())], q=1)
    members = ids[1, :count[1]][t.info["selected"]][t.info["group_of_selected"] == g]
    for want, tier, room in ((5120, "workgroup", 2048), (5121, "redo", 2044)):
        deleted = trim_list(sc, codes, 10, 1, jh, want, avoid=members)
        ids2, score2, count2, _ = o.route(codes, probe_override=10)
        t2 = predict(plan, jh, ids2, score2, count2, 1, BIG)
        assert t2.info["nsel"] == want and t2.info["room"] == room and t2.info["group_sizes"].max() == t.info["group_sizes"][g], _brief(t2)
        run_scene(pkg, "lds room %d" % want, sc, codes, 10, jh, deleted, [(None, {tier}, {"redo"} if tier != "redo" else ())], q=1)


def test_several_crowded_groups_on_different_levels(pkg, oracle):
    """Three levels of query 0 crowded: two groups above a wave's slice (the workgroup loop runs twice: its cursors are checked across
    groups) and one below it."""
    sc, codes = base_scene(oracle, 8, **LDS_KW)
    plan = planner_for(pkg, sc)(BIG, 10)
    jh = crowd_levels(oracle, sc, codes, 10, 0, [(-1, 0, 4000, 0, 1024), (-2, 0, 4000, 0, 1024), (-3, 0, 100, 0, 1024)])
    ids, score, count, _ = sc["oracle"].route(codes, probe_override=10)
    t = predict(plan, jh, ids, score, count, 0, BIG)
    top = np.sort(t.info["group_sizes"])[::-1]
    assert top[0] > 4 * t.info["wcap"] and top[1] > 4 * t.info["wcap"] and t.info["wcap"] // 2 < top[2] <= t.info["wcap"], (top[:4], t.info["wcap"])
    run_scene(pkg, "lds three crowds", sc, codes, 10, jh, None, [(None, {"wave", "workgroup"}, {"redo"}), (4000, {"wave", "workgroup"}, {"redo"})])


def test_limit_inside_and_in_front_of_a_crowded_group(pkg, oracle):
    """A level crowded into TWO groups — 450 ids in the low bins, the rest (~210) in the upper half of the table — and limits in front
    of the first group, at its first entry, its middle, near its end, its last entry and one past it.  With more than 256 ties behind
    the limit the select cuts the level by bins before it orders (a shorter group); with at most 256 the whole level is selected, the
    sorted group is cut by `rank < nout`, and the second group — also above a wave's slice — lies behind the limit: the `g0 >= nout`
    break of the workgroup loop."""
    sc, codes = base_scene(oracle, 8, **LDS_KW)
    jh = crowd_levels(oracle, sc, codes, 10, 0, [(-1, 0, 450, 0, 1024), (-1, 450, 4000, 16384, 1024)])
    ids, score, count, _ = sc["oracle"].route(codes, probe_override=10)
    s0 = score[0, :count[0]]
    lvl = int(np.argmax(np.bincount(s0)))
    g0 = int((s0 < lvl).sum())
    t = predict(planner_for(pkg, sc)(BIG, 10), jh, ids, score, count, 0, BIG)
    top = np.sort(t.info["group_sizes"])[::-1]
    a, b = int(top[0]), int(top[1])
    assert g0 > 896 and a > 3 * t.info["wcap"] and t.info["wcap"] < b and (s0 == lvl).sum() - a <= 256, (g0, a, b)   # (<= 256 behind the limit: no cut by bins)
    level = int((s0 == lvl).sum())
    cases = [(g0, {"wave"}, {"workgroup", "redo"}),              # in front of the group: nothing of the level is selected
             (g0 + 1, {"wave"}, {"workgroup", "redo"}),          # its first entry: > 256 ties behind the limit, the level is cut by bins first
             (g0 + a // 2, {"wave"}, {"redo"}),                  # its middle: likewise, what is left of the group fits a wave
             (g0 + level - 256, {"workgroup"}, {"redo"}),        # inside it, 256 ties behind the limit: the whole level is selected, rank < nout
             (g0 + a, {"workgroup"}, {"redo"}),                  #   cuts inside the sorted group and the second group lies behind nout
             (g0 + a + 1, {"workgroup"}, {"redo"}),              # its last entry, and one past it
             (g0 + level, {"workgroup"}, {"redo"})]
    assert g0 + level - 256 < g0 + a
    run_scene(pkg, "lds limits in group", sc, codes, 10, jh, None, cases)


@pytest.mark.parametrize("hard_cap", [4000, 3000])
def test_crowd_across_a_hard_cap_cut_and_a_resizing_map(pkg, oracle, hard_cap):
    """HARD_CAP 4 000: bestScore = new HashMap(4 000) starts at 4 096 bins and resizes to 8 192 on its 3 073rd id (as SIFT_P10_HIGH's
    28 000 does at 32 768), and the traversal stops at the 4 000th id with crowded ids on both sides of the cut: the groups are cut
    from the bins at the FINAL table length.  HARD_CAP 3 000: the cut without the resize."""
    sc, codes = base_scene(oracle, 8, **dict(LDS_KW, hard_cap=hard_cap, B=hard_cap))
    plan = planner_for(pkg, sc)(BIG, 10)
    uncut, _ = base_scene(oracle, 8, **LDS_KW)            # the same data and g-functions without the cut: the crowd is taken from ITS list
    assert np.array_equal(uncut["X"], sc["X"]) and np.array_equal(uncut["alpha"], sc["alpha"])
    # (the cut takes ids off the levels 1, 2 and 6 at HARD_CAP 4 000, off the levels 0 - 6 at 3 000)
    jh = crowd_levels(oracle, sc, codes, 10, 0, [(2, 0, 4000, 0, 1024) if hard_cap == 4000 else (-1, 0, 4000, 0, 512)], list_from=uncut)
    ids, score, count, _ = sc["oracle"].route(codes, probe_override=10)
    t = predict(plan, jh, ids, score, count, 0, BIG)
    assert t.info["capf"] == (8192 if hard_cap == 4000 else 4096) and hard_cap <= count[0] < hard_cap + 64 and plan["cap0"] == 4096
    assert t.info["group_sizes"].max() > t.info["wcap"] + 64, _brief(t)
    crowd = crowded_ids(oracle, jh)
    kept = int(np.isin(crowd, ids[0, :count[0]]).sum())
    assert t.info["wcap"] < kept < len(crowd) - 50, (kept, len(crowd))           # crowded ids in the list AND (> 50) behind the cut
    run_scene(pkg, "lds hard cap %d" % hard_cap, sc, codes, 10, jh, None, [(None, {"workgroup"}, {"redo"}), (2000, {"workgroup"}, {"redo"})])


def test_crowded_lists_through_the_bounded_selects_hand_back(pkg, oracle, monkeypatch):
    """limit 1 000 (<= 1 024: the bounded select is legal; > 896: the full select that redoes a handed-back query has its sub-key
    buffer) with a crowded group of ~400 inside the first 1 000 entries; limit 600: a handed-back list of <= 896 entries is ranked;
    limit 1 000 again with two crowded groups above a wave's slice in front of the limit."""
    sc, codes = base_scene(oracle, 8, **LDS_KW)
    ids, score, count, _ = sc["oracle"].route(codes, probe_override=10)
    hist = np.bincount(score[0, :count[0]])
    lvl = int(np.flatnonzero(np.cumsum(hist) - hist < 500)[-1])       # the level that starts in front of entry 500
    jh = crowd_levels(oracle, sc, codes, 10, 0, [(lvl, 0, 4000, 0, 1024)])
    run_hand_back(pkg, monkeypatch, "lds hand-back 1000", sc, codes, 10, jh, None, 1000, {"workgroup"}, {"redo"})
    run_hand_back(pkg, monkeypatch, "lds hand-back 600", sc, codes, 10, jh, None, 600, {"rank"})
    # two levels crowded, both inside the first 1 000 entries: the workgroup loop runs more than once on a handed-back list
    jh = crowd_levels(oracle, sc, codes, 10, 0, [(lvl, 0, 4000, 0, 1024), (lvl + 1, 0, 4000, 0, 1024)])
    run_hand_back(pkg, monkeypatch, "lds hand-back two groups", sc, codes, 10, jh, None, 1000, {"workgroup"}, {"redo"},
                  check=lambda i: i["workgroup_groups"] >= 2 and not i["lvl1"])


# ---- global-arena mode: 10 x 4 tables x 20 probes x 64 = 51 200 tuple slots (the shape of test_global_arena_path) ------------------

GLOBAL_KW = dict(n=20000, d=16, T=10, D=4, m=12, lam=2, B=512, hard_cap=60000, seed=41)


@pytest.mark.parametrize("aim", ["half", "wcap-1", "wcap", "wcap+1", "4 wcap"])
def test_oversize_group_in_global_arena_mode(pkg, oracle, aim):
    """Lists of ~13 000 - 17 000 entries whose sub-keys fit the LDS region behind the wave slices (sub_lds): the most populated level
    of query 0 crowded into 2 048 bins, the group trimmed to half a wave's slice, the slice minus one, the slice, one more, and four
    slices (the slice, the room and where the sub-keys lie come from lds_sort_words here, not from the hash table's size)."""
    sc, codes = base_scene(oracle, 4, **GLOBAL_KW)
    plan = planner_for(pkg, sc)(BIG, 20)
    assert not plan["lds_mode"] and plan["g_sub"]
    jh = crowd_levels(oracle, sc, codes, 20, 0, [(-1, 0, 4600, 0, 2048)])
    target = {"half": lambda i: i["wcap"] // 2, "wcap-1": lambda i: i["wcap"] - 1, "wcap": lambda i: i["wcap"],
              "wcap+1": lambda i: i["wcap"] + 1, "4 wcap": lambda i: 4 * i["wcap"]}[aim]
    deleted, t, c = trim_group(sc, codes, 20, 0, plan, BIG, jh, target, crowded_ids(oracle, jh))
    big = aim in ("wcap+1", "4 wcap")
    assert t.info["sub_lds"] and c == target(t.info) == t.info["group_sizes"].max() and t.info["wcap"] == 1024, _brief(t)
    run_scene(pkg, "global oversize " + aim, sc, codes, 20, jh, deleted,
              [(None, {"workgroup"} if big else {"wave"}, {"redo"} if big else {"workgroup", "redo"})])


def test_oversize_group_with_the_sub_keys_in_global_memory(pkg, oracle, monkeypatch):
    """The sub-keys stay in global memory (g_sub) when the list does not fit the LDS region behind the wave slices.  At this shape the
    region holds 34 720 words, more than a scene of this size can fill, so the development switch FSPANN_ROUTE_LDS_KB = 92 plans
    with a 17 312-word region ("ordering paths"): lists of ~21 000 entries, a crowded group of ~2 000 sorted by the
    workgroup straight from global memory, and wave groups read from there."""
    monkeypatch.setenv("FSPANN_ROUTE_LDS_KB", "92")
    sc, codes = base_scene(oracle, 4, **dict(GLOBAL_KW, n=30000, seed=141))
    plan = planner_for(pkg, sc)(BIG, 20)
    assert not plan["lds_mode"] and plan["g_sub"] and 16384 <= plan["lds_sort_words"] < 20000, plan
    jh = crowd_levels(oracle, sc, codes, 20, 0, [(-1, 0, 2000, 0, 2048)])
    ids, score, count, _ = sc["oracle"].route(codes, probe_override=20)
    t = predict(plan, jh, ids, score, count, 0, BIG)
    assert not t.info["sub_lds"] and t.info["group_sizes"].max() > 2 * t.info["wcap"], _brief(t)
    run_scene(pkg, "global g_sub", sc, codes, 20, jh, None, [(None, {"wave", "workgroup"}, {"redo"})])


def test_redo_in_global_arena_mode(pkg, oracle, monkeypatch):
    """too_big in global-arena mode: a padded group larger than what the region leaves in front of the sub-keys.  With the whole LDS
    to plan with that takes a group of > 8 192 entries ("ordering paths"); with FSPANN_ROUTE_LDS_KB = 92 the region is
    17 312 words, a list of ~13 000 entries leaves room for ~3 000, and a level of > 2 048 crowded into one group is redone."""
    monkeypatch.setenv("FSPANN_ROUTE_LDS_KB", "92")
    sc, codes = base_scene(oracle, 4, **dict(GLOBAL_KW, n=30000, seed=141))
    plan = planner_for(pkg, sc)(BIG, 20)
    jh = crowd_levels(oracle, sc, codes, 20, 0, [(-1, 0, 6000, 0, 2048)])
    ids, score, count, _ = sc["oracle"].route(codes, probe_override=20)
    t = predict(plan, jh, ids, score, count, 0, BIG)
    g = int(np.argmax(t.info["group_sizes"]))
    members = ids[0, :count[0]][t.info["selected"]][t.info["group_of_selected"] == g]
    deleted = trim_list(sc, codes, 20, 0, jh, 13000, avoid=members)
    ids, score, count, _ = sc["oracle"].route(codes, probe_override=20)
    t = predict(plan, jh, ids, score, count, 0, BIG)
    assert t.info["sub_lds"] and t.info["group_sizes"].max() > 2048 and t.info["room"] < 4096, _brief(t)
    run_scene(pkg, "global redo", sc, codes, 20, jh, deleted, [(None, {"redo"}, ())])


# ---- the rank path's limit ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("live", [895, 896, 897])
def test_rank_path_limit(pkg, oracle, live):
    """Query 0 trimmed with deleted flags to exactly 895 / 896 / 897 live distinct ids: the last two lengths of the all-pairs rank and
    the first of the group path.  limit 896 plans 512 threads, no limit 1 024 threads (897 entries under limit 896: the general sort,
    no sub-key buffer is planned for a limit that short)."""
    sc, codes = base_scene(oracle, 4, n=6000, d=16, T=6, D=1, m=10, lam=2, B=2000, seed=181)
    jh = oracle.decimal_hashes(6000)
    deleted = trim_list(sc, codes, 5, 0, jh, live)
    p512, p1024 = planner_for(pkg, sc)(896, 5), planner_for(pkg, sc)(BIG, 5)
    assert p512["threads"] == 512 and p1024["threads"] == 1024 and p512["sort_cap"] >= 1024
    first, second = ({"rank"}, {"rank"}) if live <= 896 else ({"wave"}, {"bitonic_lds"})
    run_scene(pkg, "rank limit %d" % live, sc, codes, 5, jh, deleted, [(None, first, set(TIERS) - first - {"workgroup"}), (896, second, set(TIERS) - second)])


# ---- the general sort under default knobs ---------------------------------------------------------------------------------------------

def test_general_sort_when_bin_and_tuple_number_exceed_32_bits(pkg, oracle):
    """13 x 4 tables x 20 probes x 64 = 66 560 tuple slots (17 bits) and HARD_CAP 70 000 (bestScore starts at 65 536 bins: 16 bits): the
    32-bit sub-key cannot hold both, the list is sorted by the general bitonic sort — ~18 000 entries in global memory, and the
    ~950 of limit 950 in the sort buffer."""
    sc, codes = base_scene(oracle, 4, n=20000, d=16, T=13, D=4, m=12, lam=2, B=512, hard_cap=70000, seed=171)
    plan = planner_for(pkg, sc)(BIG, 20)
    assert plan["seq_bits"] == 17 and plan["cap0"] == 65536 and plan["g_sub"]
    jh = crowd_levels(oracle, sc, codes, 20, 0, [(-1, 0, 4000, 0, 2048)])
    run_scene(pkg, "general 17+16 bits", sc, codes, 20, jh, None, [(None, {"bitonic_global"}, set(TIERS) - {"bitonic_global"}),
                                                                  (950, {"bitonic_lds"}, set(TIERS) - {"bitonic_lds"})])


def test_general_sort_when_the_hash_table_is_too_small_for_groups(pkg, oracle):
    """5 tables x 5 probes x 64 = 1 600 tuple slots: a 2 048-slot hash table, less than the 4 096 words the group path needs.  Lists of
    ~1 400: sorted in the sort buffer when it was planned for them (no limit), in global memory under limit 1 000 (a 1 024-entry
    buffer and ~1 050 selected)."""
    sc, codes = base_scene(oracle, 6, n=6000, d=16, T=5, D=1, m=10, lam=2, B=2000, seed=172)
    plan = planner_for(pkg, sc)(BIG, 5)
    assert plan["ht_size"] == 2048 and plan["lds_mode"] and plan["g_sub"]
    jh = crowd_levels(oracle, sc, codes, 5, 0, [(-1, 0, 4000, 0, 512)])
    run_scene(pkg, "general small table", sc, codes, 5, jh, None, [(None, {"bitonic_lds"}, set(TIERS) - {"bitonic_lds"}),
                                                                   (1000, {"bitonic_global"}, set(TIERS) - {"bitonic_global"})])


def test_zz_every_ordering_tier_was_exercised():
    """Over the module: every tier predicted for at least two DIFFERENT (scene, limit, query) lists — the same list run with and
    without the counters counts once; the workgroup sorts and the redo at least once in LDS mode and once in global-arena mode."""
    lists = {t: set() for t in TIERS}
    by_mode = set()
    for name, lim, mode, lds_mode, q, tiers in PREDICTED:
        for i, t in enumerate(tiers):
            for k in t:
                lists[k].add((name, lim, i))
        for k in tiers[q]:
            by_mode.add((k, bool(lds_mode)))
    seen = {k: len(v) for k, v in lists.items()}
    assert all(v >= 2 for v in seen.values()), seen
    for k in ("workgroup", "redo"):
        assert (k, True) in by_mode and (k, False) in by_mode, sorted(by_mode)
