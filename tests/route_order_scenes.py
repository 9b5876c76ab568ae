"""Scene recipes for tests/test_gpu_route_order_tiers.py: opaque ids whose hashCodes crowd one range of HashMap bins (at most a few
per bin: no bin treeifies), built and aimed on the oracle alone — no GPU needed to construct one.

The recipe: route once with decimal hashCodes, take ids of one query's score levels, give them hashCodes whose bins fall round-robin
into a range of R bins, rebuild the oracle's index (the staging map's order depends on the hashCodes) and route again.  A group is
then brought to an exact size with `deleted` flags (a deleted id is never put, PIS:739; the index does not depend on them)."""
import numpy as np

from route_order_model import bins_at_final_cap, order_tiers


def spread_inv(s):
    """String.hashCode values whose HashMap.hash() spread is `s` (h ^ h >>> 16 is an involution)."""
    s = np.asarray(s).astype(np.uint32)
    return (s ^ (s >> 16)).view(np.int32)


def crowd_levels(O, sc, codes, probes, q, picks, deleted=None, list_from=None):
    """picks = [(level, start, k, first_bin, R), ...]: the ids [start, start + k) of one score level of query q's list (level >= 0: that
    score; -1, -2, ...: the most, second most, ... populated level) get DIFFERENT hashCodes whose bins are first_bin + (i mod R) at
    every table length up to 2^20.  Rebuilds the oracle's index (with decimal hashCodes first, to read the list).  Returns jh.
    list_from: a scene over the same data whose list the ids are taken from (one without the HARD_CAP cut, so that crowded ids end up
    on both sides of the cut of `sc`)."""
    o, n = sc["oracle"], sc["params"]["n"]
    src = (list_from or sc)["oracle"]
    src.set_id_meta(n, None, deleted)
    src.build_index(sc["X64"])
    ids, score, count, _ = src.route(codes, probe_override=probes)
    l, s = ids[q, :count[q]], score[q, :count[q]]
    by_size = np.argsort(-np.bincount(s), kind="stable")
    jh = O.decimal_hashes(n).copy()
    for level, start, k, b0, R in picks:
        cand = l[s == (level if level >= 0 else by_size[-level - 1])][start:start + k]
        i = np.arange(len(cand), dtype=np.int64)
        jh[cand] = spread_inv(b0 + i % R + (1 << 20) * (1 + i // R))
    o.set_id_meta(n, jh, deleted)
    o.build_index(sc["X64"])
    return jh


def max_bin_load(jh, lists, counts, cap0):
    """Per query: the largest number of (distinct, live) ids sharing one bin of the cap0 table (bins only split as the table grows)."""
    h = np.asarray(jh).view(np.uint32)
    sp = (h ^ (h >> 16)) & np.uint32(cap0 - 1)
    return np.array([np.unique(sp[l[:c]], return_counts=True)[1].max() if c else 0 for l, c in zip(lists, counts)])


def predict(plan, jh, ids, score, count, q, limit):
    """order_tiers for query q of an oracle result (the full list: every kept id)."""
    l = ids[q, :count[q]]
    return order_tiers(plan, score[q, :count[q]], bins_at_final_cap(jh, l, plan["cap0"]), limit)


def crowded_ids(O, jh):
    """The ids whose hashCode is not the decimal one: what crowd_levels moved."""
    return np.flatnonzero(np.asarray(jh) != O.decimal_hashes(len(jh)))


def trim_group(sc, codes, probes, q, plan, limit, jh, target, crowd, deleted=None, tries=6):
    """Flags ids of query q's crowded group (the group most of the ids `crowd` fall into) deleted — evenly over the group — until it
    holds exactly target(info) entries (target: an int or a function of the model's info: wcap and room move with the list's
    length).  Returns (deleted, tiers, the group's size)."""
    o, n = sc["oracle"], sc["params"]["n"]
    deleted = np.zeros(n, np.uint8) if deleted is None else deleted.copy()
    for _ in range(tries):
        o.set_id_meta(n, jh, deleted)
        ids, score, count, _ = o.route(codes, probe_override=probes)
        t = predict(plan, jh, ids, score, count, q, limit)
        sel_ids, grp = ids[q, :count[q]][t.info["selected"]], t.info["group_of_selected"]
        g = int(np.bincount(grp[np.isin(sel_ids, crowd)]).argmax())
        want = target(t.info) if callable(target) else target
        c = int(t.info["group_sizes"][g])
        if c == want:
            return deleted, t, c
        assert c > want, "the group holds %d entries, fewer than the %d aimed at: crowd more ids" % (c, want)
        members = sel_ids[grp == g]
        deleted[members[np.linspace(0, c - 1, c - want).astype(int)]] = 1
    raise AssertionError("the group did not settle at the size aimed at")


def trim_list(sc, codes, probes, q, jh, target, deleted=None, avoid=()):
    """Flags ids of query q's list deleted until it keeps exactly `target` live distinct ids (taken evenly over the list, none of
    `avoid`)."""
    o, n = sc["oracle"], sc["params"]["n"]
    deleted = np.zeros(n, np.uint8) if deleted is None else deleted.copy()
    for _ in range(6):                    # (behind a HARD_CAP cut a deleted id lets another one in: look again)
        o.set_id_meta(n, jh, deleted)
        ids, _, count, _ = o.route(codes, probe_override=probes)
        c = int(count[q])
        if c == target:
            return deleted
        assert c > target, (c, target)
        free = ids[q, :c][~np.isin(ids[q, :c], avoid)]
        deleted[free[np.linspace(0, len(free) - 1, c - target).astype(int)]] = 1
    raise AssertionError("the list did not settle at the length aimed at")
