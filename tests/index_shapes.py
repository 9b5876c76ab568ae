"""Index shapes the oracle's own build never produces: GreedyPartitioner's cut restated at any block size, and partitions
the reference would not cut but fspann_set_index accepts.  TEST INFRASTRUCTURE ONLY: no product code in it.

The order of ids in a table does not depend on the block size (GreedyPartitioner sorts first and cuts after,
GreedyPartitioner.java:37-76), so the oracle's build at its constant block size of 64 gives the order and a few lines of
numpy restate the cut (GreedyPartitioner.java:55-70, as oracle/fspann_oracle.cpp:greedyBuild restates it).  The oracle's
set_index / routeTraverse / findNearestPartition walk whatever partitions they are given, so a second oracle that imports
the re-cut tables is the reference for every shape.  tests/test_index_shapes_cpu.py pins this helper to the oracle at 64
before any GPU test relies on it.
"""
import numpy as np

_REV8 = np.array([int("{:08b}".format(i)[::-1], 2) for i in range(256)], dtype=np.uint8)
ARRAYS = ("min_key", "max_key", "rep", "id_off", "ids")


def keys_of(words0):
    """GreedyPartitioner.computeKey of first code words: code bit b -> key bit 62 - b (b < 63); bit 63 is not in the key."""
    w = np.ascontiguousarray(words0, dtype="<u8")
    by = _REV8[w.view(np.uint8).reshape(w.shape + (8,))][..., ::-1]      # bits reversed in every byte, bytes reversed
    return (np.ascontiguousarray(by).view("<u8").reshape(w.shape) >> np.uint64(1)).astype(np.int64)


def cut(ids, codes_td, sizes):
    """The five arrays of one table: `ids` (sorted order) cut into partitions of `sizes` ids; codes_td [n][W] by handle."""
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    sizes = np.asarray(sizes, dtype=np.int64)
    assert (sizes >= 0).all() and sizes.sum() == len(ids), (sizes.sum(), len(ids))
    W = codes_td.shape[1]
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    keys = keys_of(codes_td[ids, 0]) if len(ids) else np.zeros(0, np.int64)
    mn = np.zeros(len(sizes), np.int64)
    mx = np.zeros(len(sizes), np.int64)
    rep = np.zeros((len(sizes), W), np.uint64)
    full = np.flatnonzero(sizes > 0)
    a, b = off[full], off[full + 1]
    mn[full] = keys[a]
    mx[full] = keys[b - 1]
    rep[full] = codes_td[ids[a + ((b - a - 1) >> 1)]]
    # an empty partition repeats its predecessor's maxKey (as both keys) and rep; in front of the first: key 0, code 0
    prev_key, prev_rep = 0, np.zeros(W, np.uint64)
    for p in range(len(sizes)):
        if sizes[p] == 0:
            mn[p] = mx[p] = prev_key
            rep[p] = prev_rep
        else:
            prev_key, prev_rep = mx[p], rep[p]
    return dict(min_key=mn, max_key=mx, rep=rep, id_off=off, ids=ids.copy())


def recut(o, codes_by_handle, td, sizes):
    """Table td of oracle `o` (built at its block size of 64) cut again by `sizes`; codes_by_handle [n][TD][W] = o.encode(X)."""
    return cut(o.get_index(td)["ids"], codes_by_handle[:, td], sizes)


def uniform(n, S):
    """GreedyPartitioner's sizes: blocks of S and one short tail."""
    return [S] * (n // S) + ([n % S] if n % S else [])


def ragged(n, S, rng):
    """Sizes in [0, S] summing to n: a leading empty partition, a run of three empties in the middle, two trailing
    empties, and partitions of 1, S/2, S - 1 and S ids in the middle (others random, a fifth of them empty)."""
    forced = [1, S // 2, 0, 0, 0, S - 1, S]
    left = n - sum(forced)
    assert left >= 4 * S, "ragged needs room for its promised shapes"
    body = []
    while left > 0:
        u = rng.random()
        s = 0 if u < 0.2 else (S if u < 0.45 else int(rng.integers(1, S + 1)))
        s = min(s, left)
        body.append(s)
        left -= s
    h = len(body) // 2
    assert sum(body[:h]) > 0 and sum(body[h:]) > 0
    return [0] + body[:h] + forced + body[h:] + [0, 0]


def second_oracle(sc, tables, java_hash=None, deleted=None, hard_cap=None, store=True):
    """A fresh Oracle with the scene's G functions, id metadata and store that IMPORTS `tables` (one dict per td)."""
    p = sc["params"]
    o2 = type(sc["oracle"])(p["T"], p["D"], p["m"], p["lam"], p["d"], max_global_candidates=p["hard_cap"] if hard_cap is None else hard_cap,
                  refinement_limit=p["B"], probe_override=p["probe_override"], hamming_threshold=p["tau"])
    o2.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
    o2.set_id_meta(p["n"], java_hash, sc["deleted"] if deleted is None else deleted)
    if store:
        o2.set_store(sc["X64"])
    assert len(tables) == o2.TD
    for td, ix in enumerate(tables):
        o2.set_index(td, **ix)
    return o2


def subset(ix, keep_mask, codes_td, S):
    """Table `ix` without the ids whose keep_mask[id] is False, cut again in blocks of S (the order of the rest stays)."""
    ids = ix["ids"][np.asarray(keep_mask, bool)[ix["ids"]]]
    return cut(ids, codes_td, uniform(len(ids), S))


def shuffled(ix, rng):
    """The same partitions, each with its ids, in a random order: key ranges no longer ascend."""
    npart = len(ix["min_key"])
    perm = rng.permutation(npart)
    sizes = np.diff(ix["id_off"])[perm]
    off = np.zeros(npart + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    ids = np.concatenate([ix["ids"][ix["id_off"][p]:ix["id_off"][p + 1]] for p in perm]) if npart else ix["ids"].copy()
    return dict(min_key=ix["min_key"][perm].copy(), max_key=ix["max_key"][perm].copy(), rep=ix["rep"][perm].copy(), id_off=off,
                ids=np.ascontiguousarray(ids, dtype=np.int32))


def empty_table(W):
    """A table with no partitions (the reference skips it, PIS:638)."""
    return dict(min_key=np.zeros(0, np.int64), max_key=np.zeros(0, np.int64), rep=np.zeros((0, W), np.uint64),
                id_off=np.zeros(1, np.int64), ids=np.zeros(0, np.int32))


def same_tables(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in ARRAYS)


def ascends(ix):
    """The condition under which findNearestPartition's binary search is a search (what GreedyPartitioner produces)."""
    mn, mx = ix["min_key"], ix["max_key"]
    return bool((mn >= 0).all() and (mn <= mx).all() and (np.diff(mn) >= 0).all() and (np.diff(mx) >= 0).all())


def make_ctx(pkg, sc, block_size=64, java_hash=None, deleted=None, hard_cap=None):
    """A product context for the scene: G functions and id metadata set, no index yet."""
    p = sc["params"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 max_global_candidates=p["hard_cap"] if hard_cap is None else hard_cap,
                                 probe_override=p["probe_override"], hamming_prefilter_threshold=p["tau"], block_size=block_size)
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
    ctx.set_id_meta(p["n"], java_hash, sc["deleted"] if deleted is None else deleted)
    return ctx


def import_tables(ctx, tables):
    for td, ix in enumerate(tables):
        ctx.set_index(td, **ix)
    ctx.finalize()


def compare_selects(ctx, o2, codes, probes=-1, limits=(None,), bounded=(), must_be_bounded=False, allow_handback=False):
    """Route of `ctx` against o2.route, entry by entry.  limits: the full select with counters (None = unlimited); bounded:
    route mode 2 without counters at these limits — whichever select the plan names must be the one that ran, and with
    must_be_bounded it must be the bounded one, with no query handed back unless allow_handback.  Returns the oracle's
    (count, raw) and the last_route_info() of every bounded attempt."""
    ids, score, count, raw = o2.route(codes, probe_override=probes)
    assert not o2.unmodelled, "oracle HashMap order not pinned for this scene"
    assert not o2.route_treeified(codes, probe_override=probes).any(), "a bin of bestScore treeified: order not modelled"
    nq = len(count)

    def same(res, lim, what):
        for i in range(nq):
            n = int(count[i]) if not lim else min(lim, int(count[i]))
            assert res["count"][i] == n, (what, lim, i, int(res["count"][i]), n)
            assert np.array_equal(res["ids"][i, :n], ids[i, :n]), (what, lim, i)
            assert np.array_equal(res["score"][i, :n], score[i, :n]), (what, lim, i)

    for lim in limits:
        res = ctx.route(codes, probe_override=probes, limit=lim if lim else 2**31 - 1)
        assert np.array_equal(res["kept"], count), ("kept", lim)
        assert np.array_equal(res["raw_seen"], raw), ("raw_seen", lim)
        same(res, lim, "full")
    infos = []
    for lim in bounded:
        ctx.set_route_mode(2)
        try:
            planned = bool(ctx.route_plan_info(probes, lim, False)["lazy"])
            res = ctx.route(codes, probe_override=probes, limit=lim, counters=False)
            info = ctx.last_route_info()
        finally:
            ctx.set_route_mode(0)
        assert info["lazy"] == planned, (lim, info, planned)
        if must_be_bounded:
            assert planned, ("bounded select not planned", lim)
            if not allow_handback:
                assert info["overflowed"] == 0, (lim, info)
        same(res, lim, "bounded")
        infos.append(info)
    return count, raw, infos


# ---- scenes shared by tests/test_index_shapes_cpu.py (which asserts what they claim) and the two GPU files ---------------
BASE = dict(n=20000, d=16, T=6, D=1, m=12, lam=2, B=1024)
NQ = 32
_SCENES = {}


def scene(O, nq=NQ, java_hash=None, order=None, **over):
    """make_scene(**BASE, **over) once per distinct request, with codes_h [n][TD][W] (the code of every handle) and nq query
    codes (Q fp32, qcodes).  java_hash: 'opaque' (String.hashCode of made-up names) or 'mod5000' (ids sharing hashCodes in
    groups of four to six: survivors share (score, bucket), no bin treeifies); order: 'permuted' = a caller-given staged order."""
    from conftest import make_scene
    key = (nq, java_hash, order, tuple(sorted(over.items())))
    if key in _SCENES:
        return _SCENES[key]
    kw = dict(BASE, seed=7)
    kw.update(over)
    sc = make_scene(O, **kw)
    o, n = sc["oracle"], kw["n"]
    sc["java_hash"] = None
    if java_hash == "opaque":
        sc["java_hash"] = np.array([O.string_hash("vec-%05x-%d" % (i * 2654435761 % (1 << 20), i)) for i in range(n)], dtype=np.int32)
    elif java_hash == "mod5000":
        sc["java_hash"] = (np.arange(n) % 5000).astype(np.int32)
    sc["order"] = None
    if order == "permuted":
        sc["order"] = np.random.default_rng(kw["seed"] + 1000).permutation(n).astype(np.int32)
    if sc["java_hash"] is not None or sc["order"] is not None:
        o.set_id_meta(n, sc["java_hash"], sc["deleted"])      # GreedyPartitioner's input order is a HashMap iteration
        o.build_index(sc["X64"], sc["order"])
    sc["codes_h"] = o.encode(sc["X64"])
    sc["Q"] = sc["rng"].standard_normal((nq, kw["d"])).astype(np.float32)
    if kw.get("clustered"):
        sc["Q"] = (5 + 0.1 * sc["Q"]).astype(np.float32)
    sc["qcodes"] = o.encode(sc["Q"].astype(np.float64))
    _SCENES[key] = sc
    return sc


def tables_of(sc, sizes):
    """Every table of the scene cut by sizes(td) (a callable) or by the one list `sizes`."""
    o = sc["oracle"]
    return [recut(o, sc["codes_h"], td, sizes(td) if callable(sizes) else sizes) for td in range(o.TD)]


def uniform_tables(sc, S):
    return tables_of(sc, uniform(sc["params"]["n"], S))


def ragged_tables(sc, S, seed=3):
    rng = np.random.default_rng(seed)
    return tables_of(sc, lambda td: ragged(sc["params"]["n"], S, rng))


def oracle_for(sc, tables, **kw):
    """second_oracle with the scene's own hashCodes."""
    kw.setdefault("java_hash", sc["java_hash"])
    return second_oracle(sc, tables, **kw)


def partial_tables(sc, full):
    """Table 1 holds every second id only, table 2 a random 80 %; the others everything."""
    n = sc["params"]["n"]
    tb = list(full)
    tb[1] = subset(full[1], np.arange(n) % 2 == 0, sc["codes_h"][:, 1], 64)
    tb[2] = subset(full[2], np.random.default_rng(8).random(n) < 0.8, sc["codes_h"][:, 2], 64)
    return tb


# bounded-select limits per block size (6 tables x 5 probes x S ids) and the longest limit every list must exceed
BOUNDED_LIMITS = {2: (17, 33), 16: (17, 256, 257, 512), 63: (17, 256, 257, 512), 65: (17, 256, 257, 512),
                  100: (17, 256, 257, 512, 1024), 128: (17, 256, 257, 512, 1024)}
LISTS_EXCEED = {2: 33, 16: 257, 63: 512, 65: 512, 100: 1024, 128: 1024}
FULL_LIMITS = {2: (None, 33), 16: (None, 100, 257), 63: (None, 100, 512), 65: (None, 100, 512), 100: (None, 100, 1024),
               128: (None, 100, 1024)}
HARD_CAPS = ((100, 100), (100, 101), (100, 199), (100, 700), (16, 65))      # (block size, HARD_CAP): B = 64 in these scenes
HARD_CAP_SCENE = dict(B=64, seed=10)                                         # (no bin of bestScore treeifies at these caps)
ARENA = dict(T=10, D=4, seed=41)                                             # x 20 probes: scratch beyond LDS
SIZE_CLASSES = dict(T=16, n=60000, d=24, m=14, seed=77)
