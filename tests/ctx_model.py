"""A model of ONE long-lived context (and its clones) next to the CPU oracle: scenes, a plan generator, the expectations of every
operation, a comparator and a runner.  A helper module (no test, no fixture), like gt_ref.py and fallback_ref.py.

  Scene     the inputs both sides are given (rows, GFunctions, id hashes, deleted flags, store row type) + an oracle instance.  The
            data are integers in [-127, 127]: the same values are exact as FSPANN_I8 / F16 / BF16 / F32 / F64 rows, so the
            oracle's answer does not depend on the store's type, and integer squared distances tie for real in the top-k.
  plan()    pure Python: a list of operations with all their arguments (large arrays as the seed they are drawn from).  It touches
            neither GPU nor oracle.
  Model     applies state changes to the scene and computes what every query operation must return (cached per scene state and
            query batch: the CPU oracle is the slow side).
  run()     executes a plan against a context made by ctx_factory — or, with ctx_factory None, against the model alone — and keeps
            an operation log.  A mismatch raises with the plan's seed, the operation's index, the first differing query and the
            log so far: (seed, index) reproduces it.

Nothing here aims at a GPU fault: the refused calls are those the library rejects on the host before any launch, and NaN
queries, which it reports."""
import os
import random

import numpy as np

D_DIM = 16
ROW_TYPES = ("i8", "f16", "bf16", "f32", "f64")
BATCHES = (1, 2, 7, 33, 200, 600)
BOUNDED_LIMITS = (17, 256, 400, 1000)        # one per size class of the bounded select (512 / 512 / 1024 / 2048 entries)
KS = (1, 10, 33)
SIZES = (300, 3000, 40000)
BUILD_ROUTES = ("build_index", "append", "import", "load")
INT32_MAX = 2**31 - 1
ZERO_COPY_MAX_Q = 4                          # host_staging.h: kZeroCopyMaxQ

# T x D in {4, 8, 16}, m * lambda <= 28, B in {64, 256, 300, 1000}.  "spec" is 16 x 1 with 5 probes and blocks of 64: the
# shape-specialised bounded select.
FAMILIES = {
    "spec":  dict(T=16, D=1, m=12, lam=2, B=256),
    "eight": dict(T=4, D=2, m=10, lam=2, B=300),
    "four":  dict(T=2, D=2, m=8, lam=2, B=64),
    "wide":  dict(T=8, D=2, m=14, lam=2, B=1000),
}
FAMILY_ORDER = ("spec", "eight", "four", "wide")

QUERY_KINDS = ("encode", "route_full", "route_bounded", "refine_store", "refine_dense", "search_store", "search_retry",
               "search_fallback", "tick_front", "tick_refine", "tick_all", "groundtruth", "touched_check")
STATE_KINDS = ("set_deleted", "store_set", "rebuild", "set_id_meta", "touch_enable", "clone", "close_clone", "refused")
SEARCH_KINDS = ("search_store", "search_retry", "search_fallback")
REFUSALS = ("nan_query", "limit0", "cap_small", "append_without_begin", "nq0")
SHARED_REFUSALS = ("store_set", "build_index", "build_begin", "set_id_meta", "set_index", "finalize", "load_index")


# ---- data ------------------------------------------------------------------------------------------------------------
def int_rows(seed, n):
    """[n][16] float64 holding integers in [-127, 127]: round(30 N(0, 1)), clipped."""
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(30.0 * rng.standard_normal((n, D_DIM))), -127, 127)


def queries(qseed, nq):
    return int_rows(1_000_003 + qseed, nq).astype(np.float32)


def opaque_hashes(n, seed):
    """Caller hashCodes spread like tests/test_gpu_route_fuzz.py's: no HashMap bin comes near treeifying."""
    rng = np.random.default_rng(77_000 + seed)
    return (rng.permutation(n).astype(np.int64) * 7919 % (2**31 - 1)).astype(np.int32)


def handles_of(hseed, n, cnt):
    return np.sort(np.random.default_rng(55_000 + hseed).choice(n, size=min(cnt, n), replace=False)).astype(np.int32)


def typed_rows(pkg, X, row_type):
    """(array, dtype= argument) handing the integer rows X to store_set as `row_type`"""
    if row_type == "i8":
        return X.astype(np.int8), np.int8
    if row_type == "f16":
        return X.astype(np.float16), np.float16
    if row_type == "bf16":
        return X.astype(np.float32), pkg.bfloat16
    if row_type == "f32":
        return X.astype(np.float32), None
    assert row_type == "f64"
    return X.astype(np.float64), None


_G = {}


def family_g(O, fam_name):
    """One set of GFunctions per family, kept over every rebuild of a context (Setup's sample: the family's own draw)."""
    if fam_name not in _G:
        f = FAMILIES[fam_name]
        _G[fam_name] = O.registry_init(int_rows(4242, 1000), f["m"], 13, f["T"], f["D"])
    return _G[fam_name]


class Scene:
    """An oracle instance coupled with the inputs both sides are given."""

    def __init__(self, O, fam_name, n, seed, idkind="decimal", store="f32", deleted_frac=0.02):
        f = FAMILIES[fam_name]
        self.O, self.fam_name, self.fam = O, fam_name, f
        self.n, self.seed, self.idkind, self.store = n, seed, idkind, store
        self.X = int_rows(seed, n)
        self.X32 = self.X.astype(np.float32)
        self.alpha, self.r, self.omega = family_g(O, fam_name)
        self.jh = opaque_hashes(n, seed) if idkind == "opaque" else None
        rng = np.random.default_rng(9_000 + seed)
        self.deleted = (rng.random(n) < deleted_frac).astype(np.uint8)
        self.o = self.fresh_oracle()

    def fresh_oracle(self):
        f = self.fam
        o = self.O.Oracle(f["T"], f["D"], f["m"], f["lam"], D_DIM, refinement_limit=f["B"])
        o.set_gfunctions(self.alpha, self.r, self.omega)
        o.set_id_meta(self.n, self.jh, self.deleted)
        o.set_store(self.X)
        o.build_index(self.X)
        return o

    def set_deleted(self, handles, flag):
        self.deleted[handles] = 1 if flag else 0
        self.o.set_id_meta(self.n, self.jh, self.deleted)

    def set_idkind(self, idkind):
        self.idkind = idkind
        self.jh = opaque_hashes(self.n, self.seed) if idkind == "opaque" else None
        self.o.set_id_meta(self.n, self.jh, self.deleted)
        self.o.build_index(self.X)        # GreedyPartitioner's input order is a HashMap iteration: it depends on the hashes


# ---- plans -----------------------------------------------------------------------------------------------------------
def _q(rnd, nq=None):
    return dict(qseed=rnd.randrange(10**6), nq=nq if nq is not None else rnd.choice(BATCHES))


def _query_op(rnd, kind, st, nq=None):
    """One query operation of `kind` with all its arguments; st is the generator's shadow of the context's state."""
    op = dict(op=kind, via=_via(rnd, st))
    B = FAMILIES[st["fam"]]["B"]
    if kind == "encode":
        op.update(_q(rnd, nq), dtype=rnd.choice(("f32", "f64")), mode=rnd.choice((1, 2)))
    elif kind == "route_full":
        op.update(_q(rnd, nq), limit=rnd.choice((None, B)))
    elif kind == "route_bounded":
        op.update(_q(rnd, nq), limit=rnd.choice(BOUNDED_LIMITS))
    elif kind in ("refine_store", "refine_dense", "search_store", "search_retry", "search_fallback"):
        op.update(_q(rnd, nq), k=rnd.choice(KS))
        if kind == "refine_dense":
            op["nq"] = min(op["nq"], 200)           # [nq][B][16] rows from the host: keep the copy small
    elif kind == "tick_front":
        op.update(enc=_q(rnd, nq), route=_q(rnd))
    elif kind == "tick_refine":
        op.update(_q(rnd, nq), k=rnd.choice(KS), handover=rnd.random() < 0.5, dense=rnd.random() < 0.5)
        op["nq"] = min(op["nq"], 200)
    elif kind == "tick_all":
        op.update(batches=[_q(rnd, rnd.choice((7, 33, 200))) for _ in range(3)], k=rnd.choice(KS), handover=rnd.random() < 0.5,
                  dense=rnd.random() < 0.5)
    elif kind == "groundtruth":
        op.update(_q(rnd, nq if nq is not None else rnd.choice((1, 7, 33))), k=rnd.choice((1, 5)))
    elif kind == "touched_check":
        pass
    else:
        raise ValueError(kind)
    return op


def _via(rnd, st):
    """Owner (-1) or a live clone: while clones live, query operations alternate between them."""
    if not st["clones"]:
        return -1
    st["turn"] = (st["turn"] + 1) % (st["clones"] + 1)
    return st["turn"] - 1


def _state_op(rnd, kind, st, shared=None):
    op = dict(op=kind)
    if kind == "set_deleted":
        op.update(hseed=rnd.randrange(10**6), cnt=rnd.choice((1, 5, 60)), flag=rnd.random() < 0.7, via=_via(rnd, st))
    elif kind == "store_set":
        st["store"] = rnd.choice([t for t in ROW_TYPES if t != st["store"]])
        op.update(row_type=st["store"])
    elif kind == "rebuild":
        st["n"] = rnd.choice([n for n in SIZES if n != st["n"]])
        st["sseed"] += 1
        op.update(n=st["n"], seed=st["sseed"], route=BUILD_ROUTES[st["turn_build"] % 4], idkind=st["idkind"])
        st["turn_build"] += 1
    elif kind == "set_id_meta":
        st["idkind"] = "opaque" if st["idkind"] == "decimal" else "decimal"
        op.update(idkind=st["idkind"], route=rnd.choice(BUILD_ROUTES[:3]))
    elif kind == "touch_enable":
        st["touch"] = not st["touch"]
        op.update(on=st["touch"])
    elif kind == "clone":
        st["clones"] += 1
    elif kind == "close_clone":
        st["clones"] -= 1
        op.update(which=rnd.randrange(st["clones"] + 1))
    elif kind == "refused":
        if shared if shared is not None else (st["clones"] and rnd.random() < 0.6):
            op.update(what="shared", call=rnd.choice(SHARED_REFUSALS))
        else:
            what = REFUSALS[st["turn_refused"] % len(REFUSALS)]             # each in turn (none of them while ...
            st["turn_refused"] += 1
            if st["clones"] and what == "append_without_begin":            # ... a clone lives: that one is a state change itself)
                what = "nq0"
            op.update(what=what, via=_via(rnd, st), **_q(rnd, rnd.choice((2, 7, 33))))
    else:
        raise ValueError(kind)
    return op


def initial(fam, n=3000, seed=0, idkind="decimal", store="f32", touch=False):
    return dict(fam=fam, n=n, seed=seed, idkind=idkind, store=store, touch=touch)


def plan(seed, length=30):
    """The operations of fuzz seed `seed`: dict(seed, init, env, ops).  Every state change is followed, before the next one, by a
    Route call of each select and a search call, then by a few query operations drawn at random."""
    rnd = random.Random(910_000 + seed)
    fam = FAMILY_ORDER[seed % len(FAMILY_ORDER)]
    st = dict(fam=fam, n=SIZES[(seed // 4) % 3], sseed=100 * seed, idkind="decimal", store=ROW_TYPES[seed % 5], touch=False, clones=0, turn=0,
              turn_build=seed, turn_refused=2 * seed, turn_query=5 * seed)
    init = initial(fam, st["n"], st["sseed"], st["idkind"], st["store"])
    env = {"FSPANN_ROUTE_LAZY_CAP": "258"} if seed % 3 == 1 else {}
    ops = []
    # The state changes of a plan: one of two hands of six in seeded order (each kind comes round every other seed, the build routes
    # and the refused calls taking turns across seeds), then kinds drawn at random.  A clone lives across a refused state change.
    if seed % 2 == 0:
        hand = ["set_deleted", "rebuild", "refused", "clones"]
        rnd.shuffle(hand)
        i = hand.index("clones")
        hand[i:i + 1] = ["clone", "set_deleted", "shared", "close_clone"] if rnd.random() < 0.5 else ["clone", "shared", "close_clone"]
    else:
        hand = ["touch_enable", "rebuild", "store_set", "refused", "set_id_meta", "refused"]
        rnd.shuffle(hand)
    weights = dict(set_deleted=3, store_set=3, rebuild=3, set_id_meta=2, touch_enable=2, clone=2, close_clone=2, refused=3)
    while hand or len(ops) < length:
        if hand:
            kind = hand.pop(0)
        else:
            kinds = [k for k in STATE_KINDS if not (k == "close_clone" and st["clones"] == 0) and not (k == "clone" and st["clones"] >= 2)
                     and not (st["clones"] and k in ("store_set", "rebuild", "set_id_meta"))]
            kind = rnd.choices(kinds, [weights[k] for k in kinds])[0]
        ops.append(_state_op(rnd, "refused", st, shared=True) if kind == "shared" else _state_op(rnd, kind, st))
        ops.append(_query_op(rnd, "route_full", st))
        ops.append(_query_op(rnd, "route_bounded", st))
        ops.append(_query_op(rnd, rnd.choice(SEARCH_KINDS), st))
        for _ in range(rnd.randrange(0, 3)):     # the other query operations take turns, from a start that moves with the seed
            ops.append(_query_op(rnd, QUERY_KINDS[st["turn_query"] % len(QUERY_KINDS)], st))
            st["turn_query"] += 1
    while st["clones"]:                          # (a plan ends with its clones closed before the owner)
        ops.append(_state_op(rnd, "close_clone", st))
        ops += [_query_op(rnd, "route_full", st), _query_op(rnd, "route_bounded", st), _query_op(rnd, rnd.choice(SEARCH_KINDS), st)]
    return dict(seed=seed, init=init, env=env, ops=ops)


# ---- named sequences -----------------------------------------------------------------------------------------------------
def _serve(qs, B, k=10, ticks=True):
    """Every query operation once, over the query batches qs (a list of dict(qseed, nq))."""
    it = iter(qs * 20)
    nx = lambda: dict(next(it))
    ops = [dict(op="encode", via=-1, dtype="f32", mode=2, **nx()), dict(op="encode", via=-1, dtype="f64", mode=1, **nx()),
           dict(op="route_full", via=-1, limit=None, **nx()), dict(op="route_full", via=-1, limit=B, **nx())]
    ops += [dict(op="route_bounded", via=-1, limit=lim, **nx()) for lim in BOUNDED_LIMITS]
    ops += [dict(op=kind, via=-1, k=k, **nx()) for kind in ("refine_store", "refine_dense", "search_store", "search_retry", "search_fallback")]
    if ticks:
        ops += [dict(op="tick_front", via=-1, enc=nx(), route=nx()),
                dict(op="tick_refine", via=-1, k=k, handover=True, dense=False, **nx()),
                dict(op="tick_refine", via=-1, k=k, handover=False, dense=True, **nx()),
                dict(op="tick_all", via=-1, batches=[nx(), nx(), nx()], k=k, handover=True, dense=False)]
    ops += [dict(op="groundtruth", via=-1, k=5, **nx()), dict(op="touched_check")]
    return ops


def _both_selects(q, B, k=10):
    return [dict(op="route_full", via=-1, limit=B, **q), dict(op="route_bounded", via=-1, limit=256, **q), dict(op="route_bounded", via=-1, limit=17, **q),
            dict(op="search_store", via=-1, k=k, **q)]


def named_rebuild(route):
    """Build, serve through every query operation, rebuild with fewer rows, serve, rebuild with more rows, serve: 40000 -> 300 -> 3000."""
    B = FAMILIES["spec"]["B"]
    qs = [dict(qseed=11, nq=33), dict(qseed=12, nq=7), dict(qseed=13, nq=200), dict(qseed=14, nq=2)]
    ops = [dict(op="touch_enable", on=True)] + _serve(qs, B)
    ops += [dict(op="rebuild", n=300, seed=901, route=route, idkind="decimal")] + _serve(qs, B)
    ops += [dict(op="rebuild", n=3000, seed=902, route=route, idkind="decimal")] + _serve(qs, B)
    return dict(seed="rebuild-" + route, init=initial("spec", 40000, 900), env={}, ops=ops)


def named_id_meta():
    B = FAMILIES["spec"]["B"]
    q, q2 = dict(qseed=21, nq=33), dict(qseed=22, nq=200)
    ops = _both_selects(q, B) + [dict(op="set_id_meta", idkind="opaque", route="build_index", refused_between=True)] + _both_selects(q, B) + _both_selects(q2, B)
    ops += [dict(op="set_id_meta", idkind="decimal", route="import", refused_between=True)] + _both_selects(q, B) + _both_selects(q2, B)
    ops += [dict(op="set_id_meta", idkind="opaque", route="append", refused_between=True)] + _both_selects(q2, B)
    return dict(seed="id-meta", init=initial("spec", 3000, 910), env={}, ops=ops)


def named_store_type():
    q = dict(qseed=31, nq=33)
    ops = [dict(op="touch_enable", on=True)]
    for t in ("i8", "f16", "bf16", "f32", "f64", "i8"):
        ops += [dict(op="store_set", row_type=t), dict(op="refine_store", via=-1, k=10, **q), dict(op="search_store", via=-1, k=10, **q),
                dict(op="tick_refine", via=-1, k=10, handover=False, dense=False, **q), dict(op="tick_all", via=-1, batches=[q, dict(qseed=32, nq=7), dict(qseed=33, nq=200)],
                                                                                            k=10, handover=True, dense=False),
                dict(op="groundtruth", via=-1, k=5, qseed=34, nq=7), dict(op="touched_check")]
    return dict(seed="store-type", init=initial("spec", 3000, 920, store="f64"), env={}, ops=ops)


def named_batch_sizes(fam="spec"):
    """600 -> 1 -> 200 -> 2 -> 600 through each entry point on one context."""
    ops = [dict(op="touch_enable", on=True)]
    B = FAMILIES[fam]["B"]
    for kind in QUERY_KINDS:
        if kind == "touched_check":
            continue
        for i, nq in enumerate((600, 1, 200, 2, 600)):
            q = dict(qseed=40 + i, nq=nq)
            if kind == "encode":
                ops.append(dict(op=kind, via=-1, dtype=("f32", "f64")[i % 2], mode=1 + i % 2, **q))
            elif kind == "route_full":
                ops.append(dict(op=kind, via=-1, limit=(None, B)[i % 2], **q))
            elif kind == "route_bounded":
                ops.append(dict(op=kind, via=-1, limit=BOUNDED_LIMITS[i % 4], **q))
            elif kind == "tick_front":
                ops.append(dict(op=kind, via=-1, enc=q, route=dict(qseed=50 + i, nq=(2, 600, 1, 200, 600)[i])))
            elif kind == "tick_refine":
                ops.append(dict(op=kind, via=-1, k=10, handover=i % 2 == 0, dense=i == 3, **q))
            elif kind == "tick_all":
                ops.append(dict(op=kind, via=-1, batches=[q, dict(qseed=60 + i, nq=(1, 600, 2, 200, 33)[i]), dict(qseed=70 + i, nq=(200, 2, 600, 1, 7)[i])], k=10,
                                handover=i % 2 == 1, dense=False))
            elif kind == "groundtruth":
                ops.append(dict(op=kind, via=-1, k=5, **q))
            else:
                ops.append(dict(op=kind, via=-1, k=KS[i % 3], **q))
        ops.append(dict(op="touched_check"))
    return dict(seed="batch-sizes-" + fam, init=initial(fam, 3000, 930), env={}, ops=ops)


def named_size_classes():
    """FSPANN_ROUTE_LAZY_CAP=258: consecutive bounded-select calls alternate the 512 / 1024 / 2048-entry classes, interleaved with
    the search calls and front-launch ticks, so the overflow counters' turn passes between kernels of different builds."""
    ops = []
    for i, lim in enumerate((256, 400, 1000, 400, 256, 1000, 256, 256, 400)):
        q = dict(qseed=80 + i, nq=(200, 33, 600, 7, 200, 33, 600, 200, 33)[i])
        ops.append(dict(op="route_bounded", via=-1, limit=lim, expect_overflow=True, **q))
        other = (dict(op="search_store", via=-1, k=10, **q), dict(op="search_retry", via=-1, k=10, qseed=90 + i, nq=33),
                 dict(op="tick_front", via=-1, enc=dict(qseed=95 + i, nq=7), route=q))[i % 3]
        ops.append(other)
    ops.append(dict(op="route_bounded", via=-1, limit=256, expect_overflow=True, qseed=80, nq=200))
    return dict(seed="size-classes", init=initial("spec", 40000, 940), env={"FSPANN_ROUTE_LAZY_CAP": "258"}, ops=ops)


def named_redo_slots():
    """More than eight consecutive refine-only ticks with a hand-over buffer and differing parameters (nq, B, k, buffers): the
    redo-parameter slots wrap; then an earlier parameter set again."""
    sets = [dict(nq=96, B=256, k=10), dict(nq=33, B=256, k=10), dict(nq=96, B=64, k=1), dict(nq=7, B=256, k=33), dict(nq=200, B=256, k=10),
            dict(nq=33, B=64, k=10), dict(nq=96, B=256, k=33), dict(nq=2, B=256, k=1), dict(nq=200, B=64, k=10), dict(nq=33, B=256, k=1),
            dict(nq=96, B=17, k=10)]
    batches = [dict(qseed=100 + i, **s) for i, s in enumerate(sets)]
    ops = [dict(op="tick_redo", via=-1, batches=batches, repeat=(0, 3, 0)),
           dict(op="route_bounded", via=-1, limit=256, expect_overflow=True, qseed=100, nq=96), dict(op="search_store", via=-1, k=10, qseed=101, nq=33)]
    return dict(seed="redo-slots", init=initial("spec", 40000, 950), env={"FSPANN_ROUTE_LAZY_CAP": "258"}, ops=ops)


def named_failed_calls():
    q = dict(qseed=111, nq=33)
    ops = []
    for what in REFUSALS:
        ops += [dict(op="refused", what=what, via=-1, **q)]          # (the good call each imitates runs inside the operation, right behind it)
        ops += _both_selects(dict(qseed=112, nq=7), FAMILIES["eight"]["B"])
    return dict(seed="failed-calls", init=initial("eight", 3000, 960), env={}, ops=ops)


def named_fallback_after_deletes():
    """Everything two queries reach is deleted on the serving context: they come back empty and take runQueries' fallback (a whole
    search at 10 probes, in place); the deletes are taken back and the same batch is served again."""
    q = dict(qseed=131, nq=33)
    reach = dict(q, rows=(0, 20))
    ops = [dict(op="touch_enable", on=True), dict(op="search_fallback", via=-1, k=10, **q), dict(op="set_deleted", reach=reach, flag=True, via=-1),
           dict(op="search_fallback", via=-1, k=10, expect_fellback=2, **q), dict(op="search_retry", via=-1, k=10, **q), dict(op="touched_check")]
    ops += _both_selects(q, FAMILIES["eight"]["B"])
    ops += [dict(op="set_deleted", reach=reach, flag=False, via=-1), dict(op="search_fallback", via=-1, k=10, expect_fellback=0, **q),
            dict(op="search_fallback", via=-1, k=33, expect_fellback=0, qseed=132, nq=200), dict(op="touched_check")]
    return dict(seed="fallback-after-deletes", init=initial("eight", 40000, 980), env={}, ops=ops)


def named_owner_and_clones():
    B = FAMILIES["spec"]["B"]
    q = [dict(qseed=120 + i, nq=(33, 7, 200, 2, 33, 7)[i]) for i in range(6)]
    ops = [dict(op="touch_enable", on=True), dict(op="clone")]
    ops += [dict(op="search_store", via=-1, k=10, **q[0]), dict(op="search_retry", via=0, k=10, **q[1]), dict(op="route_bounded", via=0, limit=256, **q[2])]
    ops += [dict(op="set_deleted", hseed=1, cnt=60, flag=True, via=0), dict(op="route_full", via=-1, limit=B, **q[2]), dict(op="clone"),
            dict(op="set_deleted", hseed=2, cnt=60, flag=True, via=-1)]
    for i, via in enumerate((1, 0, -1, 1, 0, -1)):
        kind = ("search_store", "route_bounded", "tick_all", "search_fallback", "refine_store", "tick_refine")[i]
        op = dict(op=kind, via=via)
        if kind == "route_bounded":
            op.update(limit=17, **q[i])
        elif kind == "tick_all":
            op.update(batches=[q[0], q[1], q[2]], k=10, handover=True, dense=False)
        elif kind == "tick_refine":
            op.update(k=10, handover=True, dense=False, **q[i])
        else:
            op.update(k=10, **q[i])
        ops.append(op)
    ops.append(dict(op="set_deleted", hseed=1, cnt=60, flag=False, via=1))
    for call in SHARED_REFUSALS:
        ops += [dict(op="refused", what="shared", call=call), dict(op="route_bounded", via=(0, 1, -1)[len(ops) % 3], limit=256, **q[0])]
    ops += [dict(op="touched_check"), dict(op="close_clone", which=0), dict(op="search_store", via=0, k=10, **q[3]), dict(op="close_clone", which=0),
            dict(op="store_set", row_type="i8"), dict(op="rebuild", n=300, seed=971, route="build_index", idkind="decimal")]
    ops += _both_selects(q[0], B) + [dict(op="touched_check")]
    return dict(seed="owner-and-clones", init=initial("spec", 3000, 970), env={}, ops=ops)


def named_plans():
    out = {"rebuild-" + r: named_rebuild(r) for r in BUILD_ROUTES}
    for p in (named_id_meta(), named_store_type(), named_batch_sizes("spec"), named_batch_sizes("eight"), named_size_classes(), named_redo_slots(),
              named_failed_calls(), named_fallback_after_deletes(), named_owner_and_clones()):
        out[p["seed"]] = p
    return out


# ---- the model: expectations ---------------------------------------------------------------------------------------------
def _mask(a, cnt, width, fill=-1):
    """[nq][width]: the first cnt[i] entries of row i of a, `fill` behind them"""
    nq = a.shape[0]
    out = np.full((nq, width), fill, a.dtype)
    w = min(width, a.shape[1])
    out[:, :w] = a[:, :w]
    out[np.arange(width)[None] >= np.asarray(cnt)[:, None]] = fill
    return out


class Model:
    def __init__(self, O, plan_):
        self.O = O
        i = plan_["init"]
        self.fam_name, self.fam = i["fam"], FAMILIES[i["fam"]]
        self.scene = Scene(O, i["fam"], i["n"], i["seed"], i["idkind"], i["store"])
        self.version = 0                  # bumped by every change that can change an answer
        self.cache = {}
        self.touch_on = False
        self.touch_set = None             # None: tracking was never enabled; else the handles the device set must hold
        self.clones = 0
        self.lazy_cap = int(plan_["env"].get("FSPANN_ROUTE_LAZY_CAP", "0"))
        self.last_handles = None          # the handles of the last set_deleted (the device side deletes the same ones)
        self.treeified = 0                # queries the oracle would leave out (HashMap bin treeified): must stay 0
        self.compared = 0
        if i.get("touch"):
            self.touch_enable(True)

    # -- state changes --------------------------------------------------------------------------------------------------
    def set_deleted(self, handles, flag):
        self.scene.set_deleted(handles, flag)
        self.version += 1

    def store_set(self, row_type):
        self.scene.store = row_type       # (no version bump: the answers do not depend on the store's type)

    def rebuild(self, n, seed, idkind):
        old_n = self.scene.n
        self.scene = Scene(self.O, self.fam_name, n, seed, idkind, self.scene.store)
        self.version += 1
        if self.touch_set is not None and n != old_n:
            self.touch_set = set()        # fspann_set_id_meta: a touched set in use follows the new handle count, cleared

    def set_idkind(self, idkind):
        self.scene.set_idkind(idkind)
        self.version += 1

    def touch_enable(self, on):
        self.touch_on = bool(on)
        if on and self.touch_set is None:
            self.touch_set = set()

    def _touch(self, Q, sel, cnt):
        if not self.touch_on or self.touch_set is None:
            return
        for i in np.flatnonzero(np.isfinite(Q).all(1)):
            self.touch_set.update(int(h) for h in sel[i, :cnt[i]])

    # -- references (cached per scene state and query batch) -----------------------------------------------------------------
    def _cached(self, key, fn):
        key = (self.version,) + key
        if key not in self.cache:
            self.cache[key] = fn()
        return self.cache[key]

    def codes(self, q):
        def f():
            Q = queries(q["qseed"], q["nq"])
            return self.scene.o.encode(Q.astype(np.float64))
        return self._cached(("codes", q["qseed"], q["nq"]), f)

    def routed(self, q, po=-1):
        def f():
            o = self.scene.o
            c = self.codes(q)
            ids, score, count, raw = o.route(c, probe_override=po)
            self.treeified += int(o.route_treeified(c, probe_override=po).sum())
            assert not o.unmodelled, "oracle HashMap treeified: order not pinned for this scene"
            return ids, score, count, raw
        return self._cached(("route", q["qseed"], q["nq"], po), f)

    def reached(self, spec):
        """every handle pass 1 of a search reaches for the queries spec["rows"] of a batch — deleted or not (tests/fallback_ref.py's
        empty_scene: with all of them deleted those queries return nothing and take runQueries' fallback)"""
        was = self.scene.deleted.copy()
        self.scene.set_deleted(np.arange(self.scene.n), False)
        ids, _, count, _ = self.scene.o.route(self.codes(spec))
        self.scene.deleted[:] = was
        self.scene.set_deleted(np.arange(0), False)
        return np.unique(np.concatenate([ids[r, :count[r]] for r in spec["rows"]])).astype(np.int32)

    def selected(self, q, B, po=-1):
        """stage A.5's F_q: the first B routed ids (-1 behind them) and how many"""
        ids, _, count, _ = self.routed(q, po)
        cnt = np.minimum(count, B).astype(np.int32)
        return _mask(ids, cnt, B), cnt

    def maxcand(self, po=-1):
        return self.fam["T"] * self.fam["D"] * (5 if po < 0 else po) * 64

    def refined(self, q, B, k):
        def f():
            Q = queries(q["qseed"], q["nq"])
            sel, cnt = self.selected(q, B)
            rows = self.scene.X[np.clip(sel, 0, self.scene.n - 1)]
            ids, dist, count = self.O.refine(Q.astype(np.float64), rows, sel, cnt, k)
            return dict(ids=ids, dist=dist, count=count, scored=cnt.copy())
        return self._cached(("refine", q["qseed"], q["nq"], B, k), f)

    def searched(self, q, k, po=-1):
        def f():
            Q = queries(q["qseed"], q["nq"])
            ref = self.scene.o.search(Q.astype(np.float64), k, codes=self.codes(q), probe_override=po)
            self.routed(q, po)
            if ref["metrics"][:, 4].any():
                self.routed(q, 10)          # (the retry's Route: its treeified queries count too)
            return ref
        return self._cached(("search", q["qseed"], q["nq"], k, po), f)

    # -- what each query operation must return; the touched set follows --------------------------------------------------------
    def expect(self, op):
        kind, B = op["op"], self.fam["B"]
        if kind == "encode":
            return dict(codes=self.codes(op))
        if kind in ("route_full", "route_bounded"):
            ids, score, count, raw = self.routed(op)
            lim = op["limit"] or INT32_MAX
            width = max(1, min(lim, self.maxcand()))
            cnt = np.minimum(count, lim).astype(np.int32)
            e = dict(count=cnt, ids=_mask(ids, cnt, width), score=_mask(score, cnt, width))
            if kind == "route_full":
                e.update(kept=count, raw_seen=raw)
            else:
                e.update(lazy=np.array([1], np.int32))       # mode 2, no counters, limit <= 1024, no HARD_CAP in reach: legal
            return e
        if kind in ("refine_store", "refine_dense", "search_store", "tick_refine"):
            Q = queries(op["qseed"], op["nq"])
            sel, cnt = self.selected(op, B)
            e = dict(self.refined(op, B, op["k"]))
            if kind in ("search_store", "tick_refine"):
                e.update(sel=sel, selc=cnt)
            if kind == "search_store":
                e.update(bad=np.zeros(op["nq"], np.int32))
            self._touch(Q, sel, cnt)
            return e
        if kind == "search_retry":
            return self._expect_retry(op, op["k"])
        if kind == "search_fallback":
            import fallback_ref
            Q = queries(op["qseed"], op["nq"])
            o, k = self.scene.o, op["k"]
            F = fallback_ref.fallback_probes(-1, -1)
            ref1 = self.searched(op, k)
            fb = ref1["count"] == 0
            out = {key: v.copy() for key, v in ref1.items()}
            self._touch_search(op, Q, ref1, -1, np.ones(len(Q), bool))
            if fb.any():
                r2 = o.search(Q[fb].astype(np.float64), k, codes=self.codes(op)[fb], probe_override=F)
                for key in out:
                    out[key][fb] = r2[key]
                full = {key: out[key] for key in ("sel", "sel_count")}
                self._touch_search(op, Q, full, F, fb)
            return dict(ids=out["ids"], dist=out["dist"], count=out["count"], scored=out["metrics"][:, 2].copy(), ret=out["metrics"][:, 4].copy(),
                        selc=out["sel_count"], sel=_mask(out["sel"], out["sel_count"], B), fb=fb.astype(np.int32), bad=np.zeros(len(Q), np.int32))
        if kind == "tick_front":
            sel, cnt = self.selected(op["route"], B)
            return dict(codes=self.codes(op["enc"]), sel=sel, selc=cnt, bad=np.zeros(op["enc"]["nq"], np.int32))
        if kind in ("tick_all", "tick_redo"):
            e = {}
            order = list(range(len(op["batches"]))) + list(op.get("repeat", ()))
            for j, bi in enumerate(order):
                b = op["batches"][bi]
                Bb, k = b.get("B", B), b.get("k", op.get("k"))
                sel, cnt = self.selected(b, Bb)
                r = self.refined(b, Bb, k)
                self._touch(queries(b["qseed"], b["nq"]), sel, cnt)
                for key, v in dict(r, sel=sel, selc=cnt, codes=self.codes(b)).items():
                    e["b%d.%s" % (j, key)] = v
            return e
        if kind == "groundtruth":
            if self.scene.store == "f64":
                return dict(refused=np.array([1], np.int32))      # no ground truth over an FSPANN_F64 store (host check, no launch)
            Q = queries(op["qseed"], op["nq"])
            ids, d2 = self._cached(("gt", op["qseed"], op["nq"], op["k"]), lambda: self.O.groundtruth(self.scene.X32, Q, op["k"]))
            return dict(refused=np.array([0], np.int32), ids=ids, d2=d2)
        if kind == "touched_check":
            if self.touch_set is None:
                return dict(never_enabled=np.array([1], np.int32))
            e = dict(never_enabled=np.array([0], np.int32), touched=np.array(sorted(self.touch_set), np.int32))
            self.touch_set = set()                                # drained with reset
            return e
        raise ValueError(kind)

    def _touch_search(self, q, Q, ref, po, rows):
        """test_gpu_touched.py::_expected's rule: pass 1's F_q and the last pass's F_q of every finite query (all store rows are valid here)"""
        B = self.fam["B"]
        sel1, cnt1 = self.selected(q, B, po)
        keep = rows & np.isfinite(Q).all(1)
        self._touch(Q[keep], sel1[keep], cnt1[keep])
        self._touch(Q[keep], ref["sel"][keep], ref["sel_count"][keep])

    def _expect_retry(self, op, k, nan_rows=()):
        Q = queries(op["qseed"], op["nq"])
        B = self.fam["B"]
        if len(nan_rows):
            Q = Q.copy()
            Q[list(nan_rows), 3] = np.nan
            codes = self.scene.o.encode(np.where(np.isfinite(Q), Q, 0).astype(np.float64))     # (a non-finite query is never coded: QSI:137-140)
            ref = self.scene.o.search(Q.astype(np.float64), k, codes=codes)
            self.routed(op)
            keep = np.isfinite(Q).all(1)
            sel1, cnt1 = self.selected(op, B)
            self._touch(Q[keep], sel1[keep], cnt1[keep])
            self._touch(Q[keep], ref["sel"][keep], ref["sel_count"][keep])
        else:
            ref = self.searched(op, k)
            self._touch_search(op, Q, ref, -1, np.ones(len(Q), bool))
        bad = (~np.isfinite(Q).all(1)).astype(np.int32)
        return dict(ids=ref["ids"], dist=ref["dist"], count=ref["count"], scored=ref["metrics"][:, 2].copy(), ret=ref["metrics"][:, 4].copy(),
                    selc=ref["sel_count"], sel=_mask(ref["sel"], ref["sel_count"], B), bad=bad)


# ---- the comparator ------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def compare(got, exp, skip_rows=None):
    """Exact comparison of every expected array (floats by bit pattern).  Raises Mismatch naming the key and the first differing
    query (row).  skip_rows {key: bool [nq]}: rows of that key the reference leaves undefined (F_q of a non-finite query)."""
    for key in exp:
        if key not in got:
            raise Mismatch("output %r is missing" % key)
        a, b = np.asarray(got[key]), np.asarray(exp[key])
        if key == "touched":
            sa, sb = set(a.tolist()), set(b.tolist())
            if sa != sb or len(a) != len(b) or np.any(np.diff(a) <= 0):
                raise Mismatch("touched set differs: handles missing %s, handles unexpected %s, ascending %s" %
                               (sorted(sb - sa)[:10], sorted(sa - sb)[:10], bool(np.all(np.diff(a) > 0))))
            continue
        if a.shape != b.shape:
            raise Mismatch("%s: shape %s, expected %s (first differing query %d)" % (key, a.shape, b.shape, min(a.shape[0], b.shape[0]) if a.ndim and b.ndim else 0))
        if a.dtype.kind == "f" or b.dtype.kind == "f":
            a, b = np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64)
        ne = a != b
        if ne.ndim > 1:
            ne = ne.reshape(ne.shape[0], -1).any(1)
        if skip_rows is not None and key in skip_rows:
            ne = ne & ~skip_rows[key]
        if ne.any():
            i = int(np.flatnonzero(ne)[0])
            ga, gb = np.asarray(got[key])[i], np.asarray(exp[key])[i]
            raise Mismatch("%s differs: first differing query %d of %d (%d differ): got %s, expected %s" %
                           (key, i, len(ne), int(ne.sum()), np.array2string(np.ravel(ga)[:12]), np.array2string(np.ravel(gb)[:12])))


# ---- the device side -------------------------------------------------------------------------------------------------------
def make_cfg(pkg, fam_name):
    f = FAMILIES[fam_name]
    return pkg.PaperRuntimeConfig(tables=f["T"], divisions=f["D"], m=f["m"], lambda_=f["lam"], dim=D_DIM, refinement_limit=f["B"])


class Device:
    """The context under test and its clones; one method per operation, returning arrays in the model's shapes."""

    def __init__(self, pkg, ctx_factory, model, tmp_path):
        self.pkg, self.factory, self.m, self.tmp = pkg, ctx_factory, model, str(tmp_path)
        self.owner = ctx_factory(model.fam_name)
        self.clones = []
        self.info = {}
        sc = model.scene
        self.owner.set_gfunctions(sc.alpha, sc.r, sc.omega)
        self._build(sc, "build_index")
        self._store(sc)

    def close(self):
        for c in self.clones:
            c.close()
        self.owner.close()

    def ctx(self, via):
        return self.owner if via is None or via < 0 else self.clones[via]

    def _store(self, sc):
        rows, dt = typed_rows(self.pkg, sc.X, sc.store)
        self.owner.store_set(rows, dtype=dt)

    def _build(self, sc, route, between=None):
        c = self.owner
        if route == "load":
            path = os.path.join(self.tmp, "ctx_model_%d.fspann" % sc.seed)
            with self.factory(self.m.fam_name) as other:
                other.set_gfunctions(sc.alpha, sc.r, sc.omega)
                other.set_id_meta(sc.n, sc.jh, sc.deleted)
                other.build_index(sc.X32)
                other.save_index(path)
            c.load_index(path)
            return
        c.set_id_meta(sc.n, sc.jh, sc.deleted)
        if between is not None:
            between()
        if route == "build_index":
            c.build_index(sc.X32)
        elif route == "append":
            c.build_begin(sc.n)
            cuts = sorted({0, sc.n} | {int(sc.n * f) for f in (0.07, 0.5, 0.51)})       # ragged pieces
            for a, b in zip(cuts[:-1], cuts[1:]):
                c.build_append(sc.X32[a:b] if a % 2 == 0 else sc.X[a:b])
            c.build_finish()
        elif route == "import":
            for td in range(sc.o.TD):
                c.set_index(td, **sc.o.get_index(td))
            c.finalize()
        else:
            raise ValueError(route)

    # -- state changes --------------------------------------------------------------------------------------------------------
    def state(self, op):
        kind, m, pkg = op["op"], self.m, self.pkg
        if kind == "set_deleted":
            self.ctx(op["via"]).set_deleted(m.last_handles, op["flag"])
        elif kind == "store_set":
            self._store(m.scene)
        elif kind in ("rebuild", "set_id_meta"):
            between = None
            if op.get("refused_between"):
                def between():
                    c = m.codes(dict(qseed=1, nq=2))
                    for mode in (0, 2):
                        self.owner.set_route_mode(mode)
                        try:
                            self.owner.route(c, limit=17, counters=mode == 0)
                        except pkg.FspannStateError as e:
                            assert "not finalized" in str(e), str(e)
                        else:
                            raise Mismatch("a Route call between set_id_meta and finalize was not refused")
                    self.owner.set_route_mode(0)
            self._build(m.scene, op["route"], between)
            if kind == "rebuild":
                self._store(m.scene)
        elif kind == "touch_enable":
            self.owner.touch_enable(op["on"])
        elif kind == "clone":
            self.clones.append(self.owner.clone())
        elif kind == "close_clone":
            self.clones.pop(op["which"]).close()
        else:
            raise ValueError(kind)

    def refused(self, op):
        """The refused call itself: it must raise the library's error for it (or, nq = 0, do nothing)."""
        pkg, m, what = self.pkg, self.m, op["what"]
        sc = m.scene
        if what == "shared":
            call, c = op["call"], self.owner
            rows, dt = typed_rows(pkg, sc.X, "f32")
            calls = dict(store_set=lambda: c.store_set(rows, dtype=dt), build_index=lambda: c.build_index(sc.X32), build_begin=lambda: c.build_begin(sc.n),
                         set_id_meta=lambda: c.set_id_meta(sc.n, sc.jh, sc.deleted), set_index=lambda: c.set_index(0, **sc.o.get_index(0)),
                         finalize=lambda: c.finalize(), load_index=lambda: c.load_index(os.path.join(self.tmp, "never_read.fspann")))
            try:
                calls[call]()
            except pkg.FspannStateError as e:
                assert "shared with" in str(e), str(e)
            else:
                raise Mismatch("%s was accepted while a clone is alive" % call)
            return
        c = self.ctx(op["via"])
        codes = m.codes(op)
        B = m.fam["B"]
        if what == "nan_query":
            return
        if what == "limit0":
            for counters in (True, False):
                try:
                    c.route(codes, limit=0, cap=4, counters=counters)
                except pkg.FspannArgumentError as e:
                    assert "limit must be > 0" in str(e), str(e)
                else:
                    raise Mismatch("limit=0 was accepted")
        elif what == "cap_small":
            for mode, counters in ((0, True), (2, False)):
                c.set_route_mode(mode)
                try:
                    c.route(codes, limit=B, cap=B - 1, counters=counters)
                except pkg.FspannRangeError as e:
                    assert "worst case" in str(e), str(e)
                else:
                    raise Mismatch("cap < min(limit, worst case) was accepted")
            c.set_route_mode(0)
        elif what == "append_without_begin":
            try:
                self.owner.build_append(sc.X32[:8])
            except pkg.FspannStateError as e:
                assert "no build in progress" in str(e), str(e)
            else:
                raise Mismatch("build_append without build_begin was accepted")
        elif what == "nq0":
            got = c.route(np.zeros((0, c.TD, c.W), np.uint64), limit=B)
            assert got["count"].shape == (0,)
            assert c.encode(np.zeros((0, D_DIM), np.float32)).shape[0] == 0
        else:
            raise ValueError(what)

    # -- query operations ---------------------------------------------------------------------------------------------------------
    def query(self, op):
        kind, m, pkg = op["op"], self.m, self.pkg
        B = m.fam["B"]
        c = self.ctx(op.get("via"))
        self.info = {}
        if kind == "encode":
            Q = queries(op["qseed"], op["nq"]).astype(np.float32 if op["dtype"] == "f32" else np.float64)
            c.set_encode_mode(op["mode"])
            codes = c.encode(Q)
            c.set_encode_mode(0)
            self.info = dict(zero_copy=op["nq"] <= ZERO_COPY_MAX_Q)
            return dict(codes=codes)
        if kind in ("route_full", "route_bounded"):
            codes = m.codes(op)
            lim = op["limit"] or INT32_MAX
            if kind == "route_full":
                res = c.route(codes, limit=lim)
                self.info = dict(c.last_route_info(), zero_copy=op["nq"] <= ZERO_COPY_MAX_Q)
            else:
                c.set_route_mode(2)
                res = c.route(codes, limit=lim, counters=False)
                info = c.last_route_info()
                c.set_route_mode(0)
                res["lazy"] = np.array([int(info["lazy"])], np.int32)
                self.info = dict(info, zero_copy=op["nq"] <= ZERO_COPY_MAX_Q)
            w = res["ids"].shape[1]
            res["ids"], res["score"] = _mask(res["ids"], res["count"], w), _mask(res["score"], res["count"], w)
            return res
        if kind in ("refine_store", "refine_dense"):
            Q = queries(op["qseed"], op["nq"])
            sel, cnt = m.selected(op, B)
            if kind == "refine_store":
                return c.refine_store(Q, sel, cnt, op["k"])
            rows = m.scene.X32[np.clip(sel, 0, m.scene.n - 1)]
            if op["nq"] % 2:                     # every other size: packed into the context's pinned host block, as the adapter does
                pinned = c.host_buffer(rows.shape, np.float32)
                pinned[:] = rows
                rows = pinned
            return c.refine(Q, rows, sel, cnt, op["k"])
        if kind in ("search_store", "search_retry"):
            from test_gpu_touched import _search
            Q = queries(op["qseed"], op["nq"])
            for r in op.get("nan_rows", ()):
                Q[r, 3] = np.nan
            got = _search(c, Q, B, op["k"], -1, call="plain" if kind == "search_store" else "retry", finish=True)
            self.info = c.last_route_info()
            got["sel"] = _mask(got["sel"], np.maximum(got["selc"], 0), B)
            return got
        if kind == "search_fallback":
            import fallback_ref
            got = fallback_ref.run(c, queries(op["qseed"], op["nq"]), B, op["k"], -1, finish=True)
            self.info = dict(c.last_route_info(), fellback=int(got["fb"].sum()), retried=int(got["ret"].sum()))
            got["sel"] = _mask(got["sel"], np.maximum(got["selc"], 0), B)
            return got
        if kind == "tick_front":
            out = self._ticks(c, [op["route"], op["enc"]], [(0, None, None), (1, 0, None)], handover=False, dense=False)
            return dict(codes=out["b1.codes"], sel=out["b0.sel"], selc=out["b0.selc"], bad=out["b1.bad"])
        if kind == "tick_refine":
            out = self._ticks(c, [dict(op)], [(0, None, None), (None, 0, None), (None, None, 0)], handover=op["handover"], dense=op["dense"])
            return {key[3:]: v for key, v in out.items()}
        if kind == "tick_all":
            nb = len(op["batches"])
            sched = [(t if t < nb else None, t - 1 if 0 <= t - 1 < nb else None, t - 2 if 0 <= t - 2 < nb else None) for t in range(nb + 2)]
            return self._ticks(c, [dict(b, k=op["k"]) for b in op["batches"]], sched, handover=op["handover"], dense=op["dense"])
        if kind == "tick_redo":
            nb = len(op["batches"])
            sched = [(i, None, None) for i in range(nb)] + [(None, i, None) for i in range(nb)] + [(None, None, i) for i in range(nb)]
            out = self._ticks(c, op["batches"], sched, handover=True, dense=False, repeat=op["repeat"])
            return out
        if kind == "groundtruth":
            import torch
            dev = torch.device("cuda", 0)
            qd = torch.from_numpy(queries(op["qseed"], op["nq"])).to(dev)
            ids = torch.full((op["nq"], op["k"]), -7, dtype=torch.int32, device=dev)
            d2 = torch.zeros((op["nq"], op["k"]), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            try:
                c.groundtruth_store_dev(op["nq"], qd.data_ptr(), op["k"], ids.data_ptr(), d2.data_ptr())
            except pkg.FspannArgumentError as e:
                assert "FSPANN_F64" in str(e), str(e)
                return dict(refused=np.array([1], np.int32))
            c.sync()
            return dict(refused=np.array([0], np.int32), ids=ids.cpu().numpy(), d2=d2.cpu().numpy())
        if kind == "touched_check":
            c = self.clones[-1] if self.clones else self.owner
            try:
                n = c.touched_count()
            except pkg.FspannStateError:
                return dict(never_enabled=np.array([1], np.int32))
            got = c.drain_touched(reset=True)
            assert n == len(got) and c.touched_count() == 0
            return dict(never_enabled=np.array([0], np.int32), touched=got)
        raise ValueError(kind)

    def _ticks(self, c, batches, sched, handover, dense, repeat=()):
        """fspann_tick_dev over a schedule of (encode batch, Route batch, Refine batch) per tick; every batch has buffers of its own.
        Returns 'b<i>.<key>' for every batch that was refined (or routed / coded only).  repeat: batches refined once more, in that
        order, behind the schedule (refine-only ticks with the same parameters as before)."""
        import torch
        dev = torch.device("cuda", 0)
        m = self.m
        fam = m.fam
        TD, W = fam["T"] * fam["D"], (fam["m"] * fam["lam"] + 63) // 64
        bufs = []
        for b in batches:
            nq, Bb, k = b["nq"], b.get("B", fam["B"]), b.get("k", 10)
            t = dict(q=torch.from_numpy(queries(b["qseed"], nq)).to(dev), codes=torch.zeros((nq, TD, W), dtype=torch.int64, device=dev),
                     bad=torch.full((nq,), -7, dtype=torch.int32, device=dev), sel=torch.full((nq, Bb), -1, dtype=torch.int32, device=dev),
                     selc=torch.zeros(nq, dtype=torch.int32, device=dev), ids=torch.full((nq, k), -7, dtype=torch.int32, device=dev),
                     dist=torch.zeros((nq, k), dtype=torch.float64, device=dev), count=torch.full((nq,), -7, dtype=torch.int32, device=dev),
                     scored=torch.full((nq,), -7, dtype=torch.int32, device=dev))
            if handover:
                t["hov"] = torch.zeros(max(16, c.route_handover_bytes(nq)), dtype=torch.uint8, device=dev)
            if dense:
                # the host's load + decrypt of F_q: rows packed from the reference's list, which the Route part must reproduce
                sel, _ = m.selected(b, Bb)
                t["cand"] = torch.from_numpy(np.ascontiguousarray(m.scene.X32[np.clip(sel, 0, m.scene.n - 1)])).to(dev)
            bufs.append(t)
        torch.cuda.synchronize()
        fused, lazy = [], []

        def tick(e, r, f):
            enc = rt = rf = None
            if e is not None:
                t = bufs[e]
                enc = dict(nq=batches[e]["nq"], q=t["q"].data_ptr(), codes=t["codes"].data_ptr(), bad=t["bad"].data_ptr())
            if r is not None:
                t = bufs[r]
                rt = dict(nq=batches[r]["nq"], codes=t["codes"].data_ptr(), limit=batches[r].get("B", fam["B"]), ids=t["sel"].data_ptr(), count=t["selc"].data_ptr(),
                          handover=t["hov"].data_ptr() if handover else None)
            if f is not None:
                t = bufs[f]
                rf = dict(nq=batches[f]["nq"], q=t["q"].data_ptr(), B=batches[f].get("B", fam["B"]), ids=t["sel"].data_ptr(), count=t["selc"].data_ptr(),
                          k=batches[f].get("k", 10), out_ids=t["ids"].data_ptr(), out_dist=t["dist"].data_ptr(), out_count=t["count"].data_ptr(),
                          scored=t["scored"].data_ptr(), cand=t["cand"].data_ptr() if dense else None, codes=t["codes"].data_ptr() if handover else None,
                          handover=t["hov"].data_ptr() if handover else None)
            c.tick_dev(enc, rt, rf)
            fused.append((("e" if enc else "") + ("r" if rt else "") + ("f" if rf else ""), bool(c.last_tick_fused())))
            if rt:
                lazy.append(c.last_route_info())

        out = {}

        def snapshot(j, bi):
            t = bufs[bi]
            for key in ("ids", "dist", "count", "scored", "sel", "selc", "codes", "bad"):
                v = t[key].cpu().numpy().copy()
                if key == "codes":
                    v = v.view(np.uint64)
                if key == "sel":
                    v = _mask(v, np.maximum(t["selc"].cpu().numpy(), 0), v.shape[1])
                out["b%d.%s" % (j, key)] = v

        for e, r, f in sched:
            tick(e, r, f)
        c.sync()
        for bi in range(len(batches)):
            snapshot(bi, bi)
        for j, bi in enumerate(repeat):          # an earlier parameter set again: Route of that batch, then its refine-only tick
            for key in ("ids", "count", "scored"):
                bufs[bi][key].fill_(-7)
            torch.cuda.synchronize()
            tick(None, bi, None)
            tick(None, None, bi)
            c.sync()
            snapshot(len(batches) + j, bi)
        self.info = dict(ticks=fused, route=lazy)
        return out


# ---- the runner -----------------------------------------------------------------------------------------------------------
def _fmt(op):
    return ", ".join("%s=%s" % (k, v) for k, v in op.items())


def run(ctx_factory, plan_, O, pkg=None, tmp_path=None, monkeypatch=None, stop=None, device=None):
    """Execute plan_ against a context made by ctx_factory(family name) (None: the model alone, which still computes every
    reference and counts what the oracle would leave out).  Returns dict(log, model).  stop: run only the operations before that
    index (to reproduce a failure from (seed, index)).  device: stands in for the context under test (the CPU tests of the runner)."""
    for k, v in plan_["env"].items():
        if ctx_factory is not None:
            monkeypatch.setenv(k, v)             # knobs are read when a context is created
    m = Model(O, plan_)
    dev = device if device is not None else Device(pkg, ctx_factory, m, tmp_path) if ctx_factory is not None else None
    log = []
    try:
        for i, op in enumerate(plan_["ops"][:stop]):
            entry = dict(index=i, op=op["op"], args={k: v for k, v in op.items() if k != "op"}, path=None)
            log.append(entry)
            try:
                _step(m, dev, op, entry)
            except Mismatch as e:
                lines = "\n".join("  [%d] %s(%s) -> %s" % (x["index"], x["op"], _fmt(x["args"]), x["path"]) for x in log)
                raise AssertionError("seed=%s index=%d %s(%s): %s\noperation log:\n%s" % (plan_["seed"], i, op["op"], _fmt(entry["args"]), e, lines)) from None
    finally:
        if dev is not None:
            dev.close()
    return dict(log=log, model=m)


def apply_state(m, op):
    """The model's side of a state-changing operation."""
    kind = op["op"]
    if kind == "set_deleted":
        m.last_handles = m.reached(op["reach"]) if "reach" in op else handles_of(op["hseed"], m.scene.n, op["cnt"])
        m.set_deleted(m.last_handles, op["flag"])
    elif kind == "store_set":
        m.store_set(op["row_type"])
    elif kind == "rebuild":
        m.rebuild(op["n"], op["seed"], op["idkind"])
    elif kind == "set_id_meta":
        m.set_idkind(op["idkind"])
    elif kind == "touch_enable":
        m.touch_enable(op["on"])
    elif kind == "clone":
        m.clones += 1
    elif kind == "close_clone":
        m.clones -= 1
    else:
        raise ValueError(kind)


def _step(m, dev, op, entry):
    kind = op["op"]
    if kind == "refused":
        what = op["what"]
        if dev is not None:
            dev.refused(op)
        entry["path"] = "refused:" + (op.get("call") or what)
        if what == "shared":
            return
        q = dict(via=op["via"], qseed=op["qseed"], nq=op["nq"])
        if what == "nan_query":                  # reported (bad = 1, nothing returned), not refused: the batch's other queries are served
            rows = tuple(sorted({0, op["nq"] // 2, op["nq"] - 1}))
            exp = m._expect_retry(q, 10, nan_rows=rows)
            if dev is not None:
                got = dev.query(dict(q, op="search_retry", k=10, nan_rows=rows))
                bad = exp["bad"].astype(bool)
                compare(got, exp, skip_rows=dict(sel=bad, selc=bad))      # F_q of a non-finite query: the reference has none
            m.compared += op["nq"]
            good = dict(q, op="search_retry", k=10)
        elif what == "cap_small":
            good = dict(q, op="route_bounded", limit=m.fam["B"])
        else:
            if what == "append_without_begin" and dev is not None:
                dev._build(m.scene, "append")
            good = dict(q, op="route_full", limit=m.fam["B"])
        # ... followed by the good call it imitates
        exp = m.expect(good)
        if dev is not None:
            compare(dev.query(good), exp)
        m.compared += op["nq"]
        return
    if kind in STATE_KINDS:
        apply_state(m, op)
        if dev is not None:
            dev.state(op)
        entry["path"] = "state"
        return
    exp = m.expect(op)
    nq = op.get("nq") or sum(b["nq"] for b in op.get("batches", [])) or (op["enc"]["nq"] + op["route"]["nq"] if kind == "tick_front" else 1)
    if dev is not None:
        got = dev.query(op)
        entry["path"] = dev.info
        compare(got, exp)
        if "expect_fellback" in op and dev.info["fellback"] != op["expect_fellback"]:
            raise Mismatch("%d queries fell back, the sequence was laid out for %d" % (dev.info["fellback"], op["expect_fellback"]))
        if op.get("expect_overflow"):
            ov = dev.info["overflowed"]
            if not (dev.info["lazy"] and 0 < ov <= op["nq"]):
                raise Mismatch("overflowed = %d outside (0, %d]: this call's list only, never an accumulated one (%s)" % (ov, op["nq"], dev.info))
    m.compared += nq
