"""CPU: the model of one long-lived context (tests/ctx_model.py) on its own — what the plans contain, that the reference side of
every default plan and named sequence is fully modelled (no treeified query, nothing left out), that the comparator notices the
smallest deviation in every output of every query operation, and that the model's incrementally updated oracle agrees with one
built afresh from the scene."""
import copy
import types

import numpy as np
import pytest

import ctx_model as M

SEEDS = range(12)


@pytest.fixture(scope="module")
def plans():
    return [M.plan(s) for s in SEEDS]


# ---- plan coverage: conditions on the generator -------------------------------------------------------------------------------
def test_plans_are_pure_and_repeatable(plans):
    assert [M.plan(s) for s in SEEDS] == plans
    assert all(30 <= len(p["ops"]) <= 40 for p in plans), [len(p["ops"]) for p in plans]


def test_every_operation_kind_at_least_three_times(plans):
    count = {}
    for p in plans:
        for op in p["ops"]:
            count[op["op"]] = count.get(op["op"], 0) + 1
            if op["op"] == "refused":
                key = "refused:" + (op["what"] if op["what"] != "shared" else "shared")
                count[key] = count.get(key, 0) + 1
            if op["op"] == "rebuild":
                count["rebuild:" + op["route"]] = count.get("rebuild:" + op["route"], 0) + 1
    want = list(M.QUERY_KINDS + M.STATE_KINDS) + ["refused:" + w for w in M.REFUSALS + ("shared",)] + ["rebuild:" + r for r in M.BUILD_ROUTES]
    assert {k: count.get(k, 0) for k in want if count.get(k, 0) < 3} == {}
    sizes = {op["nq"] for p in plans for op in p["ops"] if op["op"] in ("route_full", "route_bounded", "encode")}
    assert sizes == set(M.BATCHES)
    assert {op["limit"] for p in plans for op in p["ops"] if op["op"] == "route_bounded"} == set(M.BOUNDED_LIMITS)
    assert {p["init"]["fam"] for p in plans} == set(M.FAMILIES) and any(p["env"] for p in plans) and not all(p["env"] for p in plans)


def test_every_state_change_is_followed_by_both_selects_and_a_search(plans):
    for p in plans:
        ops = p["ops"]
        idx = [i for i, op in enumerate(ops) if op["op"] in M.STATE_KINDS]
        for a, b in zip(idx, idx[1:] + [len(ops)]):
            kinds = {op["op"] for op in ops[a + 1:b]}
            assert {"route_full", "route_bounded"} <= kinds and kinds & set(M.SEARCH_KINDS), (p["seed"], a, ops[a])


def test_sizes_store_types_and_clones(plans):
    smaller = larger = 0
    types_seen = {p["init"]["store"] for p in plans}
    shared = 0
    for p in plans:
        n, clones = p["init"]["n"], 0
        for op in p["ops"]:
            if op["op"] == "rebuild":
                smaller += op["n"] < n
                larger += op["n"] > n
                n = op["n"]
            elif op["op"] == "store_set":
                types_seen.add(op["row_type"])
            elif op["op"] == "clone":
                clones += 1
            elif op["op"] == "close_clone":
                clones -= 1
            elif op["op"] == "refused" and op["what"] == "shared":
                assert clones > 0
                shared += 1
            assert 0 <= clones <= 2
            if clones:
                assert op["op"] not in ("store_set", "rebuild", "set_id_meta")
    assert smaller >= 3 and larger >= 3 and types_seen == set(M.ROW_TYPES) and shared >= 3
    named = M.named_plans()
    assert [op["n"] for op in named["rebuild-load"]["ops"] if op["op"] == "rebuild"] == [300, 3000] and named["rebuild-load"]["init"]["n"] == 40000


# ---- the reference side ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_runs(oracle, plans):
    return [M.run(None, p, oracle) for p in plans + list(M.named_plans().values())]


def test_reference_side_is_fully_modelled(reference_runs):
    """No HashMap of any scene treeifies (the model asserts `unmodelled` false at every Route reference) and no query is left out of a
    comparison: the cap is 0."""
    for r in reference_runs:
        m = r["model"]
        assert not m.scene.o.unmodelled and m.treeified == 0
        assert m.compared > 0 and all(e["path"] is not None or e["op"] in M.QUERY_KINDS + ("tick_redo",) for e in r["log"])


# ---- the comparator is not vacuous ---------------------------------------------------------------------------------------------------
def _ops_of_every_kind():
    q = dict(qseed=5, nq=7)
    return [dict(op="encode", dtype="f32", mode=1, **q), dict(op="route_full", limit=None, **q), dict(op="route_full", limit=256, **q),
            dict(op="route_bounded", limit=17, **q), dict(op="refine_store", k=10, **q), dict(op="refine_dense", k=10, **q),
            dict(op="search_store", k=10, **q), dict(op="search_retry", k=10, **q), dict(op="search_fallback", k=10, **q),
            dict(op="tick_front", enc=q, route=dict(qseed=6, nq=7)), dict(op="tick_refine", k=10, handover=True, dense=False, **q),
            dict(op="tick_all", batches=[q, dict(qseed=6, nq=7), dict(qseed=7, nq=7)], k=10, handover=False, dense=False),
            dict(op="tick_redo", batches=[dict(q, B=64, k=1), dict(qseed=6, nq=7, B=256, k=10)], repeat=(0,)),
            dict(op="groundtruth", k=5, **q), dict(op="touched_check")]


def _perturb(a, row):
    """the smallest change of one element of row `row`: an id / count off by one, a distance one ulp away, one code bit"""
    a = a.copy()
    i = (row,) + (0,) * (a.ndim - 1)
    if a.dtype.kind == "f":
        a[i] = np.nextafter(a[i], np.inf)
    elif a.dtype.kind == "u":
        a[i] ^= np.uint64(1)
    else:
        a[i] += 1
    return a


def test_comparator_notices_the_smallest_deviation(oracle):
    m = M.Model(oracle, dict(init=M.initial("spec", 3000, 3, touch=True), env={}))
    checked = 0
    for op in _ops_of_every_kind():
        exp = m.expect(op)
        M.compare(copy.deepcopy(exp), exp)                     # (equal outputs pass)
        for key, v in exp.items():
            if key == "touched":
                assert len(v) > 100
                with pytest.raises(M.Mismatch, match=r"handles missing \[%d\]" % v[40]):
                    M.compare(dict(exp, touched=np.delete(v, 40)), exp)
                with pytest.raises(M.Mismatch, match="unexpected"):
                    M.compare(dict(exp, touched=np.sort(np.append(v, [2999 if 2999 not in v else 2998]))), exp)
                checked += 2
                continue
            row = len(v) // 2
            with pytest.raises(M.Mismatch, match=r"%s differs: first differing query %d " % (key.replace(".", r"\."), row)):
                M.compare(dict(exp, **{key: _perturb(v, row)}), exp)
            checked += 1
            if key.endswith("ids") and v.ndim == 2 and v.shape[1] > 1 and v[row, 0] != v[row, 1]:
                swapped = v.copy()
                swapped[row, [0, 1]] = swapped[row, [1, 0]]                # one id swapped with its neighbour in one query
                with pytest.raises(M.Mismatch, match=r"first differing query %d " % row):
                    M.compare(dict(exp, **{key: swapped}), exp)
                checked += 1
        with pytest.raises(M.Mismatch, match="missing"):
            M.compare({}, exp)
    assert checked > 80


class EchoDevice:
    """Stands in for a context: a second model in lockstep answers every operation — a correct device — except that the answer
    to operation `at` deviates by `change`."""
    info = dict(lazy=True, overflowed=1)

    def __init__(self, O, plan, at, change):
        self.m, self.plan, self.at, self.change = M.Model(O, plan), plan, at, change

    def close(self):
        pass

    def state(self, op):
        M.apply_state(self.m, op)

    def refused(self, op):
        pass

    def _build(self, scene, route):
        pass

    def query(self, op):
        if "nan_rows" in op:
            return self.m._expect_retry(op, op["k"], nan_rows=op["nan_rows"])
        e = self.m.expect(op)
        if self.at is not None and op is self.plan["ops"][self.at]:
            e = self.change(e)
        return e


def test_run_names_seed_index_query_and_log(oracle):
    """The runner end to end against a stand-in device: a correct one passes every default plan; a count off by one in the middle of
    a plan fails with the seed, the index, the first differing query and the log up to that point — and stop= reproduces it."""
    for s in (0, 5):
        p = M.plan(s)
        res = M.run(None, p, oracle, device=EchoDevice(oracle, p, None, None))
        assert [e["index"] for e in res["log"]] == list(range(len(p["ops"])))
    p = M.plan(0)
    idx = next(i for i, op in enumerate(p["ops"]) if op["op"] in M.SEARCH_KINDS and i > 10)
    row = p["ops"][idx]["nq"] - 1
    change = lambda e: dict(e, count=_perturb(e["count"], row))
    with pytest.raises(AssertionError) as ei:
        M.run(None, p, oracle, device=EchoDevice(oracle, p, idx, change))
    msg = str(ei.value)
    assert ("seed=0 index=%d %s(" % (idx, p["ops"][idx]["op"])) in msg and ("count differs: first differing query %d " % row) in msg and "operation log:" in msg
    assert msg.count("\n  [") == idx + 1
    with pytest.raises(AssertionError, match="seed=0 index=%d " % idx):
        M.run(None, p, oracle, device=EchoDevice(oracle, p, idx, change), stop=idx + 1)
    M.run(None, p, oracle, device=EchoDevice(oracle, p, idx, change), stop=idx)


# ---- model self-consistency ----------------------------------------------------------------------------------------------------------
def _routes_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_model_agrees_with_a_freshly_built_oracle(oracle):
    """After deletes, un-deletes, an id metadata change and back, and a rebuild, the model's incrementally updated oracle answers
    what an oracle built afresh from the scene's inputs answers; a delete forgotten in the model is noticed."""
    m = M.Model(oracle, dict(init=M.initial("eight", 3000, 11), env={}))
    q = dict(qseed=9, nq=33)
    for step in (lambda: m.set_deleted(M.handles_of(1, 3000, 60), True), lambda: m.set_idkind("opaque"), lambda: m.set_deleted(M.handles_of(2, 3000, 60), True),
                 lambda: m.set_deleted(M.handles_of(1, 3000, 60), False), lambda: m.set_idkind("decimal"), lambda: m.rebuild(300, 12, "opaque"),
                 lambda: m.set_deleted(M.handles_of(3, 300, 5), True)):
        before = m.routed(q)
        step()
        after = m.routed(q)
        assert not _routes_equal(before, after)                # every one of these changes an answer: the cache must not serve the old one
        fresh = m.scene.fresh_oracle()
        c = m.codes(q)
        assert _routes_equal(fresh.route(c), after)
        ref = m.searched(q, 10)
        got = fresh.search(M.queries(9, 33).astype(np.float64), 10, codes=c)
        assert all(np.array_equal(ref[k], got[k]) for k in ref)
    # a delete the model forgets (the flags change, its oracle is not told): a fresh oracle disagrees
    ids, _, count, _ = m.routed(q)
    m.scene.deleted[ids[0, 0]] = 1
    assert not _routes_equal(m.scene.fresh_oracle().route(m.codes(q)), m.scene.o.route(m.codes(q)))


def test_store_type_switch_in_the_model(oracle):
    """All five row types hold the scene's rows exactly (the oracle's answer cannot depend on the store's type); what does depend
    on it — the ground truth over an FSPANN_F64 store is refused — follows the model's store type, so a switch that is not applied
    is noticed."""
    pkg = types.SimpleNamespace(bfloat16="bf16-marker")
    m = M.Model(oracle, dict(init=M.initial("four", 300, 13, store="f32"), env={}))
    for t in M.ROW_TYPES:
        rows, _ = M.typed_rows(pkg, m.scene.X, t)
        assert np.array_equal(rows.astype(np.float64), m.scene.X)
        if t == "bf16":
            assert not (rows.view(np.uint32) & 0xFFFF).any()   # exact as bfloat16: the low 16 bits of every fp32 pattern are zero
    op = dict(op="groundtruth", qseed=1, nq=7, k=5)
    as_f32 = m.expect(op)
    m.store_set("f64")
    as_f64 = m.expect(op)
    assert as_f32["refused"][0] == 0 and as_f64["refused"][0] == 1
    with pytest.raises(M.Mismatch):
        M.compare(as_f64, as_f32)                              # the device switched, the model did not
    m.store_set("i8")
    assert all(np.array_equal(m.expect(op)[k], as_f32[k]) for k in as_f32)
