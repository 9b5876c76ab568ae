"""GPU: random and named call SEQUENCES on one long-lived context (and its clones) against the CPU oracle.

Every other GPU test builds a scene, makes a fresh context, runs one kind of call and compares.  Here one context lives through a
whole sequence of calls of changing kinds and sizes — rebuilds on the frozen context, store replacements, id metadata changes,
deletes through owner and clones, refused calls — and every query operation in between is compared bit for bit with the oracle for
the scene as it is at that moment (tests/ctx_model.py: scenes, plans, expectations, runner).  What a context carries from call to
call is what these sequences reach: the scratch arenas, the pinned block, the overflow counters' turn, the redo-parameter slots,
epochs and dirty flags, the state an owner shares with its clones.

A failure names (seed, index): ctx_model.run(..., stop=index + 1) on the same plan reproduces it."""
import os

import pytest

import ctx_model as M

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get("FSPANN_FUZZ_SEEDS", "12"))     # FSPANN_FUZZ_SEEDS=100 for a long run
LOGS = {}            # seed / name -> operation log of every sequence that ran
NAMED = M.named_plans()


def _run(pkg, oracle, plan, tmp_path, monkeypatch):
    res = M.run(lambda fam: pkg.FspannContext(M.make_cfg(pkg, fam), 0), plan, oracle, pkg=pkg, tmp_path=tmp_path, monkeypatch=monkeypatch)
    LOGS[plan["seed"]] = res["log"]
    assert res["model"].treeified == 0
    return res


def _paths(log, kind):
    return [e["path"] for e in log if e["op"] == kind and isinstance(e["path"], dict)]


@pytest.mark.parametrize("route", M.BUILD_ROUTES)
def test_rebuild_on_a_frozen_context(pkg, oracle, route, tmp_path, monkeypatch):
    """Build, serve through every query operation, rebuild with fewer rows (40000 -> 300), serve, rebuild with more (-> 3000), serve:
    by fspann_build_index, by begin / ragged appends / finish, by set_index of the oracle's tables + finalize, by load_index of a
    file another context saved."""
    res = _run(pkg, oracle, NAMED["rebuild-" + route], tmp_path, monkeypatch)
    assert all(p["lazy"] for p in _paths(res["log"], "route_bounded"))


def test_id_metadata_changes_and_back(pkg, oracle, tmp_path, monkeypatch):
    """Decimal ids -> opaque hashCodes -> decimal ids -> opaque: both selects after each finalize; a Route call between set_id_meta
    and the finalize is refused ("not finalized")."""
    _run(pkg, oracle, NAMED["id-meta"], tmp_path, monkeypatch)


def test_store_replaced_by_every_row_type(pkg, oracle, tmp_path, monkeypatch):
    """F64 -> I8 -> F16 -> BF16 -> F32 -> F64 -> I8 over the same integer rows: refine_store, search_store_dev and the store-row tick
    give the oracle's (identical) outputs every time, the ground truth over the store follows the type (refused over F64), and so
    does the touched set."""
    _run(pkg, oracle, NAMED["store-type"], tmp_path, monkeypatch)


@pytest.mark.parametrize("fam", ["spec", "eight"])
def test_batch_sizes_up_and_down(pkg, oracle, fam, tmp_path, monkeypatch):
    """600 -> 1 -> 200 -> 2 -> 600 through each entry point on one context: arenas grow, are reused smaller and grow again, the
    zero-copy path and the copy path alternate.  16 x 1 / B = 256 (fused ticks) and 4 x 2 / B = 300 (stand-alone kernels)."""
    _run(pkg, oracle, NAMED["batch-sizes-" + fam], tmp_path, monkeypatch)


def test_size_classes_with_hand_overs(pkg, oracle, tmp_path, monkeypatch):
    """FSPANN_ROUTE_LAZY_CAP=258: consecutive bounded-select calls in the 512 / 1024 / 2048-entry classes, interleaved with
    search_store_dev, search_retry_dev and front-launch ticks.  Every call's `overflowed` is within (0, nq]: its own list."""
    res = _run(pkg, oracle, NAMED["size-classes"], tmp_path, monkeypatch)
    paths = _paths(res["log"], "route_bounded")
    assert len(paths) == 10 and all(p["lazy"] and p["overflowed"] > 0 for p in paths), paths


def test_redo_parameter_slots_wrap(pkg, oracle, tmp_path, monkeypatch):
    """Eleven consecutive refine-only ticks with a hand-over buffer and differing (nq, B, k, buffers), then three earlier parameter
    sets again: the eight redo-parameter slots wrap and are found again."""
    res = _run(pkg, oracle, NAMED["redo-slots"], tmp_path, monkeypatch)
    p = _paths(res["log"], "tick_redo")[0]
    assert sum(1 for kind, _ in p["ticks"] if kind == "f") == 14
    assert any(r["lazy"] and r["overflowed"] > 0 for r in p["route"]), p["route"]     # queries really were handed over to the refine role


def test_failed_calls_leave_nothing_behind(pkg, oracle, tmp_path, monkeypatch):
    """A NaN query, limit = 0, a cap below min(limit, worst case), build_append without build_begin, nq = 0: each followed by the
    good call it imitates and by both selects."""
    _run(pkg, oracle, NAMED["failed-calls"], tmp_path, monkeypatch)


def test_fallback_after_deletes_on_the_serving_context(pkg, oracle, tmp_path, monkeypatch):
    """set_deleted of everything two queries reach: search_fallback_dev answers them from its second search (exactly two fall back), the
    touched set holds both searches' rows; the deletes taken back, nobody falls back any more."""
    _run(pkg, oracle, NAMED["fallback-after-deletes"], tmp_path, monkeypatch)


def test_owner_and_two_clones(pkg, oracle, tmp_path, monkeypatch):
    """Two clones, interleaved queries, deletes through either, a clone made between deletes, every state change refused ("shared
    with") with the next query still right, clones closed, state changes accepted, serve."""
    _run(pkg, oracle, NAMED["owner-and-clones"], tmp_path, monkeypatch)


@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_random_sequence(pkg, oracle, seed, tmp_path, monkeypatch):
    _run(pkg, oracle, M.plan(seed), tmp_path, monkeypatch)


def test_zz_sequences_reached_the_paths():
    """From the logs of the seeded sequences: the bounded select really ran, queries were handed over, a fused tick and a stand-alone
    tick ran, the small zero-copy path was used, and an arena grew after having been used smaller."""
    logs = [LOGS[s] for s in range(12) if s in LOGS]
    if len(logs) < 12:
        return              # (only part of the default seeds ran in this session: nothing to conclude)
    route = [p for log in logs for p in _paths(log, "route_bounded")]
    assert sum(1 for p in route if p["lazy"]) >= 10
    assert any(p["lazy"] and p["overflowed"] > 0 for p in route)
    ticks = [t for log in logs for k in ("tick_all", "tick_refine") for p in _paths(log, k) for t in p["ticks"] if "f" in t[0]]
    assert any(f for _, f in ticks) and not all(f for _, f in ticks)
    assert any(p.get("zero_copy") for log in logs for k in ("encode", "route_full", "route_bounded") for p in _paths(log, k))
    grew = 0
    for log in logs:
        for kind in M.QUERY_KINDS:
            nqs = [e["args"]["nq"] for e in log if e["op"] == kind and "nq" in e["args"]]
            grew += any(b > a and any(c < a for c in nqs[i + 1:j]) for i, a in enumerate(nqs) for j, b in enumerate(nqs) if j > i + 1)
    assert grew >= 3
