"""GPU parity at block sizes other than the reference's constant 64: Setup's cut and both Route selects against the oracle.

The oracle builds at 64 only; tests/index_shapes.py restates GreedyPartitioner's cut at any block size (pinned to the oracle
at 64 by tests/test_index_shapes_cpu.py) and a second oracle imports the re-cut tables.  Pinned here, none of it reachable
at S = 64: build_cut_kernel's `i % S`, `mid` and last-block logic, the division path of FSP_TS (S not a power of two), the
SP = ceil(S / 64) piece loops (S > 64) and their magic-multiply division with the arena in global memory, the bounded
select's whole-partition path, bin16 rows of 16 and 128 entries, and HARD_CAP reached inside a partition that is not 64 wide.

Mutation check (scratch builds of the library, nothing of them kept; every mutant stays in bounds by construction).  Run
against the new tests (this file, tests/test_gpu_import_shapes.py, the oracle half of test_bounded_select_other_block_sizes)
and against the Route / Setup files of the suite as it was before them (route_edges in its earlier form, route_fuzz,
index_file, search_call, golden, parity, boundary, small_calls, baseline_shapes, row_codec, dtype_dispatch, tick: 182 tests):
  1. build_cut_kernel: max_key from keys[min(i + 64, n) - 1], a constant 64 in place of S (an index in [i, n) either
     way).  Red: test_build_cut at all nine sizes, _one_partition, _two_code_words, _with_a_given_order (not
     _on_the_host: the host cut is other code) and the Route tests over such an index.  Earlier files: green.
  2. FSP_TS, division path only: the last probe step's tuples are given to the step before it (TP - 2 >= 0, so inside
     [0, TP)).  Red: test_route_both_selects[63, 65, 100], test_route_blocks_of_1000, test_deleted_ids,
     test_opaque_hash_codes[100], test_global_arena_with_pieces[100].  Earlier files: test_bounded_select_other_block_sizes[100]
     red as well — FSP_TS belongs to the full select alone, so the earlier full-against-bounded comparison sees this one.
  3. Staging of the full select drops positions >= 64 of a partition (pos < min(pr.w, 64): fewer loads).  Red: every Route
     test here at S in 65, 100, 128, 1000 and the ragged imports at 128.  Earlier files: [100] and [128] of the same earlier
     test red as well, for the same reason.
  3b. The same mistake where both selects share it: the host's partition record carries min(size, 64) (fewer loads).
     Red: the tests of 3 and test_front_launch[128-200], test_search_store_dev_at_100.  Earlier files: [100] and [128] of that
     test red again — the bounded select reads a partition's prefix in bucket order, the full select in position order, so
     the two lose different ids: for partitions wider than a wave the earlier comparison is stronger than it looks.
  4. The host's partition record of an empty partition repeats its predecessor's offset and size (a valid id range of the
     same table).  Red: test_ragged_partitions (all six), test_ragged_import_with_hard_cap, test_save_and_load_keep_the_shape and
     the accepted ragged import of test_key_ranges_that_do_not_ascend_are_refused.  Earlier files: green (no earlier
     test imports an empty partition).
Mutants 1 and 4 can only show at a block size other than 64 or with an empty partition; the earlier suite has neither outside
the files named above.
"""
import numpy as np
import pytest

import index_shapes as ish

pytestmark = pytest.mark.gpu
K = 10


def _built(pkg, sc, S, **kw):
    ctx = ish.make_ctx(pkg, sc, block_size=S, java_hash=sc["java_hash"], **kw)
    ctx.build_index(sc["X"], order=sc["order"])
    return ctx


def _check_cut(ctx, sc, S):
    n = sc["params"]["n"]
    for td, want in enumerate(ish.uniform_tables(sc, S)):
        got = ctx.get_index(td)
        for k in ish.ARRAYS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (S, td, k)
        assert len(want["min_key"]) == (n + S - 1) // S


# ---- Setup ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 16, 63, 65, 100, 128, 1000, 1024])
def test_build_cut(pkg, oracle, S):
    """20 000 is a multiple of 16, 100 and 1000 and of none of the others: full and short last partitions."""
    sc = ish.scene(oracle)
    with _built(pkg, sc, S) as ctx:
        _check_cut(ctx, sc, S)


@pytest.mark.parametrize("n,S", [(700, 1024), (128, 128)])
def test_build_cut_one_partition(pkg, oracle, n, S):
    sc = ish.scene(oracle, n=n, B=64, seed=13)
    with _built(pkg, sc, S) as ctx:
        _check_cut(ctx, sc, S)
        assert len(ctx.get_index(0)["min_key"]) == 1


def test_build_cut_two_code_words(pkg, oracle):
    sc = ish.scene(oracle, d=20, T=2, D=2, m=40, lam=3, seed=14)
    assert sc["oracle"].W == 2
    with _built(pkg, sc, 100) as ctx:
        _check_cut(ctx, sc, 100)


@pytest.mark.parametrize("S", [16, 100])
def test_build_cut_on_the_host(pkg, oracle, S, monkeypatch):
    monkeypatch.setenv("FSPANN_GPU_CUT", "0")
    sc = ish.scene(oracle)
    with _built(pkg, sc, S) as ctx:
        _check_cut(ctx, sc, S)


def test_build_cut_with_a_given_order(pkg, oracle):
    sc = ish.scene(oracle, order="permuted", seed=15)
    with _built(pkg, sc, 100) as ctx:
        _check_cut(ctx, sc, 100)


# ---- Route ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 16, 63, 65, 100, 128])
def test_route_both_selects(pkg, oracle, S):
    """Full select with counters at unlimited limit and below the list length, then the bounded select (planned, run, no
    query handed back: decimal ids) — each against the oracle, not against each other."""
    sc = ish.scene(oracle)
    o2 = ish.oracle_for(sc, ish.uniform_tables(sc, S))
    with _built(pkg, sc, S) as ctx:
        ish.compare_selects(ctx, o2, sc["qcodes"], limits=ish.FULL_LIMITS[S], bounded=ish.BOUNDED_LIMITS[S], must_be_bounded=True)


@pytest.mark.parametrize("probes", [10, 20])
def test_route_more_probes(pkg, oracle, probes):
    sc = ish.scene(oracle)
    o2 = ish.oracle_for(sc, ish.uniform_tables(sc, 16))
    with _built(pkg, sc, 16) as ctx:
        ish.compare_selects(ctx, o2, sc["qcodes"], probes=probes, limits=(None, 257), bounded=(17, 256, 257, 512), must_be_bounded=True)


def test_route_blocks_of_1000(pkg, oracle):
    sc = ish.scene(oracle)
    o2 = ish.oracle_for(sc, ish.uniform_tables(sc, 1000), hard_cap=40000)
    with _built(pkg, sc, 1000, hard_cap=40000) as ctx:
        ish.compare_selects(ctx, o2, sc["qcodes"], limits=(None, 5000, 257), bounded=(256,))


def test_bounded_select_size_classes_at_128(pkg, oracle):
    sc = ish.scene(oracle, nq=24, **ish.SIZE_CLASSES)
    o2 = ish.oracle_for(sc, ish.uniform_tables(sc, 128))
    with _built(pkg, sc, 128) as ctx:
        ish.compare_selects(ctx, o2, sc["qcodes"], limits=(1024,), bounded=(256, 257, 512, 513, 1024), must_be_bounded=True)


@pytest.mark.parametrize("S,cap", ish.HARD_CAPS)
def test_hard_cap_inside_a_partition(pkg, oracle, S, cap):
    """The cap is reached inside a partition, the partition is finished (PIS:657-659): counts in [cap, cap - 1 + S].  The
    bounded select is not legal once the cap can bind: route mode 2 must fall to the full select, as planned."""
    sc = ish.scene(oracle, **ish.HARD_CAP_SCENE)
    o2 = ish.oracle_for(sc, ish.uniform_tables(sc, S), hard_cap=cap)
    with _built(pkg, sc, S, hard_cap=cap) as ctx:
        _, _, infos = ish.compare_selects(ctx, o2, sc["qcodes"], limits=(None, 64, 17), bounded=(64, 17))
    assert not any(i["lazy"] for i in infos)


def test_deleted_ids(pkg, oracle):
    sc = ish.scene(oracle, deleted_frac=0.3, seed=11)
    o2 = ish.oracle_for(sc, ish.uniform_tables(sc, 100))
    with _built(pkg, sc, 100) as ctx:
        ish.compare_selects(ctx, o2, sc["qcodes"], limits=(None, 257), bounded=(17, 256, 1024), must_be_bounded=True)


@pytest.mark.parametrize("S", [16, 100])
def test_opaque_hash_codes(pkg, oracle, S):
    """Caller-given String.hashCodes: the bounded select runs its exact treeify check over bin16 rows of 16 / 128 entries."""
    sc = ish.scene(oracle, java_hash="opaque", seed=12)
    o2 = ish.oracle_for(sc, ish.uniform_tables(sc, S))
    with _built(pkg, sc, S) as ctx:
        ish.compare_selects(ctx, o2, sc["qcodes"], limits=(None, 257), bounded=ish.BOUNDED_LIMITS[S][:3], must_be_bounded=True,
                            allow_handback=True)
        assert ctx.unmodelled_queries() == 0


@pytest.mark.parametrize("S", [128, 100])
def test_global_arena_with_pieces(pkg, oracle, S):
    """10 x 4 tables x 20 probes x S ids: the per-query scratch lives in global memory and a partition is two 64-lane
    pieces (S = 100: through the division path of the tuple index as well), then the same with HARD_CAP cutting inside."""
    sc = ish.scene(oracle, nq=6, **ish.ARENA)
    tb = ish.uniform_tables(sc, S)
    for cap in (60000, 9000):
        o2 = ish.oracle_for(sc, tb, hard_cap=cap)
        with _built(pkg, sc, S, hard_cap=cap) as ctx:
            assert ctx.route_plan_info(20, 2**31 - 1, True)["lds_mode"] == 0
            assert ctx.route_plan_info(20, 2**31 - 1, True)["max_tuples"] == 40 * 20 * S
            ish.compare_selects(ctx, o2, sc["qcodes"], probes=20, limits=(None, 512))


# ---- whole calls ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,B", [(16, 100), (128, 200)])
def test_front_launch(pkg, oracle, S, B):
    """fspann_tick_dev with encode + Route and no Refine (one launch) at block_size = S: codes and routed lists = the oracle's."""
    import torch
    sc = ish.scene(oracle, nq=64, B=B, seed=16)
    p = sc["params"]
    o2 = ish.oracle_for(sc, ish.uniform_tables(sc, S))
    nq, TD, W = 64, p["T"] * p["D"], 1
    dev = torch.device("cuda", 0)
    Qa = np.random.default_rng(17).standard_normal((nq, p["d"])).astype(np.float32)
    ref_b = o2.search(sc["Q"].astype(np.float64), K)
    assert not o2.unmodelled
    with _built(pkg, sc, S) as ctx:
        qa = torch.from_numpy(Qa).to(dev)
        codes_a = torch.zeros((nq, TD, W), dtype=torch.int64, device=dev)
        codes_b = torch.from_numpy(sc["qcodes"].view(np.int64)).to(dev)
        bad = torch.zeros(nq, dtype=torch.int32, device=dev)
        sel = torch.full((nq, B), -1, dtype=torch.int32, device=dev)
        cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
        ctx.tick_dev(encode=dict(nq=nq, q=qa.data_ptr(), codes=codes_a.data_ptr(), bad=bad.data_ptr()),
                     route=dict(nq=nq, codes=codes_b.data_ptr(), limit=B, ids=sel.data_ptr(), count=cnt.data_ptr()), refine=None)
        ctx.sync()
        assert ctx.last_tick_fused() and ctx.last_route_info()["lazy"]
        assert np.array_equal(codes_a.cpu().numpy().view(np.uint64), o2.encode(Qa.astype(np.float64))) and not bad.cpu().numpy().any()
        c_h, s_h = cnt.cpu().numpy(), sel.cpu().numpy()
    assert np.array_equal(c_h, ref_b["sel_count"]) and (c_h == B).all()
    assert np.array_equal(np.where(np.arange(B)[None] < c_h[:, None], s_h, -1), ref_b["sel"][:, :B])


def test_search_store_dev_at_100(pkg, oracle):
    """One fspann_search_store_dev (encode -> Route -> Refine from the store) at block_size = 100 against the oracle's search."""
    import torch
    sc = ish.scene(oracle, nq=37, B=128, seed=18)
    p = sc["params"]
    nq, B = 37, p["B"]
    o2 = ish.oracle_for(sc, ish.uniform_tables(sc, 100))
    ref = o2.search(sc["Q"].astype(np.float64), K, codes=sc["qcodes"])
    assert not o2.unmodelled and not ref["metrics"][:, 4].any()
    with _built(pkg, sc, 100) as ctx:
        ctx.store_set(sc["X"])
        dev = torch.device("cuda", 0)
        qd = torch.from_numpy(sc["Q"]).to(dev)
        out_ids = torch.full((nq, K), -7, dtype=torch.int32, device=dev)
        out_dist = torch.zeros((nq, K), dtype=torch.float64, device=dev)
        out_cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
        scored = torch.zeros(nq, dtype=torch.int32, device=dev)
        sel = torch.full((nq, B), -1, dtype=torch.int32, device=dev)
        selc = torch.zeros(nq, dtype=torch.int32, device=dev)
        ctx.search_store_dev(nq, qd.data_ptr(), pkg._native.F32, -1, B, K, out_ids.data_ptr(), out_dist.data_ptr(), out_cnt.data_ptr(),
                             scored.data_ptr(), sel.data_ptr(), selc.data_ptr())
        ctx.sync()
        got = [t.cpu().numpy() for t in (out_ids, out_dist, out_cnt, scored, sel, selc)]
    assert np.array_equal(got[5], ref["sel_count"])
    assert np.array_equal(np.where(np.arange(B)[None] < got[5][:, None], got[4], -1), ref["sel"][:, :B])
    assert np.array_equal(got[0], ref["ids"]) and np.array_equal(got[1], ref["dist"]) and np.array_equal(got[2], ref["count"])
    assert np.array_equal(got[3], ref["metrics"][:, 2])
