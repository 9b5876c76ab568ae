"""GPU parity of imported indexes GreedyPartitioner would never cut but fspann_set_index accepts: empty partitions (runs of
equal key ranges: the replayed binary search and the gap rule), short partitions in the middle of a table, a table without
partitions (PIS:638), tables that hold only some of the ids (inv = -1 in the bounded select's first-insertion step), the
refusals of fspann_set_index, and key ranges that do not ascend (refused by fspann_finalize).

Every index goes through ctx.set_index + finalize and into a second oracle (tests/index_shapes.py, pinned by
tests/test_index_shapes_cpu.py); both selects are compared with that oracle.
"""
import numpy as np
import pytest

import index_shapes as ish

pytestmark = pytest.mark.gpu


def _imported(pkg, sc, tables, S=64, **kw):
    ctx = ish.make_ctx(pkg, sc, block_size=S, java_hash=sc["java_hash"], **kw)
    ish.import_tables(ctx, tables)
    return ctx


def _both_selects(ctx, o2, sc, decimal):
    infos = []
    for probes in (5, 10):
        _, _, inf = ish.compare_selects(ctx, o2, sc["qcodes"], probes=probes, limits=(None, 256), bounded=(17, 256),
                                        must_be_bounded=True, allow_handback=not decimal)
        infos += inf
    return infos


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("ids", ["decimal", "opaque", "deleted"])
def test_ragged_partitions(pkg, oracle, S, ids):
    """Partition sizes on both sides of one wave (S = 128), empties in front, in runs and at the end, sizes 1, S/2, S - 1, S."""
    kw = dict(decimal=dict(seed=21), opaque=dict(java_hash="opaque", seed=22), deleted=dict(deleted_frac=0.3, seed=23))[ids]
    sc = ish.scene(oracle, **kw)
    tb = ish.ragged_tables(sc, S)
    o2 = ish.oracle_for(sc, tb)
    with _imported(pkg, sc, tb, S) as ctx:
        _both_selects(ctx, o2, sc, decimal=ids != "opaque")
        for td, ix in enumerate(tb):                                  # round trip of the arrays given
            assert ish.same_tables(ctx.get_index(td), ix), td


@pytest.mark.parametrize("empty_td", [0, 3, 7])
def test_table_without_partitions(pkg, oracle, empty_td):
    sc = ish.scene(oracle, java_hash="mod5000", T=8, seed=24)
    tb = ish.uniform_tables(sc, 64)
    tb[empty_td] = ish.empty_table(1)
    o2 = ish.oracle_for(sc, tb)
    with _imported(pkg, sc, tb) as ctx:
        _both_selects(ctx, o2, sc, decimal=False)
        got = ctx.get_index(empty_td)
        assert len(got["min_key"]) == 0 and len(got["ids"]) == 0 and got["id_off"].tolist() == [0]


def test_tables_holding_some_of_the_ids(pkg, oracle):
    """Table 1 holds every second id, table 2 a random 80 %: an id's position in such a table is -1 in the inverse map the
    bounded select orders survivors of one (score, bucket) with — and with hashCodes shared by four ids such survivors exist."""
    sc = ish.scene(oracle, java_hash="mod5000", T=8, seed=24)
    tb = ish.partial_tables(sc, ish.uniform_tables(sc, 64))
    o2 = ish.oracle_for(sc, tb)
    with _imported(pkg, sc, tb) as ctx:
        infos = _both_selects(ctx, o2, sc, decimal=False)
    assert any(i["lazy"] and i["overflowed"] < ish.NQ for i in infos)


def test_ragged_import_with_hard_cap(pkg, oracle):
    sc = ish.scene(oracle, B=64, seed=25)
    tb = ish.ragged_tables(sc, 64)
    o2 = ish.oracle_for(sc, tb, hard_cap=700)
    with _imported(pkg, sc, tb, hard_cap=700) as ctx:
        count, _, infos = ish.compare_selects(ctx, o2, sc["qcodes"], limits=(None, 64), bounded=(64,))
    assert not infos[0]["lazy"]


def test_save_and_load_keep_the_shape(pkg, oracle, tmp_path):
    sc = ish.scene(oracle, seed=21)
    tb = ish.ragged_tables(sc, 128)
    o2 = ish.oracle_for(sc, tb)
    path = str(tmp_path / "ragged.fspix")
    with _imported(pkg, sc, tb, 128) as ctx:
        ctx.save_index(path)
    with ish.make_ctx(pkg, sc, block_size=128) as ctx:
        ctx.load_index(path)
        for td, ix in enumerate(tb):
            assert ish.same_tables(ctx.get_index(td), ix), td
        ish.compare_selects(ctx, o2, sc["qcodes"], limits=(None, 256), bounded=(17, 256), must_be_bounded=True)


def test_set_index_refusals(pkg, oracle):
    """Each refusal with its message; after each the context still imports and serves."""
    sc = ish.scene(oracle, seed=21)
    tb = ish.uniform_tables(sc, 64)
    o2 = ish.oracle_for(sc, tb)
    N = pkg._native
    ix = tb[2]

    def serves(ctx):
        ish.import_tables(ctx, tb)
        ish.compare_selects(ctx, o2, sc["qcodes"], limits=(256,), bounded=(256,), must_be_bounded=True)

    with ish.make_ctx(pkg, sc) as ctx:
        serves(ctx)
        # a partition of block_size + 1 ids: partitions 4 and 5 become 65 + 63
        bad = dict(ix, id_off=ix["id_off"].copy())
        bad["id_off"][5] += 1
        with pytest.raises(pkg.FspannArgumentError, match=r"partition 4 of table 2 has 65 ids \(block_size 64\)"):
            ctx.set_index(2, **bad)
        serves(ctx)
        # a negative size: id_off descends
        bad = dict(ix, id_off=ix["id_off"].copy())
        bad["id_off"][7] = bad["id_off"][6] - 1
        with pytest.raises(pkg.FspannArgumentError, match=r"partition 6 of table 2 has -1 ids"):
            ctx.set_index(2, **bad)
        serves(ctx)
        bad = dict(ix, id_off=ix["id_off"].copy())
        bad["id_off"][0] = 1
        with pytest.raises(pkg.FspannArgumentError, match=r"id_off\[0\] must be 0"):
            ctx.set_index(2, **bad)
        serves(ctx)
        # a null array with n_parts > 0 (straight through the C entry point: the Python wrapper would not pass None)
        mn, mx, rp, of, ii = (np.ascontiguousarray(ix[k]) for k in ish.ARRAYS)
        import ctypes as C
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        for hole in range(5):
            args = [ptr(a) for a in (mn, mx, rp, of, ii)]
            args[hole] = None
            rc = ctx.L.fspann_set_index(ctx.handle, 2, len(mn), *args)
            assert rc == N.E_NULL
            with pytest.raises(pkg.FspannNullError, match="index array is null"):
                N.check(rc)
        serves(ctx)
        for td in (-1, o2.TD):
            with pytest.raises(pkg.FspannArgumentError, match=r"td %d out of range \[0,%d\)" % (td, o2.TD)):
                ctx.set_index(td, **ix)
        serves(ctx)


def test_key_ranges_that_do_not_ascend_are_refused(pkg, oracle):
    """findNearestPartition is a binary search: over key ranges that do not ascend the reference itself walks wherever the
    comparisons lead, and the probe's G-ary search over the same records walks elsewhere (measured before the refusal existed,
    with every table of this scene shuffled at block size 100: the full and the bounded select each differed from the oracle's
    list on 32 of 32 queries, counts 2757..2831 against 2788..2849).  Such an import is refused by fspann_finalize, naming the
    table and the first offending partition; overlapping and equal ranges that still ascend (the ragged cut) stay accepted."""
    sc = ish.scene(oracle)
    good = ish.uniform_tables(sc, 100)
    rng = np.random.default_rng(4)
    bad = list(good)
    bad[3] = ish.shuffled(good[3], rng)
    first = int(np.flatnonzero((np.diff(bad[3]["min_key"]) < 0) | (np.diff(bad[3]["max_key"]) < 0))[0]) + 1
    o2 = ish.oracle_for(sc, good)
    with ish.make_ctx(pkg, sc, block_size=100) as ctx:
        for td, ix in enumerate(bad):
            ctx.set_index(td, **ix)                                   # set_index sees one table: the order is finalize's to judge
        with pytest.raises(pkg.FspannArgumentError, match=r"table 3: key range of partition %d does not ascend" % first):
            ctx.finalize()
        with pytest.raises(pkg.FspannStateError):                     # not frozen: no Route
            ctx.route(sc["qcodes"], limit=100)
        # minKey > maxKey inside one partition is the same refusal
        worse = dict(good[3], min_key=good[3]["min_key"].copy())
        worse["min_key"][9] = worse["max_key"][9] + 1
        ctx.set_index(3, **worse)
        with pytest.raises(pkg.FspannArgumentError, match=r"table 3: key range of partition 9 does not ascend"):
            ctx.finalize()
        ctx.set_index(3, **good[3])                                   # the corrected import serves
        ctx.finalize()
        ish.compare_selects(ctx, o2, sc["qcodes"], limits=(None, 256), bounded=(256,), must_be_bounded=True)
        ragged = ish.ragged_tables(sc, 100)                           # equal and overlapping ranges ascend: accepted
        assert all((np.diff(ix["min_key"]) == 0).any() and ish.ascends(ix) for ix in ragged)
        ish.import_tables(ctx, ragged)
        ish.compare_selects(ctx, ish.oracle_for(sc, ragged), sc["qcodes"], limits=(None,), bounded=(256,), must_be_bounded=True)
    # a saved file cannot hold such a table (save needs a finalized index), so fspann_index_load meets it only in a file
    # written by someone else: the load goes through the same fspann_finalize
