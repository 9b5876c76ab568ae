"""Setup's radix sort (csrc/build.hip.h: rs_hist_kernel, rs_scan_kernel, rs_scatter_kernel, driven by build_finish_impl) at its own
edges: tile, wave and round borders, the number of passes of the bin sort and of the key sort, more than 256 tiles, more than one
upload chunk, the incremental build.  Every test builds on the GPU and compares all five arrays of every table with the oracle's
build_index (a literal HashMap iteration and a stable sort), after asserting that no bin of the oracle's staging map treeified:
with a tree bin the library takes the iteration order from its host model and the bin sort never runs.

Decimal ids treeify no bin at any n used here (asserted in every test), so only test_one_key's second half gives hashCodes of its own.

Confirmed on the oracle's HashMap model (and asserted in test_bin_sort_pass_count): HashMap<>(n) ends after n puts with a table
of 256 at n = 192, 512 at 193, 65 536 at 49 152 and 131 072 at 49 153: one, two, two and three passes of the bin sort.

Wall time on an MI355X (pytest --durations=0, call phase): the whole file 2.4 s, 1.2 s of it the session's package fixture.
test_many_tiles_and_upload_chunks 0.12 s (524 288), 0.14 s (524 289, two tables), 0.09 s (262 145, GPU and host cut); the first
test run 0.20 s (it loads the library); test_bin_sort_pass_count 0.02 s at 49 152 / 49 153; every other case 0.01 s or less.

Mutation check (scratch builds of the library, nothing of them kept).  Every mutant stays in bounds by construction: 1 and 2 only
lower a scatter destination (never below 0), 3 to 5 only leave passes out.  1 and 2 leave destinations unwritten, so their builds
also clear the sort's four key / payload buffers first: every payload a later kernel indexes with is then 0 or one written before,
a position in [0, n) — the suggested mutants alone would have read through whatever the scratch held.  Each ran once against this
file and once against the earlier Setup files (parity, boundary, block_sizes, treeify, import_shapes without fullsize: 119 tests).
  1. rs_scan_kernel: `carry` not advanced after a chunk of 256 tiles.  Red: test_many_tiles_and_upload_chunks[524289] alone ("table 1
     holds id handle ... twice").  Earlier files: green, all 119.
  2. rs_scatter_kernel: rank[r] without `prior`.  Red: everything here but n = 1, 63 and 64 (one round).  Earlier files: red too
     (78 of 119): any data has digit runs longer than a round.
  3. The key sort started at p_lo + 1 when (63 - sig) % 8 != 0.  Red: test_key_sort_pass_count[1, 8, 9, 56, 57] and every scene of
     2 or 16 code bits with more than one key.  Earlier files: red too (71 of 119): their 12, 16, 24 and 32 code bits all end inside a digit.
     Before key_width_scene moved a third of its rows a little, [56] stayed green under this mutant: no two wide keys differed in
     the lowest digit alone.  The test now asserts, on the oracle's codes, that no pass of the sort could be left out.
  4. The bin sort with one pass fewer, at every n.  Red: everything here but n = 1.  Earlier files: red too (77 of 119).
  5. The bin sort's pass count rounded down, (capbits + 6) / 8: one pass fewer at tables of 2^9 and 2^17 only.  Red:
     test_bin_sort_pass_count[193] and [49153] alone.  Earlier files: test_bounded_select_size_classes_at_128 (n = 60 000, a table of
     2^17) red, the other 118 green: the 2^9 step was unpinned, the 2^17 step pinned by one Route test.
So 1 and the lower step of 5 are what no earlier non-fullsize test could see; 2, 3 and 4 are gross enough for any build to show.
"""
import numpy as np
import pytest

import index_shapes as ish
from route_order_scenes import spread_inv

pytestmark = pytest.mark.gpu

TILE = 2048                     # kRsTile: 4 waves x 8 rounds x 64 lanes


def _scene(O, X, T, D, m, lam, seed, java_hash=None, order=None):
    """conftest.make_scene for given rows: the G functions come from 1000 random rows of the same dimension (rows that are all
    alike would give GFunctionRegistry nothing to measure), oracle and product get the same ones, the oracle's index is built."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n, d = X.shape
    X64 = X.astype(np.float64)
    alpha, r, w = O.registry_init(np.random.default_rng(seed + 5000).standard_normal((1000, d)), m, 13, T, D)
    o = O.Oracle(T, D, m, lam, d, max_global_candidates=20000, refinement_limit=64)
    o.set_gfunctions(alpha, r, w)
    o.set_id_meta(n, java_hash)
    codes = o.build_index(X64, order)                   # [n][TD][W] by staged position
    return dict(X=X, X64=X64, alpha=alpha, r=r, omega=w, oracle=o, deleted=None, java_hash=java_hash, order=order, codes=codes,
                params=dict(n=n, d=d, T=T, D=D, m=m, lam=lam, B=64, hard_cap=20000, probe_override=-1, tau=0))


def _rows(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _distinct_keys(sc, td=0):
    return len(np.unique(ish.keys_of(sc["codes"][:, td, 0])))


def _staged(O, sc):
    """The handles in staged order: the caller's, or the reference's parking rule (the first 999 rows go last)."""
    return O.Oracle.staged_order(sc["params"]["n"]) if sc["order"] is None else np.asarray(sc["order"], np.int32)


def _final_cap(O, sc):
    """(iteration order, final table length) of the oracle's HashMap model for the scene's staging map."""
    n, jh = sc["params"]["n"], sc["java_hash"]
    order = _staged(O, sc)
    h = O.decimal_hashes(n) if jh is None else jh
    it, cap, tree, unmodelled = O.hashmap_order_ex(n, order, h[order], decimal=jh is None)
    assert not tree and not unmodelled
    return it, cap


def _deciding_passes(keys, passes):
    """The byte digits whose pass an LSD radix sort of `keys` cannot leave out: without it, the stable order is another."""
    k = np.asarray(keys).astype(np.uint64)
    full = np.argsort(k, kind="stable")
    return [p for p in passes if not np.array_equal(np.argsort(k & np.uint64(~(0xFF << 8 * p) & (2**64 - 1)), kind="stable"), full)]


def _keys_in_iteration_order(O, sc, td):
    """The keys of table td in the order the key sort gets them: the staging map's iteration order."""
    order = _staged(O, sc)
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    return ish.keys_of(sc["codes"][pos[_final_cap(O, sc)[0]], td, 0])


def _same_tables(ctx, o, what=None):
    for td in range(o.TD):
        got, want = ctx.get_index(td), o.get_index(td)
        for k in ish.ARRAYS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, td, k)


def _build_and_compare(pkg, sc, what=None):
    o = sc["oracle"]
    assert not o.treeified and not o.unmodelled, "a bin of the staging map treeified: the bin sort would not run"
    with ish.make_ctx(pkg, sc, java_hash=sc["java_hash"]) as ctx:
        ctx.build_index(sc["X"], order=sc["order"])
        _same_tables(ctx, o, what)


# ---- 1: tile and wave edges under long digit runs ----------------------------------------------------------------------------
def few_keys_scene(O, n, seed=21):
    """m = 2, lambda = 1: two code bits, so at most four keys and runs of one digit through every round, wave and tile."""
    return _scene(O, _rows(n, 4, seed), 2, 1, 2, 1, seed)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 999, 1000, 1001, 2047, 2048, 2049, 4095, 4096, 4097, 6149])
def test_tile_and_wave_edges(pkg, oracle, n):
    """Below one wave, a wave +- 1, the parking rule of the default order (999 / 1000 / 1001), a tile +- 1, two tiles +- 1 and
    three tiles + 5 (a last tile whose first wave holds five items and whose other waves hold none)."""
    sc = few_keys_scene(oracle, n)
    assert _distinct_keys(sc, 0) <= 4 and _distinct_keys(sc, 1) <= 4
    _build_and_compare(pkg, sc, n)


# ---- 2: one key ------------------------------------------------------------------------------------------------------------------
ONE_KEY_N = 3 * TILE + 5


def eight_per_bin(n, seed):
    """n different hashCodes, eight ids in every used bin (the last one holds n % 8) of the 8192-table the staging map of
    n = 6149 starts with and of the 16384-table it ends with; a ninth would treeify.  Bins 21 j: both digits of the bin sort vary."""
    slot = np.random.default_rng(seed).permutation(n).astype(np.int64)
    return spread_inv(21 * (slot // 8) + 16384 * (1 + slot % 8))


def one_key_scene(O, hashes, order, seed=22):
    n = ONE_KEY_N
    X = np.repeat(_rows(1, 4, seed), n, axis=0)
    jh = eight_per_bin(n, seed) if hashes == "eight_per_bin" else None
    od = np.random.default_rng(seed + 1).permutation(n).astype(np.int32) if order == "permuted" else None
    return _scene(O, X, 2, 1, 8, 2, seed, java_hash=jh, order=od)


@pytest.mark.parametrize("order", ["default", "permuted"])
@pytest.mark.parametrize("hashes", ["decimal", "eight_per_bin"])
def test_one_key(pkg, oracle, hashes, order):
    """Every row is the same vector: the key sort must not move anything, so every table lists the ids in exactly the (bin,
    position) order — asserted against the HashMap model's iteration order directly and then, all five arrays, against the
    oracle's build."""
    sc = one_key_scene(oracle, hashes, order)
    o, n = sc["oracle"], ONE_KEY_N
    assert _distinct_keys(sc, 0) == 1 and _distinct_keys(sc, 1) == 1
    it, cap = _final_cap(oracle, sc)
    assert cap == 16384
    if hashes == "eight_per_bin":
        h = sc["java_hash"].view(np.uint32)
        sp = h ^ (h >> 16)
        for c in (8192, 16384):
            load = np.bincount(sp & np.uint32(c - 1), minlength=c)
            assert load.max() == 8 and (load == 8).sum() == n // 8, c
    assert not o.treeified and not o.unmodelled
    with ish.make_ctx(pkg, sc, java_hash=sc["java_hash"]) as ctx:
        ctx.build_index(sc["X"], order=sc["order"])
        for td in range(o.TD):
            assert np.array_equal(ctx.get_index(td)["ids"], it), td
        _same_tables(ctx, o)


# ---- 3: number of passes of the bin sort ---------------------------------------------------------------------------------------------
# n -> final table length of HashMap<>(n) after n puts; the bin sort runs ceil(log2(length) / 8) passes: 1, 2, 2, 3
BIN_PASSES = [(192, 256), (193, 512), (49152, 65536), (49153, 131072)]


@pytest.mark.parametrize("n,cap", BIN_PASSES)
def test_bin_sort_pass_count(pkg, oracle, n, cap):
    sc = few_keys_scene(oracle, n, seed=23)
    assert _final_cap(oracle, sc)[1] == cap
    assert _distinct_keys(sc, 0) <= 4
    h = oracle.decimal_hashes(n)[_staged(oracle, sc)].view(np.uint32)
    passes = list(range((cap.bit_length() - 1 + 7) // 8))
    assert _deciding_passes((h ^ (h >> 16)) & np.uint32(cap - 1), passes) == passes
    _build_and_compare(pkg, sc, n)


# ---- 4: number of passes of the key sort, key width -----------------------------------------------------------------------------------
KEY_BITS = {1: (1, 1), 7: (7, 1), 8: (8, 1), 9: (9, 1), 55: (55, 1), 56: (28, 2), 57: (57, 1), 63: (63, 1), 64: (32, 2), 65: (65, 1)}
KEY_N = TILE + 1 + 64
KEY_D = 64


def key_width_scene(O, bits, seed=24):
    """n / 3 distinct rows, each twice as it is and once moved a little, at scattered positions.  Random rows alone give
    nearly all-distinct wide keys, which differ in their top digits already: the copies give ties that only a stable sort
    keeps in (bin, position) order, the moved rows (by 0.001 to 0.1 of a standard deviation: a few projections cross into the
    next bucket, and a hash's lowest bit is among the last m code bits) keys that agree in all but the lowest digits."""
    m, lam = KEY_BITS[bits]
    assert m * lam == bits
    rng = np.random.default_rng(seed + 1)
    k = KEY_N // 3
    base = _rows(k, KEY_D, seed)
    moved = base + (10.0 ** rng.uniform(-3, -1, (k, 1)) * rng.standard_normal((k, KEY_D))).astype(np.float32)
    X = np.concatenate([base, base, moved, base[:KEY_N - 3 * k]])[rng.permutation(KEY_N)]
    return _scene(O, X, 1, 2, m, lam, seed + bits)


@pytest.mark.parametrize("bits", sorted(KEY_BITS))
def test_key_sort_pass_count(pkg, oracle, bits):
    """Passes (63 - min(63, bits)) / 8 .. 7 of the key sort: one pass at 1 and 7 bits, two from 8, seven at 55, eight from 56;
    at 63 and 64 bits the key is the whole first word but code bit 63; 65 bits: two code words, rep over both."""
    sc = key_width_scene(oracle, bits)
    o = sc["oracle"]
    assert o.W == (2 if bits == 65 else 1)
    passes = list(range((63 - min(63, bits)) // 8, 8))
    for td in range(o.TD):
        keys = _keys_in_iteration_order(oracle, sc, td)
        assert len(np.unique(keys)) <= min(2 * (KEY_N // 3), 1 << min(bits, 62))      # ties
        assert _deciding_passes(keys, passes) == passes, (td, "a pass of the key sort that this scene could do without")
    _build_and_compare(pkg, sc, bits)


# ---- 5: more than 256 tiles, more than one upload chunk ---------------------------------------------------------------------------------
def many_tiles_scene(O, n, T, seed=25):
    return _scene(O, _rows(n, 4, seed), T, 1, 8, 2, seed)


@pytest.mark.parametrize("n,T,host_cut_too", [(256 * TILE, 1, False), (256 * TILE + 1, 2, False), ((1 << 18) + 1, 1, True)])
def test_many_tiles_and_upload_chunks(pkg, oracle, monkeypatch, n, T, host_cut_too):
    """524 288: exactly 256 tiles, one full chunk of rs_scan_kernel's row walk.  524 289: a second scan chunk of one tile holding
    one item and a third upload chunk of one row, over two tables (scratch reuse, alternating digit totals).  262 145: a second
    upload chunk of one row, coded on the exact path after an MFMA-coded chunk; then the same build with the cut on the host."""
    sc = many_tiles_scene(oracle, n, T)
    assert _distinct_keys(sc, 0) < 2000          # 16 code bits of 4-dimensional rows: long runs
    _build_and_compare(pkg, sc, (n, "gpu cut"))
    if host_cut_too:
        monkeypatch.setenv("FSPANN_GPU_CUT", "0")
        _build_and_compare(pkg, sc, (n, "host cut"))


# ---- 6: incremental build ------------------------------------------------------------------------------------------------------------------
def test_incremental_build_at_tile_edges(pkg, oracle):
    """begin(2048) and pieces of 2047, 2048, 2049 and 1 rows: the code buffer grows three times.  The tables equal the oracle's
    and those of the one-shot build."""
    n = 3 * TILE + 1
    sc = few_keys_scene(oracle, n, seed=26)
    o = sc["oracle"]
    assert _distinct_keys(sc, 0) <= 4
    assert not o.treeified and not o.unmodelled
    with ish.make_ctx(pkg, sc) as ctx:
        ctx.build_begin(TILE)
        at = 0
        for k in (TILE - 1, TILE, TILE + 1, 1):
            ctx.build_append(sc["X"][at:at + k])
            at += k
        assert at == n
        ctx.build_finish()
        _same_tables(ctx, o, "incremental")
        pieces = [ctx.get_index(td) for td in range(o.TD)]
    with ish.make_ctx(pkg, sc) as ctx:
        ctx.build_index(sc["X"])
        _same_tables(ctx, o, "one shot")
        for td in range(o.TD):
            assert ish.same_tables(ctx.get_index(td), pieces[td]), td
