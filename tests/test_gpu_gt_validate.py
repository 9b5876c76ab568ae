"""GPU: GroundtruthValidator on the device (include/fspann_gt_validate.h) — the exact top-1 kernel (fspann_nn1_exact_dev / _store_dev),
validate (fspann_gt_validate_dev / _store_dev, FspannContext.validate_groundtruth) and the gate in run_queries.

Expected values come from tests/gt_validate_ref.py (numpy: the DOUBLE subtraction, sums in dimension order, strict `<` over ascending
rows).  Indices are compared with np.array_equal and distances in their fp64 bits; there are no tolerances.

The launch shape the shapes below are chosen for: 256 rows per tile, a lane per row; at most 1024 workgroups along the rows, each
walking the tiles b, b + G, b + 2 G, ... (G = grid_x(n) below); 16 queries per query tile.

One case of the issue is stated differently here, with its reason: "F32 rows of 3e38 against q = -3e38 give -1" holds for the
ground truth's FLOAT subtraction, which overflows; the validator subtracts in DOUBLE, where (-6e38)^2 = 3.6e77 is an ordinary
number, and the reference's loop names a row.  That scene is held against the restatement (a row wins), and the overflow the
validator's arithmetic does have — F64 queries of 1e200 — is the case that must give -1."""
import ctypes as C

import numpy as np
import pytest

import fallback_ref as F
import gt_ref
import gt_validate_ref as VR

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "u8", "i8", "f16", "bf16", "f8")
PASSED = "GT validation PASSED: %.2f%% match rate"
FAILED = "GT validation FAILED: %.2f%% mismatch rate exceeds %.2f%% tolerance. Groundtruth may be corrupted or computed for a different dataset."


def grid_x(n):
    tiles = (n + 255) // 256
    per = (tiles + 1023) // 1024
    return (tiles + per - 1) // per


def code(pkg, dt):
    N = pkg._native
    return dict(f32=N.F32, u8=N.U8, i8=N.I8, f16=N.F16, bf16=N.BF16, f8=N.F8E4M3)[dt]


def store_kw(pkg, dt):
    return dict(f32=np.float32, u8=np.uint8, i8=np.int8, f16=np.float16, bf16=pkg.bfloat16, f8=pkg.float8_e4m3fn)[dt]


def scene(dt, n, d, nq, seed, q64=False):
    """rows of type dt [n][d], the fp32 values they are, and queries on the type's scale with fractional parts: fp32, or float64 with
    bits below fp32's"""
    rng = np.random.default_rng([seed, DTYPES.index(dt), n, d])
    draw = gt_ref.clustered(rng, d) if d > 1 else lambda cnt: (np.float32(255.0) * rng.random((cnt, 1), dtype=np.float32)).astype(np.float32)
    raw = gt_ref.typed(dt, draw(n))
    X = gt_ref.widen(dt, raw)
    assert np.isfinite(X).all()
    unit = 1.0 if dt in ("f32", "u8", "i8") else 2.0 ** -6
    Q = gt_ref.widen(dt, gt_ref.typed(dt, draw(nq))).astype(np.float64) + unit * (0.0625 + 0.875 * rng.random((nq, d)))
    if not q64:
        Q = Q.astype(np.float32)
    else:
        assert (Q != Q.astype(np.float32)).any()
    assert (Q != np.floor(Q)).mean() > 0.99         # (fp32 rows are off the integers themselves: a sum may land on one)
    return raw, X, Q


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", 0))          # (a copy: fixtures are read-only)


def nn1(pkg, ctx, dt, raw, Q, sel=None, nsel=None, offset_elems=0, want_d2=True):
    """fspann_nn1_exact_dev over the bytes of raw (offset_elems > 0: the base starts that many ELEMENTS into a larger buffer)"""
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    raw = np.ascontiguousarray(raw)
    n, d = raw.shape
    b = raw.view(np.uint8).reshape(-1)
    off = offset_elems * raw.dtype.itemsize
    buf = torch.zeros(off + b.size + 16, dtype=torch.uint8, device=dev)
    buf[off:off + b.size] = _dev(b)
    qd = _dev(Q)
    sd = _dev(np.asarray(sel, np.int64)) if sel is not None else None
    ns = (len(sel) if sel is not None else len(Q)) if nsel is None else nsel
    idx = torch.full((max(ns, 1) + 2,), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((max(ns, 1) + 2,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.nn1_exact_dev(n, buf.data_ptr() + off, code(pkg, dt), len(Q), qd.data_ptr(), N.F64 if Q.dtype == np.float64 else N.F32, d,
                      sd.data_ptr() if sd is not None else 0, ns, idx.data_ptr(), d2.data_ptr() if want_d2 else 0)
    ctx.sync()
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert (idx[ns:] == -7).all() and (d2[ns:] == -7.0).all()          # nothing written past nsel
    return idx[:ns], d2[:ns]


def same(got, ref):
    return np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint64), ref[1].view(np.uint64))


def _cfg(pkg, d):
    return pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=d)


@pytest.fixture(scope="module")
def ctx(pkg):
    """one context for every test that passes the base by pointer (cfg.dim plays no part there)"""
    with pkg.FspannContext(_cfg(pkg, 16), 0) as c:
        yield c


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (1, 7, 32))
@pytest.mark.parametrize("q64", (False, True))
@pytest.mark.parametrize("dt", DTYPES)
def test_base_shape_every_row_type_and_query_type(pkg, ctx, dt, q64, d):
    """n = 773: three full tiles plus 5; d = 7 takes element loads, d = 32 16-byte pieces for every type; 17 queries: two query tiles,
    the second holding one"""
    raw, X, Q = scene(dt, 773, d, 17, seed=1, q64=q64)
    ref = VR.top1(X, Q)
    assert (ref[0] >= 0).all()
    assert same(nn1(pkg, ctx, dt, raw, Q), ref)


@pytest.mark.parametrize("dt", DTYPES)
def test_unaligned_base_takes_element_loads_and_says_the_same(pkg, ctx, dt):
    raw, X, Q = scene(dt, 773, 32, 5, seed=2)
    ref = VR.top1(X, Q)
    assert same(nn1(pkg, ctx, dt, raw, Q, offset_elems=1), ref) and same(nn1(pkg, ctx, dt, raw, Q), ref)


@pytest.mark.parametrize("n", (1, 200))
@pytest.mark.parametrize("dt", ("f32", "u8"))
def test_small_n(pkg, ctx, dt, n):
    """n = 1, and n = 200 where one partial tile is the whole grid"""
    raw, X, Q = scene(dt, n, 7, 17, seed=3)
    assert same(nn1(pkg, ctx, dt, raw, Q), VR.top1(X, Q))


def _plant(raw, Q, j, rows, dt):
    """query j's nearest row, exactly: Q[j] without its fraction, written to every row of `rows`; any other row of the integer types
    differs by at least 1 in some coordinate and is farther"""
    v = np.floor(Q[j]).astype(raw.dtype) if dt != "f32" else np.floor(Q[j]).astype(np.float32)
    for r in rows:
        raw[r] = v


@pytest.mark.parametrize("dt", ("u8", "f32"))
def test_ties_go_to_the_lower_index_and_winners_at_the_edges(pkg, ctx, dt):
    """an exact duplicate of the winning row in another lane of the same wave (70, 100), another wave of the same workgroup (70, 200),
    another workgroup (70, 600); the winner alone at rows 0, 255, 256 and n - 1"""
    n, d = 773, 7
    assert grid_x(n) == 4
    raw, X, Q = scene(dt, n, d, 17, seed=4)
    if dt == "f32":
        raw = np.rint(raw).astype(np.float32)          # integers: the planted row is then strictly the nearest
    raw = raw.copy()
    Q = (np.floor(Q) + np.float32(0.25)).astype(np.float32)
    pairs = [(70, 100), (70, 200), (70, 600), (300, 301), (511, 512), (5, 772)]
    for (a, b) in pairs:
        r2 = raw.copy()
        _plant(r2, Q, 0, (a, b), dt)
        got = nn1(pkg, ctx, dt, r2, Q)
        assert got[0][0] == a and got[1][0] == d * 0.0625, (a, b, got[0][0])
        assert same(got, VR.top1(gt_ref.widen(dt, r2), Q))
    r2 = raw.copy()
    for j, r in enumerate((0, 255, 256, n - 1)):
        _plant(r2, Q, j, (r,), dt)
    got = nn1(pkg, ctx, dt, r2, Q)
    assert got[0][:4].tolist() == [0, 255, 256, n - 1]
    assert same(got, VR.top1(gt_ref.widen(dt, r2), Q))


def test_a_lane_walks_several_tiles_and_queries_run_in_chunks(pkg, monkeypatch):
    """n = 263000: 1028 tiles over G = 514 workgroups, so a lane owns rows r and r + 514 * 256.  Duplicates of the winner in a later
    tile of the same lane, in another workgroup far away and near the end: the lower index wins; a winner alone at n - 1.  And under FSPANN_GT_SCRATCH_MB=1 a
    query costs 8 d + 12 G bytes of scratch, 160 queries fit, and 200 selected queries run as two chunks."""
    monkeypatch.setenv("FSPANN_GT_SCRATCH_MB", "1")
    n, d = 263000, 2
    G = grid_x(n)
    assert G == 514 and (1 << 20) // (8 * d + 12 * G) // 16 * 16 == 160
    raw, X, Q = scene("u8", n, d, 6, seed=5)
    raw = np.minimum(raw, 200)                         # no row of the draw comes near a target
    plan = [(70, 70 + G * 256), (70 + G * 256, 70 + G * 256 + 1), (1000, n - 2), (n - 1,), (256 * G - 1, 256 * G), (131, 200000, 262998)]
    Q = np.array([[210.25 + 5 * j, 17.25] for j in range(6)], np.float32)
    for j, rows in enumerate(plan):
        _plant(raw, Q, j, rows, "u8")
    X = gt_ref.widen("u8", raw)
    ref = VR.top1(X, Q)
    assert ref[0].tolist() == [p[0] for p in plan] and (ref[1] == d * 0.0625).all()
    sel = np.random.default_rng(6).integers(0, 6, 200)
    with pkg.FspannContext(_cfg(pkg, 16), 0) as c:
        assert same(nn1(pkg, c, "u8", raw, Q), ref)
        got = nn1(pkg, c, "u8", raw, Q, sel=sel)
        assert same(got, (ref[0][sel], ref[1][sel]))


def test_non_finite_distances_never_win(pkg, ctx):
    rng = np.random.default_rng(8)
    n, d = 773, 7
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((6, d)).astype(np.float32)
    Q[1, 3] = np.nan
    Q[2, 0] = np.inf
    X[::3, 1] = np.nan                                   # NaN rows, the first row among them
    X[5] = Q[0]                                          # ... and a finite exact match
    X[3] = Q[3]
    X[3, 2] = np.nan                                     # what would be query 3's nearest row is NaN
    ref = VR.top1(X, Q)
    assert ref[0][0] == 5 and ref[0][1] == ref[0][2] == -1 and ref[0][3] not in (-1, 3) and not np.isnan(X[ref[0]]).any()
    got = nn1(pkg, ctx, "f32", X, Q)
    assert same(got, ref) and np.isposinf(got[1][1:3]).all()
    # every row NaN
    allnan = np.full((n, d), np.nan, np.float32)
    got = nn1(pkg, ctx, "f32", allnan, Q)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all()
    h = np.full((n, d), np.float16(np.nan))
    got = nn1(pkg, ctx, "f16", h, Q)
    assert (got[0] == -1).all() and np.isposinf(got[1]).all()
    # one finite row among +-inf rows, in halves and in bfloat16, fp32 queries
    for dt, pinf, ninf, one in (("f16", 0x7C00, 0xFC00, 0x3C00), ("bf16", 0x7F80, 0xFF80, 0x3F80)):
        bits = np.where(rng.random((n, d)) < 0.5, pinf, ninf).astype(np.uint16)
        bits[611] = one
        raw = bits.view(np.float16) if dt == "f16" else bits
        Xv = gt_ref.widen(dt, raw)
        assert np.isinf(np.delete(Xv, 611, axis=0)).all()
        ref = VR.top1(Xv, Q)
        assert ref[0].tolist() == [611, -1, -1, 611, 611, 611]
        assert same(nn1(pkg, ctx, dt, raw, Q), ref)


def test_sums_that_overflow(pkg, ctx):
    """(this file's docstring: the scene of the issue does not overflow in the validator's arithmetic; F64 queries of 1e200 do)"""
    n, d = 300, 4
    X = np.full((n, d), 3e38, np.float32)
    q32 = np.full((2, d), -3e38, np.float32)
    ref = VR.top1(X, q32)
    assert ref[0].tolist() == [0, 0] and np.isfinite(ref[1]).all() and (ref[1] > 1e77).all()
    assert same(nn1(pkg, ctx, "f32", X, q32), ref)
    q64 = np.full((2, d), -1e200, np.float64)
    q64[1] = 0.5
    ref = VR.top1(X, q64)
    assert ref[0].tolist() == [-1, 0] and np.isposinf(ref[1][0])
    assert same(nn1(pkg, ctx, "f32", X, q64), ref)


def test_query_selection(pkg, ctx):
    raw, X, Q = scene("i8", 773, 7, 40, seed=9)
    ref = VR.top1(X, Q)
    sel = np.array([39, 3, 3, 17, 0, 39, 16, 15, 3, 22, 1, 2, 38, 37, 36, 35, 34, 5], np.int64)      # repeats, unsorted, two query tiles
    assert same(nn1(pkg, ctx, "i8", raw, Q, sel=sel), (ref[0][sel], ref[1][sel]))
    assert same(nn1(pkg, ctx, "i8", raw, Q), ref)                                                     # NULL: all nq
    assert same(nn1(pkg, ctx, "i8", raw, Q, nsel=5), (ref[0][:5], ref[1][:5]))                        # NULL: the first nsel
    got = nn1(pkg, ctx, "i8", raw, Q, sel=np.array([2, 40, -1, 7], np.int64))                         # outside [0, nq): -1 / +inf
    assert got[0].tolist() == [ref[0][2], -1, -1, ref[0][7]] and np.isposinf(got[1][1:3]).all()
    idx, d2 = nn1(pkg, ctx, "i8", raw, Q, sel=sel, want_d2=False)                                     # out_d2 may be NULL
    assert np.array_equal(idx, ref[0][sel])
    assert len(nn1(pkg, ctx, "i8", raw, Q, sel=sel, nsel=0)[0]) == 0                                  # nsel == 0: nothing written


def test_arithmetic_differs_from_the_ground_truth_on_the_device(pkg, ctx):
    """q = 2^25, rows 3 and 4: the float subtraction ties and names row 0, the double subtraction names row 1"""
    import torch
    N = pkg._native
    X, Q = VR.planted_scene()
    for dt in ("u8", "f32"):
        raw = X.astype(np.uint8) if dt == "u8" else X
        got = nn1(pkg, ctx, dt, raw, Q)
        assert got[0].tolist() == [1] and got[1][0] == 33554428.0 ** 2
        bd, qd = _dev(raw), _dev(Q)
        ids = torch.full((1, 1), -7, dtype=torch.int32, device=bd.device)
        torch.cuda.synchronize()
        ctx.groundtruth_rows_dev(2, bd.data_ptr(), code(pkg, dt), 1, qd.data_ptr(), 1, 1, ids.data_ptr())
        ctx.sync()
        assert ids.cpu().numpy().tolist() == [[0]]
    xd, qd = _dev(X), _dev(Q)
    ids = torch.full((1, 1), -7, dtype=torch.int32, device=xd.device)
    torch.cuda.synchronize()
    ctx.groundtruth_dev(2, xd.data_ptr(), 1, qd.data_ptr(), 1, 1, ids.data_ptr())
    ctx.sync()
    assert ids.cpu().numpy().tolist() == [[0]]
    assert N.F64 == 1


# ---- the store variant, states and refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ("u8", "f16", "f32"))
def test_store_variant_equals_the_plain_call(pkg, dt):
    import torch
    N = pkg._native
    raw, X, Q = scene(dt, 773, 24, 17, seed=11, q64=True)
    sel = np.array([16, 0, 5, 5], np.int64)
    ref = VR.top1(X, Q)
    with pkg.FspannContext(_cfg(pkg, 24), 0) as c:
        c.store_set(raw, dtype=store_kw(pkg, dt))
        plain = nn1(pkg, c, dt, raw, Q, sel=sel)
        qd, sd = _dev(Q), _dev(sel)
        idx = torch.full((4,), -7, dtype=torch.int32, device=qd.device)
        d2 = torch.full((4,), -7.0, dtype=torch.float64, device=qd.device)
        torch.cuda.synchronize()
        c.nn1_exact_store_dev(len(Q), qd.data_ptr(), N.F64, sd.data_ptr(), 4, idx.data_ptr(), d2.data_ptr())
        c.sync()
        assert same((idx.cpu().numpy(), d2.cpu().numpy()), plain) and same(plain, (ref[0][sel], ref[1][sel]))
        assert same(c.nn1_exact(raw, Q, dtype=store_kw(pkg, dt), sel=sel), plain)                 # the numpy-level call
        assert same(c.nn1_exact(raw, Q.astype(np.float32), dtype=store_kw(pkg, dt)), VR.top1(X, Q.astype(np.float32)))


def test_states_and_refused_types(pkg):
    import torch
    N = pkg._native
    rng = np.random.default_rng(2)
    n, d, nq = 500, 16, 6
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d))
    gt = VR.top1(X, Q)[0].reshape(nq, 1)
    err = lambda: N.lib().fspann_last_error().decode()
    v = N.GtValidation()
    with pkg.FspannContext(_cfg(pkg, d), 0) as c:
        L, h = c.L, c.handle
        xd, qd, gd = _dev(X), _dev(Q), _dev(gt)
        idx = torch.full((nq,), -7, dtype=torch.int32, device=xd.device)
        torch.cuda.synchronize()
        b, q, g, oi = xd.data_ptr(), qd.data_ptr(), gd.data_ptr(), idx.data_ptr()
        assert L.fspann_nn1_exact_store_dev(h, nq, q, N.F64, None, nq, oi, None) == N.E_STATE            # no store yet
        assert L.fspann_gt_validate_store_dev(h, nq, q, N.F64, g, nq, 1, 100, 0.05, C.byref(v)) == N.E_STATE
        c.store_set(X.astype(np.float64))
        assert L.fspann_nn1_exact_store_dev(h, nq, q, N.F64, None, nq, oi, None) == N.E_ARG and "FSPANN_F64" in err()
        assert L.fspann_gt_validate_store_dev(h, nq, q, N.F64, g, nq, 1, 100, 0.05, C.byref(v)) == N.E_ARG and "FSPANN_F64" in err()
        call = lambda bdt=N.F32, qdt=N.F64, n_=n, b_=b, q_=q, d_=d, nsel=nq, oi_=oi: L.fspann_nn1_exact_dev(h, n_, b_, bdt, nq, q_, qdt, d_, None, nsel, oi_, None)
        assert call(bdt=N.F64) == N.E_ARG and "FSPANN_F64" in err()
        assert call(bdt=77) == N.E_ARG and "77" in err()
        assert call(qdt=N.U8) == N.E_ARG and "FSPANN_U8" in err()
        assert call(qdt=N.F16) == N.E_ARG and "FSPANN_F16" in err()
        assert call(b_=None) == N.E_NULL and call(q_=None) == N.E_NULL and call(oi_=None) == N.E_NULL
        assert call(n_=0) == N.E_ARG and call(n_=1 << 31) == N.E_ARG and call(d_=0) == N.E_ARG
        assert call(nsel=-1) == N.E_ARG and call(nsel=nq + 1) == N.E_ARG
        assert call(nsel=0, oi_=None) == N.OK
        assert L.fspann_gt_validate_dev(h, n, b, N.F64, nq, q, N.F64, d, g, nq, 1, 100, 0.05, C.byref(v)) == N.E_ARG and "FSPANN_F64" in err()
        assert L.fspann_gt_validate_dev(h, n, b, N.F32, nq, q, N.F64, d, g, nq, 0, 100, 0.05, C.byref(v)) == N.E_ARG      # gt_stride < 1
        assert L.fspann_gt_validate_dev(h, n, b, N.F32, nq, q, N.F64, d, g, nq, 1, 100, 0.05, None) == N.E_NULL
        assert call() == N.OK
        c.sync()
        assert np.array_equal(idx.cpu().numpy(), gt[:, 0])


# ---- validate ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vscene():
    """n = 2000, d = 16, nq = 300; the ground truth is the validator arithmetic's own top-1 in column 0"""
    rng = np.random.default_rng(12)
    n, d, nq = 2000, 16, 300
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    nn = VR.top1(X, Q)[0]
    gt = np.stack([nn, rng.integers(0, n, nq), rng.integers(0, n, nq)], axis=1).astype(np.int32)
    gt[7, 1], gt[9, 2] = 0, n - 1
    for a in (X, Q, nn, gt):
        a.setflags(write=False)
    return X, Q, nn, gt


def _expect(ctx, nn, gt, nq, sample, tol):
    s = [int(x) for x in ctx.gt_validator_sample(nq, sample)]
    return s, VR.validate(lambda qi: nn[qi], s, nq, gt, sample, tol)


def _agrees(got, want):
    return all(got[k] == want[k] for k in ("valid", "sample_size", "mismatches", "mismatched")) and \
        np.array_equal(np.float64(got["mismatch_rate"]).view(np.uint64), np.float64(want["mismatch_rate"]).view(np.uint64))


def test_validate(pkg, ctx, vscene):
    X, Q, nn, gt = vscene
    n, nq = len(X), len(Q)
    s, want = _expect(ctx, nn, gt, nq, 100, 0.05)
    assert len(s) == 100 == len(set(s))
    got = ctx.validate_groundtruth(X, Q, gt)
    assert _agrees(got, want) and got["valid"] and got["mismatches"] == 0 and got["message"] == PASSED % 100.0
    assert (got["gt_min_id"], got["gt_max_id"], got["consistent"]) == (0, n - 1, True)
    # wrong first ids at chosen sampled queries: 5 of 100 at tolerance 0.05 is valid (`>` is strict), 6 is not, 12 lists the first 10
    for wrong in (5, 6, 12):
        g = gt.copy()
        pick = s[2::7][:wrong]
        assert len(pick) == wrong
        g[pick, 0] = (g[pick, 0] + 1) % n
        got = ctx.validate_groundtruth(X, Q, g)
        want = VR.validate(lambda qi: nn[qi], s, nq, g, 100, 0.05)
        assert _agrees(got, want) and got["mismatches"] == wrong and got["valid"] == (wrong == 5)
        assert got["mismatched"] == [q for q in s if q in set(pick)][:10]
        assert got["message"] == (PASSED % 95.0 if wrong == 5 else FAILED % (wrong * 1.0, 5.0))
    # the defaults of the wrappers, float64 queries, another sample size and tolerance
    assert _agrees(ctx.validate_groundtruth(X, Q.astype(np.float64), g, sample_size=0, tolerance=-1.0), want)
    s40, want40 = _expect(ctx, nn, g, nq, 40, 0.5)
    got = ctx.validate_groundtruth(X, Q, g, sample_size=40, tolerance=0.5)
    assert _agrees(got, want40) and got["sample_size"] == 40 and got["valid"]
    # fewer ground-truth rows than queries: sampled queries >= 250 are skipped, the denominator stays 100
    g = gt[:250].copy()
    g[:, 0] = (g[:, 0] + 1) % n
    got = ctx.validate_groundtruth(X, Q, g)
    inside = [q for q in s if q < 250]
    assert 0 < len(inside) < 100 and got["mismatches"] == len(inside) and got["sample_size"] == 100
    assert got["mismatch_rate"] == len(inside) / 100.0 and got["mismatched"] == inside[:10] and not got["valid"]
    # the two early returns
    got = ctx.validate_groundtruth(X, Q, gt[:0])
    assert (got["valid"], got["sample_size"], got["mismatch_rate"], got["message"]) == (False, 0, 1.0, "Groundtruth is empty")
    got = ctx.validate_groundtruth(X, Q[:0], gt)
    assert (got["valid"], got["sample_size"], got["mismatches"], got["message"]) == (True, 0, 0, "No queries to validate")
    # an id offset over the whole matrix is caught, and shows in the id range
    got = ctx.validate_groundtruth(X, Q, gt + 1)
    assert not got["valid"] and got["mismatches"] == 100 and got["gt_min_id"] == 1 and got["gt_max_id"] == n and not got["consistent"]
    assert got["message"] == FAILED % (100.0, 5.0)
    g = gt.copy()
    g[200, 2] = -1
    got = ctx.validate_groundtruth(X, Q, g)
    assert got["valid"] and got["gt_min_id"] == -1 and not got["consistent"]
    g[200, 2] = n
    assert not ctx.validate_groundtruth(X, Q, g)["consistent"]


def test_validate_at_the_c_level_with_sample_size_zero(pkg, ctx, vscene):
    """the call takes sample_size and tolerance as given: 0 of 0 is NaN, and NaN > tolerance is false"""
    N = pkg._native
    X, Q, nn, gt = vscene
    xd, qd, gd = _dev(X), _dev(Q), _dev(gt + 1)
    import torch
    torch.cuda.synchronize()
    v = ctx.gt_validate_dev(len(X), xd.data_ptr(), N.F32, len(Q), qd.data_ptr(), N.F32, X.shape[1], gd.data_ptr(), len(gt), gt.shape[1], 0, 0.05)
    assert v.valid == 1 and v.sample_size == 0 and v.mismatches == 0 and v.mismatch_rate != v.mismatch_rate and v.gt_min_id == 1


@pytest.mark.parametrize("dt", ("u8", "f32"))
def test_validate_against_the_store(pkg, dt):
    raw, X, Q = scene(dt, 2000, 16, 300, seed=13)
    nn = VR.top1(X, Q)[0]
    gt = nn.reshape(-1, 1).astype(np.int32)
    with pkg.FspannContext(_cfg(pkg, 16), 0) as c:
        c.store_set(raw, dtype=store_kw(pkg, dt))
        got = c.validate_groundtruth_store(Q, gt)
        assert got["valid"] and got["mismatches"] == 0 and got["sample_size"] == 100
        assert _agrees(c.validate_groundtruth(raw, Q, gt, dtype=store_kw(pkg, dt)), got)
        bad = c.validate_groundtruth_store(Q, (gt + 1) % 2000)
        assert not bad["valid"] and bad["mismatches"] == 100 and bad["mismatched"] == [int(x) for x in c.gt_validator_sample(300, 100)[:10]]


# ---- run_queries ---------------------------------------------------------------------------------------------------------------------------
def test_run_queries_gate(pkg, oracle):
    sc, Q, K, ref, fb, _, _ = F.main_scene(oracle)
    KS = (1, 10, 20)
    with F.context(pkg, sc) as ctx:
        plain = ctx.run_queries(Q, KS, B=256)
        assert "gt_validation" not in plain and sorted(plain) == sorted(
            ("ids", "dist", "count", "scored", "sel_count", "bad", "retried", "fellback", "resolved", "gt_ids", "recall", "ratio", "cand_ratio"))
        again = ctx.run_queries(Q, KS, B=256, validate=None)
        own = ctx.run_queries(Q, KS, B=256, validate=(100, 0.05))                       # no gt_ids given: nothing to validate
        for other in (again, own):
            assert sorted(other) == sorted(plain)
            for k in plain:
                a, b = np.asarray(plain[k]), np.asarray(other[k])
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), k
        got = ctx.run_queries(Q, KS, gt_ids=plain["gt_ids"], B=256, validate=(100, 0.05))
        v = got.pop("gt_validation")
        assert v["valid"] and v["sample_size"] == len(Q) and v["mismatches"] == 0 and v["message"] == PASSED % 100.0
        for k in plain:
            assert np.asarray(plain[k]).tobytes() == np.asarray(got[k]).tobytes(), k
        with pytest.raises(pkg.FspannStateError) as e:
            ctx.run_queries(Q, KS, gt_ids=plain["gt_ids"] + 1, B=256, validate=(100, 0.05))
        assert FAILED % (100.0, 5.0) in str(e.value)
