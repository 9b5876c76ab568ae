"""GPU: the exact ground truth of fp32 queries over typed rows as they are (fspann_groundtruth_rows_dev) and over the resident store
(fspann_groundtruth_store_dev), for FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 and FSPANN_F8E4M3.  Rows are drawn as values the
type holds exactly (the generators and the one rounding of tests/test_gpu_*_rows.py), queries are fp32 WITH fractional parts, and
every result must EQUAL (np.array_equal: ids and fp64 distance bits) two witnesses: the oracle's GroundtruthPrecompute.run over the
rows widened to fp32 by this file, and fspann_groundtruth_dev over that widened copy.  There are no tolerances.

One comparison is stated more narrowly, with its reason.  Where rows hold NaN, the distances of those rows are NaN, and neither
IEEE 754 nor the contract ("NaN sorts last") pins the sign or payload of a NaN, which is all that orders NaN rows among themselves.
There the results are compared exactly over the rows whose distance is a number (+inf included), and the NaN rows must be exactly
the tail, in any order."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ("u8", "i8", "f16", "bf16", "f8")


def e4m3_table():
    """value of each of the 256 patterns, from the definition: E = 0: +-M/8 * 2^-6; E = 1..15: +-(1 + M/8) * 2^(E-7); 0x7F / 0xFF NaN"""
    t = np.empty(256, np.float64)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        v = float("nan") if (e == 15 and m == 7) else (m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if s else v
    return t


TABLE32 = e4m3_table().astype(np.float32)        # (every e4m3 value is a float)


def clustered(rng, d, r=16, noise=6.0):
    """bench.py's SIFT-like generator (intrinsic dimension r) without its rounding: draw(cnt) -> float32 in [0, 255]"""
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)

    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        v = np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)
        return np.clip(v, 0, 255).astype(np.float32)
    return draw


def bf16_round(a):
    """finite float32 values -> bfloat16 bit patterns (uint16), round to nearest even on the bit pattern"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    assert ((u & 0x7F800000) != 0x7F800000).all()
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def f8_cast(a):
    """the caller's rounding: float32 values -> e4m3 bytes, torch's cast on the CPU"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()


def typed(dt, a):
    """float32 draws in [0, 255] -> the rows of type dt as the library takes them (u8 / i8 / f16 arrays, uint16 bf16 patterns, uint8
    e4m3 patterns): the one rounding, on the host.  u8, i8: the integer scale; f16, bf16: O(1); f8: [0, 64]."""
    if dt == "u8":
        return np.rint(a).astype(np.uint8)
    if dt == "i8":
        return (np.rint(a) - 128).astype(np.int8)
    if dt == "f16":
        return (a / np.float32(64.0)).astype(np.float16)
    if dt == "bf16":
        return bf16_round(a / np.float32(64.0))
    return f8_cast(a / np.float32(4.0))


def widen(dt, raw):
    """rows of type dt -> the float32 values they are (exact, and by this file: astype for the numpy types, the shift for bfloat16,
    the table of the format's definition for fp8)"""
    if dt == "bf16":
        return (np.ascontiguousarray(raw, np.uint16).astype(np.uint32) << 16).view(np.float32)
    if dt == "f8":
        return TABLE32[np.ascontiguousarray(raw, np.uint8)]
    return raw.astype(np.float32)


def code(pkg, dt):
    N = pkg._native
    return dict(u8=N.U8, i8=N.I8, f16=N.F16, bf16=N.BF16, f8=N.F8E4M3)[dt]


def store_kw(pkg, dt):
    return dict(u8=np.uint8, i8=np.int8, f16=np.float16, bf16=pkg.bfloat16, f8=pkg.float8_e4m3fn)[dt]


def scene(dt, n, d, nq, seed):
    """rows of type dt [n][d], their fp32 values, and fp32 queries from the same distribution on the type's scale, off the grid of
    the rows (a fraction of a unit added: no query is a row, none is an integer)"""
    rng = np.random.default_rng(seed)
    draw = clustered(rng, d)
    raw = typed(dt, draw(n))
    X = widen(dt, raw)
    assert np.isfinite(X).all()
    Q = widen(dt, typed(dt, draw(nq)))
    unit = np.float32(1.0) if dt in ("u8", "i8") else np.float32(2.0 ** -6)
    Q = (Q + unit * (np.float32(0.0625) + np.float32(0.875) * rng.random(Q.shape, dtype=np.float32))).astype(np.float32)
    return raw, X, Q


def _bytes(raw):
    return np.ascontiguousarray(raw).view(np.uint8).reshape(-1)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _out(nq, k):
    import torch
    dev = torch.device("cuda", 0)
    return torch.full((nq, k), -7, dtype=torch.int32, device=dev), torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)


def rows_gt(pkg, ctx, dt, raw, Q, k, offset_elems=0):
    """fspann_groundtruth_rows_dev over the bytes of raw; offset_elems > 0: the base starts that many ELEMENTS into a larger buffer"""
    import torch
    n, d = raw.shape
    b = _bytes(raw)
    off = offset_elems * raw.dtype.itemsize
    buf = torch.zeros(off + b.size + 16, dtype=torch.uint8, device=torch.device("cuda", 0))
    buf[off:off + b.size] = _dev(b)
    qd = _dev(Q)
    ids, d2 = _out(len(Q), k)
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    ctx.groundtruth_rows_dev(n, buf.data_ptr() + off, code(pkg, dt), len(Q), qd.data_ptr(), d, k, ids.data_ptr(), d2.data_ptr())
    ctx.sync()
    return ids.cpu().numpy(), d2.cpu().numpy()


def f32_gt(ctx, X, Q, k):
    import torch
    xd, qd = _dev(X), _dev(Q)
    ids, d2 = _out(len(Q), k)
    torch.cuda.synchronize()
    ctx.groundtruth_dev(len(X), xd.data_ptr(), len(Q), qd.data_ptr(), X.shape[1], k, ids.data_ptr(), d2.data_ptr())
    ctx.sync()
    return ids.cpu().numpy(), d2.cpu().numpy()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _cfg(pkg, d):
    return pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=d)


@pytest.fixture(scope="module")
def ctx(pkg):
    """one context for every test that passes the base by pointer (cfg.dim plays no part there)"""
    with pkg.FspannContext(_cfg(pkg, 16), 0) as c:
        yield c


# (300,7): element path, k near n.  (40,16): k > n, -1 fill.  (257,16): row-tile and query-tile tails on the vector path.  (64,1): d = 1.
SHAPES = [(300, 7, 5, 100), (40, 16, 3, 64), (257, 16, 17, 10), (5000, 128, 37, 10), (70000, 32, 20, 1), (64, 1, 4, 3)]


@pytest.mark.parametrize("n,d,nq,k", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_rows_ground_truth_equals_oracle_and_fp32_path(pkg, oracle, ctx, dt, n, d, nq, k):
    raw, X, Q = scene(dt, n, d, nq, seed=n + k)
    assert (Q != np.floor(Q)).all()
    got = rows_gt(pkg, ctx, dt, raw, Q, k)
    assert same(got, oracle.groundtruth(X, Q, k))
    assert same(got, f32_gt(ctx, X, Q, k))
    if k > n:
        assert (got[0][:, n:] == -1).all() and np.isposinf(got[1][:, n:]).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_ties_go_to_the_lower_id(pkg, oracle, ctx, dt):
    """rows from a four-value alphabet, the first thousand twice: many exactly equal distances (every type holds 0, 1, 2, 3)"""
    rng = np.random.default_rng(7)
    V = rng.integers(0, 4, (3000, 16)).astype(np.float32)
    V[1000:2000] = V[:1000]
    raw = dict(u8=lambda: V.astype(np.uint8), i8=lambda: V.astype(np.int8), f16=lambda: V.astype(np.float16), bf16=lambda: bf16_round(V),
               f8=lambda: f8_cast(V))[dt]()
    X = widen(dt, raw)
    assert np.array_equal(X, V)
    Q = rng.integers(0, 4, (25, 16)).astype(np.float32) + np.float32(0.5)
    ids, d2 = got = rows_gt(pkg, ctx, dt, raw, Q, 50)
    assert same(got, oracle.groundtruth(X, Q, 50)) and same(got, f32_gt(ctx, X, Q, 50))
    for i in range(len(Q)):                                  # ascending (distance, id)
        key = list(zip(d2[i], ids[i]))
        assert key == sorted(key)
        assert len(set(d2[i])) < 50                          # (and there were ties to break)


@pytest.mark.parametrize("dt", DTYPES)
def test_base_off_a_16_byte_boundary_takes_element_loads(pkg, oracle, ctx, dt):
    """d % 16 == 0, so the rows are whole 16-byte pieces, but the base starts one element into its buffer: no row is aligned"""
    raw, X, Q = scene(dt, 1000, 32, 19, seed=11)
    got = rows_gt(pkg, ctx, dt, raw, Q, 10, offset_elems=1)
    assert same(got, oracle.groundtruth(X, Q, 10))
    assert same(got, f32_gt(ctx, X, Q, 10))
    assert same(got, rows_gt(pkg, ctx, dt, raw, Q, 10))      # and the aligned base, 16 bytes at a time, says the same


EDGE = dict(
    # finite values at the ends of each type: subnormals, the largest magnitudes, both zeros
    f16=(np.array([0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x8000], np.uint16), np.array([0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01], np.uint16)),
    bf16=(np.array([0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x7F7F, 0xFF7F, 0x8000], np.uint16), np.array([0x7F80, 0xFF80, 0x7FC0, 0xFFC0, 0x7F81], np.uint16)),
    f8=(np.array([0x01, 0x81, 0x07, 0x87, 0x08, 0x7E, 0xFE, 0x80], np.uint8), np.array([0x7F, 0xFF], np.uint8)),
    i8=(np.array([-128, 127, -1, 0], np.int8), None),
    u8=(np.array([255, 0, 1, 128], np.uint8), None),
)


def _plant(raw, vals, first):
    """every value of vals in a row of its own from row `first` on, at a column that moves along; once more in a row all of that value"""
    n, d = raw.shape
    for j, v in enumerate(vals):
        raw[first + 2 * j, j % d] = v
        raw[first + 2 * j + 1, :] = v
    return first + 2 * len(vals)


def _edge_scene(dt, d, nonfinite):
    raw, _, Q = scene(dt, 600, d, 9, seed=5 + d)
    raw = raw.copy()
    shape = raw.shape
    if dt == "f16":
        raw = raw.view(np.uint16)
    fin, nonf = EDGE[dt]
    nxt = _plant(raw, fin.astype(raw.dtype), 3)
    if nonfinite:
        _plant(raw, nonf.astype(raw.dtype), nxt)
    if dt == "f16":
        raw = raw.view(np.float16)
    assert raw.shape == shape
    return raw, widen(dt, raw), Q


@pytest.mark.parametrize("d", (16, 7))
@pytest.mark.parametrize("dt", DTYPES)
def test_subnormal_and_extreme_rows(pkg, oracle, ctx, dt, d):
    """finite scene (subnormals, the largest magnitudes, -0.0; I8 -128, U8 255): the oracle and the fp32 path, k = n"""
    raw, X, Q = _edge_scene(dt, d, nonfinite=False)
    assert np.isfinite(X).all()
    if dt == "f16":
        assert X.min() == -65504 and 0 < np.abs(X[X != 0]).min() == 2.0 ** -24
    if dt == "bf16":
        assert 0 < np.abs(X[X != 0]).min() == 2.0 ** -133         # an fp32 subnormal
    if dt == "f8":
        assert X.max() == 448 and np.abs(X[X != 0]).min() == 2.0 ** -9
    got = rows_gt(pkg, ctx, dt, raw, Q, len(X))
    assert same(got, oracle.groundtruth(X, Q, len(X)))
    assert same(got, f32_gt(ctx, X, Q, len(X)))


@pytest.mark.parametrize("d", (16, 7))
@pytest.mark.parametrize("dt", ("f16", "bf16", "f8"))
def test_nonfinite_rows_take_part(pkg, ctx, dt, d):
    """+-inf gives an infinite distance (ties among them by id), NaN sorts last: k = n against the fp32 path over the widened copy,
    exactly over the rows whose distance is a number, the NaN rows exactly the tail (this file's docstring says why)"""
    raw, X, Q = _edge_scene(dt, d, nonfinite=True)
    n = len(X)
    nan_rows = np.flatnonzero(np.isnan(X).any(axis=1))
    assert len(nan_rows) >= 4 and (dt == "f8" or np.isinf(X).any())
    ids, d2 = rows_gt(pkg, ctx, dt, raw, Q, n)
    rid, rd2 = f32_gt(ctx, X, Q, n)
    m = n - len(nan_rows)
    assert np.array_equal(ids[:, :m], rid[:, :m]) and np.array_equal(d2[:, :m], rd2[:, :m])
    assert not np.isnan(d2[:, :m]).any() and (dt == "f8" or np.isposinf(d2[:, :m]).any())
    assert np.isnan(d2[:, m:]).all() and np.isnan(rd2[:, m:]).all()
    for i in range(len(Q)):
        assert np.array_equal(np.sort(ids[i, m:]), nan_rows) and np.array_equal(np.sort(rid[i, m:]), nan_rows)
    # and a smaller k never sees them
    assert same(rows_gt(pkg, ctx, dt, raw, Q, 50), f32_gt(ctx, X, Q, 50))


@pytest.mark.parametrize("dt", DTYPES)
def test_queries_run_in_chunks_under_a_small_scratch_budget(pkg, oracle, monkeypatch, dt):
    """1 MiB of scratch holds 16 rows of the [chunk x 8000] fp64 matrix: 100 queries are 7 chunks, the last one a tail"""
    monkeypatch.setenv("FSPANN_GT_SCRATCH_MB", "1")
    raw, X, Q = scene(dt, 8000, 16, 100, seed=21)
    ref = oracle.groundtruth(X, Q, 10)
    with pkg.FspannContext(_cfg(pkg, 16), 0) as c:
        assert same(rows_gt(pkg, c, dt, raw, Q, 10), ref)
        assert same(f32_gt(c, X, Q, 10), ref)


def _store_ptr(c):
    dt = C.c_int(-1)
    p = c.L.fspann_store_dev_ptr(c.handle, C.byref(dt))
    return p, dt.value


def _store_gt(c, Q, k):
    import torch
    qd = _dev(Q)
    ids, d2 = _out(len(Q), k)
    torch.cuda.synchronize()
    c.groundtruth_store_dev(len(Q), qd.data_ptr(), k, ids.data_ptr(), d2.data_ptr())
    c.sync()
    return ids.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("dt", DTYPES)
def test_store_ground_truth_and_metrics_end_to_end(pkg, oracle, dt):
    """the resident store as the base, set from the host and attached from the device: the same as the rows call over the store's own
    pointer, and its ids fed to the metrics over the same typed base give recall 1 and ratio 1"""
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    n, d, nq, k = 3000, 24, 21, 10
    raw, X, Q = scene(dt, n, d, nq, seed=31)
    ref = oracle.groundtruth(X, Q, k)
    with pkg.FspannContext(_cfg(pkg, d), 0) as c:
        c.store_set(raw, dtype=store_kw(pkg, dt))
        p, sdt = _store_ptr(c)
        assert sdt == code(pkg, dt) and p
        got = _store_gt(c, Q, k)
        assert same(got, ref)
        qd = _dev(Q)
        ids, d2 = _out(nq, k)
        torch.cuda.synchronize()
        c.groundtruth_rows_dev(n, p, sdt, nq, qd.data_ptr(), d, k, ids.data_ptr(), d2.data_ptr())
        c.sync()
        assert same(got, (ids.cpu().numpy(), d2.cpu().numpy()))
        # the numpy-level call takes the rows as store_set does
        assert same(c.groundtruth_rows(raw, Q, k, dtype=store_kw(pkg, dt)), ref)
        # end to end: ann = gt over the same typed base and the fp32 queries
        gd = _dev(got[0])
        rec = torch.zeros(nq, dtype=torch.float64, device=dev)
        rat = torch.zeros(nq, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        c.eval_metrics_typed_dev(n, p, sdt, nq, qd.data_ptr(), N.F32, d, k, gd.data_ptr(), k, 0, gd.data_ptr(), k, rec.data_ptr(), rat.data_ptr())
        c.sync()
        rec, rat = rec.cpu().numpy(), rat.cpu().numpy()
        assert (rec == 1.0).all()
        assert (got[1] > 0).all() and not np.isnan(rat).any() and (rat == 1.0).all()      # (no query is a row: the ratio is defined)
        # the same rows, owned by the caller
        own = _dev(_bytes(raw))
        torch.cuda.synchronize()
        c.store_attach_dev(n, own.data_ptr(), code(pkg, dt))
        assert _store_ptr(c) == (own.data_ptr(), code(pkg, dt))
        assert same(_store_gt(c, Q, k), ref)


def test_store_states_and_refused_types(pkg, oracle):
    import torch
    N = pkg._native
    rng = np.random.default_rng(2)
    n, d, nq, k = 500, 16, 6, 5
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    err = lambda: N.lib().fspann_last_error().decode()
    with pkg.FspannContext(_cfg(pkg, d), 0) as c:
        L, h = c.L, c.handle
        qd, xd = _dev(Q), _dev(X)
        ids, d2 = _out(nq, k)
        torch.cuda.synchronize()
        q, b, oi, od = qd.data_ptr(), xd.data_ptr(), ids.data_ptr(), d2.data_ptr()
        assert L.fspann_groundtruth_store_dev(h, nq, q, k, oi, od) == N.E_STATE                   # no store yet
        assert L.fspann_groundtruth_store_dev(h, nq, None, k, oi, od) == N.E_NULL
        assert L.fspann_groundtruth_store_dev(h, nq, q, k, None, od) == N.E_NULL
        c.store_set(X.astype(np.float64))
        assert L.fspann_groundtruth_store_dev(h, nq, q, k, oi, od) == N.E_ARG and "FSPANN_F64" in err()
        # an F32 store, and F32 rows, are fspann_groundtruth_dev
        c.store_set(X)
        ref = f32_gt(c, X, Q, k)
        assert same(ref, oracle.groundtruth(X, Q, k))
        assert same(_store_gt(c, Q, k), ref)
        assert L.fspann_groundtruth_store_dev(h, nq, q, k, oi, None) == N.OK                      # out_d2 may be NULL
        c.sync()
        assert np.array_equal(ids.cpu().numpy(), ref[0])
        c.groundtruth_rows_dev(n, b, N.F32, nq, q, d, k, oi, od)
        c.sync()
        assert same((ids.cpu().numpy(), d2.cpu().numpy()), ref)
        # the rows call: types, buffers and sizes
        rows = lambda dt, n_=n, nq_=nq, d_=d, k_=k, b_=b, q_=q, oi_=oi: L.fspann_groundtruth_rows_dev(h, n_, b_, dt, nq_, q_, d_, k_, oi_, od)
        assert rows(N.F64) == N.E_ARG and "FSPANN_F64" in err()
        assert rows(77) == N.E_ARG and "77" in err()
        for dt in (N.U8, N.I8, N.F16, N.BF16, N.F8E4M3):
            assert rows(dt, b_=None) == N.E_NULL and rows(dt, q_=None) == N.E_NULL and rows(dt, oi_=None) == N.E_NULL
            assert rows(dt, n_=0) == N.E_ARG and rows(dt, n_=1 << 31) == N.E_ARG and rows(dt, d_=0) == N.E_ARG and rows(dt, nq_=-1) == N.E_ARG
            assert rows(dt, k_=0) == N.E_ARG and rows(dt, k_=1025) == N.E_ARG and "k must be in [1, 1024]" in err()
            assert rows(dt, nq_=0) == N.OK
        # the pinned refusals of the file-pair call stand
        gt = lambda bdt, qdt: L.fspann_groundtruth_typed_dev(h, n, b, bdt, nq, q, qdt, d, k, oi, od)
        assert gt(N.F16, N.F32) == N.E_ARG and "no ground truth over FSPANN_F16" in err()
        assert gt(N.U8, N.F32) == N.E_ARG and "Base and query types must match" in err()
        c.sync()
