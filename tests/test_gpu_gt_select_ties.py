"""GPU: the exact k-NN selection (gt_select_kernel over fp64 keys, gt8_select_kernel over uint32 keys) where ties decide: whole
groups of rows at one distance, so that the id digits of the radix walk choose the result -- the third and fourth id byte included,
which need n > 65536 and n > 2^24 -- the boundary at which gt8_select_kernel may skip the id digits (k = the size of the tie group,
and one to either side), keys that differ in their low mantissa bytes only, k = 1024, non-finite distances and the tile edges of
gt_dist_kernel.  Cases a, b and c hold small integers, which every row type holds, and run through five callers: groundtruth_dev
(F32), groundtruth_rows_dev with F16 and with U8 rows and fp32 queries (gt_dist_kernel over typed rows, 16 bytes at a time where a row is a
whole number of 16-byte pieces and by element otherwise, then gt_select_kernel), and groundtruth_typed_dev over (U8, U8) and
(I8, I8) (gt8_select_kernel).  Expected values come from tests/gt_ref.py's knn() -- which tests/test_gt_ref_cpu.py holds against the
oracle on the same data sets -- and, where the data set has one, from the closed form of the ids.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import gt_ref as R

pytestmark = pytest.mark.gpu

CALLERS = ("f32", "rows_f16", "rows_u8", "u8u8", "i8i8")


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=16), 0) as c:
        yield c


def _call(pkg, ctx, caller, xd, qd, n, nq, d, k):
    """xd / qd: device tensors of the caller's types"""
    import torch
    N = pkg._native
    dev = torch.device("cuda", 0)
    ids = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    x, q, i, o = xd.data_ptr(), qd.data_ptr(), ids.data_ptr(), d2.data_ptr()
    if caller == "f32":
        ctx.groundtruth_dev(n, x, nq, q, d, k, i, o)
    elif caller == "f32_typed":
        ctx.groundtruth_typed_dev(n, x, N.F32, nq, q, N.F32, d, k, i, o)
    elif caller == "rows_f16":
        ctx.groundtruth_rows_dev(n, x, N.F16, nq, q, d, k, i, o)
    elif caller == "rows_u8":
        ctx.groundtruth_rows_dev(n, x, N.U8, nq, q, d, k, i, o)
    elif caller == "u8u8":
        ctx.groundtruth_typed_dev(n, x, N.U8, nq, q, N.U8, d, k, i, o)
    else:
        ctx.groundtruth_typed_dev(n, x, N.I8, nq, q, N.I8, d, k, i, o)
    ctx.sync()
    return ids.cpu().numpy(), d2.cpu().numpy()


ROW_T = dict(f32=np.float32, f32_typed=np.float32, rows_f16=np.float16, rows_u8=np.uint8, u8u8=np.uint8, i8i8=np.int8)
QRY_T = dict(f32=np.float32, f32_typed=np.float32, rows_f16=np.float32, rows_u8=np.float32, u8u8=np.uint8, i8i8=np.int8)


def _gt(pkg, ctx, caller, V, Q, k):
    """V, Q: float32 values (small integers unless the caller is fp32); each caller gets them in its own types"""
    import torch
    dev = torch.device("cuda", 0)
    xr, qr = V.astype(ROW_T[caller]), Q.astype(QRY_T[caller])
    assert np.array_equal(xr.astype(np.float32), V, equal_nan=True) and np.array_equal(qr.astype(np.float32), Q, equal_nan=True)
    xd, qd = torch.from_numpy(xr).to(dev), torch.from_numpy(qr).to(dev)
    return _call(pkg, ctx, caller, xd, qd, len(V), len(Q), V.shape[1], k)


def _exact(got, ids, d2, what):
    assert np.array_equal(got[0], ids), (what, np.argwhere(got[0] != ids)[:4])
    assert np.array_equal(got[1].view(np.uint64), d2.view(np.uint64)), (what, np.argwhere(got[1] != d2)[:4])


@functools.lru_cache(maxsize=None)
def _ref(name, *args):
    """knn() at the largest k of a data set, once: a smaller k is its prefix (and -1 / +inf beyond n)"""
    V, Q = getattr(R, name)(*args)
    return (V, Q) + R.knn(V, Q, 1024)


def _prefix(ref, k):
    return ref[2][:, :k], ref[3][:, :k]


# ---- a. all rows identical ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.S_IDENT_N)
@pytest.mark.parametrize("caller", CALLERS)
def test_all_rows_identical(pkg, ctx, caller, n):
    ref = _ref("sel_identical", n)
    for k in R.S_IDENT_K:
        got = _gt(pkg, ctx, caller, ref[0], ref[1], k)
        _exact(got, *_prefix(ref, k), (caller, n, k))
        kk = min(k, n)
        assert (got[0][:, :kk] == np.arange(kk)).all() and (got[0][:, kk:] == -1).all() and np.isposinf(got[1][:, kk:]).all()


# ---- b. a tie group across the 2-byte id boundary -------------------------------------------------------------------------------------
@pytest.mark.parametrize("caller", CALLERS)
def test_tie_group_across_the_two_byte_id_boundary(pkg, ctx, caller):
    """700 identical nearest rows at ids [65400, 66100) of 66800: k = 136 / 137 end at ids 65535 / 65536, k = 700 takes the whole
    group (gt8_select_kernel then skips the id digits), 699 and 701 sit either side, 1000 adds the 300 lowest far ids; 17 queries
    are two query tiles, one ragged; to query 5 the far rows are the nearer ones"""
    ref = _ref("sel_boundary")
    for k in R.S_BOUND_K:
        got = _gt(pkg, ctx, caller, ref[0], ref[1], k)
        _exact(got, *_prefix(ref, k), (caller, k))
        for i in range(len(ref[1])):
            assert np.array_equal(got[0][i], R.sel_boundary_ids(k, i == R.S_BOUND_FARQ)), (caller, k, i)


# ---- c. the top id byte -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (100, 400))
@pytest.mark.parametrize("caller", CALLERS)
def test_the_top_id_byte(pkg, ctx, caller, k):
    """n = 2^24 + 300, the smallest at which the most significant id digit of a tie is not zero: rows [0, 2^24) hold ones, the last
    300 zeros, the queries are zeros.  k = 100: ids 2^24 .. 2^24 + 99; k = 400: those 300, then ids 0 .. 99 (a tie of 2^24 rows,
    cut by id).  About 2.1 GiB of ground-truth scratch per call, within the default budget."""
    import torch
    dev = torch.device("cuda", 0)
    tt = {np.float32: torch.float32, np.float16: torch.float16, np.uint8: torch.uint8, np.int8: torch.int8}
    n, nq = R.S_TOP_N, 2
    d = 1 if caller in ("f32", "rows_f16") else 16
    xd = torch.ones((n, d), dtype=tt[ROW_T[caller]], device=dev)
    xd[n - R.S_TOP_ZEROS:] = 0
    qd = torch.zeros((nq, d), dtype=tt[QRY_T[caller]], device=dev)
    ids, d2 = _call(pkg, ctx, caller, xd, qd, n, nq, d, k)
    want = R.sel_top_ids(k)
    assert want[0] == 2 ** 24 and want[min(k, 300) - 1] == 2 ** 24 + min(k, 300) - 1 and (k <= 300 or (want[300:] == np.arange(k - 300)).all())
    for i in range(nq):
        assert np.array_equal(ids[i], want), (caller, k, i, ids[i][:4], ids[i][-4:])
        assert (d2[i, :300] == 0).all() and (d2[i, 300:] == d).all()


# ---- d. keys that differ in the low mantissa bytes only ---------------------------------------------------------------------------------
def test_keys_that_differ_in_the_low_mantissa_bytes(pkg, ctx):
    """d2 = 1 + j^2 2^-52: the radix walk passes five or six equal top digits before one decides; a row equal to the query (key 0),
    rows a float subnormal away from it, and a row whose d2 rounds to the 1.0 of another (a tie by id)"""
    ref = _ref("sel_mantissa")
    for k in R.S_MANT_K:
        _exact(_gt(pkg, ctx, "f32", ref[0], ref[1], k), *_prefix(ref, k), k)
    assert ref[2][0, 0] == 17 and ref[3][0, 1] > 0 and list(ref[2][0, 1:3]) == [2501, 2500]


# ---- e. k = 1024 in the fp32 path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("normal", "ints"))
def test_k_1024_over_fp32(pkg, ctx, kind):
    for n in R.S_K1024_N + (1, 300):                        # (1 and 300: k > n)
        ref = _ref("sel_k1024", n, kind)
        got = _gt(pkg, ctx, "f32", ref[0], ref[1], 1024)
        _exact(got, ref[2], ref[3], (kind, n))
        assert n >= 1024 or ((got[0][:, n:] == -1).all() and np.isposinf(got[1][:, n:]).all())


# ---- f. non-finite distances in the fp32 path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("caller", ("f32", "f32_typed"))
def test_nonfinite_distances_over_fp32(pkg, ctx, caller):
    """+inf distances (an overflowing float subtraction, or an infinite element) tie by id; NaN distances come last.  Exact up to
    the start of the NaN tail; the tail holds exactly the NaN rows, in any order (nothing pins a NaN's sign or payload, which is
    all that orders them: the convention of tests/test_gpu_groundtruth_rows.py)"""
    V, Q = R.sel_nonfinite()
    n = len(V)
    ids, d2, nan0 = R.knn(V, Q, n)
    got = _gt(pkg, ctx, caller, V, Q, n)
    assert np.isposinf(d2).any() and (nan0 < n).all()
    for i in range(len(Q)):
        m = nan0[i]
        _exact((got[0][i, :m], got[1][i, :m]), ids[i, :m], d2[i, :m], (caller, i))
        assert np.isnan(got[1][i, m:]).all() and np.array_equal(np.sort(got[0][i, m:]), np.sort(ids[i, m:])), (caller, i)


# ---- g. tile edges of gt_dist_kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", R.S_TILE_NQ)
def test_tile_edges_of_the_distance_kernel(pkg, ctx, nq):
    for n in R.S_TILE_N:
        for d in R.S_TILE_D:
            V, Q = R.sel_tiles(nq, n, d)
            ids, d2, _ = R.knn(V, Q, 4)
            _exact(_gt(pkg, ctx, "f32", V, Q, 4), ids, d2, (nq, n, d))
