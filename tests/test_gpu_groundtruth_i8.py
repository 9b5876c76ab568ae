"""GPU: exact ground truth over SIGNED byte vectors (FSPANN_I8 base and queries, values -128..127) —
fspann_groundtruth_typed_dev with the pair (FSPANN_I8, FSPANN_I8).  Sums of squares of differences of such values are integers
below 2^31 for dim <= 32768, exact in fp64 in any order, so the oracle over the same values as float32 is the reference: ids in the
same order (ties by lower id) and bit-identical squared distances.  The signed path computes them as 32-bit integers on the int8
matrix cores without the unsigned path's sign flip; every comparison here is exact (np.array_equal), nothing has a tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cfg(pkg, d):
    return pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=max(1, min(d, 128)))


def _gt_typed(ctx, base_ptr, q_ptr, n, nq, d, k, bdt, qdt):
    import torch
    dev = torch.device("cuda", 0)
    ids = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.groundtruth_typed_dev(n, base_ptr, bdt, nq, q_ptr, qdt, d, k, ids.data_ptr(), d2.data_ptr())
    ctx.sync()
    return ids.cpu().numpy(), d2.cpu().numpy()


def _gts(pkg, X8, Q8, k):
    """(I8, I8) over int8 arrays"""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    assert X8.dtype == np.int8 and Q8.dtype == np.int8
    with pkg.FspannContext(_cfg(pkg, X8.shape[1]), 0) as ctx:
        xd, qd = torch.from_numpy(X8).to(dev), torch.from_numpy(Q8).to(dev)
        return _gt_typed(ctx, xd.data_ptr(), qd.data_ptr(), len(X8), len(Q8), X8.shape[1], k, N.I8, N.I8)


def _check(oracle, X8, Q8, k, ids, d2):
    ref_ids, ref_d2 = oracle.groundtruth(X8.astype(np.float32), Q8.astype(np.float32), k)
    bad = np.flatnonzero((ids != ref_ids).any(1) | (d2 != ref_d2).any(1))
    assert bad.size == 0, (bad[:8], ids[bad[:1]], ref_ids[bad[:1]], d2[bad[:1]], ref_d2[bad[:1]])
    n = len(X8)
    if k > n:
        assert (ids[:, n:] == -1).all() and np.isposinf(d2[:, n:]).all()


def _draw(rng, n, d):
    """values over the whole range, with rows of all -128, all 127 and all -1 in every scene"""
    X = rng.integers(-128, 128, (n, d), dtype=np.int8)
    for r, v in zip(rng.choice(n, 3, replace=False) if n >= 3 else range(n), (-128, 127, -1)):
        X[r] = v
    return X


# k > n; d below one slot; n and nq one more than a multiple of the distance kernel's tile (128 base rows x 128 queries, in 32 x 32
# MFMA tiles); many K steps; the largest k; rows that start at odd addresses with a K tail (d = 100)
@pytest.mark.parametrize("n,d,nq,k", [(300, 7, 5, 100), (40, 16, 3, 64), (128 * 5 + 1, 64, 128 + 1, 10), (4096, 960, 8, 100),
                                      (3000, 128, 1, 1024), (20000, 100, 16, 100)])
def test_groundtruth_i8_matches_reference(pkg, oracle, n, d, nq, k):
    rng = np.random.default_rng(n + k)
    X8, Q8 = _draw(rng, n, d), _draw(rng, nq, d)
    ids, d2 = _gts(pkg, X8, Q8, k)
    _check(oracle, X8, Q8, k, ids, d2)


@pytest.mark.parametrize("d", [960, 100])
def test_groundtruth_i8_extremes(pkg, oracle, d):
    """All -128 and all 127 rows against all 127 and all -128 queries: d2 = d * 65025 — a byte read as unsigned, a K tail padded
    with anything but 0, a 16-bit overflow or a wrapped intermediate that did not wrap back shows here; d = 100 goes through the K
    tail."""
    X8 = np.full((300, d), -128, np.int8)
    X8[1::2] = 127
    Q8 = np.full((4, d), -128, np.int8)
    Q8[[0, 2]] = 127
    ids, d2 = _gts(pkg, X8, Q8, 200)
    _check(oracle, X8, Q8, 200, ids, d2)
    assert (d2[:, :150] == 0).all() and (d2[:, 150:] == d * 65025).all()
    assert np.array_equal(ids[0, :150], np.arange(1, 300, 2)) and np.array_equal(ids[1, :150], np.arange(0, 300, 2))


def test_groundtruth_i8_ties_go_to_the_lower_id(pkg, oracle):
    """Values -2..1 and every vector of the first block twice: equal distances on both sides of the k-th place for most queries."""
    rng = np.random.default_rng(7)
    X8 = rng.integers(-2, 2, (3000, 8)).astype(np.int8)
    X8[1000:2000] = X8[:1000]
    Q8 = rng.integers(-2, 2, (25, 8)).astype(np.int8)
    ids, d2 = _gts(pkg, X8, Q8, 50)
    _check(oracle, X8, Q8, 50, ids, d2)
    for i in range(len(Q8)):                                  # ascending (distance, id)
        key = list(zip(d2[i], ids[i]))
        assert key == sorted(key)


def test_groundtruth_i8_misaligned_base(pkg, oracle):
    """A base pointer one byte into its allocation: rows start at odd addresses (the byte-load instantiation)."""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    rng = np.random.default_rng(11)
    n, d, nq, k = 2500, 128, 9, 20
    X8, Q8 = _draw(rng, n, d), _draw(rng, nq, d)
    with pkg.FspannContext(_cfg(pkg, d), 0) as ctx:
        buf = torch.zeros(n * d + 64, dtype=torch.int8, device=dev)
        buf[1:1 + n * d] = torch.from_numpy(X8.reshape(-1)).to(dev)
        qd = torch.from_numpy(Q8).to(dev)
        ids, d2 = _gt_typed(ctx, buf.data_ptr() + 1, qd.data_ptr(), n, nq, d, k, N.I8, N.I8)
    _check(oracle, X8, Q8, k, ids, d2)


def test_query_chunks_under_a_small_scratch_budget(pkg, oracle, monkeypatch):
    """FSPANN_GT_SCRATCH_MB = 1 (read when the context is made): the [chunk x n] matrix holds 32 byte queries of 8000 rows, so 100
    queries take at least three chunks (the loop over chunks, which no call at the default 8 GiB reaches)."""
    monkeypatch.setenv("FSPANN_GT_SCRATCH_MB", "1")
    rng = np.random.default_rng(5)
    n, nq, k = 8000, 100, 30
    assert -(-nq // max(32, ((1 << 20) // (n * 4)) // 32 * 32)) >= 3
    for d in (128, 100):                                                # aligned rows, and rows that start at odd addresses
        X8, Q8 = _draw(rng, n, d), _draw(rng, nq, d)
        ids, d2 = _gts(pkg, X8, Q8, k)
        _check(oracle, X8, Q8, k, ids, d2)


def test_groundtruth_over_the_resident_i8_store(pkg, oracle):
    """fspann_store_dev_ptr of an I8 store is a valid base (no second copy), and the numpy convenience keeps int8 arrays as bytes."""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    rng = np.random.default_rng(21)
    n, d, nq, k = 6000, 64, 33, 25
    X8, Q8 = _draw(rng, n, d), _draw(rng, nq, d)
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=d), 0) as ctx:
        ctx.store_set(X8, dtype=np.int8)
        dt = C.c_int(-1)
        ptr = ctx.L.fspann_store_dev_ptr(ctx.handle, C.byref(dt))
        assert ptr and dt.value == N.I8
        qd = torch.from_numpy(Q8).to(dev)
        ids, d2 = _gt_typed(ctx, ptr, qd.data_ptr(), n, nq, d, k, N.I8, N.I8)
        ids2, d22 = ctx.groundtruth(X8, Q8, k)
        with pytest.raises(N.FspannArgumentError):
            ctx.groundtruth(X8, Q8.view(np.uint8), k)                   # signed with unsigned: a pair that does not match
        with pytest.raises(N.FspannArgumentError):
            ctx.groundtruth(X8, Q8.astype(np.float32), k)
    _check(oracle, X8, Q8, k, ids, d2)
    assert np.array_equal(ids, ids2) and np.array_equal(d2, d22)


@pytest.mark.parametrize("n,d,nq,k", [(5000, 128, 37, 10), (2000, 100, 130, 64)])
def test_shifted_scene_through_the_unsigned_path_agrees(pkg, n, d, nq, k):
    """A cross-check that needs no oracle: distances between vectors survive a shift, so base + 128 and queries + 128 through the
    existing (U8, U8) path give the ids and the d2 of the signed path over the scene itself."""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    rng = np.random.default_rng(n + d)
    X8, Q8 = _draw(rng, n, d), _draw(rng, nq, d)
    Xu, Qu = (X8.astype(np.int16) + 128).astype(np.uint8), (Q8.astype(np.int16) + 128).astype(np.uint8)
    assert np.array_equal(Xu, X8.view(np.uint8) ^ 0x80)
    ids, d2 = _gts(pkg, X8, Q8, k)
    with pkg.FspannContext(_cfg(pkg, d), 0) as ctx:
        xd, qd = torch.from_numpy(Xu).to(dev), torch.from_numpy(Qu).to(dev)
        idu, d2u = _gt_typed(ctx, xd.data_ptr(), qd.data_ptr(), n, nq, d, k, N.U8, N.U8)
    assert np.array_equal(ids, idu) and np.array_equal(d2, d2u)
    assert (d2 >= 0).all() and d2.max() <= d * 65025
