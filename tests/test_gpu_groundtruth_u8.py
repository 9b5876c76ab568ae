"""GPU: exact ground truth and evaluation metrics over BYTE vectors (FSPANN_U8 base and queries, .bvecs data) —
fspann_groundtruth_typed_dev / fspann_eval_metrics_typed_dev.  The reference reads .bvecs as `buf[i] & 0xFF` and then runs the
same fp64 arithmetic (GroundtruthPrecompute.java:103-108,142-163,218-228; FSA:1027-1032), so the existing oracle over the same
values as float32 is the reference: ids in the same order (ties by lower id) and bit-identical squared distances.  The byte
path computes them as 32-bit integers on the int8 matrix cores; every comparison here is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cfg(pkg, d):
    return pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=max(1, min(d, 128)))


def _gt_typed(pkg, ctx, xd, qd, n, nq, d, k, bdt, qdt, base_ptr=None):
    import torch
    dev = torch.device("cuda", 0)
    ids = torch.full((nq, k), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((nq, k), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.groundtruth_typed_dev(n, xd.data_ptr() if base_ptr is None else base_ptr, bdt, nq, qd.data_ptr(), qdt, d, k, ids.data_ptr(), d2.data_ptr())
    ctx.sync()
    return ids.cpu().numpy(), d2.cpu().numpy()


def _gt8(pkg, X8, Q8, k):
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    with pkg.FspannContext(_cfg(pkg, X8.shape[1]), 0) as ctx:
        xd, qd = torch.from_numpy(X8).to(dev), torch.from_numpy(Q8).to(dev)
        return _gt_typed(pkg, ctx, xd, qd, len(X8), len(Q8), X8.shape[1], k, N.U8, N.U8)


def _check(oracle, X8, Q8, k, ids, d2):
    ref_ids, ref_d2 = oracle.groundtruth(X8.astype(np.float32), Q8.astype(np.float32), k)
    bad = np.flatnonzero((ids != ref_ids).any(1) | (d2 != ref_d2).any(1))
    assert bad.size == 0, (bad[:8], ids[bad[:1]], ref_ids[bad[:1]], d2[bad[:1]], ref_d2[bad[:1]])
    n = len(X8)
    if k > n:
        assert (ids[:, n:] == -1).all() and np.isposinf(d2[:, n:]).all()


# the last shape: n and nq one more than a multiple of the distance kernel's tile (128 base rows x 128 queries, in 32 x 32 MFMA tiles)
@pytest.mark.parametrize("n,d,nq,k", [(5000, 128, 37, 10), (300, 7, 5, 100), (70000, 32, 20, 1), (40, 16, 3, 64), (20000, 100, 16, 100),
                                      (4096, 960, 8, 100), (3000, 128, 1, 1024), (128 * 5 + 1, 64, 128 + 1, 10)])
def test_groundtruth_u8_matches_reference(pkg, oracle, n, d, nq, k):
    rng = np.random.default_rng(n + k)
    X8 = rng.integers(0, 256, (n, d), dtype=np.uint8)
    Q8 = rng.integers(0, 256, (nq, d), dtype=np.uint8)
    ids, d2 = _gt8(pkg, X8, Q8, k)
    _check(oracle, X8, Q8, k, ids, d2)


def test_groundtruth_u8_ties_go_to_the_lower_id(pkg, oracle):
    """Values 0..3 and every vector of the first block twice: equal distances on both sides of the k-th place for most queries."""
    rng = np.random.default_rng(7)
    X8 = rng.integers(0, 4, (3000, 8)).astype(np.uint8)
    X8[1000:2000] = X8[:1000]
    Q8 = rng.integers(0, 4, (25, 8)).astype(np.uint8)
    ids, d2 = _gt8(pkg, X8, Q8, 50)
    _check(oracle, X8, Q8, 50, ids, d2)
    for i in range(len(Q8)):                                  # ascending (distance, id)
        key = list(zip(d2[i], ids[i]))
        assert key == sorted(key)


@pytest.mark.parametrize("d", [960, 100])
def test_groundtruth_u8_extremes(pkg, oracle, d):
    """All-0 and all-255 rows against all-255 and all-0 queries: d2 = d * 65025 (a wrong flip, a K tail padded before the flip
    or a 16-bit overflow shows here); d = 100 goes through the K tail."""
    X8 = np.zeros((300, d), np.uint8)
    X8[1::2] = 255
    Q8 = np.zeros((4, d), np.uint8)
    Q8[[0, 2]] = 255
    ids, d2 = _gt8(pkg, X8, Q8, 200)
    _check(oracle, X8, Q8, 200, ids, d2)
    assert (d2[:, :150] == 0).all() and (d2[:, 150:] == d * 65025).all()
    assert np.array_equal(ids[0, :150], np.arange(1, 300, 2)) and np.array_equal(ids[1, :150], np.arange(0, 300, 2))


def test_groundtruth_u8_misaligned_base(pkg, oracle):
    """A base pointer one byte into its allocation: rows start at odd addresses."""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    rng = np.random.default_rng(11)
    n, d, nq, k = 2500, 128, 9, 20
    X8 = rng.integers(0, 256, (n, d), dtype=np.uint8)
    Q8 = rng.integers(0, 256, (nq, d), dtype=np.uint8)
    with pkg.FspannContext(_cfg(pkg, d), 0) as ctx:
        buf = torch.zeros(n * d + 64, dtype=torch.uint8, device=dev)
        buf[1:1 + n * d] = torch.from_numpy(X8.reshape(-1)).to(dev)
        qd = torch.from_numpy(Q8).to(dev)
        ids, d2 = _gt_typed(pkg, ctx, buf, qd, n, nq, d, k, N.U8, N.U8, base_ptr=buf.data_ptr() + 1)
    _check(oracle, X8, Q8, k, ids, d2)


def test_query_chunks_under_a_small_scratch_budget(pkg, oracle, monkeypatch):
    """FSPANN_GT_SCRATCH_MB = 1: the [chunk x n] matrix holds 32 byte queries / 16 fp32 queries of 8000 rows, so these calls
    take at least three chunks each (the loop over chunks, which no call at the default 8 GiB reaches)."""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    monkeypatch.setenv("FSPANN_GT_SCRATCH_MB", "1")
    rng = np.random.default_rng(5)
    n, k = 8000, 30
    for d, nq in ((128, 100), (100, 70)):                               # aligned rows, and rows that start at odd addresses
        assert -(-nq // max(32, ((1 << 20) // (n * 4)) // 32 * 32)) >= 3
        X8 = rng.integers(0, 256, (n, d), dtype=np.uint8)
        Q8 = rng.integers(0, 256, (nq, d), dtype=np.uint8)
        ids, d2 = _gt8(pkg, X8, Q8, k)
        _check(oracle, X8, Q8, k, ids, d2)
    d, nq = 24, 50
    assert -(-nq // max(16, ((1 << 20) // (n * 8)) // 16 * 16)) >= 3
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    with pkg.FspannContext(_cfg(pkg, d), 0) as ctx:
        xd, qd = torch.from_numpy(X).to(dev), torch.from_numpy(Q).to(dev)
        ids = torch.zeros((nq, k), dtype=torch.int32, device=dev)
        d2 = torch.zeros((nq, k), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.groundtruth_dev(n, xd.data_ptr(), nq, qd.data_ptr(), d, k, ids.data_ptr(), d2.data_ptr())
        ctx.sync()
    ref_ids, ref_d2 = oracle.groundtruth(X, Q, k)
    assert np.array_equal(ids.cpu().numpy(), ref_ids) and np.array_equal(d2.cpu().numpy(), ref_d2)


@pytest.mark.parametrize("n,d,nq,k", [(5000, 128, 37, 10), (300, 7, 5, 100), (70000, 32, 20, 1), (40, 16, 3, 64)])
def test_typed_f32_is_groundtruth_dev(pkg, n, d, nq, k):
    """(F32, F32) through the typed call = fspann_groundtruth_dev, on the data of tests/test_gpu_groundtruth.py."""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    rng = np.random.default_rng(n + k)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    with pkg.FspannContext(_cfg(pkg, d), 0) as ctx:
        xd, qd = torch.from_numpy(X).to(dev), torch.from_numpy(Q).to(dev)
        ids, d2 = _gt_typed(pkg, ctx, xd, qd, n, nq, d, k, N.F32, N.F32)
        ids0 = torch.zeros((nq, k), dtype=torch.int32, device=dev)
        d20 = torch.zeros((nq, k), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.groundtruth_dev(n, xd.data_ptr(), nq, qd.data_ptr(), d, k, ids0.data_ptr(), d20.data_ptr())
        ctx.sync()
    assert np.array_equal(ids, ids0.cpu().numpy()) and np.array_equal(d2, d20.cpu().numpy())


def test_groundtruth_over_the_resident_u8_store(pkg, oracle):
    """fspann_store_dev_ptr of a U8 store is a valid base: recall against the resident store, no second copy."""
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    rng = np.random.default_rng(21)
    n, d, nq, k = 6000, 64, 33, 25
    X8 = rng.integers(0, 256, (n, d), dtype=np.uint8)
    Q8 = rng.integers(0, 256, (nq, d), dtype=np.uint8)
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=d), 0) as ctx:
        ctx.store_set(X8, dtype=np.uint8)
        dt = C.c_int(-1)
        ptr = ctx.L.fspann_store_dev_ptr(ctx.handle, C.byref(dt))
        assert ptr and dt.value == N.U8
        qd = torch.from_numpy(Q8).to(dev)
        ids, d2 = _gt_typed(pkg, ctx, None, qd, n, nq, d, k, N.U8, N.U8, base_ptr=ptr)
        ids2, d22 = ctx.groundtruth(X8, Q8, k)                          # the numpy convenience keeps uint8 arrays as bytes
    _check(oracle, X8, Q8, k, ids, d2)
    assert np.array_equal(ids, ids2) and np.array_equal(d2, d22)


@pytest.mark.parametrize("q_as", ["u8", "f32"])
def test_metrics_u8_match_compute_metrics_at_k(pkg, oracle, q_as):
    """The scene of test_metrics_match_compute_metrics_at_k on byte data, queries as bytes and as fp32."""
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    rng = np.random.default_rng(3)
    n, d, nq, k = 4000, 24, 64, 10
    X8 = rng.integers(0, 256, (n, d), dtype=np.uint8)
    Q8 = rng.integers(0, 256, (nq, d), dtype=np.uint8)
    Q8[5] = X8[17]                                           # distance 0 to its nearest neighbour: ratio is NaN there
    X, Q = X8.astype(np.float32), Q8.astype(np.float32)
    gt, _ = oracle.groundtruth(X, Q, 20)
    ann = gt[:, :12].copy()
    for i in range(nq):                                      # an approximate answer: some true neighbours replaced
        m = rng.random(12) < 0.4
        ann[i, m] = rng.integers(0, n, int(m.sum()))
    cnt = np.full(nq, 12, np.int32)
    cnt[3], cnt[9] = 7, 0                                    # fewer than k results: ratio NaN, recall over what exists
    ann[11, 2] = -1                                          # an unparsable id
    with pkg.FspannContext(_cfg(pkg, d), 0) as ctx:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        xd, ad, cd, gd = t(X8), t(ann), t(cnt), t(gt)
        qd, qdt = (t(Q8), N.U8) if q_as == "u8" else (t(Q), N.F32)
        rec = torch.zeros(nq, dtype=torch.float64, device=dev)
        rat = torch.zeros(nq, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        ctx.eval_metrics_typed_dev(n, xd.data_ptr(), N.U8, nq, qd.data_ptr(), qdt, d, k, ad.data_ptr(), 12, cd.data_ptr(), gd.data_ptr(), 20,
                                   rec.data_ptr(), rat.data_ptr())
        ctx.sync()
        rec, rat = rec.cpu().numpy(), rat.cpu().numpy()
    ref_rec, ref_rat = oracle.metrics(X, Q, k, ann, cnt, gt)
    assert np.array_equal(rec, ref_rec)
    assert np.array_equal(np.isnan(rat), np.isnan(ref_rat)) and np.isnan(rat[[3, 5, 9, 11]]).all()
    ok = ~np.isnan(rat)
    assert ok.sum() == nq - 4 and np.array_equal(rat[ok], ref_rat[ok])


def test_typed_calls_refuse_what_the_reference_refuses(pkg):
    import ctypes as C
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    with pkg.FspannContext(_cfg(pkg, 16), 0) as ctx:
        L, h = ctx.L, ctx.handle
        buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
        out = torch.zeros(4096, dtype=torch.float64, device=dev)
        p, o = buf.data_ptr(), out.data_ptr()
        err = lambda: L.fspann_last_error().decode()
        gt = lambda bdt, qdt, dim=16, k=5, base=p, q=p, ids=o: L.fspann_groundtruth_typed_dev(h, 10, base, bdt, 2, q, qdt, dim, k, ids, o + 16384)
        for bdt, qdt, names in ((N.U8, N.F32, ("FSPANN_U8", "FSPANN_F32")), (N.F32, N.U8, ("FSPANN_F32", "FSPANN_U8")),
                                (N.F64, N.F64, ("FSPANN_F64",)), (N.U8, N.F64, ("FSPANN_U8", "FSPANN_F64"))):
            assert gt(bdt, qdt) == N.E_ARG
            assert "Base and query types must match (both fvecs or both bvecs)" in err() and all(s in err() for s in names), err()
        assert gt(N.U8, N.U8, dim=32769) == N.E_ARG and "32768" in err()
        assert gt(N.U8, N.U8, k=0) == N.E_ARG and gt(N.U8, N.U8, k=1025) == N.E_ARG
        assert gt(N.U8, N.U8, base=None) == N.E_NULL and gt(N.U8, N.U8, q=None) == N.E_NULL and gt(N.U8, N.U8, ids=None) == N.E_NULL
        assert gt(N.U8, N.U8) == N.OK                                  # (the same call with nothing wrong is accepted)
        mt = lambda bdt, qdt, k=5, base=p: L.fspann_eval_metrics_typed_dev(h, 10, base, bdt, 2, p, qdt, 16, k, o, 8, None, o, 8, o, o)
        for bdt, qdt, names in ((N.F32, N.U8, ("FSPANN_F32", "FSPANN_U8")), (N.F64, N.F64, ("FSPANN_F64",)), (N.U8, N.F64, ("FSPANN_F64",))):
            assert mt(bdt, qdt) == N.E_ARG and all(s in err() for s in names), err()
        assert mt(N.U8, N.U8, k=0) == N.E_ARG and mt(N.U8, N.F32, k=1025) == N.E_ARG
        assert mt(N.U8, N.U8, base=None) == N.E_NULL
        ctx.sync()
        with pytest.raises(N.FspannArgumentError):
            ctx.groundtruth(np.zeros((4, 8), np.uint8), np.zeros((2, 8), np.float32), 2)
