"""GPU: the ground truth with the fp32 matrix-core pre-filter (fspann_groundtruth_mfma_dev / _store_dev, method="mfma").  Every
case must EQUAL (np.array_equal: ids and fp64 distance bits) two references: (a) the reference's statements restated in numpy by
this file — float32 difference, fp64 square, sums in dimension order, order by (distance, id) — and (b) the exact call,
method="exact".  Every case but the two ways out also asserts that no query and no call fell back to the exact path: a result that
came from there would show nothing."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "u8", "i8", "f16", "bf16", "f8")
CAP = 4096      # kGtmCap


def typed(dt, g):
    """Gaussian draws g -> (rows of type dt as the library takes them, the float32 values they are)"""
    import torch
    if dt == "u8":
        raw = np.clip(np.rint(128 + 32 * g), 0, 255).astype(np.uint8)
    elif dt == "i8":
        raw = np.clip(np.rint(32 * g), -128, 127).astype(np.int8)
    elif dt == "f16":
        raw = g.astype(np.float16)
    elif dt == "bf16":
        raw = (np.ascontiguousarray(g, np.float32).view(np.uint32) >> 16).astype(np.uint16)
        return raw, (raw.astype(np.uint32) << 16).view(np.float32)
    elif dt == "f8":
        t = torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(torch.float8_e4m3fn)
        return t.view(torch.uint8).numpy().copy(), t.to(torch.float32).numpy()
    else:
        raw = np.ascontiguousarray(g, np.float32)
    return raw, raw.astype(np.float32)


def kw(pkg, dt):
    return dict(f32=np.float32, u8=np.uint8, i8=np.int8, f16=np.float16, bf16=pkg.bfloat16, f8=pkg.float8_e4m3fn)[dt]


def ref_a(X, Q, k):
    """reference (a): GroundtruthPrecompute's arithmetic and order, in numpy"""
    n, ids = len(X), np.arange(len(X))
    s = np.zeros((len(Q), n))
    for i in range(X.shape[1]):
        df = Q[:, i, None] - X[None, :, i]                  # float32 - float32
        s = s + df.astype(np.float64) ** 2
    out_i, out_d = np.full((len(Q), k), -1, np.int32), np.full((len(Q), k), np.inf)
    for j in range(len(Q)):
        o = np.lexsort((ids, s[j]))[:k]
        out_i[j, :len(o)], out_d[j, :len(o)] = o, s[j, o]
    return out_i, out_d


@functools.lru_cache(maxsize=None)
def scene(dt, n, d, nq, k, seed=0):
    """rows, their values, fp32 queries on the rows' scale, and reference (a)"""
    rng = np.random.default_rng(seed)
    raw, X = typed(dt, rng.standard_normal((n, d), dtype=np.float32))
    gq = rng.standard_normal((nq, d), dtype=np.float32)
    Q = (128 + 32 * gq if dt == "u8" else 32 * gq if dt == "i8" else gq).astype(np.float32)
    return raw, X, Q, ref_a(X, Q, k)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def both(pkg, c, dt, raw, Q, k, ref, fell_back=False):
    """method="mfma" equals reference (a) (when given) and reference (b); returns its stats"""
    got = c.groundtruth_rows(raw, Q, k, dtype=kw(pkg, dt), method="mfma")
    st = c.last_gt_stats
    assert ref is None or same(got, ref)
    assert same(got, c.groundtruth_rows(raw, Q, k, dtype=kw(pkg, dt), method="exact"))
    if not fell_back:
        assert st["queries_exact"] == 0 and st["whole_call_exact"] == 0 and st["queries_fast"] == len(Q), st
    return st


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=16), 0) as c:
        yield c


# (4096,128,130): 32 base tiles, a partial second query block.  (1500,5): element loads, k near n.  (37,8): k > n, padding.
SHAPES = [(2000, 32, 33, 10), (4096, 128, 130, 100), (1500, 5, 3, 1024), (129, 16, 1, 1), (37, 8, 5, 100)]


@pytest.mark.parametrize("n,d,nq,k", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_equals_both_references(pkg, ctx, dt, n, d, nq, k):
    raw, X, Q, ref = scene(dt, n, d, nq, k)
    st = both(pkg, ctx, dt, raw, Q, k, ref)
    assert k <= st["survivors_max"] or n < k
    if (n, d) == (2000, 32):
        assert st["survivors_max"] < n // 2, st        # the pre-filter filters
    if k > n:
        got = ctx.groundtruth_rows(raw, Q, k, dtype=kw(pkg, dt), method="mfma")
        assert (got[0][:, n:] == -1).all() and np.isposinf(got[1][:, n:]).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_ties_across_the_cut_go_to_the_lower_id(pkg, ctx, dt):
    """40 copies of one row over both base tiles of n = 300, the query next to it, k = 20: the 20 lowest copies, in id order"""
    raw, X, Q, _ = scene(dt, 300, 16, 4, 1)
    raw, X = raw.copy(), X.copy()
    copies = np.arange(3, 300, 7)[:40]
    raw[copies], X[copies] = raw[3], X[3]
    Q = (X[3][None, :] + np.float32(0.125) * np.arange(1, 5, dtype=np.float32)[:, None]).astype(np.float32)
    ref = ref_a(X, Q, 20)
    assert copies.max() >= 128 and (ref[0] == copies[:20]).all()
    both(pkg, ctx, dt, raw, Q, 20, ref)


def mfma_dev(pkg, c, dt, raw, Q, k, offset_elems):
    """fspann_groundtruth_mfma_dev with the base `offset_elems` elements into a 16-byte aligned buffer"""
    import torch
    N, dev = pkg._native, torch.device("cuda", 0)
    b = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    off = offset_elems * raw.dtype.itemsize
    buf = torch.zeros(off + b.size + 16, dtype=torch.uint8, device=dev)
    buf[off:off + b.size] = torch.from_numpy(b).to(dev)
    qd = torch.from_numpy(Q).to(dev)
    ids, d2 = torch.full((len(Q), k), -7, dtype=torch.int32, device=dev), torch.full((len(Q), k), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    code = dict(f32=N.F32, u8=N.U8, i8=N.I8, f16=N.F16, bf16=N.BF16, f8=N.F8E4M3)[dt]
    c.groundtruth_mfma_dev(raw.shape[0], buf.data_ptr() + off, code, len(Q), qd.data_ptr(), raw.shape[1], k, ids.data_ptr(), d2.data_ptr())
    c.sync()
    return ids.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("n,d,off", [(1000, 32, 1), (500, 7, 0)])
@pytest.mark.parametrize("dt", DTYPES)
def test_unaligned_rows_take_element_loads(pkg, ctx, dt, n, d, off):
    raw, X, Q, ref = scene(dt, n, d, 19, 10)
    assert same(mfma_dev(pkg, ctx, dt, raw, Q, 10, off), ref)
    st = ctx.last_gt_stats
    assert st["queries_exact"] == 0 and st["whole_call_exact"] == 0


@pytest.mark.parametrize("dt", ("f32", "u8", "bf16"))
def test_queries_run_in_chunks_under_a_small_scratch_budget(pkg, monkeypatch, dt):
    """1 MiB holds 32 queries' estimates of 4000 rows and their lists: 100 queries are 4 chunks, the last a tail"""
    monkeypatch.setenv("FSPANN_GT_SCRATCH_MB", "1")
    raw, X, Q, ref = scene(dt, 4000, 16, 100, 10)
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=16), 0) as c:
        both(pkg, c, dt, raw, Q, 10, ref)


@pytest.mark.parametrize("dt", ("f32", "u8"))
def test_way_out_of_a_query_with_too_many_survivors(pkg, ctx, dt):
    """more identical rows than a list holds: every query is finished by the exact path"""
    raw, X, Q, _ = scene(dt, 8, 8, 3, 10)
    raw, X = np.repeat(raw[:1], CAP + 200, axis=0), np.repeat(X[:1], CAP + 200, axis=0)
    st = both(pkg, ctx, dt, raw, Q, 10, ref_a(X, Q, 10), fell_back=True)
    assert st["queries_exact"] == len(Q) and st["queries_fast"] == 0 and st["whole_call_exact"] == 0 and st["survivors_max"] == CAP + 200


@pytest.mark.parametrize("dt", ("f32", "f16", "bf16"))
def test_way_out_of_a_call_with_nonfinite_rows(pkg, ctx, dt):
    """one NaN row and one row with +inf and -inf: the whole call goes to the exact path (k small: no NaN distance is returned)"""
    raw, X, Q, _ = scene(dt, 600, 16, 7, 10)
    raw = raw.copy()
    bits = raw.view(np.uint32 if dt == "f32" else np.uint16)
    nan, pinf, ninf = dict(f32=(0x7FC00000, 0x7F800000, 0xFF800000), f16=(0x7E00, 0x7C00, 0xFC00), bf16=(0x7FC0, 0x7F80, 0xFF80))[dt]
    bits[17, 3], bits[400, 0], bits[400, 9] = nan, pinf, ninf
    st = both(pkg, ctx, dt, raw, Q, 10, None, fell_back=True)
    assert st["whole_call_exact"] == 1 and st["queries_fast"] == 0


@pytest.mark.parametrize("dt", ("f16", "u8"))
def test_store_call(pkg, dt):
    raw, X, Q, ref = scene(dt, 3000, 24, 21, 10)
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=24), 0) as c:
        c.store_set(raw, dtype=kw(pkg, dt))
        got = c.groundtruth_store(Q, 10, method="mfma")
        st = c.last_gt_stats
        assert same(got, ref) and same(got, c.groundtruth_store(Q, 10))
        assert st["queries_exact"] == 0 and st["whole_call_exact"] == 0 and st["queries_fast"] == len(Q)
