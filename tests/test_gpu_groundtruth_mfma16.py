"""GPU: the ground truth with the pre-filter on the 16-bit matrix cores (fspann_groundtruth_mfma16_dev / _store_dev,
method="mfma16").  As in test_gpu_groundtruth_mfma.py, whose numpy restatement of the reference's chain this file imports, every
case must EQUAL (np.array_equal: ids and fp64 distance bits) that restatement and method="exact", and every case but the ways out
asserts that no query and no call fell back to the exact path."""
import numpy as np
import pytest

from test_gpu_groundtruth_mfma import CAP, kw, ref_a, same, scene

pytestmark = pytest.mark.gpu

DTYPES = ("u8", "i8", "f16", "bf16", "f8")
BITS = dict(f16=(0x7E00, 0x7C00, 0xFC00), bf16=(0x7FC0, 0x7F80, 0xFF80))      # NaN, +inf, -inf


def both(pkg, c, dt, raw, Q, k, ref, fell_back=False):
    """method="mfma16" equals reference (a) (when given) and reference (b); returns its stats"""
    got = c.groundtruth_rows(raw, Q, k, dtype=kw(pkg, dt), method="mfma16")
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


# (4096,128,130): 16 base tiles, a partial second query block.  (1500,5): d below one operand, element loads.  (37,8): k > n, padding.
# (700,24): a K step that is half zeros (two-byte rows), element loads of one and a half pieces (one-byte rows).
SHAPES = [(2000, 32, 33, 10), (4096, 128, 130, 100), (1500, 5, 3, 1024), (129, 16, 1, 1), (37, 8, 5, 100), (700, 24, 9, 10)]


@pytest.mark.parametrize("n,d,nq,k", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_equals_both_references(pkg, ctx, dt, n, d, nq, k):
    raw, X, Q, ref = scene(dt, n, d, nq, k)
    st = both(pkg, ctx, dt, raw, Q, k, ref)
    assert k <= st["survivors_max"] or n < k
    if (n, d) == (2000, 32):
        assert st["survivors_max"] < n // 2, st        # the pre-filter filters
    if k > n:
        got = ctx.groundtruth_rows(raw, Q, k, dtype=kw(pkg, dt), method="mfma16")
        assert (got[0][:, n:] == -1).all() and np.isposinf(got[1][:, n:]).all()


@pytest.mark.parametrize("dt", DTYPES)
def test_ties_across_the_cut_go_to_the_lower_id(pkg, ctx, dt):
    """40 copies of one row spread over n = 300, the query next to it, k = 20: the 20 lowest copies, in id order"""
    raw, X, Q, _ = scene(dt, 300, 16, 4, 1)
    raw, X = raw.copy(), X.copy()
    copies = np.arange(3, 300, 7)[:40]
    raw[copies], X[copies] = raw[3], X[3]
    Q = (X[3][None, :] + np.float32(0.125) * np.arange(1, 5, dtype=np.float32)[:, None]).astype(np.float32)
    ref = ref_a(X, Q, 20)
    assert (ref[0] == copies[:20]).all()
    both(pkg, ctx, dt, raw, Q, 20, ref)


def values(dt, raw):
    return raw.astype(np.float32) if dt != "bf16" else (raw.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_the_split_keeps_what_no_16_bit_value_holds(pkg, ctx, dt):
    """300 rows that are one row with +-1 ulp in three coordinates each; the queries are that row widened plus low fp32 bits"""
    rng = np.random.default_rng(5)
    raw0, X0, _, _ = scene(dt, 8, 32, 1, 1)
    bits = np.repeat(raw0[:1].view(np.uint16), 300, axis=0)
    for i in range(1, 300):
        at = rng.choice(32, 3, replace=False)
        bits[i, at] += rng.choice(np.array([1, 0xFFFF], np.uint16), 3)      # (+-1 on the pattern: one ulp of a finite non-zero value)
    raw = bits.view(raw0.dtype)
    low = rng.integers(0, 1 << (13 if dt == "f16" else 16), (6, 32), dtype=np.uint32)
    Q = (np.repeat(X0[:1], 6, axis=0).view(np.uint32) | low).view(np.float32)
    both(pkg, ctx, dt, raw, Q, 20, ref_a(values(dt, raw), Q, 20))


@pytest.mark.parametrize("case", ("up", "down", "subnormal", "largest"))
@pytest.mark.parametrize("dt", ("f16", "u8"))
def test_the_scale_of_the_queries(pkg, ctx, dt, case):
    """queries times 2^40 and 2^-40, one all-zero query among them; f16 rows holding subnormal halves, and +-65504"""
    raw, X, Q, _ = scene(dt, 2000, 32, 33, 10)
    raw, Q = raw.copy(), (Q * np.float32(2.0 ** dict(up=40, down=-40).get(case, 0))).astype(np.float32)
    Q[7] = 0
    if dt == "f16" and case == "subnormal":
        raw.view(np.uint16)[10:60, ::3] = np.arange(1, 551, dtype=np.uint16).reshape(50, 11) ^ np.uint16(0x8000) * (np.arange(11, dtype=np.uint16) & 1)
    if dt == "f16" and case == "largest":
        raw.view(np.uint16)[5], raw.view(np.uint16)[6, ::2] = 0x7BFF, 0xFBFF
    st = both(pkg, ctx, dt, raw, Q, 10, ref_a(values(dt, raw), Q, 10))
    if case == "subnormal":
        assert st["survivors_max"] < 1000, st


def mfma16_dev(pkg, c, dt, raw, Q, k, offset_elems):
    """fspann_groundtruth_mfma16_dev with the base `offset_elems` elements into a 16-byte aligned buffer"""
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
    c.groundtruth_mfma16_dev(raw.shape[0], buf.data_ptr() + off, code, len(Q), qd.data_ptr(), raw.shape[1], k, ids.data_ptr(), d2.data_ptr())
    c.sync()
    return ids.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("n,d,off", [(1000, 32, 1), (500, 7, 0)])
@pytest.mark.parametrize("dt", DTYPES)
def test_unaligned_rows_take_element_loads(pkg, ctx, dt, n, d, off):
    raw, X, Q, ref = scene(dt, n, d, 19, 10)
    assert same(mfma16_dev(pkg, ctx, dt, raw, Q, 10, off), ref)
    st = ctx.last_gt_stats
    assert st["queries_exact"] == 0 and st["whole_call_exact"] == 0 and st["queries_fast"] == 19


@pytest.mark.parametrize("dt", ("u8", "f16", "bf16"))
def test_queries_run_in_chunks_under_a_small_scratch_budget(pkg, monkeypatch, dt):
    """1 MiB holds 32 queries' estimates of 4000 rows, their lists and their terms: 100 queries are 4 chunks, the last a tail"""
    monkeypatch.setenv("FSPANN_GT_SCRATCH_MB", "1")
    raw, X, Q, ref = scene(dt, 4000, 16, 100, 10)
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=16), 0) as c:
        both(pkg, c, dt, raw, Q, 10, ref)


@pytest.mark.parametrize("dt", ("u8", "f16"))
def test_way_out_of_a_query_with_too_many_survivors(pkg, ctx, dt):
    """more identical rows than a list holds: every query is finished by the exact path"""
    raw, X, Q, _ = scene(dt, 8, 8, 3, 10)
    raw, X = np.repeat(raw[:1], CAP + 200, axis=0), np.repeat(X[:1], CAP + 200, axis=0)
    st = both(pkg, ctx, dt, raw, Q, 10, ref_a(X, Q, 10), fell_back=True)
    assert st["queries_exact"] == len(Q) and st["queries_fast"] == 0 and st["whole_call_exact"] == 0 and st["survivors_max"] == CAP + 200


@pytest.mark.parametrize("what", ("rows", "query"))
@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_way_out_of_a_call_with_nonfinite_values(pkg, ctx, dt, what):
    """a NaN row and a row with +inf and -inf, or a NaN query: the whole call goes to the exact path"""
    raw, X, Q, _ = scene(dt, 600, 16, 7, 10)
    raw, Q = raw.copy(), Q.copy()
    if what == "rows":
        bits = raw.view(np.uint16)
        bits[17, 3], bits[400, 0], bits[400, 9] = BITS[dt]
    else:
        Q[2, 5] = np.nan
    got = ctx.groundtruth_rows(raw, Q, 10, dtype=kw(pkg, dt), method="mfma16")
    st = ctx.last_gt_stats
    exact = ctx.groundtruth_rows(raw, Q, 10, dtype=kw(pkg, dt), method="exact")
    assert np.array_equal(got[0], exact[0]) and np.array_equal(got[1], exact[1], equal_nan=True)
    assert st["whole_call_exact"] == 1 and st["queries_fast"] == 0


@pytest.mark.parametrize("dt", ("f16", "u8"))
def test_store_call(pkg, dt):
    raw, X, Q, ref = scene(dt, 3000, 24, 21, 10)
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=24), 0) as c:
        c.store_set(raw, dtype=kw(pkg, dt))
        got = c.groundtruth_store(Q, 10, method="mfma16")
        st = c.last_gt_stats
        assert same(got, ref) and same(got, c.groundtruth_store(Q, 10))
        assert st["queries_exact"] == 0 and st["whole_call_exact"] == 0 and st["queries_fast"] == len(Q)


def test_f32_rows_are_refused(pkg, ctx):
    import torch
    N = pkg._native
    raw, X, Q, _ = scene("f32", 37, 8, 5, 100)
    for call in (lambda: ctx.groundtruth_rows(raw, Q, 3, method="mfma16"), lambda: ctx.groundtruth(raw, Q, 3, method="mfma16")):
        with pytest.raises(N.FspannArgumentError, match="fspann_groundtruth_mfma_dev takes fp32 rows"):
            call()
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    assert N.lib().fspann_groundtruth_mfma16_dev(ctx._h, 4, t.data_ptr(), N.F32, 2, t.data_ptr(), 8, 2, t.data_ptr(), None, None) == N.E_ARG
