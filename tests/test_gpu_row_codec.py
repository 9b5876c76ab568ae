"""GPU: every bit pattern of every row-only type reads as the same value in every kernel that reads rows.

The host side is one decode table per type (256 or 65 536 entries, numpy's own reading of the bits).  A row is one 16-byte slot
(d = N elements) holding pattern p at element p mod N and zeros elsewhere: the byte types get 256 x 16 rows, so that every pattern
meets every position of a slot; the 16-bit types get the 65 536 rows at p mod 8 and the 65 536 at (p + 1) mod 8.  Then
  (a) Refine from the store, slot path: all-zero queries take the rows 256 at a time with k = 256, as fp64 (every element is tested)
      and as fp32 ("the sum tells"): a finite pattern is scored with distance exactly |value| (x^2 is exact in fp64 for all these
      types, and the correctly rounded root of an exact square is |x|), a non-finite one is left out, scored = the finite rows;
  (b) the same with d = N + 1 and a trailing zero: the element-wise path;
  (c) with touch tracking on, each of those calls marks exactly the finite rows;
  (d) the ground truth over the store, k = 1, of queries equal to a sample of the finite rows and to their negations: id and
      squared distance are those of the host table over the finite rows (a row equal to the query: distance 0);
  (e) Setup from the finite rows gives the tables of the F32 build of the decoded values.
Every assertion is an equality."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK = 0
F32, F64, U8, F16, BF16, F8, I8 = range(7)
TYPES = pytest.mark.parametrize("t", [U8, F16, BF16, F8, I8], ids=["u8", "f16", "bf16", "f8", "i8"])
CHUNK = 256


@functools.lru_cache(None)
def _table(t):
    """value of every bit pattern of type t, as float64 (exact: every value of these types is a float)"""
    b8, b16 = np.arange(256, dtype=np.uint8), np.arange(65536, dtype=np.uint16)
    if t == U8:
        return b8.astype(np.float64)
    if t == I8:
        return b8.view(np.int8).astype(np.float64)
    if t == F16:
        return b16.view(np.float16).astype(np.float64)
    if t == BF16:
        with np.errstate(invalid="ignore"):      # (numpy warns when it widens a signalling NaN)
            return (b16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    # OCP fp8 e4m3fn: S EEEE MMM, bias 7; E = 0: +-M/8 * 2^-6; 0x7F / 0xFF NaN
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    mag[(e == 15) & (m == 7)] = np.nan
    return np.where(b & 0x80, -mag, mag)


@functools.lru_cache(None)
def _rows(t):
    """(rows [n][N] as the library takes them, value of each row's pattern, its position, finite).  Never written to."""
    if t in (F16, BF16):
        r = np.arange(2 * 65536)
        p, pos, raw = r & 0xFFFF, ((r & 0xFFFF) + (r >> 16)) % 8, np.zeros((2 * 65536, 8), np.uint16)
    else:
        r = np.arange(256 * 16)
        p, pos, raw = r & 0xFF, r >> 8, np.zeros((256 * 16, 16), np.uint8)
    raw[r, pos] = p
    val = _table(t)[p]
    for a in (raw, val, pos):
        a.setflags(write=False)
    return raw, val, pos, np.isfinite(val)


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _ctx(pkg, d):
    return pkg.FspannContext(pkg.PaperRuntimeConfig(tables=2, divisions=1, m=4, lambda_=2, dim=d, refinement_limit=CHUNK, block_size=8, default_probes=1), 0)


@pytest.mark.parametrize("extra", [0, 1], ids=["slots", "elementwise"])
@TYPES
def test_refine_scores_every_pattern_and_touch_marks_it(pkg, t, extra):
    import torch
    L = pkg._native.lib()
    raw, val, _, fin = _rows(t)
    n, N = raw.shape
    d, nq, k = N + extra, n // CHUNK, CHUNK
    rows = np.ascontiguousarray(np.concatenate([raw, np.zeros((n, extra), raw.dtype)], axis=1))
    # what QueryServiceImpl's refinement leaves of 256 rows against the zero query: the finite ones by (|value|, position)
    dist = np.where(fin, np.abs(val), np.inf).reshape(nq, CHUNK)
    order = np.argsort(dist, axis=1, kind="stable")
    nfin = fin.reshape(nq, CHUNK).sum(1).astype(np.int32)
    live = np.arange(CHUNK)[None] < nfin[:, None]
    ids = np.arange(n, dtype=np.int32).reshape(nq, CHUNK)
    want_ids = np.where(live, np.take_along_axis(ids, order, 1), -1)
    want_dist = np.where(live, np.take_along_axis(dist, order, 1), np.inf)
    with _ctx(pkg, d) as ctx:
        h = ctx.handle
        ctx.set_id_meta(n)
        assert L.fspann_store_set(h, n, _hp(rows), t) == OK, L.fspann_last_error()
        ctx.touch_enable()
        ids_d, cnt_d = _dev(ids), _dev(np.full(nq, CHUNK, np.int32))
        for qdt, Q in ((F64, np.zeros((nq, d), np.float64)), (F32, np.zeros((nq, d), np.float32))):
            qd = _dev(Q)
            dev = qd.device
            o_ids, o_cnt, o_sc = (torch.full(s, -7, dtype=torch.int32, device=dev) for s in ((nq, k), (nq,), (nq,)))
            o_dist = torch.zeros((nq, k), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            assert L.fspann_refine_store_dev(h, nq, qd.data_ptr(), qdt, CHUNK, ids_d.data_ptr(), cnt_d.data_ptr(), k, o_ids.data_ptr(), o_dist.data_ptr(),
                                             o_cnt.data_ptr(), o_sc.data_ptr()) == OK, L.fspann_last_error()
            ctx.sync()
            what = (t, d, qdt)
            assert np.array_equal(o_sc.cpu().numpy(), nfin), what
            assert np.array_equal(o_cnt.cpu().numpy(), nfin), what
            assert np.array_equal(o_ids.cpu().numpy(), want_ids), what
            assert np.array_equal(o_dist.cpu().numpy(), want_dist), what
            assert np.array_equal(ctx.drain_touched(), np.flatnonzero(fin)), what


@TYPES
def test_groundtruth_reads_every_sampled_pattern(pkg, t):
    import torch
    L = pkg._native.lib()
    raw, val, pos, fin = _rows(t)
    n, N = raw.shape
    with np.errstate(invalid="ignore", over="ignore"):
        v32 = val.astype(np.float32)
    assert np.array_equal(v32[fin].astype(np.float64), val[fin])
    # the sample: every finite row of a byte type; of a 16-bit type every 1031st finite row and the edges of the format (zeros,
    # smallest and largest subnormal, smallest and largest normal, of both signs)
    if N == 16:
        s = np.flatnonzero(fin)
    else:
        edges = [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x7BFF, 0xFBFF, 0x007F, 0x807F, 0x0080, 0x8080, 0x7F7F, 0xFF7F]
        s = np.unique(np.concatenate([np.flatnonzero(fin)[::1031], [e for e in edges if fin[e]], [65536 + e for e in edges if fin[e]]]))
    qv, qpos = np.concatenate([v32[s], -v32[s]]), np.concatenate([pos[s], pos[s]])
    nq = len(qv)
    Q = np.zeros((nq, N), np.float32)
    Q[np.arange(nq), qpos] = qv
    # GroundtruthPrecompute's distance from the table: a float subtraction per dimension, fp64 squares; a query and a row differ in
    # one dimension (same position) or two, and a sum of two squares is one rounding whatever its order
    want_id, want_d2 = np.empty(nq, np.int32), np.empty(nq)
    with np.errstate(over="ignore", invalid="ignore"):
        for j0 in range(0, nq, 64):
            a, ap = qv[j0:j0 + 64, None], qpos[j0:j0 + 64, None]
            same = (a - v32[None]).astype(np.float64) ** 2
            apart = a.astype(np.float64) ** 2 + v32[None].astype(np.float64) ** 2
            D = np.where(fin[None], np.where(ap == pos[None], same, apart), np.inf)
            want_id[j0:j0 + 64], want_d2[j0:j0 + 64] = D.argmin(1), D.min(1)
    assert (want_d2[:len(s)] == 0).all()
    with _ctx(pkg, N) as ctx:
        assert L.fspann_store_set(ctx.handle, n, _hp(raw), t) == OK, L.fspann_last_error()
        qd = _dev(Q)
        o_ids = torch.full((nq, 1), -7, dtype=torch.int32, device=qd.device)
        o_d2 = torch.full((nq, 1), -7.0, dtype=torch.float64, device=qd.device)
        torch.cuda.synchronize()
        assert L.fspann_groundtruth_store_dev(ctx.handle, nq, qd.data_ptr(), 1, o_ids.data_ptr(), o_d2.data_ptr()) == OK, L.fspann_last_error()
        ctx.sync()
        assert np.array_equal(o_d2.cpu().numpy()[:, 0], want_d2), t
        assert np.array_equal(o_ids.cpu().numpy()[:, 0], want_id), t


@TYPES
def test_setup_widens_every_pattern(pkg, t):
    L = pkg._native.lib()
    raw, val, pos, fin = _rows(t)
    keep = np.flatnonzero(fin[:65536])                # every finite pattern once (a byte type: at every position)
    rows = np.ascontiguousarray(raw[keep])
    n, N = rows.shape
    V = np.zeros((n, N), np.float32)
    V[np.arange(n), pos[keep]] = val[keep]
    with _ctx(pkg, N) as ctx, _ctx(pkg, N) as c32:
        ctx.registry_initialize(np.random.default_rng(t).standard_normal((1000, N)))
        for c in (ctx, c32):
            c.set_gfunctions(*ctx.get_gfunctions())
            c.set_id_meta(n)
        assert L.fspann_build_index(ctx.handle, n, _hp(rows), t, None) == OK, L.fspann_last_error()
        c32.build_index(V)
        for td in range(ctx.TD):
            a, b = ctx.get_index(td), c32.get_index(td)
            assert sorted(a) == sorted(b) and all(np.array_equal(a[key], b[key]) for key in a), (t, td)
