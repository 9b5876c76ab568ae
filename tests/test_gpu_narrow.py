"""GPU: lossless row narrowing on the device (include/fspann_narrow.h) — fspann_rows_fit_dev, fspann_rows_narrow_dev,
fspann_store_fit and fspann_store_narrow.  Every expectation comes from numpy / CPU torch round trips and from
engine._typed_rows (what store_set(dtype=...) accepts and uploads on the host), never from the kernels under test."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64, U8, F16, BF16, F8, I8 = range(7)
ALL = 0x7F
NAMES = {F32: "FSPANN_F32", F64: "FSPANN_F64", U8: "FSPANN_U8", F16: "FSPANN_F16", BF16: "FSPANN_BF16", F8: "FSPANN_F8E4M3", I8: "FSPANN_I8"}
SIZE = {F32: 4, F64: 8, U8: 1, F16: 2, BF16: 2, F8: 1, I8: 1}
SRC = {F32: np.float32, F64: np.float64}
FIT_TILE = 4096              # elements of a rows_fit_kernel workgroup (whole rows): kNarrowTile of csrc/narrow.hip.h
NARROW_SLOTS = 256 * 4       # 16-byte output slots of a rows_narrow_kernel workgroup: kNarrowThreads * kNarrowSlots


def narrower(src):
    return [t for t in (U8, I8, F8, F16, BF16, F32) if SIZE[t] < SIZE[src]]


def elem_bits(v):
    """per element: the mask of the types it is exactly a value of, by round trip on the CPU (its own and any wider type always)"""
    import torch
    src = F32 if v.dtype == np.float32 else F64
    with np.errstate(all="ignore"):
        nan = v != v
        whole = v == np.floor(v)
        f32 = v.astype(np.float32)
        is32 = (f32.astype(v.dtype) == v) | nan
        t8 = torch.from_numpy(v.astype(np.float64)).to(torch.float8_e4m3fn).to(torch.float64).numpy()
        fit = {U8: (v >= 0) & (v <= 255) & whole, I8: (v >= -128) & (v <= 127) & whole,
               F8: ((t8 == v) & np.isfinite(v)) | nan,
               F16: (v.astype(np.float16).astype(v.dtype) == v) | nan,
               BF16: (((f32.view(np.uint32) & 0xFFFF) == 0) & is32) | nan,
               F32: is32}
    bits = np.full(v.shape, (1 << F32 | 1 << F64) if src == F32 else 1 << F64, np.uint8)
    for t in narrower(src):
        bits |= (fit[t].astype(np.uint8) << t)
    return bits


def expect_fit(v2d):
    """fits, first_misfit [7], nonfinite, row mask of a 2-D block, from elem_bits"""
    eb = elem_bits(v2d)
    flat = eb.reshape(-1)
    first = np.full(7, -1, np.int64)
    fits = 0
    for t in range(7):
        miss = np.flatnonzero(~(flat >> t) & 1)
        if len(miss):
            first[t] = miss[0]
        else:
            fits |= 1 << t
    return dict(fits=fits, first_misfit=first, nonfinite=int((~np.isfinite(v2d)).sum()), row_fits=np.bitwise_and.reduce(eb, axis=1))


@pytest.fixture(scope="module")
def ctx(pkg):
    cfg = pkg.PaperRuntimeConfig(tables=2, divisions=2, m=8, lambda_=2, dim=16, refinement_limit=64)
    with pkg.FspannContext(cfg, 0) as c:
        yield c


def dev_rows(v, offset=0):
    """the array in device memory, `offset` bytes behind a 256-byte-aligned address; (tensor kept alive, pointer)"""
    import torch
    raw = np.ascontiguousarray(v).view(np.uint8).reshape(-1)
    t = torch.zeros(len(raw) + offset + 64, dtype=torch.uint8, device="cuda:0")
    t[offset:offset + len(raw)] = torch.from_numpy(raw.copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + offset


def run_fit(ctx, v2d, allowed=0, mask=True, offset=0):
    import torch
    n, dim = v2d.shape
    keep, p = dev_rows(v2d, offset)
    rf = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()                                    # (torch fills on its own stream, the library works on the context's)
    f = ctx.rows_fit_dev(n, p, F32 if v2d.dtype == np.float32 else F64, dim, allowed, rf.data_ptr() if mask else 0)
    rows = rf.cpu().numpy()
    assert (rows[n:] == 0xEE).all(), "row mask written past [n]"
    return dict(fits=int(f.fits), narrowest=int(f.narrowest), first_misfit=np.array(f.first_misfit[:7], np.int64), nonfinite=int(f.nonfinite),
                row_fits=rows[:n] if mask else None, unused=int(f.first_misfit[7]))


def check_fit(ctx, v2d, offset=0):
    exp = expect_fit(v2d)
    for mask in (True, False):
        got = run_fit(ctx, v2d, mask=mask, offset=offset)
        assert got["fits"] == exp["fits"], (hex(got["fits"]), hex(exp["fits"]), mask)
        assert np.array_equal(got["first_misfit"], exp["first_misfit"]), (got["first_misfit"], exp["first_misfit"], mask)
        assert got["nonfinite"] == exp["nonfinite"] and got["unused"] == -1
        if mask:
            assert np.array_equal(got["row_fits"], exp["row_fits"]), np.flatnonzero(got["row_fits"] != exp["row_fits"])[:10]
    return exp


def run_narrow(pkg, ctx, v2d, t, offset=0, dst_offset=0):
    """fspann_rows_narrow_dev into a buffer with canary bytes on both sides; (return code, misfits, bytes)"""
    import torch
    n, dim = v2d.shape
    keep, p = dev_rows(v2d, offset)
    nb = n * dim * SIZE[t]
    dst = torch.full((nb + dst_offset + 256,), 0xC3, dtype=torch.uint8, device="cuda:0")
    mis = C.c_int64(-5)
    torch.cuda.synchronize()
    rc = ctx.L.fspann_rows_narrow_dev(ctx.handle, n, p, F32 if v2d.dtype == np.float32 else F64, dim, dst.data_ptr() + dst_offset, t, C.byref(mis))
    out = dst.cpu().numpy()
    assert (out[:dst_offset] == 0xC3).all() and (out[dst_offset + nb:] == 0xC3).all(), "canary bytes around dst overwritten"
    return rc, int(mis.value), out[dst_offset:dst_offset + nb]


def typed_bytes(pkg, v, t):
    """what store_set(dtype=...) uploads for these values: engine._typed_rows' bytes"""
    kind = {U8: np.uint8, I8: np.int8, F8: pkg.float8_e4m3fn, F16: np.float16, BF16: pkg.bfloat16, F32: np.float32}[t]
    rows, code, _ = pkg.engine._typed_rows(v, kind, "test")
    assert code == t
    return np.ascontiguousarray(rows).view(np.uint8).reshape(-1)


def is_nan_pattern(bits, t):
    if t == F8:
        return (bits & 0x7F) == 0x7F
    if t == F16:
        return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x3FF) != 0)
    if t == BF16:
        return ((bits & 0x7F80) == 0x7F80) & ((bits & 0x7F) != 0)
    return ((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x7FFFFF) != 0)


def check_narrow(pkg, ctx, v2d, t, offset=0, dst_offset=0):
    """the target's bytes equal _typed_rows' over the same data: non-NaN elements bit for bit, a NaN some NaN"""
    rc, mis, got = run_narrow(pkg, ctx, v2d, t, offset, dst_offset)
    assert rc == 0 and mis == 0, (rc, mis, ctx.L.fspann_last_error())
    want = typed_bytes(pkg, v2d, t)
    word = {1: np.uint8, 2: np.uint16, 4: np.uint32}[SIZE[t]]
    g, w = got.view(word).astype(np.uint32), want.view(word).astype(np.uint32)
    nan = (v2d != v2d).reshape(-1)
    assert np.array_equal(g[~nan], w[~nan]), np.flatnonzero((g != w) & ~nan)[:10]
    if nan.any():
        assert is_nan_pattern(g[nan], t).all()


# ---- every value of every type, and its neighbours ------------------------------------------------------------------------------

def patterns(t):
    """all bit patterns of a type and their values, widened on the CPU"""
    import torch
    if t in (U8, I8):
        b = np.arange(256, dtype=np.uint8)
        return b, (b if t == U8 else b.view(np.int8)).astype(np.float32)
    if t == F8:
        b = np.arange(256, dtype=np.uint8)
        return b, torch.from_numpy(b).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    h = np.arange(65536, dtype=np.uint16)
    return h, h.view(np.float16).astype(np.float32) if t == F16 else (h.astype(np.uint32) << 16).view(np.float32)


@pytest.fixture(scope="module")
def all_values():
    with np.errstate(invalid="ignore"):
        v = np.concatenate([patterns(t)[1] for t in (U8, I8, F8, F16, BF16)])
        return np.concatenate([v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))])


@pytest.mark.parametrize("src", [F32, F64])
def test_every_value_and_its_neighbours_fit_as_on_the_cpu(ctx, all_values, src):
    """dim = 1: the row mask is the element's mask — every pattern of the five narrow types and both fp32 neighbours of each"""
    with np.errstate(invalid="ignore"):
        v = all_values.astype(SRC[src]).reshape(-1, 1)
    check_fit(ctx, v)


@pytest.mark.parametrize("src", [F32, F64])
@pytest.mark.parametrize("t", [U8, I8, F8, F16, BF16])
def test_every_pattern_narrows_back_to_itself(pkg, ctx, src, t):
    bits, vals = patterns(t)
    with np.errstate(invalid="ignore"):
        v = vals.astype(SRC[src]).reshape(-1, 1)
    rc, mis, got = run_narrow(pkg, ctx, v, t)
    assert rc == 0 and mis == 0, ctx.L.fspann_last_error()
    got = got.view(bits.dtype)
    nan = (vals != vals)
    assert np.array_equal(got[~nan], bits[~nan]), np.flatnonzero((got != bits) & ~nan)[:10]      # (-0.0 of F8 / F16 / BF16 keeps its sign)
    if nan.any():
        assert is_nan_pattern(got[nan].astype(np.uint32), t).all()
    check_narrow(pkg, ctx, v, t)
    if t in (U8, I8):                                                                            # -0.0 gives the byte 0
        rc, mis, z = run_narrow(pkg, ctx, np.array([[-0.0], [0.0]], SRC[src]), t)
        assert rc == 0 and mis == 0 and (z == 0).all()


BOUNDARY = {
    U8: [(255, 1), (256, 0), (-1, 0), (0.5, 0), (-0.0, 1)],
    I8: [(-128, 1), (-129, 0), (127, 1), (128, 0)],
    F8: [(448, 1), (449, 0), (480, 0), (2.0 ** -9, 1), (2.0 ** -10, 0), (1.125, 1), (1.0625, 0), (np.inf, 0), (np.nan, 1)],
    F16: [(65504, 1), (65520, 0), (2.0 ** -24, 1), (2.0 ** -25, 0), (1 + 2.0 ** -10, 1), (1 + 2.0 ** -11, 0), (np.inf, 1)],
    BF16: [(1 + 2.0 ** -7, 1), (1 + 2.0 ** -8, 0), (2.0 ** -133, 1), (2.0 ** -149, 0)],
    F32: [(1 + 2.0 ** -23, 1), (1 + 2.0 ** -24, 0), (1e300, 0), (2.0 ** -149, 1), (2.0 ** -150, 0)],
}


@pytest.mark.parametrize("src", [F32, F64])
def test_boundary_values(pkg, ctx, src):
    """the values at each type's edges, with the answer written out (and checked against the CPU round trip as well)"""
    for t in narrower(src):
        vals = np.array([x for x, _ in BOUNDARY[t]], SRC[src]).reshape(-1, 1)
        want = np.array([f for _, f in BOUNDARY[t]], bool)
        assert np.array_equal((elem_bits(vals)[:, 0] >> t) & 1, want), NAMES[t]
        got = run_fit(ctx, vals)
        assert np.array_equal((got["row_fits"] >> t) & 1, want), (NAMES[t], got["row_fits"])
        exp_first = -1 if want.all() else int(np.flatnonzero(~want)[0])
        assert got["first_misfit"][t] == exp_first and bool(got["fits"] >> t & 1) == bool(want.all())
        check_narrow(pkg, ctx, vals[want], t)
        for i in np.flatnonzero(~want):
            rc, mis, _ = run_narrow(pkg, ctx, vals[i:i + 1], t)
            assert rc == pkg._native.E_ARG and mis == 1, (NAMES[t], vals[i])


# ---- shapes ------------------------------------------------------------------------------------------------------------------------

PALETTE = np.array([0, 1, 7, 15, 200, 255, -3, -128, 0.5, 1.5, -2.5, 448, 1 + 2.0 ** -10, 1000.25, 65504, 1 + 2.0 ** -7, 2.0 ** 100, 3.0e38,
                    0.1, 1 + 2.0 ** -20, np.nan, np.inf, -np.inf, -0.0], np.float32)
FITTING = {      # values of a type that fit it (a NaN and an inf where the type has one)
    U8: np.array([0, 1, 200, 255, -0.0, 17], np.float32), I8: np.array([-128, 127, -1, 0, 5], np.float32),
    F8: np.array([0.5, -2.5, 448, 2.0 ** -9, np.nan, -0.0, 1.125], np.float32),
    F16: np.array([65504, 1 + 2.0 ** -10, 2.0 ** -24, np.inf, np.nan, -0.0, 0.5], np.float32),
    BF16: np.array([2.0 ** 100, 1 + 2.0 ** -7, 2.0 ** -133, -np.inf, np.nan, -0.0], np.float32),
    F32: np.array([0.1, 1 + 2.0 ** -23, 2.0 ** -149, np.inf, np.nan, 3.0e38], np.float32),
}


def mixed(rng, n, dim, dt):
    """rows of several kinds: some fit every type, some only the wide ones, a few hold a misfit of everything or a non-finite value"""
    with np.errstate(invalid="ignore"):
        v = rng.choice(PALETTE[:4], (n, dim)).astype(dt)
        kind = rng.integers(0, 4, n)
        for r in range(n):
            if kind[r] == 1:
                v[r] = rng.choice(PALETTE[:12], dim)
            elif kind[r] == 2:
                v[r, rng.integers(0, dim)] = rng.choice(PALETTE)
            elif kind[r] == 3:
                v[r] = rng.choice(PALETTE, dim)
    return v


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("src", [F32, F64])
@pytest.mark.parametrize("dim", [1, 3, 16, 17, 128, 130])
def test_shapes_fit_and_narrow(pkg, ctx, dim, src, offset):
    """n in {1, 7, 257} at every dim, the base pointer 16-byte aligned and 4 bytes off (fp64 rows then start off their own
    element's alignment too): the fit pass over mixed rows, the narrow pass to every target over rows that fit it"""
    rng = np.random.default_rng(dim * 10 + src)
    for n in (1, 7, 257):
        check_fit(ctx, mixed(rng, n, dim, SRC[src]), offset)
        for t in narrower(src):
            with np.errstate(invalid="ignore"):
                v = rng.choice(FITTING[t], (n, dim)).astype(SRC[src])
            check_narrow(pkg, ctx, v, t, offset, dst_offset=SIZE[t] * (offset // 4))


@pytest.mark.parametrize("src", [F32, F64])
def test_whole_tiles_one_short_and_one_past(pkg, ctx, src):
    """dim = 1, so a row-aligned workgroup tile of the fit pass is exactly FIT_TILE elements: two tiles, one element fewer, one more
    (the last with a misfit as its very last element); the narrow pass likewise around two of its workgroups' outputs per target"""
    rng = np.random.default_rng(3)
    for n in (2 * FIT_TILE - 1, 2 * FIT_TILE, 2 * FIT_TILE + 1):
        v = rng.integers(0, 16, (n, 1)).astype(SRC[src])
        check_fit(ctx, v)
        v[-1] = 0.5
        exp = check_fit(ctx, v)
        assert exp["first_misfit"][U8] == n - 1
    for t in narrower(src):
        per_wg = NARROW_SLOTS * (16 // SIZE[t])
        for n in (2 * per_wg - 1, 2 * per_wg, 2 * per_wg + 1):
            with np.errstate(invalid="ignore"):
                check_narrow(pkg, ctx, rng.choice(FITTING[t], (n, 1)).astype(SRC[src]), t)


@pytest.mark.parametrize("src", [F32, F64])
def test_more_tiles_than_workgroups(ctx, src):
    """dim > FIT_TILE / 2 makes every row a tile of its own, and 2 300 of them are more than the fit pass launches workgroups
    (eight per CU): a workgroup then walks several tiles; misfits in its later ones, a row mask for every row"""
    n, dim = 2300, FIT_TILE // 2 + 1
    v = np.random.default_rng(13).integers(0, 16, (n, dim)).astype(SRC[src])
    v[2250, 17], v[2299, dim - 1], v[2100, 5] = 0.5, np.inf, 300.0
    exp = check_fit(ctx, v)
    assert exp["first_misfit"][U8] == 2100 * dim + 5 and exp["first_misfit"][F8] == 2100 * dim + 5 and exp["first_misfit"][F16] == -1
    assert exp["nonfinite"] == 1 and exp["row_fits"][2299] == ALL & ~(1 << U8 | 1 << I8 | 1 << F8)      # (+inf is a half and a bfloat16)


@pytest.mark.parametrize("src", [F32, F64])
@pytest.mark.parametrize("place", ["first", "last", "tile_end", "tail"])
def test_one_planted_half(ctx, src, place):
    """A block that fits every type (integers 0..15), three and a bit workgroup tiles of 256 rows, and a single 0.5: fits loses
    exactly the byte types, first_misfit is that index for each of them and -1 elsewhere, the row mask is clear in that row only."""
    dim, n = 16, 3 * 256 + 7
    v = np.random.default_rng(9).integers(0, 16, (n, dim)).astype(SRC[src])
    offset = 4 if place == "tail" else 0                    # (off the 16-byte grid the last slot is a partial one)
    idx = {"first": 0, "last": n * dim - 1, "tile_end": FIT_TILE - 1, "tail": n * dim - 2}[place]
    base = run_fit(ctx, v, offset=offset)
    assert base["fits"] == ALL and (base["first_misfit"] == -1).all() and (base["row_fits"] == ALL).all() and base["narrowest"] == U8
    v.reshape(-1)[idx] = 0.5
    for mask in (True, False):
        got = run_fit(ctx, v, mask=mask, offset=offset)
        assert got["fits"] == ALL & ~(1 << U8 | 1 << I8)
        for t in range(7):
            assert got["first_misfit"][t] == (idx if t in (U8, I8) else -1), (t, got["first_misfit"])
        assert got["narrowest"] == F8 and got["nonfinite"] == 0
        if mask:
            want = np.full(n, ALL, np.uint8)
            want[idx // dim] = ALL & ~(1 << U8 | 1 << I8)
            assert np.array_equal(got["row_fits"], want)


@pytest.mark.parametrize("src", [F32, F64])
def test_two_misfits_the_lower_index_wins(ctx, src):
    """misfits in two workgroups, the later one of more types: each type reports its own lowest index"""
    dim, n = 16, 3 * 256 + 7
    v = np.random.default_rng(10).integers(0, 16, (n, dim)).astype(SRC[src])
    flat = v.reshape(-1)
    flat[9000], flat[5000], flat[11000] = 300.0, 0.5, 0.5           # 300: no byte, no fp8; 0.5: no byte
    for mask in (True, False):
        got = run_fit(ctx, v, mask=mask)
        assert got["first_misfit"][U8] == 5000 and got["first_misfit"][I8] == 5000 and got["first_misfit"][F8] == 9000
        assert got["fits"] == ALL & ~(1 << U8 | 1 << I8 | 1 << F8) and got["narrowest"] == F16
    check_fit(ctx, v)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_row_calls(pkg, ctx):
    N = pkg._native
    v = np.arange(32, dtype=np.float32).reshape(2, 16)
    v[1, 3] = 0.5
    v[1, 9] = -7.25
    rc, mis, _ = run_narrow(pkg, ctx, v, U8)
    msg = ctx.L.fspann_last_error().decode()
    assert rc == N.E_ARG and mis == 2 and "FSPANN_U8" in msg and "2 element" in msg and "index 19" in msg, msg
    rc, mis, _ = run_narrow(pkg, ctx, v, I8)
    assert rc == N.E_ARG and mis == 2 and "FSPANN_I8" in ctx.L.fspann_last_error().decode()
    keep, p = dev_rows(v)
    fit, m = N.Fit(), C.c_int64(0)
    for dst in (F32, F64):                                     # a target not narrower than the source
        assert ctx.L.fspann_rows_narrow_dev(ctx.handle, 2, p, F32, 16, p, dst, C.byref(m)) == N.E_ARG
        assert b"not narrower" in ctx.L.fspann_last_error()
    assert ctx.L.fspann_rows_narrow_dev(ctx.handle, 2, p, F64, 16, p, F64, C.byref(m)) == N.E_ARG
    for t in (U8, F16, BF16, F8, I8):                          # a row-only source dtype, named
        assert ctx.L.fspann_rows_fit_dev(ctx.handle, 2, p, t, 16, 0, None, C.byref(fit)) == N.E_ARG
        assert NAMES[t].encode() in ctx.L.fspann_last_error()
        assert ctx.L.fspann_rows_narrow_dev(ctx.handle, 2, p, t, 16, p, U8, C.byref(m)) == N.E_ARG
        assert NAMES[t].encode() in ctx.L.fspann_last_error()
    for bad in (7, -1, 99):                                    # an unknown dtype
        assert ctx.L.fspann_rows_fit_dev(ctx.handle, 2, p, bad, 16, 0, None, C.byref(fit)) == N.E_ARG
        assert b"unknown dtype" in ctx.L.fspann_last_error()
        assert ctx.L.fspann_rows_narrow_dev(ctx.handle, 2, p, bad, 16, p, U8, C.byref(m)) == N.E_ARG
        assert ctx.L.fspann_rows_narrow_dev(ctx.handle, 2, p, F32, 16, p, bad, C.byref(m)) == N.E_ARG
    assert ctx.L.fspann_rows_fit_dev(ctx.handle, 0, p, F32, 16, 0, None, C.byref(fit)) == N.E_ARG
    assert ctx.L.fspann_rows_fit_dev(ctx.handle, 2, p, F32, 0, 0, None, C.byref(fit)) == N.E_ARG
    assert ctx.L.fspann_rows_fit_dev(ctx.handle, 2, p, F32, 16, 1 << 9, None, C.byref(fit)) == N.E_ARG
    assert ctx.L.fspann_rows_fit_dev(ctx.handle, 2, None, F32, 16, 0, None, C.byref(fit)) == N.E_NULL
    assert ctx.L.fspann_rows_fit_dev(ctx.handle, 2, p, F32, 16, 0, None, None) == N.E_NULL


def small_ctx(pkg, dim=16):
    cfg = pkg.PaperRuntimeConfig(tables=2, divisions=2, m=8, lambda_=2, dim=dim, refinement_limit=64)
    return pkg.FspannContext(cfg, 0)


def store_ptr(ctx):
    dt = C.c_int(-1)
    p = ctx.L.fspann_store_dev_ptr(ctx.handle, C.byref(dt))
    return p, dt.value


def test_refusals_of_the_store_calls(pkg):
    N = pkg._native
    X = np.random.default_rng(2).integers(0, 256, (300, 16)).astype(np.float64)
    with small_ctx(pkg) as c:
        with pytest.raises(N.FspannStateError, match="store not set"):
            c.store_narrow()
        with pytest.raises(N.FspannStateError, match="store not set"):
            c.store_fit()
        keep, p = dev_rows(X)
        c.store_attach_dev(300, p, F64)                         # an attached, caller-owned store
        assert c.store_fit()["narrowest"] == U8
        with pytest.raises(N.FspannStateError, match="fspann_rows_narrow_dev"):
            c.store_narrow()
        assert store_ptr(c) == (p, F64)
        c.store_set(X)
        p0 = store_ptr(c)
        c.registry_initialize(X)                                # (a clone is taken of a finalized index)
        c.set_id_meta(300)
        c.build_index(X)
        with c.clone() as k:                                   # a store shared with a clone: neither side may change it
            with pytest.raises(N.FspannStateError, match=r"shared with 1 clone\(s\): destroy them first"):
                c.store_narrow()
            with pytest.raises(N.FspannStateError):
                k.store_narrow()
            assert store_ptr(c) == p0
        assert c.store_narrow() == np.uint8                     # the clone gone, it narrows
        p1 = store_ptr(c)
        assert p1[1] == U8
        assert c.store_narrow() == np.uint8 and store_ptr(c) == p1      # a row-only type already: FSPANN_OK, unchanged
        f = c.store_fit()
        assert f["fits"] == 1 << U8 and f["narrowest"] == U8


# ---- order and `allowed` ---------------------------------------------------------------------------------------------------------

ONLY = {   # data that fits the type and nothing earlier in the order
    U8: [0, 200, 255, 17], I8: [-128, 127, -1, 5], F8: [0.5, -2.5, 448, 1.125], F16: [1 + 2.0 ** -10, 65504, 0.5, -3],
    BF16: [2.0 ** 100, 1 + 2.0 ** -7, 0.5, 3], F32: [0.1, 1 + 2.0 ** -23, 7, 0.5],
}


@pytest.mark.parametrize("src", [F32, F64])
def test_narrowest_follows_the_order(pkg, ctx, src):
    rng = np.random.default_rng(4)
    for t in (U8, I8, F8, F16, BF16, F32):
        v = rng.choice(np.array(ONLY[t], np.float32), (40, 24)).astype(SRC[src])
        v[0, :4] = np.array(ONLY[t], np.float32)
        got = run_fit(ctx, v)
        assert got["narrowest"] == (t if SIZE[t] < SIZE[src] else src), (NAMES[t], got)
        assert got["fits"] == expect_fit(v)["fits"]
    ints = rng.integers(0, 100, (40, 24)).astype(SRC[src])
    assert run_fit(ctx, ints, allowed=1 << F16 | 1 << BF16)["narrowest"] == F16
    assert run_fit(ctx, ints, allowed=1 << BF16)["narrowest"] == BF16
    assert run_fit(ctx, ints, allowed=1 << I8 | 1 << F16)["narrowest"] == I8
    assert run_fit(ctx, ints, allowed=1 << src)["narrowest"] == src
    assert run_fit(ctx, ints + 0.5, allowed=1 << U8 | 1 << I8)["narrowest"] == src           # nothing allowed fits: the source itself
    assert ctx.rows_fit(ints, allowed=[F16, BF16])["narrowest"] == F16                       # the numpy wrapper, codes as a list


def test_random_fp64_store_stays_as_it_is(pkg):
    X = np.random.default_rng(6).standard_normal((500, 16))
    with small_ctx(pkg) as c:
        c.store_set(X)
        p0 = store_ptr(c)
        f = c.store_fit()
        assert f["fits"] == 1 << F64 and f["narrowest"] == F64 and (f["first_misfit"][[U8, I8, F8, F16, BF16, F32]] == 0).all()
        assert c.store_narrow() == np.float64 and c.store_dtype == np.float64
        assert store_ptr(c) == p0                               # same rows, same type: nothing was swapped
        assert c.store_set_narrowest(X.astype(np.float32).astype(np.float64)) == np.float32
        assert store_ptr(c)[1] == F32


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def _search(ctx, Q, B, K):
    import torch
    dev = torch.device("cuda", 0)
    nq = len(Q)
    qd = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    t = dict(ids=torch.full((nq, K), -7, dtype=torch.int32, device=dev), dist=torch.zeros((nq, K), dtype=torch.float64, device=dev),
             count=torch.full((nq,), -7, dtype=torch.int32, device=dev), scored=torch.full((nq,), -7, dtype=torch.int32, device=dev),
             sel=torch.full((nq, B), -1, dtype=torch.int32, device=dev), selc=torch.full((nq,), -7, dtype=torch.int32, device=dev),
             bad=torch.full((nq,), -7, dtype=torch.int32, device=dev), ret=torch.full((nq,), -7, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ctx.search_retry_dev(nq, qd.data_ptr(), F32, -1, B, K, t["ids"].data_ptr(), t["dist"].data_ptr(), t["count"].data_ptr(), t["scored"].data_ptr(),
                         t["sel"].data_ptr(), t["selc"].data_ptr(), t["bad"].data_ptr(), t["ret"].data_ptr())
    ctx.sync()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    for i in range(nq):                                         # (beyond a query's count the sel list is not part of the result)
        out["sel"][i, max(out["selc"][i], 0):] = -1
    return out


def _groundtruth_store(ctx, Q, K):
    import torch
    qd = torch.from_numpy(np.ascontiguousarray(Q)).to("cuda:0")
    ids = torch.full((len(Q), K), -7, dtype=torch.int32, device="cuda:0")
    d2 = torch.zeros((len(Q), K), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.groundtruth_store_dev(len(Q), qd.data_ptr(), K, ids.data_ptr(), d2.data_ptr())
    ctx.sync()
    return ids.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("kind", ["bytes", "halves", "halves_nonfinite"])
def test_store_narrow_end_to_end(pkg, kind):
    """An fp64 store of byte-valued (half-valued) data: the search with its retry, the store refine and the touched set are
    bit-identical before and after store_narrow; afterwards the store is FSPANN_U8 (FSPANN_F16) and the ground truth over the
    store, refused for fp64 rows, runs and equals the ground truth over the same values as fp32."""
    N = pkg._native
    rng = np.random.default_rng(12)
    n, d, B, K = 4000, 32, 64, 5
    X = rng.integers(0, 256, (n, d)).astype(np.float64)
    if kind != "bytes":
        X /= 2
    want_code, want_kept = (U8, np.uint8) if kind == "bytes" else (F16, np.float16)
    Xs = X.copy()
    if kind == "halves_nonfinite":
        Xs[7, 3] = np.nan
        Xs[11, 30] = np.inf
    Q = (X[rng.integers(0, n, 48)] + rng.integers(-3, 4, (48, d))).astype(np.float32)
    cand = rng.integers(0, n, (48, B)).astype(np.int32)
    cand[cand == 7], cand[cand == 11] = 8, 12
    cand[:, 5], cand[:, 9] = 7, 11                               # the two non-finite rows are candidates of every query, once each
    cnt = np.full(48, B, np.int32)
    cfg = pkg.PaperRuntimeConfig(tables=4, divisions=2, m=8, lambda_=2, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as c:
        c.registry_initialize(X[:1000])
        c.set_id_meta(n)
        c.build_index(X)
        c.store_set(Xs)
        assert store_ptr(c)[1] == F64
        with pytest.raises(N.FspannArgumentError, match="FSPANN_F64 store"):
            _groundtruth_store(c, Q, K)

        def everything():
            c.touch_enable(True)
            s = _search(c, Q, B, K)
            r = c.refine_store(Q, cand, cnt, K)
            touched = c.drain_touched(reset=True)
            c.touch_enable(False)
            return s, r, touched
        s0, r0, t0 = everything()
        assert s0["count"].sum() > 0 and r0["count"].sum() > 0 and len(t0) > 0
        fit = c.store_fit()
        assert fit["narrowest"] == want_code and fit["nonfinite"] == (2 if kind == "halves_nonfinite" else 0)
        assert c.store_narrow() == want_kept and c.store_dtype == want_kept
        assert store_ptr(c)[1] == want_code
        s1, r1, t1 = everything()
        for k in s0:
            assert np.array_equal(s0[k], s1[k]), k
        for k in r0:
            assert np.array_equal(r0[k], r1[k]), k
        assert np.array_equal(t0, t1)
        if kind == "halves_nonfinite":                          # both rows still skipped, not scored
            assert not np.isin(r1["ids"], (7, 11)).any() and (r1["scored"] == B - 2).all()
            assert not np.isin(t1, (7, 11)).any()
        gi, gd = _groundtruth_store(c, Q, K)
        ri, rd = c.groundtruth(Xs.astype(np.float32), Q, K)
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd)
