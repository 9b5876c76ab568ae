"""A plain numpy restatement of the exact ground truth and of the evaluation metrics, written from the Java and not from oracle/:
GroundtruthPrecompute.java:142-189 (l2sq: `double d = q[i] - v` with q and v floats, i.e. a FLOAT subtraction widened, `sum += d*d`;
HeapK with BY_D_THEN_ID: Double.compare, then the lower id), ForwardSecureANNSystem.java:770-835 (computeMetricsAtK) and
BaseVectorReader.l2 (`double d = q[i] - v` with q a double[], the sum in dimension order, Math.sqrt).  A helper module (no test,
no fixture): the GPU tests take their expected values from here, tests/test_gt_ref_cpu.py holds it against the oracle, and both take
their data sets from the generators below, so the two cannot drift.  numpy only."""
import functools

import numpy as np

I32_MAX = 2 ** 31 - 1


# ---- the reference -------------------------------------------------------------------------------------------------------------
def d2(base_f32, q_f32):
    """[nq][n] squared distances: one float subtraction and one fp64 add per dimension, in dimension order"""
    base, q = np.asarray(base_f32), np.asarray(q_f32)
    assert base.dtype == np.float32 and q.dtype == np.float32
    s = np.zeros((len(q), len(base)), np.float64)
    with np.errstate(all="ignore"):
        for i in range(base.shape[1]):
            df = q[:, None, i] - base[None, :, i]
            assert df.dtype == np.float32
            dd = df.astype(np.float64)
            s = s + dd * dd
    return s


def knn(base_f32, q_f32, k):
    """(ids [nq][k] int32, d2 [nq][k] float64, nan0 [nq]): ascending (distance, id), NaN distances after every number, -1 / +inf
    beyond n; nan0[i] = the place where query i's NaN tail begins (min(k, n) when it has none)"""
    D = d2(base_f32, q_f32)
    nq, n = D.shape
    kk = min(k, n)
    ids = np.full((nq, k), -1, np.int32)
    out = np.full((nq, k), np.inf, np.float64)
    nan0 = np.empty(nq, np.int64)
    for i in range(nq):
        row = D[i]
        isn = np.isnan(row)
        good = np.flatnonzero(~isn)
        order = np.concatenate([good[np.lexsort((good, row[good]))], np.flatnonzero(isn)])[:kk]
        ids[i, :kk] = order
        out[i, :kk] = row[order]
        nan0[i] = min(len(good), kk)
    return ids, out, nan0


def l2(q64, v64):
    """BaseVectorReader.l2 of one query against rows v64 [m][d]: a sequential sum over d, then sqrt"""
    s = np.zeros(len(v64), np.float64)
    for t in range(len(q64)):
        dd = q64[t] - v64[:, t]
        s = s + dd * dd
    return np.sqrt(s)


def ratio_terms(base64, q64, ann_row, gt_row, k):
    """dAnn / dGt of the places i < k that computeMetricsAtK uses, in index order (None where it says `continue`)"""
    n = len(base64)
    a, g = np.asarray(ann_row[:k], np.int64), np.asarray(gt_row[:k], np.int64)
    ok = (a >= 0) & (a < n) & (g >= 0) & (g < n)
    d_gt = np.zeros(k)
    d_ann = np.zeros(k)
    d_gt[ok] = l2(q64, base64[g[ok]])
    d_ann[ok] = l2(q64, base64[a[ok]])
    return [float(d_ann[i]) / float(d_gt[i]) if ok[i] and not d_gt[i] <= 0 else None for i in range(k)]


def metrics(base64, q64, k, ann, ann_count, gt):
    """(recall [nq], ratio [nq]).  ann [nq][stride] with ann_count results per query (None: stride of them; a count is taken into
    0..stride, which is all the list can hold), gt [nq][>= k].  base64 / q64: the fp64 values of the elements."""
    base64, q64 = np.asarray(base64, np.float64), np.asarray(q64, np.float64)
    nq, stride = ann.shape
    rec = np.empty(nq, np.float64)
    rat = np.full(nq, np.nan, np.float64)
    for qi in range(nq):
        na = stride if ann_count is None else max(0, min(int(ann_count[qi]), stride))
        top = set(int(x) for x in gt[qi, :k])
        hits = 0
        for i in range(min(k, na)):
            if int(ann[qi, i]) in top:
                hits += 1
        rec[qi] = hits / float(k)
        if na >= k:
            total, used = 0.0, 0
            for t in ratio_terms(base64, q64[qi], ann[qi], gt[qi], k):
                if t is None:
                    continue
                total += t
                used += 1
            if used == k:
                rat[qi] = total / k
    return rec, rat


# ---- row types: values on each type's own grid ------------------------------------------------------------------------------------
DTYPES = ("f32", "u8", "i8", "f16", "bf16", "f8")


def e4m3_table():
    """value of each of the 256 patterns, from the definition: E = 0: +-M/8 * 2^-6; E = 1..15: +-(1 + M/8) * 2^(E-7); 0x7F / 0xFF NaN"""
    t = np.empty(256, np.float64)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        v = float("nan") if (e == 15 and m == 7) else (m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if s else v
    return t


E4M3 = e4m3_table().astype(np.float32)       # (every e4m3 value is a float)
E4M3_POS = np.arange(0x00, 0x7F, dtype=np.uint8)
E4M3_SORTED = E4M3[E4M3_POS]                 # ascending: the non-negative finite values


def bf16_round(a):
    """finite float32 values -> bfloat16 bit patterns (uint16), round to nearest even on the bit pattern"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    assert ((u & 0x7F800000) != 0x7F800000).all()
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def f8_round(a):
    """non-negative float32 values below 448 -> the nearest e4m3 byte (the smaller of two equally near)"""
    a = np.asarray(a, np.float32)
    hi = np.clip(np.searchsorted(E4M3_SORTED, a), 1, len(E4M3_SORTED) - 1)
    lo = hi - 1
    return E4M3_POS[np.where(a - E4M3_SORTED[lo] <= E4M3_SORTED[hi] - a, lo, hi)]


def clustered(rng, d, r=16, noise=6.0):
    """a SIFT-like generator (intrinsic dimension r): draw(cnt) -> float32 in [0, 255]"""
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)

    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        v = np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)
        return np.clip(v, 0, 255).astype(np.float32)
    return draw


def typed(dt, a):
    """float32 draws in [0, 255] -> rows of type dt as the library takes them: the one rounding, on the host.  f32: as drawn; u8, i8:
    the integer scale; f16, bf16: O(1), as uint16 patterns for bf16; f8: [0, 64] as e4m3 bytes."""
    if dt == "f32":
        return a
    if dt == "u8":
        return np.rint(a).astype(np.uint8)
    if dt == "i8":
        return (np.rint(a) - 128).astype(np.int8)
    if dt == "f16":
        return (a / np.float32(64.0)).astype(np.float16)
    if dt == "bf16":
        return bf16_round(a / np.float32(64.0))
    return f8_round(a / np.float32(4.0))


def widen(dt, raw):
    """rows of type dt -> the float32 values they are (exact)"""
    if dt == "bf16":
        return (np.ascontiguousarray(raw, np.uint16).astype(np.uint32) << 16).view(np.float32)
    if dt == "f8":
        return E4M3[np.ascontiguousarray(raw, np.uint8)]
    return raw.astype(np.float32)


# ---- the metrics data sets ------------------------------------------------------------------------------------------------------------
M_N, M_NQ = 3000, 12
M_KS = (1, 63, 64, 65, 100, 128, 129, 1000, 1024)
M_SHAPES = [(24, k) for k in M_KS] + [(d, k) for d in (1, 100) for k in (65, 100, 1024)]
# (rows, queries): F32 x F32 runs through both entry points; a byte type takes itself or fp32 queries; the rest fp32 queries
M_PAIRS = (("f32", "f32"), ("u8", "u8"), ("u8", "f32"), ("i8", "i8"), ("i8", "f32"), ("f16", "f32"), ("bf16", "f32"), ("f8", "f32"))
BAD_IDS = (-1, None, I32_MAX)          # None: n, the first id past the base
# queries by role (each edge on a query of its own, so the others stay defined)
Q_PLAIN, Q_TAIL, Q_SHORT, Q_NONE, Q_NEG, Q_CLAMP, Q_BAD0, Q_GTHOLE, Q_ROW, Q_ROW70 = 0, 1, 2, 3, 4, 5, 6, 9, 10, 11
# data sets whose first draw cannot tell the folds apart (tests/test_gt_ref_cpu.py asserts that these can): the draw to take instead
M_SEEDS = {("f32", "f32", 100, 65): 1, ("u8", "u8", 1, 65): 5, ("u8", "f32", 24, 65): 1, ("u8", "f32", 1, 65): 2, ("u8", "f32", 100, 65): 6,
           ("i8", "i8", 24, 100): 1, ("i8", "i8", 1, 65): 14, ("i8", "i8", 1, 100): 1, ("i8", "f32", 24, 65): 1, ("f16", "f32", 1, 65): 3,
           ("bf16", "f32", 24, 65): 4, ("f8", "f32", 24, 129): 1}


def bad_places(k):
    return sorted({p for p in (0, 63, 64, k - 1) if p < k})


@functools.lru_cache(maxsize=None)
def metrics_scene(bdt, qdt, d, k, n=M_N, nq=M_NQ):
    """One data set: raw rows of type bdt, raw queries of type qdt (a byte type's own bytes, or fp32 off the rows' grid), gt =
    the true k + 7 nearest by knn() with the edges of tests/test_gpu_metrics_fold.py planted, ann [nq][k] = gt with about 40 % of
    the places replaced and some ids repeated, counts.  Everything a caller must not change is read-only."""
    seed = 1000 * d + k + 7919 * M_SEEDS.get((bdt, qdt, d, k), 0)
    rng = np.random.default_rng([seed, DTYPES.index(bdt), DTYPES.index(qdt)])
    # (d = 1: uniform over the range, so that the k nearest of a byte query are not all one or two units away: quotients of such
    # distances are dyadic, their sums exact in any order, and no fold could be told from another)
    draw = clustered(rng, d) if d > 1 else lambda cnt: (np.float32(255.0) * rng.random((cnt, 1), dtype=np.float32)).astype(np.float32)
    raw = typed(bdt, draw(n))
    if qdt == bdt and bdt != "f32":
        qraw = typed(qdt, draw(nq))
        while True:                    # a byte query that is a base row has dGt = 0 (at d = 1 that would be every query): move such rows
            hit = (raw[:, None, :] == qraw[None, :, :]).all(axis=2).any(axis=1)
            if not hit.any():
                break
            raw[hit, 0] += 1           # (wraps; twelve queries cannot hold every value)
    else:                              # fp32 queries on the rows' scale with a fraction of a unit added: none is a row
        unit = np.float32(1.0) if bdt in ("u8", "i8") else np.float32(2.0 ** -6)
        qraw = widen(bdt, typed(bdt, draw(nq)))
        qraw = (qraw + unit * (np.float32(0.0625) + np.float32(0.875) * rng.random(qraw.shape, dtype=np.float32))).astype(np.float32)
    X = widen(bdt, raw)
    assert np.isfinite(X).all()
    row, row70 = int(rng.integers(0, n)), int(rng.integers(0, n))
    if n > k + 7:
        qraw[Q_ROW] = raw[row] if qdt == bdt else X[row]
        if k > 70:
            qraw[Q_ROW70] = raw[row70] if qdt == bdt else X[row70]
    Q = widen(qdt, qraw)
    gt, gd2, _ = knn(X, Q, k + 7)
    gt = gt.copy()
    ann = gt[:, :k].copy()
    for i in range(nq):
        m = rng.random(k) < 0.4
        ann[i, m] = rng.integers(0, n, int(m.sum()))
        for _ in range(max(1, k // 16)):                       # some ids twice
            a, b = rng.integers(0, k, 2)
            ann[i, a] = ann[i, b]
    cnt = np.full(nq, k, np.int32)
    cnt[Q_SHORT], cnt[Q_NONE], cnt[Q_NEG] = k - 1, 0, -3       # (Q_CLAMP is set by the caller: it depends on the stride)
    if n > k + 7:
        ann[Q_TAIL, k // 2] = gt[Q_TAIL, k + int(rng.integers(0, 7))]      # a true neighbour just past k: no hit
        places = bad_places(k)
        for j, bad in enumerate(BAD_IDS):
            ann[Q_BAD0 + j, places[(j + k) % len(places)]] = n if bad is None else bad
        if k > 64:
            gt[Q_GTHOLE, (64, k - 1)[k % 2]] = -1                # (its ann holds no -1: that pair is outside the reference's domain)
            assert (ann[Q_GTHOLE] >= 0).all()
        assert gd2[Q_ROW, 0] == 0
        if k > 70:
            assert gd2[Q_ROW70, 0] == 0                          # the row the query equals, moved to the second round of 64
            gt[Q_ROW70, [0, 70]] = gt[Q_ROW70, [70, 0]]
    for a in (raw, qraw, X, Q, gt, gd2, ann, cnt):
        a.setflags(write=False)
    return dict(raw=raw, qraw=qraw, X=X, Q=Q, gt=gt, gd2=gd2, ann=ann, cnt=cnt, n=n, k=k, d=d)


def padded(a, stride, fill):
    """[nq][stride] with a's columns first and `fill` columns after"""
    out = np.empty((a.shape[0], stride), np.int32)
    out[:, :a.shape[1]] = a
    out[:, a.shape[1]:] = fill[:, :stride - a.shape[1]]
    return out


def metrics_call(sc, ann_stride, gt_stride):
    """(ann [nq][ann_stride], counts, gt [nq][gt_stride]) of one call: places past k of ann hold true neighbours (hits, were they
    counted), the count of Q_CLAMP is stride + 9"""
    k = sc["k"]
    ann = padded(sc["ann"], ann_stride, sc["gt"])
    cnt = sc["cnt"].copy()
    cnt[Q_CLAMP] = ann_stride + 9
    return ann, cnt, np.ascontiguousarray(sc["gt"][:, :gt_stride])


def tiny_scene():
    """n = 5, k = 5, d = 1: every place of every row in use"""
    X = np.array([[3.0], [1.0], [4.0], [1.5], [9.0]], np.float32)
    Q = np.array([[2.25], [0.0], [10.0]], np.float32)
    gt, _, _ = knn(X, Q, 5)
    ann = np.array([[1, 3, 0, 2, 4], [4, 4, 1, 5, 2], [0, 1, 2, 3, 3]], np.int32)      # (5 = n: no row)
    return dict(X=X, Q=Q, gt=gt, ann=ann, cnt=np.array([5, 5, 4], np.int32), n=5, k=5, d=1)


# ---- wrong folds of the ratio's terms: what the data must be able to tell from the index-order sum --------------------------------
def fold_index(t):
    s = 0.0
    for v in t:
        s += v
    return s


def fold_pairwise(t):
    return float(np.sum(np.asarray(t, np.float64)))


def fold_lane_major(t):
    return fold_index([t[i] for l in range(64) for i in range(l, len(t), 64)])


def fold_first_round(t):
    return fold_index(t[:64]) * (len(t) / 64.0)


WRONG_FOLDS = (fold_pairwise, fold_lane_major, fold_first_round)


def folds_not_told_apart(sc):
    """names of the wrong computations that give the right bits on every query of a k > 64 data set (the list must be empty)"""
    k = sc["k"]
    X64, Q64 = sc["X"].astype(np.float64), sc["Q"].astype(np.float64)
    ann, cnt, g = metrics_call(sc, k, k + 7)
    rec, rat = metrics(X64, Q64, k, ann, cnt, g)
    terms = {qi: ratio_terms(X64, Q64[qi], ann[qi], g[qi], k) for qi in (Q_PLAIN, Q_TAIL, Q_CLAMP)}
    for qi, t in terms.items():
        assert None not in t and fold_index(t) / k == rat[qi]
    same = [w.__name__ for w in WRONG_FOLDS if all(w(t) / k == rat[qi] for qi, t in terms.items())]
    rec64, _ = metrics(X64, Q64, k, np.ascontiguousarray(ann[:, :64]), np.minimum(cnt, 64), g)
    return same + (["recall over ann[:64]"] if np.array_equal(rec64, rec) else [])


# ---- the selection data sets: small integers, which every row type holds ---------------------------------------------------------
S_IDENT_N, S_IDENT_K = (1, 255, 256, 257, 1025, 70001), (1, 256, 257, 1024)
S_BOUND_K = (1, 136, 137, 300, 699, 700, 701, 1000)
S_BOUND_N, S_BOUND_LO, S_BOUND_HI, S_BOUND_FARQ = 66800, 65400, 66100, 5
S_TOP_N, S_TOP_ZEROS = 2 ** 24 + 300, 300


def sel_identical(n):
    """every row the same: (V [n][8], Q [3][8]) float32"""
    V = np.full((n, 8), 2, np.float32)
    Q = np.array([[2] * 8, [0] * 8, [3, 1, 0, 2, 3, 3, 1, 0]], np.float32)
    return V, Q


def sel_boundary():
    """n = 66800: rows [65400, 66100) are all ones (700 rows, the nearest), every other row all threes; 17 queries of zeros and
    ones, but for query 5, all threes, to which the far rows are the nearer ones"""
    V = np.full((S_BOUND_N, 8), 3, np.float32)
    V[S_BOUND_LO:S_BOUND_HI] = 1
    Q = np.random.default_rng(41).integers(0, 2, (17, 8)).astype(np.float32)
    Q[0] = 1
    Q[S_BOUND_FARQ] = 3
    return V, Q


def sel_boundary_ids(k, far):
    """the expected ids in closed form"""
    near = np.arange(S_BOUND_LO, S_BOUND_HI)
    rest = np.concatenate([np.arange(0, S_BOUND_LO), np.arange(S_BOUND_HI, S_BOUND_N)])
    return (np.concatenate([rest, near]) if far else np.concatenate([near, rest]))[:k].astype(np.int32)


def sel_top_ids(k):
    z0 = S_TOP_N - S_TOP_ZEROS
    return np.concatenate([np.arange(z0, S_TOP_N), np.arange(0, z0)])[:k].astype(np.int32)


def sel_mantissa():
    """d = 2, q = 0: row j = (1, j 2^-26) in a random order, so d2 = 1 + j^2 2^-52 exactly and the keys share their top five or six
    bytes; a row equal to the query, and rows whose difference from it is a float subnormal.  A second query, off the grid."""
    perm = np.random.default_rng(43).permutation(3000)
    V = np.stack([np.ones(3000), perm * 2.0 ** -26], axis=1).astype(np.float32)
    assert np.array_equal(V[:, 1].astype(np.float64), perm * 2.0 ** -26)
    V[17] = (0, 0)
    V[400] = (1, 2.0 ** -140)           # d2 = 1 + 2^-280 = 1: ties with j = 0 by id
    V[2500] = (0, 2.0 ** -140)          # d2 = 2^-280
    V[2501] = (0, -2.0 ** -149)         # d2 = 2^-298
    V[33] = (2.0 ** -130, 0)
    Q = np.array([[0, 0], [0, 2.0 ** -27]], np.float32)
    return V, Q


S_MANT_K = (1, 255, 1024)
S_K1024_N = (1024, 1025, 5000)


def sel_k1024(n, kind):
    rng = np.random.default_rng(n + len(kind))
    if kind == "normal":
        return rng.standard_normal((n, 8)).astype(np.float32), rng.standard_normal((5, 8)).astype(np.float32)
    V = rng.integers(0, 4, (n, 8)).astype(np.float32)          # the data of the existing tie test: a third of the rows twice
    V[n // 3:2 * (n // 3)] = V[:n // 3]
    return V, rng.integers(0, 4, (5, 8)).astype(np.float32)


def sel_nonfinite():
    """n = 600, d = 4: rows of +-3e38 against queries of -+3e38 (the float subtraction overflows: d2 = +inf, ties by id), rows with
    NaN or +-inf elements"""
    rng = np.random.default_rng(47)
    V = rng.standard_normal((600, 4)).astype(np.float32)
    Q = rng.standard_normal((5, 4)).astype(np.float32)
    V[10:40:3] = 3e38
    V[200:260:7] = -3e38
    V[300, 1], V[301, 0], V[555, 3] = np.inf, -np.inf, np.inf
    V[5, 2], V[302, :], V[599, 0], V[123, 3] = np.nan, np.nan, np.nan, np.nan
    V[450] = (np.inf, np.nan, 0, 1)
    Q[1], Q[2] = -3e38, 3e38
    Q[3, 0] = 3e38
    return V, Q


S_TILE_NQ, S_TILE_N, S_TILE_D = (1, 15, 16, 17, 33), (1, 255, 256, 257), (1, 3)


def sel_tiles(nq, n, d):
    rng = np.random.default_rng(1000 * nq + 10 * n + d)
    return rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
