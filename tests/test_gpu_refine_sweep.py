"""GPU: fspann_refine_store_sweep_dev / fspann_refine_sweep_dev — Refine at several refinement limits from one scan.

The judge is the library's own single-limit call: plane j must be bit-identical (ids, counts, scored, distances compared as
uint64) to fspann_refine_store_dev with B = stride and every count replaced by min(max(count, 0), limits[j]).  For F32 / F64 rows
oracle.refine is a second judge.  One store of 4 096 rows per row dtype, candidate ids built here (no index), nq = 8, stride 700:

  query 0  count 700; ids -1 and >= n (points that failed to load) and non-finite rows at positions 254..257 and 510..513, so that
           `scored` differs on each side of the limits 255 / 256 / 257 and 511 / 512
  query 1  count 699; four all-zero store rows (distinct ids, equal bytes) at positions 255 | 256 and 511 | 512 and a query next to
           zero: the twins are the nearest rows at equal distance and straddle the limits 256 and 512 — the later twin must be
           absent from the earlier plane and must lose the tie in the later one
  others   counts 0, -1, 1, 256, 257 and 5 000 (above the stride: clamped as the single-limit call clamps it)
and every call is made a second time with query 4 (count 256) turned into NaN."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32, F64, U8, F16, BF16, F8, I8 = range(7)
N, NQ, STRIDE = 4096, 8, 700
COUNTS = np.array([700, 699, 0, -1, 256, 1, 257, 5000], np.int32)
LIMITS = [1, 255, 256, 257, 511, 512, 700]
LIMITS16 = [1, 2, 64, 255, 256, 257, 300, 400, 511, 512, 513, 600, 650, 698, 699, 700]
KS = (1, 10, 100, 257, 1024)
TWINS = (4000, 4001, 4002, 4003)      # all-zero store rows
NONFINITE = (4010, 4011)              # non-finite store rows (dtypes that have any)
CANARY = -77


def _store(rng, dt, d):
    """raw store rows [N][d] of row dtype dt (as the library takes them), None or the float64 values, whether a row can be non-finite"""
    if dt in (F32, F64):
        X = rng.standard_normal((N, d)).astype(np.float32 if dt == F32 else np.float64)
        X[list(TWINS)] = 0
        X[NONFINITE[0]] = np.nan
        X[NONFINITE[1], d // 2] = np.inf
        return X, X.astype(np.float64), True
    if dt == F16:
        X = rng.standard_normal((N, d)).astype(np.float16)
        X[list(TWINS)] = 0
        X[NONFINITE[0], 0] = np.nan
        X[NONFINITE[1], d - 1] = -np.inf
        return X, None, True
    if dt == BF16:
        X = (rng.standard_normal((N, d)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
        X[list(TWINS)] = 0
        X[NONFINITE[0], 1] = 0x7FC0
        X[NONFINITE[1], d - 2] = 0xFF80
        return X, None, True
    X = rng.integers(1, 255, (N, d)).astype(np.uint8)
    X[list(TWINS)] = 0
    if dt == F8:
        X[np.isin(X, (0x7F, 0xFF))] = 0x3C
        X[NONFINITE[0], 2] = 0x7F
        X[NONFINITE[1], d - 3] = 0xFF
        return X, None, True
    return (X if dt == U8 else X.view(np.int8)), None, False


def _cand_ids(rng, can_be_nonfinite):
    ids = rng.integers(0, 3999, (NQ, STRIDE)).astype(np.int32)
    bad_row = NONFINITE if can_be_nonfinite else (-1, N + 9)
    ids[0, 254], ids[0, 255], ids[0, 256], ids[0, 257] = -1, N + 5, bad_row[0], N
    ids[0, 510], ids[0, 511], ids[0, 512], ids[0, 513] = bad_row[1], -1, 2**31 - 1, bad_row[0]
    ids[1, 255], ids[1, 256], ids[1, 511], ids[1, 512] = TWINS
    return ids


def _queries(rng, qdt, d):
    Q = rng.standard_normal((NQ, d))
    Q[1] *= 1e-3                      # next to the zero rows
    Q = Q.astype(np.float32 if qdt == F32 else np.float64)
    Qn = Q.copy()
    Qn[4, d // 3] = np.nan
    return Q, Qn


class _Run:
    def __init__(self, ctx, ids, d):
        import torch
        self.torch, self.dev, self.ctx, self.d = torch, torch.device("cuda", 0), ctx, d
        self.ids_h = ids
        self.ids = torch.from_numpy(ids).to(self.dev)
        self.cnt = torch.from_numpy(COUNTS).to(self.dev)

    def _out(self, nl, k):
        t, dev = self.torch, self.dev
        return dict(ids=t.full((nl + 1, NQ, k), CANARY, dtype=t.int32, device=dev), dist=t.full((nl + 1, NQ, k), -5.0, dtype=t.float64, device=dev),
                    count=t.full((nl + 1, NQ), CANARY, dtype=t.int32, device=dev), scored=t.full((nl + 1, NQ), CANARY, dtype=t.int32, device=dev))

    def _down(self, o, nl):
        self.ctx.sync()
        h = {key: v.cpu().numpy() for key, v in o.items()}
        assert (h["ids"][nl] == CANARY).all() and (h["dist"][nl] == -5.0).all() and (h["count"][nl] == CANARY).all() and (h["scored"][nl] == CANARY).all()
        return {key: v[:nl] for key, v in h.items()}

    def sweep(self, qd, qdt, limits, k, cand=None, cand_dt=None):
        o = self._out(len(limits), k)
        outs = (o["ids"].data_ptr(), o["dist"].data_ptr(), o["count"].data_ptr(), o["scored"].data_ptr())
        if cand is None:
            self.ctx.refine_store_sweep_dev(NQ, qd.data_ptr(), qdt, STRIDE, self.ids.data_ptr(), self.cnt.data_ptr(), limits, k, *outs)
        else:
            self.ctx.refine_sweep_dev(NQ, qd.data_ptr(), qdt, cand.data_ptr(), cand_dt, STRIDE, self.ids.data_ptr(), self.cnt.data_ptr(), limits, k, *outs)
        return self._down(o, len(limits))

    def single(self, qd, qdt, limit, k, cand=None, cand_dt=None):
        """the judge: the single-limit call with B = stride and the counts clipped to `limit`"""
        o = self._out(1, k)
        outs = (o["ids"].data_ptr(), o["dist"].data_ptr(), o["count"].data_ptr(), o["scored"].data_ptr())
        cl = self.torch.from_numpy(np.minimum(np.maximum(COUNTS, 0), limit).astype(np.int32)).to(self.dev)
        if cand is None:
            self.ctx.refine_store_dev(NQ, qd.data_ptr(), qdt, STRIDE, self.ids.data_ptr(), cl.data_ptr(), k, *outs)
        else:
            self.ctx.refine_dev(NQ, qd.data_ptr(), qdt, cand.data_ptr(), cand_dt, STRIDE, self.ids.data_ptr(), cl.data_ptr(), k, *outs)
        return {key: v[0] for key, v in self._down(o, 1).items()}


def _same(got, j, ref, what):
    assert np.array_equal(got["count"][j], ref["count"]), (what, got["count"][j], ref["count"])
    assert np.array_equal(got["scored"][j], ref["scored"]), (what, got["scored"][j], ref["scored"])
    assert np.array_equal(got["ids"][j], ref["ids"]), (what, np.flatnonzero((got["ids"][j] != ref["ids"]).any(1)))
    assert np.array_equal(got["dist"][j].view(np.uint64), ref["dist"].view(np.uint64)), what


def _ctx(pkg, d):
    cfg = pkg.PaperRuntimeConfig(tables=2, divisions=1, m=4, lambda_=2, dim=d, refinement_limit=STRIDE, block_size=8, default_probes=1)
    return pkg.FspannContext(cfg, 0)


def _twin_checks(got, limits, k):
    """query 1: the zero rows at positions 255 | 256 and 511 | 512 are its nearest rows, at one distance"""
    t1, t2, t3, t4 = TWINS
    for j, lim in enumerate(limits):
        want = [t for t, pos in zip(TWINS, (255, 256, 511, 512)) if pos < min(lim, 699)][:k]      # in candidate order: the earlier position wins the tie
        row = got["ids"][j][1]
        assert list(row[:len(want)]) == want, (lim, k, row[:4])
        assert not np.isin(row[len(want):], TWINS).any(), (lim, k)


CASES = [(dt, qdt, 32) for dt in (F32, F64, U8, F16, BF16, F8, I8) for qdt in (F32, F64)] + [(F32, F32, 18), (F32, F64, 18)]


@pytest.mark.parametrize("dt,qdt,d", CASES)
def test_planes_equal_the_single_limit_call(pkg, oracle, dt, qdt, d):
    import torch
    rng = np.random.default_rng(100 * dt + 10 * qdt + d)
    X, X64, nonfinite = _store(rng, dt, d)
    ids = _cand_ids(rng, nonfinite)
    Q, Qn = _queries(rng, qdt, d)
    told = set()
    with _ctx(pkg, d) as ctx:
        ctx.store_set(X, dtype={BF16: pkg.bfloat16, F8: pkg.float8_e4m3fn}.get(dt, X.dtype))
        run = _Run(ctx, ids, d)
        for Qv, has_nan in ((Q, False), (Qn, True)):
            qd = torch.from_numpy(Qv).to(run.dev)
            for k in KS:
                judge = {lim: run.single(qd, qdt, lim, k) for lim in sorted(set(LIMITS + LIMITS16 + [300]))}
                for limits in (LIMITS, [300], LIMITS16):
                    got = run.sweep(qd, qdt, limits, k)
                    for j, lim in enumerate(limits):
                        _same(got, j, judge[lim], (dt, qdt, d, k, lim, has_nan))
                    _twin_checks(got, limits, k)
                    if has_nan:
                        assert (got["count"][:, 4] == 0).all() and (got["scored"][:, 4] == 0).all() and (got["ids"][:, 4] == -1).all()
                # what the scene claims: scored differs across the planted limits, the clamp, the empty and the short queries
                sc = {lim: judge[lim]["scored"] for lim in LIMITS}
                assert sc[255][0] == 254 and sc[257][0] == 254 and sc[511][0] == 506 and sc[700][0] == 692, sc
                assert (judge[700]["count"][[2, 3]] == 0).all() and judge[700]["scored"][7] == 700 and judge[700]["scored"][5] == 1
                told.add(int(judge[255]["count"][0] < k))
                if X64 is not None and not has_nan:
                    # second judge: the oracle's refine over the same rows (a point that failed to load has no row: NaN)
                    safe = np.where((ids >= 0) & (ids < N), ids, NONFINITE[0])
                    cand = X64[safe]
                    for lim in LIMITS:
                        oi, od, oc = oracle.refine(Qv.astype(np.float64), cand, ids, np.minimum(np.maximum(COUNTS, 0), lim), k)
                        assert np.array_equal(oc, judge[lim]["count"]), (lim, k)
                        for q in range(NQ):
                            c = oc[q]
                            assert np.array_equal(oi[q, :c], judge[lim]["ids"][q, :c]) and np.array_equal(od[q, :c], judge[lim]["dist"][q, :c]), (lim, k, q)
    assert told == {0, 1}          # a k below and a k above what a limit scores (out_count < k)


def test_dense_rows(pkg):
    """fspann_refine_sweep_dev over caller-held rows [nq][stride][dim] against fspann_refine_dev"""
    import torch
    d = 32
    rng = np.random.default_rng(5)
    X, X64, _ = _store(rng, F32, d)
    ids = _cand_ids(rng, True)
    Q, _ = _queries(rng, F32, d)
    cand_h = X[np.where((ids >= 0) & (ids < N), ids, NONFINITE[0])]
    with _ctx(pkg, d) as ctx:
        run = _Run(ctx, ids, d)
        qd, cand = torch.from_numpy(Q).to(run.dev), torch.from_numpy(np.ascontiguousarray(cand_h)).to(run.dev)
        for k in (10, 257):
            got = run.sweep(qd, F32, LIMITS, k, cand, F32)
            for j, lim in enumerate(LIMITS):
                _same(got, j, run.single(qd, F32, lim, k, cand, F32), (k, lim))
            _twin_checks(got, LIMITS, k)


def test_one_workgroup_per_chunk_scan(pkg, monkeypatch):
    """the scan the stream does not take (FSPANN_REFINE_STREAM=0) leaves the same keys"""
    import torch
    d = 32
    rng = np.random.default_rng(6)
    X, _, _ = _store(rng, F16, d)
    ids = _cand_ids(rng, True)
    Q, _ = _queries(rng, F32, d)
    monkeypatch.setenv("FSPANN_REFINE_STREAM", "0")
    with _ctx(pkg, d) as ctx:
        ctx.store_set(X, dtype=X.dtype)
        run = _Run(ctx, ids, d)
        qd = torch.from_numpy(Q).to(run.dev)
        got = run.sweep(qd, F32, LIMITS, 100)
        for j, lim in enumerate(LIMITS):
            _same(got, j, run.single(qd, F32, lim, 100), lim)


def test_argument_errors(pkg):
    import torch
    d = 32
    rng = np.random.default_rng(7)
    X, _, _ = _store(rng, F32, d)
    ids = _cand_ids(rng, True)
    Q, _ = _queries(rng, F32, d)
    with _ctx(pkg, d) as ctx:
        run = _Run(ctx, ids, d)
        qd = torch.from_numpy(Q).to(run.dev)
        o = run._out(17, 8)
        outs = (o["ids"].data_ptr(), o["dist"].data_ptr(), o["count"].data_ptr(), o["scored"].data_ptr())

        def call(limits, k=8, stride=STRIDE, nq=NQ):
            ctx.refine_store_sweep_dev(nq, qd.data_ptr(), F32, stride, run.ids.data_ptr(), run.cnt.data_ptr(), limits, k, *outs)

        with pytest.raises(pkg.FspannStateError):            # no store yet
            call([10, 20])
        ctx.store_set(X)
        for limits, word in (([20, 10], "ascending"), ([10, 10], "ascending"), ([], "nl"), (list(range(1, 18)), "nl"), ([0, 5], "limits[0]"),
                             ([5, 2**31], "limits[1]")):
            with pytest.raises(pkg.FspannArgumentError, match=word.replace("[", r"\[").replace("]", r"\]")):
                call(limits)
        for k in (0, 1025):
            with pytest.raises(pkg.FspannArgumentError, match="k "):
                call([10, 20], k=k)
        with pytest.raises(pkg.FspannArgumentError, match="stride"):
            call([10, 701])
        with pytest.raises(pkg.FspannArgumentError, match="stride"):
            call([10, 20], stride=19)
        call([10, 20], nq=0)                                  # empty batch: nothing written
        ctx.sync()
        assert (o["ids"].cpu().numpy() == CANARY).all() and (o["count"].cpu().numpy() == CANARY).all()
        call([10, 20])
        ctx.sync()
        assert (o["count"].cpu().numpy()[:2] != CANARY).all() and (o["count"].cpu().numpy()[2:] == CANARY).all()
