"""GPU: fspann_eval_kvariants_dev — recall, distance ratio and candidate ratio at every k of ks from one result list, one launch.
Row j of recall / ratio must be what fspann_eval_metrics_typed_dev writes for k = ks[j] over the same arguments, compared as uint64
(NaN payloads included: there is no tolerance); for fp32 rows the oracle's computeMetricsAtK is a second judge.  Data sets are
tests/gt_ref.py's (invalid ids, dGt = 0, short, zero, negative and clamped counts, repeated ids, a gt hole), at d in {1, 7, 16, 100,
128} (rows of whole 16-byte pieces and not, per row type) and kmax in {1, 63, 64, 65, 100, 1024} (the fold's rounds of 64; the
largest k), for every pair of row and query type the call takes.  ks is unsorted and holds a repeat."""
import itertools

import numpy as np
import pytest

import gt_ref as R

pytestmark = pytest.mark.gpu

DS = (1, 7, 16, 100, 128)
KMAX = (1, 63, 64, 65, 100, 1024)
UNIQUE = (0, -3, 1, 257)
NAN_BITS = np.uint64(0x7FF8000000000000)


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=16), 0) as c:
        yield c


def _codes(pkg):
    N = pkg._native
    return dict(f32=N.F32, f64=N.F64, u8=N.U8, i8=N.I8, f16=N.F16, bf16=N.BF16, f8=N.F8E4M3)


def _dev(a, off=0):
    """the array on the device; off: that many elements past a 256-byte boundary"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:                                 # (bfloat16 patterns: bytes are bytes)
        a = a.view(np.int16)
    t = torch.from_numpy(a.copy().reshape(-1))
    buf = torch.zeros(t.numel() + off, dtype=t.dtype, device=torch.device("cuda", 0))
    buf[off:] = t
    return buf[off:]


def _ks(kmax):
    return [min(max(k, 1), kmax) for k in (kmax, 1, 10, 10, kmax - 1)]


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _sweep(pkg, ctx, bdt, qdt, xd, qd, n, nq, d, ks, ann, cnt, gt, unique, spare=0):
    """one call -> recall, ratio, cand_ratio [nk][nq] (cand_ratio None without unique) and the `spare` canary rows behind them"""
    import torch
    c = _codes(pkg)
    ad, gd = _dev(ann), _dev(gt)
    cd = None if cnt is None else _dev(cnt)
    ud = None if unique is None else _dev(unique)
    nk = len(ks)
    out = torch.full((3 + spare, nk, nq), -7.0, dtype=torch.float64, device=torch.device("cuda", 0))
    ctx.eval_kvariants_dev(n, xd.data_ptr(), c[bdt], nq, qd.data_ptr(), c[qdt], d, ks, ad.data_ptr(), ann.shape[1], _ptr(cd), gd.data_ptr(), gt.shape[1],
                           _ptr(ud), out[0].data_ptr(), out[1].data_ptr(), 0 if unique is None else out[2].data_ptr())
    ctx.sync()
    o = out.cpu().numpy()
    return o[0], o[1], (None if unique is None else o[2]), o[2 if unique is None else 3:]


def _per_k(pkg, ctx, bdt, qdt, xd, qd, n, nq, d, ks, ann, cnt, gt):
    """the specification: one fspann_eval_metrics_typed_dev call per k"""
    import torch
    c = _codes(pkg)
    ad, gd = _dev(ann), _dev(gt)
    cd = None if cnt is None else _dev(cnt)
    out = torch.full((2, len(ks), nq), -7.0, dtype=torch.float64, device=torch.device("cuda", 0))
    for j, k in enumerate(ks):
        ctx.eval_metrics_typed_dev(n, xd.data_ptr(), c[bdt], nq, qd.data_ptr(), c[qdt], d, k, ad.data_ptr(), ann.shape[1], _ptr(cd), gd.data_ptr(), gt.shape[1],
                                   out[0, j].data_ptr(), out[1, j].data_ptr())
    ctx.sync()
    o = out.cpu().numpy()
    return o[0], o[1]


def _cand(unique, ks):
    u = np.asarray(unique, np.int64)[None, :].astype(np.float64)
    k = np.asarray(ks, np.float64)[:, None]
    want = u / k
    want.view(np.uint64)[np.broadcast_to(u <= 0, want.shape)] = NAN_BITS
    return want


def _same_bits(got, want, what):
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (what, bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("kmax", KMAX)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("bdt,qdt", R.M_PAIRS)
def test_every_k_equals_the_per_k_call(pkg, oracle, ctx, bdt, qdt, d, kmax):
    sc = R.metrics_scene(bdt, qdt, d, kmax)
    n, nq = sc["n"], len(sc["Q"])
    ks = _ks(kmax)
    xd, qd = _dev(sc["raw"]), _dev(sc["qraw"])
    unique = np.array([UNIQUE[i % 4] for i in range(nq)], np.int32)
    # ann_stride = kmax with counts (short, zero, negative, clamped), then ann_stride > kmax without counts; gt_stride = kmax + 7
    for ann_stride, counts in ((kmax, True), (kmax + 5, False)):
        ann, cnt, gt = R.metrics_call(sc, ann_stride, kmax + 7)
        cnt = cnt if counts else None
        rec, rat, cr, _ = _sweep(pkg, ctx, bdt, qdt, xd, qd, n, nq, d, ks, ann, cnt, gt, unique)
        wrec, wrat = _per_k(pkg, ctx, bdt, qdt, xd, qd, n, nq, d, ks, ann, cnt, gt)
        what = "%s x %s d %d ks %s ann_stride %d counts %s: " % (bdt, qdt, d, ks, ann_stride, counts)
        _same_bits(rec, wrec, what + "recall")
        _same_bits(rat, wrat, what + "ratio")
        _same_bits(cr, _cand(unique, ks), what + "cand_ratio")
        assert np.isnan(wrat).any() and (~np.isnan(wrat)).any()
        if bdt == "f32":
            for j, k in enumerate(ks):
                orec, orat = oracle.metrics(sc["X"], sc["Q"], k, ann, cnt, gt)
                _same_bits(rec[j], orec, what + "recall against the oracle, k %d" % k)
                assert np.array_equal(np.isnan(rat[j]), np.isnan(orat)), what
                ok = ~np.isnan(orat)
                _same_bits(rat[j][ok], orat[ok], what + "ratio against the oracle, k %d" % k)


@pytest.mark.parametrize("bdt,qdt,d", [("f32", "f32", 16), ("u8", "u8", 16), ("f16", "f32", 128), ("bf16", "f32", 16), ("f8", "f32", 128), ("i8", "f32", 16)])
def test_base_off_a_16_byte_boundary_and_few_queries(pkg, ctx, bdt, qdt, d):
    """rows of whole pieces whose matrix starts one element past a 16-byte boundary take the element loop; nq = 5; gt_stride = kmax"""
    kmax = 65
    sc = R.metrics_scene(bdt, qdt, d, kmax)
    n, nq = sc["n"], 5
    ks = _ks(kmax)
    xd, qd = _dev(sc["raw"], off=1), _dev(sc["qraw"][:nq], off=3)
    assert xd.data_ptr() % 16 != 0
    ann, cnt, gt = R.metrics_call(sc, kmax + 5, kmax)
    ann, cnt, gt = ann[:nq], cnt[:nq], gt[:nq]
    rec, rat, cr, _ = _sweep(pkg, ctx, bdt, qdt, xd, qd, n, nq, d, ks, ann, cnt, gt, np.arange(nq, dtype=np.int32))
    wrec, wrat = _per_k(pkg, ctx, bdt, qdt, xd, qd, n, nq, d, ks, ann, cnt, gt)
    _same_bits(rec, wrec, "recall")
    _same_bits(rat, wrat, "ratio")
    _same_bits(cr, _cand(np.arange(nq), ks), "cand_ratio")


def test_no_unique_leaves_the_next_buffer_alone_and_no_queries_write_nothing(pkg, ctx):
    sc = R.metrics_scene("f32", "f32", 16, 100)
    n, nq, ks = sc["n"], 6, _ks(100)
    xd, qd = _dev(sc["raw"]), _dev(sc["qraw"][:nq])
    ann, cnt, gt = R.metrics_call(sc, 100, 107)
    ann, cnt, gt = ann[:nq], cnt[:nq], gt[:nq]
    rec, rat, cr, spare = _sweep(pkg, ctx, "f32", "f32", xd, qd, n, nq, 16, ks, ann, cnt, gt, None, spare=1)
    wrec, wrat = _per_k(pkg, ctx, "f32", "f32", xd, qd, n, nq, 16, ks, ann, cnt, gt)
    _same_bits(rec, wrec, "recall")
    _same_bits(rat, wrat, "ratio")
    assert cr is None and (spare == -7.0).all()
    # nq = 0: nothing is written (the outputs hold the canary), with and without unique
    import torch
    out = torch.full((3, len(ks), nq), -7.0, dtype=torch.float64, device=torch.device("cuda", 0))
    ad, gd, ud = _dev(ann), _dev(gt), _dev(np.ones(nq, np.int32))
    for u, c in ((0, 0), (ud.data_ptr(), out[2].data_ptr())):
        ctx.eval_kvariants_dev(n, xd.data_ptr(), 0, 0, qd.data_ptr(), 0, 16, ks, ad.data_ptr(), 100, 0, gd.data_ptr(), 107, u, out[0].data_ptr(),
                               out[1].data_ptr(), c)
    ctx.sync()
    assert (out.cpu().numpy() == -7.0).all()


@pytest.mark.parametrize("bdt,qdt", [("f32", "f32"), ("u8", "u8"), ("u8", "f32"), ("f16", "f32")])
def test_numpy_level_call_is_the_device_call(pkg, ctx, bdt, qdt):
    """FspannContext.eval_kvariants over host arrays (rows kept in their type, byte queries kept as bytes over byte rows) against
    eval_kvariants_dev over the same data: with counts and unique, without either, and with no query at all."""
    d, kmax = 16, 65
    sc = R.metrics_scene(bdt, qdt, d, kmax)
    n, nq, ks = sc["n"], len(sc["Q"]), _ks(kmax)
    xd, qd = _dev(sc["raw"]), _dev(sc["qraw"])
    ann, cnt, gt = R.metrics_call(sc, kmax + 5, kmax + 7)
    unique = np.array([UNIQUE[i % 4] for i in range(nq)], np.int32)
    for counts, uq in ((cnt, unique), (None, None)):
        rec, rat, cr, _ = _sweep(pkg, ctx, bdt, qdt, xd, qd, n, nq, d, ks, ann, counts, gt, uq)
        got = ctx.eval_kvariants(sc["raw"], sc["qraw"], ks, ann, counts, gt, unique=uq)
        assert sorted(got) == ["cand_ratio", "ratio", "recall"]
        _same_bits(got["recall"], rec, "recall")
        _same_bits(got["ratio"], rat, "ratio")
        if uq is None:
            assert got["cand_ratio"] is None and cr is None
        else:
            _same_bits(got["cand_ratio"], cr, "cand_ratio")
    if bdt == "u8":                                          # values handed over as floats with dtype=: the same rows
        rec, rat, _, _ = _sweep(pkg, ctx, bdt, qdt, xd, qd, n, nq, d, ks, ann, cnt, gt, None)
        again = ctx.eval_kvariants(sc["X"], sc["qraw"], ks, ann, cnt, gt, dtype=np.uint8)
        _same_bits(again["recall"], rec, "dtype=uint8: recall")
        _same_bits(again["ratio"], rat, "dtype=uint8: ratio")
        assert np.isnan(rat).any() and (~np.isnan(rat)).any()
    none = ctx.eval_kvariants(sc["raw"], sc["qraw"][:0], ks, ann[:0], cnt[:0], gt[:0], unique=unique[:0])
    assert all(none[k].shape == (len(ks), 0) for k in ("recall", "ratio", "cand_ratio"))
    with pytest.raises(pkg.FspannArgumentError):
        ctx.eval_kvariants(sc["raw"], sc["qraw"][:, :d - 1], ks, ann, cnt, gt)


def test_refusals(pkg, ctx):
    import torch
    N = pkg._native
    c = _codes(pkg)
    sc = R.metrics_scene("f32", "f32", 16, 100)
    n, nq = sc["n"], 4
    xd, qd = _dev(sc["raw"]), _dev(sc["qraw"][:nq])
    ann, cnt, gt = R.metrics_call(sc, 100, 107)
    ad, gd, ud = _dev(ann[:nq]), _dev(gt[:nq]), _dev(np.ones(nq, np.int32))
    out = torch.full((3, 65, nq), -7.0, dtype=torch.float64, device=torch.device("cuda", 0))

    def call(ks, bdt="f32", qdt="f32", gt_stride=107, unique=True, cand=True, ann_stride=100):
        ctx.eval_kvariants_dev(n, xd.data_ptr(), c[bdt], nq, qd.data_ptr(), c[qdt], 16, ks, ad.data_ptr(), ann_stride, 0, gd.data_ptr(), gt_stride,
                               ud.data_ptr() if unique else 0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr() if cand else 0)

    call([100, 1, 10])                                    # (the arguments the refusals below vary are good)
    for ks in ([], [5] * 65, [5, 0], [1025, 5], [-1]):
        with pytest.raises(N.FspannArgumentError):
            call(ks)
    call([5] * 64)
    with pytest.raises(N.FspannArgumentError):
        call([100, 5], gt_stride=99)
    call([100, 5], gt_stride=100)
    with pytest.raises(N.FspannArgumentError):
        call([5], ann_stride=0)
    for unique, cand in ((True, False), (False, True)):
        with pytest.raises(N.FspannArgumentError):
            call([5], unique=unique, cand=cand)
    names = dict(f32="FSPANN_F32", f64="FSPANN_F64", u8="FSPANN_U8", i8="FSPANN_I8", f16="FSPANN_F16", bf16="FSPANN_BF16", f8="FSPANN_F8E4M3")
    refused = [p for p in itertools.product(names, names) if p not in R.M_PAIRS]
    assert len(refused) == 49 - 8
    for bdt, qdt in refused:
        with pytest.raises(N.FspannArgumentError) as e:
            call([5], bdt=bdt, qdt=qdt)
        with pytest.raises(N.FspannArgumentError) as e1:            # the per-k call refuses the same pair in the same words
            ctx.eval_metrics_typed_dev(n, xd.data_ptr(), c[bdt], nq, qd.data_ptr(), c[qdt], 16, 5, ad.data_ptr(), 100, 0, gd.data_ptr(), 107,
                                       out[0].data_ptr(), out[1].data_ptr())
        assert str(e.value) == str(e1.value) and names[bdt] in str(e.value) and names[qdt] in str(e.value), (bdt, qdt, str(e.value))
    ctx.sync()
    with pytest.raises(N.FspannNullError):
        ctx.eval_kvariants_dev(n, 0, 0, nq, qd.data_ptr(), 0, 16, [5], ad.data_ptr(), 100, 0, gd.data_ptr(), 107, 0, out[0].data_ptr(), out[1].data_ptr(), 0)
