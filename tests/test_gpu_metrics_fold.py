"""GPU: gt_metrics_kernel<TB, TQ> (fspann_eval_metrics_dev / _typed_dev) at k on both sides of 64 and up to 1024,
where the ratio's fold takes more than one round of 64 lanes and the recall loop strides: k in {1, 63, 64, 65, 100, 128, 129, 1000,
1024} at d = 24, {65, 100, 1024} at d = 1 and 100, n = 3000, 12 queries, every pair of row and query type the call takes, rows on
each type's own grid.  Expected values come from tests/gt_ref.py (a plain restatement of computeMetricsAtK; typed rows go in as the
fp64 values of their elements) and, as a second judge, from the oracle over the fp32 copy.  NaN places must be the same; everything
else is compared in its bits: there is no tolerance.  tests/test_gt_ref_cpu.py shows that each k > 64 data set gives other bits
under a pairwise fold, a lane-major fold, a dropped round and a recall over the first 64 places.

A call: gt = the true k + 7 nearest at gt_stride = k + 7 (and k, for k <= 128); ann = gt with about 40 % of the places replaced and
some ids repeated, at ann_stride = k (what bench.py passes) and k + 5; once with counts and once with the count pointer 0.  By query:
0 plain; 1 holds a true neighbour from gt[k : k + 7] (no hit); 2, 3, 4 have counts k - 1, 0, -3; 5 has count stride + 9 (clamps);
6, 7, 8 hold the ann ids -1, n, 2^31 - 1 at one of the places 0, 63, 64, k - 1 (which one moves with k); 9 has gt id -1 at place 64
or k - 1 (k > 64; its ann holds no -1); 10 equals a base row (dGt = 0 at place 0); 11 equals a base row whose id sits at gt place 70
(k > 70: dGt = 0 in the second round)."""
import numpy as np
import pytest

import gt_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    with pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=16), 0) as c:
        yield c


def _code(pkg, dt):
    N = pkg._native
    return dict(f32=N.F32, u8=N.U8, i8=N.I8, f16=N.F16, bf16=N.BF16, f8=N.F8E4M3)[dt]


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:                                 # (bfloat16 patterns: bytes are bytes)
        a = a.view(np.int16)
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def _run(pkg, ctx, entry, bdt, qdt, xd, qd, n, nq, d, k, ann, cnt, gt):
    """one call; ann [nq][ann_stride], gt [nq][gt_stride], cnt None: the count pointer is 0"""
    import torch
    dev = torch.device("cuda", 0)
    ad, gd = _dev(ann), _dev(gt)
    cd = None if cnt is None else _dev(cnt)
    rec = torch.full((nq,), -7.0, dtype=torch.float64, device=dev)
    rat = torch.full((nq,), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    cp = 0 if cd is None else cd.data_ptr()
    if entry == "f32":
        ctx.eval_metrics_dev(n, xd.data_ptr(), nq, qd.data_ptr(), d, k, ad.data_ptr(), ann.shape[1], cp, gd.data_ptr(), gt.shape[1], rec.data_ptr(), rat.data_ptr())
    else:
        ctx.eval_metrics_typed_dev(n, xd.data_ptr(), _code(pkg, bdt), nq, qd.data_ptr(), _code(pkg, qdt), d, k, ad.data_ptr(), ann.shape[1], cp,
                                   gd.data_ptr(), gt.shape[1], rec.data_ptr(), rat.data_ptr())
    ctx.sync()
    return rec.cpu().numpy(), rat.cpu().numpy()


def _bits_equal(got, want, what):
    print(what, "got", got.tolist(), "want", want.tolist())
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64)), what


def _check(pkg, ctx, oracle, entry, bdt, qdt, sc, strides):
    n, k, d = sc["n"], sc["k"], sc["d"]
    X64, Q64 = sc["X"].astype(np.float64), sc["Q"].astype(np.float64)
    xd, qd = _dev(sc["raw"]), _dev(sc["qraw"])
    nq = len(Q64)
    for ann_stride, gt_stride in strides:
        ann, cnt, gt = R.metrics_call(sc, ann_stride, gt_stride) if "gd2" in sc else (sc["ann"], sc["cnt"], sc["gt"])
        for counts in (cnt, None):
            want = R.metrics(X64, Q64, k, ann, counts, gt)
            second = oracle.metrics(sc["X"], sc["Q"], k, ann, counts, gt)
            got = _run(pkg, ctx, entry, bdt, qdt, xd, qd, n, nq, d, k, ann, counts, gt)
            what = "%s %s x %s d %d k %d ann_stride %d gt_stride %d counts %s: " % (entry, bdt, qdt, d, k, ann_stride, gt_stride, counts is not None)
            for j, name in enumerate(("recall", "ratio")):
                _bits_equal(got[j], want[j], what + name + " against gt_ref")
                _bits_equal(got[j], second[j], what + name + " against the oracle")


ENTRIES = [("f32", "f32", "f32")] + [("typed", b, q) for b, q in R.M_PAIRS]


@pytest.mark.parametrize("d,k", R.M_SHAPES)
@pytest.mark.parametrize("entry,bdt,qdt", ENTRIES)
def test_metrics_at_every_k(pkg, oracle, ctx, entry, bdt, qdt, d, k):
    sc = R.metrics_scene(bdt, qdt, d, k)
    strides = [(k, k + 7), (k + 5, k + 7)] + ([(k, k), (k + 5, k)] if k <= 128 else [])
    _check(pkg, ctx, oracle, entry, bdt, qdt, sc, strides)


@pytest.mark.parametrize("entry", ("f32", "typed"))
def test_metrics_tiny_case(pkg, oracle, ctx, entry):
    """n = 5, k = 5, d = 1: k = n = both strides"""
    sc = dict(R.tiny_scene())
    sc["raw"], sc["qraw"] = sc["X"], sc["Q"]
    _check(pkg, ctx, oracle, entry, "f32", "f32", sc, [(5, 5)])
