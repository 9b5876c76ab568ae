"""The front launch's encode role (front_kernel, tick.hip.h): with FSPANN_FRONT_ENCODE unset it is the MFMA role
(encode_mfma_block, encode.hip.h), with FSPANN_FRONT_ENCODE=exact the exact fp64 role.  The code words and NaN / Inf flags the
front launch writes must equal, bit for bit, those of the exact role and of the oracle (idx/Coding.java:250-301)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
B = 64


def _ctx(pkg, T, m, lam, d, X, gfun, exact):
    cfg = pkg.PaperRuntimeConfig(tables=T, divisions=1, m=m, lambda_=lam, dim=d, refinement_limit=B)
    old = os.environ.get("FSPANN_FRONT_ENCODE")
    os.environ["FSPANN_FRONT_ENCODE"] = "exact" if exact else "mfma"     # read once, when the context is made
    try:
        ctx = pkg.FspannContext(cfg, 0)
    finally:
        if old is None:
            del os.environ["FSPANN_FRONT_ENCODE"]
        else:
            os.environ["FSPANN_FRONT_ENCODE"] = old
    ctx.set_gfunctions(*gfun)
    ctx.set_id_meta(len(X))
    ctx.build_index(X)
    return ctx


def _front(ctx, Qh, T, W, mfma):
    """codes and bad flags of Qh as the encode part of one front launch (encode + Route, no Refine)"""
    import torch
    dev = torch.device("cuda", 0)
    nq, nr = len(Qh), 16
    q = torch.from_numpy(np.ascontiguousarray(Qh, dtype=np.float32)).to(dev)
    codes = torch.full((nq, T, W), -1, dtype=torch.int64, device=dev)
    bad = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    rcodes = torch.zeros((nr, T, W), dtype=torch.int64, device=dev)      # valid codes for the Route part (not looked at)
    sel = torch.zeros((nr, B), dtype=torch.int32, device=dev)
    cnt = torch.zeros(nr, dtype=torch.int32, device=dev)
    hov = torch.zeros(max(1, ctx.route_handover_bytes(nr)), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.tick_dev(encode=dict(nq=nq, q=q.data_ptr(), codes=codes.data_ptr(), bad=bad.data_ptr()),
                 route=dict(nq=nr, codes=rcodes.data_ptr(), limit=B, ids=sel.data_ptr(), count=cnt.data_ptr(), handover=hov.data_ptr()))
    ctx.sync()
    assert ctx.last_tick_fused()
    assert ctx.last_front_encode_mfma() == mfma, "the front launch did not take the encode role the context asked for"
    return codes.cpu().numpy().view(np.uint64), bad.cpu().numpy()     # (the oracle's code words are uint64)


def _check(pkg, oracle, T, m, lam, d, Q, gfun_edit=None, n=3000, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    W = (m * lam + 63) // 64
    gfun = oracle.registry_init(X[:1000].astype(np.float64), m, 13, T, 1)
    if gfun_edit:
        gfun = gfun_edit(*gfun)
    got = {}
    for exact in (False, True):
        with _ctx(pkg, T, m, lam, d, X, gfun, exact) as ctx:
            got[exact] = _front(ctx, Q, T, W, mfma=not exact)
    (cm, bm), (ce, be) = got[False], got[True]
    assert np.array_equal(cm, ce), "MFMA role differs from the exact role"
    assert np.array_equal(bm, be)
    Q64 = np.asarray(Q, dtype=np.float32).astype(np.float64)
    fin = np.isfinite(Q64).all(axis=1)
    assert np.array_equal(bm != 0, ~fin)
    o = oracle.Oracle(T, 1, m, lam, d, refinement_limit=B)
    o.set_gfunctions(*gfun)
    if fin.any():
        assert np.array_equal(cm[fin].reshape(int(fin.sum()), -1), o.encode(Q64[fin]).reshape(int(fin.sum()), -1)), "codes differ from the oracle"
    return cm


@pytest.mark.parametrize("nq", [1, 17, 1000])
def test_front_encode_config2_shape(pkg, oracle, nq):
    """BASELINE config #2's coding shape: 16 tables x m = 16, lambda = 2, d = 128 (P = 256, one code word)."""
    Q = np.random.default_rng(nq).standard_normal((nq, 128)).astype(np.float32)
    _check(pkg, oracle, 16, 16, 2, 128, Q)


@pytest.mark.parametrize("T,m,lam,d", [(8, 8, 3, 50), (7, 5, 3, 37), (3, 20, 4, 130)])
def test_front_encode_generic_shapes(pkg, oracle, T, m, lam, d):
    """Shapes that run the generic front_kernel build; d off the 16-wide k trip, P not a multiple of 4 or of 64, several words."""
    Q = np.random.default_rng(d).standard_normal((45, d)).astype(np.float32)
    _check(pkg, oracle, T, m, lam, d, Q)


def test_front_encode_bucket_boundaries(pkg, oracle):
    """Rows scaled so that (alpha.v + r) / omega lands within 1e-12 .. 3e-6 of an integer for one projection each."""
    T, m, lam, d, n = 16, 16, 2, 128, 3000
    rng = np.random.default_rng(99)
    X = rng.standard_normal((n, d)).astype(np.float32)
    alpha, r, w = oracle.registry_init(X[:1000].astype(np.float64), m, 13, T, 1)
    rows = []
    for _ in range(300):
        v = rng.standard_normal(d)
        p = rng.integers(0, T * m)
        a = alpha.reshape(-1, d)[p]
        y = float(np.dot(v, a))
        eps = rng.choice([0.0, 1e-12, -1e-12, 1e-9, -1e-9, 1e-7, -1e-7, 3e-6, -3e-6])
        target = (rng.integers(-3, 4) + eps) * w.reshape(-1)[p] - r.reshape(-1)[p]
        rows.append(v * (target / y) if abs(y) > 1e-3 else v)
    _check(pkg, oracle, T, m, lam, d, np.array(rows).astype(np.float32), n=n, seed=99)


def test_front_encode_nonfinite_rows(pkg, oracle):
    """Rows with NaN / Inf: flagged in `bad`, and their code words are what the exact role writes."""
    Q = np.random.default_rng(3).standard_normal((40, 128)).astype(np.float32)
    Q[1, 5] = np.nan
    Q[7, 0] = np.inf
    Q[16, 127] = -np.inf
    Q[33, :] = np.nan
    Q[39, 64] = np.nan
    _check(pkg, oracle, 16, 16, 2, 128, Q)


def test_front_encode_respects_exact_encode_mode(pkg, oracle):
    """fspann_set_encode_mode(1) (exact fp64 coding only) keeps the front launch on the exact role."""
    T, m, lam, d, n = 16, 16, 2, 128, 3000
    X = np.random.default_rng(1).standard_normal((n, d)).astype(np.float32)
    gfun = oracle.registry_init(X[:1000].astype(np.float64), m, 13, T, 1)
    Q = np.random.default_rng(4).standard_normal((33, d)).astype(np.float32)
    with _ctx(pkg, T, m, lam, d, X, gfun, exact=False) as ctx:
        c_m, _ = _front(ctx, Q, T, 1, mfma=True)
        ctx.set_encode_mode(1)
        c_e, _ = _front(ctx, Q, T, 1, mfma=False)
    assert np.array_equal(c_m, c_e)


def test_front_encode_degenerate_omega(pkg, oracle):
    """omega so small that every pair lies inside the guard band: the whole tile is re-checked with the exact chain."""
    Q = (np.random.default_rng(5).standard_normal((40, 128)) * 50).astype(np.float32)
    _check(pkg, oracle, 16, 16, 2, 128, Q, gfun_edit=lambda a, r, w: (a, r * 0 + 3e-7, np.full_like(w, 1e-6)))
