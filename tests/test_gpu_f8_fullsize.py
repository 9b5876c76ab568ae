"""GPU parity of FSPANN_F8E4M3 rows at full size, at the sizes of tests/test_gpu_bf16_fullsize.py.  Rows are float32 draws rounded to
OCP fp8 e4m3fn once by the caller (torch's cast on the CPU); the oracle gets those values widened to float64 by this file's own
256-entry table (built from the format's definition, not from library code); every comparison is bit for bit.

config #4's routing and refine shape (BASELINE: 768-dimensional rows, 32 tables x 64-bit codes, B = 1 024, k = 10) at N = 1 M,
where the oracle still finishes (as tests/test_gpu_fullsize.py::test_config4_shape_at_1m_against_the_oracle has it for fp32 rows):
the product builds its index from the BIT PATTERNS (`build_index(Xb, dtype=float8_e4m3fn)`: uploaded as bytes, widened on the
device) and keeps them as its
store; the oracle builds its own index.  Tables 0, 16 and 31 are compared, then every query goes through
`fspann_search_store_dev` (+ `_finish_dev`) and must equal `oracle.search` — F_q, top-k ids, fp64 distances, counts, scored.

A RedCaps-like long list (the reference's RedCaps profile: 512-dimensional CLIP embeddings, B = 28 000, k = 100): 64 queries over
a dense [64][28 000][512] fp8 block (110 chunks per query: runs of chunks with the running top-k), against the oracle's Refine."""
import os

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.fullsize]


def e4m3_table():
    """value of each of the 256 patterns, from the definition: E = 0: +-M/8 * 2^-6; E = 1..15: +-(1 + M/8) * 2^(E-7); 0x7F / 0xFF NaN"""
    t = np.empty(256, np.float64)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        v = float("nan") if (e == 15 and m == 7) else (m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if s else v
    return t


TABLE = e4m3_table()


def f8_cast(a):
    """the caller's rounding: float32 values -> e4m3 bytes, torch's cast on the CPU; no value of these tests is near 448"""
    import torch
    b = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    assert ((b & 0x7F) != 0x7F).all()
    return b


def widen64(b):
    return TABLE[b]


def _search(pkg, ctx, Q, B, K):
    import torch
    dev = torch.device("cuda", 0)
    nq = len(Q)
    qd = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).to(dev)
    oi = torch.full((nq, K), -7, dtype=torch.int32, device=dev)
    od = torch.zeros((nq, K), dtype=torch.float64, device=dev)
    oc = torch.zeros(nq, dtype=torch.int32, device=dev)
    scn = torch.zeros(nq, dtype=torch.int32, device=dev)
    sel = torch.full((nq, B), -1, dtype=torch.int32, device=dev)
    selc = torch.zeros(nq, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    args = (nq, qd.data_ptr(), pkg._native.F32, -1, B, K, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), scn.data_ptr(), sel.data_ptr(), selc.data_ptr())
    ctx.search_store_dev(*args)
    ctx.search_store_finish_dev(*args)          # (finishes queries whose map treeified a bin: the host model)
    ctx.sync()
    c = selc.cpu().numpy()
    return dict(ids=oi.cpu().numpy(), dist=od.cpu().numpy(), count=oc.cpu().numpy(), scored=scn.cpu().numpy(),
                sel=np.where(np.arange(B)[None] < c[:, None], sel.cpu().numpy(), -1), sel_count=c)


def test_config4_shape_at_1m_from_f8(pkg, oracle):
    n = int(os.environ.get("FSPANN_TEST_CFG4S_N", "1000000"))
    d, T, D, m, lam, B, K, nq = 768, 32, 1, 32, 2, 1024, 10, 256
    rng = np.random.default_rng(4)
    Xb = f8_cast(rng.standard_normal((n, d), dtype=np.float32) * np.float32(16))   # the one rounding: N(0, 16^2), far below 448
    Q = rng.standard_normal((nq, d), dtype=np.float32) * np.float32(16)            # a query is not an fp8
    X64 = widen64(Xb)
    alpha, r, w = oracle.registry_init(X64[:1000], m, 13, T, D)
    o = oracle.Oracle(T, D, m, lam, d, refinement_limit=B)
    o.set_gfunctions(alpha, r, w)
    o.set_id_meta(n)
    o.set_store(X64)
    o.build_index(X64)                                                             # the oracle's own index (NOT imported from the GPU)
    assert not o.unmodelled, "a HashMap bin treeified in the oracle: iteration order not pinned at this size"
    del X64
    cfg = pkg.PaperRuntimeConfig(tables=T, divisions=D, m=m, lambda_=lam, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as ctx:
        ctx.set_gfunctions(alpha, r, w)
        ctx.set_id_meta(n)
        ctx.build_index(Xb, dtype=pkg.float8_e4m3fn)                               # Setup from fp8 bit patterns
        for td in (0, T // 2, T - 1):
            a, b = ctx.get_index(td), o.get_index(td)
            assert all(np.array_equal(a[k], b[k]) for k in b), td
        ctx.store_set(Xb, dtype=pkg.float8_e4m3fn)
        assert ctx.store_dtype is pkg.float8_e4m3fn
        ref = o.search(Q.astype(np.float64), K)
        assert not o.unmodelled and not ref["metrics"][:, 4].any()                 # B >= 10 K: the adaptive retry does not trigger
        res = _search(pkg, ctx, Q, B, K)
        info = ctx.last_route_info()
        assert ctx.unmodelled_queries() == 0
        assert np.array_equal(res["sel_count"], ref["sel_count"])
        assert np.array_equal(res["sel"], ref["sel"][:, :B])
        assert np.array_equal(res["ids"], ref["ids"]), np.flatnonzero((res["ids"] != ref["ids"]).any(1))[:8]
        assert np.array_equal(res["dist"].view(np.uint64), ref["dist"].view(np.uint64))
        assert np.array_equal(res["count"], ref["count"]) and np.array_equal(res["scored"], ref["metrics"][:, 2])
    assert info["lazy"], "fspann_search_store_dev did not take the bounded select at config #4's shape"


def test_redcaps_like_long_list_dense_f8(pkg, oracle):
    import torch
    dev = torch.device("cuda", 0)
    N = pkg._native
    d, B, K, nq, n = 512, 28000, 100, 64, 200_000
    rng = np.random.default_rng(12)
    # CLIP-like: unit-norm rows (elements of a few hundredths: e4m3 normals and subnormals), duplicates so that equal distances are
    # ordered by position
    raw = rng.standard_normal((n, d), dtype=np.float32)
    raw /= np.linalg.norm(raw, axis=1, keepdims=True)
    raw[n // 2:] = raw[rng.integers(0, 1000, n - n // 2)]
    Xb = f8_cast(raw)                                                              # the one rounding
    del raw
    Q = rng.standard_normal((nq, d), dtype=np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    ids = rng.integers(0, n, (nq, B)).astype(np.int32)
    count = rng.integers(B // 2, B + 1, nq).astype(np.int32)
    count[:3] = (B, B - 1, B // 2)
    cand8 = Xb[ids]                                                               # [64][28 000][512] bit patterns
    ei, ed, ec = np.empty((nq, K), np.int32), np.empty((nq, K), np.float64), np.empty(nq, np.int32)
    for s in range(0, nq, 8):                                                      # the oracle's Refine, 8 queries (0.9 GB of float64) at a time
        e = s + 8
        ei[s:e], ed[s:e], ec[s:e] = oracle.refine(Q[s:e].astype(np.float64), widen64(cand8[s:e]), ids[s:e], count[s:e], K)
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B)
    with pkg.FspannContext(cfg, 0) as ctx:
        cd = torch.from_numpy(cand8).to(dev).view(torch.float8_e4m3fn)
        assert cd.element_size() == 1
        qd, idd, cntd = torch.from_numpy(Q).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(count).to(dev)
        oi = torch.full((nq, K), -7, dtype=torch.int32, device=dev)
        od = torch.zeros((nq, K), dtype=torch.float64, device=dev)
        oc = torch.zeros(nq, dtype=torch.int32, device=dev)
        scn = torch.zeros(nq, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.refine_dev(nq, qd.data_ptr(), N.F32, cd.data_ptr(), N.F8E4M3, B, idd.data_ptr(), cntd.data_ptr(), K, oi.data_ptr(), od.data_ptr(),
                       oc.data_ptr(), scn.data_ptr())
        ctx.sync()
        gi, gd, gc, gs = oi.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy(), scn.cpu().numpy()
        del cd
    assert np.array_equal(gi, ei), np.flatnonzero((gi != ei).any(1))[:8]
    assert np.array_equal(gd.view(np.uint64), ed.view(np.uint64))
    assert np.array_equal(gc, ec) and (gc == K).all()
    assert np.array_equal(gs, count)
