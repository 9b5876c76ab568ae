"""GPU parity of FSPANN_U8 rows at full size, on SIFT-like byte data (integers 0..255).

config #2 (BASELINE: 1 M x 128, 16 tables x 32 bits, B = 256, k = 10, Q = 1 024): the product builds its index from the BYTES
(`build_index(X8)`: uploaded as bytes, widened on the device) and keeps them as its store; the oracle builds its own index from
the same values as float64.  All 16 tables are compared, then every one of the 1 024 queries goes through
`fspann_search_store_dev` (+ `_finish_dev`) and must equal `oracle.search` — F_q, top-k ids, fp64 distances, counts, scored —
as tests/test_gpu_fullsize.py asks of fp32 rows.  SIFT_P10_HIGH (the reference's shipped profile with the longest candidate
lists: B = 22 000 = 86 chunks per query, k = 100) at n = 200 000, nq = 48, the same way."""
import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.fullsize]


def siftlike(rng, n, d, r=16, noise=6.0):
    """bench.py's SIFT-like generator (integers 0..255 of intrinsic dimension r), as tests/test_gpu_shipped_profiles.py has it."""
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)
    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        return np.clip(np.rint(np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)), 0, 255).astype(np.float32)
    return draw


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


def _parity(pkg, oracle, n, nq, T, D, m, B, K, probes=-1, hard_cap=20000, tables=None, seed=1):
    d, lam = 128, 2
    rng = np.random.default_rng(seed)
    draw = siftlike(rng, n, d)
    X8 = draw(n).astype(np.uint8)
    Q = draw(nq) + np.float32(0.25)                                    # a query is not byte data
    X64 = X8.astype(np.float64)
    alpha, r, w = oracle.registry_init(X64[:1000], m, 13, T, D)
    o = oracle.Oracle(T, D, m, lam, d, max_global_candidates=hard_cap, refinement_limit=B, probe_override=probes)
    o.set_gfunctions(alpha, r, w)
    o.set_id_meta(n)
    o.set_store(X64)
    o.build_index(X64)                                                 # the oracle's own index (NOT imported from the GPU)
    assert not o.unmodelled
    del X64
    cfg = pkg.PaperRuntimeConfig(tables=T, divisions=D, m=m, lambda_=lam, dim=d, refinement_limit=B, max_global_candidates=hard_cap,
                                 probe_override=probes)
    with pkg.FspannContext(cfg, 0) as ctx:
        ctx.set_gfunctions(alpha, r, w)
        ctx.set_id_meta(n)
        ctx.build_index(X8)                                            # Setup from bytes
        for td in (range(T * D) if tables is None else tables):
            a, b = ctx.get_index(td), o.get_index(td)
            assert all(np.array_equal(a[k], b[k]) for k in b), td
        ctx.store_set(X8, dtype=np.uint8)
        ref = o.search(Q.astype(np.float64), K)
        assert not o.unmodelled and not ref["metrics"][:, 4].any()     # B >= 10 K: the adaptive retry does not trigger
        res = _search(pkg, ctx, Q, B, K)
        info = ctx.last_route_info()
        assert ctx.unmodelled_queries() == 0
        assert np.array_equal(res["sel_count"], ref["sel_count"])
        assert np.array_equal(res["sel"], ref["sel"][:, :B])
        assert np.array_equal(res["ids"], ref["ids"]), np.flatnonzero((res["ids"] != ref["ids"]).any(1))[:8]
        assert np.array_equal(res["dist"], ref["dist"])
        assert np.array_equal(res["count"], ref["count"]) and np.array_equal(res["scored"], ref["metrics"][:, 2])
    return info, ref


def test_config2_full_size_from_bytes(pkg, oracle):
    """BASELINE config #2 exactly, on bytes: N = 1 M x 128, T*D = 16, m = 16, lambda = 2, B = 256, Q = 1 024, k = 10."""
    info, _ = _parity(pkg, oracle, n=1_000_000, nq=1024, T=16, D=1, m=16, B=256, K=10)
    assert info["lazy"], "fspann_search_store_dev did not take the bounded select at the headline configuration"


def test_sift_p10_high_long_lists_from_bytes(pkg, oracle):
    """SIFT_P10_HIGH (m 26, 7 x 8 tables, 10 probes, refinementLimit 22 000, maxGlobalCandidates 28 000), k = 100: the chunked
    scan over 86 chunks per query + merge, rows gathered from the U8 store."""
    info, ref = _parity(pkg, oracle, n=200_000, nq=48, T=7, D=8, m=26, B=22000, K=100, probes=10, hard_cap=28000, tables=(0, 7, 55), seed=11)
    assert ref["sel_count"].min() > 22000 // 4                         # the profile's operating range: long lists
