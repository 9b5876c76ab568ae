"""GPU: the native pipeline with QueryServiceImpl's adaptive retry switched on (fspann_pipeline_set_retry) equals oracle.search
batch by batch — deleted and tampered records included — and with the retry off it is what it was: the pass alone."""
import numpy as np
import pytest

from conftest import make_scene

pytestmark = pytest.mark.gpu

K = 10


def _setup(oracle, gone_n=4000):
    sc = make_scene(oracle, n=20000, d=16, T=2, D=2, m=10, lam=2, B=128, seed=31, probe_override=2)
    o, rng = sc["oracle"], sc["rng"]
    valid = np.ones(20000, np.uint8)
    gone = rng.choice(20000, gone_n, replace=False)
    valid[gone] = 0
    o.set_store(sc["X64"], valid)                                    # loadPointIfActive() == null / decrypt failure for those
    batches = [rng.standard_normal((nq, 16)).astype(np.float32) for nq in (200, 128, 7, 200, 200, 33)]
    return sc, gone, batches


def _ctx(pkg, sc):
    p = sc["params"]
    cfg = pkg.PaperRuntimeConfig(tables=p["T"], divisions=p["D"], m=p["m"], lambda_=p["lam"], dim=p["d"], refinement_limit=p["B"],
                                 probe_override=p["probe_override"])
    ctx = pkg.FspannContext(cfg, 0)
    ctx.set_gfunctions(sc["alpha"], sc["r"], sc["omega"])
    ctx.set_id_meta(p["n"])
    ctx.build_index(sc["X"])
    return ctx


def _store(hostpipe, sc, gone):
    ps = hostpipe.PointStore(sc["params"]["n"], 16)
    ps.encrypt(sc["X"], threads=8)
    half = len(gone) // 2
    for h in gone[:half]:
        ps.delete(int(h))                                            # no record
    for h in gone[half:]:
        ver, iv, ct = ps.get_record(int(h))
        ps.put_record(int(h), ver, iv, ct[:-1] + bytes([ct[-1] ^ 0x80]))   # tag mismatch
    return ps


def _run(pl, batches):
    out = []
    for qb in batches:                       # keep the pipeline full: submit ahead, collect in order
        pl.submit(qb)
        if pl.in_flight == 4:
            out.append(pl.collect())
    while pl.in_flight:
        out.append(pl.collect())
    assert [o["ticket"] for o in out] == sorted(o["ticket"] for o in out)
    return out


def test_pipeline_retry_matches_oracle_search(pkg, oracle):
    from fspann_amd import hostpipe
    sc, gone, batches = _setup(oracle)
    o = sc["oracle"]
    refs = [o.search(qb.astype(np.float64), K) for qb in batches]
    nret = sum(int(r["metrics"][:, 4].sum()) for r in refs)
    assert 0 < nret < sum(len(b) for b in batches)
    with _ctx(pkg, sc) as ctx, _store(hostpipe, sc, gone) as ps:
        with hostpipe.Pipeline(ctx, ps, 200, sc["params"]["B"], K, host_threads=8, retry=True) as pl:
            out = _run(pl, batches)
            st = pl.stats()
        with hostpipe.Pipeline(ctx, ps, 200, sc["params"]["B"], K, host_threads=8) as pl:
            off = _run(pl, batches)
            st_off = pl.stats()
    assert st["retried"] == nret and st["batches"] == len(batches) and st["retry_ms"] > 0
    assert st_off["retried"] == 0 and st_off["retry_ms"] == 0
    for res, ref in zip(out, refs):
        assert np.array_equal(res["count"], ref["count"])
        assert np.array_equal(res["ids"], ref["ids"]) and np.array_equal(res["dist"], ref["dist"])
    # retry off (the default): the pass alone — oracle.search on every query the oracle does not retry, a different answer somewhere
    differs = False
    for res, ref, qb in zip(off, refs, batches):
        keep = ref["metrics"][:, 4] == 0
        assert np.array_equal(res["ids"][keep], ref["ids"][keep]) and np.array_equal(res["count"][keep], ref["count"][keep])
        differs = differs or not np.array_equal(res["ids"], ref["ids"])
    assert differs


def test_pipeline_retry_toggle_refused_in_flight(pkg, oracle):
    from fspann_amd import hostpipe
    sc, gone, batches = _setup(oracle, gone_n=100)
    with _ctx(pkg, sc) as ctx, _store(hostpipe, sc, gone) as ps:
        with hostpipe.Pipeline(ctx, ps, 200, sc["params"]["B"], K, host_threads=4) as pl:
            pl.submit(batches[0])
            with pytest.raises(pkg.FspannStateError, match="in flight"):
                pl.set_retry(True)
            pl.collect()
            pl.set_retry(True)                                       # idle again: allowed
            pl.submit(batches[1])
            with pytest.raises(pkg.FspannStateError, match="in flight"):
                pl.set_retry(False)
            res = pl.collect()
            pl.set_retry(False)
    ref = sc["oracle"].search(batches[1].astype(np.float64), K)
    assert np.array_equal(res["ids"], ref["ids"]) and np.array_equal(res["count"], ref["count"])
