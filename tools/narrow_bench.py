"""Dev tool: the fit and narrow passes of include/fspann_narrow.h over 1 M x 128 SIFT-like rows held as fp32 and as fp64, and the
store refine / search over the wide store beside the narrowed one.

  python tools/narrow_bench.py [--parts fit,narrow,store] [--n 1000000] [--tag NAME]

One process, device events on the context's stream around every call, 4 warm-up + 16 timed calls per reading, the median.
  fit     fspann_rows_fit_dev (no row mask) over rows where EVERYTHING fits (bytes 0..255) and over rows where NOTHING fits (the
          same rows + 0.3 as fp32, + 1e-9 as fp64), side by side: the second must not be slower than the first, or the first-misfit
          bookkeeping is wrong.  GB/s = source bytes over time, and that as a fraction of fspann_hbm_read_peak of the same run.
  narrow  fspann_rows_narrow_dev to FSPANN_U8; GB/s = source + destination bytes over time.
          Both calls synchronise, so a reading holds the two small memsets in front of the kernel and the result's copy behind it.
  store   fspann_refine_store_dev and fspann_search_store_dev at config #2's shape (1 024 x 256, k 10) over an fp32 store, an fp64
          store and the fp64 store after fspann_store_narrow (FSPANN_U8), alternated, two rounds.  The comparison is the wide
          store of the SAME run."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
N = pkg._native
DEV = torch.device("cuda", 0)
WARM, TIMED = 4, 16
D = 128


def timed(ctx, calls):
    stream = torch.cuda.ExternalStream(ctx.stream)
    for f in calls[:WARM]:
        f()
    ctx.sync()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls[WARM:]]
    for (e0, e1), f in zip(evs, calls[WARM:]):
        e0.record(stream)
        f()
        e1.record(stream)
    ctx.sync()
    return np.array([e0.elapsed_time(e1) for e0, e1 in evs]) * 1e3


def siftlike(rng, d, r=16, noise=6.0):
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)

    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        return np.clip(np.rint(np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)), 0, 255).astype(np.float32)
    return draw


def line(tag, what, ts, nbytes, peak):
    med = float(np.median(ts))
    gbs = nbytes / med / 1e3
    print(f"{tag} {what}: median {med:.1f} us  min {ts.min():.1f}  max {ts.max():.1f}  {gbs:.0f} GB/s  {gbs / peak:.2f} of hbm_read_peak {peak:.0f} GB/s", flush=True)
    return med


def bench_rows(tag, parts, n, X):
    ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=D, refinement_limit=64), 0)
    peak = ctx.hbm_read_peak()
    print(f"{tag} fspann_hbm_read_peak: {peak:.0f} GB/s", flush=True)
    base = torch.from_numpy(X).to(DEV)
    for name, tdt, code, bump in (("fp32", torch.float32, N.F32, 0.3), ("fp64", torch.float64, N.F64, 1e-9)):
        fits_all = base.to(tdt)
        fits_none = fits_all + bump
        dst = torch.empty((n, D), dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        src_bytes = n * D * fits_all.element_size()
        if "fit" in parts:
            meds = {}
            for rnd in range(2):
                for what, t in (("everything_fits", fits_all), ("nothing_fits", fits_none)):
                    f = ctx.rows_fit_dev(n, t.data_ptr(), code, D)
                    want = N.U8 if what == "everything_fits" else code
                    assert f.narrowest == want, (what, f.narrowest)
                    meds[what] = line(tag, f"fit {name} {what} round={rnd} n={n} dim={D} narrowest={f.narrowest} first_misfit[U8]={f.first_misfit[N.U8]}",
                                      timed(ctx, [lambda t=t: ctx.rows_fit_dev(n, t.data_ptr(), code, D)] * (WARM + TIMED)), src_bytes, peak)
                print(f"{tag} fit {name} round={rnd}: nothing_fits / everything_fits = {meds['nothing_fits'] / meds['everything_fits']:.2f}", flush=True)
        if "narrow" in parts:
            for rnd in range(2):
                line(tag, f"narrow {name}->u8 round={rnd} n={n} dim={D}",
                     timed(ctx, [lambda: ctx.rows_narrow_dev(n, fits_all.data_ptr(), code, D, dst.data_ptr(), N.U8)] * (WARM + TIMED)), src_bytes + n * D, peak)
            assert torch.equal(dst, base.to(torch.uint8))
        del fits_all, fits_none, dst
        torch.cuda.empty_cache()
    ctx.close()


def bench_store(tag, n, X, draw):
    nq, B, k = 1024, 256, 10                        # BASELINE config #2
    cfg = pkg.PaperRuntimeConfig(tables=16, divisions=1, m=16, lambda_=2, dim=D, refinement_limit=B, max_global_candidates=20000)
    ctxs = {}
    for rows in ("f32", "f64", "narrowed"):
        c = pkg.FspannContext(cfg, 0)
        c.registry_initialize(X[:1000].astype(np.float64))
        c.set_id_meta(n)
        c.build_index(X)
        c.store_set(X if rows == "f32" else X.astype(np.float64))
        if rows == "narrowed":
            kept = c.store_narrow()
            assert kept == np.uint8, kept
        ctxs[rows] = c
    qs = [torch.from_numpy(draw(nq) + np.float32(0.25)).to(DEV) for _ in range(6)]
    idsets = [torch.randint(0, n, (nq, B), device=DEV, dtype=torch.int32) for _ in range(6)]
    cnt = torch.full((nq,), B, dtype=torch.int32, device=DEV)
    oi = torch.zeros((nq, k), dtype=torch.int32, device=DEV)
    od = torch.zeros((nq, k), dtype=torch.float64, device=DEV)
    oc, sc = torch.zeros(nq, dtype=torch.int32, device=DEV), torch.zeros(nq, dtype=torch.int32, device=DEV)
    ref = {}
    for rnd in range(2):
        for rows, c in ctxs.items():
            ts = timed(c, [(lambda s=idsets[i % 6]: c.refine_store_dev(nq, qs[0].data_ptr(), N.F32, B, s.data_ptr(), cnt.data_ptr(), k, oi.data_ptr(), od.data_ptr(),
                                                                       oc.data_ptr(), sc.data_ptr())) for i in range(WARM + TIMED)])
            print(f"{tag} refine_store config2 store={rows} round={rnd} nq={nq} B={B} k={k}: median {np.median(ts):.1f} us  min {ts.min():.1f}  max {ts.max():.1f}", flush=True)
            ts = timed(c, [(lambda q=qs[i % 6]: c.search_store_dev(nq, q.data_ptr(), N.F32, -1, B, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), sc.data_ptr()))
                           for i in range(WARM + TIMED)])
            print(f"{tag} search_store config2 store={rows} round={rnd} nq={nq} B={B} k={k}: median {np.median(ts):.1f} us  min {ts.min():.1f}  max {ts.max():.1f}", flush=True)
            c.sync()
            res = (oi.cpu().numpy().copy(), od.cpu().numpy().copy())
            ref.setdefault("r", res)
            assert np.array_equal(ref["r"][0], res[0]) and np.array_equal(ref["r"][1], res[1]), "results differ between stores"
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="fit,narrow,store")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--tag", default="branch")
    a = ap.parse_args()
    parts = a.parts.split(",")
    print(f"# {a.tag}: lib {os.path.relpath(N._SO)}  n {a.n}  dim {D}  {WARM} warm-up + {TIMED} timed calls per reading", flush=True)
    draw = siftlike(np.random.default_rng(1), D)
    X = draw(a.n)
    if "fit" in parts or "narrow" in parts:
        bench_rows(a.tag, parts, a.n, X)
    if "store" in parts:
        bench_store(a.tag, a.n, X, draw)
