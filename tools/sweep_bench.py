"""Dev tool: one search at several refinement limits (fspann_search_sweep_dev) against the same limits searched one by one
(fspann_search_retry_dev per limit), and the sweep refine alone (fspann_refine_store_sweep_dev) against one
fspann_refine_store_dev at the largest limit.  Shape: the reference's shipped profile SIFT_P10_HIGH (1 M x 128, 7 x 8 tables,
m = 26, 10 probes, maxGlobalCandidates 28 000, 256 queries) on siftlike:16:6 data, limits {2 000, 4 000, 8 000, 16 000, 22 000},
k = 100.  Method of tools/retry_bench.py: whole calls back to back, no events in the loop, one synchronisation at the end; the two
sides alternate over three rounds and the best round counts.
  --lib PATH   load another build of libfspann_hip.so (the parent commit's, say); a build without the sweep calls times the
               separate calls and the single refine only
  --only refine | search   one half only (a profiler run over the refine half shows the prefix kernel's own time)
Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--only", default=None, choices=("refine", "search"))
ap.add_argument("--reps", type=int, default=int(os.environ.get("SWEEP_BENCH_REPS", "30")))
args = ap.parse_args()
pkg = g.load_package()
N = pkg._native
have_sweep = True
if args.lib:
    import ctypes
    N._SO = os.path.abspath(args.lib)
    probe = ctypes.CDLL(N._SO)
    have_sweep = hasattr(probe, "fspann_search_sweep_dev")
    if not have_sweep:
        N._SIGS_SWEEP.clear()

n, d, T, D, m, lam, probes, hard_cap, Q, K = 1000000, 128, 7, 8, 26, 2, 10, 28000, 256, 100
LIMITS = [2000, 4000, 8000, 16000, 22000]
BMAX, NL = LIMITS[-1], len(LIMITS)
REPS = args.reps


def siftlike(rng, r=16, noise=6.0):
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)
    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        return np.clip(np.rint(np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)), 0, 255).astype(np.float32)
    return draw


rng = np.random.default_rng(1)
draw = siftlike(rng)
X = draw(n)
ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=T, divisions=D, m=m, lambda_=lam, dim=d, refinement_limit=BMAX, max_global_candidates=hard_cap,
                                               probe_override=probes), 0)
ctx.registry_initialize(X[:1000].astype(np.float64)); ctx.set_id_meta(n); ctx.build_index(X); ctx.store_set(X)
dev = torch.device("cuda", 0)
F32 = N.F32
qs = [torch.from_numpy(draw(Q) + np.float32(0.25)).to(dev) for _ in range(6)]
oi = torch.zeros((NL, Q, K), dtype=torch.int32, device=dev); od = torch.zeros((NL, Q, K), dtype=torch.float64, device=dev)
oc, sc, un, ret = (torch.zeros((NL, Q), dtype=torch.int32, device=dev) for _ in range(4))
bad = torch.zeros(Q, dtype=torch.int32, device=dev)
sel = torch.full((Q, BMAX), -1, dtype=torch.int32, device=dev); selc = torch.zeros(Q, dtype=torch.int32, device=dev)


def plane(t, j):
    return t[j].data_ptr()


def separate(q):
    for j, B in enumerate(LIMITS):
        ctx.search_retry_dev(Q, q.data_ptr(), F32, -1, B, K, plane(oi, j), plane(od, j), plane(oc, j), plane(sc, j), 0, plane(un, j), bad.data_ptr(), plane(ret, j))


def sweep(q):
    ctx.search_sweep_dev(Q, q.data_ptr(), F32, -1, LIMITS, K, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), sc.data_ptr(), un.data_ptr(), bad.data_ptr(), ret.data_ptr())


def refine_one(q):
    ctx.refine_store_dev(Q, q.data_ptr(), F32, BMAX, sel.data_ptr(), selc.data_ptr(), K, plane(oi, NL - 1), plane(od, NL - 1), plane(oc, NL - 1), plane(sc, NL - 1))


def refine_sweep(q):
    ctx.refine_store_sweep_dev(Q, q.data_ptr(), F32, BMAX, sel.data_ptr(), selc.data_ptr(), LIMITS, K, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), sc.data_ptr())


def timed(fn):
    for i in range(5):
        fn(qs[i % len(qs)])
    ctx.sync()
    t0 = time.perf_counter()
    for i in range(REPS):
        fn(qs[i % len(qs)])
    ctx.sync()
    return 1e6 * (time.perf_counter() - t0) / REPS


def best(fns):
    res = [[] for _ in fns]
    for _ in range(3):
        for r, fn in zip(res, fns):
            r.append(timed(fn))
    return [round(min(r), 1) for r in res]


out = dict(lib=args.lib or "this build", have_sweep=have_sweep, shape=dict(n=n, d=d, T=T, D=D, m=m, probes=probes, hard_cap=hard_cap, nq=Q, k=K, limits=LIMITS),
           reps=REPS)
if args.only != "refine":
    separate(qs[0]); ctx.sync()
    out["retried_per_limit"] = ret.sum(1).tolist()
    out["mean_unique_per_limit"] = [round(float(x), 1) for x in un.to(torch.float64).mean(1).tolist()]
    if have_sweep:
        want = [t.clone() for t in (oi, od, oc, sc, un, ret)]
        for t in (oi, od, oc, sc, un, ret):
            t.zero_()
        sweep(qs[0]); ctx.sync()
        out["sweep_equals_separate"] = all(torch.equal(a, b) for a, b in zip(want, (oi, od, oc, sc, un, ret)))
        out["separate_us"], out["sweep_us"] = best([separate, sweep])
    else:
        out["separate_us"], = best([separate])
if args.only != "search":
    # candidate lists of one batch at the largest limit (the refine half reads the same lists for every batch of queries)
    ctx.search_store_dev(Q, qs[0].data_ptr(), F32, -1, BMAX, K, plane(oi, 0), plane(od, 0), plane(oc, 0), plane(sc, 0), sel.data_ptr(), selc.data_ptr())
    ctx.sync()
    out["mean_candidates"] = round(float(selc.to(torch.float64).mean().item()), 1)
    if have_sweep:
        out["refine_store_us"], out["refine_sweep_us"] = best([refine_one, refine_sweep])
    else:
        out["refine_store_us"], = best([refine_one])
print(json.dumps(out))
