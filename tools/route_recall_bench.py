"""Dev tool: what recall attribution costs.  The rank call (fspann_gt_rank_dev) at 1 024 queries over Route's full lists, at two
shapes: the default step of bench.py (1 M x 128 gaussian, 16 x 1 tables, m = 16, default probes, K = 10) and the reference's shipped
profile SIFT_P10_HIGH (7 x 8 tables, m = 26, 10 probes, maxGlobalCandidates 28 000, K = 100, siftlike:16:6 data) — the lists are the
`kept` that data gives.  Per shape it prints
  * microseconds per rank call (whole calls back to back, one synchronisation at the end, best of three rounds) and the bytes of
    list read per second beside hbm_read_peak() of the same process; the ceiling call the same way;
  * route_recall next to limit_sweep at the same 16 limits, both with the ground truth handed in: the cost of predicting the
    recall-against-limit curve against the cost of measuring it (host wall clock around the whole numpy-level call).
  --shape default | p10 | both     --reps N
One JSON line per shape."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="both", choices=("default", "p10", "both"))
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--n", type=int, default=1_000_000)
args = ap.parse_args()
pkg = g.load_package()
N = pkg._native
dev = torch.device("cuda", 0)
NQ = 1024
SHAPES = dict(default=dict(d=128, T=16, D=1, m=16, B=256, K=10, probes=-1, hard_cap=20000, data="gaussian", bmax=4096),
              p10=dict(d=128, T=7, D=8, m=26, B=22000, K=100, probes=10, hard_cap=28000, data="siftlike", bmax=22000))


def make(kind, n, d, rng):
    if kind == "gaussian":
        return lambda cnt: rng.standard_normal((cnt, d), dtype=np.float32)
    U = (rng.standard_normal((16, d)) / np.sqrt(16)).astype(np.float32)

    def draw(cnt):
        y = rng.standard_normal((cnt, 16), dtype=np.float32) @ U
        return np.clip(np.rint(np.float32(64.0) + np.float32(48.0) * y + np.float32(6.0) * rng.standard_normal((cnt, d), dtype=np.float32)), 0, 255).astype(np.float32)
    return draw


def best(fn, sync, reps):
    res = []
    for _ in range(3):
        for _ in range(3):
            fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        res.append(1e6 * (time.perf_counter() - t0) / reps)
    return round(min(res), 1)


def run(name, s):
    rng = np.random.default_rng(1)
    draw = make(s["data"], args.n, s["d"], rng)
    X = draw(args.n)
    Q = draw(NQ)
    cfg = pkg.PaperRuntimeConfig(tables=s["T"], divisions=s["D"], m=s["m"], lambda_=2, dim=s["d"], refinement_limit=s["B"], max_global_candidates=s["hard_cap"],
                                 probe_override=s["probes"])
    with pkg.FspannContext(cfg, 0) as ctx:
        ctx.registry_initialize(X[:1000].astype(np.float64)); ctx.set_id_meta(args.n); ctx.build_index(X); ctx.store_set(X)
        K, cap = s["K"], max(1, ctx.route_max_candidates(-1))
        qd = torch.from_numpy(Q).to(dev)
        codes = torch.zeros((NQ, ctx.TD, ctx.W), dtype=torch.int64, device=dev)
        ids = torch.full((NQ, cap), -1, dtype=torch.int32, device=dev); score = torch.zeros((NQ, cap), dtype=torch.int32, device=dev)
        cnt, kept = (torch.zeros(NQ, dtype=torch.int32, device=dev) for _ in range(2))
        gt, rank, gsc = (torch.zeros((NQ, K), dtype=torch.int32, device=dev) for _ in range(3))
        ctx.encode_dev(NQ, qd.data_ptr(), N.F32, codes.data_ptr())
        rargs = (NQ, codes.data_ptr(), -1, N.INT32_MAX, cap, ids.data_ptr(), score.data_ptr(), cnt.data_ptr(), kept.data_ptr(), 0)
        ctx.route_dev(*rargs)
        resolved = ctx.route_resolve_dev(*rargs)
        ctx.groundtruth_store_dev(NQ, qd.data_ptr(), K, gt.data_ptr())
        ctx.sync()
        c = cnt.cpu().numpy().astype(np.int64)
        limits = sorted(set(int(x) for x in np.geomspace(16, s["bmax"], 16)))
        ks = sorted({1, 10, K})
        hits = torch.zeros((len(limits) + 1, len(ks), NQ), dtype=torch.int32, device=dev)
        ceil = torch.zeros((len(limits) + 1, len(ks), NQ), dtype=torch.float64, device=dev)

        def rank_call():
            ctx.gt_rank_dev(NQ, ids.data_ptr(), score.data_ptr(), cap, cnt.data_ptr(), gt.data_ptr(), K, K, rank.data_ptr(), gsc.data_ptr())

        def ceil_call():
            ctx.recall_ceiling_dev(NQ, rank.data_ptr(), K, ks, limits, hits.data_ptr(), ceil.data_ptr())
        rank_us, ceil_us = best(rank_call, ctx.sync, args.reps), best(ceil_call, ctx.sync, args.reps)
        list_bytes = int(c.clip(0).sum()) * 4
        peak = ctx.hbm_read_peak()
        gth = gt.cpu().numpy()
        whole = {}
        for label, fn in (("route_recall_us", lambda: ctx.route_recall(Q, ks, limits=limits, gt_ids=gth)),
                          ("limit_sweep_us", lambda: ctx.limit_sweep(Q, limits, ks, gt_ids=gth))):
            whole[label] = best(fn, ctx.sync, 3)
        rr = ctx.route_recall(Q, ks, limits=limits, gt_ids=gth)
        out = dict(shape=name, n=args.n, nq=NQ, K=K, cap=cap, kept_min=int(c.min()), kept_mean=round(float(c.mean()), 1), kept_max=int(c.max()), resolved=resolved,
                   list_megabytes=round(list_bytes / 1e6, 2), rank_call_us=rank_us, list_read_gb_per_s=round(list_bytes / rank_us / 1e3, 1),
                   hbm_read_peak_gb_per_s=round(peak, 1), ceiling_call_us=ceil_us, limits=limits, ks=ks, **whole,
                   route_ceiling=[round(float(x), 4) for x in rr["route_ceiling"].mean(1)],
                   ceiling_at_largest_limit=[round(float(x), 4) for x in rr["ceiling"][len(limits) - 1].mean(1)])
    print(json.dumps(out), flush=True)


for name in (("default", "p10") if args.shape == "both" else (args.shape,)):
    run(name, SHAPES[name])
