"""Dev tool: what the Route coverage map costs.  The reach call (fspann_gt_reach_dev) at 1 024 queries beside ONE full-list Route
(fspann_route_dev, limit = INT32_MAX, score and kept requested) at the same probes on the same context — the cost of one point of the
(tables, divisions, probes) cube the old way — at two shapes: the default step of bench.py (1 M x 128 gaussian, 16 x 1 tables,
m = 16, default probes, K = 10) and the reference's shipped profile SIFT_P10_HIGH (7 x 8 tables, m = 26, 10 probes,
maxGlobalCandidates 28 000, K = 100, siftlike:16:6 data).  Per shape it prints
  * microseconds per reach call and per Route (whole calls back to back, one synchronisation at the end, best of three rounds), and
    the id bytes the reach call reads per second — the ids of the partitions the probe lists name, T * D * P * S * 4 per query —
    beside hbm_read_peak() of the same process;
  * microseconds per coverage call over the full cube in groups of 64 configurations, and of the numpy-level route_coverage with the
    ground truth handed in (host wall clock around the whole call).
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
SHAPES = dict(default=dict(d=128, T=16, D=1, m=16, B=256, K=10, probes=-1, hard_cap=20000, data="gaussian"),
              p10=dict(d=128, T=7, D=8, m=26, B=22000, K=100, probes=10, hard_cap=28000, data="siftlike"))


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
        K, P, S, TD = s["K"], ctx.effective_probes(-1), cfg.block_size, ctx.TD
        cap = max(1, ctx.route_max_candidates(-1))
        qd = torch.from_numpy(Q).to(dev)
        codes = torch.zeros((NQ, TD, ctx.W), dtype=torch.int64, device=dev)
        ids = torch.full((NQ, cap), -1, dtype=torch.int32, device=dev); score = torch.zeros((NQ, cap), dtype=torch.int32, device=dev)
        cnt, kept = (torch.zeros(NQ, dtype=torch.int32, device=dev) for _ in range(2))
        gt = torch.zeros((NQ, K), dtype=torch.int32, device=dev)
        reach = torch.zeros((NQ, K, TD), dtype=torch.int32, device=dev)
        ctx.encode_dev(NQ, qd.data_ptr(), N.F32, codes.data_ptr())
        ctx.groundtruth_store_dev(NQ, qd.data_ptr(), K, gt.data_ptr())
        rargs = (NQ, codes.data_ptr(), -1, N.INT32_MAX, cap, ids.data_ptr(), score.data_ptr(), cnt.data_ptr(), kept.data_ptr(), 0)
        ctx.sync()

        def reach_call():
            ctx.gt_reach_dev(NQ, codes.data_ptr(), P, gt.data_ptr(), K, K, reach.data_ptr())

        def route_call():
            ctx.route_dev(*rargs)
        grid = pkg.coverage_grid(range(1, s["T"] + 1), range(1, s["D"] + 1), range(1, P + 1))
        ks = sorted({1, 10, K})
        groups = [grid[i:i + 64] for i in range(0, len(grid), 64)]
        hits = torch.zeros((64, len(ks), NQ), dtype=torch.int32, device=dev)
        ceil = torch.zeros((64, len(ks), NQ), dtype=torch.float64, device=dev)
        sco = torch.zeros((64, NQ, K), dtype=torch.int32, device=dev)

        def cover_call():
            for part in groups:
                ctx.route_coverage_dev(NQ, reach.data_ptr(), K, P, ks, part, hits.data_ptr(), ceil.data_ptr(), sco.data_ptr())
        reach_us, route_us, cover_us = best(reach_call, ctx.sync, args.reps), best(route_call, ctx.sync, args.reps), best(cover_call, ctx.sync, args.reps)
        # the ids the reach call reads are those Route's staging reads: the partitions the probe lists name, P blocks of S ids per
        # table (a table's one short tail partition aside)
        resolved = ctx.route_resolve_dev(*rargs)
        ctx.sync()
        id_bytes = NQ * TD * P * S * 4
        peak = ctx.hbm_read_peak()
        gth = gt.cpu().numpy()
        whole_us = best(lambda: ctx.route_coverage(Q, ks, grid, gt_ids=gth), ctx.sync, 3)
        rc = ctx.route_coverage(Q, ks, grid, gt_ids=gth)
        full = len(grid) - 1                           # the index's own tables and divisions at P probes
        out = dict(shape=name, n=args.n, nq=NQ, K=K, tables=s["T"], divisions=s["D"], probes=P, block_size=S, configs=len(grid), resolved=resolved,
                   id_megabytes=round(id_bytes / 1e6, 2), id_bytes_per_query=TD * P * S * 4, reach_call_us=reach_us, route_full_list_us=route_us,
                   reach_over_route=round(reach_us / route_us, 3), id_read_gb_per_s=round(id_bytes / reach_us / 1e3, 1), hbm_read_peak_gb_per_s=round(peak, 1),
                   coverage_cube_us=cover_us, coverage_launches=len(groups), route_coverage_us=whole_us, exact_configs=int(rc["exact"].sum()),
                   ceiling_full=[round(float(x), 4) for x in rc["ceiling"][full].mean(1)],
                   ceiling_half_tables=[round(float(x), 4) for x in rc["ceiling"][int(np.flatnonzero((rc["grid"] == (max(1, s["T"] // 2), s["D"], P)).all(1))[0])].mean(1)],
                   ceiling_one_probe=[round(float(x), 4) for x in rc["ceiling"][int(np.flatnonzero((rc["grid"] == (s["T"], s["D"], 1)).all(1))[0])].mean(1)], ks=ks)
    print(json.dumps(out), flush=True)


for name in (("default", "p10") if args.shape == "both" else (args.shape,)):
    run(name, SHAPES[name])
