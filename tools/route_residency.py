"""Debug tool (FSPANN_BUILD_DEBUG=1 build): residency census of the bounded select — how many Route workgroups one CU holds at once.

Every workgroup stamps where it runs (XCC_ID and HW_ID, dbg_hw_where in route_lazy.hip.h) and when it starts and ends
(wall_clock64).  Per CU the intervals are swept in time order: the peak is the most Route workgroups resident on one CU at one
moment, the mean is the time-weighted number while the CU holds at least one.  This is what the hardware admitted, whatever the
compiler's occupancy remark says.

  front  (default): the front launches of the bench's default step (BASELINE config #2 shape: 1 M x 128, 16 tables, B = 256,
         1 024 queries, three contexts, front_kernel = encode + Route) back to back on three streams.  The scan is left out: a
         debug build cannot launch it (its stamp arrays take the static LDS the scan's 159 KB request leaves), and it changes
         nothing about how many Route workgroups fit.  The stamps of the last --record front launches of every context are kept.
  lazy:  route_select_lazy_kernel alone (the serial path) over --queries queries, enough for a grid of 8 workgroups per CU.

AB_LIB=<path of a debug libfspann_hip.so> runs another build (the parent's, for a before/after census)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("mode", nargs="?", default="front", choices=["front", "lazy"])
ap.add_argument("--contexts", type=int, default=3)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--record", type=int, default=4, help="front launches per context whose stamps are kept")
ap.add_argument("--queries", type=int, default=4096, help="lazy mode: queries of the one route launch")
ap.add_argument("--json", default=None, help="write the summary here as well")
args = ap.parse_args()

pkg = g.load_package()
if os.environ.get("AB_LIB"):
    pkg._native._SO = os.path.abspath(os.environ["AB_LIB"])
L = pkg._native.lib()
if not hasattr(L, "fspann_debug_route_stamps"):
    sys.exit("route_residency.py needs a FSPANN_BUILD_DEBUG=1 build")
L.fspann_debug_route_stamps.argtypes = [C.c_void_p, C.c_void_p]
L.fspann_debug_route_stamps.restype = C.c_int
dev = torch.device("cuda", 0)

n, d, T, m, lam, B, Q = 1_000_000, 128, 16, 16, 2, 256, 1024
rng = np.random.default_rng(1)
X = rng.standard_normal((n, d), dtype=np.float32)
cfg = pkg.PaperRuntimeConfig(tables=T, divisions=1, m=m, lambda_=lam, dim=d, seed=13, refinement_limit=B, max_global_candidates=20000)   # bench.py's
ctx = pkg.FspannContext(cfg, 0)
ctx.registry_initialize(X[:1000].astype(np.float64))
ctx.set_id_meta(n)
ctx.build_index(X)
ctx.store_set(X)


def where_key(w):
    """one CU of the chip: XCC, then HW_ID[15:8] (shader engine, shader array, CU)"""
    w = w.astype(np.int64)
    return ((w >> 32) & 0xF) * 256 + ((w >> 8) & 0xFF)


def census(key, t0, t1):
    peaks, means = [], []
    for cu in np.unique(key):
        sel = key == cu
        ev = np.concatenate([np.stack([t0[sel], np.ones(sel.sum())], 1), np.stack([t1[sel], -np.ones(sel.sum())], 1)])
        ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]            # at equal times the end comes first: no false overlap
        level = np.cumsum(ev[:, 1])
        peaks.append(int(level.max()))
        dt = np.diff(ev[:, 0])
        busy = dt[level[:-1] > 0]
        means.append(float((level[:-1][level[:-1] > 0] * busy).sum() / max(busy.sum(), 1)))
    peaks = np.array(peaks)
    return dict(cus=int(len(peaks)), peak=int(peaks.max()), peak_p50=float(np.median(peaks)),
                cus_at_peak=int((peaks == peaks.max()).sum()), peak_hist={int(v): int((peaks == v).sum()) for v in np.unique(peaks)},
                mean_while_busy=round(float(np.mean(means)), 2), workgroups=int(len(key)))


if args.mode == "lazy":
    Qn = args.queries
    Qh = np.random.default_rng(2).standard_normal((Qn, d), dtype=np.float32)
    codes = torch.from_numpy(ctx.encode(Qh).view(np.int64)).to(dev)
    sel = torch.zeros((Qn, B), dtype=torch.int32, device=dev)
    cnt = torch.zeros(Qn, dtype=torch.int32, device=dev)
    dbg = torch.zeros((2 * Qn, 16), dtype=torch.int64, device=dev)   # rows [grid, 2 grid): the probe's stamps
    for _ in range(3):
        ctx.route_dev(Qn, codes.data_ptr(), -1, B, B, sel.data_ptr(), 0, cnt.data_ptr(), 0, 0)
    ctx.sync()
    L.fspann_debug_route_stamps(ctx.handle, dbg.data_ptr())
    ctx.route_dev(Qn, codes.data_ptr(), -1, B, B, sel.data_ptr(), 0, cnt.data_ptr(), 0, 0)
    ctx.sync()
    L.fspann_debug_route_stamps(ctx.handle, None)
    s = dbg[:Qn].cpu().numpy()
    s = s[(s[:, 0] > 0) & (s[:, 9] != 0)]                   # workgroup rows only (the grid's; rows past it hold probe stamps)
    # one query per workgroup or more: stamps 0 / 7 bracket the FIRST query of a workgroup, so the census is a lower bound
    res = census(where_key(s[:, 9]), s[:, 0].astype(np.float64), s[:, 7].astype(np.float64))
    res.update(mode="lazy", grid=int(len(s)), route_info=ctx.last_route_info())
else:
    # one bounded select on the root first: it uploads the index incl. the bucket-sorted id lists, which clones copy when made
    c0 = torch.from_numpy(ctx.encode(np.random.default_rng(3).standard_normal((Q, d), dtype=np.float32)).view(np.int64)).to(dev)
    s0, n0 = torch.zeros((Q, B), dtype=torch.int32, device=dev), torch.zeros(Q, dtype=torch.int32, device=dev)
    ctx.route_dev(Q, c0.data_ptr(), -1, B, B, s0.data_ptr(), 0, n0.data_ptr(), 0, 0)
    ctx.sync()
    ctxs = [ctx] + [ctx.clone() for _ in range(args.contexts - 1)]
    NB = 2 * args.contexts
    Qs = torch.from_numpy(np.random.default_rng(2).standard_normal((NB, Q, d), dtype=np.float32)).to(dev)
    hov_bytes = max(1, ctx.route_handover_bytes(Q))
    bufs = [dict(codes=[torch.zeros((Q, T, 1), dtype=torch.int64, device=dev) for _ in range(2)], bad=torch.zeros(Q, dtype=torch.int32, device=dev),
                 sel=torch.full((Q, B), -1, dtype=torch.int32, device=dev), cnt=torch.zeros(Q, dtype=torch.int32, device=dev),
                 hov=torch.zeros(hov_bytes, dtype=torch.uint8, device=dev)) for _ in ctxs]
    GMAX = 8 * Q                                            # rows per stamp buffer: far above encode + route workgroups of one launch
    stamps = [[torch.zeros((GMAX, 4), dtype=torch.int64, device=dev) for _ in range(args.record)] for _ in ctxs]
    # (the first front launch of a context routes all-zero codes: valid codes, and the census does not look at results)
    total = args.warmup + args.record
    for j in range(total):
        for i, cx in enumerate(ctxs):
            b = bufs[i]
            rec = j - args.warmup
            L.fspann_debug_route_stamps(cx.handle, stamps[i][rec].data_ptr() if rec >= 0 else None)
            cx.tick_dev(encode=dict(nq=Q, q=Qs[((j + 1) * len(ctxs) + i) % NB].data_ptr(), codes=b["codes"][(j + 1) & 1].data_ptr(), bad=b["bad"].data_ptr()),
                        route=dict(nq=Q, codes=b["codes"][j & 1].data_ptr(), limit=B, ids=b["sel"].data_ptr(), count=b["cnt"].data_ptr(),
                                   handover=b["hov"].data_ptr()))
    for cx in ctxs:
        cx.sync()
    rows = np.concatenate([st.cpu().numpy() for per in stamps for st in per])
    rows = rows[rows[:, 2] > 0]
    route = rows[rows[:, 0] == 1]
    res = census(where_key(route[:, 1]), route[:, 2].astype(np.float64), route[:, 3].astype(np.float64))
    res.update(mode="front", launches=args.record * len(ctxs), contexts=len(ctxs),
               all_roles=census(where_key(rows[:, 1]), rows[:, 2].astype(np.float64), rows[:, 3].astype(np.float64)))
    # slot-time of the two roles per front launch (sum of workgroup durations) and how long the encode workgroups run beside Route
    us = 0.01                                               # wall_clock64: 100 MHz
    per = []
    for st in (s_ for per_ctx in stamps for s_ in per_ctx):
        r_ = st.cpu().numpy()
        r_ = r_[r_[:, 2] > 0]
        enc, rt = r_[r_[:, 0] == 0], r_[r_[:, 0] == 1]
        if len(enc) == 0 or len(rt) == 0:
            continue
        e0, e1, r0, r1 = enc[:, 2].min(), enc[:, 3].max(), rt[:, 2].min(), rt[:, 3].max()
        per.append(dict(encode_wgs=len(enc), encode_slot_us=float((enc[:, 3] - enc[:, 2]).sum()) * us,
                        encode_wg_mean_us=float((enc[:, 3] - enc[:, 2]).mean()) * us, route_slot_us=float((rt[:, 3] - rt[:, 2]).sum()) * us,
                        encode_span_us=float(e1 - e0) * us, launch_span_us=float(max(e1, r1) - min(e0, r0)) * us,
                        encode_route_overlap_us=float(max(0, min(e1, r1) - max(e0, r0))) * us))
    if per:
        res["per_launch_mean"] = {k: round(float(np.mean([x[k] for x in per])), 2) for k in per[0]}
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
