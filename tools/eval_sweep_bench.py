"""Dev tool: one fspann_eval_kvariants_dev call beside the fspann_eval_metrics_typed_dev calls it replaces (one per k).

  python tools/eval_sweep_bench.py [--n 1000000] [--d 128] [--nq 10000] [--ks 1,10,20,40,60,80,100] [--rows f32,u8] [--rounds 3] [--tag NAME]

The method of tools/gt_rows_bench.py.  Per reading: device events around the call(s) on the context's stream, WARM warm-up + TIMED
timed repetitions, the median; the two sides alternate in one process, --rounds rounds each, and the spread of a side's figure is the
range of its round medians.  ann = gt = random ids (every place scores: the most distance work the metrics can have); the tool
first checks that recall and ratio of the one call equal the per-k calls' bit for bit and fails if they do not.  The yardstick is the
per-k side: no ratio is expected, only that computing each distance once is not slower beyond the yardstick's own spread."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
N = pkg._native
DEV = torch.device("cuda", 0)
WARM, TIMED = 3, 12
TDT = {"f32": torch.float32, "u8": torch.uint8}
CDT = {"f32": N.F32, "u8": N.U8}


def timed(ctx, call):
    stream = torch.cuda.ExternalStream(ctx.stream)
    for _ in range(WARM):
        call()
    ctx.sync()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(TIMED)]
    for e0, e1 in evs:
        e0.record(stream)
        call()
        e1.record(stream)
    ctx.sync()
    return np.array([e0.elapsed_time(e1) for e0, e1 in evs])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--ks", default="1,10,20,40,60,80,100")
    ap.add_argument("--rows", default="f32,u8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tag", default="branch")
    a = ap.parse_args()
    n, d, nq, rows_list = a.n, a.d, a.nq, a.rows.split(",")
    ks = [int(x) for x in a.ks.split(",")]
    nk, kmax = len(ks), max(ks)
    print(f"# {a.tag}: lib {os.path.relpath(pkg._native._SO)}  n={n} d={d} nq={nq} ks={ks}  rows {rows_list}  {WARM} warm-up + {TIMED} timed per reading, "
          f"{a.rounds} rounds", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(1)
    X = torch.randint(0, 256, (n, d), device=DEV, generator=gen, dtype=torch.int32)
    bases = {r: X.to(TDT[r]).contiguous() for r in rows_list}
    del X
    q = (torch.randint(0, 256, (nq, d), device=DEV, generator=gen, dtype=torch.int32).to(torch.float32) + torch.rand((nq, d), device=DEV, generator=gen)).contiguous()
    ids = torch.randint(0, n, (nq, kmax), device=DEV, generator=gen, dtype=torch.int32).contiguous()       # ann = gt
    ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d), 0)
    one = torch.zeros((2, nk, nq), dtype=torch.float64, device=DEV)
    per = torch.zeros((2, nk, nq), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()

    def sweep(r):
        ctx.eval_kvariants_dev(n, bases[r].data_ptr(), CDT[r], nq, q.data_ptr(), N.F32, d, ks, ids.data_ptr(), kmax, 0, ids.data_ptr(), kmax, 0,
                               one[0].data_ptr(), one[1].data_ptr(), 0)

    def per_k(r):
        for j, k in enumerate(ks):
            ctx.eval_metrics_typed_dev(n, bases[r].data_ptr(), CDT[r], nq, q.data_ptr(), N.F32, d, k, ids.data_ptr(), kmax, 0, ids.data_ptr(), kmax,
                                       per[0, j].data_ptr(), per[1, j].data_ptr())

    for r in rows_list:
        one.fill_(-7.0)
        per.fill_(-7.0)
        sweep(r)
        per_k(r)
        ctx.sync()
        same = torch.equal(one.view(torch.int64), per.view(torch.int64))
        print(f"{a.tag} rows={r}: recall and ratio of the one call equal the {nk} per-k calls' bits at nq={nq}: {same}", flush=True)
        assert same, r
    meds = {(r, s): [] for r in rows_list for s in ("sweep", "per_k")}
    for rnd in range(a.rounds):
        for r in rows_list:
            for s, fn in (("per_k", per_k), ("sweep", sweep)):
                ts = timed(ctx, lambda r=r, fn=fn: fn(r))
                meds[(r, s)].append(float(np.median(ts)))
                print(f"{a.tag} rows={r} {s} round={rnd}: median {np.median(ts):.3f} ms  min {ts.min():.3f}  max {ts.max():.3f}", flush=True)
    for r in rows_list:
        p, s = meds[(r, "per_k")], meds[(r, "sweep")]
        print(f"{a.tag} summary rows={r}: {nk} per-k calls {min(p):.3f}..{max(p):.3f} ms (spread {100 * (max(p) - min(p)) / np.median(p):.1f} %), "
              f"one call {min(s):.3f}..{max(s):.3f} ms, median {np.median(s):.3f} ms = {np.median(s) / np.median(p):.3f} x the per-k calls", flush=True)
    ctx.close()
