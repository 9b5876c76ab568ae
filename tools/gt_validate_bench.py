"""Dev tool: fspann_nn1_exact_dev (the validator's exact top-1, one fused kernel) beside the nearest thing the library had for the
same job: the ground truth at k = 1 over the same queries (fspann_groundtruth_dev for fp32 rows, fspann_groundtruth_rows_dev for
U8 rows: a [Q x N] fp64 matrix in scratch and a 12-pass radix select).  The arithmetic differs (double against float subtraction);
the work is the same.

  python tools/gt_validate_bench.py [--n 1000000] [--d 128] [--nq 10000] [--sample 100] [--rows f32,u8] [--rounds 3] [--out FILE]

SIFT-like rows (integers 0..255, which both types hold), fp32 queries with fractional parts in sixteenths, the validator's own sample of the
queries (fspann_gt_validator_sample) gathered into a dense [sample][d] block for the ground-truth call, passed as the selection
list to the new one.  Per reading: device events around WARM warm-up + TIMED timed calls on the context's stream, the median; the
two calls alternate inside every round, --rounds rounds, and a call's figure is the BEST round median.  Before anything is timed the
tool checks the new call against the ground-truth call: on this data the two arithmetics agree (an integer below 256 from a multiple
of 1/16 below 257 is exact in float), so indices and distance bits must be equal, and the tool fails if they are not.
Bound printed with each line: fp64 lane-instructions of the distance loop (new call: subtract, multiply, add = 3 per row element
and query; ground truth: those plus a v_cvt_f64_f32 = 4) over 39e12 per second."""
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
FP64_RATE = 39e12
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
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--rows", default="f32,u8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, d, nq, rows_list = a.n, a.d, a.nq, a.rows.split(",")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d), 0)
    sel_host = ctx.gt_validator_sample(nq, a.sample)
    ns = len(sel_host)
    say(f"# gt_validate_bench: lib {os.path.relpath(pkg._native._SO)}  n={n} d={d} nq={nq} sample={ns}  rows {rows_list}  "
        f"{WARM} warm-up + {TIMED} timed calls per reading, {a.rounds} alternated rounds, best round median")
    gen = torch.Generator(device=DEV).manual_seed(1)
    # SIFT-like: a low-rank part plus noise, clipped and rounded to 0..255
    U = torch.randn((16, d), device=DEV, generator=gen) / 4.0
    X = (64.0 + 48.0 * (torch.randn((n, 16), device=DEV, generator=gen) @ U) + 6.0 * torch.randn((n, d), device=DEV, generator=gen)).clamp_(0, 255).round_()
    q = (64.0 + 48.0 * (torch.randn((nq, 16), device=DEV, generator=gen) @ U) + 6.0 * torch.randn((nq, d), device=DEV, generator=gen)).clamp_(0, 255).round_()
    q = (q + torch.randint(1, 16, (nq, d), device=DEV, generator=gen).to(torch.float32) / 16.0).to(torch.float32).contiguous()      # fractions of 1/16
    sel = torch.from_numpy(np.array(sel_host)).to(DEV)
    qs = q[sel].contiguous()                     # the ground-truth calls take their queries dense
    bases = {r: X.to(TDT[r]).contiguous() for r in rows_list}
    del X
    new_out = (torch.zeros(ns, dtype=torch.int32, device=DEV), torch.zeros(ns, dtype=torch.float64, device=DEV))
    old_out = (torch.zeros((ns, 1), dtype=torch.int32, device=DEV), torch.zeros((ns, 1), dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()

    def new_call(r):
        ctx.nn1_exact_dev(n, bases[r].data_ptr(), CDT[r], nq, q.data_ptr(), N.F32, d, sel.data_ptr(), ns, new_out[0].data_ptr(), new_out[1].data_ptr())

    def old_call(r):
        if r == "f32":
            ctx.groundtruth_dev(n, bases[r].data_ptr(), ns, qs.data_ptr(), d, 1, old_out[0].data_ptr(), old_out[1].data_ptr())
        else:
            ctx.groundtruth_rows_dev(n, bases[r].data_ptr(), CDT[r], ns, qs.data_ptr(), d, 1, old_out[0].data_ptr(), old_out[1].data_ptr())

    for r in rows_list:
        new_call(r)
        old_call(r)
        ctx.sync()
        same = torch.equal(new_out[0], old_out[0][:, 0]) and torch.equal(new_out[1], old_out[1][:, 0])
        say(f"rows={r}: exact top-1 equals the k = 1 ground truth (indices and distance bits) on this data: {same}")
        assert same, r
    t3, t4 = n * d * ns * 3 / FP64_RATE * 1e3, n * d * ns * 4 / FP64_RATE * 1e3
    best = {}
    for rnd in range(a.rounds):
        for r in rows_list:
            for name, call, bound in (("nn1_exact", new_call, t3), ("groundtruth_k1", old_call, t4)):
                ts = timed(ctx, lambda r=r, call=call: call(r))
                med = float(np.median(ts))
                best[(r, name)] = min(best.get((r, name), np.inf), med)
                say(f"rows={r} {name} round={rnd}: median {med:.3f} ms  min {ts.min():.3f}  max {ts.max():.3f}  fp64 bound {bound:.3f} ms")
    for r in rows_list:
        a_, b_ = best[(r, "nn1_exact")], best[(r, "groundtruth_k1")]
        say(f"summary rows={r}: nn1_exact {a_:.3f} ms, groundtruth at k = 1 {b_:.3f} ms, ratio {a_ / b_:.3f}")
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
