"""Dev tool: fspann_groundtruth_rows_dev per row type beside fspann_groundtruth_dev over the widened fp32 copy of the same data.

  python tools/gt_rows_bench.py [--n 1000000] [--d 128] [--nq 256] [--k 100] [--rows f32,u8,i8,f16,bf16,f8] [--rounds 3] [--tag NAME]

The method of tools/refine_f16_bench.py.  Per reading: device events around every call on the context's stream (a call is the
distance kernel and the select kernel, one chunk at the default shape: 256 x 1 M fp64 distances are 2 GB of the 8 GB scratch budget),
WARM warm-up + TIMED timed calls, the median; the row types alternate in one process, --rounds rounds each, and the spread of a
type's figure is the range of its round medians.  Every type holds the SAME values (integers 0..15, which all five hold exactly,
queries fp32 with fractional parts), so every type must return the fp32 call's ids and distances at the timed size too: the tool
checks that before it times anything and fails if they differ.
Bounds printed with each line: the distance kernel's fp64-pipe lane-instructions (per row element and query: subtract — two per
instruction where the compiler packs it —, v_cvt_f64_f32, v_mul_f64, v_add_f64 = 4) over 39e12 per second, and the bytes (the
distance matrix written once and read by the select's 13 passes, the base read once per 16 queries) over 6.3 TB/s.  A byte base of 1 M x 128 (128 MB) fits
the 256 MiB Infinity Cache where the fp32 copy (512 MB) does not; the kernel is bound by the fp64 pipe either way."""
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
HBM, FP64_RATE = 6.3e12, 39e12
ES = {"f32": 4, "f16": 2, "bf16": 2, "f8": 1, "u8": 1, "i8": 1}
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f8": torch.float8_e4m3fn, "u8": torch.uint8, "i8": torch.int8}
CDT = {"f32": N.F32, "f16": N.F16, "bf16": N.BF16, "f8": N.F8E4M3, "u8": N.U8, "i8": N.I8}


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
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rows", default="f32,u8,i8,f16,bf16,f8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tag", default="branch")
    a = ap.parse_args()
    n, d, nq, k, rows_list = a.n, a.d, a.nq, a.k, a.rows.split(",")
    assert rows_list[0] == "f32", "the fp32 call is the reference of the others: name it first"
    print(f"# {a.tag}: lib {os.path.relpath(pkg._native._SO)}  n={n} d={d} nq={nq} k={k}  rows {rows_list}  {WARM} warm-up + {TIMED} timed calls per reading, "
          f"{a.rounds} rounds", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(1)
    X = torch.randint(0, 16, (n, d), device=DEV, generator=gen, dtype=torch.int32).to(torch.float32)
    q = torch.randint(0, 16, (nq, d), device=DEV, generator=gen, dtype=torch.int32).to(torch.float32) + torch.rand((nq, d), device=DEV, generator=gen)
    bases = {}
    for r in rows_list:              # every type holds the values exactly (fp8: torch's cast, there and back, on the CPU)
        host = r == "f8"
        src = X.cpu() if host else X
        t = src.to(TDT[r])
        assert torch.equal(t.to(torch.float32), src), r
        bases[r] = t.to(DEV).contiguous()
    del X
    ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d), 0)
    outs = {r: (torch.zeros((nq, k), dtype=torch.int32, device=DEV), torch.zeros((nq, k), dtype=torch.float64, device=DEV)) for r in rows_list}
    torch.cuda.synchronize()

    def call(r):
        oi, od = outs[r]
        if r == "f32":
            ctx.groundtruth_dev(n, bases[r].data_ptr(), nq, q.data_ptr(), d, k, oi.data_ptr(), od.data_ptr())
        else:
            ctx.groundtruth_rows_dev(n, bases[r].data_ptr(), CDT[r], nq, q.data_ptr(), d, k, oi.data_ptr(), od.data_ptr())

    for r in rows_list:
        call(r)
    ctx.sync()
    for r in rows_list[1:]:
        same = torch.equal(outs[r][0], outs["f32"][0]) and torch.equal(outs[r][1], outs["f32"][1])
        print(f"{a.tag} rows={r}: ids and distances equal the fp32 call's at n={n} nq={nq}: {same}", flush=True)
        assert same, r
    t_fp64 = n * d * nq * 4 / FP64_RATE * 1e3
    meds = {r: [] for r in rows_list}
    for rnd in range(a.rounds):
        for r in rows_list:
            ts = timed(ctx, lambda r=r: call(r))
            med = float(np.median(ts))
            meds[r].append(med)
            t_bytes = (14 * nq * n * 8 + (nq + 15) // 16 * n * d * ES[r]) / HBM * 1e3
            print(f"{a.tag} groundtruth rows={r} round={rnd}: median {med:.2f} ms  min {ts.min():.2f}  max {ts.max():.2f}  "
                  f"{n * d * nq / med / 1e9:.2f} Telem/s  bounds: fp64 {t_fp64:.2f} ms, bytes {t_bytes:.2f} ms", flush=True)
    f = meds["f32"]
    print(f"{a.tag} summary f32: round medians {min(f):.2f}..{max(f):.2f} ms (spread {100 * (max(f) - min(f)) / np.median(f):.1f} %)", flush=True)
    for r in rows_list[1:]:
        m = meds[r]
        print(f"{a.tag} summary {r}: round medians {min(m):.2f}..{max(m):.2f} ms, median {np.median(m):.2f} ms = {np.median(m) / np.median(f):.3f} x f32", flush=True)
    ctx.close()
