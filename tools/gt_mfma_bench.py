"""Dev tool: fspann_groundtruth_mfma_dev and fspann_groundtruth_mfma16_dev beside fspann_groundtruth_rows_dev over the same base, per
row type.

  python tools/gt_mfma_bench.py [--n 1000000] [--d 128] [--nq 1024] [--k 100] [--rows f32,f16,u8] [--methods exact,mfma,mfma16] [--rounds 3]
                                [--exact-lib PATH] [--tag NAME]

The method of tools/gt_rows_bench.py.  Per reading: device events around every whole call on its context's stream, WARM warm-up +
TIMED timed calls, the median; the methods and the row types alternate in one process (mfma16 is left out for f32 rows), --rounds rounds each, and the spread of a
figure is the range of its round medians.  --exact-lib: another build of libfspann_hip.so (the parent commit's) whose
fspann_groundtruth_rows_dev is the exact reading, on a context of its own; without it this build's call is.  Rows are Gaussian
(integers 128 + 32 g for u8, 32 g for i8), queries fp32 from the same distribution.  Before anything is timed every method runs at the
timed size and must return the exact call's arrays; the pre-filtered calls' stats are printed.
--once: that comparison only, one call each (what a kernel trace is taken of)."""
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
WARM, TIMED = 2, 7
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f8": torch.float8_e4m3fn, "u8": torch.uint8, "i8": torch.int8}
CDT = {"f32": N.F32, "f16": N.F16, "bf16": N.BF16, "f8": N.F8E4M3, "u8": N.U8, "i8": N.I8}


class ExactLib:
    """fspann_groundtruth_rows_dev of another build of the library, on a context of its own"""

    def __init__(self, path, cfg):
        self.L = L = C.CDLL(path)
        L.fspann_ctx_create.argtypes, L.fspann_ctx_create.restype = [C.c_int, C.POINTER(N.Cfg), C.POINTER(C.c_void_p)], C.c_int
        L.fspann_ctx_stream.argtypes, L.fspann_ctx_stream.restype = [C.c_void_p], C.c_void_p
        L.fspann_sync.argtypes, L.fspann_ctx_destroy.argtypes, L.fspann_ctx_destroy.restype = [C.c_void_p], [C.c_void_p], None
        L.fspann_groundtruth_rows_dev.argtypes = N._SIGS_ROWS["fspann_groundtruth_rows_dev"][1]
        self.h = C.c_void_p()
        assert L.fspann_ctx_create(0, C.byref(cfg.to_c()), C.byref(self.h)) == 0
        self.stream = int(L.fspann_ctx_stream(self.h) or 0)

    def sync(self):
        assert self.L.fspann_sync(self.h) == 0

    def groundtruth_rows_dev(self, *args):
        assert self.L.fspann_groundtruth_rows_dev(self.h, *args) == 0

    def close(self):
        self.L.fspann_ctx_destroy(self.h)


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
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rows", default="f32,f16,u8")
    ap.add_argument("--methods", default="exact,mfma")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--exact-lib", default=None)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--tag", default="branch")
    a = ap.parse_args()
    n, d, nq, k, rows_list = a.n, a.d, a.nq, a.k, a.rows.split(",")
    fast = [m for m in a.methods.split(",") if m != "exact"]
    assert set(fast) <= {"mfma", "mfma16"}, a.methods
    methods = lambda r: ["exact"] + [m for m in fast if not (m == "mfma16" and r == "f32")]
    print(f"# {a.tag}: lib {os.path.relpath(N._SO)}  exact call of {a.exact_lib or 'the same library'}  n={n} d={d} nq={nq} k={k}  rows {rows_list}  "
          f"{WARM} warm-up + {TIMED} timed calls per reading, {a.rounds} rounds", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(1)
    G = torch.randn((n, d), device=DEV, generator=gen)
    Gq = torch.randn((nq, d), device=DEV, generator=gen)
    scale = lambda r, t: 128 + 32 * t if r == "u8" else 32 * t if r == "i8" else t
    bases, qs = {}, {}
    for r in rows_list:
        v = scale(r, G)
        v = v.round().clamp(0, 255) if r == "u8" else v.round().clamp(-128, 127) if r == "i8" else v
        bases[r] = (v.cpu().to(TDT[r]).to(DEV) if r == "f8" else v.to(TDT[r])).contiguous()
        qs[r] = scale(r, Gq).contiguous()
    del G
    cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d)
    ctx = pkg.FspannContext(cfg, 0)
    ex = ExactLib(a.exact_lib, cfg) if a.exact_lib else ctx
    out = {m: (torch.zeros((nq, k), dtype=torch.int32, device=DEV), torch.zeros((nq, k), dtype=torch.float64, device=DEV)) for m in ("exact", "mfma", "mfma16")}
    torch.cuda.synchronize()

    def call(m, r):
        oi, od = out[m]
        f = ex.groundtruth_rows_dev if m == "exact" else getattr(ctx, f"groundtruth_{m}_dev")
        f(n, bases[r].data_ptr(), CDT[r], nq, qs[r].data_ptr(), d, k, oi.data_ptr(), od.data_ptr())

    for r in rows_list:
        call("exact", r)
        ex.sync()
        for m in methods(r)[1:]:
            call(m, r)
            ctx.sync()
            same = torch.equal(out["exact"][0], out[m][0]) and torch.equal(out["exact"][1], out[m][1])
            print(f"{a.tag} rows={r}: ids and distances of exact and {m} equal at n={n} nq={nq}: {same}  stats {ctx.last_gt_stats}", flush=True)
            assert same, (r, m)
    meds = {(m, r): [] for r in rows_list for m in methods(r)}
    for rnd in range(0 if a.once else a.rounds):
        for r in rows_list:
            for m in methods(r):
                ts = timed(ex if m == "exact" else ctx, lambda: call(m, r))
                meds[m, r].append(float(np.median(ts)))
                print(f"{a.tag} groundtruth {m} rows={r} round={rnd}: median {meds[m, r][-1]:.2f} ms  min {ts.min():.2f}  max {ts.max():.2f}", flush=True)
    for r in rows_list if not a.once else []:
        e = meds["exact", r]
        for m in methods(r)[1:]:
            f = meds[m, r]
            print(f"{a.tag} summary {r}: exact round medians {min(e):.2f}..{max(e):.2f} ms, {m} {min(f):.2f}..{max(f):.2f} ms, "
                  f"exact / {m} = {np.median(e) / np.median(f):.1f}", flush=True)
    if ex is not ctx:
        ex.close()
    ctx.close()
