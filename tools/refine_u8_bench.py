"""Dev tool: the refinement scan over FSPANN_U8 rows beside the same scan over FSPANN_F32 rows, and fspann_search_store_dev end to
end over a U8 and an F32 store, at BASELINE config #2's shape and at the scan shapes of the reference's shipped profiles.

  python tools/refine_u8_bench.py [--rows f32,u8] [--parts dense,gather,search] [--tag NAME]
  AB_LIB=<path to another libfspann_hip.so> ... --rows f32        the same F32 readings with another build (the parent's)

Per reading: device events around every launch on the context's stream, 8 warm-up + 40 timed launches, the median; inputs are
rotated from launch to launch over more than 512 MB per dtype (dense blocks, id sets over a 5 M-row store), so neither dtype is
served from the 256 MiB Infinity Cache; F32 and U8 readings alternate in the same process (two rounds each).  The end-to-end
readings run over a 1 M x 128 store as a deployment holds it (U8: 128 MB, which the cache CAN hold — that is the point of it).
Each line: median us, algorithmic bytes (B d s + d 4 + k 8 per query, s = bytes per row element) over time, and the two lower
bounds: bytes / 6.3 TB/s and the scan's fp64-pipe instructions (5 per element for both row types, counted from the ISA of the
consume loop: two conversions, subtract, multiply, add) / 39e12 lane-instructions per second."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
if os.environ.get("AB_LIB"):
    pkg._native._SO = os.path.abspath(os.environ["AB_LIB"])   # a variant build
N = pkg._native
DEV = torch.device("cuda", 0)
WARM, TIMED = 8, 40
ROTATE_BYTES = 600 << 20
HBM, FP64_RATE, FP64_PER_ELEM = 6.3e12, 39e12, 5

SHAPES = {   # name: (nq, B, k)
    "config2": (1024, 256, 10),
    "SIFT_P4_FAST": (256, 8000, 100),
    "SIFT_P10_HIGH": (256, 22000, 100),
}
PROFILES = {  # for the end-to-end readings: T, D, m, probes, hard_cap
    "config2": dict(T=16, D=1, m=16, probes=-1, hard_cap=20000),
    "SIFT_P4_FAST": dict(T=5, D=8, m=20, probes=4, hard_cap=10000),
    "SIFT_P10_HIGH": dict(T=7, D=8, m=26, probes=10, hard_cap=28000),
}
D = 128


def timed(ctx, launches):
    """launches: a list of WARM + TIMED callables (already rotated); returns the TIMED durations in us."""
    stream = torch.cuda.ExternalStream(ctx.stream)
    for f in launches[:WARM]:
        f()
    ctx.sync()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in launches[WARM:]]
    for (e0, e1), f in zip(evs, launches[WARM:]):
        e0.record(stream)
        f()
        e1.record(stream)
    ctx.sync()
    return np.array([e0.elapsed_time(e1) for e0, e1 in evs]) * 1e3


def report(tag, part, shape, rows, rnd, ts, nq, B, k):
    es = 1 if rows == "u8" else 4
    byt = nq * (B * D * es + D * 4 + k * 8)
    med = float(np.median(ts))
    t_bytes, t_fp64 = byt / HBM * 1e6, nq * B * D * FP64_PER_ELEM / FP64_RATE * 1e6
    print(f"{tag} {part} {shape} rows={rows} round={rnd} nq={nq} B={B} k={k}: median {med:.1f} us  min {ts.min():.1f}  max {ts.max():.1f}  "
          f"{med * 1024 / nq:.1f} us/1024q  {byt / med / 1e6:.2f} TB/s algorithmic  bounds: bytes {t_bytes:.1f} us, fp64 {t_fp64:.1f} us "
          f"-> nearer to {'fp64' if t_fp64 > t_bytes else 'bytes'} ({med / max(t_bytes, t_fp64):.2f}x of it)", flush=True)


def outs(nq, k):
    return (torch.zeros((nq, k), dtype=torch.int32, device=DEV), torch.zeros((nq, k), dtype=torch.float64, device=DEV),
            torch.zeros(nq, dtype=torch.int32, device=DEV), torch.zeros(nq, dtype=torch.int32, device=DEV))


def bench_dense(tag, rows_list, shapes):
    for shape in shapes:
        nq, B, k = SHAPES[shape]
        ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=D, refinement_limit=B), 0)
        q = torch.randint(0, 256, (nq, D), device=DEV).to(torch.float32) + 0.25
        ids = torch.arange(nq * B, dtype=torch.int32, device=DEV).reshape(nq, B)
        cnt = torch.full((nq,), B, dtype=torch.int32, device=DEV)
        oi, od, oc, sc = outs(nq, k)
        bufs = {}
        for rows in rows_list:
            es = 1 if rows == "u8" else 4
            nb = max(2, -(-ROTATE_BYTES // (nq * B * D * es)) + 1)
            bufs[rows] = [torch.randint(0, 256, (nq, B, D), device=DEV, dtype=torch.uint8) if rows == "u8" else
                          torch.randint(0, 256, (nq, B, D), device=DEV, dtype=torch.uint8).to(torch.float32) for _ in range(nb)]
        torch.cuda.synchronize()
        for rnd in range(2):
            for rows in rows_list:
                cdt = N.U8 if rows == "u8" else N.F32
                bb = bufs[rows]
                launches = [(lambda b=bb[i % len(bb)]: ctx.refine_dev(nq, q.data_ptr(), N.F32, b.data_ptr(), cdt, B, ids.data_ptr(), cnt.data_ptr(), k,
                                                                      oi.data_ptr(), od.data_ptr(), oc.data_ptr(), sc.data_ptr())) for i in range(WARM + TIMED)]
                report(tag, "scan_dense", shape, rows, rnd, timed(ctx, launches), nq, B, k)
        ctx.close()
        del bufs
        torch.cuda.empty_cache()


def bench_gather(tag, rows_list, shapes):
    n = 5_000_000                                  # 640 MB of bytes, 2.56 GB of fp32: neither store fits the Infinity Cache
    base = torch.randint(0, 256, (n, D), device=DEV, dtype=torch.uint8)
    stores = {"u8": base}
    if "f32" in rows_list:
        stores["f32"] = base.to(torch.float32)
    torch.cuda.synchronize()
    for shape in shapes:
        nq, B, k = SHAPES[shape]
        ctxs = {}
        for rows in rows_list:
            c = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=D, refinement_limit=B), 0)
            c.store_attach_dev(n, stores[rows].data_ptr(), N.U8 if rows == "u8" else N.F32)
            ctxs[rows] = c
        q = torch.randint(0, 256, (nq, D), device=DEV).to(torch.float32) + 0.25
        nset = max(3, -(-ROTATE_BYTES // (nq * B * D)) + 1)
        idsets = [torch.randint(0, n, (nq, B), device=DEV, dtype=torch.int32) for _ in range(nset)]
        cnt = torch.full((nq,), B, dtype=torch.int32, device=DEV)
        oi, od, oc, sc = outs(nq, k)
        torch.cuda.synchronize()
        for rnd in range(2):
            for rows in rows_list:
                c = ctxs[rows]
                launches = [(lambda s=idsets[i % nset]: c.refine_store_dev(nq, q.data_ptr(), N.F32, B, s.data_ptr(), cnt.data_ptr(), k, oi.data_ptr(),
                                                                           od.data_ptr(), oc.data_ptr(), sc.data_ptr())) for i in range(WARM + TIMED)]
                report(tag, "scan_gather", shape, rows, rnd, timed(c, launches), nq, B, k)
        for c in ctxs.values():
            c.close()
    del stores, base
    torch.cuda.empty_cache()


def siftlike(rng, n, d, r=16, noise=6.0):
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)
    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        return np.clip(np.rint(np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)), 0, 255).astype(np.float32)
    return draw


def bench_search(tag, rows_list, shapes):
    n = 1_000_000
    rng = np.random.default_rng(1)
    draw = siftlike(rng, n, D)
    X = draw(n)
    X8 = X.astype(np.uint8)
    for shape in shapes:
        nq, B, k = SHAPES[shape]
        pr = PROFILES[shape]
        cfg = pkg.PaperRuntimeConfig(tables=pr["T"], divisions=pr["D"], m=pr["m"], lambda_=2, dim=D, refinement_limit=B,
                                     max_global_candidates=pr["hard_cap"], probe_override=pr["probes"])
        ctxs = {}
        for rows in rows_list:
            c = pkg.FspannContext(cfg, 0)
            c.registry_initialize(X[:1000].astype(np.float64))
            c.set_id_meta(n)
            c.build_index(X)
            if rows == "u8":
                c.store_set(X8, dtype=np.uint8)
            else:
                c.store_set(X)
            ctxs[rows] = c
        qs = [torch.from_numpy(draw(nq) + np.float32(0.25)).to(DEV) for _ in range(6)]
        oi, od, oc, sc = outs(nq, k)
        sel = torch.full((nq, B), -1, dtype=torch.int32, device=DEV)
        selc = torch.zeros(nq, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        for rnd in range(2):
            for rows in rows_list:
                c = ctxs[rows]
                launches = [(lambda qq=qs[i % len(qs)]: c.search_store_dev(nq, qq.data_ptr(), N.F32, -1, B, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                                                           sc.data_ptr(), sel.data_ptr(), selc.data_ptr())) for i in range(WARM + TIMED)]
                ts = timed(c, launches)
                scored = float(sc.to(torch.float64).mean().item())
                report(tag, "search_store", shape, rows, rnd, ts, nq, B, k)
                print(f"{tag} search_store {shape} rows={rows} round={rnd}: mean scored rows per query {scored:.0f} of B={B}", flush=True)
        for c in ctxs.values():
            c.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="f32,u8")
    ap.add_argument("--parts", default="dense,gather,search")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--tag", default="branch")
    a = ap.parse_args()
    rows_list, shapes = a.rows.split(","), a.shapes.split(",")
    print(f"# {a.tag}: lib {os.path.relpath(pkg._native._SO)}  rows {rows_list}  {WARM} warm-up + {TIMED} timed launches per reading", flush=True)
    for part in a.parts.split(","):
        dict(dense=bench_dense, gather=bench_gather, search=bench_search)[part](a.tag, rows_list, shapes)
