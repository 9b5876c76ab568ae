"""Dev tool: the refinement scan over FSPANN_F16 (and, with --rows f32,f16,bf16 / f32,f16,f8, FSPANN_BF16 / FSPANN_F8E4M3) rows beside the same scan over
FSPANN_F32 rows, and fspann_search_store_dev end to end over an F16 (BF16) and an F32 store, at the shapes whose rows are float
embeddings: BASELINE config #2, config #4's shard, config #3's shard and a RedCaps-like long list (the reference's
REDCAPS_LAMBDA3 profile: B = 28 000 over 512-dimensional rows).

  python tools/refine_f16_bench.py [--rows f32,f16[,bf16][,f8] | f32,u8,i8] [--parts dense,gather,search] [--shapes ...] [--tag NAME]
  AB_LIB=<path to another libfspann_hip.so> ... --rows f32        the same F32 readings with another build (the parent's)

The method of tools/refine_u8_bench.py.  Per reading: device events around every launch on the context's stream, 8 warm-up + 40
timed launches, the median; inputs are rotated from launch to launch over more than 512 MB per dtype (dense blocks, id sets over
a 2 M-row store), so neither dtype is served from the 256 MiB Infinity Cache; F32 and F16 readings alternate in the same process
(two rounds each); the parent's and the branch's library alternate process by process (the caller's loop).  The end-to-end readings
run over a 500 000-row store.  Each line: median us, algorithmic bytes (B d s + d 4 + k 8 per query, s = bytes per row element)
over time, and the two lower bounds: bytes / 6.3 TB/s and the scan's fp64-pipe instructions per element (F32: two conversions,
subtract, multiply, add = 5; F16: one more conversion for the row element = 6; BF16: one integer operation for the row element
instead, which issues at the same rate = 6; F8E4M3: one v_cvt_pk_f32_fp8 per two row elements and a v_cvt_f64_f32 each = 5.5)
/ 39e12 lane-instructions per second.
bf16 / f8 rows hold the halves' values rounded once more to bfloat16 / fp8 e4m3fn (torch's rounding, the benchmark's own data:
timings do not depend on the values, and a standard normal stays far below 448, so no fp8 row turns NaN); without bf16 / f8 in
--rows every reading is taken exactly as before.
u8 / i8 rows (FSPANN_U8 / FSPANN_I8: a bit-field extract and an integer conversion per row element = 6, like F16) hold
round(40 x) clipped to -128..127 (u8: + 128); when --rows names either, the end-to-end part builds every index and store, F32
included, from those quantised values (u8: its own shifted copy, queries shifted too), so that every store routes the same lists."""
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
HBM, FP64_RATE = 6.3e12, 39e12
FP64_PER_ELEM = {"f32": 5, "f16": 6, "bf16": 6, "f8": 5.5, "u8": 6, "i8": 6}
ES = {"f32": 4, "f16": 2, "bf16": 2, "f8": 1, "u8": 1, "i8": 1}
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f8": torch.float8_e4m3fn, "u8": torch.uint8, "i8": torch.int8}
BYTE_SCALE = 40.0

SHAPES = {   # name: (nq, B, d, k)
    "config2": (1024, 256, 128, 10),
    "config4_shard": (1024, 1024, 768, 10),
    "config3_shard": (512, 512, 960, 10),
    "redcaps_like": (256, 28000, 512, 100),
}
PROFILES = {  # for the end-to-end readings: T, D, m, lambda, probes, hard_cap
    "config2": dict(T=16, D=1, m=16, lam=2, probes=-1, hard_cap=20000),
    "config4_shard": dict(T=32, D=1, m=32, lam=2, probes=-1, hard_cap=20000),
    "config3_shard": dict(T=16, D=1, m=16, lam=2, probes=-1, hard_cap=20000),
    "redcaps_like": dict(T=7, D=8, m=26, lam=3, probes=10, hard_cap=34000),
}


def cdt(rows):
    return N.F16 if rows == "f16" else N.BF16 if rows == "bf16" else N.F8E4M3 if rows == "f8" else N.U8 if rows == "u8" else N.I8 if rows == "i8" else N.F32


def as_rows(t, rows):
    """a device tensor of halves as rows of the given type (byte types: quantised, see the module text)"""
    if rows in ("u8", "i8"):
        v = (t.to(torch.float32) * BYTE_SCALE).round().clamp(-128, 127)
        return (v + 128).to(torch.uint8) if rows == "u8" else v.to(torch.int8)
    return t.to(TDT[rows])


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


def report(tag, part, shape, rows, rnd, ts, nq, B, d, k):
    byt = nq * (B * d * ES[rows] + d * 4 + k * 8)
    med = float(np.median(ts))
    t_bytes, t_fp64 = byt / HBM * 1e6, nq * B * d * FP64_PER_ELEM[rows] / FP64_RATE * 1e6
    print(f"{tag} {part} {shape} rows={rows} round={rnd} nq={nq} B={B} d={d} k={k}: median {med:.1f} us  min {ts.min():.1f}  max {ts.max():.1f}  "
          f"{med * 1024 / nq:.1f} us/1024q  {byt / med / 1e6:.2f} TB/s algorithmic  {nq * B * d / med / 1e6:.2f} Telem/s  "
          f"bounds: bytes {t_bytes:.1f} us, fp64 {t_fp64:.1f} us "
          f"-> nearer to {'fp64' if t_fp64 > t_bytes else 'bytes'} ({med / max(t_bytes, t_fp64):.2f}x of it)", flush=True)


def outs(nq, k):
    return (torch.zeros((nq, k), dtype=torch.int32, device=DEV), torch.zeros((nq, k), dtype=torch.float64, device=DEV),
            torch.zeros(nq, dtype=torch.int32, device=DEV), torch.zeros(nq, dtype=torch.int32, device=DEV))


def halves(shape):
    """random halves on the device (standard normal, rounded once) — the F32 copy holds the same values"""
    return torch.randn(shape, device=DEV, dtype=torch.float32).to(torch.float16)


def bench_dense(tag, rows_list, shapes):
    for shape in shapes:
        nq, B, d, k = SHAPES[shape]
        ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B), 0)
        q = torch.randn((nq, d), device=DEV, dtype=torch.float32)
        ids = torch.arange(nq * B, dtype=torch.int32, device=DEV).reshape(nq, B)
        cnt = torch.full((nq,), B, dtype=torch.int32, device=DEV)
        oi, od, oc, sc = outs(nq, k)
        bufs = {}
        for rows in rows_list:
            nb = max(2, -(-ROTATE_BYTES // (nq * B * d * ES[rows])) + 1)
            bufs[rows] = [as_rows(halves((nq, B, d)), rows) for _ in range(nb)]
        torch.cuda.synchronize()
        for rnd in range(2):
            for rows in rows_list:
                bb = bufs[rows]
                launches = [(lambda b=bb[i % len(bb)], r=rows: ctx.refine_dev(nq, q.data_ptr(), N.F32, b.data_ptr(), cdt(r), B, ids.data_ptr(), cnt.data_ptr(), k,
                                                                              oi.data_ptr(), od.data_ptr(), oc.data_ptr(), sc.data_ptr())) for i in range(WARM + TIMED)]
                report(tag, "scan_dense", shape, rows, rnd, timed(ctx, launches), nq, B, d, k)
        ctx.close()
        del bufs
        torch.cuda.empty_cache()


def bench_gather(tag, rows_list, shapes):
    n = 2_000_000                                  # d = 128: 512 MB of halves, 1 GB of fp32 — no store fits the Infinity Cache
    for shape in shapes:
        nq, B, d, k = SHAPES[shape]
        base = halves((n, d))
        stores = {r: as_rows(base, r) for r in rows_list}
        del base
        ctxs = {}
        for rows in rows_list:
            c = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d, refinement_limit=B), 0)
            c.store_attach_dev(n, stores[rows].data_ptr(), cdt(rows))
            ctxs[rows] = c
        q = torch.randn((nq, d), device=DEV, dtype=torch.float32)
        nset = max(3, -(-ROTATE_BYTES // (nq * B * d * 2)) + 1)
        idsets = [torch.randint(0, n, (nq, B), device=DEV, dtype=torch.int32) for _ in range(nset)]
        cnt = torch.full((nq,), B, dtype=torch.int32, device=DEV)
        oi, od, oc, sc = outs(nq, k)
        torch.cuda.synchronize()
        for rnd in range(2):
            for rows in rows_list:
                c = ctxs[rows]
                launches = [(lambda s=idsets[i % nset], c=c: c.refine_store_dev(nq, q.data_ptr(), N.F32, B, s.data_ptr(), cnt.data_ptr(), k, oi.data_ptr(),
                                                                                od.data_ptr(), oc.data_ptr(), sc.data_ptr())) for i in range(WARM + TIMED)]
                report(tag, "scan_gather", shape, rows, rnd, timed(c, launches), nq, B, d, k)
        for c in ctxs.values():
            c.close()
        del stores
        torch.cuda.empty_cache()


def embedlike(rng, d, r=32, noise=0.25):
    """float embeddings of intrinsic dimension r, O(1) elements"""
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)
    def draw(cnt):
        return (rng.standard_normal((cnt, r), dtype=np.float32) @ U + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)).astype(np.float32)
    return draw


def bench_search(tag, rows_list, shapes):
    n = 500_000
    for shape in shapes:
        nq, B, d, k = SHAPES[shape]
        pr = PROFILES[shape]
        rng = np.random.default_rng(1)
        draw = embedlike(rng, d)
        X16 = draw(n).astype(np.float16)           # the one rounding; both stores hold these values
        X = X16.astype(np.float32)
        bytes_run = any(r in ("u8", "i8") for r in rows_list)
        if bytes_run:                                # every store holds the quantised values (u8: shifted by 128, queries too)
            X = np.clip(np.rint(X * np.float32(BYTE_SCALE)), -128, 127).astype(np.float32)
            X16 = X.astype(np.float16)
        cfg = pkg.PaperRuntimeConfig(tables=pr["T"], divisions=pr["D"], m=pr["m"], lambda_=pr["lam"], dim=d, refinement_limit=B,
                                     max_global_candidates=pr["hard_cap"], probe_override=pr["probes"])
        ctxs = {}
        for rows in rows_list:
            c = pkg.FspannContext(cfg, 0)
            Xr = X + np.float32(128) if rows == "u8" else X
            c.registry_initialize(Xr[:1000].astype(np.float64))
            c.set_id_meta(n)
            c.build_index(Xr)
            if rows == "u8":
                c.store_set(Xr.astype(np.uint8), dtype=np.uint8)
            elif rows == "i8":
                c.store_set(X.astype(np.int8), dtype=np.int8)
            elif rows == "f16":
                c.store_set(X16, dtype=np.float16)
            elif rows == "bf16":
                c.store_set(torch.from_numpy(X).to(torch.bfloat16), dtype=pkg.bfloat16)
            elif rows == "f8":
                c.store_set(torch.from_numpy(X).to(torch.float8_e4m3fn), dtype=pkg.float8_e4m3fn)
            else:
                c.store_set(X)
            ctxs[rows] = c
        qs = [torch.from_numpy(draw(nq) * np.float32(BYTE_SCALE if bytes_run else 1.0)).to(DEV) for _ in range(6)]
        qs_u8 = [qq + 128 for qq in qs] if "u8" in rows_list else None
        oi, od, oc, sc = outs(nq, k)
        sel = torch.full((nq, B), -1, dtype=torch.int32, device=DEV)
        selc = torch.zeros(nq, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        for rnd in range(2):
            for rows in rows_list:
                c = ctxs[rows]
                qr = qs_u8 if rows == "u8" else qs
                launches = [(lambda qq=qr[i % len(qr)], c=c: c.search_store_dev(nq, qq.data_ptr(), N.F32, -1, B, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(),
                                                                                sc.data_ptr(), sel.data_ptr(), selc.data_ptr())) for i in range(WARM + TIMED)]
                ts = timed(c, launches)
                scored = float(sc.to(torch.float64).mean().item())
                report(tag, "search_store", shape, rows, rnd, ts, nq, B, d, k)
                print(f"{tag} search_store {shape} rows={rows} round={rnd}: mean scored rows per query {scored:.0f} of B={B}", flush=True)
        for c in ctxs.values():
            c.close()
        del X, X16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="f32,f16")
    ap.add_argument("--parts", default="dense,gather,search")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--tag", default="branch")
    a = ap.parse_args()
    rows_list, shapes = a.rows.split(","), a.shapes.split(",")
    print(f"# {a.tag}: lib {os.path.relpath(pkg._native._SO)}  rows {rows_list}  {WARM} warm-up + {TIMED} timed launches per reading", flush=True)
    for part in a.parts.split(","):
        dict(dense=bench_dense, gather=bench_gather, search=bench_search)[part](a.tag, rows_list, shapes)
