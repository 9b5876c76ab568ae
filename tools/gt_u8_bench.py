"""Dev tool: exact ground truth over 1 M x 128 SIFT-like BYTES (fspann_groundtruth_typed_dev, FSPANN_U8) beside the fp32 call
over the same values widened (fspann_groundtruth_dev), k = 100, nq = 1 024 and 10 000.

  python tools/gt_u8_bench.py [--nq 1024,10000] [--readings a,b,c] [--rounds 3] [--warm 2] [--timed 5] [--tag NAME]
  AB_LIB=<path to another libfspann_hip.so> ...      reading (a) runs with that build (the parent's); without it (a) is left out

Readings: (a) AB_LIB's fspann_groundtruth_dev over fp32 rows; (b) this build, the same call; (c) this build, the typed call over
the bytes.  All live in one process (two libraries, one context each); per reading and round: `warm` warm-up calls, then `timed`
calls, each between two device events on the context's stream (a whole call: norms, distances and selection of every query
chunk); the readings alternate a / b / c over the rounds.  After the rounds: median and range (min .. max) of every reading's
timed calls, the outputs of (a) (or (b)) and (c) compared array for array, and the two verdicts — (b) inside the range of (a),
(c) faster than (a) by more than the width of (a)'s range.  `--readings c --rounds 1 --warm 0 --timed 1` is one (c) call, for
a kernel trace.
The signed leg: reading (d) is this build's typed call over the same scene shifted by -128 and held as SIGNED bytes (FSPANN_I8
base and queries: the same distances, so its outputs must equal (c)'s array for array), and reading (e) is AB_LIB's typed
(FSPANN_U8, FSPANN_U8) call, the parent's byte ground truth.  `--readings e,c,d` with AB_LIB set alternates the three; the verdict
is whether (d)'s median lies inside the range of (e) (without AB_LIB: of (c)) or below it — the signed path does strictly less work."""
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
N_BASE, D, K = 1_000_000, 128, 100


def siftlike(rng, n, d, r=16, noise=6.0):
    U = (rng.standard_normal((r, d)) / np.sqrt(r)).astype(np.float32)
    def draw(cnt):
        y = rng.standard_normal((cnt, r), dtype=np.float32) @ U
        return np.clip(np.rint(np.float32(64.0) + np.float32(48.0) * y + np.float32(noise) * rng.standard_normal((cnt, d), dtype=np.float32)), 0, 255).astype(np.float32)
    return draw


class OtherLib:
    """A context of another build of the library: only what reading (a) needs (its binding table may lack newer symbols)."""
    def __init__(self, path):
        self.L = L = C.CDLL(os.path.abspath(path))
        vp, i64, i = C.c_void_p, C.c_int64, C.c_int
        L.fspann_ctx_create.argtypes, L.fspann_ctx_create.restype = [i, C.POINTER(N.Cfg), C.POINTER(vp)], i
        L.fspann_ctx_destroy.argtypes, L.fspann_ctx_destroy.restype = [vp], None
        L.fspann_ctx_stream.argtypes, L.fspann_ctx_stream.restype = [vp], vp
        L.fspann_sync.argtypes, L.fspann_sync.restype = [vp], i
        L.fspann_last_error.restype = C.c_char_p
        L.fspann_groundtruth_dev.argtypes, L.fspann_groundtruth_dev.restype = [vp, i64, vp, i64, vp, i, i, vp, vp], i
        L.fspann_groundtruth_typed_dev.argtypes, L.fspann_groundtruth_typed_dev.restype = [vp, i64, vp, i, i64, vp, i, i, i, vp, vp], i
        self.h = vp()
        cc = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=D).to_c()
        self.ck(L.fspann_ctx_create(0, C.byref(cc), C.byref(self.h)))
        self.stream = int(L.fspann_ctx_stream(self.h) or 0)

    def ck(self, rc):
        if rc != 0:
            raise RuntimeError(f"other library: rc {rc}: {self.L.fspann_last_error().decode()}")

    def groundtruth_dev(self, n, b, nq, q, d, k, ids, d2):
        self.ck(self.L.fspann_groundtruth_dev(self.h, n, b, nq, q, d, k, ids, d2))

    def groundtruth_typed_dev(self, n, b, bdt, nq, q, qdt, d, k, ids, d2):
        self.ck(self.L.fspann_groundtruth_typed_dev(self.h, n, b, bdt, nq, q, qdt, d, k, ids, d2))

    def sync(self):
        self.ck(self.L.fspann_sync(self.h))

    def close(self):
        self.L.fspann_ctx_destroy(self.h)


def timed(ctx, call, warm, reps):
    stream = torch.cuda.ExternalStream(ctx.stream)
    for _ in range(warm):
        call()
    ctx.sync()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in evs:
        e0.record(stream)
        call()
        e1.record(stream)
    ctx.sync()
    return [e0.elapsed_time(e1) for e0, e1 in evs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", default="1024,10000")
    ap.add_argument("--readings", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--timed", type=int, default=5)
    ap.add_argument("--tag", default="gt_u8")
    a = ap.parse_args()
    readings = a.readings.split(",")
    ab = os.environ.get("AB_LIB")
    for r in ("a", "e"):
        if r in readings and not ab:
            print(f"# AB_LIB is not set: reading ({r}) is left out", flush=True)
            readings.remove(r)
    rng = np.random.default_rng(1)
    draw = siftlike(rng, N_BASE, D)
    X8 = draw(N_BASE).astype(np.uint8)
    nqs = [int(v) for v in a.nq.split(",")]
    Q8 = draw(max(nqs)).astype(np.uint8)
    x8 = torch.from_numpy(X8).to(DEV)
    q8 = torch.from_numpy(Q8).to(DEV)
    xs8 = (x8.to(torch.int16) - 128).to(torch.int8) if "d" in readings else None      # the same scene as signed bytes
    qs8 = (q8.to(torch.int16) - 128).to(torch.int8) if "d" in readings else None
    x32 = x8.to(torch.float32) if ("a" in readings or "b" in readings) else None
    q32 = q8.to(torch.float32) if x32 is not None else None
    torch.cuda.synchronize()
    ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=D), 0)
    other = OtherLib(ab) if ("a" in readings or "e" in readings) else None
    print(f"# {a.tag}: n {N_BASE} d {D} k {K}  lib {os.path.relpath(N._SO)}  AB_LIB {ab}  {a.rounds} rounds x ({a.warm} warm-up + {a.timed} timed calls)",
          flush=True)
    for nq in nqs:
        out = {r: (torch.zeros((nq, K), dtype=torch.int32, device=DEV), torch.zeros((nq, K), dtype=torch.float64, device=DEV)) for r in readings}
        calls = {
            "a": (other, lambda: other.groundtruth_dev(N_BASE, x32.data_ptr(), nq, q32.data_ptr(), D, K, out["a"][0].data_ptr(), out["a"][1].data_ptr())),
            "b": (ctx, lambda: ctx.groundtruth_dev(N_BASE, x32.data_ptr(), nq, q32.data_ptr(), D, K, out["b"][0].data_ptr(), out["b"][1].data_ptr())),
            "c": (ctx, lambda: ctx.groundtruth_typed_dev(N_BASE, x8.data_ptr(), N.U8, nq, q8.data_ptr(), N.U8, D, K, out["c"][0].data_ptr(),
                                                         out["c"][1].data_ptr())),
            "d": (ctx, lambda: ctx.groundtruth_typed_dev(N_BASE, xs8.data_ptr(), N.I8, nq, qs8.data_ptr(), N.I8, D, K, out["d"][0].data_ptr(),
                                                         out["d"][1].data_ptr())),
            "e": (other, lambda: other.groundtruth_typed_dev(N_BASE, x8.data_ptr(), N.U8, nq, q8.data_ptr(), N.U8, D, K, out["e"][0].data_ptr(),
                                                             out["e"][1].data_ptr())),
        }
        ts = {r: [] for r in readings}
        for rnd in range(a.rounds):
            for r in readings:
                c, f = calls[r]
                t = timed(c, f, a.warm, a.timed)
                ts[r] += t
                print(f"{a.tag} nq={nq} reading={r} round={rnd}: " + " ".join(f"{v:.3f}" for v in t) + " ms", flush=True)
        st = {r: (float(np.median(v)), min(v), max(v)) for r, v in ts.items()}
        for r in readings:
            med, lo, hi = st[r]
            print(f"{a.tag} nq={nq} reading={r}: median {med:.3f} ms  range {lo:.3f} .. {hi:.3f} ms  ({len(ts[r])} calls)", flush=True)
        ref = "a" if "a" in readings else ("b" if "b" in readings else None)
        if ref and "c" in readings:
            same = bool(torch.equal(out[ref][0], out["c"][0]) and torch.equal(out[ref][1], out["c"][1]))
            print(f"{a.tag} nq={nq}: ids and squared distances of ({ref}) and (c) equal: {same}", flush=True)
        if "a" in readings and "b" in readings:
            print(f"{a.tag} nq={nq}: (b) median inside the range of (a): {st['a'][1] <= st['b'][0] <= st['a'][2]}", flush=True)
        if "a" in readings and "c" in readings:
            width = st["a"][2] - st["a"][1]
            print(f"{a.tag} nq={nq}: (c) faster than (a) by {st['a'][0] - st['c'][0]:.3f} ms = {st['a'][0] / st['c'][0]:.2f}x; the range of (a) is "
                  f"{width:.3f} ms wide: {st['a'][0] - st['c'][0] > width}", flush=True)
        if "d" in readings and ("c" in readings or "e" in readings):
            u = "e" if "e" in readings else "c"
            same = bool(torch.equal(out[u][0], out["d"][0]) and torch.equal(out[u][1], out["d"][1]))
            print(f"{a.tag} nq={nq}: ids and squared distances of ({u}) and (d) equal: {same}", flush=True)
            print(f"{a.tag} nq={nq}: (d) median {st['d'][0]:.3f} ms against ({u}) {st[u][0]:.3f} ms (range {st[u][1]:.3f} .. {st[u][2]:.3f}): inside the "
                  f"range or below it: {st['d'][0] <= st[u][2]}", flush=True)
        del out
    ctx.close()
    if other:
        other.close()


if __name__ == "__main__":
    main()
