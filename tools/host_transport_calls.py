#!/usr/bin/env python3
"""Dev tool (GPU box): how many copy commands, launches and synchronisations each host-pointer call issues on each transport.

  rocprofv3 --hip-runtime-trace --output-format csv -d OUT -- python3 tools/host_transport_calls.py      (HIP runtime tracing only)
  python3 tools/host_transport_calls.py --parse OUT                                                      -> one line per case
  AB_LIB=<path to another libfspann_hip.so> rocprofv3 ...                                                the same with another build

Every case (the sizes of tests/test_gpu_host_transports.py) is issued twice on a fresh context: once to settle the allocations, once
bracketed by two hipDeviceSynchronize calls of this script (the library never calls it), which is how --parse finds it in the trace."""
import ctypes
import csv
import glob
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTED = ("hipMemcpyAsync", "hipMemcpy", "launch", "hipStreamSynchronize")
N, D, B, K = 2000, 8, 64, 10


def cases():
    """(name, FSPANN_ZERO_COPY, call(ctx, data))"""
    out = []
    for name, zc, nq in (("encode mapped", "1", 1), ("encode direct (zero copy off)", "0", 1), ("encode direct (nq 5)", "1", 5)):
        for hashes in (False, True):
            out.append((f"{name}{', hashes' if hashes else ''}", zc, lambda c, d, nq=nq, h=hashes: c.encode(d["Q"][:nq], want_hashes=h)))
    for name, zc, nq, cap in (("route mapped", "1", 1, B), ("route block (zero copy off)", "0", 1, B), ("route block (nq 5)", "1", 5, B),
                              ("route direct (cap 140000)", "1", 1, 140000)):
        for counters in (True, False):
            out.append((f"{name}, counters {'on' if counters else 'off'}", zc,
                        lambda c, d, nq=nq, cap=cap, cn=counters: c.route(d["codes"][:nq], limit=B, cap=cap, counters=cn)))
    for name, b, cnt, dt in (("refine mapped (B 64)", 64, 50, "float64"), ("refine block (B 2100)", 2100, 64, "float64"),
                             ("refine direct (B 262148)", 262148, 300, "float32")):
        out.append((name, "1", lambda c, d, b=b, cnt=cnt, dt=dt: c.refine(d["Q"][:1].astype(dt), d["rows"](b, dt), d["ids"](b), [cnt], K)))
    for nq in (1, 5):
        out.append((f"refine_store (nq {nq})", "1", lambda c, d, nq=nq: c.refine_store(d["Q"][:nq], d["sids"][:nq], [100] * nq, K)))
    return out


def run():
    import numpy as np
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    if os.environ.get("AB_LIB"):
        pkg._native._SO = os.path.abspath(os.environ["AB_LIB"])
    hip = ctypes.CDLL("libamdhip64.so")
    rng = np.random.default_rng(3)
    X = rng.standard_normal((N, D)).astype(np.float32)
    data = dict(Q=rng.standard_normal((5, D)).astype(np.float32).astype(np.float64),
                sids=np.stack([rng.permutation(N)[:100] for _ in range(5)]).astype(np.int32),
                ids=lambda b: (np.arange(b, dtype=np.int32) % N)[None], rows=lambda b, dt: X[np.arange(b) % N].astype(dt)[None])
    cfg = pkg.PaperRuntimeConfig(tables=2, divisions=2, m=6, lambda_=2, dim=D, refinement_limit=B)
    gf = None
    for name, zc, call in cases():
        os.environ["FSPANN_ZERO_COPY"] = zc
        with pkg.FspannContext(cfg, 0) as ctx:
            if gf is None:
                ctx.registry_initialize(X[:1000].astype(np.float64))
                gf = ctx.get_gfunctions()
            else:
                ctx.set_gfunctions(*gf)
            ctx.set_id_meta(N)
            ctx.build_index(X)
            ctx.store_set(X)
            data["codes"] = ctx.encode(data["Q"])
            call(ctx, data)
            hip.hipDeviceSynchronize()
            call(ctx, data)
            hip.hipDeviceSynchronize()
    print(f"{len(cases())} cases issued")


def parse(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*hip_api_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    brackets, cur = [], None
    for r in rows:
        f = r["Function"]
        if f == "hipDeviceSynchronize":
            if cur is None:
                cur = Counter()
            else:
                brackets.append(cur)
                cur = None
        elif cur is not None:
            cur["launch" if "LaunchKernel" in f else f] += 1
    names = [c[0] for c in cases()]
    assert len(brackets) == len(names), (len(brackets), len(names))
    print(f"{'case':44s}" + "".join(f"{k:>22s}" for k in COUNTED))
    for n, b in zip(names, brackets):
        print(f"{n:44s}" + "".join(f"{b[k]:22d}" for k in COUNTED))


if __name__ == "__main__":
    parse(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--parse" else run()
