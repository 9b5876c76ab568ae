"""Dev tool: encode kernel, exact fp64 VALU path vs MFMA fp32 GEMM + exact re-check vs the split-k MFMA path (mode 3).
SHAPE=cfg3 / cfg4: the shards of BASELINE configs #3 / #4.  ROUNDS=n: n rounds of the 20-call event timing per reading (median and
spread printed).  SPLITK=2,4,8: besides mode 3 under its own rule, one reading per forced slice count (FSPANN_ENCODE_SPLITK is
read when a context is made: each count gets a context of its own over the same GFunctions)."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
d, T, D, m, lam = 128, 16, 1, 16, 2
NQS = (1024, 262144)
if os.environ.get("SHAPE") == "cfg3": d, T, m, NQS = 960, 16, 16, (512, 4096)          # BASELINE config #3: GIST-shaped, 512 queries per GPU
if os.environ.get("SHAPE") == "cfg4": d, T, m, NQS = 768, 32, 32, (1024, 8192)         # config #4: 32 tables x 64 bits, 1 024 queries per GPU
ROUNDS = int(os.environ.get("ROUNDS", "1"))
SWEEP = [int(s) for s in os.environ.get("SPLITK", "").split(",") if s]
rng = np.random.default_rng(1)
S = rng.standard_normal((1000, d))
os.environ.pop("FSPANN_ENCODE_SPLITK", None)
ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=T, divisions=D, m=m, lambda_=lam, dim=d), 0)
ctx.registry_initialize(S)
legs = [(ctx, 1, "exact fp64 VALU"), (ctx, 2, "MFMA f32 + re-check")]
try:
    ctx.set_encode_mode(3)
    legs.append((ctx, 3, "split-k MFMA (rule)"))
    for s in SWEEP:
        os.environ["FSPANN_ENCODE_SPLITK"] = str(s)
        c = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=T, divisions=D, m=m, lambda_=lam, dim=d), 0)
        c.set_gfunctions(*ctx.get_gfunctions())
        legs.append((c, 3, f"split-k MFMA S={s}"))
except pkg.FspannArgumentError:
    print("(this library has no encode mode 3)")
F32 = pkg._native.F32
for nq in NQS:
    q = torch.randn((nq, d), device="cuda")
    codes = torch.zeros((nq, T * D, 1), dtype=torch.int64, device="cuda")
    want = None
    bad = torch.zeros(nq, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for c, mode, name in legs:
        stream = torch.cuda.ExternalStream(c.stream)
        c.set_encode_mode(mode)
        for _ in range(3):
            c.encode_dev(nq, q.data_ptr(), F32, codes.data_ptr(), 0, bad.data_ptr())
        c.sync()
        us = []
        for _ in range(ROUNDS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(20):
                c.encode_dev(nq, q.data_ptr(), F32, codes.data_ptr(), 0, bad.data_ptr())
            e1.record(stream)
            c.sync()
            us.append(e0.elapsed_time(e1) / 20 * 1e3)
        got = codes.cpu()
        want = got if want is None else want
        med = float(np.median(us))
        flops = 2.0 * nq * d * T * D * m
        print(f"nq={nq:7d} {name:22s} {med:9.1f} us  (min {min(us):.1f} max {max(us):.1f} of {ROUNDS})  {flops/med/1e6:8.2f} TFLOP/s  "
              f"rechecked={c.last_encode_rechecked()}  codes {'same' if torch.equal(got, want) else 'DIFFER'}", flush=True)
