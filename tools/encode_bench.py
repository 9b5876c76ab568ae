"""Dev tool: encode kernel, exact fp64 VALU path vs MFMA fp32 GEMM + exact re-check vs the split-k MFMA path (mode 3) vs the k-wave
MFMA kernel (set_encode_kwaves).
SHAPE=cfg3 / cfg4: the shards of BASELINE configs #3 / #4.  ROUNDS=n: n rounds of the 20-call event timing per reading (median and
spread printed); the legs ALTERNATE inside a round, so every reading of a round is taken next to the others.
SPLITK=2,4,8: besides mode 3 under its own rule, one reading per forced slice count (FSPANN_ENCODE_SPLITK is read when a context is
made: each count gets a context of its own over the same GFunctions).
KWAVES=2,4: one reading per k-group count of the k-wave kernel (mode 2 with set_encode_kwaves(G)).
PARENT_LIB=path: another build of libfspann_hip.so (the parent commit's) loaded beside this one; its exact and unsplit MFMA readings
alternate with this library's in the same process.
NQ=n: that batch size alone.  ONLY=text: only the legs whose name contains text (a kernel trace of one variant alone: ONLY=k-wave)."""
import ctypes as C
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
N = pkg._native
d, T, D, m, lam = 128, 16, 1, 16, 2
NQS = (1024, 262144)
if os.environ.get("SHAPE") == "cfg3": d, T, m, NQS = 960, 16, 16, (512, 4096)          # BASELINE config #3: GIST-shaped, 512 queries per GPU
if os.environ.get("SHAPE") == "cfg4": d, T, m, NQS = 768, 32, 32, (1024, 8192)         # config #4: 32 tables x 64 bits, 1 024 queries per GPU
if os.environ.get("NQ"): NQS = (int(os.environ["NQ"]),)
ROUNDS = int(os.environ.get("ROUNDS", "1"))
SWEEP = [int(s) for s in os.environ.get("SPLITK", "").split(",") if s]
KWAVES = [int(s) for s in os.environ.get("KWAVES", "").split(",") if s]
F32 = N.F32


class ParentCtx:
    """A context of another build of the library: the few calls this tool makes, bound by hand (that build's own Python is not here)."""

    def __init__(self, path, cfg, gfunctions):
        self.L = L = C.CDLL(path)
        vp, i64 = C.c_void_p, C.c_int64
        for name, res, args in (("fspann_ctx_create", C.c_int, [C.c_int, C.POINTER(N.Cfg), C.POINTER(vp)]), ("fspann_ctx_destroy", None, [vp]),
                                ("fspann_ctx_stream", vp, [vp]), ("fspann_sync", C.c_int, [vp]), ("fspann_set_gfunctions", C.c_int, [vp, vp, vp, vp]),
                                ("fspann_set_encode_mode", C.c_int, [vp, C.c_int]), ("fspann_last_encode_rechecked", i64, [vp]),
                                ("fspann_encode_dev", C.c_int, [vp, i64, vp, C.c_int, vp, vp, vp])):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
        h = vp()
        assert L.fspann_ctx_create(0, C.byref(cfg.to_c()), C.byref(h)) == 0
        self._h = h
        self.g = [np.ascontiguousarray(a, np.float64) for a in gfunctions]
        assert L.fspann_set_gfunctions(h, *[a.ctypes.data_as(vp) for a in self.g]) == 0
        self.stream = L.fspann_ctx_stream(h)

    def set_encode_mode(self, mode): assert self.L.fspann_set_encode_mode(self._h, mode) == 0
    def encode_dev(self, nq, q, dt, codes, hashes, bad): assert self.L.fspann_encode_dev(self._h, nq, q, dt, codes, hashes or None, bad) == 0
    def sync(self): assert self.L.fspann_sync(self._h) == 0
    def last_encode_rechecked(self): return int(self.L.fspann_last_encode_rechecked(self._h))


rng = np.random.default_rng(1)
S = rng.standard_normal((1000, d))
os.environ.pop("FSPANN_ENCODE_SPLITK", None)
os.environ.pop("FSPANN_ENCODE_KWAVES", None)
cfg = pkg.PaperRuntimeConfig(tables=T, divisions=D, m=m, lambda_=lam, dim=d)
ctx = pkg.FspannContext(cfg, 0)
ctx.registry_initialize(S)
has_kwaves = hasattr(ctx.L, "fspann_set_encode_kwaves")
# a leg: (context, encode mode, k-groups, name)
legs = [(ctx, 1, 0, "exact fp64 VALU"), (ctx, 2, 0, "MFMA f32 + re-check")]
if os.environ.get("PARENT_LIB"):
    par = ParentCtx(os.environ["PARENT_LIB"], cfg, ctx.get_gfunctions())
    legs += [(par, 1, 0, "parent: exact fp64 VALU"), (par, 2, 0, "parent: MFMA f32"), ]
try:
    ctx.set_encode_mode(3)
    legs.append((ctx, 3, 0, "split-k MFMA (rule)"))
    for s in SWEEP:
        os.environ["FSPANN_ENCODE_SPLITK"] = str(s)
        c = pkg.FspannContext(cfg, 0)
        c.set_gfunctions(*ctx.get_gfunctions())
        legs.append((c, 3, 0, f"split-k MFMA S={s}"))
except pkg.FspannArgumentError:
    print("(this library has no encode mode 3)")
if has_kwaves:
    legs += [(ctx, 2, G, f"k-wave MFMA G={G}") for G in KWAVES]
elif KWAVES:
    print("(this library has no k-wave encode)")
if os.environ.get("ONLY"):
    legs = [leg for leg in legs if os.environ["ONLY"] in leg[3]]


def arm(c, mode, groups):
    c.set_encode_mode(mode)
    if has_kwaves and c is ctx:
        c.set_encode_kwaves(groups)


for nq in NQS:
    q = torch.randn((nq, d), device="cuda")
    codes = torch.zeros((nq, T * D, 1), dtype=torch.int64, device="cuda")
    bad = torch.zeros(nq, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    us, got, fixed = {}, {}, {}
    for c, mode, groups, name in legs:                               # warm-up of every leg, and its codes
        arm(c, mode, groups)
        for _ in range(3):
            c.encode_dev(nq, q.data_ptr(), F32, codes.data_ptr(), 0, bad.data_ptr())
        c.sync()
        got[name], fixed[name], us[name] = codes.cpu(), c.last_encode_rechecked(), []
    for _ in range(ROUNDS):
        for c, mode, groups, name in legs:
            arm(c, mode, groups)
            stream = torch.cuda.ExternalStream(c.stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(20):
                c.encode_dev(nq, q.data_ptr(), F32, codes.data_ptr(), 0, bad.data_ptr())
            e1.record(stream)
            c.sync()
            us[name].append(e0.elapsed_time(e1) / 20 * 1e3)
    want = got[legs[0][3]]
    for c, mode, groups, name in legs:
        med = float(np.median(us[name]))
        flops = 2.0 * nq * d * T * D * m
        print(f"nq={nq:7d} {name:24s} {med:9.1f} us  (min {min(us[name]):.1f} max {max(us[name]):.1f} of {ROUNDS})  {flops/med/1e6:8.2f} TFLOP/s  "
              f"rechecked={fixed[name]}  codes {'same' if torch.equal(got[name], want) else 'DIFFER'}", flush=True)
