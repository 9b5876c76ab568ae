"""Dev tool: cost of the touched-record set (fspann_touch_*) at BASELINE config #2's shape (1 M x 128, 16 tables x 1 division,
16 x 32 bits, B = 256, Q = 1 024, resident fp32 store).  Method of tools/retry_bench.py: whole calls back to back, one
synchronisation at the end, off and on alternating over three rounds.
  1. fspann_search_retry_dev step time with tracking off and on (the mark kernels behind each Refine)
  2. fspann_touch_drain of the set after one batch, 1 M handles, host wall time per call (count + scan + compaction + copy and
     two synchronisations), with reset (the clearing stores included) and without; the set is refilled before every call
  3. the same with a 10 M-handle set (dim 4 store, 262 144 marks by one fspann_refine_store_dev)
Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/touch_bench.py` (touch_* kernels), with
TOUCH_BENCH_KEEP=0 so that every drain profiled is a resetting one."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
n, d, T, m, lam, B, Q, K = 1000000, 128, 16, 16, 2, 256, 1024, 10
REPS = int(os.environ.get("TOUCH_BENCH_REPS", "200"))
KEEP = os.environ.get("TOUCH_BENCH_KEEP", "1") != "0"     # 0: resetting drains only (kernel stats of the real drain)
rng = np.random.default_rng(1)
X = rng.standard_normal((n, d), dtype=np.float32)
ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=T, divisions=1, m=m, lambda_=lam, dim=d, refinement_limit=B), 0)
ctx.registry_initialize(X[:1000].astype(np.float64)); ctx.set_id_meta(n); ctx.build_index(X); ctx.store_set(X)
dev = torch.device("cuda", 0)
F32 = pkg._native.F32
qs = [torch.randn((Q, d), device=dev) for _ in range(8)]
oi = torch.zeros((Q, K), dtype=torch.int32, device=dev); od = torch.zeros((Q, K), dtype=torch.float64, device=dev)
oc = torch.zeros(Q, dtype=torch.int32, device=dev); sc = torch.zeros(Q, dtype=torch.int32, device=dev)
sel = torch.zeros((Q, B), dtype=torch.int32, device=dev); selc = torch.zeros(Q, dtype=torch.int32, device=dev)
bad = torch.zeros(Q, dtype=torch.int32, device=dev); ret = torch.zeros(Q, dtype=torch.int32, device=dev)
torch.cuda.synchronize()


def step(i):
    ctx.search_retry_dev(Q, qs[i % 8].data_ptr(), F32, -1, B, K, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), sc.data_ptr(), sel.data_ptr(),
                         selc.data_ptr(), bad.data_ptr(), ret.data_ptr())


def timed(fn, reps=REPS):
    for i in range(10):
        fn(i)
    ctx.sync()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i)
    ctx.sync()
    return 1e6 * (time.perf_counter() - t0) / reps


out = {}
ctx.touch_enable(True)
ctx.touch_enable(False)
t_off, t_on = [], []
for _ in range(3):
    ctx.touch_enable(False); t_off.append(timed(step))
    ctx.touch_enable(True); t_on.append(timed(step))
out["step_off_us"], out["step_on_us"] = min(t_off), min(t_on)
out["step_overhead_pct"] = 100.0 * (out["step_on_us"] - out["step_off_us"]) / out["step_off_us"]
ctx.drain_touched(reset=True)
step(0); ctx.sync()
out["touched_one_batch"] = ctx.touched_count()
hb = np.empty(n, np.int32)
import ctypes as C
nn = C.c_int64(0)
L = pkg._native.lib()


def drain_wall(c, remark, reset, reps=10):
    """Median host wall time of one fspann_touch_drain into a buffer of every handle (count + scan + compaction [+ clearing
    stores] + copy + two synchronisations); the set is filled again by `remark` (not timed) before every call."""
    ts = []
    for i in range(reps):
        remark(i)
        c.sync()
        t0 = time.perf_counter()
        pkg._native.check(L.fspann_touch_drain(c.handle, hb.ctypes.data_as(C.c_void_p), len(hb), C.byref(nn), reset))
        ts.append(1e6 * (time.perf_counter() - t0))
    return float(np.median(ts)), int(nn.value)


out["drain_1m_reset_us"], out["drain_1m_n"] = drain_wall(ctx, step, 1)
if KEEP:
    out["drain_1m_keep_us"], _ = drain_wall(ctx, step, 0)
ctx.touch_enable(False)
ctx.close()

# a 10 M-handle set: a dim-4 store, 262 144 scattered marks
n10, d10 = 10000000, 4
c10 = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=1, divisions=1, m=8, lambda_=2, dim=d10, refinement_limit=B), 0)
c10.set_id_meta(n10)
c10.store_attach_dev(n10, (X10 := torch.randn((n10, d10), device=dev)).data_ptr(), F32)
c10.touch_enable(True)
ids10 = torch.from_numpy(rng.choice(n10, Q * B, replace=False).astype(np.int32).reshape(Q, B)).to(dev)
cnt10 = torch.full((Q,), B, dtype=torch.int32, device=dev)
q10 = torch.randn((Q, d10), device=dev)
torch.cuda.synchronize()


def mark10(i):
    c10.refine_store_dev(Q, q10.data_ptr(), F32, B, ids10.data_ptr(), cnt10.data_ptr(), K, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), sc.data_ptr())


hb = np.empty(n10, np.int32)
out["drain_10m_reset_us"], out["drain_10m_n"] = drain_wall(c10, mark10, 1)
if KEEP:
    out["drain_10m_keep_us"], _ = drain_wall(c10, mark10, 0)
c10.close()
print(json.dumps(out))
