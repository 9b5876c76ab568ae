"""Dev tool: cost of the adaptive retry on the device (fspann_search_retry_dev) against fspann_search_store_dev, at BASELINE
config #2's shape (1 M x 128, 16 tables x 1 division, 16 x 32 bits, B = 256, Q = 1 024).  Method of tools/step_bench.py: whole
calls back to back, no events in the loop, one synchronisation at the end; the two calls alternate over three rounds.
  1. no short query (k = 10):        retry call vs fspann_search_store_dev
  2. 5 % short queries (k = 10):     most candidate rows of 5 % of the queries fail to load; the retry pass's cost, against a
                                     whole second pass (fspann_search_store_dev at 10 probes)
  3. B < 10 k (k = 30, all retry):   retry call vs two fspann_search_store_dev calls (pass 1, then 10 probes)"""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
n, d, T, m, lam, B, Q = 1000000, 128, 16, 16, 2, 256, 1024
REPS = int(os.environ.get("RETRY_BENCH_REPS", "300"))
rng = np.random.default_rng(1)
X = rng.standard_normal((n, d), dtype=np.float32)
ctx = pkg.FspannContext(pkg.PaperRuntimeConfig(tables=T, divisions=1, m=m, lambda_=lam, dim=d, refinement_limit=B), 0)
ctx.registry_initialize(X[:1000].astype(np.float64)); ctx.set_id_meta(n); ctx.build_index(X); ctx.store_set(X)
dev = torch.device("cuda", 0)
F32 = pkg._native.F32
qs = [torch.randn((Q, d), device=dev) for _ in range(8)]
kmax = 30
oi = torch.zeros((Q, kmax), dtype=torch.int32, device=dev); od = torch.zeros((Q, kmax), dtype=torch.float64, device=dev)
oc = torch.zeros(Q, dtype=torch.int32, device=dev); sc = torch.zeros(Q, dtype=torch.int32, device=dev)
sel = torch.zeros((Q, B), dtype=torch.int32, device=dev); selc = torch.zeros(Q, dtype=torch.int32, device=dev)
bad = torch.zeros(Q, dtype=torch.int32, device=dev); ret = torch.zeros(Q, dtype=torch.int32, device=dev)


def call(kind, q, k, po=-1):
    a = (Q, q.data_ptr(), F32, po, B, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr(), sc.data_ptr(), sel.data_ptr(), selc.data_ptr(), bad.data_ptr())
    if kind == "retry":
        ctx.search_retry_dev(*a, ret.data_ptr())
    else:
        ctx.search_store_dev(*a)


def timed(fn):
    for i in range(20):
        fn(i)
    ctx.sync()
    t0 = time.perf_counter()
    for i in range(REPS):
        fn(i)
    ctx.sync()
    return 1e6 * (time.perf_counter() - t0) / REPS


def ab(fa, fb):
    ra, rb = [], []
    for _ in range(3):
        ra.append(timed(fa)); rb.append(timed(fb))
    return min(ra), min(rb)


def retried(q, k):
    call("retry", q, k); ctx.sync()
    return int(ret.sum().item())


out = {}
# 1. no short query
nshort = [retried(qs[i], 10) for i in range(8)]
plain, retry = ab(lambda i: call("plain", qs[i % 8], 10), lambda i: call("retry", qs[i % 8], 10))
out["no_short"] = dict(retried_per_batch=nshort, store_dev_us=round(plain, 2), retry_dev_us=round(retry, 2), extra_us=round(retry - plain, 2))
# 3. B < 10 k: every query retries
plain2, retry2 = ab(lambda i: (call("plain", qs[i % 8], kmax), call("plain", qs[i % 8], kmax, 10)), lambda i: call("retry", qs[i % 8], kmax))
out["all_short"] = dict(retried=retried(qs[0], kmax), two_store_dev_us=round(plain2, 2), retry_dev_us=round(retry2, 2))
# 2. 5 % short queries: 70 % of the candidate rows of 51 queries fail to load (non-finite rows in a copy of the store)
q0 = qs[0]
call("plain", q0, 10); ctx.sync()
pick = np.sort(rng.choice(Q, Q // 20, replace=False))
s_np, c_np = sel.cpu().numpy(), selc.cpu().numpy()
ids = np.concatenate([s_np[i, :c_np[i]] for i in pick])
ids = ids[rng.random(len(ids)) < 0.7]
Xs = X.copy()
Xs[ids] = np.nan
ctx.store_set(Xs)
nr = retried(q0, 10)
plain3, retry3 = ab(lambda i: call("plain", q0, 10), lambda i: call("retry", q0, 10))
full2 = min(timed(lambda i: call("plain", q0, 10, 10)) for _ in range(3))
out["five_percent_short"] = dict(retried=nr, store_dev_us=round(plain3, 2), retry_dev_us=round(retry3, 2), retry_pass_us=round(retry3 - plain3, 2),
                                 full_second_pass_us=round(full2, 2))
print(json.dumps(out))
