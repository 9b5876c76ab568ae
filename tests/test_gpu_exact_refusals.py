"""GPU: what the exact-scan calls (ground truth, metrics at one k and at every k, exact top-1, validate) answer to arguments they
refuse, over the C ABI itself (ctypes, no package-side checks), on one tiny context.

1. Dtype pairs test_gpu_dtype_dispatch's matrix does not hold: fspann_eval_kvariants_dev answers every pair of DTYPES exactly as
   fspann_eval_metrics_typed_dev does, and fspann_nn1_exact_dev / fspann_gt_validate_dev their own two sentences.
2. Which refusal wins when two arguments are wrong at once: one case per adjacent pair of each call's checks, nq = 0 with a bad
   stride or a bad k included (the refusal still comes; nq = 0 alone is FSPANN_OK).

Every expectation is the return code and the WHOLE fspann_last_error() string, written out here and not derived from the library.
Nothing is launched that can go wrong: every case is a refusal, nq = 0, or a valid call at dim = 16, n = 4, nq = 2, k = 2."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_gpu_dtype_dispatch import DTYPES, F32, F64, U8, F16, I8, NAMES, _check, _dev, _hp, _name, want_metrics_typed

pytestmark = pytest.mark.gpu

OK, E_STATE, E_ARG, E_NULL = 0, -1, -2, -3

GT_NULL = (E_NULL, "ground truth buffer is null")
GT_EMPTY = (E_ARG, "Empty or malformed vector files (zero records).")
GT_K = (E_ARG, "k must be in [1, 1024]")
GT_ROWS = "ground truth rows are FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3 (the reference's ground truth reads floats): base %s (%d)"
GT_NO_F64_STORE = (E_ARG, "no ground truth over an FSPANN_F64 store: the reference's ground truth reads floats")
M_NULL = (E_NULL, "metrics buffer is null")
M_SHAPE = (E_ARG, "k must be in [1, 1024] and gt must hold >= k ids per query")
KV_NQ = (E_ARG, "nq < 0 or nq > INT32_MAX")
KV_PAIR = (E_ARG, "unique_dev and cand_ratio_dev go together: both or neither")
NN1_NULL = (E_NULL, "exact top-1 buffer is null")
NN1_NO_F64_STORE = (E_ARG, "no exact top-1 over an FSPANN_F64 store: the reference's validator reads floats or bytes")
NO_STORE = (E_STATE, "plaintext store not set")
GOOD = (OK, None)


def want_nn1(b, q):
    """fspann_nn1_exact_dev and fspann_gt_validate_dev: the rows' sentence, then the queries'"""
    if b not in NAMES or b == F64:
        return E_ARG, ("exact top-1 rows are FSPANN_F32, FSPANN_U8, FSPANN_I8, FSPANN_F16, FSPANN_BF16 or FSPANN_F8E4M3 (the reference's validator reads floats or bytes): "
                       "base %s (%d)" % (_name(b), b))
    if q not in (F32, F64):
        return E_ARG, "exact top-1 queries are FSPANN_F64 (the reference's double[]) or FSPANN_F32: query %s (%d)" % (_name(q), q)
    return GOOD


def test_exact_scan_refusals(pkg):
    import torch
    L = pkg._native.lib()
    d, n, nq, B, k = 16, 4, 2, 4, 2
    cfg = pkg.PaperRuntimeConfig(tables=2, divisions=1, m=4, lambda_=2, dim=d, refinement_limit=B, block_size=2, default_probes=1)
    # zeros are a finite value of every dtype: one zeroed block serves as queries, rows and ground-truth base of every type
    Zd = _dev(np.zeros(4096, np.uint8))
    z = Zd.data_ptr()
    ids = _dev(np.tile(np.arange(B, dtype=np.int32), (nq, 1))).data_ptr()      # result lists and ground truth [nq][B]: ids 0 .. 3
    dev = torch.device("cuda", 0)
    o_ids = torch.zeros((nq, B), dtype=torch.int32, device=dev)
    o_d2 = torch.zeros((nq, B), dtype=torch.float64, device=dev)
    o_f64 = torch.zeros((3, 3, nq), dtype=torch.float64, device=dev)             # recall, ratio, cand_ratio of up to three k
    o_uq = torch.ones(nq, dtype=torch.int32, device=dev)
    oi, od, uq = o_ids.data_ptr(), o_d2.data_ptr(), o_uq.data_ptr()
    rec, rat, crat = (o_f64[i].data_ptr() for i in range(3))
    val = pkg._native.GtValidation()
    with pkg.FspannContext(cfg, 0) as ctx:
        h = ctx.handle

        def run(what, want, fn, *args):
            rc = fn(h, *args)
            _check(L, what, rc, want)
            ctx.sync()

        def kvariants(what, want, ks, nk=None, n_=n, base=z, b=F32, nq_=nq, q=F32, ann_stride=B, gt_stride=B, unique=uq, cand=crat):
            arr = None if ks is None else (C.c_int32 * len(ks))(*ks)
            run(("eval_kvariants_dev",) + what, want, L.fspann_eval_kvariants_dev, n_, base, b, nq_, z, q, d, arr, len(ks) if nk is None else nk, ids, ann_stride, None,
                ids, gt_stride, unique, rec, rat, cand)

        # ---- the dtype pairs --------------------------------------------------------------------------------------------------
        for b, q in itertools.product(DTYPES, DTYPES):
            kvariants((b, q), want_metrics_typed(b, q), [2, 1], b=b, q=q)
            run(("nn1_exact_dev", b, q), want_nn1(b, q), L.fspann_nn1_exact_dev, n, z, b, nq, z, q, d, None, nq, oi, od)
            run(("gt_validate_dev", b, q), want_nn1(b, q), L.fspann_gt_validate_dev, n, z, b, nq, z, q, d, ids, nq, B, 2, 0.0, C.byref(val))

        # ---- the three ground-truth calls: null buffer, dtype or pair, n / nq / dim, (bytes) dim > 32768, k, nq == 0 ----------------
        gt, rows, typed = L.fspann_groundtruth_dev, L.fspann_groundtruth_rows_dev, L.fspann_groundtruth_typed_dev
        run("gt: null, n", GT_NULL, gt, 0, None, nq, z, d, k, oi, od)
        run("gt: null ids, k", GT_NULL, gt, n, z, nq, z, d, 0, None, od)
        run("gt: n, k", GT_EMPTY, gt, 0, z, nq, z, d, 0, oi, od)
        run("gt: n = 2^31, k", GT_EMPTY, gt, 1 << 31, z, nq, z, d, 0, oi, od)
        run("gt: nq < 0, k", GT_EMPTY, gt, n, z, -1, z, d, 0, oi, od)
        run("gt: dim, k, nq = 0", GT_EMPTY, gt, n, z, 0, z, 0, 1025, oi, od)
        run("gt: k, nq = 0", GT_K, gt, n, z, 0, z, d, 0, oi, od)
        run("gt: k = 1025", GT_K, gt, n, z, nq, z, d, 1025, oi, od)
        run("gt: nq = 0", GOOD, gt, n, z, 0, z, d, k, oi, od)
        run("gt", GOOD, gt, n, z, nq, z, d, k, oi, None)
        run("rows: null, dtype", GT_NULL, rows, n, None, F64, nq, z, d, k, oi, od)
        run("rows: null q, F32, n", GT_NULL, rows, 0, z, F32, nq, None, d, k, oi, od)
        run("rows: dtype, n", (E_ARG, GT_ROWS % ("FSPANN_F64", 1)), rows, 0, z, F64, nq, z, d, k, oi, od)
        run("rows: dtype, k, nq = 0", (E_ARG, GT_ROWS % ("unknown dtype", 7)), rows, n, z, 7, 0, z, d, 0, oi, od)
        for t in (F32, U8, F16):
            run(("rows: n, k", t), GT_EMPTY, rows, 0, z, t, nq, z, d, 0, oi, od)
            run(("rows: k, nq = 0", t), GT_K, rows, n, z, t, 0, z, d, 1025, oi, od)
            run(("rows: nq = 0", t), GOOD, rows, n, z, t, 0, z, d, k, oi, od)
        run("typed: null, pair", GT_NULL, typed, n, z, F16, nq, None, F32, d, k, oi, od)
        run("typed: named, n", (E_ARG, "no ground truth over FSPANN_F16 (base and query are both FSPANN_F32 or both FSPANN_U8): base FSPANN_F16, query FSPANN_F32"),
            typed, 0, z, F16, nq, z, F32, d, k, oi, od)
        run("typed: match, n, nq = 0", (E_ARG, "Base and query types must match (both fvecs or both bvecs): base FSPANN_U8, query FSPANN_F32"),
            typed, 0, z, U8, 0, z, F32, d, k, oi, od)
        for t in (F32, U8, I8):
            run(("typed: n, dim > 32768, k", t), GT_EMPTY, typed, 0, z, t, nq, z, t, 32769, 0, oi, od)
            run(("typed: k, nq = 0", t), GT_K, typed, n, z, t, 0, z, t, d, 0, oi, od)
            run(("typed: nq = 0", t), GOOD, typed, n, z, t, 0, z, t, d, k, oi, od)
            run(("typed", t), GOOD, typed, n, z, t, nq, z, t, d, k, oi, od)
        # the integer path alone has a largest dim, asked for between n / nq / dim and k
        run("typed: dim > 32768, k, F32", GT_K, typed, n, z, F32, nq, z, F32, 32769, 0, oi, od)
        run("typed: dim > 32768, k, U8", (E_ARG, "dim 32769 > 32768: FSPANN_U8 distances would not fit 32 bits"), typed, n, z, U8, nq, z, U8, 32769, 0, oi, od)
        run("typed: dim > 32768, nq = 0, I8", (E_ARG, "dim 32769 > 32768: FSPANN_I8 distances would not fit 32 bits"), typed, n, z, I8, 0, z, I8, 32769, k, oi, od)

        # ---- the two metrics calls: null, pair, shape, nq == 0 ----------------------------------------------------------------------
        met, mtyped = L.fspann_eval_metrics_dev, L.fspann_eval_metrics_typed_dev
        run("metrics: null, k", M_NULL, met, n, z, nq, z, d, 0, ids, B, None, ids, B, None, rat)
        run("metrics: k, nq = 0", M_SHAPE, met, n, z, 0, z, d, 0, ids, B, None, ids, B, rec, rat)
        run("metrics: gt_stride < k, nq = 0", M_SHAPE, met, n, z, 0, z, d, k, ids, B, None, ids, k - 1, rec, rat)
        run("metrics: ann_stride, nq = 0", M_SHAPE, met, n, z, 0, z, d, k, ids, 0, None, ids, B, rec, rat)
        run("metrics: nq < 0", M_SHAPE, met, n, z, -1, z, d, k, ids, B, None, ids, B, rec, rat)
        run("metrics: nq = 0", GOOD, met, n, z, 0, z, d, k, ids, B, None, ids, B, rec, rat)
        run("metrics", GOOD, met, n, z, nq, z, d, k, ids, B, None, ids, B, rec, rat)
        run("metrics_typed: null, pair", M_NULL, mtyped, n, z, F64, nq, z, F16, d, k, None, B, None, ids, B, rec, rat)
        run("metrics_typed: pair, k", want_metrics_typed(U8, I8), mtyped, n, z, U8, nq, z, I8, d, 0, ids, B, None, ids, B, rec, rat)
        run("metrics_typed: pair, stride, nq = 0", want_metrics_typed(F64, F32), mtyped, n, z, F64, 0, z, F32, d, k, ids, 0, None, ids, B, rec, rat)
        for b, q in ((F32, F32), (U8, U8), (F16, F32)):
            run(("metrics_typed: k, nq = 0", b, q), M_SHAPE, mtyped, n, z, b, 0, z, q, d, 1025, ids, B, None, ids, B, rec, rat)
            run(("metrics_typed: n, nq < 0", b, q), M_SHAPE, mtyped, 0, z, b, -1, z, q, d, k, ids, B, None, ids, B, rec, rat)
            run(("metrics_typed: nq = 0", b, q), GOOD, mtyped, n, z, b, 0, z, q, d, k, ids, B, None, ids, B, rec, rat)

        # ---- metrics at every k: ks null, nk, ks[j], unique / cand_ratio together, the metrics order at max(ks), nq's range, nq == 0 ----
        kvariants(("ks null, nk",), (E_NULL, "ks is null"), None, nk=0)
        kvariants(("nk = 0, ks[0]",), (E_ARG, "nk must be in [1, 64]: 0"), [0], nk=0)
        kvariants(("nk = 65, ks[0]",), (E_ARG, "nk must be in [1, 64]: 65"), [0] * 65)
        kvariants(("ks[1], unique alone",), (E_ARG, "ks[1] = 0: k must be in [1, 1024]"), [2, 0], cand=None)
        kvariants(("ks[0] = 1025, null",), (E_ARG, "ks[0] = 1025: k must be in [1, 1024]"), [1025, 1], base=None)
        kvariants(("unique alone, null",), KV_PAIR, [2, 1], cand=None, base=None)
        kvariants(("cand_ratio alone, pair",), KV_PAIR, [2, 1], unique=None, b=F64)
        kvariants(("null, pair",), M_NULL, [2, 1], base=None, b=F64)
        kvariants(("pair, gt_stride < max(ks)",), want_metrics_typed(F16, F16), [1, 4], b=F16, q=F16, gt_stride=3)
        kvariants(("gt_stride < max(ks), nq < 0",), M_SHAPE, [1, 4, 2], gt_stride=3, nq_=-1)
        kvariants(("ann_stride, nq = 0",), M_SHAPE, [2, 1], ann_stride=0, nq_=0)
        kvariants(("n, nq > INT32_MAX",), M_SHAPE, [2, 1], n_=0, nq_=1 << 31)
        kvariants(("nq < 0",), KV_NQ, [2, 1], nq_=-1)
        kvariants(("nq > INT32_MAX",), KV_NQ, [2, 1], nq_=1 << 31)
        kvariants(("nq = 0",), GOOD, [2, 1], nq_=0)
        kvariants(("gt_stride = max(ks)",), GOOD, [1, 4, 2])
        kvariants(("no unique, no cand_ratio",), GOOD, [2, 1], unique=None, cand=None)

        # ---- the calls over the resident store ----------------------------------------------------------------------------------------
        gt_store, nn1_store, val_store = L.fspann_groundtruth_store_dev, L.fspann_nn1_exact_store_dev, L.fspann_gt_validate_store_dev

        def store_calls(state, gt_first, nn1_first):
            """each call with two wrong arguments: the ground truth asks for its buffers first, the two others for the store first"""
            run(("groundtruth_store_dev: null", state), GT_NULL, gt_store, nq, None, k, oi, od)
            run(("groundtruth_store_dev: k", state), gt_first, gt_store, nq, z, 0, oi, od)
            run(("nn1_exact_store_dev: null, q_dtype", state), nn1_first, nn1_store, nq, None, U8, None, nq, oi, od)
            run(("gt_validate_store_dev: null, q_dtype", state), nn1_first, val_store, nq, None, U8, ids, nq, B, 2, 0.0, C.byref(val))

        store_calls("no store", NO_STORE, NO_STORE)
        run("gt_validate_store_dev: no store, out", NO_STORE, val_store, nq, z, F32, ids, nq, B, 2, 0.0, None)
        X = np.zeros((n, d), np.float32)
        run("store_set F32", GOOD, L.fspann_store_set, n, _hp(X), F32)
        store_calls("F32 store", GT_K, NN1_NULL)
        run("gt_validate_store_dev: out", (E_NULL, "out is null"), val_store, nq, z, F32, ids, nq, B, 2, 0.0, None)
        run("nn1_exact_store_dev: q_dtype", want_nn1(F32, U8), nn1_store, nq, z, U8, None, nq, oi, od)
        run("groundtruth_store_dev", GOOD, gt_store, nq, z, k, oi, od)
        run("groundtruth_store_dev: nq = 0", GOOD, gt_store, 0, z, k, oi, od)
        run("nn1_exact_store_dev", GOOD, nn1_store, nq, z, F64, None, nq, oi, od)
        run("gt_validate_store_dev", GOOD, val_store, nq, z, F32, ids, nq, B, 2, 0.0, C.byref(val))
        # an fp64 copy of the four rows, last: the F64 store is refused behind the ground truth's buffers and in front of everything else
        X64 = X.astype(np.float64)
        run("store_set F64", GOOD, L.fspann_store_set, n, _hp(X64), F64)
        store_calls("F64 store", GT_NO_F64_STORE, NN1_NO_F64_STORE)
        run("gt_validate_store_dev: F64 store, out", NN1_NO_F64_STORE, val_store, nq, z, F32, ids, nq, B, 2, 0.0, None)
        run("groundtruth_store_dev: F64 store", GT_NO_F64_STORE, gt_store, nq, z, k, oi, od)
        run("nn1_exact_store_dev: F64 store", NN1_NO_F64_STORE, nn1_store, nq, z, F64, None, nq, oi, od)
        run("gt_validate_store_dev: F64 store", NN1_NO_F64_STORE, val_store, nq, z, F32, ids, nq, B, 2, 0.0, C.byref(val))
