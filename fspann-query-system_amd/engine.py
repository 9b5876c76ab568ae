"""FspannContext — numpy-facing wrapper of one `fspann_ctx` (one GPU, one HIP stream).

Batch-first: every call takes nq >= 1 queries.  Host arrays go through the
host-pointer entry points of include/fspann.h; `*_dev` methods take raw device
pointers (ints, e.g. torch.Tensor.data_ptr()) and only enqueue work on the
context's stream.  Product code — never imports oracle/.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _native as N


@dataclass
class PaperRuntimeConfig:
    """The nine knobs the path reads (config/SystemConfig.java:237-338)."""
    tables: int = 6
    divisions: int = 3
    m: int = 24
    lambda_: int = 2
    dim: int = 128
    seed: int = 13
    refinement_limit: int = 20000
    max_global_candidates: int = 20000
    probe_override: int = -1
    hamming_prefilter_threshold: int = 0
    block_size: int = 64
    default_probes: int = 5

    def to_c(self) -> N.Cfg:
        return N.Cfg(self.tables, self.divisions, self.m, self.lambda_, self.dim, self.block_size,
                     self.default_probes, self.probe_override, self.max_global_candidates,
                     self.refinement_limit, self.hamming_prefilter_threshold, 0)


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Bfloat16:
    """Marker for bfloat16 rows (FSPANN_BF16), passed as dtype= where numpy has no dtype to name: `pkg.bfloat16`."""
    __slots__ = ()

    def __repr__(self):
        return "bfloat16"


bfloat16 = _Bfloat16()


def _bf16_bits(x, what):
    """The uint16 bit patterns of rows handed over as bfloat16: a CPU torch.bfloat16 tensor as it is, a uint16 array as bit patterns,
    a float array only if every value already is a bfloat16 (exact in fp32 with the low 16 bits of the pattern zero; NaN counts as
    NaN).  The library never rounds for the caller."""
    if type(x).__module__.split(".")[0] == "torch":
        import torch
        if x.dtype != torch.bfloat16:
            raise N.FspannArgumentError(f"{what}(dtype=bfloat16): a torch tensor must be torch.bfloat16, not {x.dtype}")
        if x.device.type != "cpu":
            raise N.FspannArgumentError(f"{what}(dtype=bfloat16): the tensor must be on the CPU (device rows: store_attach_dev)")
        return np.ascontiguousarray(x.contiguous().view(torch.int16).numpy()).view(np.uint16)
    v = np.ascontiguousarray(x)
    if v.dtype == np.uint16:
        return v
    if v.dtype.kind != "f":
        raise N.FspannArgumentError(f"{what}(dtype=bfloat16): rows are a torch.bfloat16 tensor, uint16 bit patterns or a float array, not {v.dtype}")
    with np.errstate(over="ignore", invalid="ignore"):
        f = v.astype(np.float32)
        back = f.astype(v.dtype)
        bits = f.view(np.uint32)
        nan = v != v
        exact = bool(np.all(((back == v) & ((bits & 0xFFFF) == 0)) | nan))
    if not exact:
        raise N.FspannArgumentError(f"{what}(dtype=bfloat16): every value must be exactly representable as a bfloat16 "
                                    "(round the data yourself: the library never does)")
    hi = (bits >> 16).astype(np.uint16)
    hi[nan & ((hi & 0x7F) == 0)] |= 0x40       # a NaN whose payload sat in the low bits only stays a NaN
    return hi


class _Float8E4M3:
    """Marker for OCP fp8 e4m3fn rows (FSPANN_F8E4M3), passed as dtype= where numpy has no dtype to name: `pkg.float8_e4m3fn`."""
    __slots__ = ()

    def __repr__(self):
        return "float8_e4m3fn"


float8_e4m3fn = _Float8E4M3()


def _f8_bits(x, what):
    """The uint8 bit patterns of rows handed over as fp8 e4m3fn (S EEEE MMM, bias 7, no infinity, 0x7F / 0xFF NaN): a CPU
    torch.float8_e4m3fn tensor as it is, a uint8 array as bit patterns, a float array only if every value already is an e4m3 value
    (a multiple of 2^-9 with at most four significant bits and magnitude <= 448; NaN becomes 0x7F, -0.0 keeps its sign, +-inf is
    refused: the format has none).  The library never rounds for the caller."""
    if type(x).__module__.split(".")[0] == "torch":
        import torch
        if x.dtype != torch.float8_e4m3fn:
            raise N.FspannArgumentError(f"{what}(dtype=float8_e4m3fn): a torch tensor must be torch.float8_e4m3fn, not {x.dtype}")
        if x.device.type != "cpu":
            raise N.FspannArgumentError(f"{what}(dtype=float8_e4m3fn): the tensor must be on the CPU (device rows: store_attach_dev)")
        return np.ascontiguousarray(x.contiguous().view(torch.uint8).numpy())
    v = np.ascontiguousarray(x)
    if v.dtype == np.uint8:
        return v
    if v.dtype.kind != "f":
        raise N.FspannArgumentError(f"{what}(dtype=float8_e4m3fn): rows are a torch.float8_e4m3fn tensor, uint8 bit patterns or a float array, not {v.dtype}")
    with np.errstate(over="ignore", invalid="ignore"):
        f = v.astype(np.float64)                # (exact from every float type)
        nan = f != f
        a = np.where(nan, 0.0, np.abs(f))
        m, e = np.frexp(a)                      # a = m * 2^e, m in [0.5, 1) (0 for a = 0)
        exact = bool(np.all((a <= 448.0) & (a * 512.0 == np.floor(a * 512.0)) & (m * 16.0 == np.floor(m * 16.0))))
    if not exact:
        raise N.FspannArgumentError(f"{what}(dtype=float8_e4m3fn): every value must be exactly representable as an fp8 e4m3fn "
                                    "(round the data yourself: the library never does)")
    sub = a < 2.0 ** -6                         # subnormals and zero: M / 8 * 2^-6
    bits = np.where(sub, a * 512.0, (e + 6) * 8 + (m * 16.0 - 8.0)).astype(np.uint8)
    bits |= (np.signbit(f) & ~nan).astype(np.uint8) << 7
    bits[nan] = 0x7F
    return bits


def _i8_rows(x, what):
    """Rows handed over as signed bytes (FSPANN_I8): an int8 array as it is, any other array only if every value is an integer in
    -128..127 (NaN and +-inf are not).  No scale and no zero point: the library never quantises for the caller."""
    v = np.ascontiguousarray(x)
    if v.dtype == np.int8:
        return v
    with np.errstate(invalid="ignore"):
        exact = v.dtype.kind in "biuf" and bool(np.all((v >= -128) & (v <= 127) & (v == np.floor(v))))
    if not exact:
        raise N.FspannArgumentError(f"{what}(dtype=int8): every value must be an integer in -128..127")
    return v.astype(np.int8)


def _dt(a):
    if a.dtype == np.float32:
        return N.F32
    if a.dtype == np.float64:
        return N.F64
    if a.dtype == np.uint8:     # rows only (FSPANN_U8): the library refuses it wherever a query dtype is given
        return N.U8
    if a.dtype == np.float16:   # rows only (FSPANN_F16): refused likewise
        return N.F16
    raise N.FspannArgumentError(f"unsupported dtype {a.dtype}")


def _row_dt(a):
    """_dt for ROWS (store, Setup input, ground-truth pairs): an int8 array is FSPANN_I8 there.  _dt itself, which types queries
    too, keeps refusing signed bytes."""
    if a.dtype == np.int8:
        return N.I8
    return _dt(a)


def _typed_rows(vectors, dtype, what):
    """Rows as store_set takes them (its docstring says what each dtype= accepts; `what` names the caller in the messages): the
    contiguous array to hand over, its FSPANN_* code, and what store_dtype reports for it."""
    if dtype is float8_e4m3fn:
        return _f8_bits(vectors, what), N.F8E4M3, float8_e4m3fn
    if dtype is bfloat16:
        return _bf16_bits(vectors, what), N.BF16, bfloat16
    v = np.ascontiguousarray(vectors)
    if dtype is not None and np.dtype(dtype) == np.uint8:
        if v.dtype != np.uint8:
            with np.errstate(invalid="ignore"):
                exact = bool(np.all((v >= 0) & (v <= 255) & (v == np.floor(v))))
            if not exact:
                raise N.FspannArgumentError(f"{what}(dtype=uint8): every value must be an integer in 0..255")
            v = v.astype(np.uint8)
    elif dtype is not None and np.dtype(dtype) == np.int8:
        v = _i8_rows(v, what)
    elif dtype is not None and np.dtype(dtype) == np.float16:
        if v.dtype != np.float16:
            with np.errstate(over="ignore", invalid="ignore"):
                h = v.astype(np.float16)
                back = h.astype(v.dtype)
                exact = bool(np.all((back == v) | ((back != back) & (v != v))))
            if not exact:
                raise N.FspannArgumentError(f"{what}(dtype=float16): every value must be exactly representable as an IEEE half "
                                            "(round the data yourself: the library never does)")
            v = h
    elif dtype is not None:
        v = v.astype(np.dtype(dtype))
        if v.dtype not in (np.float32, np.float64):
            raise N.FspannArgumentError(f"unsupported dtype {v.dtype}")
    elif v.dtype not in (np.float32, np.float64):
        v = v.astype(np.float64)
    return v, _row_dt(v), v.dtype


def coverage_grid(tables, divisions, probes):
    """every (tables, divisions, probes) of the three sequences, as route_coverage's grid [nc][3] (the last varies fastest)"""
    return np.array([(t, d, p) for t in tables for d in divisions for p in probes], np.int32).reshape(-1, 3)


class FspannContext:
    def __init__(self, cfg: PaperRuntimeConfig, device: int = 0):
        self.cfg = cfg
        self.L = N.lib()
        h = C.c_void_p()
        cc = cfg.to_c()
        N.check(self.L.fspann_ctx_create(device, C.byref(cc), C.byref(h)))
        self._h = h
        self.TD = cfg.tables * cfg.divisions
        self.bits = cfg.m * cfg.lambda_
        self.W = (self.bits + 63) // 64
        self.hard_cap = max(cfg.max_global_candidates, cfg.refinement_limit)
        self.device = device
        self._store_n = 0            # rows of the resident store (store_set / store_attach_dev; a clone takes its parent's)

    # -- lifecycle -----------------------------------------------------------
    def clone(self) -> "FspannContext":
        """A context on the same device that reads THIS context's GFunctions, frozen index, id metadata and store in place
        (fspann_ctx_clone) and owns its stream and work areas: one index in HBM served from several streams."""
        other = FspannContext.__new__(FspannContext)
        other.cfg, other.L = self.cfg, self.L
        h = C.c_void_p()
        N.check(self.L.fspann_ctx_clone(self._h, C.byref(h)))
        other._h = h
        other.TD, other.bits, other.W, other.hard_cap, other.device = self.TD, self.bits, self.W, self.hard_cap, self.device
        # the clone reads this context's store in place: what this object knows about it goes along (the library refuses to change
        # a store while clones are alive, so the two cannot drift)
        other._store_n = self._store_n
        if hasattr(self, "store_dtype"):
            other.store_dtype = self.store_dtype
        return other

    def close(self):
        if getattr(self, "_h", None):
            self.L.fspann_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return int(self.L.fspann_ctx_stream(self._h) or 0)

    def sync(self):
        N.check(self.L.fspann_sync(self._h))

    # -- Setup ---------------------------------------------------------------
    def set_gfunctions(self, alpha, r, omega):
        c = self.cfg
        a = _c(alpha, np.float64).reshape(self.TD, c.m, c.dim)
        rr = _c(r, np.float64).reshape(self.TD, c.m)
        ww = _c(omega, np.float64).reshape(self.TD, c.m)
        N.check(self.L.fspann_set_gfunctions(self._h, _p(a), _p(rr), _p(ww)))

    def registry_initialize(self, sample, base_seed=None):
        s = _c(sample, np.float64).reshape(-1, self.cfg.dim)
        seed = self.cfg.seed if base_seed is None else base_seed
        N.check(self.L.fspann_registry_initialize(self._h, _p(s), s.shape[0], seed))

    def get_gfunctions(self):
        c = self.cfg
        a = np.empty((self.TD, c.m, c.dim), np.float64)
        r = np.empty((self.TD, c.m), np.float64)
        w = np.empty((self.TD, c.m), np.float64)
        N.check(self.L.fspann_get_gfunctions(self._h, _p(a), _p(r), _p(w)))
        return a, r, w

    def set_id_meta(self, n_ids, java_hash=None, deleted=None):
        jh = None if java_hash is None else _c(java_hash, np.int32)
        dl = None if deleted is None else _c(deleted, np.uint8)
        N.check(self.L.fspann_set_id_meta(self._h, n_ids, _p(jh), _p(dl)))
        self.n_ids = n_ids

    def set_index(self, td, min_key, max_key, rep, id_off, ids):
        mn, mx = _c(min_key, np.int64), _c(max_key, np.int64)
        rp, of, ii = _c(rep, np.uint64), _c(id_off, np.int64), _c(ids, np.int32)
        N.check(self.L.fspann_set_index(self._h, td, len(mn), _p(mn), _p(mx), _p(rp), _p(of), _p(ii)))

    def finalize(self):
        N.check(self.L.fspann_finalize(self._h))

    def build_index(self, vectors, order=None, dtype=None):
        """A uint8 array goes to the library as bytes (FSPANN_U8: widened on the device; same tables, a quarter of the traffic),
        an int8 array as signed bytes (FSPANN_I8: likewise), a float16 array as halves (FSPANN_F16: same tables, half the traffic).  dtype=bfloat16 (the package's marker): the rows
        go up as bfloat16 bit patterns (FSPANN_BF16; a torch.bfloat16 tensor, uint16 patterns, or floats that already are
        bfloat16 values, as in store_set): same tables, half the traffic.  dtype=float8_e4m3fn likewise (FSPANN_F8E4M3; a
        torch.float8_e4m3fn tensor, uint8 patterns, or floats that already are e4m3 values): same tables, a quarter of the traffic."""
        if dtype is bfloat16:
            v = _bf16_bits(vectors, "build_index").reshape(-1, self.cfg.dim)
            o = None if order is None else _c(order, np.int32)
            N.check(self.L.fspann_build_index(self._h, v.shape[0], _p(v), N.BF16, _p(o)))
            return
        if dtype is float8_e4m3fn:
            v = _f8_bits(vectors, "build_index").reshape(-1, self.cfg.dim)
            o = None if order is None else _c(order, np.int32)
            N.check(self.L.fspann_build_index(self._h, v.shape[0], _p(v), N.F8E4M3, _p(o)))
            return
        if dtype is not None:
            raise N.FspannArgumentError("build_index(dtype=): only the bfloat16 and float8_e4m3fn markers are given by name; other rows are typed by their array")
        v = np.ascontiguousarray(vectors)
        if v.dtype not in (np.float32, np.float64, np.uint8, np.int8, np.float16):
            v = v.astype(np.float64)
        v = v.reshape(-1, self.cfg.dim)
        o = None if order is None else _c(order, np.int32)
        N.check(self.L.fspann_build_index(self._h, v.shape[0], _p(v), _row_dt(v), _p(o)))

    def build_begin(self, n_total: int):
        """Incremental Setup: begin(n) -> append(rows of the next handles) ... -> finish(order) (fspann_build_begin / _append / _finish)."""
        N.check(self.L.fspann_build_begin(self._h, int(n_total)))

    def build_append(self, rows, dtype=None):
        if dtype is bfloat16:
            v = _bf16_bits(rows, "build_append").reshape(-1, self.cfg.dim)
            N.check(self.L.fspann_build_append(self._h, v.shape[0], _p(v), N.BF16))
            return
        if dtype is float8_e4m3fn:
            v = _f8_bits(rows, "build_append").reshape(-1, self.cfg.dim)
            N.check(self.L.fspann_build_append(self._h, v.shape[0], _p(v), N.F8E4M3))
            return
        if dtype is not None:
            raise N.FspannArgumentError("build_append(dtype=): only the bfloat16 and float8_e4m3fn markers are given by name; other rows are typed by their array")
        v = np.ascontiguousarray(rows)
        if v.dtype not in (np.float32, np.float64, np.uint8, np.int8, np.float16):
            v = v.astype(np.float64)
        v = v.reshape(-1, self.cfg.dim)
        N.check(self.L.fspann_build_append(self._h, v.shape[0], _p(v), _row_dt(v)))

    def build_finish(self, order=None):
        o = None if order is None else _c(order, np.int32)
        N.check(self.L.fspann_build_finish(self._h, _p(o)))

    def set_deleted(self, handles, flag=True):
        """Live mirror of metadata.isDeleted (PIS:739): no un-freeze, works on the owner or any clone while they serve queries."""
        h = _c(handles, np.int32).reshape(-1)
        N.check(self.L.fspann_set_deleted(self._h, _p(h), len(h), 1 if flag else 0))

    def save_index(self, path: str):
        N.check(self.L.fspann_index_save(self._h, os.fsencode(path)))

    def load_index(self, path: str):
        N.check(self.L.fspann_index_load(self._h, os.fsencode(path)))

    def get_index(self, td):
        npart, nid = C.c_int64(), C.c_int64()
        N.check(self.L.fspann_index_dims(self._h, td, C.byref(npart), C.byref(nid)))
        mn = np.empty(npart.value, np.int64)
        mx = np.empty(npart.value, np.int64)
        rep = np.empty((npart.value, self.W), np.uint64)
        off = np.empty(npart.value + 1, np.int64)
        ids = np.empty(nid.value, np.int32)
        N.check(self.L.fspann_get_index(self._h, td, _p(mn), _p(mx), _p(rep), _p(off), _p(ids)))
        return dict(min_key=mn, max_key=mx, rep=rep, id_off=off, ids=ids)

    # -- TokenGen ----------------------------------------------------------------
    def encode(self, q, want_hashes=False):
        if q is None:
            raise N.FspannNullError("query vector is null")
        q = np.ascontiguousarray(q)
        if q.dtype not in (np.float32, np.float64):
            q = q.astype(np.float64)
        if q.size % self.cfg.dim != 0:
            raise N.FspannArgumentError(f"Expected vector length {self.cfg.dim}")
        q = q.reshape(-1, self.cfg.dim)
        nq = q.shape[0]
        codes = np.zeros((nq, self.TD, self.W), np.uint64)
        hs = np.zeros((nq, self.TD, self.cfg.m), np.int32) if want_hashes else None
        N.check(self.L.fspann_encode(self._h, nq, _p(q), _dt(q), _p(codes), _p(hs)))
        return (codes, hs) if want_hashes else codes

    def set_encode_mode(self, mode: int):
        """0 auto, 1 exact fp64, 2 MFMA fp32 + exact re-check (all bit-identical)."""
        N.check(self.L.fspann_set_encode_mode(self._h, mode))

    def last_encode_rechecked(self) -> int:
        return int(self.L.fspann_last_encode_rechecked(self._h))

    # -- Route ---------------------------------------------------------------------
    def effective_probes(self, probe_override=-1):
        return self.L.fspann_effective_probes(self._h, probe_override)

    def set_route_mode(self, mode):
        """0 auto, 1 full select only, 2 bounded select whenever legal (identical results)."""
        N.check(self.L.fspann_set_route_mode(self._h, int(mode)))

    def last_route_info(self):
        import ctypes as C
        lazy, ovf = C.c_int(0), C.c_int(0)
        N.check(self.L.fspann_last_route_info(self._h, C.byref(lazy), C.byref(ovf)))
        return dict(lazy=bool(lazy.value), overflowed=int(ovf.value))

    def unmodelled_queries(self, reset=True) -> int:
        """Queries flagged 'HashMap bin treeified' (count = -1) by Route calls since the last reset."""
        v = C.c_int64(0)
        N.check(self.L.fspann_unmodelled_queries(self._h, C.byref(v), 1 if reset else 0))
        return int(v.value)

    # -- touched records (selective re-encryption) ---------------------------------------------------
    def touch_enable(self, on=True):
        """Start (or stop) marking the records every Refine of this index family scores (fspann_touch_enable); the set
        belongs to the index owner and is shared by its clones."""
        N.check(self.L.fspann_touch_enable(self._h, 1 if on else 0))

    def touched_count(self) -> int:
        """ReencryptionTracker.uniqueCount(): touched handles (synchronises this context's stream)."""
        v = C.c_int64(0)
        N.check(self.L.fspann_touch_count(self._h, C.byref(v)))
        return int(v.value)

    def drain_touched(self, reset=True, cap=None) -> np.ndarray:
        """ReencryptionTracker.drainTouchedIds(): the touched handles, ascending (int32).  cap bounds how many are returned (the
        smallest); reset clears exactly those returned.  cap None: all of them, sized from a count."""
        if cap is None:
            cap = self.touched_count()
        out = np.empty(max(int(cap), 1), np.int32)
        n = C.c_int64(0)
        N.check(self.L.fspann_touch_drain(self._h, out.ctypes.data_as(C.c_void_p), int(cap), C.byref(n), 1 if reset else 0))
        return out[:min(int(cap), int(n.value))].copy()

    def route_max_candidates(self, probe_override=-1):
        return int(self.L.fspann_route_max_candidates(self._h, probe_override))

    ROUTE_PLAN_FIELDS = ("ht_size", "lds_sort_words", "sort_cap", "lds_mode", "threads", "max_tuples", "maxcand", "nbins", "cap0",
                         "slice_ht", "lazy", "g_sub", "seq_bits", "wave_sort", "lazy_cap", "probes")

    def route_plan_info(self, probe_override=-1, limit=N.INT32_MAX, counters=True):
        """Diagnostics: the plan route(..., probe_override, limit, counters) would run with, as a dict (fspann_route_plan_info;
        host only, nothing is launched)."""
        out = np.zeros(len(self.ROUTE_PLAN_FIELDS), np.int32)
        rc = self.L.fspann_route_plan_info(self._h, probe_override, min(limit, N.INT32_MAX), 1 if counters else 0, _p(out), len(out))
        if rc < 0:
            N.check(rc)
        assert rc == len(out), rc
        return {k: int(v) for k, v in zip(self.ROUTE_PLAN_FIELDS, out)}

    def route(self, codes, probe_override=-1, limit=N.INT32_MAX, cap=None, counters=True, allow_unmodelled=False):
        """allow_unmodelled: return the per-query flags (count = -1: a HashMap bin would be treeified, the JVM's order
        is not modelled) instead of raising FspannStateError for the whole batch."""
        if codes is None:
            raise N.FspannStateError("MSANNP violation: QueryToken missing BitSet codes")
        codes = _c(codes, np.uint64).reshape(-1, self.TD, self.W)
        nq = codes.shape[0]
        if cap is None:
            cap = max(1, min(limit, self.route_max_candidates(probe_override)))
        ids = np.full((nq, cap), -1, np.int32)
        score = np.full((nq, cap), -1, np.int32)
        count = np.zeros(nq, np.int32)
        kept = np.zeros(nq, np.int32)
        raw = np.zeros(nq, np.int32)
        rc = self.L.fspann_route(self._h, nq, _p(codes), probe_override, min(limit, N.INT32_MAX), cap, _p(ids),
                                 _p(score), _p(count), _p(kept) if counters else None, _p(raw) if counters else None)
        if not (allow_unmodelled and rc == N.E_STATE and (count < 0).any()):   # outputs are complete in that case
            N.check(rc)
        if not counters:   # lastCandKept / rawSeen not requested: the bounded select may run
            return dict(ids=ids, score=score, count=count)
        return dict(ids=ids, score=score, count=count, kept=kept, raw_seen=raw)

    def route_flags(self, codes, probe_override=-1):
        """Diagnostics: which queries the full select FLAGS (count = -1: a HashMap bin of bestScore would be treeified) before the
        host model finishes them — fspann_route_dev with the counters requested (exact detection), nothing resolved."""
        codes = _c(codes, np.uint64).reshape(-1, self.TD, self.W)
        nq = codes.shape[0]
        cap = max(1, self.route_max_candidates(probe_override))
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            N.check(self.L.fspann_dev_alloc(self._h, nbytes, C.byref(p)))
            bufs.append(p)
            return p
        try:
            d_codes, d_ids, d_cnt, d_kept = dev(codes.nbytes), dev(nq * cap * 4), dev(nq * 4), dev(nq * 4)
            N.check(self.L.fspann_h2d(self._h, d_codes, _p(codes), codes.nbytes))
            N.check(self.L.fspann_route_dev(self._h, nq, d_codes, probe_override, N.INT32_MAX, cap, d_ids, None, d_cnt, d_kept, None))
            count = np.zeros(nq, np.int32)
            N.check(self.L.fspann_d2h(self._h, _p(count), d_cnt, nq * 4))
            self.unmodelled_queries(reset=True)
        finally:
            for p in bufs:
                self.L.fspann_dev_free(self._h, p)
        return count < 0

    def route_flags_bounded(self, codes, limit, probe_override=-1):
        """Diagnostics: which queries end FLAGGED (count = -1) when fspann_route_dev runs the way stage A.5 calls it — first
        `limit` entries, no counters, so the bounded select runs where it is legal and hands over what it cannot hold or what
        its exact treeify check catches; the full select then flags a treeified bestScore map.  Nothing is resolved."""
        codes = _c(codes, np.uint64).reshape(-1, self.TD, self.W)
        nq = codes.shape[0]
        bufs = []

        def dev(nbytes):
            p = C.c_void_p()
            N.check(self.L.fspann_dev_alloc(self._h, nbytes, C.byref(p)))
            bufs.append(p)
            return p
        try:
            d_codes, d_ids, d_cnt = dev(codes.nbytes), dev(nq * limit * 4), dev(nq * 4)
            N.check(self.L.fspann_h2d(self._h, d_codes, _p(codes), codes.nbytes))
            N.check(self.L.fspann_route_dev(self._h, nq, d_codes, probe_override, limit, limit, d_ids, None, d_cnt, None, None))
            count = np.zeros(nq, np.int32)
            N.check(self.L.fspann_d2h(self._h, _p(count), d_cnt, nq * 4))
            self.unmodelled_queries(reset=True)
        finally:
            for p in bufs:
                self.L.fspann_dev_free(self._h, p)
        return count < 0

    # -- Refine ----------------------------------------------------------------------
    def refine(self, q, cand, cand_ids, cand_count, k):
        cand = np.ascontiguousarray(cand)
        if cand.dtype not in (np.float32, np.float64):
            cand = cand.astype(np.float64)
        nq, B, d = cand.shape
        q = _c(q, cand.dtype).reshape(nq, d)
        ci = _c(cand_ids, np.int32).reshape(nq, B)
        cc = _c(cand_count, np.int32).reshape(nq)
        out_ids = np.empty((nq, k), np.int32)
        out_dist = np.empty((nq, k), np.float64)
        out_count = np.empty(nq, np.int32)
        scored = np.empty(nq, np.int32)
        N.check(self.L.fspann_refine(self._h, nq, _p(q), _p(cand), _dt(cand), B, _p(ci), _p(cc), k, _p(out_ids),
                                     _p(out_dist), _p(out_count), _p(scored)))
        return dict(ids=out_ids, dist=out_dist, count=out_count, scored=scored)

    def host_buffer(self, shape, dtype=np.float64):
        """A numpy view of the context's PINNED host block (fspann_host_buffer), at least as large as `shape` x `dtype`: what the adapter
        packs decrypted candidate rows into (QSI:238-271) — rows handed to refine() from here travel by plain DMA.  The view dies with the
        next larger request or with the context."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.L.fspann_host_buffer(self._h, max(n, 16))
        if not p:
            raise MemoryError(self.L.fspann_last_error().decode())
        return np.frombuffer((C.c_char * n).from_address(p), dtype=dtype).reshape(shape)

    def refine_store(self, q, cand_ids, cand_count, k):
        """Refine with rows read from the resident store by id (no staging copy)."""
        ci = _c(cand_ids, np.int32)
        nq, B = ci.shape
        q = np.ascontiguousarray(q)
        if q.dtype not in (np.float32, np.float64):
            q = q.astype(np.float64)
        q = q.reshape(nq, self.cfg.dim)
        cc = _c(cand_count, np.int32).reshape(nq)
        out_ids = np.empty((nq, k), np.int32)
        out_dist = np.empty((nq, k), np.float64)
        out_count = np.empty(nq, np.int32)
        scored = np.empty(nq, np.int32)
        N.check(self.L.fspann_refine_store(self._h, nq, _p(q), _dt(q), B, _p(ci), _p(cc), k, _p(out_ids),
                                           _p(out_dist), _p(out_count), _p(scored)))
        return dict(ids=out_ids, dist=out_dist, count=out_count, scored=scored)

    # -- plaintext store (test / bench harness) --------------------------------------
    def store_set(self, vectors, dtype=None):
        """dtype=np.uint8 keeps the rows as bytes (FSPANN_U8): only for data whose values are the integers 0..255 (a uint8
        array, or an array holding nothing else), where a byte is exactly what the reference's double[] holds.  Without it a
        uint8 array is widened to float64 like every other non-float array.
        dtype=np.int8 keeps the rows as signed bytes (FSPANN_I8): an int8 array as it is, any other array only if every value is an
        integer in -128..127 (no scale, no zero point: the library never quantises for the caller).  Without it an int8 array
        is widened to float64 as well.
        dtype=np.float16 keeps the rows as halves (FSPANN_F16): a float16 array as it is, any other array only if every value
        already is a half (it survives astype(float16) and back unchanged, NaN counting as NaN) — the library never rounds for
        the caller.  Without it a float16 array is widened to float64 as well.
        dtype=bfloat16 (the package's marker; numpy has no such dtype) keeps the rows as bfloat16 (FSPANN_BF16): a CPU
        torch.bfloat16 tensor as it is, a uint16 array as bit patterns, a float array only if every value already is a bfloat16
        (exact in fp32 with the low 16 bits of the pattern zero, NaN counting as NaN).  store_dtype then reports the marker.
        dtype=float8_e4m3fn (the package's marker) keeps the rows as OCP fp8 e4m3fn (FSPANN_F8E4M3): a CPU torch.float8_e4m3fn
        tensor as it is, a uint8 array as bit patterns, a float array only if every value already is an e4m3 value (NaN becomes
        0x7F; +-inf is refused, the format has none).  store_dtype then reports the marker."""
        v, code, kept = _typed_rows(vectors, dtype, "store_set")                # (raises before the store is touched)
        v = v.reshape(-1, self.cfg.dim)
        N.check(self.L.fspann_store_set(self._h, v.shape[0], _p(v), code))
        self.store_dtype = kept
        self._store_n = v.shape[0]

    def store_attach_dev(self, n, ptr, dtype):
        """Use caller-owned device rows [n][dim] as the store (no copy; keep them alive).  dtype: N.F32, N.F64, N.U8, N.F16, N.BF16, N.F8E4M3 or N.I8."""
        N.check(self.L.fspann_store_attach_dev(self._h, int(n), ptr, dtype))
        self._store_n = int(n)

    # -- lossless narrowing on the device (include/fspann_narrow.h) -----------------------
    @staticmethod
    def _allowed(allowed):
        """`allowed` of the narrowing calls as the C mask: None = every type, an int as it is, else an iterable of FSPANN_* codes"""
        if allowed is None:
            return 0
        if isinstance(allowed, (int, np.integer)):
            return int(allowed)
        return sum({1 << int(t) for t in allowed})

    @staticmethod
    def _kept(code):
        """what store_dtype reports for an FSPANN_* code: the numpy dtype, or the package's marker where numpy has none"""
        return {N.F32: np.dtype(np.float32), N.F64: np.dtype(np.float64), N.U8: np.dtype(np.uint8), N.I8: np.dtype(np.int8),
                N.F16: np.dtype(np.float16), N.BF16: bfloat16, N.F8E4M3: float8_e4m3fn}[code]

    @staticmethod
    def _fit_dict(f):
        return dict(fits=int(f.fits), narrowest=int(f.narrowest), first_misfit=np.array(f.first_misfit[:7], np.int64), nonfinite=int(f.nonfinite))

    def rows_fit_dev(self, n, rows_ptr, dtype, dim, allowed=0, row_fits_ptr=0) -> N.Fit:
        f = N.Fit()
        N.check(self.L.fspann_rows_fit_dev(self._h, n, rows_ptr, dtype, dim, allowed, row_fits_ptr or None, C.byref(f)))
        return f

    def rows_narrow_dev(self, n, src_ptr, src_dtype, dim, dst_ptr, dst_dtype) -> None:
        """src [n][dim] re-packed as the narrower dst_dtype, both in device memory; FspannArgumentError when an element is not a value of it"""
        N.check(self.L.fspann_rows_narrow_dev(self._h, n, src_ptr, src_dtype, dim, dst_ptr, dst_dtype, None))

    def rows_fit(self, rows, allowed=None):
        """Which row types hold the fp32 or fp64 array rows [n][dim] exactly, decided on the device: dict(fits = mask of
        1 << FSPANN_x, narrowest = the FSPANN_* code the order of include/fspann_narrow.h picks among fits & allowed, first_misfit
        [7] = per code the flat index of the first element that is not a value of it or -1, nonfinite, row_fits [n] = the mask per row)."""
        v = np.ascontiguousarray(rows)
        if v.dtype not in (np.float32, np.float64):
            v = v.astype(np.float64)
        if v.ndim != 2:
            raise N.FspannArgumentError("rows_fit: rows are a 2-D array [n][dim]")
        with self._Dev(self) as dv:
            rf = dv.new(v.shape[0], np.uint8)
            f = self.rows_fit_dev(v.shape[0], dv.up(v), _dt(v), v.shape[1], self._allowed(allowed), rf)
            return dict(self._fit_dict(f), row_fits=dv.down(rf))

    def store_fit(self, allowed=None):
        """rows_fit over the resident store (no row mask)"""
        f = N.Fit()
        N.check(self.L.fspann_store_fit(self._h, self._allowed(allowed), C.byref(f)))
        return self._fit_dict(f)

    def store_narrow(self, allowed=None):
        """Re-pack the resident store, in HBM, as the narrowest allowed row type that holds every element exactly (nothing is ever
        rounded; when nothing narrower fits the store stays as it is).  Returns what store_dtype then reports: a numpy dtype, or the
        package's marker."""
        code = C.c_int(-1)
        N.check(self.L.fspann_store_narrow(self._h, self._allowed(allowed), C.byref(code)))
        self.store_dtype = self._kept(code.value)
        return self.store_dtype

    def store_set_narrowest(self, vectors, allowed=None):
        """store_set(vectors) as they are (fp32 or fp64), then store_narrow(allowed): the caller need not know what the data holds"""
        self.store_set(vectors)
        return self.store_narrow(allowed)

    def hbm_read_peak(self, nbytes=1 << 32, reps=5) -> float:
        """GB/s of a pure-load kernel over `nbytes` of HBM on this device (bench.py roofline.peak_measured)."""
        v = C.c_double(0.0)
        N.check(self.L.fspann_hbm_read_peak(self._h, int(nbytes), int(reps), C.byref(v)))
        return float(v.value)

    def hbm_read_window(self, nbytes=1 << 32, window=134823936, reps=20) -> float:
        """GB/s of the same pure-load kernel when one launch reads only `window` bytes of cold HBM (average over `reps`)."""
        v = C.c_double(0.0)
        N.check(self.L.fspann_hbm_read_window(self._h, int(nbytes), int(window), int(reps), C.byref(v)))
        return float(v.value)

    # -- device-pointer entry points (ints) ----------------------------------------------
    def encode_dev(self, nq, q_ptr, dtype, codes_ptr, hashes_ptr=0, bad_ptr=0):
        N.check(self.L.fspann_encode_dev(self._h, nq, q_ptr, dtype, codes_ptr, hashes_ptr or None, bad_ptr or None))

    def route_dev(self, nq, codes_ptr, probe_override, limit, cap, ids_ptr, score_ptr, count_ptr, kept_ptr, raw_ptr):
        N.check(self.L.fspann_route_dev(self._h, nq, codes_ptr, probe_override, limit, cap, ids_ptr, score_ptr or None,
                                        count_ptr, kept_ptr or None, raw_ptr or None))

    def route_resolve_dev(self, nq, codes_ptr, probe_override, limit, cap, ids_ptr, score_ptr, count_ptr, kept_ptr=0, raw_ptr=0) -> int:
        """Finish the queries an asynchronous Route call flagged (count -1: a HashMap bin treeified) with the host model; returns how many."""
        done = C.c_int64(0)
        N.check(self.L.fspann_route_resolve_dev(self._h, nq, codes_ptr, probe_override, limit, cap, ids_ptr, score_ptr or None, count_ptr,
                                                kept_ptr or None, raw_ptr or None, C.byref(done)))
        return int(done.value)

    def search_store_finish_dev(self, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr=0,
                                sel_ids_ptr=0, sel_count_ptr=0) -> int:
        """Completes the preceding search_store_dev call: flagged queries are finished on the host and the batch is scored again."""
        done = C.c_int64(0)
        N.check(self.L.fspann_search_store_finish_dev(self._h, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr, out_count_ptr,
                                                      scored_ptr or None, sel_ids_ptr or None, sel_count_ptr or None, C.byref(done)))
        return int(done.value)

    def store_gather_dev(self, nq, sel_ids_ptr, sel_count_ptr, B, cand_ptr):
        N.check(self.L.fspann_store_gather_dev(self._h, nq, sel_ids_ptr, sel_count_ptr, B, cand_ptr))

    def search_store_dev(self, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr=0,
                         sel_ids_ptr=0, sel_count_ptr=0, bad_ptr=0):
        """encode -> route(limit = B) -> refine from the resident store, one call (device pointers, stream order)."""
        N.check(self.L.fspann_search_store_dev(self._h, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr,
                                               out_count_ptr, scored_ptr or None, sel_ids_ptr or None, sel_count_ptr or None,
                                               bad_ptr or None))

    def search_retry_dev(self, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr=0,
                         sel_ids_ptr=0, sel_count_ptr=0, bad_ptr=0, retried_ptr=0):
        """search_store_dev plus QueryServiceImpl's adaptive retry (QSI:327-337): the short queries are searched again with 10
        probes on the device, in stream order; retried [nq] (optional) says which did."""
        N.check(self.L.fspann_search_retry_dev(self._h, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr,
                                               out_count_ptr, scored_ptr or None, sel_ids_ptr or None, sel_count_ptr or None,
                                               bad_ptr or None, retried_ptr or None))

    def search_retry_finish_dev(self, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr=0,
                                sel_ids_ptr=0, sel_count_ptr=0, bad_ptr=0, retried_ptr=0) -> int:
        """Completes the preceding search_retry_dev call (same arguments): queries Route flagged in either pass are finished on
        the host and scored, a short one flagged in pass 1 takes its pass 2.  Returns how many were finished on the host."""
        done = C.c_int64(0)
        N.check(self.L.fspann_search_retry_finish_dev(self._h, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr,
                                                      out_count_ptr, scored_ptr or None, sel_ids_ptr or None, sel_count_ptr or None,
                                                      bad_ptr or None, retried_ptr or None, C.byref(done)))
        return int(done.value)

    def search_fallback_dev(self, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr=0,
                            sel_ids_ptr=0, sel_count_ptr=0, bad_ptr=0, retried_ptr=0, fellback_ptr=0):
        """search_retry_dev plus ForwardSecureANNSystem.runQueries' empty-result fallback (FSA:667-678): the queries that returned
        nothing are searched again on the device, a whole QSI.search at max(2 * base probes, 4) probes, in stream order and in
        place; fellback [nq] (optional) says which were."""
        N.check(self.L.fspann_search_fallback_dev(self._h, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr,
                                                  out_count_ptr, scored_ptr or None, sel_ids_ptr or None, sel_count_ptr or None,
                                                  bad_ptr or None, retried_ptr or None, fellback_ptr or None))

    def search_fallback_finish_dev(self, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr=0,
                                   sel_ids_ptr=0, sel_count_ptr=0, bad_ptr=0, retried_ptr=0, fellback_ptr=0) -> int:
        """Completes the preceding search_fallback_dev call (same arguments): queries Route flagged in either search are finished on
        the host and scored, those of search 1 take their fallback when empty.  Returns how many were finished on the host."""
        done = C.c_int64(0)
        N.check(self.L.fspann_search_fallback_finish_dev(self._h, nq, q_ptr, q_dtype, probe_override, B, k, out_ids_ptr, out_dist_ptr,
                                                         out_count_ptr, scored_ptr or None, sel_ids_ptr or None, sel_count_ptr or None,
                                                         bad_ptr or None, retried_ptr or None, fellback_ptr or None, C.byref(done)))
        return int(done.value)

    def eval_kvariants_dev(self, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, ks, ann_ptr, ann_stride, ann_count_ptr, gt_ptr, gt_stride,
                           unique_ptr, recall_ptr, ratio_ptr, cand_ratio_ptr=0):
        """eval_metrics_typed_dev for every k of ks (a host sequence, at most 64) in one launch: recall / ratio [nk][nq], row j what
        that call writes for k = ks[j], and cand_ratio [nk][nq] = unique / k (NaN where unique <= 0) when unique_ptr is given."""
        kk = [int(x) for x in ks]
        arr = (C.c_int32 * max(1, len(kk)))(*kk)
        N.check(self.L.fspann_eval_kvariants_dev(self._h, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, arr, len(kk), ann_ptr, ann_stride,
                                                 ann_count_ptr or None, gt_ptr, gt_stride, unique_ptr or None, recall_ptr, ratio_ptr,
                                                 cand_ratio_ptr or None))

    def groundtruth_dev(self, n, base_ptr, nq, q_ptr, dim, k, out_ids_ptr, out_d2_ptr=0):
        """Exact k-NN (GroundtruthPrecompute semantics) of device-resident fp32 base / query rows."""
        N.check(self.L.fspann_groundtruth_dev(self._h, n, base_ptr, nq, q_ptr, dim, k, out_ids_ptr, out_d2_ptr or None))

    def eval_metrics_dev(self, n, base_ptr, nq, q_ptr, dim, k, ann_ptr, ann_stride, ann_count_ptr, gt_ptr, gt_stride, recall_ptr, ratio_ptr):
        """recall@k / distance ratio@k per query (ForwardSecureANNSystem.computeMetricsAtK)."""
        N.check(self.L.fspann_eval_metrics_dev(self._h, n, base_ptr, nq, q_ptr, dim, k, ann_ptr, ann_stride, ann_count_ptr or None, gt_ptr, gt_stride,
                                               recall_ptr, ratio_ptr))

    def groundtruth_typed_dev(self, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, k, out_ids_ptr, out_d2_ptr=0):
        """Exact k-NN of device-resident rows: (N.F32, N.F32) as groundtruth_dev, (N.U8, N.U8) over bytes and (N.I8, N.I8) over signed bytes
        on the int8 matrix cores, ids and squared distances bit-identical to the reference's."""
        N.check(self.L.fspann_groundtruth_typed_dev(self._h, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, k, out_ids_ptr, out_d2_ptr or None))

    def eval_metrics_typed_dev(self, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, k, ann_ptr, ann_stride, ann_count_ptr, gt_ptr, gt_stride,
                               recall_ptr, ratio_ptr):
        """eval_metrics_dev over typed rows: N.F32 rows with N.F32 queries, or N.U8 rows with N.U8 / N.F32 queries, or N.I8 rows with
        N.I8 / N.F32 queries, or N.F16 / N.BF16 / N.F8E4M3 rows with N.F32 queries (recall and ratio against a resident half, bfloat16 or fp8 store without an fp32 copy)."""
        N.check(self.L.fspann_eval_metrics_typed_dev(self._h, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, k, ann_ptr, ann_stride,
                                                     ann_count_ptr or None, gt_ptr, gt_stride, recall_ptr, ratio_ptr))

    def groundtruth_rows_dev(self, n, base_ptr, base_dtype, nq, q_ptr, dim, k, out_ids_ptr, out_d2_ptr=0):
        """Exact k-NN of device-resident fp32 queries over typed rows as they are (N.U8, N.I8, N.F16, N.BF16, N.F8E4M3; N.F32 is
        groundtruth_dev): every element widened exactly, ids and squared distances bit-identical to groundtruth_dev over the same
        values held as fp32."""
        N.check(self.L.fspann_groundtruth_rows_dev(self._h, n, base_ptr, base_dtype, nq, q_ptr, dim, k, out_ids_ptr, out_d2_ptr or None))

    def groundtruth_store_dev(self, nq, q_ptr, k, out_ids_ptr, out_d2_ptr=0):
        """groundtruth_rows_dev with the resident store (store_set or store_attach_dev) as the base: the ids eval_metrics_typed_dev
        needs for recall against that store, with no fp32 copy of it."""
        N.check(self.L.fspann_groundtruth_store_dev(self._h, nq, q_ptr, k, out_ids_ptr, out_d2_ptr or None))

    def groundtruth_rows(self, base, q, k, dtype=None):
        """Exact k-NN of fp32 queries over host rows kept in their type on the device.  base [n][dim] and dtype= are what store_set
        takes (np.uint8 / np.int8 / np.float16 arrays or values, the bfloat16 / float8_e4m3fn markers with tensors, bit patterns or
        exact floats); without dtype= a uint8, int8 or float16 array keeps its own type (nothing here widens rows).  q [nq][dim] goes
        as fp32.  float64 rows are refused (the reference's ground truth reads floats: pass dtype=np.float32 to have them cast).
        Returns ids [nq][k] int32 (-1 beyond n) and squared distances [nq][k] float64 (+inf beyond n), what groundtruth() returns
        for the same values held as float32."""
        if dtype is None and getattr(base, "dtype", None) in (np.uint8, np.int8, np.float16):
            dtype = base.dtype
        b, code, _ = _typed_rows(base, dtype, "groundtruth_rows")
        return self._groundtruth_host(b, _c(q, np.float32), k,
                                      lambda n, bd, nq, qd, dim, idd, d2d: self.groundtruth_rows_dev(n, bd, code, nq, qd, dim, k, idd, d2d))

    def gt_validator_sample(self, nq, sample_size=100) -> np.ndarray:
        """GroundtruthValidator's sample (java.util.Random(42).nextInt(nq) into a HashSet<Integer> until it holds
        min(sample_size, nq) values) in the set's iteration order, int64."""
        out = np.empty(max(0, min(int(sample_size), int(nq))), np.int64)
        cnt = C.c_int64(0)
        N.check(self.L.fspann_gt_validator_sample(int(nq), int(sample_size), _p(out) if out.size else None, C.byref(cnt)))
        return out[:cnt.value]

    def nn1_exact_dev(self, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, qsel_ptr, nsel, out_idx_ptr, out_d2_ptr=0):
        """BaseVectorReader.bruteForceNN of device-resident rows (every row dtype but N.F64) for the queries qsel [nsel] (int64
        device list; 0: the first nsel) of q [nq][dim] (N.F64 or N.F32): the subtraction in DOUBLE, a strict `<` minimum over
        ascending rows, -1 / +inf when no sum is below +inf.  One fused kernel, no distance matrix; stream order."""
        N.check(self.L.fspann_nn1_exact_dev(self._h, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, qsel_ptr or None, nsel, out_idx_ptr,
                                            out_d2_ptr or None))

    def nn1_exact_store_dev(self, nq, q_ptr, q_dtype, qsel_ptr, nsel, out_idx_ptr, out_d2_ptr=0):
        """nn1_exact_dev with the resident store as the base."""
        N.check(self.L.fspann_nn1_exact_store_dev(self._h, nq, q_ptr, q_dtype, qsel_ptr or None, nsel, out_idx_ptr, out_d2_ptr or None))

    def gt_validate_dev(self, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, gt_ptr, gt_rows, gt_stride, sample_size, tolerance) -> N.GtValidation:
        """GroundtruthValidator.validate over device buffers (host-synchronous): the fspann_gt_validation it fills."""
        v = N.GtValidation()
        N.check(self.L.fspann_gt_validate_dev(self._h, n, base_ptr, base_dtype, nq, q_ptr, q_dtype, dim, gt_ptr or None, gt_rows, gt_stride,
                                              sample_size, tolerance, C.byref(v)))
        return v

    def gt_validate_store_dev(self, nq, q_ptr, q_dtype, gt_ptr, gt_rows, gt_stride, sample_size, tolerance) -> N.GtValidation:
        """gt_validate_dev against the resident store."""
        v = N.GtValidation()
        N.check(self.L.fspann_gt_validate_store_dev(self._h, nq, q_ptr, q_dtype, gt_ptr or None, gt_rows, gt_stride, sample_size, tolerance,
                                                    C.byref(v)))
        return v

    class _Dev:
        """device buffers of a numpy-level call: up(array) / new(shape, dtype) -> pointer, down(pointer) -> array; freed on exit"""

        def __init__(self, ctx):
            self.ctx, self.bufs = ctx, []

        def __enter__(self):
            return self

        def __exit__(self, *a):
            for p, _, _ in self.bufs:
                self.ctx.L.fspann_dev_free(self.ctx._h, p)

        def new(self, shape, dtype):
            p = C.c_void_p()
            N.check(self.ctx.L.fspann_dev_alloc(self.ctx._h, int(np.prod(shape)) * np.dtype(dtype).itemsize, C.byref(p)))
            self.bufs.append((p, tuple(np.atleast_1d(shape)), np.dtype(dtype)))
            return p

        def up(self, a):
            p = self.new(a.shape, a.dtype)
            if a.nbytes:
                N.check(self.ctx.L.fspann_h2d(self.ctx._h, p, _p(a), a.nbytes))
            return p

        def down(self, p):
            shape, dtype = next((sh, dt) for q, sh, dt in self.bufs if q is p)
            out = np.empty(shape, dtype)
            if out.nbytes:
                N.check(self.ctx.L.fspann_d2h(self.ctx._h, _p(out), p, out.nbytes))
            return out

    def eval_kvariants(self, base, q, ks, ann, ann_count, gt, unique=None, dtype=None):
        """recall@k, distance ratio@k and candidate ratio@k for every k of ks (ForwardSecureANNSystem.computeMetricsAtK over prefixes
        of one result list, FSA:684-692) of host arrays.  base [n][dim] and dtype= are what groundtruth_rows takes; q [nq][dim] goes
        as fp32, or as bytes when it has the byte type of the rows.  ann [nq][stride] result ids with ann_count per query (None: all),
        gt [nq][>= max(ks)] ground-truth ids, unique [nq] = |F_q| of each query's last pass (None: no candidate ratio).
        Returns dict(recall, ratio, cand_ratio) of float64 [nk][nq] (cand_ratio None without unique)."""
        if dtype is None and getattr(base, "dtype", None) in (np.uint8, np.int8, np.float16):
            dtype = base.dtype
        b, code, _ = _typed_rows(base, dtype, "eval_kvariants")
        qq = np.ascontiguousarray(q)
        if not (qq.dtype == b.dtype and code in (N.U8, N.I8)):
            qq = _c(q, np.float32)
        if b.ndim != 2 or qq.ndim != 2 or b.shape[1] != qq.shape[1]:
            raise N.FspannArgumentError("base [n][dim] and q [nq][dim] must share dim")
        a, g = _c(ann, np.int32), _c(gt, np.int32)
        (n, dim), nq, nk = b.shape, qq.shape[0], len(ks)
        if a.ndim != 2 or g.ndim != 2 or a.shape[0] != nq or g.shape[0] != nq:
            raise N.FspannArgumentError("ann [nq][stride] and gt [nq][>= max(ks)] must have one row per query")
        with self._Dev(self) as dv:
            bd, qd, ad, gd = dv.up(b), dv.up(qq), dv.up(a), dv.up(g)
            cd = dv.up(_c(ann_count, np.int32).reshape(nq)) if ann_count is not None else 0
            ud = dv.up(_c(unique, np.int32).reshape(nq)) if unique is not None else 0
            rec, rat = dv.new((nk, nq), np.float64), dv.new((nk, nq), np.float64)
            cr = dv.new((nk, nq), np.float64) if unique is not None else 0
            self.eval_kvariants_dev(n, bd, code, nq, qd, _row_dt(qq), dim, ks, ad, a.shape[1], cd, gd, g.shape[1], ud, rec, rat, cr)
            return dict(recall=dv.down(rec), ratio=dv.down(rat), cand_ratio=dv.down(cr) if cr else None)

    @staticmethod
    def _validator_queries(q):
        """queries as the validator calls take them: float64 stays float64 (the reference's double[]), anything else goes as fp32"""
        qq = np.ascontiguousarray(q)
        return (qq, N.F64) if qq.dtype == np.float64 else (_c(q, np.float32), N.F32)

    @staticmethod
    def _validation_dict(v, tolerance):
        """fspann_gt_validation -> dict, with ValidationResult's message (GroundtruthValidator.java:94-100, 166-182)"""
        rate = float(v.mismatch_rate)
        if v.valid and v.sample_size == 0:
            msg = "No queries to validate"
        elif not v.valid and v.sample_size == 0:
            msg = "Groundtruth is empty"
        elif v.valid:
            msg = "GT validation PASSED: %.2f%% match rate" % ((1 - rate) * 100)
        else:
            msg = ("GT validation FAILED: %.2f%% mismatch rate exceeds %.2f%% tolerance. "
                   "Groundtruth may be corrupted or computed for a different dataset." % (rate * 100, tolerance * 100))
        return dict(valid=bool(v.valid), sample_size=int(v.sample_size), mismatches=int(v.mismatches), mismatch_rate=rate, message=msg,
                    mismatched=[int(x) for x in v.mismatched[:v.n_mismatched]], gt_min_id=int(v.gt_min_id), gt_max_id=int(v.gt_max_id),
                    consistent=bool(v.consistent), tolerance=float(tolerance))

    @staticmethod
    def _validator_defaults(sample_size, tolerance):
        """FSA:2151-2152: a sample size <= 0 becomes 100, a tolerance <= 0 becomes 0.05"""
        return (int(sample_size) if sample_size > 0 else 100), (float(tolerance) if tolerance > 0 else 0.05)

    def nn1_exact(self, base, q, dtype=None, sel=None):
        """The validator's exact nearest row (BaseVectorReader.bruteForceNN: the subtraction in double) of host arrays.  base [n][dim]
        and dtype= are what groundtruth_rows takes; q [nq][dim] goes as float64 if it is float64, otherwise as fp32; sel: the query
        indices to run, in any order, repeats allowed (None: all).  Returns (idx int32, d2 float64), one entry per selected query:
        -1 / +inf where no row's sum is below +inf."""
        if dtype is None and getattr(base, "dtype", None) in (np.uint8, np.int8, np.float16):
            dtype = base.dtype
        b, code, _ = _typed_rows(base, dtype, "nn1_exact")
        qq, qcode = self._validator_queries(q)
        if b.ndim != 2 or qq.ndim != 2 or b.shape[1] != qq.shape[1]:
            raise N.FspannArgumentError("base [n][dim] and q [nq][dim] must share dim")
        (n, dim), nq = b.shape, qq.shape[0]
        s = None if sel is None else _c(sel, np.int64).reshape(-1)
        nsel = nq if s is None else s.size
        with self._Dev(self) as dv:
            bd, qd = dv.up(b), dv.up(qq)
            sd = dv.up(s) if s is not None else 0
            idx, d2 = dv.new((nsel,), np.int32), dv.new((nsel,), np.float64)
            self.nn1_exact_dev(n, bd, code, nq, qd, qcode, dim, sd, nsel, idx, d2)
            return dv.down(idx), dv.down(d2)

    def validate_groundtruth(self, base, q, gt_ids, sample_size=100, tolerance=0.05, dtype=None):
        """GroundtruthValidator.validate (FSA:2144-2193) of host arrays: a deterministic sample of the queries, the exact nearest row
        of each against gt_ids[qi][0].  base, dtype= and q as nn1_exact takes them; gt_ids [gt_rows][stride] int32 (fewer rows than
        queries: the queries past them are skipped but stay in the denominator).  sample_size <= 0 becomes 100 and tolerance <= 0
        becomes 0.05 (FSA:2151-2152).  Returns dict(valid, sample_size, mismatches, mismatch_rate, message, mismatched (the first 10,
        in the sample's order), gt_min_id, gt_max_id, consistent, ...); nothing is raised for an invalid result."""
        sample_size, tolerance = self._validator_defaults(sample_size, tolerance)
        if dtype is None and getattr(base, "dtype", None) in (np.uint8, np.int8, np.float16):
            dtype = base.dtype
        b, code, _ = _typed_rows(base, dtype, "validate_groundtruth")
        qq, qcode = self._validator_queries(q)
        if b.ndim != 2 or qq.ndim != 2 or b.shape[1] != qq.shape[1]:
            raise N.FspannArgumentError("base [n][dim] and q [nq][dim] must share dim")
        g = _c(gt_ids, np.int32)
        if g.ndim != 2:
            raise N.FspannArgumentError("gt_ids must be [gt_rows][stride]")
        with self._Dev(self) as dv:
            bd, qd, gd = dv.up(b), dv.up(qq), dv.up(g)
            v = self.gt_validate_dev(b.shape[0], bd, code, qq.shape[0], qd, qcode, b.shape[1], gd, g.shape[0], g.shape[1], sample_size, tolerance)
        return self._validation_dict(v, tolerance)

    def validate_groundtruth_store(self, q, gt_ids, sample_size=100, tolerance=0.05):
        """validate_groundtruth against the resident store (store_set or store_attach_dev)."""
        sample_size, tolerance = self._validator_defaults(sample_size, tolerance)
        qq, qcode = self._validator_queries(q)
        qq = qq.reshape(-1, self.cfg.dim)
        g = _c(gt_ids, np.int32)
        if g.ndim != 2:
            raise N.FspannArgumentError("gt_ids must be [gt_rows][stride]")
        with self._Dev(self) as dv:
            qd, gd = dv.up(qq), dv.up(g)
            v = self.gt_validate_store_dev(qq.shape[0], qd, qcode, gd, g.shape[0], g.shape[1], sample_size, tolerance)
        return self._validation_dict(v, tolerance)

    def run_queries(self, q, k_variants, gt_ids=None, probe_override=-1, B=None, validate=None, attribution=False):
        """ForwardSecureANNSystem.runQueries (FSA:622-748) for a batch over the resident store: one search at K = max(k_variants) with
        its adaptive retry and the empty-result fallback (search_fallback_dev + its finish call), the ground truth over the store
        (groundtruth_store_dev) unless gt_ids [nq][>= K] is given, and recall / ratio / candidate ratio at every k of k_variants
        from that one result list (eval_kvariants_dev with unique = sel_count).  q [nq][dim] goes as fp32.  B: candidates per query
        (cfg.refinement_limit).  An FSPANN_F64 store is refused: the reference's ground truth reads floats.
        validate=(sample_size, tolerance) with gt_ids given: GroundtruthValidator.validate over the store runs first (FSA:2144-2193);
        an invalid result raises FspannStateError with its message (IllegalStateException, FSA:2185), a valid one is returned as
        gt_validation.  validate=None (the default): no validation, the same launches and the same keys as before.
        Returns dict(ids, dist, count, scored, sel_count, bad, retried, fellback, resolved, gt_ids, recall, ratio, cand_ratio), the
        last three float64 [nk][nq].  (plus gt_validation when it ran)
        attribution=True adds where the recall was lost (route_recall's pass, taken at the probes of each query's LAST pass: 10 if it
        retried, else max(2 base, 4) if it fell back, else the caller's effective probes — at most three groups, one full-list Route
        each): last_probes [nq], gt_rank [nq][K] (the rank of each true neighbour in that pass's full candidate list, -1: Route never
        offered it), route_ceiling and limit_ceiling float64 [nk][nq] (the recall Route's list allows at all, and within its first B
        entries), true_nn_rank = gt_rank[:, 0] and true_nn_seen.  A bad (non-finite) query is not routed: its ranks are -1 and its
        ceilings 0.  attribution=False (the default): the launches and the keys above."""
        code = C.c_int(0)
        store = self.L.fspann_store_dev_ptr(self._h, C.byref(code))
        if not store:
            raise N.FspannStateError("plaintext store not set")
        if code.value == N.F64:
            raise N.FspannArgumentError("run_queries over an FSPANN_F64 store: the reference's ground truth reads floats")
        ks = [int(x) for x in k_variants]
        if not ks:
            raise N.FspannArgumentError("k_variants is empty")
        K, nk = max(ks), len(ks)
        B = int(self.cfg.refinement_limit if B is None else B)
        qq = _c(q, np.float32).reshape(-1, self.cfg.dim)
        nq = qq.shape[0]
        g = None
        if gt_ids is not None:
            g = _c(gt_ids, np.int32)
            if g.ndim != 2 or g.shape[0] != nq or g.shape[1] < K:
                raise N.FspannArgumentError("gt_ids must be [nq][>= max(k_variants)]")
        validation = None
        if validate is not None and g is not None:
            validation = self.validate_groundtruth_store(qq, g, *validate)
            if not validation["valid"]:
                raise N.FspannStateError(validation["message"])
        with self._Dev(self) as dv:
            qd = dv.up(qq)
            ids, dist = dv.new((nq, K), np.int32), dv.new((nq, K), np.float64)
            cnt, sc, selc, bad, ret, fb = (dv.new((nq,), np.int32) for _ in range(6))
            sel = dv.new((nq, B), np.int32)
            args = (nq, qd, N.F32, probe_override, B, K, ids, dist, cnt, sc, sel, selc, bad, ret, fb)
            self.search_fallback_dev(*args)
            resolved = self.search_fallback_finish_dev(*args)
            if g is None:
                gd, gs = dv.new((nq, K), np.int32), K
                self.groundtruth_store_dev(nq, qd, K, gd)
            else:
                gd, gs = dv.up(g), g.shape[1]
            rec, rat, cr = (dv.new((nk, nq), np.float64) for _ in range(3))
            self.eval_kvariants_dev(self._store_n, store, code.value, nq, qd, N.F32, self.cfg.dim, ks, ids, K, cnt, gd, gs, selc, rec, rat, cr)
            out = dict(ids=dv.down(ids), dist=dv.down(dist), count=dv.down(cnt), scored=dv.down(sc), sel_count=dv.down(selc), bad=dv.down(bad),
                       retried=dv.down(ret), fellback=dv.down(fb), resolved=resolved, gt_ids=dv.down(gd), recall=dv.down(rec), ratio=dv.down(rat),
                       cand_ratio=dv.down(cr))
            if validation is not None:
                out["gt_validation"] = validation
            if attribution:
                self._attribute(dv, out, qq, gd, gs, ks, B, probe_override)
            return out

    @staticmethod
    def _limits(limits):
        """limits of a sweep call as the host array the C side reads (it checks count, order and range)"""
        ll = [int(x) for x in limits]
        return (C.c_int64 * max(1, len(ll)))(*ll), len(ll)

    def refine_store_sweep_dev(self, nq, q_ptr, q_dtype, stride, cand_ids_ptr, cand_count_ptr, limits, k, out_ids_ptr, out_dist_ptr,
                               out_count_ptr, scored_ptr=0):
        """refine_store_dev at every limit of limits (a host sequence, ascending, at most 16) from one scan: plane j of ids / dist
        [nl][nq][k] and count / scored [nl][nq] is what refine_store_dev writes with B = stride and the counts clipped to limits[j]."""
        arr, nl = self._limits(limits)
        N.check(self.L.fspann_refine_store_sweep_dev(self._h, nq, q_ptr, q_dtype, stride, cand_ids_ptr, cand_count_ptr, arr, nl, k,
                                                     out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr or None))

    def refine_sweep_dev(self, nq, q_ptr, q_dtype, cand_ptr, cand_dtype, stride, cand_ids_ptr, cand_count_ptr, limits, k, out_ids_ptr,
                         out_dist_ptr, out_count_ptr, scored_ptr=0):
        """refine_store_sweep_dev over caller-held candidate rows [nq][stride][dim] (refine_dev's)."""
        arr, nl = self._limits(limits)
        N.check(self.L.fspann_refine_sweep_dev(self._h, nq, q_ptr, q_dtype, cand_ptr, cand_dtype, stride, cand_ids_ptr, cand_count_ptr, arr, nl, k,
                                               out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr or None))

    def search_sweep_dev(self, nq, q_ptr, q_dtype, probe_override, limits, k, out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr=0,
                         unique_ptr=0, bad_ptr=0, retried_ptr=0):
        """search_retry_dev at every refinement limit of limits in one pass: one encode, one Route at max(limits), one scan; plane j of
        every output is what search_retry_dev + its finish call write at B = limits[j] (unique = that call's sel_count)."""
        arr, nl = self._limits(limits)
        N.check(self.L.fspann_search_sweep_dev(self._h, nq, q_ptr, q_dtype, probe_override, arr, nl, k, out_ids_ptr, out_dist_ptr, out_count_ptr,
                                               scored_ptr or None, unique_ptr or None, bad_ptr or None, retried_ptr or None))

    def search_sweep_finish_dev(self, nq, q_ptr, q_dtype, probe_override, limits, k, out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr=0,
                                unique_ptr=0, bad_ptr=0, retried_ptr=0) -> int:
        """Completes the preceding search_sweep_dev call (same arguments) as search_retry_finish_dev completes its call.  Returns how
        many queries were finished on the host."""
        arr, nl = self._limits(limits)
        done = C.c_int64(0)
        N.check(self.L.fspann_search_sweep_finish_dev(self._h, nq, q_ptr, q_dtype, probe_override, arr, nl, k, out_ids_ptr, out_dist_ptr,
                                                      out_count_ptr, scored_ptr or None, unique_ptr or None, bad_ptr or None,
                                                      retried_ptr or None, C.byref(done)))
        return int(done.value)

    def _search_sweep(self, dv, qd, nq, limits, k, probe_override):
        """search_sweep_dev + its finish call into fresh device planes: (ids, dist, count, scored, unique, bad, retried, resolved)"""
        nl = len(limits)
        ids, dist = dv.new((nl, nq, k), np.int32), dv.new((nl, nq, k), np.float64)
        cnt, sc, un, ret = (dv.new((nl, nq), np.int32) for _ in range(4))
        bad = dv.new((nq,), np.int32)
        args = (nq, qd, N.F32, probe_override, limits, k, ids, dist, cnt, sc, un, bad, ret)
        self.search_sweep_dev(*args)
        resolved = self.search_sweep_finish_dev(*args)
        return ids, dist, cnt, sc, un, bad, ret, resolved

    def search_sweep(self, q, limits, k, probe_override=-1):
        """QueryServiceImpl.search with its adaptive retry at every refinement limit of limits (ascending, at most 16) in one pass over
        the resident store.  q [nq][dim] goes as fp32.  Returns dict(ids, dist [nl][nq][k], count, scored, unique, retried [nl][nq],
        bad [nq], resolved): plane j is the search at refinement limit limits[j]."""
        ll = [int(x) for x in limits]
        qq = _c(q, np.float32).reshape(-1, self.cfg.dim)
        nq = qq.shape[0]
        with self._Dev(self) as dv:
            qd = dv.up(qq)
            ids, dist, cnt, sc, un, bad, ret, resolved = self._search_sweep(dv, qd, nq, ll, int(k), probe_override)
            return dict(ids=dv.down(ids), dist=dv.down(dist), count=dv.down(cnt), scored=dv.down(sc), unique=dv.down(un), retried=dv.down(ret),
                        bad=dv.down(bad), resolved=resolved)

    def limit_sweep(self, q, limits, k_variants, gt_ids=None, probe_override=-1):
        """recall@k / ratio@k / candidate ratio@k against the refinement limit, from one pass: one search_sweep at K = max(k_variants),
        the ground truth over the store once (groundtruth_store_dev) unless gt_ids [nq][>= K] is given, and eval_kvariants_dev once per
        limit with that plane's unique.  An FSPANN_F64 store is refused as run_queries refuses it.  The sweep is QueryServiceImpl.search,
        not runQueries: would_fall_back [nl][nq] (count == 0 and not bad) says where run_queries would have searched again.
        Returns the keys of search_sweep plus gt_ids, recall, ratio, cand_ratio (float64 [nl][nk][nq]) and would_fall_back."""
        code = C.c_int(0)
        store = self.L.fspann_store_dev_ptr(self._h, C.byref(code))
        if not store:
            raise N.FspannStateError("plaintext store not set")
        if code.value == N.F64:
            raise N.FspannArgumentError("limit_sweep over an FSPANN_F64 store: the reference's ground truth reads floats")
        ks = [int(x) for x in k_variants]
        if not ks:
            raise N.FspannArgumentError("k_variants is empty")
        ll = [int(x) for x in limits]
        K, nk, nl = max(ks), len(ks), len(ll)
        qq = _c(q, np.float32).reshape(-1, self.cfg.dim)
        nq = qq.shape[0]
        g = None
        if gt_ids is not None:
            g = _c(gt_ids, np.int32)
            if g.ndim != 2 or g.shape[0] != nq or g.shape[1] < K:
                raise N.FspannArgumentError("gt_ids must be [nq][>= max(k_variants)]")
        with self._Dev(self) as dv:
            qd = dv.up(qq)
            ids, dist, cnt, sc, un, bad, ret, resolved = self._search_sweep(dv, qd, nq, ll, K, probe_override)
            if g is None:
                gd, gs = dv.new((nq, K), np.int32), K
                self.groundtruth_store_dev(nq, qd, K, gd)
            else:
                gd, gs = dv.up(g), g.shape[1]
            rec, rat, cr = (dv.new((nl, nk, nq), np.float64) for _ in range(3))
            for j in range(nl):
                def plane(p, per_q, size):
                    return C.c_void_p(p.value + j * per_q * size)
                self.eval_kvariants_dev(self._store_n, store, code.value, nq, qd, N.F32, self.cfg.dim, ks, plane(ids, nq * K, 4), K,
                                        plane(cnt, nq, 4), gd, gs, plane(un, nq, 4), plane(rec, nk * nq, 8), plane(rat, nk * nq, 8),
                                        plane(cr, nk * nq, 8))
            out = dict(ids=dv.down(ids), dist=dv.down(dist), count=dv.down(cnt), scored=dv.down(sc), unique=dv.down(un), retried=dv.down(ret),
                       bad=dv.down(bad), resolved=resolved, gt_ids=dv.down(gd), recall=dv.down(rec), ratio=dv.down(rat), cand_ratio=dv.down(cr))
            out["would_fall_back"] = (out["count"] == 0) & (out["bad"][None, :] == 0)
            return out

    # -- recall attribution (include/fspann_route_recall.h) -----------------------------------
    def gt_rank_dev(self, nq, list_ids_ptr, list_score_ptr, list_stride, list_count_ptr, gt_ptr, gt_stride, kg, rank_ptr, gt_score_ptr=0):
        """rank [nq][kg]: the position of every ground-truth id among the first min(list_count, list_stride) entries of its query's
        list (-1: not there; -2: list_count -1, a flagged query nobody resolved), and gt_score [nq][kg] = list_score at that position
        (-1 where rank < 0) when both score pointers are given.  One pass over the list, stream order."""
        N.check(self.L.fspann_gt_rank_dev(self._h, nq, list_ids_ptr, list_score_ptr or None, list_stride, list_count_ptr or None, gt_ptr,
                                          gt_stride, kg, rank_ptr, gt_score_ptr or None))

    def recall_ceiling_dev(self, nq, rank_ptr, rank_stride, ks, limits, hits_ptr, ceiling_ptr=0):
        """hits / ceiling [nl + 1][nk][nq] from rank [nq][rank_stride]: plane l counts the first ks[j] ranks in [0, limits[l]), the
        last plane those >= 0 (Route's own ceiling); ceiling = hits / ks[j].  ks (at most 64) and limits (ascending, at most 16, may
        be empty) are host sequences."""
        kk = [int(x) for x in ks]
        arr = (C.c_int32 * max(1, len(kk)))(*kk)
        lim, nl = self._limits(limits)
        N.check(self.L.fspann_recall_ceiling_dev(self._h, nq, rank_ptr, rank_stride, arr, len(kk), lim, nl, hits_ptr, ceiling_ptr or None))

    def _route_rank(self, dv, nq, qd, gd, gs, K, probe_override, rank, gscore=0):
        """One encode and one full-list Route (limit INT32_MAX, score and kept requested) of the device queries qd at probe_override,
        the flagged queries finished by the host model, then the rank of the ground truth gd [nq][gs] in that list into rank [nq][K].
        Returns (kept pointer, resolved)."""
        cap = max(1, self.route_max_candidates(probe_override))
        codes = dv.new((nq, self.TD, self.W), np.uint64)
        ids, score = dv.new((nq, cap), np.int32), dv.new((nq, cap), np.int32)
        cnt, kept = dv.new((nq,), np.int32), dv.new((nq,), np.int32)
        self.encode_dev(nq, qd, N.F32, codes)
        rargs = (nq, codes, probe_override, N.INT32_MAX, cap, ids, score, cnt, kept, 0)
        self.route_dev(*rargs)
        resolved = self.route_resolve_dev(*rargs)
        self.gt_rank_dev(nq, ids, score if gscore else 0, cap, cnt, gd, gs, K, rank, gscore)
        return kept, resolved

    def _attribution_args(self, what, q, k_variants, gt_ids):
        """store pointer and dtype, ks, queries as fp32 and the caller's ground truth of an attribution call, checked"""
        code = C.c_int(0)
        store = self.L.fspann_store_dev_ptr(self._h, C.byref(code))
        if not store:
            raise N.FspannStateError("plaintext store not set")
        if code.value == N.F64:
            raise N.FspannArgumentError(what + " over an FSPANN_F64 store: the reference's ground truth reads floats")
        ks = [int(x) for x in k_variants]
        if not ks:
            raise N.FspannArgumentError("k_variants is empty")
        qq = _c(q, np.float32).reshape(-1, self.cfg.dim)
        g = None
        if gt_ids is not None:
            g = _c(gt_ids, np.int32)
            if g.ndim != 2 or g.shape[0] != qq.shape[0] or g.shape[1] < max(ks):
                raise N.FspannArgumentError("gt_ids must be [nq][>= max(k_variants)]")
        return ks, qq, g

    def route_recall(self, q, k_variants, limits=(), gt_ids=None, probe_override=-1):
        """Where recall is lost, without one Refine: the rank of every true neighbour in Route's full candidate list
        (lookupCandidatesWithScores' order; the rank of an id is the refinement limit at which the search starts to score it) and the
        recall ceilings the ranks imply — Route's own (the id is in the list at all: probes and tables) and the ceiling at every
        refinement limit of limits (the id is among the first B entries: refinementLimit).  One encode, one Route at limit INT32_MAX
        with score and kept requested, the flagged queries finished by the host model (never -2 here), the ground truth over the
        store at K = max(k_variants) (groundtruth_store_dev) unless gt_ids [nq][>= K] is given, then gt_rank_dev and
        recall_ceiling_dev.  No candidate row is read.  An FSPANN_F64 store is refused as run_queries refuses it, a non-finite query
        as encode() refuses it.
        Returns dict(gt_ids, rank, gt_score [nq][K]; kept [nq]; hits int32, ceiling float64 [nl + 1][nk][nq], plane l at limits[l], the
        last plane Route's own; route_ceiling [nk][nq] = that last plane; true_nn_rank = rank[:, 0], true_nn_seen; resolved) — what
        the reference's lastTrueNNRank / lastTrueNNSeen columns (FSA:740-741) were declared for and never assigned."""
        ks, qq, g = self._attribution_args("route_recall", q, k_variants, gt_ids)
        if not np.isfinite(qq).all():
            raise N.FspannArgumentError("Vector contains NaN/Inf")      # (what encode() says: Coding.java:360)
        ll = [int(x) for x in limits]
        K, nk, nl, nq = max(ks), len(ks), len(ll), qq.shape[0]
        with self._Dev(self) as dv:
            qd = dv.up(qq)
            if g is None:
                gd, gs = dv.new((nq, K), np.int32), K
                self.groundtruth_store_dev(nq, qd, K, gd)
            else:
                gd, gs = dv.up(g), g.shape[1]
            rank, gscore = dv.new((nq, K), np.int32), dv.new((nq, K), np.int32)
            kept, resolved = self._route_rank(dv, nq, qd, gd, gs, K, probe_override, rank, gscore)
            hits, ceil = dv.new((nl + 1, nk, nq), np.int32), dv.new((nl + 1, nk, nq), np.float64)
            self.recall_ceiling_dev(nq, rank, K, ks, ll, hits, ceil)
            out = dict(gt_ids=dv.down(gd)[:, :K].copy(), rank=dv.down(rank), gt_score=dv.down(gscore), kept=dv.down(kept), hits=dv.down(hits),
                       ceiling=dv.down(ceil), resolved=resolved)
        out["route_ceiling"] = out["ceiling"][nl]
        out["true_nn_rank"] = out["rank"][:, 0].copy()
        out["true_nn_seen"] = out["true_nn_rank"] >= 0
        return out

    # -- Route coverage map (include/fspann_route_coverage.h) -----------------------------------
    def gt_reach_dev(self, nq, codes_ptr, probes_max, gt_ptr, gt_stride, kg, reach_ptr):
        """reach [nq][kg][T*D]: per ground-truth id and table (step << 16) | hamming — the position of the id's partition in the order
        Route polls that table's partitions for the query, and the partition's Hamming score — or -1 (the table does not offer the
        id within probes_max probes; padding, an id >= n_ids or a deleted id: every table).  probes_max is literal, 1 .. 32.  One
        launch, stream order."""
        N.check(self.L.fspann_gt_reach_dev(self._h, nq, codes_ptr, probes_max, gt_ptr, gt_stride, kg, reach_ptr))

    def route_coverage_dev(self, nq, reach_ptr, kg, reach_probes, ks, grid, hits_ptr, ceiling_ptr=0, score_ptr=0):
        """hits / ceiling [nc][nk][nq] and score [nc][nq][kg] of the configurations grid [nc][3] = (tables, divisions, probes) from the
        records of gt_reach_dev at probes_max = reach_probes.  ks (at most 64) and grid (at most 64 rows) are host sequences.
        Returns exact [nc] (bool): the configuration cannot meet HARD_CAP, its answer is Route's own; elsewhere it is an upper bound."""
        kk = [int(x) for x in ks]
        karr = (C.c_int32 * max(1, len(kk)))(*kk)
        gg = [int(x) for row in grid for x in row]
        if len(gg) % 3:
            raise N.FspannArgumentError("grid must be [nc][3] = (tables, divisions, probes)")
        nc = len(gg) // 3
        garr = (C.c_int32 * max(3, len(gg)))(*gg)
        exact = (C.c_uint8 * max(1, nc))()
        N.check(self.L.fspann_route_coverage_dev(self._h, nq, reach_ptr, kg, reach_probes, karr, len(kk), garr, nc, hits_ptr, ceiling_ptr or None,
                                                 score_ptr or None, exact))
        return np.frombuffer(exact, np.uint8, nc).astype(bool)

    def route_coverage(self, q, k_variants, grid, gt_ids=None, probes_max=None):
        """How many tables, divisions and probes Route needs before it offers the true neighbours, for every configuration of grid
        [nc][3] = (tables <= T, divisions <= D, probes) at once, from this index and one pass: the probe order of a table does not
        depend on the probe count, and the index a Setup at (T', D') builds is the sub-grid of tables t < T', d < D' of this one.  One
        encode, the ground truth over the store at K = max(k_variants) (groundtruth_store_dev) unless gt_ids [nq][>= K] is given,
        gt_reach_dev at probes_max (default: the largest probes of grid) and route_coverage_dev in groups of 64 configurations.  No
        candidate row is read, nothing is set up or routed.
        Returns dict(gt_ids [nq][K]; step, hamming [nq][K][T][D] (-1: not reached within probes_max); hits int32, ceiling float64
        [nc][nk][nq]; score [nc][nq][K] (the Hamming score Route ranks the id with, -1: not offered); exact [nc] bool — where False,
        HARD_CAP may stop Route early: offered is a superset and ceiling an upper bound; grid [nc][3])."""
        ks, qq, g = self._attribution_args("route_coverage", q, k_variants, gt_ids)
        if not np.isfinite(qq).all():
            raise N.FspannArgumentError("Vector contains NaN/Inf")      # (what encode() says: Coding.java:360)
        gr = np.asarray(grid, np.int64).reshape(-1, 3)
        if not len(gr):
            raise N.FspannArgumentError("grid is empty")
        P = int(gr[:, 2].max()) if probes_max is None else int(probes_max)
        K, nk, nc, nq = max(ks), len(ks), len(gr), qq.shape[0]
        T, D = self.cfg.tables, self.cfg.divisions
        with self._Dev(self) as dv:
            qd = dv.up(qq)
            if g is None:
                gd, gs = dv.new((nq, K), np.int32), K
                self.groundtruth_store_dev(nq, qd, K, gd)
            else:
                gd, gs = dv.up(g), g.shape[1]
            codes = dv.new((nq, self.TD, self.W), np.uint64)
            self.encode_dev(nq, qd, N.F32, codes)
            reach = dv.new((nq, K, self.TD), np.int32)
            self.gt_reach_dev(nq, codes, P, gd, gs, K, reach)
            hits, ceil, score, exact = [], [], [], []
            for c0 in range(0, nc, 64):
                part = gr[c0:c0 + 64]
                h, ce, sc = dv.new((len(part), nk, nq), np.int32), dv.new((len(part), nk, nq), np.float64), dv.new((len(part), nq, K), np.int32)
                exact.append(self.route_coverage_dev(nq, reach, K, P, ks, part, h, ce, sc))
                hits.append(dv.down(h)), ceil.append(dv.down(ce)), score.append(dv.down(sc))
            rec = dv.down(reach).reshape(nq, K, T, D)
            gt = dv.down(gd)[:, :K].copy()
        return dict(gt_ids=gt, step=np.where(rec >= 0, rec >> 16, -1).astype(np.int32), hamming=np.where(rec >= 0, rec & 0xFFFF, -1).astype(np.int32),
                    hits=np.concatenate(hits), ceiling=np.concatenate(ceil), score=np.concatenate(score), exact=np.concatenate(exact),
                    grid=gr.astype(np.int32))

    def _last_probes(self, probe_override, retried, fellback):
        """The probes of each query's last pass in run_queries (the rule of fspann_eval.h for whose rows a query keeps): 10 if it
        retried, else max(2 base, 4) if it fell back (FSA:640, 668-673), else the caller's effective probes."""
        po = probe_override if probe_override >= 0 else self.cfg.probe_override
        base = po if po >= 0 else self.cfg.default_probes
        F = min(max(2 * base, 4), N.INT32_MAX)
        return np.where(retried != 0, 10, np.where(fellback != 0, F, self.effective_probes(probe_override))).astype(np.int32)

    def _attribute(self, dv, out, qq, gd, gs, ks, B, probe_override):
        """run_queries(attribution=True): the ranks of the ground truth in the full list of each query's last pass.  The batch splits
        by the probes of that pass into at most three groups, one full-list Route each."""
        K, nq = max(ks), qq.shape[0]
        last = self._last_probes(probe_override, out["retried"], out["fellback"])
        gt = dv.down(gd)
        rank = np.full((nq, K), -1, np.int32)
        good = out["bad"] == 0              # a non-finite query was never coded or searched: its ranks stay -1, its ceilings 0
        for p in np.unique(last[good]):
            sel = np.flatnonzero((last == p) & good)
            qd, gsel = dv.up(np.ascontiguousarray(qq[sel])), dv.up(np.ascontiguousarray(gt[sel]))
            r = dv.new((len(sel), K), np.int32)
            self._route_rank(dv, len(sel), qd, gsel, gs, K, int(p), r)
            rank[sel] = dv.down(r)
        rd = dv.up(rank)
        ceil_hits, ceil = dv.new((2, len(ks), nq), np.int32), dv.new((2, len(ks), nq), np.float64)
        self.recall_ceiling_dev(nq, rd, K, ks, [B], ceil_hits, ceil)
        c = dv.down(ceil)
        out.update(last_probes=last, gt_rank=rank, limit_ceiling=c[0], route_ceiling=c[1], true_nn_rank=rank[:, 0].copy(),
                   true_nn_seen=rank[:, 0] >= 0)

    def _groundtruth_host(self, b, qq, k, run):
        """base b and queries qq (host arrays as they go to the device) -> ids, d2 of the device call `run`"""
        if b.ndim != 2 or qq.ndim != 2 or b.shape[1] != qq.shape[1]:
            raise N.FspannArgumentError("base [n][dim] and q [nq][dim] must share dim")
        (n, dim), nq = b.shape, qq.shape[0]
        ids, d2 = np.empty((nq, k), np.int32), np.empty((nq, k), np.float64)
        ptrs = []
        try:
            for nbytes in (b.nbytes, qq.nbytes, ids.nbytes, d2.nbytes):
                p = C.c_void_p()
                N.check(self.L.fspann_dev_alloc(self._h, nbytes, C.byref(p)))
                ptrs.append(p)
            bd, qd, idd, d2d = ptrs
            N.check(self.L.fspann_h2d(self._h, bd, _p(b), b.nbytes))
            N.check(self.L.fspann_h2d(self._h, qd, _p(qq), qq.nbytes))
            run(n, bd, nq, qd, dim, idd, d2d)
            N.check(self.L.fspann_d2h(self._h, _p(ids), idd, ids.nbytes))
            N.check(self.L.fspann_d2h(self._h, _p(d2), d2d, d2.nbytes))
        finally:
            for p in ptrs:
                self.L.fspann_dev_free(self._h, p)
        return ids, d2

    def groundtruth(self, base, q, k):
        """Exact k-NN of host arrays: uint8 arrays stay bytes on the device, int8 arrays signed bytes, anything else goes as fp32
        (base and q alike; bytes with anything but bytes of the same signedness do not match).
        Returns ids [nq][k] int32 (-1 beyond n) and squared distances [nq][k] float64 (+inf beyond n)."""
        base, q = np.asarray(base), np.asarray(q)
        if (base.dtype == np.uint8) != (q.dtype == np.uint8) or (base.dtype == np.int8) != (q.dtype == np.int8):
            raise N.FspannArgumentError("Base and query types must match (both fvecs or both bvecs)")
        dt = base.dtype if base.dtype in (np.uint8, np.int8) else np.float32
        b, qq = _c(base, dt), _c(q, dt)
        return self._groundtruth_host(b, qq, k, lambda n, bd, nq, qd, dim, idd, d2d: self.groundtruth_typed_dev(n, bd, _row_dt(b), nq, qd, _row_dt(qq), dim, k,
                                                                                                        idd, d2d))

    def route_handover_bytes(self, nq, probe_override=-1) -> int:
        return int(self.L.fspann_route_handover_bytes(self._h, nq, probe_override))

    def tick_dev(self, encode=None, route=None, refine=None):
        """One launch for encode / Route / Refine of three batches in flight (fspann_tick_dev).  Each part is a dict of
        device pointers (ints) or None:
          encode: nq, q, codes, [dtype = F32], [bad]
          route:  nq, codes, limit, ids, count, [probe_override], [handover]
          refine: nq, q, B, ids, count, k, out_ids, out_dist, out_count, [cand (None: from the store)], [q_dtype], [cand_dtype],
                  [codes + handover of that batch], [probe_override], [scored]"""
        t = N.Tick()
        if encode:
            t.nq_encode, t.enc_q_dev, t.enc_dtype = encode["nq"], encode["q"], encode.get("dtype", N.F32)
            t.enc_codes_dev, t.enc_bad_dev = encode["codes"], encode.get("bad") or None
        if route:
            t.nq_route, t.route_codes_dev, t.route_limit = route["nq"], route["codes"], route["limit"]
            t.route_probe_override = route.get("probe_override", -1)
            t.route_ids_dev, t.route_count_dev, t.route_handover_dev = route["ids"], route["count"], route.get("handover") or None
        if refine:
            t.nq_refine, t.ref_q_dev, t.ref_B, t.k = refine["nq"], refine["q"], refine["B"], refine["k"]
            t.ref_q_dtype, t.ref_cand_dtype = refine.get("q_dtype", N.F32), refine.get("cand_dtype", N.F32)
            t.ref_cand_dev = refine.get("cand") or None
            t.ref_ids_dev, t.ref_count_dev = refine["ids"], refine["count"]
            t.ref_codes_dev, t.ref_handover_dev = refine.get("codes") or None, refine.get("handover") or None
            t.ref_probe_override = refine.get("probe_override", -1)
            t.out_ids_dev, t.out_dist_dev, t.out_count_dev = refine["out_ids"], refine["out_dist"], refine["out_count"]
            t.scored_dev = refine.get("scored") or None
        N.check(self.L.fspann_tick_dev(self._h, C.byref(t)))

    def last_tick_fused(self) -> bool:
        return bool(self.L.fspann_last_tick_fused(self._h))

    def last_front_encode_mfma(self) -> bool:
        """True if the last tick_dev coded its encode batch with the front launch's MFMA role (encode_mfma_block)."""
        return bool(self.L.fspann_last_front_encode_mfma(self._h))

    def refine_timing_begin(self, max_launches, every=1):
        N.check(self.L.fspann_refine_timing_begin(self._h, int(max_launches), int(every)))

    def refine_timing_end(self):
        """(dispatches, total ms) of the refinement-scan kernels launched since refine_timing_begin (kernel-attached HIP events)."""
        import ctypes as C
        n, ms = C.c_int(0), C.c_double(0.0)
        N.check(self.L.fspann_refine_timing_end(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def refine_store_dev(self, nq, q_ptr, q_dtype, B, cand_ids_ptr, cand_count_ptr, k, out_ids_ptr, out_dist_ptr,
                         out_count_ptr, scored_ptr=0):
        N.check(self.L.fspann_refine_store_dev(self._h, nq, q_ptr, q_dtype, B, cand_ids_ptr, cand_count_ptr, k,
                                               out_ids_ptr, out_dist_ptr, out_count_ptr, scored_ptr or None))

    def refine_dev(self, nq, q_ptr, q_dtype, cand_ptr, cand_dtype, B, cand_ids_ptr, cand_count_ptr, k, out_ids_ptr,
                   out_dist_ptr, out_count_ptr, scored_ptr=0):
        N.check(self.L.fspann_refine_dev(self._h, nq, q_ptr, q_dtype, cand_ptr, cand_dtype, B, cand_ids_ptr,
                                         cand_count_ptr, k, out_ids_ptr, out_dist_ptr, out_count_ptr,
                                         scored_ptr or None))
