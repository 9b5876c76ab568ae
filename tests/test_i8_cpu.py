"""CPU: the FSPANN_I8 row type (signed bytes, value = the two's-complement integer -128..127) exists in every layer of the ABI
(header, ctypes binding, JNI generator and generated Java), the numpy wrapper takes int8 rows without shifting, rounding or scaling
them, the entry points that take the dtype answer a null context as before, the wrap-around identity the signed ground truth
rests on holds at its extremes, and the built gfx950 code object holds the int8_t instantiations of every kernel a signed byte
row can reach — without scratch memory, the dense streaming ones with the registers and the LDS of their FSPANN_U8 twins."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_abi_constant_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "fspann.h")).read()
    assert re.search(r"^#define\s+FSPANN_I8\s+6\s*$", hdr, re.M)
    assert re.search(r"^#define\s+FSPANN_F8E4M3\s+5\s*$", hdr, re.M) and re.search(r"^#define\s+FSPANN_U8\s+2\s*$", hdr, re.M)
    N = pkg._native
    assert N.I8 == 6 and (N.F32, N.F64, N.U8, N.F16, N.BF16, N.F8E4M3) == (0, 1, 2, 3, 4, 5)
    java = open(os.path.join(ROOT, "java", "com", "fspann", "gpu", "FspannNative.java")).read()
    assert re.search(r"\bI8 = 6\b", java) and re.search(r"\bU8 = 2\b", java)
    gen = open(os.path.join(ROOT, "tools", "gen_jni.py")).read()
    assert re.search(r"\bint I8 = 6\b", gen)
    names = open(os.path.join(ROOT, "jni", "bound_symbols.txt")).read().split()
    assert len(names) == 94 and len(pkg._native.exported_symbols()) == 94          # no entry point is added


def test_row_typing_of_int8_arrays(pkg):
    from fspann_amd import engine
    N = pkg._native
    assert engine._row_dt(np.zeros(1, np.int8)) == N.I8                   # rows: store, Setup input, ground-truth pairs
    assert engine._row_dt(np.zeros(1, np.uint8)) == N.U8 and engine._row_dt(np.zeros(1, np.float32)) == N.F32
    assert engine._row_dt(np.zeros(1, np.float64)) == N.F64 and engine._row_dt(np.zeros(1, np.float16)) == N.F16
    with pytest.raises(pkg.FspannArgumentError):
        engine._row_dt(np.zeros(1, np.int16))
    # _dt also types queries, and a query is never a signed byte: it keeps refusing int8 (tests/test_u8_cpu.py holds it to that)
    with pytest.raises(pkg.FspannArgumentError):
        engine._dt(np.zeros(1, np.int8))


def test_wrapper_takes_exact_values_only(pkg):
    from fspann_amd.engine import _i8_rows
    a = np.arange(-128, 128, dtype=np.int8).reshape(16, 16)
    out = _i8_rows(a, "store_set")
    assert out.dtype == np.int8 and np.array_equal(out, a)
    for dt in (np.float32, np.float64, np.float16, np.int16, np.int32, np.int64):
        got = _i8_rows(np.array([[127, -128, 0, -1, 1, 5]], dt), "store_set")     # the extremes are taken from any array
        assert got.dtype == np.int8 and got.tolist() == [[127, -128, 0, -1, 1, 5]]
    got = _i8_rows(np.array([[200, 127]], np.uint8)[:, 1:], "store_set")           # an unsigned array within range
    assert got.dtype == np.int8 and got.tolist() == [[127]]
    for bad in (128.0, -129.0, 0.5, -0.5, np.nan, np.inf, -np.inf, 1e10):
        with pytest.raises(pkg.FspannArgumentError, match="int8"):
            _i8_rows(np.array([[0.0, bad, 1.0]], np.float64), "store_set")
    with pytest.raises(pkg.FspannArgumentError, match="int8"):
        _i8_rows(np.array([[128]], np.int16), "store_set")
    with pytest.raises(pkg.FspannArgumentError, match="int8"):
        _i8_rows(np.array([[-129]], np.int64), "store_set")
    with pytest.raises(pkg.FspannArgumentError, match="int8"):
        _i8_rows(np.array([[255]], np.uint8), "store_set")                         # bytes are not reinterpreted


class _FakeLib:
    """records the calls store_set / build_index / build_append make (no device)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


def _fake_ctx(pkg, d):
    ctx = object.__new__(pkg.FspannContext)
    ctx.cfg = pkg.PaperRuntimeConfig(tables=1, divisions=1, m=4, lambda_=2, dim=d)
    ctx.L, ctx._h = _FakeLib(), None
    return ctx


def test_store_set_and_build_type_int8_rows(pkg):
    N = pkg._native
    ctx = _fake_ctx(pkg, 4)
    X = np.array([[-128, 127, -1, 0], [1, 2, 3, -4]], np.int8)
    ctx.store_set(X, dtype=np.int8)
    name, a = ctx.L.calls[-1]
    assert name == "fspann_store_set" and a[1] == 2 and a[3] == N.I8 and ctx.store_dtype == np.int8
    ctx.store_set(X.astype(np.float32), dtype=np.int8)                        # integers -128..127 held as fp32: packed
    assert ctx.L.calls[-1][1][3] == N.I8 and ctx.store_dtype == np.int8
    ctx.store_set(X)                                                          # no dtype: widened to float64, as before
    assert ctx.L.calls[-1][1][3] == N.F64 and ctx.store_dtype == np.float64
    ncalls = len(ctx.L.calls)
    for bad in (X.astype(np.float64) + 0.5, np.full((1, 4), 128.0), np.full((1, 4), -129.0), np.full((1, 4), np.nan), np.full((1, 4), np.inf)):
        with pytest.raises(pkg.FspannArgumentError):
            ctx.store_set(bad, dtype=np.int8)
    assert len(ctx.L.calls) == ncalls                                          # refused before the store is touched
    ctx.build_index(X)                                                        # Setup types int8 arrays by their array, as it does uint8
    name, a = ctx.L.calls[-1]
    assert name == "fspann_build_index" and a[3] == N.I8
    ctx.build_append(X)
    name, a = ctx.L.calls[-1]
    assert name == "fspann_build_append" and a[3] == N.I8
    ctx.build_index(X.view(np.uint8))
    assert ctx.L.calls[-1][1][3] == N.U8
    ctx.build_index(X.astype(np.int16))                                       # any other integer array is still widened
    assert ctx.L.calls[-1][1][3] == N.F64
    # ground truth: a signed array pairs with a signed array only
    for b, q in ((np.int8, np.uint8), (np.uint8, np.int8), (np.int8, np.float32), (np.float32, np.int8)):
        with pytest.raises(pkg.FspannArgumentError, match="must match"):
            ctx.groundtruth(np.zeros((4, 4), b), np.zeros((2, 4), q), 2)


def test_null_context_without_gpu(pkg):
    N = pkg._native
    L = N.lib()
    I8 = N.I8
    assert L.fspann_store_set(None, 4, None, I8) == N.E_NULL
    assert L.fspann_store_attach_dev(None, 4, None, I8) == N.E_NULL
    assert L.fspann_build_index(None, 4, None, I8, None) == N.E_NULL
    assert L.fspann_build_append(None, 4, None, I8) == N.E_NULL
    assert L.fspann_encode(None, 1, None, I8, None, None) == N.E_NULL
    assert L.fspann_encode_dev(None, 1, None, I8, None, None, None) == N.E_NULL
    assert L.fspann_refine(None, 1, None, None, I8, 4, None, None, 1, None, None, None, None) == N.E_NULL
    assert L.fspann_refine_dev(None, 1, None, N.F32, None, I8, 4, None, None, 1, None, None, None, None) == N.E_NULL
    assert L.fspann_refine_store_dev(None, 1, None, I8, 4, None, None, 1, None, None, None, None) == N.E_NULL
    assert L.fspann_groundtruth_typed_dev(None, 10, None, I8, 2, None, I8, 16, 5, None, None) == N.E_NULL
    assert L.fspann_eval_metrics_typed_dev(None, 10, None, I8, 2, None, I8, 16, 5, None, 5, None, None, 5, None, None) == N.E_NULL
    # the point store has no device in it: it refuses signed bytes by name, behind its own argument checks
    import ctypes as C
    ps = C.c_void_p()
    N.check(L.fspann_pointstore_create(8, 4, C.byref(ps)))
    try:
        buf = np.zeros(64, np.int8)
        vp = buf.ctypes.data_as(C.c_void_p)
        assert L.fspann_pointstore_encrypt(ps, 0, 2, vp, I8, 1) == N.E_ARG
        assert b"FSPANN_I8" in L.fspann_last_error()
        hi, hn = np.zeros((1, 2), np.int32), np.zeros(1, np.int32)
        ip = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.fspann_pointstore_open_batch(ps, 1, 2, ip(hi), ip(hn), vp, I8, ip(hi.copy()), ip(hn.copy()), 1) == N.E_ARG
        assert b"FSPANN_I8" in L.fspann_last_error() and b"dst_dtype" in L.fspann_last_error()
    finally:
        L.fspann_pointstore_destroy(ps)


@pytest.mark.parametrize("d", [1, 7, 100, 960, 32768])
def test_wraparound_identity_at_the_extremes(d):
    """What gt8_dist_kernel<int8_t, .> stores is |q|^2 + |x|^2 - 2 q.x in uint32 arithmetic.  Restated in numpy with the same wrap-around:
    it equals sum (q - x)^2 for every pairing of all -128, all 127, all -1 and mixed rows, up to d = 32768, where |q|^2 + |x|^2
    reaches 2^30, 2 q.x is negative (wraps as an unsigned) and the distance itself is d * 65025 < 2^31."""
    rng = np.random.default_rng(d)
    rows = [np.full(d, -128, np.int64), np.full(d, 127, np.int64), np.full(d, -1, np.int64), np.zeros(d, np.int64),
            rng.integers(-128, 128, d), np.where(np.arange(d) % 2 == 0, -128, 127)]
    M = 1 << 32
    for q in rows:
        for x in rows:
            nq, nx, dot = int((q * q).sum()), int((x * x).sum()), int((q * x).sum())
            assert nq <= 16384 * d and nx <= 16384 * d and abs(dot) <= 16384 * d < 2 ** 31     # the int32 accumulator holds q.x
            u = lambda v: np.array([v % M], np.uint32)                                         # (uint32 arrays wrap silently)
            got = u(nq) + u(nx) - u(2) * u(dot)                                                # (u(dot): the int32 taken as unsigned)
            want = int(((q - x) ** 2).sum())
            assert want <= d * 65025 < 2 ** 31
            assert int(got[0]) == want, (d, nq, nx, dot)
    assert int(((rows[0] - rows[1]) ** 2).sum()) == d * 65025
    if d == 32768:
        assert 2 * (-128 * 127) * d < -(2 ** 29) and 16384 * d + 16129 * d > 2 ** 29     # the intermediates do leave the result's range


@pytest.fixture(scope="module")
def kernels(pkg, tmp_path_factory):
    """{demangled kernel name: metadata} of the built library's gfx950 code object."""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf not in this image")
    pkg._native.build()
    tmp = tmp_path_factory.mktemp("co_i8")
    so = str(tmp / "libfspann_hip.so")
    shutil.copy(pkg._native._SO, so)
    subprocess.run([OBJDUMP, "--offloading", so], check=True, capture_output=True, cwd=str(tmp))
    objs = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f]
    assert len(objs) == 1, objs
    co = str(tmp / objs[0])
    notes = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, text=True).stdout
    out, blk = {}, {}

    def commit():
        if "name" in blk:
            out[blk.pop("name")] = dict(blk)
        blk.clear()
    for line in notes.splitlines():
        if re.match(r"^  - ", line):
            commit()
        m = re.search(r"\.name:\s+(\S+)", line)
        if m:
            blk["name"] = m.group(1)
        m = re.search(r"\.(private_segment_fixed_size|vgpr_count|sgpr_count|group_segment_fixed_size):\s+(\d+)", line)
        if m:
            blk[m.group(1)] = int(m.group(2))
    commit()
    names = [k for k in out if k.startswith("_Z")]
    dem = subprocess.run(["c++filt"] + [n.replace("DF16_", "Dh") for n in names], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(dem) == len(names)
    return dict(co=co, k={d: dict(out[n], mangled=n) for n, d in zip(names, dem)})


T = "signed char"
# (kernel<template arguments>, dense streaming kernel: must fit four workgroups per CU): the kernels a U8 row reaches, with int8_t
I8_KERNELS = [
    (f"refine_stream_kernel<{T}, float, 128, false, false>", True),      # dense
    (f"refine_stream_kernel<{T}, double, 128, false, false>", True),
    (f"refine_stream_kernel<{T}, float, 128, true, false>", False),      # store gather
    (f"refine_stream_kernel<{T}, double, 128, true, false>", False),
    (f"refine_stream_kernel<{T}, float, 128, false, true>", True),       # runs of chunks (running top-k)
    (f"refine_stream_kernel<{T}, double, 128, false, true>", True),
    (f"refine_stream_list_kernel<{T}, float, 128, true>", False),        # the retry's list mode (store gather)
    (f"refine_stream_list_kernel<{T}, double, 128, true>", False),
    (f"refine_scan_list_kernel<{T}, float, 128, false, true>", False),
    (f"refine_scan_list_kernel<{T}, double, 128, false, true>", False),
    (f"refine_stream_fix_kernel<{T}, false>", True),                     # hand-over, dense
    (f"refine_stream_fix_kernel<{T}, true>", False),                     # hand-over, store gather
    (f"refine_scan_kernel<{T}, float, 128, false, false>", False),       # element-wise path (d % 16 != 0, or rows off 16 bytes)
    (f"refine_scan_kernel<{T}, double, 128, false, true>", False),
    (f"refine_scan_kernel<{T}, float, 128, true, true>", False),
    (f"store_gather_kernel<{T}>", False),
    (f"touch_mark_rows_kernel<float, {T}>", False),
    (f"touch_mark_rows_kernel<double, {T}>", False),
    (f"build_widen_kernel<{T}>", False),
    (f"gt_metrics_kernel<{T}, {T}>", False),
    (f"gt_metrics_kernel<{T}, float>", False),
    (f"gt8_norm_kernel<{T}, true>", False),
    (f"gt8_norm_kernel<{T}, false>", False),
    (f"gt8_dist_kernel<{T}, true>", False),
    (f"gt8_dist_kernel<{T}, false>", False),
]


@pytest.mark.parametrize("frag,dense_stream", I8_KERNELS, ids=[re.sub(r"[^A-Za-z0-9]+", "_", f).strip("_") for f, _ in I8_KERNELS])
def test_i8_kernels_exist_without_scratch(kernels, frag, dense_stream):
    ks = kernels["k"]
    hit = [k for k in ks if ("fspann::" + frag + "(") in k]
    assert len(hit) == 1, (frag, hit)
    md = ks[hit[0]]
    assert md["private_segment_fixed_size"] == 0, md
    if T in frag:                                         # the FSPANN_U8 twin: the same LDS, and registers within the same budget
        u8 = [k for k in ks if ("fspann::" + frag.replace(T, "unsigned char") + "(") in k]
        assert len(u8) == 1, u8
        assert md["group_segment_fixed_size"] == ks[u8[0]]["group_segment_fixed_size"]
    if dense_stream:
        assert md["vgpr_count"] <= 128, md            # 512 / 128 = 4 waves per SIMD: four 256-thread workgroups per CU
        # 36 KB tile (256 rows of 128 + 16 one-byte elements) + static LDS within a quarter of the CU's 160 KB: the U8 geometry
        assert 256 * (128 + 16) * 1 + md["group_segment_fixed_size"] <= 160 * 1024 // 4, md


def test_one_byte_kernel_per_type_and_alignment(kernels):
    """one instantiation of the byte ground-truth kernels per (type, aligned) and one select for both; one hand-over kernel per
    (row type, GATHER), fp32 rows included"""
    ks = kernels["k"]
    for a in ("true", "false"):
        for t in ("unsigned char", T):
            assert len([k for k in ks if f"fspann::gt8_norm_kernel<{t}, {a}>(" in k]) == 1
            assert len([k for k in ks if f"fspann::gt8_dist_kernel<{t}, {a}>(" in k]) == 1
        assert len([k for k in ks if f"fspann::refine_stream_fix_kernel<float, {a}>(" in k]) == 1
        assert len([k for k in ks if f"fspann::refine_stream_fix_kernel<{T}, {a}>(" in k]) == 1
        assert len([k for k in ks if f"fspann::refine_stream_fix_kernel<unsigned char, {a}>(" in k]) == 1
        assert len([k for k in ks if f"fspann::refine_stream_fix_kernel<fspann::fsp_f8e4m3, {a}>(" in k]) == 1
    assert len([k for k in ks if "fspann::gt8_select_kernel(" in k]) == 1
    assert len([k for k in ks if "gt8_norm_kernel<" in k]) == 4 and len([k for k in ks if "gt8_dist_kernel<" in k]) == 4
    assert not [k for k in ks if "gt8s_" in k]                            # no kernel of its own for signed bytes: one selection serves both


def _body(kernels, frag):
    ks = kernels["k"]
    hit = [k for k in ks if ("fspann::" + frag + "(") in k]
    assert len(hit) == 1, (frag, hit)
    sym = ks[hit[0]]["mangled"]
    dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--mcpu=gfx950", f"--disassemble-symbols={sym}", kernels["co"]], check=True,
                         capture_output=True, text=True).stdout
    return [ln.split("//")[0].strip() for ln in dis.splitlines() if ln.startswith("\t")]


@pytest.mark.parametrize("tq", ["float", "double"])
def test_dense_stream_kernel_widens_signed_and_does_not_contract(kernels, tq):
    """A signed byte is widened by a sign-extending extract (v_bfe_i32, or v_ashrrev_i32 for a dword's top byte) and
    v_cvt_f64_i32: no unsigned conversion, no detour through fp32, as many integer-to-fp64 conversions as the U8 kernel of the same
    shape holds, and s = s + d * d is never contracted (no v_fma_f64 in front of the square root's v_rsq_f64)."""
    ins = _body(kernels, f"refine_stream_kernel<{T}, {tq}, 128, false, false>")
    u8 = _body(kernels, f"refine_stream_kernel<unsigned char, {tq}, 128, false, false>")
    assert len(ins) > 200, len(ins)
    ncvt = sum(i.startswith("v_cvt_f64_i32") for i in ins)
    assert ncvt >= 64 and ncvt == sum(i.startswith("v_cvt_f64_u32") for i in u8), ncvt
    assert not [i for i in ins if i.startswith("v_cvt_f64_u32") or i.startswith("v_cvt_f32_ubyte") or i.startswith("v_cvt_f32_i32")]
    ext = sum(i.startswith("v_bfe_i32") or i.startswith("v_ashrrev_i32") for i in ins)
    assert ext >= ncvt, (ext, ncvt)                                  # one sign-extending extract per element
    rsq = [n for n, i in enumerate(ins) if i.startswith("v_rsq_f64")]
    assert len(rsq) == 1, rsq
    fma = [n for n, i in enumerate(ins) if i.startswith("v_fma_f64")]
    assert all(n > rsq[0] for n in fma) and len(fma) == sum(i.startswith("v_fma_f64") for i in u8), fma
    assert sum(i.startswith("v_mul_f64") for i in ins) == sum(i.startswith("v_mul_f64") for i in u8)
    # a signed byte is always finite: no row element is tested (the class tests left are those of the sum and the query, as in U8)
    assert sum(i.startswith("v_cmp_class") for i in ins) == sum(i.startswith("v_cmp_class") for i in u8)
    assert not [i for i in ins if i.startswith("v_cmp_class_f32") or i.startswith("v_cmp_class_f16")]


def test_signed_dist_kernel_runs_on_the_int8_matrix_cores(kernels):
    for a in ("true", "false"):
        ins = _body(kernels, f"gt8_dist_kernel<{T}, {a}>")
        assert len(ins) > 50 and any(i.startswith("v_mfma_i32_32x32x32_i8") for i in ins)
        assert not [i for i in ins if "_f64" in i]
    # the aligned load takes the bytes as they are: the unsigned kernel's flip constant is not in it
    assert not [i for i in _body(kernels, f"gt8_dist_kernel<{T}, true>") if "0x80808080" in i]
    assert [i for i in _body(kernels, "gt8_dist_kernel<unsigned char, true>") if "0x80808080" in i]
