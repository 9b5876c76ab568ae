"""CPU: the FSPANN_F8E4M3 row type (OCP fp8 e4m3fn) exists in every layer of the ABI (header, ctypes binding, JNI generator and
generated Java), the numpy wrapper takes fp8 rows without ever rounding them (a torch.float8_e4m3fn tensor, uint8 bit patterns
given with the marker, or floats that already are e4m3 values), and the built gfx950 code object holds the fsp_f8e4m3
instantiations of every kernel an fp8 row can reach — without scratch memory, the dense streaming ones within the 128 vector
registers and the LDS that four workgroups per CU need.  The dense streaming kernels are disassembled: they widen with the
hardware's fp8 conversion and v_cvt_f64_f32 and hold no fused fp64 multiply-add in the scan.  Expected values come from a 256-entry table
built here from the format's definition (S EEEE MMM, bias 7), not from library code; torch's own cast is a second witness."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def e4m3_table():
    """value of each of the 256 patterns, from the definition: E = 0: +-M/8 * 2^-6; E = 1..15: +-(1 + M/8) * 2^(E-7); 0x7F / 0xFF NaN"""
    t = np.empty(256, np.float64)
    for b in range(256):
        s, e, m = b >> 7, (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = (m / 8.0) * 2.0 ** -6
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = -v if s else v
    return t


TABLE = e4m3_table()
FINITE = np.array([b for b in range(256) if (b & 0x7F) != 0x7F], np.uint8)


def test_table_is_the_format():
    assert len(FINITE) == 254 and TABLE[0x7E] == 448.0 and TABLE[0x01] == 2.0 ** -9 and TABLE[0xFE] == -448.0
    assert TABLE[0x80] == 0.0 and np.signbit(TABLE[0x80]) and np.isnan(TABLE[0x7F]) and np.isnan(TABLE[0xFF])
    assert np.all(TABLE[FINITE] * 512 == np.floor(TABLE[FINITE] * 512))            # multiples of 2^-9
    assert np.array_equal(TABLE[FINITE].astype(np.float16).astype(np.float64), TABLE[FINITE])     # e4m3 is a subset of fp16
    import torch
    tt = torch.from_numpy(np.arange(256, dtype=np.uint8)).view(torch.float8_e4m3fn).to(torch.float32).numpy().astype(np.float64)
    assert np.array_equal(tt[FINITE], TABLE[FINITE]) and np.array_equal(np.signbit(tt[FINITE]), np.signbit(TABLE[FINITE]))
    assert np.isnan(tt[0x7F]) and np.isnan(tt[0xFF])


def test_abi_constant_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "fspann.h")).read()
    assert re.search(r"^#define\s+FSPANN_F8E4M3\s+5\s*$", hdr, re.M)
    assert re.search(r"^#define\s+FSPANN_BF16\s+4\s*$", hdr, re.M)
    N = pkg._native
    assert N.F8E4M3 == 5 and (N.F32, N.F64, N.U8, N.F16, N.BF16) == (0, 1, 2, 3, 4)
    java = open(os.path.join(ROOT, "java", "com", "fspann", "gpu", "FspannNative.java")).read()
    assert re.search(r"\bF8E4M3 = 5\b", java) and re.search(r"\bBF16 = 4\b", java)
    gen = open(os.path.join(ROOT, "tools", "gen_jni.py")).read()
    assert "F8E4M3 = 5" in gen
    names = open(os.path.join(ROOT, "jni", "bound_symbols.txt")).read().split()
    assert len(names) == 94                              # no entry point is added


def test_marker_is_exported(pkg):
    from fspann_amd import engine
    assert pkg.float8_e4m3fn is engine.float8_e4m3fn and repr(pkg.float8_e4m3fn) == "float8_e4m3fn"
    assert pkg.float8_e4m3fn is not pkg.bfloat16 and not (pkg.float8_e4m3fn == np.uint8)
    # without the marker nothing changes: a uint8 array is FSPANN_U8, and a uint16 array is still nothing
    assert engine._dt(np.zeros(1, np.uint8)) == pkg._native.U8
    with pytest.raises(pkg.FspannArgumentError):
        engine._dt(np.zeros(1, np.uint16))


def test_null_context_without_gpu(pkg):
    """the entry points that take the new dtype still look at the context first"""
    N = pkg._native
    pkg._native.build()
    L = N.lib()
    assert L.fspann_store_set(None, 10, None, N.F8E4M3) == N.E_NULL
    assert L.fspann_store_attach_dev(None, 10, None, N.F8E4M3) == N.E_NULL
    assert L.fspann_build_index(None, 10, None, N.F8E4M3, None) == N.E_NULL
    assert L.fspann_build_append(None, 10, None, N.F8E4M3) == N.E_NULL
    assert L.fspann_encode(None, 1, None, N.F8E4M3, None, None) == N.E_NULL
    assert L.fspann_eval_metrics_typed_dev(None, 10, None, N.F8E4M3, 2, None, N.F32, 16, 5, None, 5, None, None, 5, None, None) == N.E_NULL


def test_wrapper_takes_all_256_patterns_as_they_are(pkg):
    from fspann_amd.engine import _f8_bits
    bits = np.arange(256, dtype=np.uint8).reshape(16, 16)
    out = _f8_bits(bits, "store_set")
    assert out.dtype == np.uint8 and np.array_equal(out, bits)
    for dt in (np.int8, np.int16, np.int64, np.uint16):       # other integer arrays are neither bits nor floats
        with pytest.raises(pkg.FspannArgumentError, match="float8_e4m3fn"):
            _f8_bits(np.zeros((2, 16), dt), "store_set")


@pytest.mark.parametrize("dt", [np.float16, np.float32, np.float64])
def test_wrapper_takes_exact_values_and_never_rounds(pkg, dt):
    """_f8_bits is what store_set / build_index / build_append(dtype=float8_e4m3fn) hand to the library: it raises before anything is
    touched, so a store set before stays as it was (the GPU test checks that on a live context)."""
    from fspann_amd.engine import _f8_bits
    E = pkg.FspannArgumentError
    # every finite value of the table, in this float type, comes back as its own pattern (-0.0 as 0x80, 2^-9 as 0x01, +-448 as 0x7E / 0xFE)
    got = _f8_bits(TABLE[FINITE].astype(dt), "store_set")
    assert got.dtype == np.uint8 and np.array_equal(got, FINITE)
    spec = np.array([2.0 ** -9, 448.0, -448.0, -0.0, 0.0, np.nan], dt)
    assert _f8_bits(spec, "store_set").tolist() == [0x01, 0x7E, 0xFE, 0x80, 0x00, 0x7F]
    # refused: not e4m3 values, out of range, and the infinities the format does not have
    for bad in (0.1, 1.0 + 2.0 ** -4, 2.0 ** -10, 449.0, 1e6, np.inf, -np.inf, 480.0, 3.0 * 2.0 ** -10):
        with np.errstate(over="ignore"):
            y = np.full((4, 16), 0.5, dt)
            y[2, 5] = bad
        if dt == np.float16 and bad == 1e6:
            assert np.isinf(y[2, 5])
        with pytest.raises(E, match="float8_e4m3fn"):
            _f8_bits(y, "store_set")


def test_wrapper_takes_a_torch_float8_tensor(pkg):
    import torch
    from fspann_amd.engine import _f8_bits
    x = torch.tensor([[0.5, -2.0, 448.0, 2.0 ** -9, -0.0, 0.1, 1e6, 17.3]], dtype=torch.float32)
    t = x.to(torch.float8_e4m3fn)                                       # torch rounds here: the CALLER's rounding
    got = _f8_bits(t, "store_set")
    assert got.dtype == np.uint8 and got.shape == (1, 8)
    assert np.array_equal(got, t.view(torch.uint8).numpy())             # the tensor's own bytes
    want = t.to(torch.float32).numpy().astype(np.float64)
    assert np.array_equal(TABLE[got], want, equal_nan=True)             # and the table says what torch says
    assert got[0, :5].tolist() == [0x30, 0xC0, 0x7E, 0x01, 0x80]
    assert (got[0, 6] & 0x7F) == 0x7F                                   # torch does not saturate: 1e6 became NaN
    nc = torch.zeros((4, 32), dtype=torch.float8_e4m3fn)[:, ::2]        # not contiguous: copied, not refused
    assert _f8_bits(nc, "store_set").shape == (4, 16)
    for other in (x, x.to(torch.float16), x.to(torch.bfloat16), torch.zeros((1, 16), dtype=torch.float8_e5m2)):
        with pytest.raises(pkg.FspannArgumentError, match="float8_e4m3fn"):
            _f8_bits(other, "store_set")                                # a tensor of another type is not fp8 rows


def test_dtype_messages_keep_their_words(pkg):
    """build_index / build_append(dtype=<anything else>) still name the bfloat16 marker, and now the fp8 one"""
    from fspann_amd import engine
    src = open(engine.__file__).read()
    for fn in ("build_index", "build_append"):
        m = re.search(fn + r"\(dtype=\): only the ([^\"]*)\"", src)
        assert m and "bfloat16" in m.group(1) and "float8_e4m3fn" in m.group(1)


@pytest.fixture(scope="module")
def code_object(pkg, tmp_path_factory):
    """path of the built library's gfx950 code object"""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf not in this image")
    pkg._native.build()
    tmp = tmp_path_factory.mktemp("co_f8")
    so = str(tmp / "libfspann_hip.so")
    shutil.copy(pkg._native._SO, so)
    subprocess.run([OBJDUMP, "--offloading", so], check=True, capture_output=True, cwd=str(tmp))
    objs = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f]
    assert len(objs) == 1, objs
    return str(tmp / objs[0])


@pytest.fixture(scope="module")
def kernels(code_object):
    """{demangled kernel name: metadata} of the code object."""
    notes = subprocess.run([READELF, "--notes", code_object], check=True, capture_output=True, text=True).stdout
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
    return {d: dict(out[n], mangled=n) for n, d in zip(names, dem)}


def test_no_kernel_uses_scratch(kernels):
    assert len(kernels) > 250
    assert not {k: v for k, v in kernels.items() if v["private_segment_fixed_size"] != 0}


T = "fspann::fsp_f8e4m3"
# (kernel<template arguments>, dense streaming kernel: must fit four workgroups per CU): the BF16_KERNELS of tests/test_bf16_cpu.py
# with the fp8 row type (the byte geometry of FSPANN_U8: one 128-byte tile = 128 dims), its Setup widening and its metrics kernel
F8_KERNELS = [
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
    (f"touch_store_valid_kernel<{T}>", False),
    (f"build_widen_kernel<{T}>", False),
    (f"gt_metrics_kernel<{T}, float>", False),
]


@pytest.mark.parametrize("frag,dense_stream", F8_KERNELS, ids=[re.sub(r"[^A-Za-z0-9]+", "_", f).strip("_") for f, _ in F8_KERNELS])
def test_f8_kernels_exist_without_scratch(kernels, frag, dense_stream):
    hit = [k for k in kernels if ("fspann::" + frag + "(") in k]
    assert len(hit) == 1, (frag, hit)
    md = kernels[hit[0]]
    assert md["private_segment_fixed_size"] == 0, md
    if dense_stream:
        assert md["vgpr_count"] <= 128, md            # 512 / 128 = 4 waves per SIMD: four 256-thread workgroups per CU
        # 36 KB tile (256 rows of 128 + 16 one-byte elements) + static LDS within a quarter of the CU's 160 KB: the U8 geometry
        assert 256 * (128 + 16) * 1 + md["group_segment_fixed_size"] <= 160 * 1024 // 4, md
        u8 = [k for k in kernels if ("fspann::" + frag.replace(T, "unsigned char") + "(") in k]
        assert len(u8) == 1, u8
        assert md["group_segment_fixed_size"] == kernels[u8[0]]["group_segment_fixed_size"]


def test_one_hand_over_kernel_per_row_type(kernels):
    """refine_stream_fix_kernel<row type, GATHER>: exactly one instantiation for fp32, for U8, for BF16 and for F8E4M3 rows, per GATHER"""
    for g in ("true", "false"):
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<float, {g}>(" in k]) == 1
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<unsigned char, {g}>(" in k]) == 1
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<fspann::fsp_bf16, {g}>(" in k]) == 1
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<{T}, {g}>(" in k]) == 1


def _body(kernels, code_object, frag):
    hit = [k for k in kernels if ("fspann::" + frag + "(") in k]
    assert len(hit) == 1, (frag, hit)
    sym = kernels[hit[0]]["mangled"]
    dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--mcpu=gfx950", f"--disassemble-symbols={sym}", code_object], check=True,
                         capture_output=True, text=True).stdout
    return [ln.split("//")[0].strip() for ln in dis.splitlines() if ln.startswith("\t")]


@pytest.mark.parametrize("frag", [f"refine_stream_kernel<{T}, float, 128, false, false>",
                                  f"refine_stream_kernel<{T}, double, 128, false, false>"])
def test_dense_stream_kernel_widens_in_hardware_and_does_not_contract(kernels, code_object, frag):
    """An fp8 pair is widened by v_cvt_pk_f32_fp8 (the variant kept: one instruction per two elements, the high word of a dword
    through SDWA) and each element by v_cvt_f64_f32: no byte extract, no integer conversion, no v_cvt_f32_f16, and s = s + d * d is
    never contracted.  As in every row type, the fp64 square root behind the scan (QSI.java:371) is expanded into v_rsq_f64 and
    three fused refinement steps: no v_fma_f64 in the scan (from the first to the last v_cvt_f64_f32 in front of the v_rsq_f64),
    none in front of the v_rsq_f64, and exactly as many in the whole kernel as the fp32 kernel of the same shape holds."""
    ins = _body(kernels, code_object, frag)
    assert len(ins) > 200, len(ins)
    assert not [i for i in ins if i.startswith("v_cvt_f32_f16") or i.startswith("v_cvt_f64_u32") or i.startswith("v_cvt_f32_ubyte")
                or i.startswith("v_cvt_f32_bf8") or i.startswith("v_cvt_pk_f32_bf8")]
    rsq = [n for n, i in enumerate(ins) if i.startswith("v_rsq_f64")]
    assert len(rsq) == 1, rsq
    cvt = [n for n, i in enumerate(ins) if i.startswith("v_cvt_f64_f32") and n < rsq[0]]
    assert len(cvt) >= 64, len(cvt)                                  # one per row element of an unrolled pass (an fp32 query's too)
    scan = ins[cvt[0] - 1:cvt[-1] + 1]
    pk = [i for i in scan if i.startswith("v_cvt_pk_f32_fp8")]
    assert len(pk) >= 32, len(pk)                                    # one per two elements: four 16-byte slots = 64 elements at least
    assert any("src0_sel:WORD_1" in i for i in pk) and any("sdwa" not in i for i in pk)     # both words of a dword
    assert not [i for i in scan if i.startswith("v_cvt_f32_fp8")]  # (the one-per-element conversion is a build switch, not the default)
    assert sum(i.startswith("v_add_f64") for i in scan) >= 128 and sum(i.startswith("v_mul_f64") for i in scan) >= 64, "the fp64 chain is not in the scan"
    assert not [i for i in scan if i.startswith("v_fma_f64")]      # s = s + d * d stays a multiply and an add (QSI.l2's rounding)
    fma = [n for n, i in enumerate(ins) if i.startswith("v_fma_f64")]
    assert all(n > rsq[0] for n in fma), (rsq, fma)
    f32 = _body(kernels, code_object, "refine_stream_kernel<float, float, 32, false, false>")
    assert len(fma) == sum(i.startswith("v_fma_f64") for i in f32) == 3
    assert not [i for i in ins if i.startswith("scratch_")]
    assert not [i for i in scan if i.startswith("v_cmp_class")]   # no class test: an fp32 query's sum tells, and ...
    masks = [i for i in scan if i.startswith("v_and_b32") and "0x7f7f7f7f" in i]
    if ", double," in frag:                                        # ... against an fp64 query every element is tested (QSI.isValid), four
        assert len(masks) >= 16, len(masks)                        # at once on their dword: (w & 0x7f7f7f7f) + 0x01010101 carries into a
        assert any("0x1010101" in i for i in scan)                 # byte's top bit iff the byte is a NaN pattern
    else:
        assert not masks
