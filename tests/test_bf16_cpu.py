"""CPU: the FSPANN_BF16 row type exists in every layer of the ABI (header, ctypes binding, JNI generator and generated Java), the
numpy wrapper takes bfloat16 rows without ever rounding them (a torch.bfloat16 tensor, uint16 bit patterns, or floats that already
are bfloat16 values), and the built gfx950 code object holds the fsp_bf16 instantiations of every kernel a BF16 row can reach —
without scratch memory, the dense streaming ones within the 128 vector registers and the LDS that four workgroups per CU need.
One dense streaming kernel is disassembled: it widens with integer operations and v_cvt_f64_f32 only (no v_cvt_f32_f16, nothing
that could round) and holds no fused fp64 multiply-add in the scan.  Read from the code object's kernel metadata, as
tests/test_f16_cpu.py does."""
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
    assert re.search(r"^#define\s+FSPANN_BF16\s+4\s*$", hdr, re.M)
    assert re.search(r"^#define\s+FSPANN_F16\s+3\s*$", hdr, re.M)
    N = pkg._native
    assert N.BF16 == 4 and (N.F32, N.F64, N.U8, N.F16) == (0, 1, 2, 3)
    java = open(os.path.join(ROOT, "java", "com", "fspann", "gpu", "FspannNative.java")).read()
    assert re.search(r"\bBF16 = 4\b", java) and re.search(r"\bF16 = 3\b", java) and "F32 = 0, F64 = 1" in java
    gen = open(os.path.join(ROOT, "tools", "gen_jni.py")).read()
    assert "BF16 = 4" in gen
    names = open(os.path.join(ROOT, "jni", "bound_symbols.txt")).read().split()
    assert len(names) == 94                              # no entry point is added


def test_marker_is_exported(pkg):
    from fspann_amd import engine
    assert pkg.bfloat16 is engine.bfloat16 and repr(pkg.bfloat16) == "bfloat16"
    assert not (pkg.bfloat16 == np.float16) and not (pkg.bfloat16 == np.float32)
    # the array-typed rows keep their mapping: numpy has no bfloat16, so nothing maps to BF16 by its array type
    assert engine._dt(np.zeros(1, np.float16)) == pkg._native.F16
    with pytest.raises(pkg.FspannArgumentError):
        engine._dt(np.zeros(1, np.uint16))


def test_null_context_without_gpu(pkg):
    """the entry points that take the new dtype still look at the context first"""
    N = pkg._native
    pkg._native.build()
    L = N.lib()
    assert L.fspann_store_set(None, 10, None, N.BF16) == N.E_NULL
    assert L.fspann_eval_metrics_typed_dev(None, 10, None, N.BF16, 2, None, N.F32, 16, 5, None, 5, None, None, 5, None, None) == N.E_NULL


def _f32(bits16):
    return (np.asarray(bits16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def test_wrapper_takes_exact_values_and_never_rounds(pkg):
    """_bf16_bits is what store_set / build_index / build_append(dtype=bfloat16) hand to the library: it raises before anything is
    touched, so a store set before stays as it was (the GPU test checks that on a live context)."""
    from fspann_amd.engine import _bf16_bits
    E = pkg.FspannArgumentError
    # exact values, as float32 and float64 and float16
    vals = np.array([0.5, 1.0, -3.0, 2.0 ** 33, 2.0 ** -130, 1.0 + 2.0 ** -7, -255.0, 3.3895313892515355e38], np.float64)
    want = (vals.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(_f32(want).astype(np.float64), vals)          # (they are bfloat16 values)
    for dt in (np.float32, np.float64):
        got = _bf16_bits(vals.astype(dt), "store_set")
        assert got.dtype == np.uint16 and np.array_equal(got, want), dt
    assert np.array_equal(_bf16_bits(np.array([0.5, -2.0, 1.5], np.float16), "store_set"), np.array([0x3F00, 0xC000, 0x3FC0], np.uint16))
    # refused: 0.1f, 1 + 2^-8, an fp64 value that is not an fp32, a half with more than eight significant bits, and out of range
    for bad in (np.float32(0.1), np.float32(1.0 + 2.0 ** -8), np.float64(1.0) + 2.0 ** -30, np.float64(0.1), np.float16(1.0 + 2.0 ** -10),
                np.float64(1e300), np.float64(2.0 ** -150), np.float32(1e10)):
        y = np.full((4, 8), 0.5, np.asarray(bad).dtype)
        y[2, 5] = bad
        with pytest.raises(E, match="bfloat16"):
            _bf16_bits(y, "store_set")
    # subnormals, +-inf, NaN and -0.0 pass, bit for bit
    spec = np.array([2.0 ** -133, -(2.0 ** -127), np.inf, -np.inf, np.nan, -0.0, 0.0], np.float32)
    got = _bf16_bits(spec, "store_set")
    assert got.tolist()[:4] == [0x0001, 0x8040, 0x7F80, 0xFF80] and got.tolist()[5:] == [0x8000, 0x0000]
    assert (got[4] & 0x7F80) == 0x7F80 and (got[4] & 0x7F) != 0        # NaN stays NaN
    lownan = np.array([0x7F800001], np.uint32).view(np.float32)         # a NaN whose payload sits in the low 16 bits only
    g = _bf16_bits(lownan, "store_set")
    assert (g[0] & 0x7F80) == 0x7F80 and (g[0] & 0x7F) != 0
    assert np.array_equal(_bf16_bits(spec.astype(np.float64), "store_set")[[0, 1, 2, 3, 5, 6]], got[[0, 1, 2, 3, 5, 6]])
    # a uint16 array is taken as bits, whatever they are
    bits = np.array([[0x0001, 0x7F7F, 0x7F80, 0xFFC1, 0x8000, 0x3DCD]], np.uint16)
    out = _bf16_bits(bits, "store_set")
    assert out.dtype == np.uint16 and np.array_equal(out, bits)
    # other integer arrays are neither bits nor floats
    for dt in (np.int16, np.int64, np.uint8):
        with pytest.raises(E):
            _bf16_bits(np.zeros((2, 8), dt), "store_set")


def test_wrapper_takes_a_torch_bfloat16_tensor(pkg):
    import torch
    from fspann_amd.engine import _bf16_bits
    x = torch.tensor([[0.5, -2.0, 1e10, float("inf"), -0.0, 0.1]], dtype=torch.float32)
    t = x.to(torch.bfloat16)                                            # torch rounds here: the CALLER's rounding
    got = _bf16_bits(t, "store_set")
    assert got.dtype == np.uint16 and got.shape == (1, 6)
    assert np.array_equal(_f32(got), t.to(torch.float32).numpy())       # the tensor's values, bit for bit
    assert got[0, 4] == 0x8000 and got[0, 3] == 0x7F80
    nc = torch.zeros((4, 6), dtype=torch.bfloat16)[:, ::2]              # not contiguous: copied, not refused
    assert _bf16_bits(nc, "store_set").shape == (4, 3)
    with pytest.raises(pkg.FspannArgumentError):
        _bf16_bits(x, "store_set")                                      # a float32 tensor is not bfloat16 rows
    with pytest.raises(pkg.FspannArgumentError):
        _bf16_bits(x.to(torch.float16), "store_set")


@pytest.fixture(scope="module")
def code_object(pkg, tmp_path_factory):
    """path of the built library's gfx950 code object"""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf not in this image")
    pkg._native.build()
    tmp = tmp_path_factory.mktemp("co_bf16")
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
    # (a c++filt that does not know DF16_ leaves the _Float16 kernels mangled: tests/test_f16_cpu.py; the type here is a struct)
    dem = subprocess.run(["c++filt"] + [n.replace("DF16_", "Dh") for n in names], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(dem) == len(names)
    return {d: dict(out[n], mangled=n) for n, d in zip(names, dem)}


T = "fspann::fsp_bf16"
# (kernel<template arguments>, dense streaming kernel: must fit four workgroups per CU): the F16_KERNELS of tests/test_f16_cpu.py
# with the bfloat16 row type (one 128-byte tile = 64 dims), its Setup widening and its metrics kernel
BF16_KERNELS = [
    (f"refine_stream_kernel<{T}, float, 64, false, false>", True),      # dense
    (f"refine_stream_kernel<{T}, double, 64, false, false>", True),
    (f"refine_stream_kernel<{T}, float, 64, true, false>", False),      # store gather
    (f"refine_stream_kernel<{T}, double, 64, true, false>", False),
    (f"refine_stream_kernel<{T}, float, 64, false, true>", True),       # runs of chunks (running top-k)
    (f"refine_stream_kernel<{T}, double, 64, false, true>", True),
    (f"refine_stream_list_kernel<{T}, float, 64, true>", False),        # the retry's list mode (store gather)
    (f"refine_stream_list_kernel<{T}, double, 64, true>", False),
    (f"refine_scan_list_kernel<{T}, float, 64, false, true>", False),
    (f"refine_scan_list_kernel<{T}, double, 64, false, true>", False),
    (f"refine_stream_fix_kernel<{T}, false>", True),                    # hand-over, dense
    (f"refine_stream_fix_kernel<{T}, true>", False),                    # hand-over, store gather
    (f"refine_scan_kernel<{T}, float, 64, false, false>", False),       # element-wise path (d % 8 != 0, or rows off 16 bytes)
    (f"refine_scan_kernel<{T}, double, 64, false, true>", False),
    (f"refine_scan_kernel<{T}, float, 64, true, true>", False),
    (f"store_gather_kernel<{T}>", False),
    (f"touch_mark_rows_kernel<float, {T}>", False),
    (f"touch_mark_rows_kernel<double, {T}>", False),
    (f"touch_store_valid_kernel<{T}>", False),
    (f"build_widen_kernel<{T}>", False),
    (f"gt_metrics_kernel<{T}, float>", False),
]


@pytest.mark.parametrize("frag,dense_stream", BF16_KERNELS, ids=[re.sub(r"[^A-Za-z0-9]+", "_", f).strip("_") for f, _ in BF16_KERNELS])
def test_bf16_kernels_exist_without_scratch(kernels, frag, dense_stream):
    hit = [k for k in kernels if ("fspann::" + frag + "(") in k]
    assert len(hit) == 1, (frag, hit)
    md = kernels[hit[0]]
    assert md["private_segment_fixed_size"] == 0, md
    if dense_stream:
        assert md["vgpr_count"] <= 128, md            # 512 / 128 = 4 waves per SIMD: four 256-thread workgroups per CU
        # 36 KB tile (256 rows of 64 + 8 two-byte elements) + static LDS within a quarter of the CU's 160 KB: the F16 geometry
        assert 256 * (64 + 8) * 2 + md["group_segment_fixed_size"] <= 160 * 1024 // 4, md
        f16 = [k for k in kernels if ("fspann::" + frag.replace(T, "_Float16") + "(") in k or ("fspann::" + frag.replace(T, "half") + "(") in k]
        assert len(f16) == 1, f16
        assert md["group_segment_fixed_size"] == kernels[f16[0]]["group_segment_fixed_size"]


def test_one_hand_over_kernel_per_row_type(kernels):
    """refine_stream_fix_kernel<row type, GATHER>: exactly one instantiation for fp32, for U8 and for BF16 rows, per GATHER"""
    for g in ("true", "false"):
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<float, {g}>(" in k]) == 1
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<unsigned char, {g}>(" in k]) == 1
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<{T}, {g}>(" in k]) == 1


def _body(kernels, code_object, frag):
    hit = [k for k in kernels if ("fspann::" + frag + "(") in k]
    assert len(hit) == 1, (frag, hit)
    sym = kernels[hit[0]]["mangled"]
    dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--mcpu=gfx950", f"--disassemble-symbols={sym}", code_object], check=True,
                         capture_output=True, text=True).stdout
    return [ln.split("//")[0].strip() for ln in dis.splitlines() if ln.startswith("\t")]


@pytest.mark.parametrize("frag", [f"refine_stream_kernel<{T}, float, 64, false, false>",
                                  f"refine_stream_kernel<{T}, double, 64, false, false>"])
def test_dense_stream_kernel_widens_by_shifting_and_does_not_contract(kernels, code_object, frag):
    """A bfloat16 is widened by an integer operation on its dword (v_lshlrev_b32 by 16 for the low element, v_and_b32 with 0xffff0000
    for the high one) and v_cvt_f64_f32: the kernel holds no v_cvt_f32_f16 and no other conversion to fp32 that could round, and
    s = s + d * d is never contracted.  As in every row type, the fp64 square root behind the scan (QSI.java:371) is expanded into
    v_rsq_f64 and three fused refinement steps: no v_fma_f64 in the scan (from the first to the last v_cvt_f64_f32 in front of the
    v_rsq_f64), none in front of the v_rsq_f64, and exactly as many in the whole kernel as the fp32 kernel of the same shape holds."""
    ins = _body(kernels, code_object, frag)
    assert len(ins) > 200, len(ins)
    assert not [i for i in ins if i.startswith("v_cvt_f32_f16") or i.startswith("v_cvt_f16") or i.startswith("v_cvt_f32_bf16")
                or i.startswith("v_cvt_pk")]
    rsq = [n for n, i in enumerate(ins) if i.startswith("v_rsq_f64")]
    assert len(rsq) == 1, rsq
    cvt = [n for n, i in enumerate(ins) if i.startswith("v_cvt_f64_f32") and n < rsq[0]]
    assert len(cvt) >= 32, len(cvt)                                  # one per row element of an unrolled pass (an fp32 query's too)
    scan = ins[cvt[0]:cvt[-1] + 1]
    assert any(re.match(r"v_lshlrev_b32(_e32|_e64)? v\d+, 16, v\d+", i) for i in scan), "no dword << 16 in the scan"
    assert any(i.startswith("v_and_b32") and "0xffff0000" in i for i in scan), "no dword & 0xffff0000 in the scan"
    assert sum(i.startswith("v_add_f64") for i in scan) >= 64 and sum(i.startswith("v_mul_f64") for i in scan) >= 32, "the fp64 chain is not in the scan"
    assert not [i for i in scan if i.startswith("v_fma_f64")]      # s = s + d * d stays a multiply and an add (QSI.l2's rounding)
    fma = [n for n, i in enumerate(ins) if i.startswith("v_fma_f64")]
    assert all(n > rsq[0] for n in fma), (rsq, fma)
    f32 = _body(kernels, code_object, "refine_stream_kernel<float, float, 32, false, false>")
    assert len(fma) == sum(i.startswith("v_fma_f64") for i in f32) == 3
    assert not [i for i in ins if i.startswith("scratch_")]
    if ", double," in frag:                                        # an fp64 query: every raw element is tested (QSI.isValid) — its exponent
        # field is the widened float's, so the test is v_cmp_class_f32 on the float the shift has made, one per element of a tile pass
        assert sum(i.startswith("v_cmp_class_f32") for i in scan) >= 32
        assert not [i for i in ins if i.startswith("v_cmp_class_f16")]
    else:                                                          # an fp32 query: the sum tells, no element is tested
        assert not [i for i in scan if i.startswith("v_cmp_class")]
