"""CPU: the FSPANN_F16 row type exists in every layer of the ABI (header, ctypes binding, JNI generator and generated Java), and
the built gfx950 code object holds the _Float16 instantiations of every kernel an F16 row can reach — without scratch memory,
the dense streaming ones within the 128 vector registers and the LDS that four workgroups per CU need.  One dense streaming
kernel is disassembled: it widens with v_cvt_f32_f16 and holds no fused fp64 multiply-add (contraction off).  Read from the
code object's kernel metadata, as tests/test_u8_cpu.py does."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_abi_constant_in_every_layer(pkg):
    hdr = open(os.path.join(ROOT, "include", "fspann.h")).read()
    assert re.search(r"^#define\s+FSPANN_F16\s+3\s*$", hdr, re.M)
    assert re.search(r"^#define\s+FSPANN_U8\s+2\s*$", hdr, re.M)
    assert pkg._native.F16 == 3 and (pkg._native.F32, pkg._native.F64, pkg._native.U8) == (0, 1, 2)
    java = open(os.path.join(ROOT, "java", "com", "fspann", "gpu", "FspannNative.java")).read()
    assert re.search(r"\bF16 = 3\b", java) and re.search(r"\bU8 = 2\b", java) and "F32 = 0, F64 = 1" in java
    gen = open(os.path.join(ROOT, "tools", "gen_jni.py")).read()
    assert "F16 = 3" in gen


def test_numpy_wrapper_maps_float16(pkg):
    import numpy as np
    from fspann_amd import engine
    assert engine._dt(np.zeros(1, np.float16)) == pkg._native.F16
    assert engine._dt(np.zeros(1, np.uint8)) == pkg._native.U8
    assert engine._dt(np.zeros(1, np.float32)) == pkg._native.F32


def test_null_context_without_gpu(pkg):
    """the entry points that take the new dtype still look at the context first"""
    N = pkg._native
    pkg._native.build()
    L = N.lib()
    assert L.fspann_store_set(None, 10, None, N.F16) == N.E_NULL
    assert L.fspann_eval_metrics_typed_dev(None, 10, None, N.F16, 2, None, N.F32, 16, 5, None, 5, None, None, 5, None, None) == N.E_NULL


@pytest.fixture(scope="module")
def code_object(pkg, tmp_path_factory):
    """path of the built library's gfx950 code object"""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf not in this image")
    pkg._native.build()
    tmp = tmp_path_factory.mktemp("co_f16")
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
    # a c++filt that does not know the builtin type code DF16_ (_Float16) leaves such names mangled: it is given the older code
    # of the same standing (Dh, printed "half"; builtin types take no part in substitutions) and the name is put right afterwards
    dem = subprocess.run(["c++filt"] + [n.replace("DF16_", "Dh") for n in names], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(dem) == len(names)
    dem = [re.sub(r"\bhalf\b", "_Float16", d) if "DF16_" in n else d for n, d in zip(names, dem)]
    return {d: dict(out[n], mangled=n) for n, d in zip(names, dem)}


# (kernel<template arguments>, dense streaming kernel: must fit four workgroups per CU): the U8_KERNELS of tests/test_u8_cpu.py
# with _Float16 and one 128-byte tile = 64 dims, plus the Setup widening and the metrics kernel
F16_KERNELS = [
    ("refine_stream_kernel<_Float16, float, 64, false, false>", True),      # dense
    ("refine_stream_kernel<_Float16, double, 64, false, false>", True),
    ("refine_stream_kernel<_Float16, float, 64, true, false>", False),      # store gather
    ("refine_stream_kernel<_Float16, double, 64, true, false>", False),
    ("refine_stream_kernel<_Float16, float, 64, false, true>", True),       # runs of chunks (running top-k)
    ("refine_stream_kernel<_Float16, double, 64, false, true>", True),
    ("refine_stream_list_kernel<_Float16, float, 64, true>", False),        # the retry's list mode (store gather)
    ("refine_stream_list_kernel<_Float16, double, 64, true>", False),
    ("refine_scan_list_kernel<_Float16, float, 64, false, true>", False),
    ("refine_scan_list_kernel<_Float16, double, 64, false, true>", False),
    ("refine_stream_fix_kernel<_Float16, false>", True),                    # hand-over, dense
    ("refine_stream_fix_kernel<_Float16, true>", False),                    # hand-over, store gather
    ("refine_scan_kernel<_Float16, float, 64, false, false>", False),       # element-wise path (d % 8 != 0, or rows off 16 bytes)
    ("refine_scan_kernel<_Float16, double, 64, false, true>", False),
    ("refine_scan_kernel<_Float16, float, 64, true, true>", False),
    ("store_gather_kernel<_Float16>", False),
    ("touch_mark_rows_kernel<float, _Float16>", False),
    ("touch_store_valid_kernel<_Float16>", False),
    ("build_widen_kernel<_Float16>", False),
    ("gt_metrics_kernel<_Float16, float>", False),
]


@pytest.mark.parametrize("frag,dense_stream", F16_KERNELS, ids=[re.sub(r"[^A-Za-z0-9]+", "_", f).strip("_") for f, _ in F16_KERNELS])
def test_f16_kernels_exist_without_scratch(kernels, frag, dense_stream):
    hit = [k for k in kernels if ("fspann::" + frag + "(") in k]
    assert len(hit) == 1, (frag, hit)
    md = kernels[hit[0]]
    assert md["private_segment_fixed_size"] == 0, md
    if dense_stream:
        assert md["vgpr_count"] <= 128, md            # 512 / 128 = 4 waves per SIMD: four 256-thread workgroups per CU
        # 36 KB tile (256 rows of 64 + 8 halves) + static LDS within a quarter of the CU's 160 KB
        assert 256 * (64 + 8) * 2 + md["group_segment_fixed_size"] <= 160 * 1024 // 4, md


def test_one_hand_over_kernel_per_row_type(kernels):
    """refine_stream_fix_kernel<row type, GATHER>: exactly one instantiation for fp32, for U8 and for F16 rows, per GATHER"""
    for g in ("true", "false"):
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<float, {g}>(" in k]) == 1
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<unsigned char, {g}>(" in k]) == 1


def _body(kernels, code_object, frag):
    hit = [k for k in kernels if ("fspann::" + frag + "(") in k]
    assert len(hit) == 1, (frag, hit)
    sym = kernels[hit[0]]["mangled"]
    dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--mcpu=gfx950", f"--disassemble-symbols={sym}", code_object], check=True,
                         capture_output=True, text=True).stdout
    return [ln.split("//")[0].strip() for ln in dis.splitlines() if ln.startswith("\t")]


@pytest.mark.parametrize("frag", ["refine_stream_kernel<_Float16, float, 64, false, false>",
                                  "refine_stream_kernel<_Float16, double, 64, false, false>"])
def test_dense_stream_kernel_widens_halves_and_does_not_contract(kernels, code_object, frag):
    """v_cvt_f32_f16 widens, and s = s + d * d is never contracted.  The kernel is not free of v_fma_f64 altogether: the fp64 square
    root behind the scan (QSI.java:371) is expanded by the compiler into v_rsq_f64 and three fused refinement steps, in every row
    type.  So: no v_fma_f64 anywhere in the scan (from the first to the last widening of a half), none in front of the v_rsq_f64,
    and exactly as many in the whole kernel as the fp32 kernel of the same shape holds."""
    ins = _body(kernels, code_object, frag)
    assert len(ins) > 200, len(ins)
    cvt = [n for n, i in enumerate(ins) if i.startswith("v_cvt_f32_f16")]
    assert cvt, "no v_cvt_f32_f16"
    assert any("src0_sel:WORD_1" in ins[n] for n in cvt)           # the high half of a dword: no shift
    assert any(i.startswith("v_cvt_f64_f32") for i in ins)
    scan = ins[cvt[0]:cvt[-1] + 1]
    assert sum(i.startswith("v_add_f64") for i in scan) >= 64 and sum(i.startswith("v_mul_f64") for i in scan) >= 32, "the fp64 chain is not in the scan"
    assert not [i for i in scan if i.startswith("v_fma_f64")]      # s = s + d * d stays a multiply and an add (QSI.l2's rounding)
    fma = [n for n, i in enumerate(ins) if i.startswith("v_fma_f64")]
    rsq = [n for n, i in enumerate(ins) if i.startswith("v_rsq_f64")]
    assert len(rsq) == 1 and all(n > rsq[0] for n in fma), (rsq, fma)
    f32 = _body(kernels, code_object, "refine_stream_kernel<float, float, 32, false, false>")
    assert len(fma) == sum(i.startswith("v_fma_f64") for i in f32)
    assert not [i for i in ins if i.startswith("scratch_")]
    if ", double," in frag:                                        # an fp64 query: every raw half is tested (QSI.isValid)
        assert any(i.startswith("v_cmp_class_f16") for i in ins)
