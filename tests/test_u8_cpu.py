"""CPU: the FSPANN_U8 row type exists in every layer of the ABI (header, ctypes binding, generated JNI binding), and the built
gfx950 code object holds the uint8_t instantiations of every kernel a U8 row can reach — without scratch memory, the dense
streaming ones within the 128 vector registers that four workgroups per CU need.  Read from the code object's kernel metadata,
as tests/test_route_residency.py does."""
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
    assert re.search(r"^#define\s+FSPANN_U8\s+2\s*$", hdr, re.M)
    assert re.search(r"^#define\s+FSPANN_F32\s+0\s*$", hdr, re.M) and re.search(r"^#define\s+FSPANN_F64\s+1\s*$", hdr, re.M)
    assert pkg._native.U8 == 2 and (pkg._native.F32, pkg._native.F64) == (0, 1)
    java = open(os.path.join(ROOT, "java", "com", "fspann", "gpu", "FspannNative.java")).read()
    assert re.search(r"\bU8 = 2\b", java) and "F32 = 0, F64 = 1" in java
    gen = open(os.path.join(ROOT, "tools", "gen_jni.py")).read()
    assert "U8 = 2" in gen


def test_numpy_wrapper_maps_uint8(pkg):
    import numpy as np
    from fspann_amd import engine
    assert engine._dt(np.zeros(1, np.uint8)) == pkg._native.U8
    with pytest.raises(pkg.FspannArgumentError):
        engine._dt(np.zeros(1, np.int8))            # signed bytes are not a row type


@pytest.fixture(scope="module")
def kernels(pkg, tmp_path_factory):
    """{demangled kernel name: metadata} of the built library's gfx950 code object."""
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf not in this image")
    pkg._native.build()
    tmp = tmp_path_factory.mktemp("co_u8")
    so = str(tmp / "libfspann_hip.so")
    shutil.copy(pkg._native._SO, so)
    subprocess.run([OBJDUMP, "--offloading", so], check=True, capture_output=True, cwd=str(tmp))
    objs = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f]
    assert len(objs) == 1, objs
    notes = subprocess.run([READELF, "--notes", str(tmp / objs[0])], check=True, capture_output=True, text=True).stdout
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
    dem = subprocess.run(["c++filt"] + names, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(dem) == len(names)
    return {d: out[n] for n, d in zip(names, dem)}


# (kernel<template arguments>, dense streaming kernel: must fit four workgroups per CU)
U8_KERNELS = [
    ("refine_stream_kernel<unsigned char, float, 128, false, false>", True),      # dense
    ("refine_stream_kernel<unsigned char, double, 128, false, false>", True),
    ("refine_stream_kernel<unsigned char, float, 128, true, false>", False),      # store gather
    ("refine_stream_kernel<unsigned char, double, 128, true, false>", False),
    ("refine_stream_kernel<unsigned char, float, 128, false, true>", True),       # runs of chunks (running top-k)
    ("refine_stream_kernel<unsigned char, double, 128, false, true>", True),
    ("refine_stream_list_kernel<unsigned char, float, 128, true>", False),        # the retry's list mode (store gather)
    ("refine_stream_list_kernel<unsigned char, double, 128, true>", False),
    ("refine_scan_list_kernel<unsigned char, float, 128, false, true>", False),
    ("refine_scan_list_kernel<unsigned char, double, 128, false, true>", False),
    ("refine_stream_fix_kernel<unsigned char, false>", True),                     # hand-over, dense
    ("refine_stream_fix_kernel<unsigned char, true>", False),                     # hand-over, store gather
    ("refine_scan_kernel<unsigned char, float, 128, false, false>", False),       # element-wise path (d % 16 != 0)
    ("refine_scan_kernel<unsigned char, double, 128, false, true>", False),
    ("refine_scan_kernel<unsigned char, float, 128, true, true>", False),
    ("store_gather_kernel<unsigned char>", False),
    ("touch_mark_rows_kernel<float, unsigned char>", False),
    ("build_widen_kernel<unsigned char>", False),
]


@pytest.mark.parametrize("frag,dense_stream", U8_KERNELS, ids=[re.sub(r"[^A-Za-z0-9]+", "_", f).strip("_") for f, _ in U8_KERNELS])
def test_u8_kernels_exist_without_scratch(kernels, frag, dense_stream):
    hit = [k for k in kernels if ("fspann::" + frag + "(") in k]
    assert len(hit) == 1, (frag, hit)
    md = kernels[hit[0]]
    assert md["private_segment_fixed_size"] == 0, md
    if dense_stream:
        assert md["vgpr_count"] <= 128, md            # 512 / 128 = 4 waves per SIMD: four 256-thread workgroups per CU
        assert 256 * (128 + 16) + md["group_segment_fixed_size"] <= 160 * 1024 // 4, md    # 36 KB tile + static LDS


def test_one_hand_over_kernel_per_row_type(kernels):
    """refine_stream_fix_kernel<row type, GATHER>: exactly one instantiation for fp32 rows and one for U8 rows, per GATHER"""
    for g in ("true", "false"):
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<float, {g}>(" in k]) == 1
        assert len([k for k in kernels if f"fspann::refine_stream_fix_kernel<unsigned char, {g}>(" in k]) == 1
