"""CPU: the bounded select's 512-entry class at the specialised 16 x 5 shape (BASELINE config #2's headline step) keeps the
resources that let EIGHT of its 256-thread workgroups share a CU: <= 64 VGPRs, <= 80 SGPRs (blocks per CU = min(8,
800 // (ceil(sgpr / 16) * 16 + 16))), no scratch, and <= 160 KiB / 8 of LDS.  Read from the built code object's kernel
metadata, as test_abi.py does; the residency itself is measured by tools/route_residency.py on a debug build."""
import os
import re
import shutil
import subprocess

import pytest

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = ("route_select_lazy_kernelILi256ELi512ELb0ELi16ELi5E", "front_kernelILi512ELb0ELi16ELi5E")
LDS_PER_CU = 160 * 1024
TARGET = 8


def lz_lds_bytes(kent, td, p):
    """route_lazy.hip.h's lz_lds_bytes (the dynamic LDS the host launches the bounded select with)"""
    tp = td * p
    sort_max = kent - 128
    order = (tp + 2) * 8 + (((tp + 1) * 4 + 7) & ~7) + tp * 8 + ((tp * 2 + 3) & ~3)
    return (2 * kent * 8 + tp * 16 + kent * 4 + 4096 + ((max(order, sort_max * 4) + 7) & ~7) + td * 8 + kent * 2 + sort_max * 4 + td * 4
            + (td * 4 + tp * 4 if kent != 512 else 0))


@pytest.fixture(scope="module")
def kernels(pkg, tmp_path_factory):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm-objdump / llvm-readelf not in this image")
    pkg._native.build()
    tmp = tmp_path_factory.mktemp("co")
    so = str(tmp / "libfspann_hip.so")
    shutil.copy(pkg._native._SO, so)
    subprocess.run([OBJDUMP, "--offloading", so], check=True, capture_output=True, cwd=str(tmp))
    objs = [f for f in os.listdir(tmp) if "amdgcn" in f and "gfx950" in f]
    assert len(objs) == 1, objs
    notes = subprocess.run([READELF, "--notes", str(tmp / objs[0])], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in notes.splitlines():
        m = re.search(r"\.name:\s+(\S+)", line)
        if m and m.group(1).startswith("_Z"):
            name = m.group(1)
            out[name] = {}
        m = re.search(r"\.(private_segment_fixed_size|vgpr_count|sgpr_count|group_segment_fixed_size):\s+(\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


@pytest.mark.parametrize("frag", KERNELS)
def test_eight_workgroups_per_cu_fit(kernels, frag):
    hit = [k for k in kernels if frag in k]
    assert len(hit) == 1, (frag, hit)
    md = kernels[hit[0]]
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_count"] <= 64, md                     # 512 / 64 = 8 waves per SIMD
    assert md["sgpr_count"] <= 80, md                     # 800 // (80 + 16) = 8 workgroups per CU
    assert 800 // (-(-md["sgpr_count"] // 16) * 16 + 16) >= TARGET
    lds = lz_lds_bytes(512, 16, 5) + md["group_segment_fixed_size"]
    assert lds <= LDS_PER_CU // TARGET, (lds, md)


def test_lds_formula_mirror_matches_the_header():
    """the Python mirror above against the numbers the header's static_assert pins"""
    assert lz_lds_bytes(512, 16, 5) == 20152
    assert lz_lds_bytes(512, 16, 5) + 256 <= LDS_PER_CU // TARGET    # the host's grid sizing: lds_limit / (lds + 256) per CU
