"""CPU: what can be asked of the typed ground-truth / metrics entry points without a device — the library exports them, the
binding table holds them, a null context is FSPANN_E_NULL — and what the built gfx950 code object says of the byte path's
distance kernel: it runs on the int8 matrix cores and holds no fp64 instruction."""
import os
import re
import shutil
import subprocess

import pytest

TYPED = ("fspann_groundtruth_typed_dev", "fspann_eval_metrics_typed_dev")


def test_typed_entry_points_are_exported_and_bound(pkg):
    pkg._native.build()
    L = pkg._native.lib()
    for s in TYPED:
        assert hasattr(L, s), s
        assert s in pkg._native.exported_symbols(), s
    assert hasattr(pkg.FspannContext, "groundtruth_typed_dev") and hasattr(pkg.FspannContext, "eval_metrics_typed_dev")
    assert hasattr(pkg.FspannContext, "groundtruth")


def test_null_context_without_gpu(pkg):
    N = pkg._native
    L = N.lib()
    assert L.fspann_groundtruth_typed_dev(None, 10, None, N.U8, 2, None, N.U8, 16, 5, None, None) == N.E_NULL
    assert L.fspann_eval_metrics_typed_dev(None, 10, None, N.U8, 2, None, N.U8, 16, 5, None, 5, None, None, 5, None, None) == N.E_NULL


def test_gt8_dist_kernel_runs_on_the_int8_matrix_cores(pkg, tmp_path):
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not in this image")
    pkg._native.build()
    so = str(tmp_path / "libfspann_hip.so")
    shutil.copy(pkg._native._SO, so)
    subprocess.run([objdump, "--offloading", so], check=True, capture_output=True, cwd=str(tmp_path))
    objs = [f for f in os.listdir(tmp_path) if "amdgcn" in f and "gfx950" in f]
    assert len(objs) == 1, objs
    dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", "--mcpu=gfx950", str(tmp_path / objs[0])], check=True, capture_output=True,
                         text=True).stdout
    bodies, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:\s*$", line)
        if m:
            cur = bodies.setdefault(m.group(1), []) if "gt8_dist_kernel" in m.group(1) and not m.group(1).endswith(".kd") else None
        elif cur is not None and line.startswith("\t"):
            cur.append(line.split("//")[0].strip())
    assert len(bodies) >= 2, list(bodies)                 # the 16-byte-load and the byte-load instantiation, of uint8_t and of int8_t
    for name, ins in bodies.items():
        assert len(ins) > 50, (name, len(ins))
        assert any(i.startswith("v_mfma_i32_") for i in ins), name
        assert not [i for i in ins if "_f64" in i], name
