"""CPU: the dtype table (csrc/dtypes.h: sizes, names, is-row / is-query, the two dispatchers, the refusal by name) is plain host
code.  tests/cpp/dtype_table_check.cpp walks every dtype id from -2 to 80 through it and compares each answer with values written
out there; it is built as a stand-alone program with AddressSanitizer + UBSan on the host side only and run as it is (no device,
nothing preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "dtype_table_check.cpp")


def test_dtype_table_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "dtype_table_check")
    subprocess.check_call(["hipcc", "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and "83 ids checked, 0 wrong" in r.stdout, r.stdout + r.stderr[-3000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
