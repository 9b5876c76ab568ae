"""CPU: the layouts and the transport choice of the host-pointer calls (csrc/host_staging.h) are plain host code.
tests/cpp/host_staging_check.cpp drives them with raw byte counts for fspann_encode / _route / _refine / _refine_store and compares
the transport and every piece's offset with formulas written out there; it is built as a stand-alone program with AddressSanitizer
+ UBSan on the host side only and run as it is (no device, nothing preloaded)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "host_staging_check.cpp")


def test_host_staging_under_address_and_ub_sanitizers(tmp_path):
    exe = str(tmp_path / "host_staging_check")
    subprocess.check_call(["hipcc", "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    m = re.search(r"^(\d+) cases checked, (\d+) wrong$", r.stdout, re.M)
    # 3 values of nq x 8 combinations of the three facts x (5 encode + 9 route + 2 x 10 refine) size cases
    assert r.returncode == 0 and m and int(m.group(1)) == 3 * 8 * 34 and int(m.group(2)) == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
