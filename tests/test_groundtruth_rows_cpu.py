"""CPU: what can be asked of the ground truth over typed rows (fspann_groundtruth_rows_dev / _store_dev) without a device — the
companion header include/fspann_groundtruth_rows.h declares both and nothing else, the library exports them, the binding and the
context wrap them, a null context is FSPANN_E_NULL — and that fspann.h's counted set of entry points does not hold them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS = ("fspann_groundtruth_rows_dev", "fspann_groundtruth_store_dev")


def test_rows_entry_points_are_exported_and_wrapped(pkg):
    pkg._native.build()
    L = pkg._native.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fspann_groundtruth_rows.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fspann_[a-z0-9_]+)\s*\(", txt))) == sorted(ROWS)
    assert pkg._native.rows_symbols() == sorted(ROWS)
    for s in ROWS:
        assert hasattr(L, s), s
        assert s not in pkg._native.exported_symbols(), s           # (the set of fspann.h, which the JNI shim binds)
    for m in ("groundtruth_rows_dev", "groundtruth_store_dev", "groundtruth_rows", "groundtruth", "groundtruth_typed_dev"):
        assert hasattr(pkg.FspannContext, m), m


def test_null_context_without_gpu(pkg):
    N = pkg._native
    L = N.lib()
    for dt in (N.U8, N.I8, N.F16, N.BF16, N.F8E4M3, N.F32, N.F64):
        assert L.fspann_groundtruth_rows_dev(None, 10, None, dt, 2, None, 16, 5, None, None) == N.E_NULL
    assert L.fspann_groundtruth_store_dev(None, 2, None, 5, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
