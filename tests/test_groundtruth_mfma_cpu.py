"""CPU: what can be asked of the ground truth with the matrix-core pre-filter without a device — the library exports the two calls
of include/fspann_groundtruth_mfma.h and the binding holds them in a table of their own, the numpy-level calls refuse an unknown
method before anything else, a null context is FSPANN_E_NULL in the existing words."""
import numpy as np
import pytest

MFMA = ["fspann_groundtruth_mfma_dev", "fspann_groundtruth_mfma_store_dev"]


def test_entry_points_are_exported_and_bound(pkg):
    pkg._native.build()
    L = pkg._native.lib()
    assert pkg._native.gt_mfma_symbols() == MFMA
    for s in MFMA:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
        assert s not in pkg._native.exported_symbols(), s           # (the set of fspann.h, which the JNI shim binds)
    for m in ("groundtruth_mfma_dev", "groundtruth_mfma_store_dev", "groundtruth_store"):
        assert hasattr(pkg.FspannContext, m), m


@pytest.mark.parametrize("call", ("groundtruth_rows", "groundtruth", "groundtruth_store"))
def test_unknown_method_is_refused(pkg, call):
    X, args = np.zeros((4, 8), np.float32), ()
    args = (X, 2) if call == "groundtruth_store" else (X, X, 2)
    with pytest.raises(pkg._native.FspannArgumentError, match="method must be 'exact' or 'mfma'"):
        getattr(pkg.FspannContext, call)(None, *args, method="fast")


def test_null_context_without_gpu(pkg):
    N = pkg._native
    L = N.lib()
    assert L.fspann_groundtruth_mfma_dev(None, 10, None, N.F16, 2, None, 16, 5, None, None, None) == N.E_NULL
    assert L.fspann_groundtruth_mfma_store_dev(None, 2, None, 5, None, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
