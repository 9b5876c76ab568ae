"""CPU: what can be asked of the ground truth on the 16-bit matrix cores without a device — the library exports the two calls of
include/fspann_groundtruth_mfma16.h, the binding holds them in a table of their own and in no other, a null context is
FSPANN_E_NULL, and the numpy-level calls know the method's name."""
import sys

import numpy as np
import pytest

MFMA16 = ["fspann_groundtruth_mfma16_dev", "fspann_groundtruth_mfma16_store_dev"]


def test_entry_points_are_exported_and_bound_in_their_own_table(pkg):
    N = pkg._native
    N.build()
    L = N.lib()
    assert N.gt_mfma16_symbols() == MFMA16
    assert len(N.exported_symbols()) == 94                     # (the set of fspann.h, which the JNI shim binds)
    others = [t for t in dir(N) if t.endswith("_symbols") and t != "gt_mfma16_symbols"]
    assert "exported_symbols" in others and "gt_mfma_symbols" in others
    for s in MFMA16:
        assert hasattr(L, s) and getattr(L, s).argtypes is not None, s
        assert not [t for t in others if s in getattr(N, t)()], s
    for m in ("groundtruth_mfma16_dev", "groundtruth_mfma16_store_dev"):
        assert hasattr(pkg.FspannContext, m), m


def test_null_context_without_gpu(pkg):
    N = pkg._native
    L = N.lib()
    assert L.fspann_groundtruth_mfma16_dev(None, 10, None, N.F16, 2, None, 16, 5, None, None, None) == N.E_NULL
    assert L.fspann_groundtruth_mfma16_store_dev(None, 2, None, 5, None, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()


def test_the_method_is_known_and_an_unknown_one_still_refused(pkg):
    check = sys.modules[pkg.FspannContext.__module__]._gt_method
    assert (check("exact"), check("mfma"), check("mfma16")) == ("", "mfma", "mfma16")
    with pytest.raises(pkg._native.FspannArgumentError, match="method must be 'exact' or 'mfma'"):
        pkg.FspannContext.groundtruth_rows(None, np.zeros((4, 8), np.float16), np.zeros((4, 8), np.float32), 2, method="fast")
