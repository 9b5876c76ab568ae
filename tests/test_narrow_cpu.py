"""CPU: what can be asked of include/fspann_narrow.h without a device — the header declares the four narrowing entry points and
nothing else, the library exports them, the binding holds them in a table of its own (fspann.h's counted set stays exactly that
header's set), and a null context is FSPANN_E_NULL."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NARROW = ("fspann_rows_fit_dev", "fspann_rows_narrow_dev", "fspann_store_fit", "fspann_store_narrow")


def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fspann_[a-z0-9_]+)\s*\(", txt)))


def test_narrow_entry_points_are_exported_and_bound(pkg):
    pkg._native.build()
    L = pkg._native.lib()
    assert _declared("fspann_narrow.h") == sorted(NARROW)
    assert pkg._native.narrow_symbols() == sorted(NARROW)
    for s in NARROW:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
        for other in ("exported_symbols", "rows_symbols", "eval_symbols", "validate_symbols", "plan_symbols", "sweep_symbols"):
            assert s not in getattr(pkg._native, other)(), (s, other)
    for m in ("rows_fit_dev", "rows_narrow_dev", "rows_fit", "store_fit", "store_narrow", "store_set_narrowest"):
        assert hasattr(pkg.FspannContext, m), m


def test_exported_symbols_are_still_fspann_h(pkg):
    assert pkg._native.exported_symbols() == _declared("fspann.h")
    assert len(pkg._native.exported_symbols()) == 94


def test_header_is_a_build_input(pkg):
    """a change of the header rebuilds the library"""
    import inspect
    assert "fspann_narrow.h" in inspect.getsource(pkg._native.needs_build)


def test_fit_struct_matches_the_header(pkg):
    """fspann_fit: uint32 fits, int32 narrowest, int64 first_misfit[8], int64 nonfinite — 80 bytes, no padding"""
    F = pkg._native.Fit
    assert C.sizeof(F) == 80
    assert (F.fits.offset, F.narrowest.offset, F.first_misfit.offset, F.nonfinite.offset) == (0, 4, 8, 72)


def test_null_context_without_gpu(pkg):
    N = pkg._native
    L = N.lib()
    fit = N.Fit()
    mis = C.c_int64(0)
    dt = C.c_int(0)
    assert L.fspann_rows_fit_dev(None, 2, None, N.F32, 4, 0, None, C.byref(fit)) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
    assert L.fspann_rows_narrow_dev(None, 2, None, N.F32, 4, None, N.U8, C.byref(mis)) == N.E_NULL
    assert L.fspann_store_fit(None, 0, C.byref(fit)) == N.E_NULL
    assert L.fspann_store_narrow(None, 0, C.byref(dt)) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
