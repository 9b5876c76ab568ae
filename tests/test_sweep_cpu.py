"""CPU: what can be asked of include/fspann_sweep.h without a device — the header declares the four sweep entry points and nothing
else, the library exports them, the binding holds them in a table of its own (fspann.h's counted set stays exactly that header's
set), and a null context is FSPANN_E_NULL."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWEEP = ("fspann_refine_sweep_dev", "fspann_refine_store_sweep_dev", "fspann_search_sweep_dev", "fspann_search_sweep_finish_dev")


def _declared(header):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(fspann_[a-z0-9_]+)\s*\(", txt)))


def test_sweep_entry_points_are_exported_and_bound(pkg):
    pkg._native.build()
    L = pkg._native.lib()
    assert _declared("fspann_sweep.h") == sorted(SWEEP)
    assert pkg._native.sweep_symbols() == sorted(SWEEP)
    for s in SWEEP:
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s
        for other in ("exported_symbols", "rows_symbols", "eval_symbols", "validate_symbols", "plan_symbols"):
            assert s not in getattr(pkg._native, other)(), (s, other)
    for m in ("refine_store_sweep_dev", "refine_sweep_dev", "search_sweep_dev", "search_sweep_finish_dev", "search_sweep", "limit_sweep"):
        assert hasattr(pkg.FspannContext, m), m


def test_exported_symbols_are_still_fspann_h(pkg):
    assert pkg._native.exported_symbols() == _declared("fspann.h")
    assert len(pkg._native.exported_symbols()) == 94


def test_header_is_a_build_input(pkg):
    """a change of the header rebuilds the library"""
    import inspect
    assert "fspann_sweep.h" in inspect.getsource(pkg._native.needs_build)


def test_null_context_without_gpu(pkg):
    N = pkg._native
    L = N.lib()
    lim = (C.c_int64 * 2)(10, 20)
    assert L.fspann_refine_sweep_dev(None, 2, None, N.F32, None, N.F32, 20, None, None, lim, 2, 5, None, None, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
    assert L.fspann_refine_store_sweep_dev(None, 2, None, N.F32, 20, None, None, lim, 2, 5, None, None, None, None) == N.E_NULL
    assert L.fspann_search_sweep_dev(None, 2, None, N.F32, -1, lim, 2, 5, None, None, None, None, None, None, None) == N.E_NULL
    assert L.fspann_search_sweep_finish_dev(None, 2, None, N.F32, -1, lim, 2, 5, None, None, None, None, None, None, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
