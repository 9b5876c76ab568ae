"""CPU: the touched-record entry points (fspann_touch_enable / _count / _drain, include/fspann.h) are declared, exported, bound
by ctypes and by the JNI shim, and refuse a null context without a GPU."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("fspann_touch_enable", "fspann_touch_count", "fspann_touch_drain")


def test_touch_symbols_are_declared_exported_and_bound(pkg):
    pkg._native.build()
    L = pkg._native.lib()
    hdr = open(os.path.join(ROOT, "include", "fspann.h")).read()
    bound = open(os.path.join(ROOT, "jni", "bound_symbols.txt")).read().split()
    jni = open(os.path.join(ROOT, "jni", "fspann_jni.cpp")).read()
    java = open(os.path.join(ROOT, "java", "com", "fspann", "gpu", "FspannNative.java")).read()
    for s in SYMS:
        assert f"int {s}(" in hdr
        assert hasattr(L, s)
        assert s in pkg._native.exported_symbols()
        assert s in bound
        assert f"{s}(" in jni
    for m in ("touchEnable(long ctx, int on)", "touchCount(long ctx, long[] unique)",
              "touchDrain(long ctx, ByteBuffer handles, long cap, long[] n, int reset)"):
        assert m in java


def test_touch_null_context(pkg):
    N = pkg._native
    L = N.lib()
    n = C.c_int64(-7)
    buf = (C.c_int32 * 4)()
    assert L.fspann_touch_enable(None, 1) == N.E_NULL
    assert L.fspann_touch_enable(None, 0) == N.E_NULL
    assert L.fspann_touch_count(None, C.byref(n)) == N.E_NULL
    assert L.fspann_touch_count(None, None) == N.E_NULL
    assert L.fspann_touch_drain(None, buf, 4, C.byref(n), 1) == N.E_NULL
    assert L.fspann_touch_drain(None, None, 0, None, 0) == N.E_NULL
    assert n.value == -7                      # nothing written on failure
    assert b"ctx is null" in L.fspann_last_error()
