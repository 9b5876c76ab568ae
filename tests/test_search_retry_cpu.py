"""CPU: the retry entry points (fspann_search_retry_dev / fspann_search_retry_finish_dev) are declared, exported by the built
library, bound by ctypes and by the generated JNI shim, and their list-mode kernels are in the gfx950 code object."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fspann_search_retry_dev", "fspann_search_retry_finish_dev", "fspann_pipeline_set_retry", "fspann_pipeline_retry_stats")


def test_retry_entry_points_are_declared_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "fspann.h")).read()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert name in pkg._native._SIGS, name
        assert callable(getattr(pkg._native.lib(), name))
    # retried_dev follows the arguments of fspann_search_store_dev; the finish call adds *resolved
    base = len(pkg._native._SIGS["fspann_search_store_dev"][1])
    assert len(pkg._native._SIGS["fspann_search_retry_dev"][1]) == base + 1
    assert len(pkg._native._SIGS["fspann_search_retry_finish_dev"][1]) == base + 2
    assert hasattr(pkg.FspannContext, "search_retry_dev") and hasattr(pkg.FspannContext, "search_retry_finish_dev")


def test_retry_entry_points_are_exported(pkg):
    so = pkg._native.build()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert name in syms, name


def test_jni_shim_covers_the_retry_calls():
    bound = open(os.path.join(ROOT, "jni", "bound_symbols.txt")).read().split()
    java = open(os.path.join(ROOT, "java", "com", "fspann", "gpu", "FspannNative.java")).read()
    shim = open(os.path.join(ROOT, "jni", "fspann_jni.cpp")).read()
    for name in NEW:
        assert name in bound and (name + "(") in shim, name
        camel = re.sub(r"_([a-z])", lambda m: m.group(1).upper(), name[len("fspann_"):])
        assert re.search(r"public static native \w+ " + camel + r"\(", java), camel


def test_list_mode_kernels_are_built_for_gfx950(pkg):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kregs
    ks = kregs.kernels(pkg._native.build())
    names = " ".join(ks)
    for k in ("retry_pick_kernel", "route_probe_list_kernel", "route_select_lazy_list_kernel", "refine_stream_list_kernel",
              "refine_merge_list_kernel"):
        assert k in names, k
    # one pick kernel, one instantiation per rule: the retry, the fallback, the retry among the fallen-back, the sweep
    picks = [name for name in ks if "retry_pick_kernel" in name]
    assert len(picks) == 4 and all(rule in " ".join(picks) for rule in ("RetryRule", "FallbackRule", "MemberRetryRule", "SweepRule")), picks
    for name, v in ks.items():
        if "list_kernel" in name or "retry_pick" in name:
            assert v.get("private_segment_fixed_size", 0) == 0, name


def test_null_handles_are_refused_without_a_device(pkg):
    """Argument checks that need no context: a null context / pipeline is FSPANN_E_NULL before anything touches a device."""
    import ctypes as C
    L, N = pkg._native.lib(), pkg._native
    ret = C.c_int64(0)
    assert L.fspann_search_retry_dev(None, 4, None, 0, -1, 64, 10, None, None, None, None, None, None, None, None) == N.E_NULL
    assert L.fspann_search_retry_finish_dev(None, 4, None, 0, -1, 64, 10, None, None, None, None, None, None, None, None, C.byref(ret)) == N.E_NULL
    assert L.fspann_pipeline_set_retry(None, 1) == N.E_NULL
    assert L.fspann_pipeline_retry_stats(None, None, None) == N.E_NULL

