"""CPU: what can be asked of include/fspann_gt_validate.h without a device.

  * the header declares exactly the five entry points, the library exports them, the binding holds them in a table of its own
    (the three existing tables stay as they are), a null context is FSPANN_E_NULL;
  * fspann_gt_validator_sample (host/java_random.hpp + host/java_hashmap.hpp) against a pure-Python restatement written here from
    the documented algorithms: java.util.Random's LCG, both branches of nextInt(bound), and a dict-of-buckets model of the growing
    HashSet<Integer> table (plain chains: the model asserts that no bin comes near treeifying on these inputs);
  * the two widely published values of new Random(42).nextInt();
  * the same header in a stand-alone g++ program under -fsanitize=address,undefined (tests/cpp/gt_sampler_test.cpp, no preload);
  * tests/gt_validate_ref.py against a literal loop, and against gt_ref.knn on the planted scene where the validator's double
    subtraction and the ground truth's float subtraction name different rows.

No JVM exists here: agreement pins coding slips, not the recollection of the JDK (parity unpinned)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gt_ref
import gt_validate_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VALIDATE = ("fspann_gt_validator_sample", "fspann_nn1_exact_dev", "fspann_nn1_exact_store_dev", "fspann_gt_validate_dev",
            "fspann_gt_validate_store_dev")

# (1, 1); a power-of-two bound; the whole set; either side of the first resize (13 > 12); the reference's default at two sizes;
# values above 65535, where the spread matters; a sample clamped to nq
PAIRS = [(1, 1), (16, 5), (10, 10), (1000, 12), (1000, 13), (1000, 100), (10000, 100), (200000, 100), (7, 100)]
ANCHORS = (-1170105035, 234785527)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
MASK48 = (1 << 48) - 1


class JavaRandom:
    def __init__(self, seed):
        self.seed = (seed ^ 0x5DEECE66D) & MASK48

    def next(self, bits):
        self.seed = (self.seed * 0x5DEECE66D + 0xB) & MASK48
        v = self.seed >> (48 - bits)
        return v - (1 << 32) if v >= (1 << 31) else v           # (int)

    def next_int(self, bound=None):
        if bound is None:
            return self.next(32)
        r = self.next(31)
        m = bound - 1
        if bound & m == 0:
            return (bound * r) >> 31
        u = r
        while True:
            r = u % bound
            s = (u - r + m) & 0xFFFFFFFF                        # int arithmetic wraps
            if s < (1 << 31):                                   # ... >= 0
                return r
            u = self.next(31)


def java_sample(nq, sample):
    """new Random(42); while (set.size() < min(sample, nq)) set.add(rnd.nextInt(nq)); the set's iteration order.  The table: 16
    bins, threshold 12; above the threshold it doubles and every bin splits in order into (same index, index + old length)."""
    want = min(sample, nq)
    if nq <= 0 or want <= 0:
        return []
    cap, thr, size = 16, 12, 0
    bins = {}
    rnd = JavaRandom(42)
    while size < want:
        v = rnd.next_int(nq)
        h = v ^ (v >> 16)                                       # Integer.hashCode() is the value; HashMap.hash spreads it
        chain = bins.setdefault(h & (cap - 1), [])
        if v in chain:
            continue
        chain.append(v)
        assert len(chain) < 8, "a bin this long is about to treeify: outside this model"
        size += 1
        if size > thr:
            grown = {}
            for b in sorted(bins):
                for x in bins[b]:
                    hx = x ^ (x >> 16)
                    grown.setdefault(hx & (2 * cap - 1), []).append(x)
            bins, cap, thr = grown, 2 * cap, 2 * thr
    return [x for b in sorted(bins) for x in bins[b]]


def lib_sample(L, nq, sample):
    out = np.full(max(1, min(sample, nq)) + 3, -7, np.int64)
    cnt = C.c_int64(-1)
    assert L.fspann_gt_validator_sample(nq, sample, out.ctypes.data_as(C.c_void_p), C.byref(cnt)) == 0
    assert (out[cnt.value:] == -7).all()
    return [int(x) for x in out[:cnt.value]]


# ---- the entry points ----------------------------------------------------------------------------------------------------------------
def test_validate_entry_points_are_exported_and_wrapped(pkg):
    pkg._native.build()
    N = pkg._native
    L = N.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fspann_gt_validate.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(fspann_[a-z0-9_]+)\s*\(", txt))) == sorted(VALIDATE)
    assert N.validate_symbols() == sorted(VALIDATE)
    for s in VALIDATE:
        assert hasattr(L, s), s
        assert s not in N.exported_symbols() and s not in N.rows_symbols() and s not in N.eval_symbols(), s
    for m in ("gt_validator_sample", "nn1_exact_dev", "nn1_exact_store_dev", "gt_validate_dev", "gt_validate_store_dev", "nn1_exact",
              "validate_groundtruth", "validate_groundtruth_store"):
        assert hasattr(pkg.FspannContext, m), m
    # the struct the binding fills is the header's: 4 + 4 + 8 + 8 + 8 + 4 * 4 + 10 * 8 bytes
    assert C.sizeof(N.GtValidation) == 128


def test_null_context_without_gpu(pkg):
    N = pkg._native
    L = N.lib()
    v = N.GtValidation()
    assert L.fspann_nn1_exact_dev(None, 10, None, N.F32, 2, None, N.F64, 16, None, 2, None, None) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()
    assert L.fspann_nn1_exact_store_dev(None, 2, None, N.F64, None, 2, None, None) == N.E_NULL
    assert L.fspann_gt_validate_dev(None, 10, None, N.F32, 2, None, N.F64, 16, None, 2, 1, 100, 0.05, C.byref(v)) == N.E_NULL
    assert L.fspann_gt_validate_store_dev(None, 2, None, N.F64, None, 2, 1, 100, 0.05, C.byref(v)) == N.E_NULL
    assert b"ctx is null" in L.fspann_last_error()


def test_sampler_arguments(pkg):
    N = pkg._native
    L = N.lib()
    cnt = C.c_int64(-1)
    for nq, sample in ((0, 10), (-3, 10), (10, 0), (10, -1)):
        cnt.value = -1
        assert L.fspann_gt_validator_sample(nq, sample, None, C.byref(cnt)) == N.OK and cnt.value == 0
    assert L.fspann_gt_validator_sample(10, 5, None, None) == N.E_NULL
    assert L.fspann_gt_validator_sample(10, 5, None, C.byref(cnt)) == N.E_NULL
    assert L.fspann_gt_validator_sample(1 << 31, 5, None, C.byref(cnt)) == N.E_ARG


# ---- the sample ------------------------------------------------------------------------------------------------------------------------
def test_random_42_anchors():
    r = JavaRandom(42)
    assert (r.next_int(), r.next_int()) == ANCHORS


@pytest.mark.parametrize("nq,sample", PAIRS)
def test_sample_equals_the_restatement(pkg, nq, sample):
    want = java_sample(nq, sample)
    assert len(want) == min(nq, sample) == len(set(want)) and all(0 <= x < nq for x in want)
    assert lib_sample(pkg._native.lib(), nq, sample) == want


def test_the_pairs_reach_what_they_are_for():
    assert sorted(java_sample(10, 10)) == list(range(10)) and java_sample(7, 100) == java_sample(7, 7)
    assert max(java_sample(200000, 100)) > 65535
    # 12 values sit in 16 bins, the 13th doubles the table: the order of the first 12 changes where a bin splits
    a, b = java_sample(1000, 12), java_sample(1000, 13)
    assert set(a) < set(b) and [x & 15 for x in a] == sorted(x & 15 for x in a) and [x & 31 for x in b] == sorted(x & 31 for x in b)
    # the rejection loop of nextInt(bound) is reached by the draws of a large odd bound, the power-of-two branch differs from it
    r, hit = JavaRandom(42), 0
    for _ in range(200):
        s0 = r.seed
        r.next_int((1 << 30) + 1)
        t = JavaRandom(0)
        t.seed = s0
        t.next(31)
        hit += t.seed != r.seed
    assert hit > 0


def test_stand_alone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gt_sampler_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "gt_sampler_test.cpp")])
    r = subprocess.run([exe] + [f"{nq}:{s}" for nq, s in PAIRS], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "anchors %d %d" % ANCHORS
    assert len(lines) == 1 + len(PAIRS)
    for (nq, s), line in zip(PAIRS, lines[1:]):
        head, _, vals = line.partition(":")
        assert head == f"{nq} {s}" and [int(x) for x in vals.split()] == java_sample(nq, s), (nq, s)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------------
def test_reference_top1_equals_the_literal_loop():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((90, 5)).astype(np.float32)
    X[40] = X[7]                                    # an exact duplicate: the lower index stays
    X[11, 2], X[12, :] = np.nan, np.inf
    Q = np.concatenate([rng.standard_normal((6, 5)), X[7:8].astype(np.float64) + 2.0 ** -30, np.full((1, 5), np.nan), np.full((1, 5), np.inf)])
    a, b = VR.top1(X, Q), VR.top1_loop(X, Q)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert a[0][6] == 7 and list(a[0][7:]) == [-1, -1] and np.isposinf(a[1][7:]).all()
    assert np.array_equal(VR.top1(X, Q, sel=[6, 0, 6])[0], a[0][[6, 0, 6]])


def test_double_and_float_subtraction_name_different_rows():
    """the restatement can tell the validator's arithmetic from the ground truth's"""
    X, Q = VR.planted_scene()
    assert np.float32(Q[0, 0] - X[0, 0]) == np.float32(Q[0, 0] - X[1, 0]) == np.float32(33554428.0)
    ids, d2, _ = gt_ref.knn(X, Q, 1)
    assert ids[0, 0] == 0 and d2[0, 0] == 33554428.0 ** 2
    idx, dd = VR.top1(X, Q)
    assert idx[0] == 1 and dd[0] == 33554428.0 ** 2 and VR.d2(X, Q)[0, 0] == 33554429.0 ** 2


def test_reference_validate_rules():
    nn = {qi: qi % 50 for qi in range(300)}
    gt = np.array([[nn[qi], 0] for qi in range(300)], np.int32)
    sample = java_sample(300, 100)
    ok = VR.validate(nn.get, sample, 300, gt, 100, 0.05)
    assert ok == dict(valid=True, sample_size=100, mismatches=0, mismatch_rate=0.0, mismatched=[])
    for wrong, valid in ((5, True), (6, False), (12, False)):
        g = gt.copy()
        g[sample[3:3 + wrong], 0] += 1
        r = VR.validate(nn.get, sample, 300, g, 100, 0.05)
        assert r["valid"] is valid and r["mismatches"] == wrong and r["mismatched"] == sample[3:3 + min(wrong, 10)]
    short = VR.validate(nn.get, sample, 300, gt[:250] + 1, 100, 0.05)
    assert short["sample_size"] == 100 and short["mismatches"] == sum(q < 250 for q in sample) < 100
    assert VR.validate(nn.get, [], 0, gt, 100, 0.05)["valid"] and not VR.validate(nn.get, sample, 300, gt[:0], 100, 0.05)["valid"]
    nan = VR.validate(nn.get, [], 300, gt, 0, 0.05)
    assert nan["valid"] and nan["mismatch_rate"] != nan["mismatch_rate"]
