"""CPU: tests/route_order_model.py — the restatement of the full select's ordering-path choice (route.hip.h, phase C) — fed with
hand-built lists on both sides of every threshold.  A changed constant on either side shows up here as a diff: the GPU tests use the
model only to prove that a scene reaches the path it was built for."""
import ctypes as C
import os
import re

import numpy as np

from route_order_model import TIERS, final_cap, order_tiers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIG = 2**31 - 1


def plan(**over):
    """LDS mode, 8 192-word region, 1 024 threads, a sub-key buffer: the plan of 8 tables x 10 probes x 64 with no limit."""
    p = dict(ht_size=8192, lds_sort_words=0, sort_cap=8192, lds_mode=1, threads=1024, max_tuples=5120, maxcand=5120, nbins=25,
             cap0=32768, slice_ht=0, lazy=0, g_sub=1, seq_bits=13, wave_sort=1, lazy_cap=0, probes=10)
    p.update(over)
    return p


def spread_list(n, level=3, cap=32768):
    """n entries on one level, bins spread evenly: groups near n >> gb."""
    return np.full(n, level), (np.arange(n) * (cap // max(n, 1))) % cap


def crowded(n_rest, c, level=3, cap=32768):
    """c entries of `level` in bins 0 .. (one group for any gb <= 10), n_rest entries spread over level + 1."""
    s = np.concatenate([np.full(c, level), np.full(n_rest, level + 1)])
    b = np.concatenate([np.arange(c) % 32, (np.arange(n_rest) * 37 + 5000) % cap])
    return s, b


def test_final_cap_is_the_hashmaps():
    assert final_cap(32768, 24576) == 32768 and final_cap(32768, 24577) == 65536 and final_cap(4096, 3073) == 8192
    assert final_cap(64, 48) == 64 and final_cap(64, 49) == 128 and final_cap(64, 97) == 256


def test_rank_path_limit_896_897():
    s, b = spread_list(896)
    assert order_tiers(plan(), s, b, BIG) == {"rank"}
    s, b = spread_list(897)
    assert order_tiers(plan(), s, b, BIG) == {"wave"}
    # ... and only where the sort buffer holds 1 024 keys
    s, b = spread_list(300)
    assert order_tiers(plan(sort_cap=1024), s, b, BIG) == {"rank"}
    assert order_tiers(plan(sort_cap=512), s, b, BIG) == {"wave"}
    # a limit below the list: what counts is what the select keeps (limit + ties), not the list
    s, b = spread_list(3000)
    s[:800] = 1
    t = order_tiers(plan(), s, b, 700)
    assert t == {"rank"} and t.info["nsel"] == 800 and t.info["star"] == 1 and t.info["nout"] == 700


def test_tie_level_is_cut_by_bins_when_more_than_256_ties_lie_behind_the_limit():
    s, b = spread_list(3000)                       # one level: tie = 3000
    t = order_tiers(plan(), s, b, 2744)            # tie - need = 256: not cut
    assert not t.info["lvl1"] and t.info["nsel"] == 3000
    t = order_tiers(plan(), s, b, 2743)            # 257: cut by the top 10 bits of the bin
    assert t.info["lvl1"] and 2743 <= t.info["nsel"] < 2743 + 8


def test_group_of_wcap_and_wcap_plus_one():
    # nsel = 128 + 3000: room = (8192 - 1024 - 3128) & ~3 = 4040 -> wcap 128 (128 * 32 = 4096 > 4040)
    s, b = crowded(3000, 128)
    t = order_tiers(plan(), s, b, BIG)
    assert t == {"wave"} and t.info["wcap"] == 128 and t.info["room"] == 4040 and t.info["group_sizes"].max() == 128
    s, b = crowded(3000, 129)
    t = order_tiers(plan(), s, b, BIG)
    assert t == {"wave", "workgroup"} and t.info["wcap"] == 128 and t.info["group_sizes"].max() == 129
    # one entry fewer in the list: room 4096 -> wcap 256, and 129 fits a wave again
    s, b = crowded(2943, 129)
    t = order_tiers(plan(), s, b, BIG)
    assert t.info["room"] == 4096 and t.info["wcap"] == 256 and t == {"wave"}
    # whole-workgroup sorts only (wave_sort off): every group is "above the slice"
    assert order_tiers(plan(wave_sort=0), s, b, BIG) == {"workgroup"}
    # 512 threads: 8 waves share the room, a slice is twice as long
    s, b = crowded(3000, 129)
    assert order_tiers(plan(threads=512), s, b, BIG).info["wcap"] == 256


def test_padded_group_of_room_words_and_the_next_power_of_two():
    # 5 120 entries: room = 2 048.  A group of 2 048 pads to 2 048 (fits), 2 049 pads to 4 096 (redo)
    s, b = crowded(5120 - 2048, 2048)
    t = order_tiers(plan(), s, b, BIG)
    assert t.info["room"] == 2048 and "workgroup" in t and "redo" not in t
    s, b = crowded(5120 - 2049, 2049)
    assert "redo" in order_tiers(plan(), s, b, BIG)
    # 1 025 .. 2 048 all pad to 2 048: at 5 121 entries the room is 2 044 and they no longer fit
    s, b = crowded(5121 - 1025, 1025)
    t = order_tiers(plan(), s, b, BIG)
    assert t.info["room"] == 2044 and "redo" in t
    s, b = crowded(5120 - 1025, 1025)
    assert "redo" not in order_tiers(plan(), s, b, BIG)


def test_groups_behind_the_limit_are_not_sorted():
    # level 3: 2 800 spread entries; level 9: 100 in the lowest bins and 200 in the upper half of the table (a group above the slice)
    s = np.concatenate([np.full(2800, 3), np.full(300, 9)])
    b = np.concatenate([(np.arange(2800) * 37 + 5000) % 32768, np.arange(100) % 32, 16384 + np.arange(200) % 32])
    t = order_tiers(plan(), s, b, 2900)            # 200 ties behind the limit: the whole level is selected, the big group starts AT nout
    assert not t.info["lvl1"] and t.info["nsel"] == 3100 and t.info["nout"] == 2900 and t.info["wcap"] == 128 and t == {"wave"}
    assert order_tiers(plan(), s, b, 2901) == {"wave", "workgroup"}


def test_sub_keys_in_lds_or_global_memory():
    # region 17 312 words (global-arena mode), 16 waves: sub-keys in LDS while 1 024 + nsel <= 16 288
    p = plan(lds_mode=0, ht_size=65536, lds_sort_words=17312, sort_cap=1024, cap0=65536, seq_bits=16, max_tuples=51200, maxcand=51200)
    s, b = spread_list(15264, cap=65536)
    t = order_tiers(p, s, b, BIG)
    assert t.info["sub_lds"] and t.info["room"] == 1024 and t.info["wcap"] == 64
    s, b = spread_list(15265, cap=65536)
    t = order_tiers(p, s, b, BIG)
    assert not t.info["sub_lds"] and t.info["room"] == 16288 and t.info["wcap"] == 512


def test_group_bits_follow_the_largest_level():
    s, b = spread_list(4000)
    t = order_tiers(plan(), s, b, BIG)             # 25 levels x 2^5 = 800 groups <= 1024; 4000 >> 5 = 125 <= 128
    assert t.info["lmax"] == 4000 and t.info["nlev"] == 22 and t.info["gb"] == 5
    t = order_tiers(plan(nbins=41), s, b, BIG)     # 38 levels: 38 << 5 > 1024 -> one bit fewer
    assert t.info["nlev"] == 38 and t.info["gb"] == 4
    s, b = spread_list(1031)
    assert order_tiers(plan(), s, b, BIG).info["gb"] == 3       # 1031 >> 3 = 128: not above the ~128 a group aims at
    s, b = spread_list(1032)
    assert order_tiers(plan(), s, b, BIG).info["gb"] == 4


def test_general_sort_conditions():
    s, b = spread_list(3000)
    # bin bits + tuple-number bits: 32 fits the 32-bit sub-key, 33 does not
    assert order_tiers(plan(cap0=65536, seq_bits=16), s, b * 2, BIG) == {"wave"}
    assert order_tiers(plan(cap0=65536, seq_bits=17), s, b * 2, BIG) == {"bitonic_lds"}
    # the LDS region: 4 096 words are enough, 4 095 are not (LDS mode: the hash table; global-arena mode: the reserved words)
    s, b = spread_list(1500)
    assert "wave" in order_tiers(plan(ht_size=4096), s, b, BIG)
    assert order_tiers(plan(ht_size=4095), s, b, BIG) == {"bitonic_lds"}
    assert "wave" in order_tiers(plan(lds_mode=0, lds_sort_words=4096), s, b, BIG)
    assert order_tiers(plan(lds_mode=0, lds_sort_words=4095, sort_cap=1024), s, b, BIG) == {"bitonic_global"}
    # no sub-key buffer (a limit <= 896 plans none), more than 512 score levels
    assert order_tiers(plan(g_sub=0), s, b, BIG) == {"bitonic_lds"}
    assert order_tiers(plan(nbins=512), s, b, BIG) == {"workgroup"}      # (509 levels leave one bin bit: two groups of 750)
    assert order_tiers(plan(nbins=513), s, b, BIG) == {"bitonic_lds"}
    # LDS or global: the padded list against the sort buffer
    s, b = spread_list(1024)
    assert order_tiers(plan(g_sub=0, sort_cap=1024), s, b, BIG) == {"bitonic_lds"}
    s, b = spread_list(1025)
    assert order_tiers(plan(g_sub=0, sort_cap=1024), s, b, BIG) == {"bitonic_global"}


def test_every_tier_has_a_name():
    assert set(TIERS) == {"rank", "wave", "workgroup", "redo", "bitonic_lds", "bitonic_global"}


def test_plan_info_is_declared_bound_and_exported(pkg):
    """include/fspann_route_plan.h declares one call; the library exports it, Python binds it from a table of its own, and the
    counted set of fspann.h (the JNI shim's) does not hold it.  A null context is refused without a device."""
    N = pkg._native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fspann_route_plan.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(fspann_[a-z0-9_]+)\s*\(", txt)))
    assert syms == ["fspann_route_plan_info"] == N.plan_symbols()
    assert hasattr(N.lib(), syms[0])
    assert syms[0] not in N.exported_symbols() + N.rows_symbols() + N.eval_symbols() + N.validate_symbols()
    assert syms[0] not in open(os.path.join(ROOT, "jni", "bound_symbols.txt")).read().split()
    out = (C.c_int32 * 16)()
    assert N.lib().fspann_route_plan_info(None, -1, 100, 1, out, 16) == N.E_NULL
    from fspann_amd import engine
    assert len(engine.FspannContext.ROUTE_PLAN_FIELDS) == 16
