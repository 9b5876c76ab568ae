"""Which ordering path of the full select (route_select_kernel, csrc/route.hip.h, phase C) a query's candidate list takes.

A plain restatement of the kernel's path CHOICE only: it never produces a list (expected lists always come from the oracle).
The tests use it to prove that a scene reaches the tier it was built for, and to aim a scene at a limit of a tier.

    plan    the dict of FspannContext.route_plan_info() (or a hand-built one with the same keys)
    scores  the score of every distinct live id the query keeps (the oracle's full list), any order
    bins    those ids' bins at the map's FINAL table length: spread(hashCode) & (final_cap(cap0, n) - 1), same order
    limit   the call's limit

Tiers: "rank" (all-pairs rank), "wave" (group path, one wave per group), "workgroup" (group path, a group above a wave's slice
sorted by the whole workgroup), "redo" (group path, a padded group that does not fit: the whole list re-sorted by the general
path), "bitonic_lds" / "bitonic_global" (the general sort, in the LDS sort buffer / in global memory).
"""
import numpy as np

RANK_SORT_MAX = 1024      # kRankSortMax
RANK_LIMIT = RANK_SORT_MAX - 128
GROUP_REGION_MIN = 4096   # words of LDS the group path needs
GROUP_TARGET = 128        # entries per group the cut of the bins aims at
TIERS = ("rank", "wave", "workgroup", "redo", "bitonic_lds", "bitonic_global")


def final_cap(cap0, n):
    """java.util.HashMap's table length after n puts into a table that started at cap0 (load factor 0.75)."""
    cap, thr = int(cap0), int(np.float32(cap0) * np.float32(0.75))
    while n > thr and cap < (1 << 30):
        old = cap
        cap <<= 1
        thr = (thr << 1) if old >= 16 else int(np.float32(cap) * np.float32(0.75))
    return cap


def spread(java_hash):
    h = np.asarray(java_hash).astype(np.int32).view(np.uint32)
    return h ^ (h >> 16)


def bins_at_final_cap(java_hash, ids, cap0):
    """The bins of `ids` (a query's full list) at the final table length of its bestScore map."""
    return (spread(java_hash)[np.asarray(ids)] & np.uint32(final_cap(cap0, len(ids)) - 1)).astype(np.int64)


def _find_cut(hist, need):
    """wave_find_cut: the first bin at which the running sum reaches `need`, and the sum in front of it."""
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, need, side="left"))
    if b >= len(hist):
        return len(hist) - 1, int(cum[-1] - hist[-1])
    return b, int(cum[b] - hist[b])


def _pow2(c):
    n2 = 1
    while n2 < c:
        n2 <<= 1
    return n2


class TierSet(set):
    """The tiers one query runs through; `.info` holds the numbers a test aims with."""
    info = None


def order_tiers(plan, scores, bins_at_final_cap, limit):
    scores = np.asarray(scores).astype(np.int64)
    bins = np.asarray(bins_at_final_cap).astype(np.int64)
    n = len(scores)
    assert len(bins) == n
    nbins = plan["nbins"]
    capf = final_cap(plan["cap0"], n)
    capbits = capf.bit_length() - 1
    assert n == 0 or (bins.min() >= 0 and bins.max() < capf)
    hist = np.bincount(scores, minlength=nbins)
    # level 0: the cut score; level 1: the tie level cut further by the top 10 bits of the bin
    star, need, tie = nbins - 1, None, 0
    if n > limit:
        star, before = _find_cut(hist, limit)
        need, tie = limit - before, int(hist[star])
    upto = hist[:star + 1]
    occ = np.flatnonzero(upto)
    smin = int(occ[0]) if len(occ) else star
    lmax = int(upto.max()) if len(occ) else 0
    lvl1 = n > limit and tie - need > 256
    take = scores <= star
    if lvl1:
        top10 = (bins >> (capbits - 10)) if capbits >= 10 else (bins << (10 - capbits))
        b1, _ = _find_cut(np.bincount(top10[scores == star], minlength=1024), need)
        take &= ~((scores == star) & (top10 > b1))
    nsel = int(take.sum())
    nout = min(nsel, limit)
    region = plan["ht_size"] if plan["lds_mode"] else plan["lds_sort_words"]
    out = TierSet()
    out.info = dict(n=n, capf=capf, capbits=capbits, star=star, smin=smin, lmax=lmax, lvl1=bool(lvl1), nsel=nsel, nout=nout,
                    region=region)
    if nsel <= RANK_LIMIT and plan["sort_cap"] >= RANK_SORT_MAX:
        out.add("rank")
        return out
    if not (plan["g_sub"] and capbits + plan["seq_bits"] <= 32 and nbins <= 512 and region >= GROUP_REGION_MIN):
        out.add("bitonic_lds" if _pow2(nsel) <= plan["sort_cap"] else "bitonic_global")
        return out
    # the group path: groups = (score level, top gb bits of the bin)
    smin = min(smin, star)
    nlev = star - smin + 1
    gb = 0
    while gb < 10 and gb < capbits and (nlev << (gb + 1)) <= 1024 and (lmax >> gb) > GROUP_TARGET:
        gb += 1
    ngrp = nlev << gb
    nwv = plan["threads"] >> 6
    sub_lds = nwv * 64 + nsel <= region - 1024
    room = ((region - 1024 - nsel) & ~3) if sub_lds else region - 1024
    wcap = 64
    while wcap * 2 * nwv <= room and wcap < 4096:
        wcap <<= 1
    if not plan["wave_sort"]:
        wcap = 0
    grp = ((scores[take] - smin) << gb) | (bins[take] >> (capbits - gb))
    sizes = np.bincount(grp, minlength=ngrp)
    starts = np.cumsum(sizes) - sizes
    out.info.update(gb=gb, ngrp=ngrp, nlev=nlev, sub_lds=bool(sub_lds), room=int(room), wcap=wcap, group_sizes=sizes, group_starts=starts,
                    selected=take, group_of_selected=grp)
    ahead = (sizes > 0) & (starts < nout)              # groups behind the limit are never sorted
    out.info.update(wave_groups=int((ahead & (sizes <= wcap)).sum()), workgroup_groups=0)
    if out.info["wave_groups"]:
        out.add("wave")
    for c in sizes[ahead & (sizes > wcap)].tolist():   # the workgroup loop: in group order, until one does not fit
        if _pow2(c) <= room:
            out.add("workgroup")
            out.info["workgroup_groups"] += 1
        else:
            out.add("redo")
            break
    return out
