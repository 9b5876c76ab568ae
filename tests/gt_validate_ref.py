"""A plain numpy restatement of GroundtruthValidator's exact top-1 and of validate, written from the Java and not from the product
or oracle/: BaseVectorReader.l2sq (GroundtruthValidator.java:219-242: `double d = query[i] - v` with query a double[], i.e. a DOUBLE
subtraction, `sum += d * d` from 0.0 in dimension order), bruteForceNN (:252-265: a strict `<` running minimum over ascending
indices from +inf) and validate's loop (:112-183).  A helper module (no test, no fixture): tests/test_gpu_gt_validate.py takes its
expected values from here, tests/test_gt_validate_cpu.py holds it against a literal loop and against gt_ref.  numpy only."""
import numpy as np


def d2(base, q):
    """[nq][n] float64 sums.  base [n][d]: the VALUES of the rows (float32, or anything that widens exactly to float64); q [nq][d]
    float64, or float32 to be widened.  One double subtraction, one multiply and one add per dimension, in dimension order."""
    b64, q64 = np.asarray(base).astype(np.float64), np.asarray(q).astype(np.float64)
    acc = np.zeros((len(q64), len(b64)), np.float64)
    with np.errstate(all="ignore"):
        for i in range(b64.shape[1]):
            d = q64[:, None, i] - b64[None, :, i]
            acc = acc + d * d
    return acc


def top1(base, q, sel=None):
    """(idx [nsel] int32, d2 [nsel] float64) of bruteForceNN for the queries q[sel] (None: all): the first row, ascending, whose
    sum is below every sum before it, from +inf — the first occurrence of the minimum among the sums < +inf; none: -1 / +inf."""
    q = np.asarray(q)
    if sel is not None:
        q = q[np.asarray(sel, np.int64)]
    D = d2(base, q)
    idx = np.full(len(q), -1, np.int32)
    out = np.full(len(q), np.inf, np.float64)
    for j in range(len(q)):
        row = D[j]
        with np.errstate(invalid="ignore"):
            ok = row < np.inf                       # NaN and +inf never win
        if ok.any():
            i = int(np.argmin(np.where(ok, row, np.inf)))      # argmin: the FIRST of equal minima, which is what strict `<` keeps
            idx[j], out[j] = i, row[i]
    return idx, out


def top1_loop(base, q):
    """the same, statement for statement as the Java reads (small inputs only)"""
    b64, q64 = np.asarray(base).astype(np.float64), np.asarray(q).astype(np.float64)
    idx = np.full(len(q64), -1, np.int32)
    out = np.full(len(q64), np.inf, np.float64)
    with np.errstate(all="ignore"):
        for j in range(len(q64)):
            best, best_i = np.float64(np.inf), -1
            for r in range(len(b64)):
                s = np.float64(0.0)
                for i in range(b64.shape[1]):
                    d = q64[j, i] - b64[r, i]
                    s = s + d * d
                if s < best:
                    best, best_i = s, r
            idx[j], out[j] = best_i, best
    return idx, out


def validate(nn1_of, sample, nq, gt_ids, sample_size, tolerance):
    """validate's loop over `sample` (the HashSet's iteration order): nn1_of(qi) = the exact nearest row of query qi.
    -> dict(valid, sample_size, mismatches, mismatch_rate, mismatched)"""
    gt_ids = np.asarray(gt_ids)
    if nq == 0:
        return dict(valid=True, sample_size=0, mismatches=0, mismatch_rate=0.0, mismatched=[])
    if len(gt_ids) == 0:
        return dict(valid=False, sample_size=0, mismatches=0, mismatch_rate=1.0, mismatched=[])
    effective = min(sample_size, nq)
    mism, listed = 0, []
    for qi in sample:
        if qi >= len(gt_ids):                      # no ground truth for it: skipped, but it stays in the denominator
            continue
        if int(gt_ids[qi][0]) != int(nn1_of(qi)):
            mism += 1
            if len(listed) < 10:
                listed.append(int(qi))
    with np.errstate(all="ignore"):
        rate = float(np.float64(mism) / np.float64(effective))
    return dict(valid=not (rate > tolerance), sample_size=effective, mismatches=mism, mismatch_rate=rate, mismatched=listed)


def planted_scene():
    """q = 2^25 as fp32, d = 1, row 0 = 3, row 1 = 4.  In float q - 3 rounds to 33554428 = q - 4: a tie, the lower id wins and the
    float ground truth says 0.  In double 33554429 > 33554428: the validator says 1.  (3 and 4 are values every row type holds.)"""
    return np.array([[3.0], [4.0]], np.float32), np.array([[2.0 ** 25]], np.float32)
