"""Shared by the precision-recall tests and their fixture generator (tests/golden/make_pr_golden.py): the cases (those of
tests/roc_cases.py plus a tie in the best Dice) and a numpy restatement of step 6 of csrc/roc.hip -- the walk over the runs of
equal score that yields every point of the precision-recall curve, the average precision in the kernel's summation order and the
best Dice by integer comparison.  No sklearn and no device needed here: the fixture tests/golden/pr_kat.npz holds what
sklearn.metrics.precision_recall_curve / average_precision_score returned and what a brute-force search with fractions found."""
import numpy as np

import roc_cases as rc

THREADS, WAVES = 1024, 16                                    # the workgroup of csrc/roc.hip
EXTRA = ("tie_dice",)
SMALL = rc.SMALL + EXTRA                                     # inputs stored in the fixture
SUMMARISED = rc.MAPS + ("long",)                             # one segment each: length + SHA-256 of the curve, scalars


def make_case(name):
    if name == "tie_dice":
        # P = 2.  score >= 4: tp 1, fp 1 -> 2 / 4; score >= 0.5: tp 2, fp 4 -> 4 / 8; everything between is lower, >= 5 gives 0:
        # two thresholds reach the best Dice 1 / 2 and the higher one, 4, has to win
        return (np.array([0, 1, 0, 0, 0, 1, 0], np.float32), np.array([5, 4, 3, 2, 1, 0.5, 0.25], np.float32))
    return rc.make_case(name)


def ap_tolerance(n):
    """Each term (p_r / P) * (tps_r / cnt_r) carries three roundings and the terms sum to at most 1, as do sklearn's
    diff(recall) * precision; either sum, in any order of at most n additions, stays within about (n + 3) * 2^-53 of the exact
    value.  Asserted bound on their difference: n * 2^-52, the bound of rc.auc_tolerance."""
    return rc.auc_tolerance(n)


def run_records(mask, score):
    """Steps 1 to 3 of csrc/roc.hip exactly as rc.roc_numpy states them: sorted keys, runpos / runtp with their sentinel."""
    mask = np.asarray(mask, np.float32).reshape(-1)
    score = np.asarray(score, np.float32).reshape(-1)
    n = score.size
    bits = (score + np.float32(0)).view(np.uint32)
    key = np.sort((bits << np.uint32(1)) | (mask != 0).astype(np.uint32))
    s, lab = key >> np.uint32(1), (key & np.uint32(1)).astype(np.int64)
    bnd = np.r_[True, s[1:] != s[:-1]]
    runpos = np.r_[np.flatnonzero(bnd), n].astype(np.int64)
    runtp = np.r_[0, np.cumsum(lab)][runpos]
    return key, runpos, runtp


def _kernel_sum(terms):
    """fp64 sum in the order of the kernel: thread t adds terms t, t + 1024, ... in that order; a halving tree folds the 64
    partials of each wave, then the 16 wave sums.  (Padding with +0.0 leaves the bits of a non-negative partial alone.)"""
    rows = -(-terms.size // THREADS)
    padded = np.zeros(rows * THREADS, np.float64)
    padded[:terms.size] = terms
    part = np.zeros(THREADS, np.float64)
    for row in padded.reshape(rows, THREADS):
        part = part + row
    w = part.reshape(WAVES, 64)
    off = 32
    while off:
        w = w[:, :off] + w[:, off:2 * off]
        off >>= 1
    v = w[:, 0]
    off = WAVES // 2
    while off:
        v = v[:off] + v[off:2 * off]
        off >>= 1
    return float(v[0])


def pr_numpy(mask, score):
    """Step 6 of csrc/roc.hip (and its full-curve mode) in numpy.  Returns P, N, R (Python ints), every curve point fps / tps
    (int64) / thresholds (fp32) from the highest score down, ap (float: NaN without a positive, 1.0 without a negative) and
    best_dice (float, NaN without a positive) / best_threshold (np.float32) / best_tp / best_fp (Python ints)."""
    key, runpos, runtp = run_records(mask, score)
    n, R, P = int(runpos[-1]), runpos.size - 1, int(runtp[-1])
    thr_of = (key[runpos[:-1]] >> np.uint32(1)).astype(np.uint32).view(np.float32)
    tps = P - runtp[:-1]                                     # per run, ascending score: counts of the prediction score >= thr
    cnt = n - runpos[:-1]                                    # tps + fps
    p_r = np.diff(runtp)
    if P == 0:
        ap = float("nan")
    elif P == n:
        ap = 1.0
    else:
        ap = _kernel_sum((p_r.astype(np.float64) / np.float64(P)) * (tps.astype(np.float64) / cnt.astype(np.float64)))
    # best Dice 2 tps / (cnt + P): exact comparison of the cross products, ties to the higher score
    best = 0
    btp, bden = int(tps[0]), int(cnt[0]) + P
    for r, (t, c) in enumerate(zip(tps.tolist(), cnt.tolist())):
        x, y = t * bden, btp * (c + P)
        if x > y or (x == y and r > best):
            best, btp, bden = r, t, c + P
    dice = float("nan") if P == 0 else (2 * btp) / bden      # int / int: correctly rounded, as the kernel's one fp64 division
    return {"P": P, "N": n - P, "R": R, "fps": (cnt - tps)[::-1], "tps": tps[::-1], "thresholds": thr_of[::-1], "ap": ap,
            "best_dice": dice, "best_threshold": thr_of[best], "best_tp": btp, "best_fp": bden - P - btp}


def sklearn_triple(fps, tps, thresholds):
    """What the host side of PR_curve does with the points: divide the counts in fp64, ascending thresholds, append (1, 0)."""
    tps, fps = np.asarray(tps, np.float64), np.asarray(fps, np.float64)
    prec = tps / (tps + fps)
    rec = tps / tps[-1] if tps[-1] > 0 else np.ones_like(tps)
    return np.hstack((prec[::-1], 1)), np.hstack((rec[::-1], 0)), np.asarray(thresholds, np.float32)[::-1]


def same_float(a, b):
    """Equal, or both NaN."""
    return (np.isnan(a) and np.isnan(b)) or a == b


# ---- the criteria, shared by tests/test_pr_reference.py (the restatement) and tests/test_gpu_pr.py (the kernel)
def check_ap(got, want, P, n, what):
    """want: sklearn's.  Without a positive sklearn says 0.0 (after a warning) and the native path NaN."""
    print(f"{what}: ap {got!r} fixture {want!r} |diff| {abs(got - want):.3g} bound {ap_tolerance(n):.3g}")
    if P == 0:
        assert np.isnan(got) and want == 0.0, what
    else:
        assert abs(got - want) <= ap_tolerance(n), what


def check_best(kat, prefix, j, r, what):
    """r: the best-Dice fields of pr_numpy / metrics.pr_points.  j: index into the arrays of a summarised case, or None."""
    want = {k: (kat[f"{prefix}_{k}"] if j is None else kat[f"{prefix}_{k}"][j]) for k in ("best_dice", "best_thr", "best_tp", "best_fp")}
    print(f"{what}: best dice {r['best_dice']!r} at {r['best_threshold']!r} tp {r['best_tp']} fp {r['best_fp']}; fixture "
          f"{float(want['best_dice'])!r} at {float(want['best_thr'])!r} tp {int(want['best_tp'])} fp {int(want['best_fp'])}")
    assert same_float(r["best_dice"], float(want["best_dice"])), what
    assert rc.bits_equal(np.float32(r["best_threshold"]), np.float32(want["best_thr"])), what
    assert (r["best_tp"], r["best_fp"]) == (int(want["best_tp"]), int(want["best_fp"])), what


def check_summary(kat, prefix, j, r, n):
    prec, rec, thr = sklearn_triple(r["fps"], r["tps"], r["thresholds"])
    assert r["P"] == int(kat[f"{prefix}_P"][j]) and prec.size == int(kat[f"{prefix}_len"][j])
    assert rc.sha_curve(prec, rec, thr) == str(kat[f"{prefix}_curve_sha"][j]), (prefix, j)
    check_ap(r["ap"], float(kat[f"{prefix}_ap"][j]), r["P"], n, f"{prefix}[{j}]")
    check_best(kat, prefix, j, r, f"{prefix}[{j}]")
