"""Shared by the ROC / AUC tests and their fixture generator (tests/golden/make_roc_golden.py): the seeded input recipes of the
cases, and a numpy restatement of what csrc/roc.hip computes (keys, sort, runs, integer twoU, sklearn's drop rule).  No sklearn and
no device needed here: the fixture tests/golden/roc_kat.npz holds what sklearn.metrics.roc_curve / auc returned for these inputs."""
import hashlib

import numpy as np

SIDE = 256
N256 = SIDE * SIDE
SMALL = ("round4_4096", "all_equal", "mask_all0", "mask_all1", "n1", "n2", "n63", "n65", "n1025")     # inputs stored in the fixture
MAPS = ("continuous", "round64", "zero_bg")                                                           # 256^2: recipe + SHA-256 + curve
LONG_N = 1 << 22
BATCH = 55
BATCH_ALL_ZERO_MASK = 7


def _scores(rng, n, pos_frac, shift=0.35):
    """Squared-error-like scores in [0, 1.5): positives (mask 1) sit higher on average, with plenty of overlap."""
    mask = (rng.random(n) < pos_frac).astype(np.float32)
    base = rng.random(n, dtype=np.float32)
    score = (base * base * np.float32(0.9) + mask * rng.random(n, dtype=np.float32) * np.float32(shift)).astype(np.float32)
    return mask, score


def _variant(kind, rng, n, pos_frac):
    mask, score = _scores(rng, n, pos_frac)
    if kind == "round64":                                    # about 100 distinct values
        score = (np.round(score * 64) / 64).astype(np.float32)
    elif kind == "round1024":
        score = (np.round(score * 1024) / 1024).astype(np.float32)
    elif kind == "zero_bg":                                  # 60 % of the pixels are exactly-zero background
        score = np.where(rng.random(n) < 0.6, np.float32(0), score).astype(np.float32)
    elif kind == "round4":                                   # a handful of distinct values
        score = (np.round(score * 4) / 4).astype(np.float32)
    else:
        assert kind == "continuous", kind
    return mask, score


def make_case(name):
    """(mask, score) of a single-segment case, fp32, flattened."""
    if name in MAPS:
        return _variant(name, np.random.default_rng(100 + MAPS.index(name)), N256, 0.03)
    if name == "long":
        return _variant("continuous", np.random.default_rng(300), LONG_N, 0.05)
    rng = np.random.default_rng(200 + SMALL.index(name))
    if name == "round4_4096":
        return _variant("round4", rng, 4096, 0.1)
    if name == "all_equal":
        mask, _ = _scores(rng, 4096, 0.2)
        return mask, np.full(4096, 0.375, np.float32)
    if name == "mask_all0":
        return np.zeros(4096, np.float32), _scores(rng, 4096, 0.2)[1]
    if name == "mask_all1":
        return np.ones(4096, np.float32), _scores(rng, 4096, 0.2)[1]
    n = int(name[1:])
    mask, score = _scores(rng, n, 0.4)
    if n >= 2:
        mask[0], mask[1] = 0.0, 1.0                          # both classes present
        score[n // 2:] = score[:n - n // 2]                  # and some tied scores
    return mask, score


RAGGED_N = 5000                                              # no fixture entry: the expected values are computed at test time


def make_ragged():
    """(mask, score) of RAGGED_N elements with about 100 distinct scores.  The wave chunk is 320: waves 0 to 14 scatter one full
    unrolled group of 256 and then ONE slice of 64, wave 15 has 200 elements (three slices and a slice of 8); the ties cross every
    chunk border (tests/test_roc_reference.py checks that)."""
    return _variant("round64", np.random.default_rng(400), RAGGED_N, 0.1)


def make_batch():
    """([55, 256^2] masks, [55, 256^2] scores): different contents per segment, one all-zero mask."""
    kinds = ("continuous", "round64", "zero_bg", "round1024", "round4")
    masks, scores = np.empty((BATCH, N256), np.float32), np.empty((BATCH, N256), np.float32)
    for j in range(BATCH):
        masks[j], scores[j] = _variant(kinds[j % len(kinds)], np.random.default_rng(1000 + j), N256, 0.01 + 0.004 * j)
    masks[BATCH_ALL_ZERO_MASK] = 0.0
    return masks, scores


def sha_inputs(mask, score):
    return hashlib.sha256(np.ascontiguousarray(mask).tobytes() + np.ascontiguousarray(score).tobytes()).hexdigest()


def sha_curve(fpr, tpr, thresholds):
    return hashlib.sha256(np.ascontiguousarray(fpr).tobytes() + np.ascontiguousarray(tpr).tobytes()
                          + np.ascontiguousarray(thresholds).tobytes()).hexdigest()


def auc_tolerance(n):
    """The integer form is correctly rounded up to one division; sklearn's auc is an fp64 trapezoid sum over at most n + 1 terms
    of magnitude at most 1, so the two differ by at most about (n + 1) * 2^-53.  Asserted bound: n * 2^-52."""
    return n * 2.0 ** -52


def roc_numpy(mask, score):
    """Steps 1 to 5 of csrc/roc.hip in numpy.  Returns P, N, twoU, R (Python ints), auc (float) and the kept curve points
    fps / tps (int64) / thresholds (fp32) from the highest score down, without the (0, 0, inf) point sklearn prepends."""
    mask = np.asarray(mask, np.float32).reshape(-1)
    score = np.asarray(score, np.float32).reshape(-1)
    n = score.size
    # 1. keys: the bit pattern of a finite score >= 0 is monotone, the sign bit is free for the label
    bits = (score + np.float32(0)).view(np.uint32)
    key = (bits << np.uint32(1)) | (mask != 0).astype(np.uint32)
    # 2. sort
    key = np.sort(key)
    s, lab = key >> np.uint32(1), (key & np.uint32(1)).astype(np.int64)
    # 3. runs of equal score, ascending: start position, positives below it (+ a sentinel for the end of the last run)
    bnd = np.r_[True, s[1:] != s[:-1]]
    runpos = np.r_[np.flatnonzero(bnd), n].astype(np.int64)
    tp_below = np.r_[0, np.cumsum(lab)]                      # positives at positions < i
    runtp = tp_below[runpos]
    P, R = int(runtp[-1]), runpos.size - 1
    N = n - P
    # 4. twoU = sum_v P_v (2 N_below(v) + N_v), integers
    p_r = np.diff(runtp)
    n_r = np.diff(runpos) - p_r
    two_u = int(np.sum(p_r * (2 * (runpos[:-1] - runtp[:-1]) + n_r)))
    auc = float("nan") if P == 0 or N == 0 else two_u / (2.0 * P * N)
    # 5. curve points, from the highest score down; keep the first, the last and every point where the next lower run has
    #    other counts (= a non-zero second difference of fps or of tps)
    keep = np.ones(R, bool)
    keep[1:R - 1] = ((p_r[1:R - 1] != p_r[0:R - 2]) | (n_r[1:R - 1] != n_r[0:R - 2])) if R > 2 else keep[1:R - 1]
    r = np.flatnonzero(keep)[::-1]
    tps = P - runtp[r]
    fps = (n - runpos[r]) - tps
    thresholds = (key[runpos[r]] >> np.uint32(1)).astype(np.uint32).view(np.float32)
    return {"P": P, "N": N, "twoU": two_u, "R": R, "auc": auc, "fps": fps, "tps": tps, "thresholds": thresholds}


def sklearn_triple(fps, tps, thresholds):
    """What the host side of ROC_AUC does with the kept points: prepend (0, 0, inf), divide the counts in fp64."""
    fps = np.r_[0.0, np.asarray(fps, np.float64)]
    tps = np.r_[0.0, np.asarray(tps, np.float64)]
    thresholds = np.r_[np.float32(np.inf), np.asarray(thresholds, np.float32)].astype(np.float32)
    fpr = fps / fps[-1] if fps[-1] > 0 else np.repeat(np.nan, fps.shape)
    tpr = tps / tps[-1] if tps[-1] > 0 else np.repeat(np.nan, tps.shape)
    return fpr, tpr, thresholds


def bits_equal(a, b):
    """Same shape, same dtype, same bit pattern (NaN == NaN, +0.0 != -0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
