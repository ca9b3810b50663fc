"""Shared by the per-region overlap tests and their fixture generator (tests/golden/make_pro_golden.py): the cases and three CPU
restatements of the PRO curve and AUPRO (Bergmann et al., "The MVTec Anomaly Detection Dataset", IJCV 2021) as
include/anoddpm_hip.h defines them --

  pro_exact    scipy.ndimage.label + exact rational arithmetic (integers over a common denominator, fractions.Fraction at the cut)
  pro_fp64     fp64 in the summation order of csrc/pro.hip (stable sort, Hillis-Steele group scan, carries, strided term sum)
  pro_cumsum   the cumulative-sum form of the published evaluation code (argsort, cumsum, keep the last of equal scores, trapezoid
               with the last segment interpolated at the limit)

A case is (mask, score, limit, connectivity): score [S, m, H, W] fp32 -- S segments of m planes -- and mask of that shape or
[m, H, W] (shared by the segments).  The reference has no counterpart; nothing here needs a device."""
import hashlib
import math
from fractions import Fraction

import numpy as np
from scipy import ndimage

import pr_cases as pc

WAVES = 16                                                   # waves in the workgroup of csrc/pro.hip
STRUCTURE = {1: ndimage.generate_binary_structure(2, 1), 2: ndimage.generate_binary_structure(2, 2)}

SMALL = ("plane16", "plane32", "odd40x33", "tiny5x7", "ties4", "ties8", "all_equal", "perfect", "diag_c2", "diag_c1", "one_pixel",
         "border", "pooled4", "mask_all0", "mask_all1", "first_beyond", "at_limit", "limit1", "neg_zero", "shared3")
LARGE = ("pooled3x64", "map256")                             # the only workload-sized cases: summarised in the fixture
STATUS = ("nan_score", "negative_score", "bad_mask")
RAGGED = "ragged50x100"                                      # no fixture entry: the expected values are computed at test time


def tolerance(n):
    """n * 2^-50 against the exact rational value.  Every PRO value is a sum of at most n terms fl(1 / area), each with a relative
    error of 2^-53; the additions of partial sums <= K add at most n K 2^-53, and the division by K leaves about n 2^-53.  The
    truncated integral scales that by at most `limit` and the division by `limit` returns it.  A factor of 8 covers second-order
    terms, the FPR division and the interpolation."""
    return n * 2.0 ** -50


def _blobs(rng, H, W, count, size):
    m = np.zeros((H, W), np.float32)
    for _ in range(count):
        h, w = rng.integers(1, size + 1, 2)
        y, x = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
        m[y:y + h, x:x + w] = 1
    return m


def _scores(rng, mask, shift=0.4, levels=None):
    s = rng.random(mask.shape) + shift * mask
    if levels:
        s = np.floor(s * levels / (1 + shift)) / levels
    return (s * s).astype(np.float32)


def make_case(name):
    """(mask, score, limit, connectivity) of a case."""
    rng = np.random.default_rng(sum(name.encode()) + 20211)
    limit, conn = 0.3, 2
    if name in ("plane16", "limit1"):
        mask = _blobs(np.random.default_rng(5), 16, 16, 3, 5)[None]
        score = _scores(np.random.default_rng(6), mask)[None]
        limit = 1.0 if name == "limit1" else 0.3
    elif name == "plane32":
        mask = _blobs(rng, 32, 32, 5, 7)[None]
        score = _scores(rng, mask)[None]
    elif name == "odd40x33":                                 # odd width; n = 1320 is no multiple of the wave chunk
        mask = _blobs(rng, 40, 33, 6, 8)[None]
        score = _scores(rng, mask)[None]
    elif name == "tiny5x7":                                  # n = 35: smaller than the workgroup
        mask = _blobs(rng, 5, 7, 2, 2)[None]
        score = _scores(rng, mask)[None]
    elif name in ("ties4", "ties8"):
        mask = _blobs(rng, 32, 32, 5, 7)[None]
        score = _scores(rng, mask, levels=int(name[4:]))[None]
    elif name == "all_equal":                                # one run
        mask = _blobs(rng, 16, 16, 3, 5)[None]
        score = np.full((1, 1, 16, 16), 0.25, np.float32)
    elif name == "perfect":                                  # every region pixel above every background pixel: exactly 1
        mask = np.zeros((1, 16, 16), np.float32)
        mask[0, 1:3, 1:3] = 1
        mask[0, 8:12, 9:13] = 1
        score = (rng.random((1, 1, 16, 16)) * 0.5 + mask[None]).astype(np.float32)
    elif name in ("diag_c2", "diag_c1"):                     # two pixels touching only diagonally: one region or two
        mask = np.zeros((1, 8, 8), np.float32)
        mask[0, 3, 3] = mask[0, 4, 4] = 1
        score = _scores(rng, mask)[None]
        conn = int(name[-1])
    elif name == "one_pixel":
        mask = np.zeros((1, 16, 16), np.float32)
        mask[0, 5, 11] = 1
        mask[0, 9:14, 2:8] = 1
        score = _scores(rng, mask)[None]
    elif name == "border":                                   # regions on the plane's border and in its corners
        mask = np.zeros((1, 16, 24), np.float32)
        mask[0, 0, 0:3] = mask[0, 15, 21:24] = mask[0, 6:9, 23] = mask[0, 13:16, 0] = mask[0, 0, 23] = 1
        score = _scores(rng, mask)[None]
    elif name == "pooled4":                                  # the last row of plane 1 lies directly "above" the first row of plane 2
        mask = np.zeros((4, 16, 24), np.float32)
        mask[1, 15, 4:9] = 1
        mask[2, 0, 4:9] = 1
        mask[0, 3:6, 3:6] = 1
        mask[3, 10, 20] = 1
        score = _scores(rng, mask)[None]
    elif name == "mask_all0":
        mask = np.zeros((1, 16, 16), np.float32)
        score = _scores(rng, mask)[None]
    elif name == "mask_all1":
        mask = np.ones((1, 16, 16), np.float32)
        score = _scores(rng, mask)[None]
    elif name == "first_beyond":                             # N = 56; the first curve point has FPR 24 / 56 > 0.3 and PRO 1: 0.35
        mask = np.zeros((1, 8, 8), np.float32)
        mask[0, 2, :] = 1
        s = np.zeros((8, 8), np.float32)
        s[2, :] = 4
        s[3:6, :] = 4                                        # 24 negatives share the highest score with the region
        s[6:, :] = rng.random((2, 8)).astype(np.float32)
        score = s[None, None]
    elif name == "at_limit":                                 # N = 10; the point with 3 negatives above the cut has FPR = 0.3 exactly
        mask = np.zeros((1, 3, 4), np.float32)
        mask[0, 1, 1:3] = 1
        s = np.array([[8, 7, 0.5, 0.25], [1, 9, 6, 2], [5, 3, 0.75, 0.125]], np.float32)
        score = s[None, None]
    elif name == "neg_zero":                                 # -0.0 and +0.0 are one score
        mask = _blobs(rng, 16, 16, 3, 5)[None]
        s = _scores(rng, mask)
        s[s < 0.3] = 0
        z = s == 0
        z[0, 1::2, :] = False
        s[z] = np.float32(-0.0)                              # about half of the zeros carry the sign bit
        score = s[None]
    elif name == "shared3":                                  # three maps, one mask
        mask = _blobs(rng, 16, 16, 3, 5)[None]
        score = np.stack([_scores(rng, mask, shift) for shift in (0.1, 0.4, 0.9)])
    elif name == "pooled3x64":
        mask = np.stack([_blobs(rng, 64, 64, k, 12) for k in (4, 0, 7)])
        score = _scores(rng, mask)[None]
    elif name == "map256":
        mask = _blobs(rng, 256, 256, 9, 40)[None]
        mask[0, 100, 200] = 1
        score = _scores(rng, mask)[None]
    elif name == RAGGED:
        # n = 5000: the wave chunk is 320, so waves 0 to 14 scatter one full unrolled group of 256 and then ONE slice of 64, and
        # wave 15 has 200 elements (three slices and a slice of 8).  Regions of 1, 6, 62, 200 and 600 pixels, three of them side
        # by side in the rows 10 to 24, and eight score levels: equal keys carry different areas on both sides of the chunk
        # borders there, and only a stable payload order gives the right bits
        mask = np.zeros((1, 50, 100), np.float32)
        mask[0, 2, 3] = 1
        mask[0, 46:48, 90:93] = 1
        mask[0, 10:41, 60:62] = 1
        mask[0, 5:45, 5:10] = 1
        mask[0, 5:25, 20:50] = 1
        score = _scores(rng, mask, levels=8)[None]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(mask), np.ascontiguousarray(score), limit, conn


def status_batch():
    """Three segments of 16 x 16 with their own masks; segment j breaks the precondition named STATUS[j] and nothing else does."""
    rng = np.random.default_rng(77)
    mask = np.stack([_blobs(rng, 16, 16, 3, 5)[None] for _ in range(3)])
    score = _scores(rng, mask)
    score[0, 0, 3, 4] = np.nan
    score[1, 0, 7, 1] = -0.5
    mask[2, 0, 2, 2] = 0.5
    return mask, score


def segment_mask(mask, score, s):
    return mask if mask.ndim == 3 else mask[s]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------- regions
def regions(mask, connectivity, level=0.0):
    """mask [m, H, W] -> (area int64 [m, H, W], regions per plane int64 [m]): scipy.ndimage.label per plane."""
    area = np.zeros(mask.shape, np.int64)
    counts = np.zeros(mask.shape[0], np.int64)
    for p, plane in enumerate(mask):
        lab, counts[p] = ndimage.label(plane > level, STRUCTURE[connectivity])
        size = np.bincount(lab.ravel())
        size[0] = 0
        area[p] = size[lab]
    return area, counts


def _runs(score, pos):
    """Descending order of the distinct scores: (thresholds fp32, fps int64, order, run-end indices into the descending order)."""
    s = (score.reshape(-1) + np.float32(0))
    bits = s.view(np.uint32).astype(np.int64)
    key = (bits << 1) | pos.reshape(-1)
    order = np.argsort(key, kind="stable")[::-1]             # position j of the kernel's walk: sorted index n - 1 - j
    sb = bits[order]
    end = np.r_[sb[1:] != sb[:-1], True]
    cp = np.cumsum(pos.reshape(-1)[order])
    idx = np.flatnonzero(end)
    return s[order][idx], (idx + 1) - cp[idx], order, idx


# ---------------------------------------------------------------------------------------------------- exact
def pro_exact(mask, score, limit, connectivity):
    """One segment, exactly.  PRO values are num / den with Python integers; `pro` and `aupro` are those rationals rounded ONCE
    to fp64 (int / int and float(Fraction) round correctly).  aupro is NaN when K == 0 or N == 0."""
    area, counts = regions(mask, connectivity)
    K, n = int(counts.sum()), score.size
    pos = (area.reshape(-1) != 0).astype(np.int64)
    P = int(pos.sum())
    N = n - P
    thr, fps, order, idx = _runs(score, pos)
    out = {"K": K, "N": N, "P": P, "fps": fps, "thresholds": thr, "n": n}
    if K == 0:
        out["pro"], out["aupro"] = np.full(idx.size, np.nan), float("nan")
        return out
    sizes = [int(v) for v in np.unique(area[area != 0])]
    lcm = 1
    for v in sizes:
        lcm = lcm * v // math.gcd(lcm, v)
    den = lcm * K
    a_sorted = area.reshape(-1)[order]
    wnum = np.array([lcm // int(v) if v else 0 for v in a_sorted], dtype=object)
    num = np.cumsum(wnum)[idx]                               # Python integers: exact
    out["pro"] = np.array([int(v) / den for v in num], np.float64)
    if N == 0:
        out["aupro"] = float("nan")
        return out
    lim = Fraction(float(limit))
    limN = lim * N                                           # the cut in units of false positives
    twice = 0                                                # 2 * N * den * area under the full segments
    f0, y0 = 0, 0
    cut = Fraction(0)
    for f1, y1 in zip(fps.tolist(), num.tolist()):
        if f0 >= limN:
            break
        if f1 <= limN:
            twice += (f1 - f0) * (y1 + y0)
        else:
            yl = Fraction(y0) + Fraction(y1 - y0) * (limN - f0) / (f1 - f0)
            cut = (limN - f0) * (yl + y0)
        f0, y0 = f1, y1
    out["aupro_fraction"] = (Fraction(twice) + cut) / (2 * N * den) / lim
    out["aupro"] = float(out["aupro_fraction"])
    return out


# ---------------------------------------------------------------------------------------------------- the kernel's order
def _group_scan(rows):
    """Inclusive Hillis-Steele scan along the 64 lanes of every row, as csrc/pro.hip's group_scan."""
    v = rows.copy()
    off = 1
    while off < 64:
        v[:, off:] = v[:, off:] + v[:, :-off]
        off <<= 1
    return v


def trapezoid_terms(x, y, limit):
    """The term of every curve point as step 4 of csrc/pro.hip forms it (x, y without the (0, 0) point in front)."""
    x0, y0 = np.r_[0.0, x[:-1]], np.r_[0.0, y[:-1]]
    full = (x - x0) * (y + y0) * 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        yl = y0 + (y - y0) * ((limit - x0) / (x - x0))
    cut = (limit - x0) * (yl + y0) * 0.5
    return np.where(x0 < limit, np.where(x <= limit, full, cut), 0.0)


def pro_fp64(mask, score, limit, connectivity):
    """One segment in fp64, every addition in the order of csrc/pro.hip."""
    area, counts = regions(mask, connectivity)
    K, n = int(counts.sum()), score.size
    pos = (area.reshape(-1) != 0).astype(np.int64)
    P = int(pos.sum())
    N = n - P
    thr, fps, order, idx = _runs(score, pos)
    a_sorted = area.reshape(-1)[order].astype(np.float64)
    w = np.zeros(n, np.float64)
    w[a_sorted != 0] = 1.0 / a_sorted[a_sorted != 0]
    chunk = ((n + WAVES - 1) // WAVES + 63) & ~63
    cum = np.zeros(n, np.float64)
    totals, pieces = [], []
    for wave in range(WAVES):
        c0, c1 = min(wave * chunk, n), min(wave * chunk + chunk, n)
        groups = -(-(c1 - c0) // 64)
        rows = np.zeros((groups, 64), np.float64)
        rows.reshape(-1)[:c1 - c0] = w[c0:c1]
        incl = _group_scan(rows)
        total = 0.0
        for g in range(groups):
            total = total + incl[g, 63]
        totals.append(total)
        pieces.append((c0, c1, incl))
    carry = 0.0
    for wave, (c0, c1, incl) in enumerate(pieces):
        c = carry
        for g in range(incl.shape[0]):
            lo = c0 + g * 64
            hi = min(lo + 64, c1)
            cum[lo:hi] = c + incl[g, :hi - lo]
            c = c + incl[g, 63]
        carry = carry + totals[wave]
    pro = np.minimum(cum[idx] / np.float64(K), 1.0) if K else np.full(idx.size, np.nan)
    out = {"K": K, "N": N, "P": P, "fps": fps, "thresholds": thr, "pro": pro, "n": n}
    if K == 0 or N == 0:
        out["aupro"] = float("nan")
    else:
        x = fps.astype(np.float64) / np.float64(N)
        out["aupro"] = pc._kernel_sum(trapezoid_terms(x, pro, np.float64(limit))) / float(limit)
    return out


# ---------------------------------------------------------------------------------------------------- the published form
def pro_cumsum(mask, score, limit, connectivity):
    """AUPRO as the published evaluation code computes it: sort all pixels by descending score, cumulative sums of the
    false-positive and per-region-overlap increments, the last of equal scores kept, the curve starts at (0, 0), and the trapezoid
    up to `limit` with the crossing segment interpolated; divided by `limit`.  Returns (fpr, pro, aupro)."""
    area, counts = regions(mask, connectivity)
    K = int(counts.sum())
    a = area.reshape(-1)
    N = int((a == 0).sum())
    if K == 0 or N == 0:
        return None, None, float("nan")
    s = score.reshape(-1) + np.float32(0)
    order = np.argsort(-s, kind="stable")
    fp_change = (a[order] == 0) / N
    pro_change = np.where(a[order] != 0, 1.0 / np.maximum(a[order], 1), 0.0) / K
    fprs, pros = np.cumsum(fp_change), np.cumsum(pro_change)
    keep = np.r_[s[order][1:] != s[order][:-1], True]
    fprs, pros = np.r_[0.0, np.clip(fprs[keep], 0, 1)], np.r_[0.0, np.clip(pros[keep], 0, 1)]
    below = fprs <= limit
    x, y = fprs[below], pros[below]
    val = float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) * 0.5))
    if not below.all() and x[-1] < limit:
        j = x.size
        yl = y[-1] + (pros[j] - y[-1]) * (limit - x[-1]) / (fprs[j] - x[-1])
        val += (limit - x[-1]) * (yl + y[-1]) * 0.5
    return fprs, pros, val / limit


# ---------------------------------------------------------------------------------------------------- criteria
def check_against_exact(got, want, what):
    """got: the fields of pro_fp64 / metrics.pro_points; want: pro_exact (or the fixture's copy of it).  Counts, fps and
    thresholds are integers / bit patterns; pro and aupro lie within tolerance(n) of the exact value -- `want` holds it rounded
    once, 2^-53 of which the bound gives up."""
    n = want["n"]
    tol = tolerance(n) - 2.0 ** -53
    assert (got["K"], got["N"], got["P"]) == (want["K"], want["N"], want["P"]), (what, got["K"], got["N"], got["P"])
    assert np.array_equal(got["fps"], want["fps"]), what
    assert np.array_equal(np.asarray(got["thresholds"], np.float32).view(np.uint32), np.asarray(want["thresholds"], np.float32).view(np.uint32)), what
    if want["K"] == 0:
        assert np.isnan(got["aupro"]), what
        return
    worst = float(np.max(np.abs(got["pro"] - want["pro"]))) if want["pro"].size else 0.0
    print(f"{what}: n {n} K {want['K']} N {want['N']} points {want['fps'].size}; max |pro - exact| {worst:.3g}; aupro {got['aupro']!r} "
          f"exact {want['aupro']!r} |diff| {abs(got['aupro'] - want['aupro']):.3g}; bound {tol:.3g}")
    assert worst <= tol, what
    assert ((got["pro"] >= 0) & (got["pro"] <= 1)).all(), what
    if want["N"] == 0:
        assert np.isnan(got["aupro"]), what
    else:
        assert abs(got["aupro"] - want["aupro"]) <= tol, what
