"""Shared by the tests of csrc/select_wide.hip: the seeded input recipes of the cases and plain-numpy restatements of its two
entry points,
  `select_numpy`   value, above, equal and top-k mean of every rank, max and mean of the segment (anoddpm_select_wide, bit for
                   bit): `numpy.partition` on the uint32 patterns, the sums by `smooth_cases.tree_sum` -- the order of additions
                   of anoddpm_map_scores, which this kernel continues
  `counts_numpy`   tp / fp at every threshold, P / N (anoddpm_threshold_counts): plain comparisons and sums
Each takes `defect=` to plant one of DEFECTS; the tests show that each changes some case's output.  No device is needed here.
Inputs are built from elementwise IEEE arithmetic on seeded PCG64 draws only, at the smallest shapes at which each step of the
kernels can go wrong."""
import numpy as np

from smooth_cases import _errors, scores_numpy, tree_sum

MAX_RANKS = 16                                               # ANODDPM_SELECT_MAX_RANKS
MAX_THRESHOLDS = 16                                          # ANODDPM_THRESHOLD_COUNTS_MAX
ABS = np.uint32(0x7fffffff)
NAN_BIT, INF_BIT, NEGATIVE_BIT, BAD_MASK_BIT, BAD_RANK_BIT = 1, 2, 4, 8, 32
COUNT_TILE = 4096                                            # values per workgroup of anoddpm_threshold_counts
DEFECTS = ("bottom", "sign", "lowbyte", "above_ge", "pred_ge", "ragged", "shared_prefix")
SELECT_DEFECTS = tuple(d for d in DEFECTS if d != "pred_ge")
COUNT_DEFECTS = ("pred_ge", "ragged")
BIG_N, BIG_RANKS = (1 << 24) + 4097, (0, 167772, (1 << 24) + 4096)      # the ground anoddpm_map_scores refuses


def default_tile(n):
    """Tile 0 of anoddpm_select_wide: n / 2048 rounded up to a multiple of 256, at least 1024 and at most 16384."""
    t = -(-(-(-n // 2048)) // 256) * 256
    return min(max(t, 1024), 16384)


# name -> (n, tile, kind, ranks); n - 1 is written as -1
SELECT = {
    "n1": (1, 256, "errors", (0,)),
    "n63_top": (63, 256, "errors", (0,)),
    "n64_bottom": (64, 256, "errors", (-1,)),
    "n65_both": (65, 256, "errors", (0, -1)),
    "n255": (255, 256, "errors", (0, 127, -1)),
    "n256_bottom": (256, 256, "errors", (-1,)),
    "n257": (257, 256, "errors", (0, 128, -1)),
    "n3001_16ranks": (3001, 256, "errors", (0, 1, 10, 11, 11, 30, 300, 1500, 1500, 2999, 3000, 3000, 7, 2000, 2500, 100)),
    "n70001_t0": (70001, 0, "errors", (0, 700, 35000, -1)),
    "constant": (3001, 256, "constant", (0, 1500, -1)),
    "lowbyte": (3001, 256, "lowbyte", (0, 5, 1500, -1)),      # any two ranks share three bytes
    "topbyte": (257, 256, "topbyte", (0, 100, -1)),
    "halfzero": (3001, 256, "halfzero", (0, 1400, 1600, -1)),
    "tie_run": (3001, 256, "tie_run", (4, 5, 20, 44, 45)),    # 5 ... 44 lie inside one run of equal values
    "nan_last": (3001, 256, "nan", (0, 10)),
    "inf_last": (3001, 256, "inf", (0, 10)),
    "negative_last": (3001, 256, "negative", (0, 10)),
}
STATUS = {"nan_last": NAN_BIT, "inf_last": INF_BIT, "negative_last": NEGATIVE_BIT}
STRIDED = (3, 3001, 3100, 256, (0, 30, 3000))                # S, n, stride, tile, ranks: NaN in the gaps, segment 1 holds an inf


def make_select_case(name):
    """-> (x fp32 [n], ranks tuple, tile)"""
    n, tile, kind, ranks = SELECT[name]
    rng = np.random.default_rng(9950 + sorted(SELECT).index(name))
    x = _errors(rng, (n,))
    if kind == "constant":
        x = np.full((n,), 0.3, np.float32)
    elif kind == "lowbyte":
        x = (np.uint32(0x3f000000) | rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    elif kind == "topbyte":                                  # exponent field at most 0xfe: every pattern is finite
        x = ((rng.integers(0, 128, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456)).view(np.float32)
    elif kind == "halfzero":
        x[::2] = np.float32(0.0)
        x[::4] = np.float32(-0.0)
    elif kind == "tie_run":
        x = (x * np.float32(0.25)).astype(np.float32)
        pos = rng.permutation(n)
        x[pos[:5]] = np.float32(2.0)
        x[pos[5:45]] = np.float32(1.5)
    elif kind == "nan":
        x[-3] = np.nan
    elif kind == "inf":
        x[-2] = np.inf
    elif kind == "negative":
        x[-1] = np.float32(-0.25)
    return x, tuple(r % n for r in ranks), tile


def make_strided():
    """-> (buffer fp32 [S][stride], ranks, tile, n): segment s is buffer[s, :n]; the gaps hold NaN, segment 1 one inf."""
    S, n, stride, tile, ranks = STRIDED
    rng = np.random.default_rng(9990)
    buf = np.full((S, stride), np.nan, np.float32)
    buf[:, :n] = _errors(rng, (S, n))
    buf[1, n - 1] = np.inf
    return buf, ranks, tile, n


def make_big():
    x = _errors(np.random.default_rng(9991), (BIG_N,))
    return x, BIG_RANKS, 0


def _status(x):
    st = 0
    if np.isnan(x).any():
        st |= NAN_BIT
    if np.isinf(x).any():
        st |= INF_BIT
    if (x < 0).any():
        st |= NEGATIVE_BIT
    return st


def select_numpy(x, ranks, tile=0, defect=None):
    """anoddpm_select_wide of ONE segment: dict of `value` fp32 [Q], `above`, `equal` int64 [Q], `topk` fp64 [Q], `max` fp32,
    `mean` fp64, `status` int.  Rank r is the 0-based position from the top.  The float outputs of a segment whose status is
    non-zero are unspecified (the kernel's and these may differ)."""
    x = np.asarray(x, np.float32).reshape(-1)
    if defect == "ragged":                                   # the last, ragged tile never read
        t = tile or default_tile(x.size)
        if x.size > t and x.size % t:
            x = x[:x.size // t * t]
    n = x.size
    bits = x.view(np.uint32) if defect == "sign" else x.view(np.uint32) & ABS
    v = bits.view(np.float32)
    v64 = v.astype(np.float64)
    with np.errstate(invalid="ignore"):
        mx, mean, _ = scores_numpy(x, 1)
    out = {"value": [], "above": [], "equal": [], "topk": [], "max": mx, "mean": mean, "status": _status(x)}
    true = []
    for q, r in enumerate(ranks):
        r = min(int(r), n - 1)
        pos = r if defect == "bottom" else n - 1 - r
        vk = np.partition(bits, pos)[pos]
        true.append(vk)
        if defect == "lowbyte":
            vk = vk & np.uint32(0xffffff00)
        if defect == "shared_prefix" and q > 0 and (vk >> 16) == (true[0] >> 16) and ((vk >> 8) & 255) != ((true[0] >> 8) & 255):
            vk = true[0]                                     # rank q refined inside rank 0's third byte
        hi = bits >= vk if defect == "above_ge" else bits > vk
        above, k = int(hi.sum()), r + 1
        value = float(np.array([vk], np.uint32).view(np.float32)[0])
        with np.errstate(invalid="ignore", over="ignore"):
            topk = (tree_sum(np.where(hi, v64, 0.0)) + float(np.uint32((k - above) & 0xffffffff)) * value) / float(k)
        out["value"].append(np.float32(value))
        out["above"].append(above)
        out["equal"].append(int((bits == vk).sum()))
        out["topk"].append(topk)
    out["value"] = np.array(out["value"], np.float32)
    out["above"], out["equal"] = np.array(out["above"], np.int64), np.array(out["equal"], np.int64)
    out["topk"] = np.array(out["topk"], np.float64)
    return out


def same_select(a, b, floats=True):
    """Bit equality of two `select_numpy`-shaped results; `floats=False` leaves out what a non-zero status leaves unspecified."""
    keys = ("value", "above", "equal", "topk", "max", "mean", "status") if floats else ("status",)
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


# ---------------------------------------------------------------------------------- counts at thresholds
# name -> (S, n, T, kind)
COUNTS = {
    "t1_equal": (1, 257, 1, "equal"),
    "t16_shared": (3, 3001, 16, "shared"),
    "t4_per_segment": (3, 3001, 4, "per_segment"),
    "zeros": (1, 256, 2, "zeros"),
    "n70001": (2, 70001, 8, "shared"),
    "bad_mask": (2, 3001, 3, "bad_mask"),
    "nan_score": (2, 3001, 3, "nan_score"),
}


def make_count_case(name):
    """-> (mask fp32 [S][n] or [n] (one mask for every segment), score fp32 [S][n], thr fp32 [T] or [S][T])"""
    S, n, T, kind = COUNTS[name]
    rng = np.random.default_rng(9970 + sorted(COUNTS).index(name))
    score = _errors(rng, (S, n))
    mask = (rng.random((S, n)) < 0.1).astype(np.float32)
    thr = np.sort(_errors(rng, (T,)))
    if kind == "equal":
        thr[0] = score[0, 7]                                 # a score that occurs: strictly above it is not predicted
    elif kind == "shared":
        mask = mask[0].copy()                                # one mask plane for every segment
        thr[0], thr[1], thr[-1] = np.float32(0.0), score[1, 11], np.float32(score.max() * 2 + 1)      # occurs; above the maximum
    elif kind == "per_segment":
        thr = np.sort(_errors(rng, (S, T)), axis=1)
        thr[2, 1] = score[2, 5]
    elif kind == "zeros":
        score[0, ::2] = np.float32(0.0)
        score[0, ::4] = np.float32(-0.0)
        thr = np.array([0.0, -0.0], np.float32)
    elif kind == "bad_mask":
        mask[1, n - 2] = np.float32(0.5)
    elif kind == "nan_score":
        score[0, n - 1] = np.nan
        mask[0, n - 1] = np.float32(1.0)
        thr[0] = np.float32(0.0)
    return mask, score, thr


def counts_numpy(mask, score, thr, defect=None):
    """anoddpm_threshold_counts: dict of `tp`, `fp` int64 [S][T], `P`, `N` int64 [S], `status` int32 [S].  score [S][n]; mask
    [S][n] or [n]; thr [T] or [S][T].  The prediction at threshold j is `score > thr[j]`."""
    score = np.asarray(score, np.float32)
    S, n = score.shape
    mask = np.broadcast_to(np.asarray(mask, np.float32), (S, n))
    thr = np.asarray(thr, np.float32)
    thr = np.broadcast_to(thr, (S, thr.shape[-1]))
    if defect == "ragged" and n > COUNT_TILE and n % COUNT_TILE:
        n = n // COUNT_TILE * COUNT_TILE
        score, mask = score[:, :n], mask[:, :n]
    with np.errstate(invalid="ignore"):
        pred = score[:, None, :] >= thr[:, :, None] if defect == "pred_ge" else score[:, None, :] > thr[:, :, None]
    pos = mask != 0
    status = np.where(((mask != 0) & (mask != 1)).any(axis=1), BAD_MASK_BIT, 0) | np.where(np.isnan(score).any(axis=1), NAN_BIT, 0)
    return {"tp": (pred & pos[:, None, :]).sum(axis=2).astype(np.int64), "fp": (pred & ~pos[:, None, :]).sum(axis=2).astype(np.int64),
            "P": pos.sum(axis=1).astype(np.int64), "N": (~pos).sum(axis=1).astype(np.int64), "status": status.astype(np.int32)}


def same_counts(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("tp", "fp", "P", "N", "status"))


# ---------------------------------------------------------------------------------- the calibration rule
def rank_of(fpr, negatives):
    """`HealthyPool.thresholds`: k = floor(fpr * negatives) in Python floats."""
    return int(float(fpr) * float(negatives))


def threshold_numpy(v, fpr, negatives=None):
    """The operating threshold: the value of descending rank k -- the smallest pooled value that at most k pooled values exceed."""
    v = np.abs(np.asarray(v, np.float32).reshape(-1))
    return np.sort(v)[::-1][rank_of(fpr, v.size if negatives is None else negatives)]
