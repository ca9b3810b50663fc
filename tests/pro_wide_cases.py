"""Shared by the tests of the chip-wide AUPRO path (csrc/pro_wide.hip): a numpy restatement of its launch sequence -- the (key,
area) pairs sorted per tile with the stable scatter positions of tests/roc_wide_cases.py, the lane-63 totals of the 64-lane group
scans of the descending walk, the carries in pro.hip's wave-chunk order, the per-tile counts with their carries and the compact
run arrays, the trapezoid terms per tile of runs, the 1024-lane sum -- and the inputs constructed for what random data does not
reach.  `defect=` plants one of DEFECTS into the restatement; tests/test_pro_wide_reference.py shows that the case list catches
every one of them.  `pool_numpy` restates metrics.PooledRegionCurves: planes of mixed shapes pooled into one segment.
No device needed."""
import numpy as np

import pr_cases as prc
import pro_cases as pc
import roc_wide_cases as wc

TILES = (256, 1024)
WAVES = pc.WAVES
DEFECTS = ("carry_per_tile", "totals_tile_major", "groups_in_i", "payload_own_rank", "run_end_blind", "term_blind", "trapezoid_per_tile",
           "shared_once")


# ---------------------------------------------------------------------------------------------- constructed inputs
def _plane(H, W, rects, seed, levels=None, shift=0.4):
    mask = np.zeros((1, H, W), np.float32)
    for y, x, h, w in rects:
        mask[0, y:y + h, x:x + w] = 1
    score = pc._scores(np.random.default_rng(seed), mask, shift, levels)[None]
    return mask, score, 0.3, 2


# regions of 1, 2, 3, 7, 6 and 15 pixels: 1 / 3, 1 / 7, 1 / 6 and 1 / 15 are inexact in fp64, so the order of the additions shows
ODD_RECTS = ((1, 1, 1, 1), (3, 5, 1, 2), (6, 2, 1, 3), (9, 9, 1, 7), (12, 20, 2, 3), (17, 3, 3, 5))


def make_last_one():
    """25 x 41 = 1025 elements: at tile 256 the last tile is one element.  Continuous scores: 1025 runs, two rounds of the lane sum."""
    return _plane(25, 41, ODD_RECTS, 700)


def make_full_curve():
    """40 x 33 up to the limit 1.0: every one of the 1320 runs has a term that is not zero, two rounds of the lane sum."""
    mask, score, _, conn = _plane(40, 33, ODD_RECTS + ((25, 8, 9, 11),), 707)
    return mask, score, 1.0, conn


def make_chunk_is_tile():
    """128 x 128 = 16384: the wave chunk is 1024, a multiple of both tiles; few score levels, so runs span the borders."""
    return _plane(128, 128, ODD_RECTS + ((40, 40, 30, 31), (90, 10, 7, 7), (100, 100, 11, 13)), 701, levels=24)


def make_long_run():
    """32 x 32: 600 of 1024 elements share one score, 200 are lower, 224 higher: the run covers the walk's positions 224 ... 823, so
    at tile 256 the tiles 1 and 2 hold no run end at all."""
    mask, score, limit, conn = _plane(32, 32, ODD_RECTS, 702)
    rng = np.random.default_rng(703)
    flat = np.r_[rng.random(200, dtype=np.float32) * np.float32(0.25), np.full(600, 0.5, np.float32),
                 np.float32(0.75) + rng.random(224, dtype=np.float32) * np.float32(0.25)].astype(np.float32)
    return mask, flat[rng.permutation(1024)].reshape(1, 1, 32, 32), limit, conn


def make_all_equal_1024():
    mask, _, limit, conn = _plane(32, 32, ODD_RECTS, 704)
    return mask, np.full((1, 1, 32, 32), 0.375, np.float32), limit, conn


def make_tile_digit():
    """32 x 32: the first 256 elements (rows 0 to 7: tile 0 of the first pass at tile 256) are k / 256 outside every region: their
    keys all end in the byte 0 while the other keys do not.  A skip flag taken from one tile's histogram would leave the pass out."""
    mask, score, limit, conn = _plane(32, 32, tuple((y + 10, x, h, w) for y, x, h, w in ODD_RECTS), 705)
    score[0, 0, :8, :] = (np.arange(256, dtype=np.float32) / np.float32(256)).reshape(8, 32)
    assert not mask[0, :8].any()
    return mask, score, limit, conn


def make_many_ties():
    """40 x 33 with 12 score levels: runs of about a hundred elements that mix regions of different inexact weights."""
    return _plane(40, 33, ODD_RECTS + ((25, 8, 9, 11),), 706, levels=12)


CONSTRUCTED = {"last_one": make_last_one, "chunk_is_tile": make_chunk_is_tile, "long_run": make_long_run, "all_equal_1024": make_all_equal_1024,
               "tile_digit": make_tile_digit, "many_ties": make_many_ties, "full_curve": make_full_curve}


def make_case(name):
    """(mask [m, H, W], score [S, m, H, W], limit, connectivity)."""
    return CONSTRUCTED[name]() if name in CONSTRUCTED else pc.make_case(name)


CPU_CASES = pc.SMALL + (pc.RAGGED,) + tuple(CONSTRUCTED)


def default_tile(n):
    return wc.default_tile(n)


# ---------------------------------------------------------------------------------------------- the launch sequence
def keys_of(area, score):
    bits = (np.asarray(score, np.float32).reshape(-1) + np.float32(0)).view(np.uint32)
    return (bits << np.uint32(1)) | (np.asarray(area).reshape(-1) != 0).astype(np.uint32)


def _exclusive(x):
    return np.cumsum(x) - x


def sort_pass(key, pay, tile, shift, defect=None):
    """One LSD pass over the pairs: the positions of tests/roc_wide_cases.sort_pass, applied to key and payload at once."""
    n = key.size
    T = -(-n // tile)
    dg = ((key >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
    t_of = np.arange(n) // tile
    hist = np.zeros((256, T), np.int64)
    np.add.at(hist, (dg, t_of), 1)
    ex = _exclusive(hist.reshape(-1)).reshape(256, T)        # (digit, tile) order
    if bool((hist.sum(axis=1) == n).any()):                  # the whole segment has one digit: the pass copies
        return key.copy(), pay.copy()
    order = np.lexsort((np.arange(n), dg, t_of))
    g_dg, g_t = dg[order], t_of[order]
    start = np.r_[True, (g_dg[1:] != g_dg[:-1]) | (g_t[1:] != g_t[:-1])]
    first = np.maximum.accumulate(np.where(start, np.arange(n), 0))
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - first
    pos = ex[dg, t_of] + rank
    out_k, out_p = np.zeros_like(key), np.zeros_like(pay)
    out_k[pos] = key
    if defect == "payload_own_rank":                         # the payload ranked by a pass of its own, from the other end
        pos = ex[dg, t_of] + (hist[dg, t_of] - 1 - rank)
    out_p[pos] = pay
    return out_k, out_p


def _carries(gtot, chunk_groups):
    """The carry in front of every group: the groups of a chunk added one after the other to a running carry that starts, for
    chunk c, at ((0 + T_0) + T_1) + ... + T_(c-1), T_v the sequential sum of chunk v's totals from 0.0."""
    NG = gtot.size
    carry = np.zeros(NG, np.float64)
    start = 0.0
    for g0 in range(0, NG, chunk_groups):
        total, run = 0.0, start
        for g in range(g0, min(g0 + chunk_groups, NG)):
            carry[g] = run
            run = run + gtot[g]
            total = total + gtot[g]
        start = start + total
    return carry


def _terms(x, y, x0, y0, limit):
    full = (x - x0) * (y + y0) * 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        yl = y0 + (y - y0) * ((limit - x0) / (x - x0))
    cut = (limit - x0) * (yl + y0) * 0.5
    return np.where(x0 < limit, np.where(x <= limit, full, cut), 0.0)


def wide_numpy(area, score, K, limit, tile, defect=None):
    """What anoddpm_pro_auc_wide computes for one segment (flat int area per pixel, flat fp32 score, K regions) at `tile` elements
    per workgroup: the fields of pc.pro_fp64 and `R`."""
    area = np.asarray(area).reshape(-1).astype(np.int64)
    key, pay = keys_of(area, score), area.copy()
    n = key.size
    T = -(-n // tile)
    assert tile % 256 == 0 and tile >= 256 and T <= wc.MAX_TILES
    for p in range(4):
        key, pay = sort_pass(key, pay, tile, 8 * p, defect)
    # the walk from the highest score down: j = n - 1 - i
    kd, ad = key[::-1], pay[::-1]
    pos = (kd & np.uint32(1)).astype(np.int64)
    sb = kd >> np.uint32(1)
    end = np.r_[sb[1:] != sb[:-1], True]                     # compares against key i - 1, across the tile border
    j_idx = np.arange(n)
    if defect == "run_end_blind":
        end = end | (j_idx % tile == tile - 1)
    w = np.zeros(n, np.float64)
    with np.errstate(divide="ignore"):
        w[pos != 0] = 1.0 / ad[pos != 0].astype(np.float64)
    lead = (-n) % 64 if defect == "groups_in_i" else 0       # groups aligned in i: the first group of the walk is the partial one
    NG = -(-(n + lead) // 64)
    rows = np.zeros((NG, 64), np.float64)
    rows.reshape(-1)[lead:lead + n] = w
    incl = pc._group_scan(rows)
    gtot = incl[:, 63].copy()
    chunk = ((n + WAVES - 1) // WAVES + 63) & ~63
    chunk_groups = {"carry_per_tile": tile // 64, "totals_tile_major": NG}.get(defect, chunk // 64)
    cum = (_carries(gtot, chunk_groups)[:, None] + incl).reshape(-1)[lead:lead + n]
    # per tile of the walk: counts, their carries, the compact run arrays
    t_of = j_idx // tile
    tile_p, tile_e = np.bincount(t_of, pos, T).astype(np.int64), np.bincount(t_of, end, T).astype(np.int64)
    carry_p, carry_e = _exclusive(tile_p), _exclusive(tile_e)
    P, R = int(tile_p.sum()), int(tile_e.sum())
    N = n - P
    runfps, runpro, thr = np.zeros(R, np.int64), np.zeros(R, np.float64), np.zeros(R, np.float32)
    for t in range(T):
        j0, j1 = t * tile, min((t + 1) * tile, n)
        e = np.flatnonzero(end[j0:j1])
        q = carry_e[t] + np.arange(e.size)
        cp = carry_p[t] + np.cumsum(pos[j0:j1])[e]
        runfps[q] = (j0 + e + 1) - cp
        runpro[q] = np.minimum(cum[j0 + e] / np.float64(K), 1.0) if K else np.nan
        thr[q] = sb[j0 + e].astype(np.uint32).view(np.float32)
    out = {"K": int(K), "N": N, "P": P, "R": R, "fps": runfps, "thresholds": thr, "pro": runpro, "n": n}
    if K == 0 or N == 0:
        out["aupro"] = float("nan")
        return out
    # the trapezoid: terms per tile of runs, point q - 1 read across the border; then the 1024-lane sum over all of them
    x, y = runfps.astype(np.float64) / np.float64(N), runpro
    x0, y0 = np.r_[0.0, x[:-1]], np.r_[0.0, y[:-1]]
    if defect == "term_blind":
        first = np.arange(R) % tile == 0
        x0, y0 = np.where(first, 0.0, x0), np.where(first, 0.0, y0)
    terms = _terms(x, y, x0, y0, np.float64(limit))
    if defect == "trapezoid_per_tile":
        total = 0.0
        for q0 in range(0, R, tile):
            total = total + prc._kernel_sum(terms[q0:q0 + tile])
    else:
        total = prc._kernel_sum(terms)
    out["aupro"] = float(total) / float(limit)
    return out


def wide_case(mask, score, limit, connectivity, tile, defect=None):
    """wide_numpy of one segment of a case: mask [m, H, W], score [m, H, W]."""
    area, counts = pc.regions(mask, connectivity)
    return wide_numpy(area, score, int(counts.sum()), limit, tile, defect)


FIELDS = ("K", "N", "P", "fps", "thresholds", "pro", "aupro")


def differences(got, want):
    """Names of the fields in which two results differ bit for bit; empty when they agree."""
    bad = [k for k in ("K", "N", "P") if got[k] != want[k]]
    bad += [k for k in ("fps",) if not np.array_equal(got[k], want[k])]
    bad += [k for k in ("thresholds", "pro") if np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes()]
    bad += [] if np.float64(got["aupro"]).tobytes() == np.float64(want["aupro"]).tobytes() else ["aupro"]
    return bad


def case_differences(name, tile, defect=None):
    """wide_numpy (with `defect`) against pc.pro_fp64 on every segment of a case."""
    mask, score, limit, conn = make_case(name)
    bad = []
    for s in range(score.shape[0]):
        m = pc.segment_mask(mask, score, s)
        bad += differences(wide_case(m, score[s], limit, conn, tile, defect), pc.pro_fp64(m, score[s], limit, conn))
    return bad


# ---------------------------------------------------------------------------------------------- the pool
def pool_adds():
    """The adds of the pooled-run tests: (mask [..., H, W], score) pairs of three plane shapes; the third add shares one mask plane
    among three score planes.  Regions of inexact weight in every add."""
    rng = np.random.default_rng(710)
    adds = []
    for H, W, planes in ((16, 16, 2), (40, 33, 1), (5, 7, 1)):
        rects = tuple(r for r in ODD_RECTS if r[0] + r[2] <= H and r[1] + r[3] <= W)
        mask = np.zeros((planes, H, W), np.float32)
        for p in range(planes):
            for y, x, h, w in rects[p:]:
                mask[p, y:y + h, x:x + w] = 1
        adds.append((mask, pc._scores(rng, mask, levels=20 if H == 40 else None)))
    shared = np.zeros((1, 16, 16), np.float32)
    for y, x, h, w in ((2, 2, 1, 3), (8, 4, 1, 7), (12, 12, 3, 3)):
        shared[0, y:y + h, x:x + w] = 1
    adds.append((shared, np.stack([pc._scores(rng, shared, shift) for shift in (0.1, 0.4, 0.9)])[:, 0]))
    return adds


def pool_numpy(adds, limit, connectivity, tile, defect=None):
    """The pooled segment of `adds` through wide_numpy: scipy's areas per mask plane, a mask shared by k score planes written out k
    times, and every (mask plane, score plane) pair an image of the set: the regions of a shared mask count k times."""
    areas, scores, K = [], [], 0
    for mask, score in adds:
        H, W = mask.shape[-2:]
        a, counts = pc.regions(mask.reshape(-1, H, W), connectivity)
        k = score.size // mask.size
        areas += [a.reshape(-1)] * k
        scores.append(score.reshape(-1))
        K += int(counts.sum()) * (1 if defect == "shared_once" else k)
    return wide_numpy(np.concatenate(areas), np.concatenate(scores), K, limit, tile, defect)
