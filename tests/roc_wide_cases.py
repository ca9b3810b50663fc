"""Shared by the tests of the chip-wide ROC / PR path (csrc/roc_wide.hip): a numpy restatement of its launch sequence -- tile
histograms, the (digit, tile) scan, the stable scatter positions, the skip decision taken from the whole segment, per-tile run
and positive counts with their carries, per-tile twoU, the offsets of the kept curve points, the average-precision term array
summed in the order of pr_cases._kernel_sum -- and the inputs constructed for what random data does not reach.  `defect=` plants
one of DEFECTS into the restatement; tests/test_roc_wide_reference.py shows that the case list catches every one of them.
No device needed."""
import numpy as np

import pr_cases as pc
import roc_cases as rc

TILES = (256, 1024)
MAX_TILES = 2048                                             # ANODDPM_ROC_WIDE_MAX_TILES
DEFAULT_TILE = 4096
DEFECTS = ("scan_tile_major", "reverse_rank", "tile_first_blind", "keep_blind", "ap_per_tile", "skip_from_tile")


# ---------------------------------------------------------------------------------------------- constructed inputs
def make_long_run(n=1024):
    """600 of 1024 elements share one score; 200 are lower, 224 higher: after sorting the run covers positions 200 ... 799, so at
    tile 256 the tiles 1 and 2 hold no run start at all and their first keys continue a run of the tile before."""
    rng = np.random.default_rng(500)
    score = np.r_[rng.random(200, dtype=np.float32) * np.float32(0.25), np.full(600, 0.5, np.float32),
                  np.float32(0.75) + rng.random(n - 800, dtype=np.float32) * np.float32(0.25)].astype(np.float32)
    mask = (rng.random(n) < 0.3).astype(np.float32)
    order = rng.permutation(n)
    return mask[order], score[order]


def make_tile_digit(n=1024):
    """The first 256 elements (tile 0 of the first pass at tile 256) are k / 256 with mask 0: their keys all end in the byte 0,
    while the other keys, random scores, do not.  A skip flag taken from tile 0's histogram would leave the first pass out.
    Random data does not produce a tile of one digit, hence this input."""
    rng = np.random.default_rng(501)
    mask, score = rc._scores(rng, n, 0.3)
    score[:256] = (np.arange(256, dtype=np.float32) / np.float32(256)).astype(np.float32)
    mask[:256] = 0.0
    key = keys_of(mask, score)
    assert np.unique(key[:256] & 255).size == 1 and np.unique(key & 255).size > 1
    return mask, score


def make_border_keep(n=2304):
    """n distinct scores and three positives: every other run is one negative, so sklearn drops almost every point -- also the
    runs next to each border between tiles of runs (R = n > 1024: several tiles at both tile sizes), which a keep_point that
    cannot see across the border keeps.  The random cases with that many runs happen to have the same property; this one has it
    by construction."""
    rng = np.random.default_rng(502)
    score = (rng.permutation(n).astype(np.float32) / np.float32(n)).astype(np.float32)
    mask = np.zeros(n, np.float32)
    mask[[3, n // 2, n - 5]] = 1.0
    return mask, score


CONSTRUCTED = {"long_run": make_long_run, "tile_digit": make_tile_digit, "border_keep": make_border_keep}
BORDERS = ("long_run", "tile_digit", "all_equal_1024")       # the n = 1024 cases of the GPU test of constructed borders


def make_case(name):
    if name in CONSTRUCTED:
        return CONSTRUCTED[name]()
    if name == "all_equal_1024":                             # every pass may skip
        mask, _ = rc._scores(np.random.default_rng(503), 1024, 0.2)
        return mask, np.full(1024, 0.375, np.float32)
    if name == "ragged":
        return rc.make_ragged()
    return pc.make_case(name)


CPU_CASES = pc.SMALL + ("ragged",) + tuple(CONSTRUCTED) + ("all_equal_1024",) + rc.MAPS


def default_tile(n):
    per = -(-n // MAX_TILES)
    return max(DEFAULT_TILE, -(-per // 256) * 256)


# ---------------------------------------------------------------------------------------------- the launch sequence
def keys_of(mask, score):
    mask = np.asarray(mask, np.float32).reshape(-1)
    score = np.asarray(score, np.float32).reshape(-1)
    bits = (score + np.float32(0)).view(np.uint32)
    return (bits << np.uint32(1)) | (mask != 0).astype(np.uint32)


def _exclusive(x):
    return np.cumsum(x) - x


def sort_pass(key, tile, shift, defect=None):
    """One LSD pass: (keys after the pass, whether it was skipped)."""
    n = key.size
    T = -(-n // tile)
    dg = ((key >> np.uint32(shift)) & np.uint32(255)).astype(np.int64)
    t_of = np.arange(n) // tile
    hist = np.zeros((256, T), np.int64)                      # digit-major, one column per tile
    np.add.at(hist, (dg, t_of), 1)
    if defect == "scan_tile_major":
        ex = _exclusive(hist.T.reshape(-1)).reshape(T, 256).T
    else:
        ex = _exclusive(hist.reshape(-1)).reshape(256, T)    # (digit, tile) order
    if defect == "skip_from_tile":
        skip = bool((hist[:, 0] == min(tile, n)).any())
    else:
        skip = bool((hist.sum(axis=1) == n).any())           # the whole segment has one digit
    if skip:
        return key.copy(), True
    # rank of a key among the keys of its tile with its digit, in tile order (what the wave chunks and ballots give)
    order = np.lexsort((np.arange(n), dg, t_of))
    g_dg, g_t = dg[order], t_of[order]
    start = np.r_[True, (g_dg[1:] != g_dg[:-1]) | (g_t[1:] != g_t[:-1])]
    first = np.maximum.accumulate(np.where(start, np.arange(n), 0))
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - first
    if defect == "reverse_rank":
        rank = hist[dg, t_of] - 1 - rank
    pos = ex[dg, t_of] + rank
    out = np.zeros_like(key)
    ok = pos < n                                             # the guard of every scatter store
    out[pos[ok]] = key[ok]
    return out, False


def wide_numpy(mask, score, tile, defect=None):
    """What anoddpm_roc_auc_wide computes for one segment at `tile` keys per workgroup: the fields of rc.roc_numpy (the kept
    points under `fps` / `tps` / `thresholds`), those of pc.pr_numpy (every point under `all_fps` / `all_tps` /
    `all_thresholds`), the `skipped` passes and the `terms` array."""
    key = keys_of(mask, score)
    n = key.size
    T = -(-n // tile)
    assert tile % 256 == 0 and tile >= 256 and T <= MAX_TILES
    skipped = []
    for p in range(4):
        key, sk = sort_pass(key, tile, 8 * p, defect)
        skipped.append(sk)
    s, lab = key >> np.uint32(1), (key & np.uint32(1)).astype(np.int64)
    # runs: per-tile counts, their carries, the compacted records
    idx = np.arange(n)
    bnd = np.r_[True, s[1:] != s[:-1]]                       # a tile's first key looks at the previous tile's last key
    if defect == "tile_first_blind":
        bnd = bnd | (idx % tile == 0)
    t_of = idx // tile
    tile_b, tile_p = np.bincount(t_of, bnd, T).astype(np.int64), np.bincount(t_of, lab, T).astype(np.int64)
    carry_b, carry_p = _exclusive(tile_b), _exclusive(tile_p)
    R, P = int(tile_b.sum()), int(tile_p.sum())
    runpos, runtp = np.empty(R + 1, np.int64), np.empty(R + 1, np.int64)
    for t in range(T):
        i0, i1 = t * tile, min((t + 1) * tile, n)
        starts = np.flatnonzero(bnd[i0:i1])
        r = carry_b[t] + np.arange(starts.size)
        runpos[r] = i0 + starts
        runtp[r] = carry_p[t] + _exclusive(lab[i0:i1])[starts]
    runpos[R], runtp[R] = n, P
    # per run, in tiles of `tile` runs from the highest score down (q = R - 1 - r)
    p_r = np.diff(runtp)
    n_r = np.diff(runpos) - p_r
    term_u = p_r * (2 * (runpos[:-1] - runtp[:-1]) + n_r)
    keep = np.ones(R, bool)
    if R > 2:
        keep[1:R - 1] = (p_r[1:R - 1] != p_r[0:R - 2]) | (n_r[1:R - 1] != n_r[0:R - 2])
    q_of = R - 1 - np.arange(R)
    if defect == "keep_blind":                               # a run at the edge of its tile is taken for an end of the curve
        keep = keep | (q_of % tile == 0) | (q_of % tile == tile - 1)
    TR = -(-R // tile)
    j_of = q_of // tile
    tile_u = np.bincount(j_of, term_u.astype(np.float64), TR)                # exact below 2^53: the cases are far smaller
    two_u = int(sum(int(term_u[j_of == j].sum()) for j in range(TR)))
    assert two_u == int(tile_u.sum())
    tile_k = np.bincount(j_of, keep, TR).astype(np.int64)
    carry_k = _exclusive(tile_k)
    K = int(tile_k.sum())
    tps_r, cnt_r = P - runtp[:-1], n - runpos[:-1]
    thr_r = (key[runpos[:-1]] >> np.uint32(1)).astype(np.uint32).view(np.float32)
    fps, tps, thr = np.empty(K, np.int64), np.empty(K, np.int64), np.empty(K, np.float32)
    for j in range(TR):
        r = np.flatnonzero((j_of == j) & keep)[::-1]         # descending score inside the tile
        o = carry_k[j] + np.arange(r.size)
        tps[o], fps[o], thr[o] = tps_r[r], cnt_r[r] - tps_r[r], thr_r[r]
    # average precision: the chip fills the term array, one small launch adds it in the order of roc.hip step 6
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = np.where(p_r != 0, (p_r.astype(np.float64) / np.float64(P)) * (tps_r.astype(np.float64) / cnt_r.astype(np.float64)), 0.0)
    if P == 0:
        ap = float("nan")
    elif P == n:
        ap = 1.0
    elif defect == "ap_per_tile":
        ap = 0.0
        for j in range(TR):
            ap = ap + pc._kernel_sum(terms[j_of == j][::-1])
        ap = float(ap)
    else:
        ap = pc._kernel_sum(terms)
    # best Dice: one candidate per tile of runs, then over the tiles -- the order is total, so any shape gives the same run
    def better(a, b):
        x, y = int(tps_r[a]) * (int(cnt_r[b]) + P), int(tps_r[b]) * (int(cnt_r[a]) + P)
        return x > y or (x == y and a > b)
    cands = []
    for j in range(TR):
        best = None
        for r in np.flatnonzero(j_of == j).tolist():
            if best is None or better(r, best):
                best = r
        cands.append(best)
    best = cands[0]
    for c in cands[1:]:
        if better(c, best):
            best = c
    btp, bden = int(tps_r[best]), int(cnt_r[best]) + P
    N = n - P
    return {"P": P, "N": N, "twoU": two_u, "R": R, "auc": float("nan") if P == 0 or N == 0 else two_u / (2.0 * P * N),
            "fps": fps, "tps": tps, "thresholds": thr, "skipped": skipped, "terms": terms,
            "all_fps": (cnt_r - tps_r)[::-1], "all_tps": tps_r[::-1], "all_thresholds": thr_r[::-1], "ap": ap,
            "best_dice": float("nan") if P == 0 else (2 * btp) / bden, "best_threshold": thr_r[best], "best_tp": btp, "best_fp": bden - P - btp}


def differences(mask, score, tile, defect=None):
    """Names of the fields in which wide_numpy (with `defect`) differs from rc.roc_numpy / pc.pr_numpy; empty when it agrees."""
    w, r, p = wide_numpy(mask, score, tile, defect), rc.roc_numpy(mask, score), pc.pr_numpy(mask, score)
    bad = [k for k in ("P", "N", "twoU", "R") if w[k] != r[k]]
    bad += [k for k in ("fps", "tps") if not np.array_equal(w[k], r[k])]
    bad += [] if rc.bits_equal(w["thresholds"], r["thresholds"]) else ["thresholds"]
    bad += [] if pc.same_float(w["auc"], r["auc"]) else ["auc"]
    bad += ["all_" + k for k in ("fps", "tps") if not np.array_equal(w["all_" + k], p[k])]
    bad += [] if rc.bits_equal(w["all_thresholds"], p["thresholds"]) else ["all_thresholds"]
    bad += [k for k in ("ap", "best_dice") if not pc.same_float(w[k], p[k])]
    bad += [] if rc.bits_equal(np.float32(w["best_threshold"]), np.float32(p["best_threshold"])) else ["best_threshold"]
    bad += [k for k in ("best_tp", "best_fp") if w[k] != p[k]]
    return bad
