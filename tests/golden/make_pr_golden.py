"""Writes tests/golden/pr_kat.npz: what sklearn.metrics.precision_recall_curve / average_precision_score return for the cases of
tests/pr_cases.py, and the best Dice 2 tp / (tp + fp + P) over all thresholds -- with the highest threshold that reaches it and
tp / fp there -- found by brute force over every distinct score with fractions.Fraction.  Needs sklearn; run by hand:
    python tests/golden/make_pr_golden.py
Small cases store their inputs and the three curve arrays; the 256^2 maps, the 2^22 segment and the 55-segment batch store per
segment the SHA-256 of the regenerated inputs, curve length, SHA-256 of the three curve arrays and the scalars.  Where a segment
has no positive the recorded best Dice is NaN (every threshold gives 0); sklearn's AP is recorded as it is (0.0 there)."""
import os
import sys
import warnings
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pr_cases as pc  # noqa: E402
import roc_cases as rc  # noqa: E402


def sk(mask, score):
    from sklearn.metrics import average_precision_score, precision_recall_curve
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prec, rec, thr = precision_recall_curve(mask, score)
        ap = average_precision_score(mask, score)
    return prec, rec, thr.astype(np.float32), float(ap)


def brute_best_dice(mask, score):
    """Independent of the key sort: descending stable argsort, cumulative counts, one Fraction per distinct score."""
    score = (score + np.float32(0)).astype(np.float32)              # -0.0 is +0.0
    order = np.argsort(-score, kind="stable")
    s, m = score[order], (mask[order] != 0).astype(np.int64)
    last = np.r_[np.flatnonzero(s[1:] != s[:-1]), s.size - 1]       # last index of every distinct score, highest first
    tp, P = np.cumsum(m)[last].tolist(), int(m.sum())
    fp = ((last + 1) - np.cumsum(m)[last]).tolist()
    best, best_i = None, None
    for i in range(len(tp)):                                         # highest threshold first: only a strictly larger Dice replaces it
        d = Fraction(2 * tp[i], tp[i] + fp[i] + P)
        if best is None or d > best:
            best, best_i = d, i
    dice = float("nan") if P == 0 else float(best)                   # float(Fraction) rounds correctly
    return dice, s[last[best_i]], tp[best_i], fp[best_i]


def main():
    out = {}
    worst = 0.0

    def check(name, mask, score, prec, rec, thr, ap, brute):
        """The fixture is sklearn's and the brute-force output; the restatement has to agree with it before anything is written."""
        nonlocal worst
        r = pc.pr_numpy(mask, score)
        got = pc.sklearn_triple(r["fps"], r["tps"], r["thresholds"])
        assert rc.bits_equal(got[0], prec) and rc.bits_equal(got[1], rec) and rc.bits_equal(got[2], thr), name
        if r["P"] == 0:
            assert np.isnan(r["ap"]) and ap == 0.0, (name, ap)
        else:
            worst = max(worst, abs(ap - r["ap"]))
            assert abs(ap - r["ap"]) <= pc.ap_tolerance(score.size), (name, ap, r["ap"])
        assert pc.same_float(r["best_dice"], brute[0]) and rc.bits_equal(np.float32(r["best_threshold"]), np.float32(brute[1])), name
        assert (r["best_tp"], r["best_fp"]) == (brute[2], brute[3]), name
        return r

    for name in pc.SMALL:
        mask, score = pc.make_case(name)
        prec, rec, thr, ap = sk(mask, score)
        brute = brute_best_dice(mask, score)
        check(name, mask, score, prec, rec, thr, ap, brute)
        out[f"{name}_mask"], out[f"{name}_score"] = mask, score
        out[f"{name}_prec"], out[f"{name}_rec"], out[f"{name}_thr"], out[f"{name}_ap"] = prec, rec, thr, np.float64(ap)
        out[f"{name}_best_dice"], out[f"{name}_best_thr"] = np.float64(brute[0]), np.float32(brute[1])
        out[f"{name}_best_tp"], out[f"{name}_best_fp"] = np.int64(brute[2]), np.int64(brute[3])

    def summary(prefix, masks, scores):
        rows = {k: [] for k in ("ap", "P", "len", "curve_sha", "best_dice", "best_thr", "best_tp", "best_fp")}
        for mask, score in zip(masks, scores):
            prec, rec, thr, ap = sk(mask, score)
            brute = brute_best_dice(mask, score)
            r = check(prefix, mask, score, prec, rec, thr, ap, brute)
            for k, v in (("ap", ap), ("P", r["P"]), ("len", prec.size), ("curve_sha", rc.sha_curve(prec, rec, thr)),
                         ("best_dice", brute[0]), ("best_thr", brute[1]), ("best_tp", brute[2]), ("best_fp", brute[3])):
                rows[k].append(v)
        out[f"{prefix}_sha"] = np.array(rc.sha_inputs(masks, scores))
        out[f"{prefix}_ap"], out[f"{prefix}_best_dice"] = np.array(rows["ap"], np.float64), np.array(rows["best_dice"], np.float64)
        out[f"{prefix}_best_thr"] = np.array(rows["best_thr"], np.float32)
        for k in ("P", "len", "best_tp", "best_fp"):
            out[f"{prefix}_{k}"] = np.array(rows[k], np.int64)
        out[f"{prefix}_curve_sha"] = np.array(rows["curve_sha"])

    for name in pc.SUMMARISED:
        mask, score = pc.make_case(name)
        summary(name, mask[None], score[None])
    summary("batch", *rc.make_batch())
    path = os.path.join(HERE, "pr_kat.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, largest |ap_sklearn - ap_restatement| = {worst:.3g}")


if __name__ == "__main__":
    main()
