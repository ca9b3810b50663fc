"""Writes tests/golden/roc_kat.npz: what sklearn.metrics.roc_curve / auc -- the two calls behind the reference's
evaluation.ROC_AUC / AUC_score (evaluation.py:79-87) -- return for the cases of tests/roc_cases.py.  Needs sklearn; run by hand:
    python tests/golden/make_roc_golden.py
Small cases store their inputs; the 256^2 maps store the SHA-256 of the regenerated inputs and the expected curve; the 2^22 segment
and the 55-segment batch store per segment AUC, P, N, twoU, curve length and the SHA-256 of the three curve arrays."""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import roc_cases as rc  # noqa: E402


def sk(mask, score):
    from sklearn.metrics import auc, roc_curve
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fpr, tpr, thr = roc_curve(mask, score)
        a = auc(fpr, tpr)
    return fpr, tpr, thr.astype(np.float32), float(a)


def main():
    out = {}
    worst = 0.0

    def check(name, mask, score, fpr, tpr, thr, a):
        """The fixture is sklearn's output; the restatement has to agree with it before anything is written."""
        nonlocal worst
        r = rc.roc_numpy(mask, score)
        got = rc.sklearn_triple(r["fps"], r["tps"], r["thresholds"])
        assert rc.bits_equal(got[0], fpr) and rc.bits_equal(got[1], tpr) and rc.bits_equal(got[2], thr), name
        if np.isnan(a):
            assert np.isnan(r["auc"]), name
        else:
            worst = max(worst, abs(a - r["auc"]))
            assert abs(a - r["auc"]) <= rc.auc_tolerance(score.size), (name, a, r["auc"])
        return r

    for name in rc.SMALL + rc.MAPS:
        mask, score = rc.make_case(name)
        fpr, tpr, thr, a = sk(mask, score)
        check(name, mask, score, fpr, tpr, thr, a)
        if name in rc.SMALL:
            out[f"{name}_mask"], out[f"{name}_score"] = mask, score
        else:
            out[f"{name}_sha"] = np.array(rc.sha_inputs(mask, score))
        out[f"{name}_fpr"], out[f"{name}_tpr"], out[f"{name}_thr"], out[f"{name}_auc"] = fpr, tpr, thr, np.float64(a)

    def summary(prefix, masks, scores):
        rows = {k: [] for k in ("auc", "P", "N", "twoU", "len", "curve_sha")}
        for mask, score in zip(masks, scores):
            fpr, tpr, thr, a = sk(mask, score)
            r = check(prefix, mask, score, fpr, tpr, thr, a)
            rows["auc"].append(a)
            rows["P"].append(r["P"])
            rows["N"].append(r["N"])
            rows["twoU"].append(r["twoU"])
            rows["len"].append(fpr.size)
            rows["curve_sha"].append(rc.sha_curve(fpr, tpr, thr))
        out[f"{prefix}_sha"] = np.array(rc.sha_inputs(masks, scores))
        out[f"{prefix}_auc"] = np.array(rows["auc"], np.float64)
        for k in ("P", "N", "twoU", "len"):
            out[f"{prefix}_{k}"] = np.array(rows[k], np.int64)
        out[f"{prefix}_curve_sha"] = np.array(rows["curve_sha"])

    mask, score = rc.make_case("long")
    summary("long", mask[None], score[None])
    summary("batch", *rc.make_batch())
    path = os.path.join(HERE, "roc_kat.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, largest |auc_sklearn - auc_integer| = {worst:.3g}")


if __name__ == "__main__":
    main()
