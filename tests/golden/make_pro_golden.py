"""Writes tests/golden/pro_kat.npz: the known answers of the per-region overlap tests.  Inputs and expected values come from the
exact restatement tests/pro_cases.py::pro_exact alone (scipy.ndimage.label + rational arithmetic, each value rounded once to
fp64): the reference has no PRO score to contribute.  Small cases are stored with their inputs; the two workload-sized ones as
the SHA-256 of their regenerated inputs and curve plus the scalars.  Run from the repository root:
    python tests/golden/make_pro_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pro_cases as pc  # noqa: E402


def build():
    out = {}
    for name in pc.SMALL + pc.LARGE:
        mask, score, limit, conn = pc.make_case(name)
        small = name in pc.SMALL
        if small:
            out[f"{name}_mask"], out[f"{name}_score"] = mask.astype(np.uint8), score
        else:
            out[f"{name}_sha"] = np.array(pc.sha(mask, score))
        out[f"{name}_limit"], out[f"{name}_connectivity"] = np.float64(limit), np.int64(conn)
        rows = {k: [] for k in ("K", "N", "P", "len", "aupro", "curve_sha")}
        for s in range(score.shape[0]):
            e = pc.pro_exact(pc.segment_mask(mask, score, s), score[s], limit, conn)
            for k in ("K", "N", "P", "aupro"):
                rows[k].append(e[k])
            rows["len"].append(e["fps"].size)
            rows["curve_sha"].append(pc.sha(e["fps"], e["thresholds"], e["pro"]))
            if small:
                out[f"{name}_pro{s}"] = e["pro"]
        for k in ("K", "N", "P", "len"):
            out[f"{name}_{k}"] = np.array(rows[k], np.int64)
        out[f"{name}_aupro"] = np.array(rows["aupro"], np.float64)
        out[f"{name}_curve_sha"] = np.array(rows["curve_sha"])
    return out


def main():
    path = os.path.join(HERE, "pro_kat.npz")
    np.savez_compressed(path, **build())
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
