"""Writes tests/golden/surface_kat.npz: the known answers of the distance-transform and boundary-distance tests.  Inputs and
expected values come from scipy alone through tests/surface_cases.py (scipy.ndimage.distance_transform_edt, binary_erosion and
the percentile the header defines): the reference has no boundary distance to contribute.  Small cases are stored with their
inputs; the workload-sized ones as the SHA-256 of their regenerated inputs and of the transform, plus the scalars.  Run from the
repository root:
    python tests/golden/make_surface_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import surface_cases as sc  # noqa: E402


def build():
    out = {}
    cases = sc.transform_cases()
    for name in sc.SMALL_TRANSFORM + sc.LARGE_TRANSFORM:
        planes, level = cases[name]
        fg = sc.foreground(planes, level)
        sq = np.stack([sc.edt2_brute(f) for f in fg]).astype(np.int32)
        dist = np.stack([sc.edt_scipy(f) if not f.all() else np.full(f.shape, np.inf) for f in fg])
        if name in sc.SMALL_TRANSFORM:
            out[f"dt_{name}_fg"], out[f"dt_{name}_sq"] = fg.astype(np.uint8), sq
        out[f"dt_{name}_sha"] = np.array(sc.sha(fg.astype(np.uint8), sq, dist))
    cases = sc.surface_cases()
    for name in sc.SMALL_SURFACE + sc.LARGE_SURFACE:
        pred, ref = cases[name]
        res = [sc.surface_ref(p, r) for p, r in sc.pairs_of(pred, ref)]
        if name in sc.SMALL_SURFACE:
            out[f"sd_{name}_pred"], out[f"sd_{name}_ref"] = pred.astype(np.uint8), ref.astype(np.uint8)
        else:
            out[f"sd_{name}_sha"] = np.array(sc.sha(pred, ref))
        for k in ("counts", "max2", "mean", "p95"):
            out[f"sd_{name}_{k}"] = np.stack([r[k] for r in res])
        out[f"sd_{name}_status"] = np.array([r["status"] for r in res], np.int32)
    return out


def main():
    path = os.path.join(HERE, "surface_kat.npz")
    np.savez_compressed(path, **build())
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
