"""Writes tests/golden/postproc_kat.npz: what scipy returns for the cases of tests/postproc_cases.py --
    scipy.ndimage.median_filter(plane, size=k)                          (default mode="reflect")
    scipy.ndimage.binary_erosion(plane > level, iterations=n)           (default cross, border_value=0)
    scipy.ndimage.label(plane > 0, structure) + numpy.bincount, components below min_size cleared
Run by hand:
    python tests/golden/make_postproc_golden.py
Inputs are not stored: the fixture pins the SHA-256 of the regenerated fp32 inputs.  The outputs are bit-exact, so small cases
are stored in full (binary maps bit-packed) and the 256 x 256 and batch cases as the SHA-256 of the expected fp32 bytes plus a
few crops for diagnosis.  Before anything is written the numpy restatements of postproc_cases have to reproduce every expected
output bit for bit."""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import postproc_cases as pc  # noqa: E402


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def scipy_components(x, min_size, connectivity):
    lab, found = ndimage.label(x > 0, structure=ndimage.generate_binary_structure(2, connectivity))
    keep = np.bincount(lab.ravel(), minlength=found + 1) >= min_size
    keep[0] = False
    return keep[lab].astype(np.float32), (int(found), int(keep.sum()))


def main():
    out = {}

    def store_plane(key, want, full):
        out[key + "_sha"] = np.array(pc.sha(want))
        if full:
            out[key] = want
        else:
            for cname, sl in pc.crops(*want.shape[-2:]).items():
                out[f"{key}_{cname}"] = want[(Ellipsis,) + sl]

    # ---- median
    for name in sorted(pc.MEDIAN):
        x = pc.make_median_case(name)
        out[f"{name}_in_sha"] = np.array(pc.sha(x))
        for k in pc.WINDOWS:
            want = ndimage.median_filter(x, size=k)
            assert want.dtype == np.float32 and same(pc.median_numpy(x, k), want), (name, k)
            store_plane(pc.mkey(name, k), want, name in pc.MEDIAN_FULL)
    buf, planes = pc.make_strided()
    out["strided_in_sha"] = np.array(pc.sha(buf))
    for k in pc.WINDOWS:
        want = np.stack([ndimage.median_filter(p, size=k) for p in planes])
        assert same(pc.median_numpy(planes, k), want)
        store_plane(pc.mkey("strided", k), want, True)
    maps, roi = pc.make_batch()
    out["batch_in_sha"] = np.array(pc.sha(maps, roi))
    want = np.stack([ndimage.median_filter(m[0], size=5) * roi for m in maps])[:, None]
    assert same(pc.median_numpy(maps, 5) * roi, want) and not np.signbit(want).any()
    out["batch_k5_sha"] = np.array(pc.sha(want))
    out["batch_k5_plane_sha"] = np.array([pc.sha(w) for w in want])
    for j in (0, 27, 54):
        for cname, sl in pc.crops(256, 256).items():
            out[f"batch_k5_{j}_{cname}"] = want[j, 0][sl]
    bad = pc.make_bad_batch()
    out["bad_in_sha"] = np.array(pc.sha(bad))
    clean = [j for j in range(bad.shape[0]) if j not in pc.BAD_PLANES]
    out["bad_k5_clean"] = np.stack([ndimage.median_filter(bad[j], size=5) for j in clean])
    assert same(pc.median_numpy(bad[clean], 5), out["bad_k5_clean"])

    # ---- erosion
    for name in sorted(pc.ERODE):
        x, level = pc.make_erode_case(name)
        out[f"{name}_in_sha"] = np.array(pc.sha(x))
        b = x > np.float32(level)
        assert b[0].any() and b[-1].any() and b[:, 0].any() and b[:, -1].any(), name
        for n in pc.ERODE_N:
            want = ndimage.binary_erosion(b, iterations=n).astype(np.float32)
            assert same(pc.erode_numpy(x, n, level), want), (name, n)
            out[pc.ekey(name, n) + "_sha"] = np.array(pc.sha(want))
            out[pc.ekey(name, n) + "_bits"] = np.packbits(want.astype(bool))
            out[pc.ekey(name, n) + "_sum"] = np.int64(want.sum())

    # ---- components
    for name in sorted(pc.COMPONENTS):
        x = pc.make_components_case(name)
        out[f"{name}_in_sha"] = np.array(pc.sha(x))
        for c in (1, 2):
            lab = pc.labels_numpy(x > 0, c)
            for m in pc.COMPONENTS[name]:
                want, counts = scipy_components(x, m, c)
                got, gcounts = pc.components_numpy(x, m, c, labels=lab)
                assert same(got, want) and gcounts == counts, (name, c, m)
                key = pc.ckey(name, c, m)
                out[key + "_sha"] = np.array(pc.sha(want))
                out[key + "_counts"] = np.array(counts, np.int64)
                if name in pc.COMPONENTS_FULL:
                    out[key + "_bits"] = np.packbits(want.astype(bool))
    assert tuple(out["checker_c1_m2_counts"]) == (2048, 0) and tuple(out["checker_c2_m2049_counts"]) == (1, 0)
    assert tuple(out["full_c1_m7_counts"]) == (1, 1) and tuple(out["spiral_c1_m40000_counts"]) == (1, 0)

    out["produced_with"] = np.array(f"scipy {scipy.__version__} ndimage.median_filter / binary_erosion / label + numpy {np.__version__} "
                                    "bincount; the numpy restatements of tests/postproc_cases.py reproduced every output bit for bit")
    path = os.path.join(HERE, "postproc_kat.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} entries; {out['produced_with']}")
    assert os.path.getsize(path) < 108 * 1024


if __name__ == "__main__":
    main()
