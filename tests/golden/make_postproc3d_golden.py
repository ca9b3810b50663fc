"""Writes tests/golden/postproc3d_kat.npz: what scipy returns for the cases of tests/postproc3d_cases.py --
    scipy.ndimage.median_filter(vol, size=k)                            (default mode="reflect", all three axes)
    scipy.ndimage.binary_erosion(vol > level, iterations=n)             (default 6-neighbour cross, border_value=0)
    scipy.ndimage.label(vol > 0, generate_binary_structure(3, c)) + numpy.bincount, components below min_size cleared
Run by hand:
    python tests/golden/make_postproc3d_golden.py
Inputs are not stored: the fixture pins the SHA-256 of the regenerated fp32 inputs.  The outputs are bit-exact, so small cases
are stored in full (binary volumes bit-packed) and the larger ones as the SHA-256 of the expected bytes plus a few crops for
diagnosis.  Before anything is written the numpy restatements of postproc3d_cases have to reproduce every expected output bit
for bit, and every erosion result has to be neither empty nor full unless its case says so."""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import postproc3d_cases as pc  # noqa: E402


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def scipy_labels(x, connectivity):
    return ndimage.label(x > 0, structure=ndimage.generate_binary_structure(3, connectivity))


def scipy_components(x, min_size, connectivity):
    lab, found = scipy_labels(x, connectivity)
    keep = np.bincount(lab.ravel(), minlength=found + 1) >= min_size
    keep[0] = False
    return keep[lab].astype(np.float32), (int(found), int(keep.sum()))


def main():
    out = {}

    def store_volume(key, want, full):
        out[key + "_sha"] = np.array(pc.sha(want))
        if full:
            out[key] = want
        else:
            for cname, sl in pc.crops(*want.shape[-3:]).items():
                out[f"{key}_{cname}"] = np.ascontiguousarray(want[sl])

    for name in sorted(pc.MEDIAN):
        x = pc.make_median_case(name)
        out[f"{name}_in_sha"] = np.array(pc.sha(x))
        for k in pc.WINDOWS:
            want = ndimage.median_filter(x, size=k)
            assert same(want, pc.median3d_numpy(x, k)), (name, k)
            store_volume(pc.mkey(name, k), want, name in pc.MEDIAN_FULL)

    buf, vols, plane, roi_vol, roi_batch = pc.make_batch()
    out["batch_in_sha"] = np.array(pc.sha(buf, plane, roi_vol, roi_batch))
    for k in pc.WINDOWS:
        want = np.stack([ndimage.median_filter(v, size=k) for v in vols])
        assert same(want, pc.median3d_numpy(vols, k)), k
        out[f"batch_k{k}_sha"] = np.array(pc.sha(want))
        out[f"batch_k{k}_volume_sha"] = np.array([pc.sha(v) for v in want])
    bad = pc.make_bad_batch()
    out["bad_in_sha"] = np.array(pc.sha(bad))
    for k in pc.WINDOWS:
        out[f"bad_k{k}_clean"] = ndimage.median_filter(bad[3], size=k)
        assert same(out[f"bad_k{k}_clean"], pc.median3d_numpy(bad[3], k))

    for name in sorted(pc.ERODE):
        x, level = pc.make_erode_case(name)
        out[f"{name}_in_sha"] = np.array(pc.sha(x))
        for n in pc.ERODE_N:
            want = ndimage.binary_erosion(x > np.float32(level), iterations=n).astype(np.float32)
            assert same(want, pc.erode3d_numpy(x, n, level)), (name, n)
            assert (not want.any()) == ((name, n) in pc.ERODE_EMPTY) and not want.all(), (name, n, int(want.sum()))
            key = pc.ekey(name, n)
            out[key + "_bits"] = np.packbits(want.astype(bool))
            out[key + "_sha"] = np.array(pc.sha(want))
            out[key + "_sum"] = np.array(int(want.sum()))
    assert int(out["ones19x21x40_n8_sum"]) == 3 * 5 * 24

    for name in sorted(pc.COMPONENTS):
        x = pc.make_components_case(name)
        out[f"{name}_in_sha"] = np.array(pc.sha(x))
        for c in pc.CONNECTIVITY:
            lab = pc.labels3d_numpy(x > 0, c)
            for m in pc.COMPONENTS[name]:
                want, counts = scipy_components(x, m, c)
                got, gcounts = pc.components3d_numpy(x, m, c, labels=lab)
                assert same(want, got) and counts == gcounts, (name, c, m)
                key = pc.ckey(name, c, m)
                out[key + "_counts"] = np.array(counts, np.int64)
                out[key + "_sha"] = np.array(pc.sha(want))
                if name in pc.COMPONENTS_FULL:
                    out[key + "_bits"] = np.packbits(want.astype(bool))
            sl, found = scipy_labels(x, c)
            areas = np.where(sl > 0, np.bincount(sl.ravel())[sl], 0).astype(np.int32)
            garea, gfound = pc.areas3d_numpy(x, c)
            assert same(areas, garea) and found == gfound, (name, c)
            out[f"{name}_c{c}_areas_sha"] = np.array(pc.sha(areas))
            out[f"{name}_c{c}_areas_count"] = np.array(int(found))
    sizes = sorted(np.unique(pc.areas3d_numpy(pc.make_components_case("blobs"), 1)[0]).tolist())
    assert sizes[0] == 0 and sizes[1] < 7 < sizes[-1], sizes

    real, recon, mask = pc.make_scene()
    out["scene_in_sha"] = np.array(pc.sha(real, recon, mask))
    d = recon - real
    sq = (d * d).astype(np.float32)
    roi = np.stack([ndimage.binary_erosion(v > np.float32(pc.SCENE_ROI_LEVEL), iterations=1) for v in real]).astype(np.float32)
    sq_pp = np.stack([ndimage.median_filter(v, size=3) for v in sq]) * roi
    pred_pp = np.stack([scipy_components((v > np.float32(0.5)).astype(np.float32), 7, 1)[0] for v in sq_pp])
    assert same(sq_pp, pc.median3d_numpy(sq, 3) * pc.erode3d_numpy(real, 1, pc.SCENE_ROI_LEVEL))
    out["scene_sqerr_pp_sha"] = np.array(pc.sha(sq_pp))
    out["scene_pred_pp_bits"] = np.packbits(pred_pp.astype(bool))

    out["produced_with"] = np.array(f"scipy {scipy.__version__} (ndimage.median_filter size=k mode=reflect on [D][H][W]; ndimage.binary_erosion "
                                    f"iterations=n, 6-neighbour cross, border_value=0; ndimage.label with generate_binary_structure(3, c) + "
                                    f"numpy.bincount), numpy {np.__version__}")
    path = os.path.join(HERE, "postproc3d_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
