"""Writes tests/golden/smooth_kat.npz: what scipy returns for the cases of tests/smooth_cases.py --
    scipy.ndimage.gaussian_filter(plane, sigma, truncate=truncate)      (defaults: order 0, mode="reflect")
    scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius)         (the fp64 taps)
Run by hand:
    python tests/golden/make_smooth_golden.py
Inputs are not stored: the fixture pins the SHA-256 of the regenerated fp32 inputs.  The outputs are bit-exact, so planes of up
to 64 x 64 are stored in full and larger ones as the SHA-256 of the expected fp32 bytes plus a few crops for diagnosis.  Before
anything is written the numpy restatement of smooth_cases has to reproduce every expected output bit for bit."""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage
from scipy.ndimage._filters import _gaussian_kernel1d

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import postproc_cases as pc  # noqa: E402
import smooth_cases as sm  # noqa: E402


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def main():
    out = {}
    for (sigma, truncate), radius in sorted(sm.WEIGHTS.items()):
        want = _gaussian_kernel1d(sigma, 0, radius)
        assert sm.radius_of(sigma, truncate) == radius and same(sm.weights_numpy(sigma, truncate), want), (sigma, truncate)
        out[f"w_s{sigma}_t{truncate}"] = want

    def store(key, x, want):
        assert want.dtype == np.float32
        out[key + "_in_sha"] = np.array(sm.sha(x))
        out[key + "_out_sha"] = np.array(sm.sha(want))
        if want.shape[-2] * want.shape[-1] <= sm.FULL_LIMIT:
            out[key + "_out"] = want
        else:
            for cname, sl in pc.crops(*want.shape[-2:]).items():
                out[f"{key}_out_{cname}"] = want[(Ellipsis,) + sl]

    for name, (shape, sigma, truncate, _) in sorted(sm.GAUSS.items()):
        x = sm.make_gauss_case(name)
        want = ndimage.gaussian_filter(x, sigma, truncate=truncate)
        assert same(sm.gaussian_numpy(x, sigma, truncate), want), name
        store(name, x, want)
    assert (out["g64x64_const_out"] == np.float32(0.7)).all()
    buf, planes = sm.make_strided()
    want = np.stack([ndimage.gaussian_filter(p, 4.0) for p in planes])
    assert same(sm.gaussian_numpy(planes, 4.0), want)
    store("strided", buf, want)
    batch = sm.make_batch()
    want = np.stack([ndimage.gaussian_filter(m[0], 4.0) for m in batch])[:, None]
    assert same(sm.gaussian_numpy(batch, 4.0), want)
    out["batch_in_sha"], out["batch_out_sha"] = np.array(sm.sha(batch)), np.array(sm.sha(want))
    out["batch_out_plane_sha"] = np.array([sm.sha(w) for w in want])
    bad = sm.make_poison()
    clean = [j for j in range(bad.shape[0]) if j != sm.POISON_PLANE]
    out["poison_in_sha"] = np.array(sm.sha(bad))
    out["poison_clean_out"] = np.stack([ndimage.gaussian_filter(bad[j], 4.0) for j in clean])
    assert same(sm.gaussian_numpy(bad[clean], 4.0), out["poison_clean_out"])

    out["produced_with"] = np.array(f"scipy {scipy.__version__} ndimage.gaussian_filter + numpy {np.__version__}; the numpy restatement of "
                                    "tests/smooth_cases.py reproduced every output bit for bit")
    path = os.path.join(HERE, "smooth_kat.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} entries; {out['produced_with']}")
    assert os.path.getsize(path) < 128 * 1024


if __name__ == "__main__":
    main()
