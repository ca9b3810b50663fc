"""Writes tests/golden/gauss3d.npz: what scipy returns for the cases of tests/gauss3d_cases.py --
    scipy.ndimage.gaussian_filter(vol, (sz, sy, sx), truncate=4.0)      (defaults: order 0, mode="reflect"), per volume
    scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius)         (the fp64 taps of every filtered axis)
Run by hand:
    python tests/golden/make_gauss3d_golden.py
Inputs are not stored: the fixture pins the SHA-256 of the regenerated fp32 inputs.  The outputs are bit-exact, so outputs of up
to 4096 voxels are stored in full and larger ones as the SHA-256 of the expected fp32 bytes.  Before anything is written the numpy
restatement of gauss3d_cases has to reproduce every expected output bit for bit."""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage
from scipy.ndimage._filters import _gaussian_kernel1d

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gauss3d_cases as gc  # noqa: E402
import smooth_cases as sm  # noqa: E402


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def scipy_volumes(x, sigma):
    """gaussian_filter of every [D][H][W] volume of x."""
    flat = x.reshape((-1,) + x.shape[-3:])
    return np.stack([ndimage.gaussian_filter(v, gc.sigmas_of(sigma), truncate=gc.TRUNCATE) for v in flat]).reshape(x.shape)


def main():
    out = {}
    for sigma, truncate in gc.tables_used():
        radius = gc.radius_of(sigma, truncate)
        want = _gaussian_kernel1d(sigma, 0, radius)
        assert 1 <= radius <= gc.MAX_RADIUS and same(sm.weights_numpy(sigma, truncate), want), (sigma, truncate)
        out[f"w_s{sigma}_t{truncate}"] = want

    def store(key, pinned, vols, sigma):
        """`pinned`: the regenerated input whose SHA-256 is kept; `vols`: the volumes in it."""
        want = scipy_volumes(vols, sigma)
        got = gc.gaussian3d_numpy(vols, sigma)
        assert want.dtype == np.float32 and same(got, want), f"{key}: the restatement differs from scipy in {int((got != want).sum())} voxels"
        out[key + "_in_sha"] = np.array(gc.sha(pinned))
        out[key + "_out_sha"] = np.array(gc.sha(want))
        if want.size <= gc.FULL_LIMIT:
            out[key + "_out"] = want

    for name, (shape, sigma) in sorted(gc.CASES.items()):
        x = gc.make_case(name)
        assert x.shape == shape and np.isfinite(x).all() and (x >= 0).all()
        store(name, x, x, sigma)
    buf, vols = gc.make_strided()
    store("strided", buf, vols, gc.BATCH5[1])
    b5 = gc.make_batch5()
    store("batch5", b5, b5, gc.BATCH5[1])
    bad = gc.make_poison()
    shape, sigma, v, _ = gc.POISON
    clean = [j for j in range(shape[0]) if j != v]
    out["poison_in_sha"] = np.array(gc.sha(bad))
    want = scipy_volumes(bad[clean], sigma)
    assert same(gc.gaussian3d_numpy(bad[clean], sigma), want)
    out["poison_clean_out_sha"] = np.array(gc.sha(want))

    out["produced_with"] = np.array(f"scipy {scipy.__version__} ndimage.gaussian_filter + numpy {np.__version__}; the numpy restatement of "
                                    "tests/gauss3d_cases.py reproduced every output bit for bit")
    path = os.path.join(HERE, "gauss3d.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(out)} entries; {out['produced_with']}")
    assert os.path.getsize(path) < 128 * 1024


if __name__ == "__main__":
    main()
