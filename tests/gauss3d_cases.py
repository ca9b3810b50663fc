"""Shared by the volume-smoothing tests and their fixture generator (tests/golden/make_gauss3d_golden.py): the case table, the
seeded inputs and a plain-numpy restatement of csrc/gauss3d.hip,
  `gaussian3d_numpy`   scipy.ndimage.gaussian_filter(vol, (sz, sy, sx), truncate=t) on fp32 volumes, bit for bit: the axes in the
                       order D, H, W; per line smooth_cases' statement (fp64 taps from the edge inwards, every product and sum
                       rounded once); fp32 after EACH axis; the periodic reflect border; an axis of radius 0 skipped.
The fixture tests/golden/gauss3d.npz holds what scipy itself returns.  Outputs are compared bit for bit: no tolerance anywhere.
Neither scipy nor a device is needed here."""
import numpy as np

import smooth_cases as sm
from smooth_cases import sha  # noqa: F401  (the tests take it from here)

MAX_RADIUS = 32
TILE = 32                                                    # csrc/gauss3d.hip's tile, on (D, H*W) in the z launch and on (H, W) in the plane launch
TRUNCATE = 4.0
FULL_LIMIT = 4096                                            # expected outputs up to this many voxels are stored in full

# name -> (shape, sigma): the table of the issue; the last three dimensions are the volume
CASES = {
    "one_slice": ((1, 5, 7), 1.0),                           # the z pass reads one voxel 2r + 1 times; it must still run and round
    "d_below_rz": ((3, 33, 65), 4.0),                        # D < rz: several reflections; a second tile in y, a third in x
    "rz32_tiny_plane": ((33, 3, 5), (8.0, 0.4, 8.0)),        # radius 32 in z across two z tiles; radii 32, 2, 32
    "anisotropic": ((9, 34, 31), (1.0, 4.0, 4.0)),           # ragged tiles
    "z_skipped": ((4, 40, 70), (0.0, 2.0, 2.0)),             # one launch; gaussian_filter(vol, 2.0) slice by slice
    "z_only": ((70, 3, 5), (2.0, 0.0, 0.0)),                 # one launch, three z tiles
    "x_skipped": ((5, 6, 40), (0.5, 3.0, 0.0)),              # x skipped inside the plane launch
    "batched": ((2, 2, 2, 16, 16), 1.5),                     # leading batch dimensions
}
DEFECTS = ("x_first", "noround_z", "single_mirror_z", "sigma0_on_x", "no_z", "fp32acc")
STRIDED = (3, 6, 10, 12, 8)                                  # volumes, D, H, W, padding words behind each volume
BATCH5 = ((5, 4, 9, 33), (1.0, 2.0, 2.0))
POISON = ((4, 6, 20, 24), (1.0, 2.0, 2.0), 2, (3, 11, 17))   # shape, sigma, the volume with the NaN, where in it


def sigmas_of(sigma):
    return (float(sigma),) * 3 if isinstance(sigma, (int, float)) else tuple(float(s) for s in sigma)


def radius_of(sigma, truncate=TRUNCATE):
    """0: the axis is skipped (scipy skips sigma <= 1e-15 and applies the one-tap kernel [1.0] for any other radius 0)."""
    return 0 if sigma <= 1e-15 else int(truncate * float(sigma) + 0.5)


def tables_used():
    """Every (sigma, truncate) of the case table whose axis is filtered."""
    return sorted({(s, TRUNCATE) for _, sigma in CASES.values() for s in sigmas_of(sigma) if radius_of(s) > 0})


def _squared_normals(seed, shape):
    """Squared standard normals as fp32: finite and non-negative, like squared errors."""
    z = np.random.default_rng(seed).standard_normal(shape, dtype=np.float32)
    return (z * z).astype(np.float32)


def make_case(name):
    return _squared_normals(9300 + sorted(CASES).index(name), CASES[name][0])


def make_strided():
    """(buffer [V][D*H*W + pad], volumes [V][D][H][W]): the volumes are a view into the buffer's rows, src_stride > D*H*W."""
    V, D, H, W, pad = STRIDED
    buf = _squared_normals(9390, (V, D * H * W + pad))
    return buf, buf[:, :D * H * W].reshape(V, D, H, W)


def make_batch5():
    return _squared_normals(9391, BATCH5[0])


def make_poison():
    shape, _, v, where = POISON
    x = _squared_normals(9392, shape)
    x[(v,) + where] = np.nan
    return x


def gaussian3d_numpy(x, sigmas, truncate=TRUNCATE, defect=None):
    """`scipy.ndimage.gaussian_filter(vol, sigmas, truncate=truncate)` of every [D][H][W] volume of the fp32 array x
    ([..., D, H, W]).  `defect` plants one of DEFECTS (the tests show that each changes some case's bits)."""
    v = np.asarray(x, np.float32)
    sig = sigmas_of(sigmas)
    if defect == "sigma0_on_x":
        sig = sig[::-1]
    order = [(-3, sig[0]), (-2, sig[1]), (-1, sig[2])]
    if defect == "x_first":
        order = order[::-1]
    if defect == "no_z":
        order = order[1:]
    for axis, s in order:
        r = radius_of(s, truncate)
        if r == 0:
            continue
        line_defect = "single" if defect == "single_mirror_z" and axis == -3 else ("fp32acc" if defect == "fp32acc" else None)
        acc = np.moveaxis(sm._lines(np.moveaxis(v, axis, -1), sm.weights_numpy(s, truncate), r, line_defect), -1, axis)
        v = acc if defect == "noround_z" and axis == -3 else acc.astype(np.float32)
    return np.ascontiguousarray(v.astype(np.float32))


def check_fixture(kat, key, got):
    """`got` against the fixture: its SHA-256 always, the stored array (outputs of up to FULL_LIMIT voxels) for a readable failure."""
    assert got.dtype == np.float32
    if key + "_out" in kat.files:
        want = kat[key + "_out"]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{key}: {int((got != want).sum())} elements differ"
    assert sha(got) == str(kat[key + "_out_sha"]), key
