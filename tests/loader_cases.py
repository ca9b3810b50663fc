"""Shared by the loader element tests (tests/test_loader_reference.py on the CPU, tests/test_gpu_loader_elements.py on the device,
tests/golden/make_loader_golden.py for Pillow's own outputs): the seeded cases of the three loader entry points
(anoddpm_mri_slice_prepare, anoddpm_resize_bilinear_pil, anoddpm_volume_normalise; csrc/loader.hip) and of `MRIDataset`, with the
expected values -- all of them taken from oracle/loader_oracle.py.  No device and no Pillow here.

Slice preparation.  A case is (geometry, affine set) and always a batch of B = 3 items over two volumes of the same (X, Z):
    item 0: the Y = 2 volume, slice 0        item 1: the Y = 7 volume, slice 6 = Y - 1        item 2: the Y = 7 volume, slice 3
so every launch mixes two Y and touches the first and the last slice.  The nine (X, Z) are one per centre-crop class (`GEOMETRIES`;
the builder asserts the labelled numbers from center_crop_geometry).  The affine sets (`affine_sets`) are RandomAffine's own range
(+-3 degrees with the four sign combinations of the extreme translations, angle 0 with and without a translation, 1e-9 degrees),
coefficients only the C ABI can be handed (45, 90, 180 degrees), the four translations that push every source coordinate out on one
side (the whole output is 0), and one batch whose items differ.  The bar is the bits of center_crop(affine_nearest(take_slice)).

Resizing.  `RESIZE_CASES`, three seeded images each; the bar is the bits of resize_bilinear, then the fp32 (v - 0.5) / 0.5.

`prepare_model` and `resize_model` restate, in numpy, what the kernels and the two signed numbers of dataset.py do (pad_left - crop_left,
crop_top - pad_top); with `defect=None` they must equal the oracle on every case, and each named defect must fail the comparison the
device test uses (`same_bits`) on at least one case (tests/test_loader_reference.py).

Volume normalisation.  expected64 = clip(x, lo, hi) / (hi - lo) in fp64, lo = mean - std, hi = mean + 2 std, mean and std formed
with math.fsum in two passes (exactly rounded sums, no summation order).  The kernel sums in another order (`norm_stats_kernel` restates
it: 256 blocks of 256 threads, grid-stride loop, tree fold in shared memory, serial fold over the blocks, two passes), so its lo, hi
and hi - lo differ from the fsum ones.  Measured on the CPU over all `NORM_CASES` (tests/test_loader_reference.py prints them):
    largest relative difference of lo 6.85e-16 (brain-n1048581), of hi 1.82e-16, of hi - lo 1.81e-16
    (on the offset family hi and lo are each rounded at magnitude 1e4, a relative 3e-13 of their difference 3 -- but the
    reference forms hi - lo from the same rounded numbers, and the two orders agreed on them to the last bit in 4 of 5 sizes)
R is fixed at 16x the largest, rounded up to one digit:        R = 2e-14
and the device bar is, per element,   |got - expected64| <= 0.5 ulp32(expected64) + R |expected64|,   with the bits of
float32(expected64) wherever every value within 2 R |expected64| of expected64 rounds to the same fp32 (`norm_failures`).
A volume of zeros (and the single voxel 0.0) has range 0 and the reference yields NaN from 0 / 0: all NaN is what is stated of
those, nothing more.  (A constant c != 0 gives c / 0 = inf in the reference; the cases do not go there.)"""
import functools
import hashlib
import math

import numpy as np

from oracle import loader_oracle as lo

CROP = 235

# ---------------------------------------------------------------------------------------------------------------- images
def seeded_values(seed, shape):
    """fp32 values with exact (positive) zeros, negatives and a few large magnitudes: no two neighbours coincide by accident."""
    rng = np.random.RandomState(seed)
    v = rng.standard_normal(shape)
    v[v == 0.0] = 1.0
    u = rng.rand(*shape)
    v = np.where(u < 0.05, 0.0, v)
    v = np.where(u > 0.99, v * 1e6, v)
    return v.astype(np.float32)


def same_bits(got, want):
    """The comparison of the device tests: same shape, fp32, and the same bits."""
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape and \
        np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def checksum(a):
    """64 bits of the SHA-256 of the array's bytes."""
    return np.uint64(int.from_bytes(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()[:8], "little"))


# ---------------------------------------------------------------------------------------------------- slice preparation
GEOMETRIES = [
    # (X, Z), (pad_left, pad_top, crop_top, crop_left), class
    ((256, 192), (21, 0, 10, 0), "reference"),
    ((200, 300), (0, 17, 0, 32), "padtop-cropleft"),
    ((235, 235), (0, 0, 0, 0), "identity"),
    ((236, 234), (0, 0, 0, 0), "half-to-0"),
    ((238, 237), (0, 0, 2, 1), "half-to-2"),
    ((100, 120), (57, 67, 0, 0), "pad-both"),
    ((300, 210), (12, 0, 32, 0), "padleft-croptop-large"),
    ((40, 30), (102, 97, 0, 0), "island"),
    ((470, 471), (0, 0, 118, 118), "crop-both"),
]
GEOMETRY_NAMES = [g[2] for g in GEOMETRIES]
YDIMS = (2, 7)
ITEMS = ((0, 0), (1, 6), (1, 3))                                # (volume, slice) of the three items of every batch
AFFINE_NAMES = ["none", "rot+3_t++", "rot-3_t--", "rot+3_t-+", "rot-3_t+-", "identity", "translate", "tiny", "rot45", "rot90", "rot180",
                "out-left", "out-right", "out-top", "out-bottom", "mixed"]
ALL_ZERO = ("out-left", "out-right", "out-top", "out-bottom")
PREPARE_CASES = [(g, a) for g in GEOMETRY_NAMES for a in AFFINE_NAMES]


def geometry(gname):
    (X, Z), geom, _ = GEOMETRIES[GEOMETRY_NAMES.index(gname)]
    assert lo.center_crop_geometry(X, Z, CROP) == geom, (gname, lo.center_crop_geometry(X, Z, CROP), geom)
    return X, Z, geom


def fold_geometry(geom):
    """The two signed numbers the kernel takes: out[oy][ox] = img[oy + crop_top][ox - pad_left]."""
    pl, pt, ct, cl = geom
    return pl - cl, ct - pt


@functools.lru_cache(maxsize=None)
def geometry_volumes(gname):
    X, Z, _ = geometry(gname)
    gi = GEOMETRY_NAMES.index(gname)
    return tuple(seeded_values(1000 + 10 * gi + k, (X, Y, Z)) for k, Y in enumerate(YDIMS))


def affine_sets(X, Z):
    """name -> the (angle, (tx, ty)) of the three items (None: no affine at all).  The image is X rows by Z columns."""
    tx, ty = int(round(0.02 * Z)), int(round(0.09 * X))
    assert tx >= 1 and ty >= 1
    one = {"rot+3_t++": (3.0, (tx, ty)), "rot-3_t--": (-3.0, (-tx, -ty)), "rot+3_t-+": (3.0, (-tx, ty)), "rot-3_t+-": (-3.0, (tx, -ty)),
           "identity": (0.0, (0, 0)), "translate": (0.0, (tx, -ty)), "tiny": (1e-9, (tx, ty)),
           "rot45": (45.0, (0, 0)), "rot90": (90.0, (0, 0)), "rot180": (180.0, (0, 0)),
           "out-left": (0.0, (Z + 3, 0)), "out-right": (0.0, (-(Z + 3), 0)), "out-top": (0.0, (0, X + 3)), "out-bottom": (0.0, (0, -(X + 3)))}
    sets = {k: [v] * len(ITEMS) for k, v in one.items()}
    sets["none"] = None
    sets["mixed"] = [one["rot+3_t++"], one["translate"], one["rot90"]]
    assert sorted(sets) == sorted(AFFINE_NAMES)
    return sets


@functools.lru_cache(maxsize=None)
def prepare_case(gname, aname):
    X, Z, geom = geometry(gname)
    params = affine_sets(X, Z)[aname]
    matrices = None if params is None else [lo.inverse_affine_matrix((Z * 0.5, X * 0.5), ang, tr) for ang, tr in params]
    coeffs = None if matrices is None else np.array([lo.affine_fixed_coeffs(m) for m in matrices], dtype=np.int64)
    return dict(name=f"{gname}/{aname}", gname=gname, aname=aname, X=X, Z=Z, geom=geom, vols=geometry_volumes(gname), items=ITEMS,
                ydim=np.array([YDIMS[v] for v, _ in ITEMS], np.int32), slice_idx=np.array([s for _, s in ITEMS], np.int32),
                params=params, matrices=matrices, coeffs=coeffs)


def prepare_stages(case, b):
    """(the slice, after the affine, after the centre crop) of item b by the oracle."""
    v, s = case["items"][b]
    img = lo.take_slice(case["vols"][v], s)
    aff = img if case["matrices"] is None else lo.affine_nearest(img, case["matrices"][b])
    return img, aff, lo.center_crop(aff, CROP)


@functools.lru_cache(maxsize=None)
def prepare_expected(gname, aname):
    case = prepare_case(gname, aname)
    out = np.stack([prepare_stages(case, b)[2] for b in range(len(case["items"]))])
    out.setflags(write=False)
    return out


PREPARE_DEFECTS = ("flip_pad_left", "flip_crop_top", "flip_both", "one_ydim", "truncate")


def prepare_model(case, defect=None):
    """slice_prepare_kernel in numpy, launched the way dataset.py launches it.  Defects: the sign of pad_left / crop_top flipped,
    the first item's Y for the whole batch, the 16.16 shift replaced by truncation toward zero."""
    assert defect is None or defect in PREPARE_DEFECTS
    H, W = case["X"], case["Z"]
    pad_left, crop_top = fold_geometry(case["geom"])
    if defect in ("flip_pad_left", "flip_both"):
        pad_left = -pad_left
    if defect in ("flip_crop_top", "flip_both"):
        crop_top = -crop_top
    oy, ox = np.mgrid[0:CROP, 0:CROP].astype(np.int64)
    y0, x0 = oy + crop_top, ox - pad_left
    inside = (y0 >= 0) & (y0 < H) & (x0 >= 0) & (x0 < W)
    shift = (lambda v: np.where(v < 0, -((-v) >> 16), v >> 16)) if defect == "truncate" else (lambda v: v >> 16)
    out = np.zeros((len(case["items"]), CROP, CROP), np.float32)
    for b, (v, s) in enumerate(case["items"]):
        flat = case["vols"][v].reshape(-1)
        Y = int(case["ydim"][0 if defect == "one_ydim" else b])
        y, x, ok = y0, x0, inside
        if case["coeffs"] is not None:
            m = [int(c) for c in case["coeffs"][b]]
            y, x = shift(m[5] + m[3] * x0 + m[4] * y0), shift(m[2] + m[0] * x0 + m[1] * y0)
            ok = inside & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        idx = np.where(ok, (y * Y + s) * W + x, 0) % flat.size      # (a wrong Y may point past the volume: wrapped, it is a model)
        out[b] = np.where(ok, flat[idx], np.float32(0))
    return out


# ------------------------------------------------------------------------------------------------------------- resizing
RESIZE_CASES = [((235, 235), o) for o in ((1, 1), (1, 64), (64, 1), (33, 48), (234, 234), (235, 235), (236, 236), (300, 257), (512, 96))] + \
    [((7, 9), (5, 5)), ((30, 40), (64, 48)), ((1, 1), (4, 4))]
RESIZE_B = 3


def resize_name(c):
    return f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}"


RESIZE_NAMES = [resize_name(c) for c in RESIZE_CASES]


def resize_case(name):
    return RESIZE_CASES[RESIZE_NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def resize_images(name):
    (ih, iw), _ = resize_case(name)
    a = seeded_values(2000 + RESIZE_NAMES.index(name), (RESIZE_B, ih, iw))
    a.setflags(write=False)
    return a


def post_normalise(v):
    """torchvision Normalize(0.5, 0.5) on fp32."""
    assert v.dtype == np.float32
    return (v - np.float32(0.5)) / np.float32(0.5)


@functools.lru_cache(maxsize=None)
def resize_expected(name, normalize):
    _, (oh, ow) = resize_case(name)
    out = np.stack([lo.resize_bilinear(img, oh, ow) for img in resize_images(name)])
    out = post_normalise(out) if normalize else out
    out.setflags(write=False)
    return out


def resize_tables(name, coeffs=lo.resize_coeffs):
    """(kx, kx_min, kx_n, ky, ky_min, ky_n) of a case, from the oracle's precompute_coeffs or another one."""
    (ih, iw), (oh, ow) = resize_case(name)
    return coeffs(iw, ow) + coeffs(ih, oh)


RESIZE_DEFECTS = ("vertical_first", "fp32_accumulator")


def _pass(img, k, kmin, kn, axis, acc_t):
    """One pass of resample_pass_kernel along `axis`: ascending taps, one product and one sum per tap, fp32 store."""
    src = np.moveaxis(img, axis, 0)
    out = np.zeros((k.shape[0],) + src.shape[1:], np.float32)
    for o in range(k.shape[0]):
        acc = np.zeros(src.shape[1:], acc_t)
        for t in range(int(kn[o])):
            acc = acc + src[int(kmin[o]) + t].astype(acc_t) * acc_t(k[o, t])
        out[o] = acc.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def resize_model(img, tables, defect=None):
    """The two launches of anoddpm_resize_bilinear_pil in numpy.  Defects: the vertical pass first, an fp32 accumulator."""
    assert defect is None or defect in RESIZE_DEFECTS
    kx, xmin, xn, ky, ymin, yn = tables
    acc_t = np.float32 if defect == "fp32_accumulator" else np.float64
    if defect == "vertical_first":
        return _pass(_pass(img, ky, ymin, yn, 0, acc_t), kx, xmin, xn, 1, acc_t)
    return _pass(_pass(img, kx, xmin, xn, 1, acc_t), ky, ymin, yn, 0, acc_t)


# -------------------------------------------------------------------------------------------------------- normalisation
R = 2e-14                                                       # 16 x 6.85e-16 (brain-n1048581, lo), rounded up to one digit
NORM_THREADS, NORM_BLOCKS = 256, 256
NORM_SIZES = (255, 256, 257, 65536 + 3, 4096 * 256 + 5)
NORM_FAMILIES = ("brain", "offset", "two")
NORM_CASES = [f"{f}-n{n}" for f in NORM_FAMILIES for n in NORM_SIZES]
NORM_NAN_CASES = ["zero-n1", "zero-n257"]
_BRAIN_SHAPE = (104, 100, 101)


@functools.lru_cache(maxsize=1)
def _brain():
    v = lo.synthetic_volume(seed=47, shape=_BRAIN_SHAPE).reshape(-1)
    assert v.size >= max(NORM_SIZES)
    return v


@functools.lru_cache(maxsize=None)
def norm_volume(name):
    fam, n = name.split("-n")
    n = int(n)
    rng = np.random.RandomState(3000 + n % 1000)
    if fam == "brain":                                          # a run of voxels through the middle of the blob
        v = _brain()
        x = v[(v.size - n) // 2:(v.size - n) // 2 + n].copy()
    elif fam == "offset":                                       # the mean is 1e4 standard deviations from 0
        x = 1e4 + rng.standard_normal(n)
    elif fam == "two":                                          # two distinct values; the rarer one lies above hi and is clipped
        x = np.where(rng.rand(n) < 0.05, 1000.0, 0.0)
        x[0], x[-1] = 1000.0, 0.0
    else:
        assert fam == "zero"
        x = np.zeros(n)
    assert x.dtype == np.float64 and x.shape == (n,)
    x.setflags(write=False)
    return x


def norm_stats_fsum(x):
    """(lo, hi) with exactly rounded sums, two passes."""
    n = x.size
    mean = math.fsum(x.tolist()) / n
    d = x - mean
    std = math.sqrt(math.fsum((d * d).tolist()) / n)
    return mean - 1 * std, mean + 2 * std


def _kernel_fold(d):
    """vol_partial_kernel + vol_stat_kernel: the sums of d and d^2 in the kernels' order."""
    stride = NORM_THREADS * NORM_BLOCKS
    trips = -(-d.size // stride)
    pad = np.zeros(trips * stride)
    pad[:d.size] = d                                            # a thread past the end adds nothing
    tot = []
    for term in (pad, pad * pad):
        acc = np.zeros(stride)
        for k in range(trips):                                  # the grid-stride loop: thread (block, lane) walks i = block 256 + lane + k 65536
            acc = acc + term[k * stride:(k + 1) * stride]
        acc = acc.reshape(NORM_BLOCKS, NORM_THREADS).copy()
        o = NORM_THREADS // 2
        while o > 0:                                            # the tree fold in shared memory
            acc[:, :o] = acc[:, :o] + acc[:, o:2 * o]
            o //= 2
        s = 0.0
        for p in acc[:, 0].tolist():                            # the serial fold over the blocks
            s += p
        tot.append(s)
    return tot


def norm_stats_kernel(x):
    """(lo, hi) in the summation order of csrc/loader.hip."""
    n = x.size
    mean = _kernel_fold(x)[0] / n
    sd = math.sqrt(_kernel_fold(x - mean)[1] / n)
    return mean - 1 * sd, mean + 2 * sd


@functools.lru_cache(maxsize=None)
def norm_expected(name):
    x = norm_volume(name)
    lo_, hi_ = norm_stats_fsum(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.clip(x, lo_, hi_) / (hi_ - lo_)
    e.setflags(write=False)
    return e


def norm_failures(tag, got, e, r=None):
    """Lines for the elements that miss the bar; also returns (worst err / bound, elements held to the bits)."""
    r = R if r is None else r
    assert got.dtype == np.float32 and got.shape == e.shape and np.isfinite(e).all()
    ulp = np.spacing(np.abs(e).astype(np.float32)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - e)
    bound = 0.5 * ulp + r * np.abs(e)
    ratio = np.where(np.isfinite(got), err / bound, np.inf)
    lines = [f"{tag}: [{i}] got {got[i]:.9g} want {e[i]:.17g} err / bound {ratio[i]:.3f}" for i in np.nonzero(ratio > 1.0)[0][:8]]
    f = e.astype(np.float32)
    firm = ((e * (1 - 2 * r)).astype(np.float32) == f) & ((e * (1 + 2 * r)).astype(np.float32) == f)   # no fp32 midpoint within 2 R |e|
    off = firm & (got.view(np.uint32) != f.view(np.uint32))
    lines += [f"{tag}: [{i}] got {got[i]:.9g}, not float32({e[i]:.17g}) = {f[i]:.9g}, away from a rounding midpoint" for i in np.nonzero(off)[0][:8]]
    if ratio.max() > 1.0 or off.any():
        lines.append(f"{tag}: {int((ratio > 1.0).sum())} elements over the bound, {int(off.sum())} wrong bits, of {e.size}")
    return lines, float(ratio.max()), int(firm.sum())


# -------------------------------------------------------------------------------------------------------------- dataset
DATASET_SHAPES = ((40, 30), (100, 120))
DATASET_Y = 101
DATASET_Y2 = 130
IMG_SIZES = ((32, 48), (1, 1), (64, 64), (300, 257))


@functools.lru_cache(maxsize=None)
def dataset_volume(X, Y, Z, seed=0):
    v = seeded_values(4000 + seed + X + 7 * Z + 13 * Y, (X, Y, Z))
    v.setflags(write=False)
    return v


def dataset_draws(X, Z):
    """What RandomAffine's three uniform draws are made to return: +-3 degrees and 0 with the translations at the ends of their ranges."""
    dx, dy = float(0.02 * Z), float(0.09 * X)
    return [(3.0, dx, dy), (-3.0, -dx, -dy), (0.0, dx, -dy), (3.0, -dx, dy), (0.0, 0.0, 0.0)]


_DATASET_EXPECTED = {}


def dataset_expected(vol_key, slice_idx, img_size, affine=None):
    """default_transform of one slice; affine = (angle, (tx, ty)) with the translation already rounded to integers, or None."""
    key = (vol_key, int(slice_idx), tuple(img_size), affine)
    if key not in _DATASET_EXPECTED:
        out = lo.default_transform(lo.take_slice(dataset_volume(*vol_key), int(slice_idx)), img_size, affine=affine)
        assert out.dtype == np.float32 and out.shape == (1,) + tuple(img_size)
        _DATASET_EXPECTED[key] = out
    return _DATASET_EXPECTED[key]
