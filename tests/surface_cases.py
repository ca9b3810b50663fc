"""Cases and numpy / scipy restatements shared by test_surface_reference.py (CPU), test_gpu_surface.py and
golden/make_surface_golden.py: the exact Euclidean distance transform and the boundary distances of csrc/surface.hip
(include/anoddpm_hip.h has the definitions).

  edt2_brute     the squared distance to the nearest background pixel as an integer minimum over ALL background pixels
  edt_scipy      scipy.ndimage.distance_transform_edt
  surface_ref    scipy erosion -> border, scipy's transform -> integer squared distances, the percentile as the header defines
                 it, math.fsum means.  Its keyword arguments plant the defects test_surface_reference.py must be able to see
  surface_fp64   the same with the mean summed in the kernel's order (thread t adds the pixels t, t + 1024, ...; halving trees)
  edt2_separable column sweeps and a row search in numpy, the kernel's own decomposition, with an optional cap on the search
"""
import hashlib
import math

import numpy as np
from scipy import ndimage

THREADS, WAVES = 1024, 16
CROSS = ndimage.generate_binary_structure(2, 1)
FULL = ndimage.generate_binary_structure(2, 2)
EMPTY_PRED, EMPTY_REF = 1, 2


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------- distance transform
def edt2_brute(fg):
    """[H, W] bool -> int64 squared distance to the nearest False pixel (0 on False); -1 everywhere when there is none."""
    fg = np.asarray(fg, bool)
    H, W = fg.shape
    by, bx = np.nonzero(~fg)
    if by.size == 0:
        return np.full((H, W), -1, np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    yy, xx = yy.reshape(-1, 1).astype(np.int64), xx.reshape(-1, 1).astype(np.int64)
    out = np.empty(H * W, np.int64)
    step = max(1, (1 << 22) // by.size)
    for i in range(0, H * W, step):
        out[i:i + step] = ((yy[i:i + step] - by) ** 2 + (xx[i:i + step] - bx) ** 2).min(axis=1)
    return out.reshape(H, W)


def edt_scipy(fg):
    return ndimage.distance_transform_edt(np.asarray(fg, bool))


def edt2_separable(fg, cap=None):
    """The kernel's decomposition: g = distance to the nearest False of the own column, then min over |x - x'| <= cap of
    (x - x')^2 + g^2.  cap None: the whole row.  int64; -1 where nothing is in reach."""
    fg = np.asarray(fg, bool)
    H, W = fg.shape
    far = np.int64(1) << 40
    g = np.full((H, W), far, np.int64)
    d = np.full(W, far, np.int64)
    for y in range(H):
        d = np.where(fg[y], np.minimum(d + 1, far), 0)
        g[y] = d
    d = np.full(W, far, np.int64)
    for y in range(H - 1, -1, -1):
        d = np.where(fg[y], np.minimum(d + 1, far), 0)
        g[y] = np.minimum(g[y], d)
    g2 = np.where(g >= far, far, g * g)
    best = g2.copy()
    for k in range(1, (W if cap is None else min(cap + 1, W))):
        best[:, k:] = np.minimum(best[:, k:], g2[:, :-k] + k * k)
        best[:, :-k] = np.minimum(best[:, :-k], g2[:, k:] + k * k)
    return np.where(best >= far, -1, best)


def _edt2_scipy_exact(fg):
    """Integer squared distances from scipy's transform: the feature indices it returns, squared in integers."""
    fg = np.asarray(fg, bool)
    if fg.all():
        return np.full(fg.shape, -1, np.int64)
    iy, ix = ndimage.distance_transform_edt(fg, return_distances=False, return_indices=True)
    yy, xx = np.mgrid[0:fg.shape[0], 0:fg.shape[1]]
    return (iy.astype(np.int64) - yy) ** 2 + (ix.astype(np.int64) - xx) ** 2


def transform_cases():
    """name -> (planes [S, H, W] fp32, level)."""
    rng = np.random.default_rng(41)
    c = {}
    c["rand40x33"] = ((rng.random((2, 40, 33)) > 0.3).astype(np.float32), 0.0)                # odd width, two planes
    wide = np.ones((1, 17, 300), np.float32)                                                  # several words / blocks per row
    wide[0, 8, 3] = wide[0, 2, 150] = wide[0, 16, 299] = 0                                    # distances beyond 64 columns
    c["wide17x300"] = (wide, 0.0)
    c["tiny5x7"] = ((rng.random((1, 5, 7)) > 0.4).astype(np.float32), 0.0)
    c["one_bg"] = (np.zeros((1, 1, 1), np.float32), 0.0)
    c["one_fg"] = (np.ones((1, 1, 1), np.float32), 0.0)                                       # no background: -1 / inf
    c["checker12x13"] = (((np.add.outer(np.arange(12), np.arange(13)) & 1) == 0).astype(np.float32)[None], 0.0)
    corner = np.ones((1, 64, 64), np.float32)
    corner[0, 0, 0] = 0                                                                       # largest distance: 2 * 63^2
    c["corner64"] = (corner, 0.0)
    c["all_bg9"] = (np.zeros((1, 9, 9), np.float32), 0.0)
    mid = (rng.random((3, 20, 20)) > 0.2).astype(np.float32)
    mid[1] = 1                                                                                # all foreground between two others
    c["all_fg_mid"] = (mid, 0.0)
    img = rng.random((2, 24, 19)).astype(np.float32)
    img[0, 3, 4] = img[1, 20, 0] = img[1, 7, 7] = np.nan                                      # NaN is background
    c["level_nan"] = (img, 0.35)
    big = np.ones((1, 256, 256), np.float32)
    big.reshape(-1)[rng.choice(256 * 256, 40, replace=False)] = 0
    big[0, 100:140, 60:200] *= (rng.random((40, 140)) > 0.5)
    c["plane256"] = (big, 0.0)
    long = np.ones((2, 2, 4100), np.float32)                                                  # a row too long for the staged path
    long[0, 0, 5] = long[0, 1, 4000] = long[1, 1, 2050] = 0
    c["long2x4100"] = (long, 0.0)
    return c


def foreground(planes, level):
    with np.errstate(invalid="ignore"):
        return planes > np.float32(level)


# ---------------------------------------------------------------------------------- boundary distances
def border(m, structure=CROSS, border_value=0):
    m = np.asarray(m, bool)
    return m & ~ndimage.binary_erosion(m, structure=structure, iterations=1, border_value=border_value)


def percentile95(sq_sorted, mode="lerp"):
    """The header's percentile of the square roots of the ascending int64 squared distances; every operation rounded once."""
    n = sq_sorted.size
    k = 19 * (n - 1)
    lo, r = divmod(k, 20)
    hi = min(lo + 1, n - 1)
    if mode == "nearest":
        return float(np.sqrt(np.float64(sq_sorted[min(lo + (1 if 2 * r >= 20 else 0), n - 1)])))
    a, b = np.sqrt(np.float64(sq_sorted[lo])), np.sqrt(np.float64(sq_sorted[hi]))
    return float(a + (b - a) * (np.float64(r) / np.float64(20.0)))


def directed(pred, ref, structure=CROSS, border_value=0, to_foreground=False, row_cap=None):
    """(bp, br, d2_pr, d2_rp): the two borders [H, W] bool and the int64 squared distances on them in row-major pixel order."""
    bp, br = border(pred, structure, border_value), border(ref, structure, border_value)
    tp, tr = (np.asarray(pred, bool), np.asarray(ref, bool)) if to_foreground else (bp, br)
    if row_cap is None:
        fp, fr = _edt2_scipy_exact(~tp), _edt2_scipy_exact(~tr)
    else:
        fp, fr = edt2_separable(~tp, row_cap), edt2_separable(~tr, row_cap)
        fp, fr = np.where(fp < 0, 2 ** 31 - 1, fp), np.where(fr < 0, 2 ** 31 - 1, fr)             # nothing in reach: far away
    return bp, br, fr[bp], fp[br]


def surface_ref(pred, ref, structure=CROSS, border_value=0, to_foreground=False, row_cap=None, one_direction=False,
                percentile="lerp", pooled="pool"):
    """One pair of [H, W] 0 / 1 planes -> dict(counts, max2, mean, p95, status, hd, hd95, assd).  The defaults are the
    definition; every other value of a keyword is a planted defect."""
    bp, br, d_pr, d_rp = directed(pred, ref, structure, border_value, to_foreground, row_cap)
    counts = np.array([d_pr.size, d_rp.size], np.int32)
    status = (EMPTY_PRED if d_pr.size == 0 else 0) | (EMPTY_REF if d_rp.size == 0 else 0)
    nan = float("nan")
    if status:
        return dict(counts=counts, max2=np.array([-1, -1], np.int32), mean=np.array([nan, nan]), p95=np.array([nan, nan, nan]),
                    status=status, hd=nan, hd95=nan, assd=nan)
    if one_direction:
        d_rp = d_pr
    max2 = np.array([d_pr.max(), d_rp.max()], np.int32)
    mean = np.array([math.fsum(np.sqrt(d.astype(np.float64))) / d.size for d in (d_pr, d_rp)])
    p = [percentile95(np.sort(d), percentile) for d in (d_pr, d_rp)]
    p.append(max(p) if pooled == "max" else percentile95(np.sort(np.r_[d_pr, d_rp]), percentile))
    return dict(counts=counts, max2=max2, mean=mean, p95=np.array(p), status=0, hd=float(np.sqrt(np.float64(max2.max()))),
                hd95=p[2], assd=float((mean[0] + mean[1]) / 2))


def kernel_sum(terms):
    """fp64 sum in the kernel's order: thread t adds terms t, t + 1024, ... in that order; a halving tree folds the 64 partials
    of each wave, then the 16 wave sums.  (Adding +0.0 leaves the bits of a non-negative partial alone.)"""
    rows = -(-terms.size // THREADS)
    padded = np.zeros(rows * THREADS, np.float64)
    padded[:terms.size] = terms
    part = np.zeros(THREADS, np.float64)
    for row in padded.reshape(rows, THREADS):
        part = part + row
    w = part.reshape(WAVES, 64)
    off = 32
    while off:
        w = w[:, :off] + w[:, off:2 * off]
        off >>= 1
    v = w[:, 0]
    off = WAVES // 2
    while off:
        v = v[:off] + v[off:2 * off]
        off >>= 1
    return float(v[0])


def surface_fp64(pred, ref):
    """`surface_ref` with the means summed in the kernel's order over the plane's pixels."""
    r = surface_ref(pred, ref)
    if r["status"]:
        return r
    bp, br, d_pr, d_rp = directed(pred, ref)
    mean = []
    for b, d in ((bp, d_pr), (br, d_rp)):
        terms = np.zeros(b.size, np.float64)
        terms[b.reshape(-1)] = np.sqrt(d.astype(np.float64))
        mean.append(kernel_sum(terms) / np.float64(d.size))
    r["mean"] = np.array(mean)
    r["assd"] = float((mean[0] + mean[1]) / 2)
    return r


def _blobs(rng, shape, sigma, cut):
    return (ndimage.gaussian_filter(rng.random(shape), sigma) > cut).astype(np.float32)


def _blob_pair(seed, shape, sigma=2.0):
    rng = np.random.default_rng(seed)
    ref = _blobs(rng, shape, sigma, 0.5)
    pred = np.roll(ref, (1, 2), (0, 1)) * (rng.random(shape) > 0.03) + (_blobs(rng, shape, sigma, 0.54) > 0)
    return (pred > 0).astype(np.float32), ref


def surface_cases():
    """name -> (pred [S, H, W], ref [S, H, W] or one shared [H, W]), fp32 0 / 1."""
    c = {}
    ident = np.zeros((1, 16, 16), np.float32)
    ident[0, 3:11, 4:13] = 1
    ident[0, 12:14, 2:4] = 1
    c["identical"] = (ident, ident.copy())                                                    # every distance 0
    single = np.zeros((1, 16, 16), np.float32)
    single[0, 13, 2] = 1
    ref = np.zeros((1, 16, 16), np.float32)
    ref[0, 2:9, 6:14] = 1
    c["single_pixel"] = (single, ref)
    c["full_image"] = (np.ones((1, 12, 15), np.float32), ref[:, :12, :15].copy())             # border = the frame
    outer, inner = np.zeros((1, 32, 32), np.float32), np.zeros((1, 32, 32), np.float32)
    outer[0, 4:28, 4:28] = 1
    inner[0, 10:20, 11:21] = 1
    c["nested"] = (inner, outer)                                                              # border to border, not to the foreground
    a, b = np.zeros((1, 64, 64), np.float32), np.zeros((1, 64, 64), np.float32)
    a[0, 0, 0] = b[0, 63, 63] = 1
    c["corners64"] = (a, b)                                                                   # max2 = 2 * 63^2
    p, r = _blob_pair(5, (16, 16), 1.5)
    c["blobs16"] = (p[None], r[None])
    p, r = _blob_pair(6, (40, 33))
    c["blobs40x33"] = (p[None], r[None])
    rng = np.random.default_rng(7)
    p, r = _blobs(rng, (17, 300), 1.5, 0.5), _blobs(rng, (17, 300), 1.5, 0.5)
    p[:, 45:] = 0                                                                             # prediction at the left end,
    r[:, :200] = 0                                                                            # reference at the right: > 64 columns apart
    c["blobs17x300"] = (p[None], r[None])
    rng = np.random.default_rng(8)
    shared = _blobs(rng, (24, 20), 2.0, 0.5)
    six = np.stack([(np.roll(shared, (i - 2, 1 - i), (0, 1)) * (rng.random((24, 20)) > 0.05)).astype(np.float32) for i in range(6)])
    six[2] = 0                                                                                # an empty prediction at position 2
    c["batch6_shared"] = (six, shared)
    c["empty_ref"] = (ident.copy(), np.zeros((1, 16, 16), np.float32))
    p, r = _blob_pair(9, (256, 256), 6.0)
    c["pair256"] = (p[None], r[None])
    return c


SMALL_SURFACE = ("identical", "single_pixel", "full_image", "nested", "corners64", "blobs16", "blobs40x33", "blobs17x300", "batch6_shared",
                 "empty_ref")
LARGE_SURFACE = ("pair256",)
SMALL_TRANSFORM = ("rand40x33", "wide17x300", "tiny5x7", "one_bg", "one_fg", "checker12x13", "corner64", "all_bg9", "all_fg_mid", "level_nan")
LARGE_TRANSFORM = ("plane256", "long2x4100")


def pairs_of(pred, ref):
    """The (pred plane, ref plane) pairs of a case."""
    return [(pred[s], ref if ref.ndim == 2 else ref[s]) for s in range(pred.shape[0])]


def summary(results):
    """Everything a list of `surface_ref` results states, as bytes: two lists are equal iff every number is."""
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for r in results for k in ("counts", "max2", "mean", "p95")) + \
        bytes(r["status"] for r in results) + np.array([r["hd"] for r in results] + [r["hd95"] for r in results]).tobytes()


def ulps(a, b):
    """|a - b| in units of the spacing of fp64 at b."""
    return abs(a - b) / np.spacing(np.float64(abs(b))) if a != b else 0.0
