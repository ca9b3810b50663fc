"""Shared by the SSIM tests and their fixture generator (tests/golden/make_ssim_golden.py): the seeded input recipes of the
cases and two numpy pieces,
  (a) `ssim_expected`: the definition (include/anoddpm_hip.h, csrc/ssim.hip) in fp64 with scipy.ndimage.uniform_filter /
      gaussian_filter(sigma=1.5, truncate=3.5) -- the very filters skimage.metrics.structural_similarity calls.  The fixture
      tests/golden/ssim_kat.npz holds its results;
  (b) `ssim_kernel_numpy`: what csrc/ssim.hip computes, in its own arrangement: reflect-indexed halo, separable passes with a
      weight table accumulated from tap 0 upwards, 16 x 32 tiles whose interior values are summed per thread and by a halving
      tree, partials folded 256 at a time.
No skimage and no device needed here.  Inputs are built from elementwise IEEE arithmetic on seeded PCG64 draws only (no libm
calls), so that their SHA-256 is the same on every platform.

Tolerance, derived rather than measured: (a), (b) and the kernel are fp64 on identical fp32 inputs and differ only in summation
order.  The worst term is the cancellation uxx - ux*ux: absolute error about win^2 * 2^-53 * max|x|^2 = 3e-14 for |x| <= 1,
against C2 = 3.6e-3 in the denominator, i.e. about 1e-11 on an element of the map and far less on the mean.  Asserted:
|mssim - expected| <= 1e-10; the fp32 map within 2^-24 + 1e-10 (one rounding of a value in [-1, 1]); real == recon exactly 1.0."""
import hashlib

import numpy as np

MSSIM_TOL = 1e-10
MAP_TOL = 2.0 ** -24 + 1e-10
DATA_RANGE, K1, K2 = 2.0, 0.01, 0.03
TH, TW, THREADS = 16, 32, 256                       # the kernel's tile and workgroup
WINDOWS = (3, 7, 11, 15, "gauss")
BATCH = 55
NAN_SEGMENT = 1

# name -> windows; every window that fits for the odd sizes
SINGLE = {
    "mri256": WINDOWS,
    "noise256": (7, "gauss"),
    "const256": (7, "gauss"),
    "equal256": (7, "gauss"),
    "rgb64": (7, "gauss"),
    "s25x41": WINDOWS,
    "s7x7": (3, 7),
    "s8x300": (3, 7),
    "big512": (3, 7, "gauss"),
}
# cases whose similarity map is spot-checked: four 8 x 8 corners, the top edge strip, one interior block (see `crops`)
MAP_CASES = (("mri256", 7), ("mri256", "gauss"), ("noise256", 7), ("s25x41", 15), ("rgb64", 7), ("s8x300", 3))


def win_of(window):
    return 11 if window == "gauss" else int(window)


def _mri_like(rng, side):
    """Constant -1 background outside an ellipse (so vx is exactly 0 over large areas), blocky texture plus fine noise inside."""
    i, j = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="ij")
    c = (side - 1) / 2.0
    inside = ((i - c) / (0.42 * side)) ** 2 + ((j - c) / (0.33 * side)) ** 2 <= 1.0
    coarse = np.repeat(np.repeat(rng.random((side // 16, side // 16), dtype=np.float32), 16, axis=0), 16, axis=1)
    fine = rng.random((side, side), dtype=np.float32)
    body = (np.float32(1.2) * coarse + np.float32(0.5) * fine - np.float32(0.9)).astype(np.float32)
    return np.where(inside, np.clip(body, -1, 1), np.float32(-1)).astype(np.float32)[None]


def _noisy_copy(rng, real, amp):
    noise = (rng.random(real.shape, dtype=np.float32) - np.float32(0.5)) * np.float32(amp)
    return np.clip(real + noise, np.float32(-1), np.float32(1)).astype(np.float32)


def _uniform(rng, shape):
    return (rng.random(shape, dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)


def make_case(name):
    """(real, recon) of a single-segment case, fp32 [C][H][W]."""
    rng = np.random.default_rng(7000 + sorted(SINGLE).index(name))
    if name == "mri256":
        real = _mri_like(rng, 256)
        return real, _noisy_copy(rng, real, 0.4)
    if name == "noise256":
        return _uniform(rng, (1, 256, 256)), _uniform(rng, (1, 256, 256))
    if name == "const256":
        return np.full((1, 256, 256), 0.5, np.float32), np.full((1, 256, 256), -0.25, np.float32)
    if name == "equal256":
        real = _mri_like(rng, 256)
        return real, real.copy()
    if name == "rgb64":
        real = _uniform(rng, (3, 64, 64))
        return real, _noisy_copy(rng, real, 0.8)
    if name == "big512":
        real = np.concatenate([_mri_like(rng, 512) for _ in range(3)])
        return real, _noisy_copy(rng, real, 0.3)
    h, w = (int(v) for v in name[1:].split("x"))
    real = _uniform(rng, (1, h, w))
    return real, _noisy_copy(rng, real, 0.6)


def make_batch():
    """One 256^2 image shared by 55 reconstructions of growing noise amplitude: (real [1][256][256], recons [55][1][256][256])."""
    rng = np.random.default_rng(7100)
    real = _mri_like(rng, 256)
    return real, np.stack([_noisy_copy(rng, real, 0.02 * (j + 1)) for j in range(BATCH)])


def make_nan_batch():
    """Three 1 x 64 x 64 pairs; the reconstruction of segment NAN_SEGMENT holds one NaN."""
    rng = np.random.default_rng(7200)
    real = _uniform(rng, (3, 1, 64, 64))
    recon = _noisy_copy(rng, real, 0.5)
    recon[NAN_SEGMENT, 0, 30, 17] = np.nan
    return real, recon


def sha_inputs(real, recon):
    return hashlib.sha256(np.ascontiguousarray(real).tobytes() + np.ascontiguousarray(recon).tobytes()).hexdigest()


def key(name, window):
    return f"{name}_w{window}"


def crops(smap):
    """The spot-checked pieces of a [C][H][W] map: name -> (slices)."""
    _, H, W = smap.shape
    e = min(8, H, W)
    out = {"tl": (slice(None), slice(0, e), slice(0, e)), "tr": (slice(None), slice(0, e), slice(W - e, W)),
           "bl": (slice(None), slice(H - e, H), slice(0, e)), "br": (slice(None), slice(H - e, H), slice(W - e, W)),
           "top": (slice(None), slice(0, e), slice(0, min(W, 96))),
           "mid": (slice(None), slice(H // 2 - min(8, H // 2), H // 2 + min(8, H - H // 2)),
                   slice(W // 2 - min(8, W // 2), W // 2 + min(8, W - W // 2)))}
    return out


# ---------------------------------------------------------------------------------- (a) expected values: scipy's filters
def ssim_expected(real, recon, window, data_range=DATA_RANGE):
    """(mssim, S map [C][H][W] fp64) of one [C][H][W] pair by the definition, with the filters skimage calls."""
    from scipy import ndimage
    x, y = np.asarray(real, np.float64), np.asarray(recon, np.float64)
    win = win_of(window)
    if window == "gauss":
        def filt(v):
            return ndimage.gaussian_filter(v, sigma=1.5, truncate=3.5, mode="reflect")
        cn = 1.0
    else:
        def filt(v):
            return ndimage.uniform_filter(v, size=win, mode="reflect")
        cn = win * win / (win * win - 1.0)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    smap = np.empty_like(x)
    for c in range(x.shape[0]):
        ux, uy = filt(x[c]), filt(y[c])
        uxx, uyy, uxy = filt(x[c] * x[c]), filt(y[c] * y[c]), filt(x[c] * y[c])
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        smap[c] = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    p = (win - 1) // 2
    return float(smap[:, p:smap.shape[1] - p, p:smap.shape[2] - p].mean()), smap


# ---------------------------------------------------------------------------------- (b) the kernel's arrangement
def weights(window):
    """The weight table of anoddpm_ssim (host side of csrc/ssim.hip)."""
    win = win_of(window)
    if window == "gauss":
        w = [float(np.exp(-0.5 / (1.5 * 1.5) * float((k - 5) * (k - 5)))) for k in range(win)]
        total = 0.0
        for v in w:
            total += v
        return np.array([v / total for v in w], np.float64)
    return np.full(win, 1.0 / win, np.float64)


def _reflect_index(lo, hi, n):
    i = np.arange(lo, hi)
    i = np.where(i < 0, -i - 1, i)
    i = np.where(i >= n, 2 * n - 1 - i, i)
    return np.clip(i, 0, n - 1)


def _tree(a):
    """Halving tree over the last axis (length a power of two): a[t] += a[t + off], off = len/2 ... 1."""
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def ssim_kernel_numpy(real, recon, window, data_range=DATA_RANGE):
    """(mssim, S map [C][H][W] fp64) of one [C][H][W] pair, operation for operation as csrc/ssim.hip forms them.  The window
    means of a pixel do not depend on the tile that computes it, so the two passes run over the whole reflect-padded image; the
    partial sums follow the 16 x 32 tiles, the two pixels of a thread, the halving tree and the fold."""
    x, y = np.asarray(real, np.float32), np.asarray(recon, np.float32)
    C, H, W = x.shape
    w = weights(window)
    win = w.size
    p = (win - 1) // 2
    cn = 1.0 if window == "gauss" else win * win / (win * win - 1.0)
    c1, c2 = (K1 * data_range) * (K1 * data_range), (K2 * data_range) * (K2 * data_range)
    ri, ci = _reflect_index(-p, H + p, H), _reflect_index(-p, W + p, W)
    xp, yp = x[:, ri][:, :, ci].astype(np.float64), y[:, ri][:, :, ci].astype(np.float64)

    def passes(v):
        row = w[0] * v[:, :, 0:W]
        for k in range(1, win):
            row = row + w[k] * v[:, :, k:k + W]
        col = w[0] * row[:, 0:H]
        for k in range(1, win):
            col = col + w[k] * row[:, k:k + H]
        return col

    with np.errstate(invalid="ignore"):
        ux, uy, uxx, uyy, uxy = passes(xp), passes(yp), passes(xp * xp), passes(yp * yp), passes(xp * yp)
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        smap = ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        # partial sums: pixels outside the interior (and the tile overhang) count as +0.0
        ty, tx = -(-H // TH), -(-W // TW)
        masked = np.zeros((C, ty * TH, tx * TW), np.float64)
        masked[:, p:H - p, p:W - p] = smap[:, p:H - p, p:W - p]
        tiles = masked.reshape(C, ty, TH, tx, TW).transpose(0, 1, 3, 2, 4).reshape(C * ty * tx, TH * TW)
        acc = np.zeros((tiles.shape[0], THREADS), np.float64)
        for k in range(TH * TW // THREADS):                  # thread t owns pixels t, t + 256 of its tile
            acc = acc + tiles[:, k * THREADS:(k + 1) * THREADS]
        partial = _tree(acc)
        n = partial.size
        padded = np.zeros(-(-n // THREADS) * THREADS, np.float64)
        padded[:n] = partial
        acc = np.zeros(THREADS, np.float64)
        for row in padded.reshape(-1, THREADS):              # thread t folds partials t, t + 256, ...
            acc = acc + row
        total = _tree(acc)
    return float(total / (float(C) * float(H - 2 * p) * float(W - 2 * p))), smap
