"""Shared by the smoothing tests and their fixture generator (tests/golden/make_smooth_golden.py): the seeded input recipes of
the cases and plain-numpy restatements of the two kernels of csrc/smooth.hip,
  `weights_numpy`    the 2 r + 1 normalised fp64 taps                          (scipy.ndimage._filters._gaussian_kernel1d)
  `gaussian_numpy`   axis 0 then axis 1, fp64 taps from the edge inwards, fp32 between the axes, periodic reflect border
                                                                               (scipy.ndimage.gaussian_filter, bit for bit)
  `scores_numpy`     max, mean and top-k mean of one image in the kernel's summation order (anoddpm_map_scores, bit for bit)
The fixture tests/golden/smooth_kat.npz holds what scipy itself returns.  Filter outputs are compared bit for bit: no tolerance.
Neither scipy nor a device is needed here.  Inputs are built from elementwise IEEE arithmetic on seeded PCG64 draws only (no
libm calls), so that their SHA-256 is the same on every platform."""
import hashlib

import numpy as np

from postproc_cases import crops

MAX_RADIUS = 32
TILE = 32                                                    # csrc/smooth.hip's tile: g32x32 is one tile, g33x33 one more in each direction
MAX_N = 1 << 24                                              # ANODDPM_MAP_SCORES_MAX_N
THREADS, WAVE = 1024, 64                                     # the summation order of anoddpm_map_scores

# (sigma, truncate) -> radius, the table of the issue
WEIGHTS = {(0.5, 4.0): 2, (1.0, 4.0): 4, (2.5, 4.0): 10, (3.0, 3.0): 9, (4.0, 4.0): 16, (8.0, 4.0): 32}

# name -> (shape, sigma, truncate, kind)
GAUSS = {
    "g5x7": ((5, 7), 4.0, 4.0, "random"),
    "g3x3": ((3, 3), 4.0, 4.0, "random"),
    "g1x40": ((1, 40), 4.0, 4.0, "random"),
    "g40x1": ((40, 1), 4.0, 4.0, "random"),
    "g2x2_s8": ((2, 2), 8.0, 4.0, "random"),
    "g37x53": ((37, 53), 4.0, 4.0, "random"),
    "g32x32": ((32, 32), 4.0, 4.0, "random"),
    "g33x33": ((33, 33), 4.0, 4.0, "blobs"),
    "g9x70_s8": ((9, 70), 8.0, 4.0, "random"),
    "g70x9_s8": ((70, 9), 8.0, 4.0, "random"),
    "g17x33_s05": ((17, 33), 0.5, 4.0, "random"),
    "g20x20_s3t3": ((20, 20), 3.0, 3.0, "random"),
    "g33x20_s25": ((33, 20), 2.5, 4.0, "blobs"),
    "g64x64_const": ((64, 64), 4.0, 4.0, "constant"),
    "g256": ((256, 256), 4.0, 4.0, "blobs"),
    "g1x9_order_s1": ((1, 9), 1.0, 4.0, "order"),
}
# A line built so that its centre output lies next to the midpoint of two fp32 values: the taps summed from the edge inwards
# (scipy) and from the centre outwards round to different sides of it.  fp64 orders differ by an ulp of fp64, which random
# inputs carry into the fp32 result about once in 2^29 pixels.
ORDER_LINE = (0x3f49446c, 0x3f3db906, 0x3fcdf276, 0x3fe4bd87, 0x4001b992, 0x3f2c60a0, 0x3fff25a3, 0x3ff4ce6d, 0x35fd6428)
FULL_LIMIT = 64 * 64                                         # expected outputs up to this many pixels are stored in full
BATCH_SHAPE = (55, 1, 32, 32)
POISON_SHAPE, POISON_PLANE = (8, 24, 40), 3
DEFECTS = ("mirror", "fp32acc", "noround", "axes", "single", "centre_out")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _errors(rng, shape):
    """Values like squared errors: `random ** 4 * 3` (many small, a few large), by two multiplications."""
    u = rng.random(shape, dtype=np.float32)
    s = u * u
    return ((s * s) * np.float32(3)).astype(np.float32)


def make_gauss_case(name):
    shape, _, _, kind = GAUSS[name]
    rng = np.random.default_rng(9500 + sorted(GAUSS).index(name))
    if kind == "constant":
        return np.full(shape, 0.7, np.float32)
    if kind == "order":
        return np.array(ORDER_LINE, np.uint32).view(np.float32).reshape(shape)
    x = _errors(rng, shape)
    if kind == "blobs":                                      # structure: a bright block at a corner and one inside, over the noise
        h, w = shape
        x[:max(1, h // 8), :max(1, w // 6)] += np.float32(2.5)
        x[h // 2:h // 2 + max(1, h // 5), w // 3:w // 3 + max(1, w // 4)] += np.float32(1.25)
    return x


def make_batch():
    return _errors(np.random.default_rng(9600), BATCH_SHAPE)


def make_strided():
    """(buffer [4][16 * 24 + 8], planes [4][16][24]): the planes are a view into the buffer's rows -- row stride 392, not 384
    (the layout of postproc_cases.make_strided)."""
    rng = np.random.default_rng(9650)
    S, h, w, pad = 4, 16, 24, 8
    buf = rng.random((S, h * w + pad), dtype=np.float32)
    for j in range(S):
        buf[j, :h * w] = _errors(rng, (h, w)).reshape(-1)
    return buf, buf[:, :h * w].reshape(S, h, w)


def make_poison():
    """[8][24][40] with one NaN in plane 3."""
    x = _errors(np.random.default_rng(9700), POISON_SHAPE)
    x[POISON_PLANE, 11, 17] = np.nan
    return x


# ---------------------------------------------------------------------------------- image-score cases
# name -> (shape, k): one image per case, all its values pooled
SCORES = {
    "n1": ((1, 1), 1),
    "k1": ((9, 11), 1),
    "kn": ((9, 11), 99),
    "constant": ((16, 16), 5),
    "tie_at_k": ((8, 8), 4),
    "zeros": ((12, 12), 7),
    "negzero_denormal": ((8, 16), 9),
    "s37x53": ((37, 53), 19),
    "pooled3x64x64": ((3, 64, 64), 122),
    "s256": ((256, 256), 655),
}


def make_score_case(name):
    shape, k = SCORES[name]
    rng = np.random.default_rng(9800 + sorted(SCORES).index(name))
    if name == "constant":
        return np.full(shape, 0.3, np.float32), k
    if name == "zeros":
        return np.zeros(shape, np.float32), k
    x = _errors(rng, shape)
    if name == "tie_at_k":                                   # exactly two values above the k-th and (k+1)-th, which are equal: 3rd ... 6th tie
        x = (x * np.float32(0.25)).astype(np.float32)
        x.reshape(-1)[[5, 40]] = np.float32(2.0), np.float32(1.75)
        x.reshape(-1)[[7, 19, 33, 60]] = np.float32(1.5)
    if name == "negzero_denormal":
        f = x.reshape(-1)
        f[::3] = np.float32(-0.0)
        f[1::3] = (rng.integers(1, 1 << 22, f[1::3].shape).astype(np.uint32)).view(np.float32)      # fp32 denormals
        f[2::3] = np.float32(0.0)
        f[[4, 50, 100]] = np.float32(1e-30), np.float32(3e-38), np.float32(2e-38)
    return x, k


def make_bad_segments():
    """([6][20][30], {segment: status bit name}): segments 1, 3 and 4 break the precondition; 0, 2 and 5 are clean."""
    x = _errors(np.random.default_rng(9900), (6, 20, 30))
    x[1, 3, 4], x[3, 19, 29], x[4, 0, 0] = np.nan, np.inf, np.float32(-0.25)
    return x, {1: "nan", 3: "inf", 4: "negative"}


# ---------------------------------------------------------------------------------- restatements
def radius_of(sigma, truncate=4.0):
    return int(truncate * float(sigma) + 0.5)


def weights_numpy(sigma, truncate=4.0):
    """The 2 r + 1 taps of scipy's order-0 kernel, fp64; entry 0 is the outermost, entry r the centre."""
    r = radius_of(sigma, truncate)
    sigma2 = float(sigma) * float(sigma)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / sigma2 * x ** 2)
    return w / w.sum()


def _border(idx, n, defect):
    if defect == "mirror":                                   # d c b | a b c d | c b a: period 2n - 2
        if n == 1:
            return np.zeros_like(idx)
        m = np.mod(idx, 2 * n - 2)
        return np.where(m >= n, 2 * n - 2 - m, m)
    if defect == "single":                                   # one reflection, then clamped
        m = np.where(idx < 0, -idx - 1, idx)
        m = np.where(m >= n, 2 * n - 1 - m, m)
        return np.clip(m, 0, n - 1)
    m = np.mod(idx, 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def _lines(v, w, r, defect):
    """The symmetric kernel along the LAST axis of v; returns the accumulator's dtype (fp64)."""
    n = v.shape[-1]
    acc_t = np.float32 if defect == "fp32acc" else np.float64
    ext = v.astype(acc_t)[..., _border(np.arange(-r, n + r), n, defect)]
    w = w.astype(acc_t)
    acc = ext[..., r:r + n] * w[r]
    order = range(-1, -r - 1, -1) if defect == "centre_out" else range(-r, 0)
    for j in order:
        acc = acc + (ext[..., r + j:r + j + n] + ext[..., r - j:r - j + n]) * w[r + j]
    return acc


def gaussian_numpy(x, sigma, truncate=4.0, defect=None):
    """`scipy.ndimage.gaussian_filter(plane, sigma, truncate=truncate)` of every [H][W] plane of the fp32 array x ([..., H, W]).
    `defect` plants one of DEFECTS (the tests show that each changes some case's bits)."""
    x = np.asarray(x, np.float32)
    w, r = weights_numpy(sigma, truncate), radius_of(sigma, truncate)
    between = (lambda a: a) if defect == "noround" else (lambda a: a.astype(np.float32))
    if defect == "axes":
        t = between(_lines(x, w, r, defect))
        return np.swapaxes(_lines(np.swapaxes(t, -1, -2), w, r, defect), -1, -2).astype(np.float32)
    t = between(np.swapaxes(_lines(np.swapaxes(x, -1, -2), w, r, defect), -1, -2))
    return _lines(t, w, r, defect).astype(np.float32)


def tree_sum(v):
    """The sum of the fp64 vector v in the order of anoddpm_map_scores: thread t of 1024 adds the elements t, t + 1024, ... in
    that order; a halving tree folds the 64 partials of a wave and then the 16 wave sums.  (+0.0 stands for an element a
    thread skips: adding it to a non-negative partial changes nothing.)"""
    v = np.asarray(v, np.float64).reshape(-1)
    rows = -(-v.size // THREADS)
    p = np.zeros(rows * THREADS, np.float64)
    p[:v.size] = v
    acc = np.zeros(THREADS, np.float64)
    for row in p.reshape(rows, THREADS):
        acc = acc + row
    waves = acc.reshape(THREADS // WAVE, WAVE)
    off = WAVE // 2
    while off:
        waves = waves[:, :off] + waves[:, off:2 * off]
        off //= 2
    w = waves[:, 0]
    off = w.size // 2
    while off:
        w = w[:off] + w[off:2 * off]
        off //= 2
    return float(w[0])


def scores_numpy(x, k):
    """(max fp32, mean fp64, top-k mean fp64) of the image x (all values pooled; finite, >= 0, -0.0 counted as +0.0)."""
    v = np.abs(np.asarray(x, np.float32).reshape(-1))       # clears the sign of -0.0
    n = v.size
    assert 1 <= k <= n
    bits = v.view(np.uint32)
    vk_bits = np.partition(bits, n - k)[n - k]
    vk = float(np.array([vk_bits], np.uint32).view(np.float32)[0])
    above = bits > vk_bits
    v64 = v.astype(np.float64)
    rest = float(k - int(above.sum())) * vk
    return v.max(), tree_sum(v64) / float(n), (tree_sum(np.where(above, v64, 0.0)) + rest) / float(k)


def k_of(top, n):
    """`image_scores`' k: an int is k; a float in (0, 1] the fraction of the n values, at least one."""
    return top if isinstance(top, int) else max(1, int(top * n))


def check_fixture(kat, key, got):
    """`got` against the fixture: its SHA-256 always, the stored array or crops for a readable failure."""
    assert got.dtype == np.float32
    if key + "_out" in kat.files:
        want = kat[key + "_out"]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{key}: {int((got != want).sum())} elements differ"
    else:
        for cname, sl in crops(*got.shape[-2:]).items():
            assert got[(Ellipsis,) + sl].tobytes() == kat[f"{key}_out_{cname}"].tobytes(), f"{key}: crop {cname} differs"
    assert sha(got) == str(kat[key + "_out_sha"]), key


def within(got, want, terms):
    """The bar of the issue: `terms * 2^-52` relative (a sum of non-negative fp64 terms in any order is within (terms - 1) *
    2^-53, the division adds one rounding)."""
    return abs(got - want) <= terms * 2.0 ** -52 * abs(want)
