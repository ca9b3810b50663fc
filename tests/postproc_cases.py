"""Shared by the post-processing tests and their fixture generator (tests/golden/make_postproc_golden.py): the seeded input
recipes of the cases and plain-numpy restatements of the three steps of csrc/postproc.hip,
  `median_numpy`      symmetric pad, stack the k*k shifts, sort, take the middle      (scipy.ndimage.median_filter, reflect)
  `erode_numpy`       AND over the L1 ball of radius n on a zero-padded plane         (scipy.ndimage.binary_erosion, n iterations)
  `components_numpy`  a host union-find, sizes by bincount, the size cut              (scipy.ndimage.label + numpy.bincount)
The fixture tests/golden/postproc_kat.npz holds what scipy itself returns.  Every step selects or counts, so everything here
is compared bit for bit: there is no tolerance anywhere.  Neither scipy nor a device is needed here.  Inputs are built from
elementwise IEEE arithmetic on seeded PCG64 draws only (no libm calls), so that their SHA-256 is the same on every platform."""
import hashlib

import numpy as np

WINDOWS = (3, 5, 7)
ERODE_N = (1, 3, 8)
BATCH = 55
BAD_PLANES = {1: "nan", 3: "inf", 4: "negative"}            # plane -> what breaks the precondition in `make_bad_batch`

# ---------------------------------------------------------------------------------- median cases
# name -> (shape, quantised to 1/64)
MEDIAN = {
    "m25x41": ((25, 41), True),
    "m7x7": ((7, 7), False),
    "m8x300": ((8, 300), False),
    "m256": ((256, 256), True),
}
MEDIAN_FULL = ("m25x41", "m7x7", "m8x300", "strided")        # expected outputs stored in full; the others as SHA-256 + crops
STRIDED_SHAPE, STRIDED_PAD = (4, 16, 24), 8                  # four planes inside rows of 16 * 24 + 8 words


def _field(rng, h, w, quantise):
    """A squared-error-like field: the square of (blocky structure - fine noise), smoothed by a 2 x 2 box, small values cut to
    exact zeros; `quantise` rounds down to multiples of 1/64 (many exact ties inside every window)."""
    fine = rng.random((h, w), dtype=np.float32)
    coarse = rng.random((-(-h // 8), -(-w // 8)), dtype=np.float32)
    coarse = np.repeat(np.repeat(coarse, 8, axis=0), 8, axis=1)[:h, :w]
    d = coarse - np.float32(0.5) * fine
    s = (d * d).astype(np.float32)
    s = ((s + np.roll(s, 1, 0)) + (np.roll(s, 1, 1) + np.roll(s, (1, 1), (0, 1)))) * np.float32(0.25)
    s = np.where(s < np.float32(0.03), np.float32(0), s).astype(np.float32)
    if quantise:
        s = (np.floor(s * np.float32(64)) / np.float32(64)).astype(np.float32)
    return s


def make_median_case(name):
    (h, w), quantise = MEDIAN[name]
    return _field(np.random.default_rng(9000 + sorted(MEDIAN).index(name)), h, w, quantise)


def make_strided():
    """(buffer [4][16 * 24 + 8], planes [4][16][24]): the planes are a view into the buffer's rows -- row stride 392, not 384."""
    rng = np.random.default_rng(9050)
    S, h, w = STRIDED_SHAPE
    buf = rng.random((S, h * w + STRIDED_PAD), dtype=np.float32)
    for j in range(S):
        buf[j, :h * w] = _field(rng, h, w, j % 2 == 0).reshape(-1)
    return buf, buf[:, :h * w].reshape(S, h, w)


def make_roi(h, w, seed):
    """A 0 / 1 ellipse that leaves the corners and a band at the left edge outside."""
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    inside = ((i - (h - 1) / 2.0) / (0.45 * h)) ** 2 + ((j - (w - 1) / 2.0 - 3.0) / (0.4 * w)) ** 2 <= 1.0
    holes = np.random.default_rng(seed).random((h, w), dtype=np.float32) < np.float32(0.002)
    return (inside & ~holes).astype(np.float32)


def make_batch():
    """(maps [55][1][256][256], roi [256][256]): the maps of one detection_B sweep and the ONE region of interest they share."""
    rng = np.random.default_rng(9100)
    maps = np.stack([_field(rng, 256, 256, j % 3 == 0) for j in range(BATCH)])[:, None]
    return maps, make_roi(256, 256, 9101)


def make_bad_batch():
    """[6][32][48]: planes 1, 3 and 4 break the precondition (one NaN, one inf, one negative value); 0, 2 and 5 are clean."""
    rng = np.random.default_rng(9200)
    x = np.stack([_field(rng, 32, 48, False) for _ in range(6)])
    x[1, 5, 7], x[3, 31, 47], x[4, 0, 0] = np.nan, np.inf, np.float32(-0.25)
    return x


# ---------------------------------------------------------------------------------- erosion cases
# name -> (shape, level): the input is an image, the mask is image > level; it touches every border
ERODE = {
    "e25x41": ((25, 41), 0.0),
    "e7x7": ((7, 7), 0.0),
    "e8x300": ((8, 300), 0.0),
    "e64": ((64, 64), 0.25),
    "e256": ((256, 256), 0.0),
}


def make_erode_case(name):
    (h, w), level = ERODE[name]
    rng = np.random.default_rng(9300 + sorted(ERODE).index(name))
    x = rng.random((h, w), dtype=np.float32) * np.float32(0.5) + np.float32(0.5)          # in [0.5, 1): above both levels
    if name == "e7x7":
        return x, level                                                                    # all ones: n = 3 leaves the centre pixel
    holes = rng.random((h, w), dtype=np.float32) < np.float32(0.004)
    x = np.where(holes, np.float32(0) if level == 0.0 else np.float32(0.25), x).astype(np.float32)   # exactly AT the level: not above
    x[0, w // 2] = x[h - 1, w // 3] = x[h // 2, 0] = x[h // 3, w - 1] = np.float32(0.75)    # set on every border
    return x, level


# ---------------------------------------------------------------------------------- component cases
# name -> min_size values; every case runs at connectivity 1 and 2
COMPONENTS = {
    "empty": (1, 7),
    "full": (1, 7, 65537),
    "checker": (1, 2, 7, 2049),
    "spiral": (1, 7, 40000),
    "blobs": (1, 7, 30, 5000),
    "blobs40x56": (1, 7, 100),
}
COMPONENTS_FULL = ("blobs40x56",)                            # expected map stored in full (bit-packed); the others as SHA-256


def spiral(n):
    """A one-pixel-wide path that winds inwards from (0, 0), clockwise, one empty pixel between its turns: one long chain."""
    g = np.zeros((n, n), np.float32)
    y, x, dy, dx = 0, 0, 0, 1
    g[0, 0] = 1

    def free(yy, xx):
        return not (0 <= yy < n and 0 <= xx < n) or g[yy, xx] == 0

    while True:
        for _ in range(2):                                               # straight on, else one turn to the right
            ny, nx = y + dy, x + dx
            if 0 <= ny < n and 0 <= nx < n and g[ny, nx] == 0 and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            return g
        y, x = ny, nx
        g[y, x] = 1


def make_components_case(name):
    if name == "empty":
        return np.zeros((256, 256), np.float32)
    if name == "full":
        return np.ones((256, 256), np.float32)
    if name == "checker":
        i, j = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
        return ((i + j) % 2 == 0).astype(np.float32)
    if name == "spiral":
        return spiral(256)
    side = (256, 256) if name == "blobs" else (40, 56)
    f = _field(np.random.default_rng(9400 + len(name)), side[0], side[1], False)
    f = median_numpy(f, 3)
    return (f > np.float32(0.2)).astype(np.float32)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def crops(h, w):
    """The pieces of a big expected plane kept in the fixture for diagnosis: name -> (slices)."""
    e = min(8, h, w)
    return {"tl": (slice(0, e), slice(0, e)), "tr": (slice(0, e), slice(w - e, w)), "bl": (slice(h - e, h), slice(0, e)),
            "br": (slice(h - e, h), slice(w - e, w)), "mid": (slice(h // 2 - 8, h // 2 + 8), slice(w // 2 - 8, w // 2 + 8))}


def check_plane(kat, key, got, full):
    """`got` against the fixture's entry: its SHA-256 always, the stored array or crops for a readable failure."""
    assert got.dtype == np.float32
    if full:
        want = kat[key]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{key}: {int((got != want).sum())} elements differ"
    else:
        for cname, sl in crops(*got.shape[-2:]).items():
            want = kat[f"{key}_{cname}"]
            assert got[(Ellipsis,) + sl].tobytes() == want.tobytes(), f"{key}: crop {cname} differs"
    assert sha(got) == str(kat[key + "_sha"]), key


# ---------------------------------------------------------------------------------- restatements
def median_numpy(x, k):
    """The k x k median of an [H][W] (or [..., H, W]) fp32 array, border rule d c b a | a b c d | d c b a."""
    x = np.asarray(x, np.float32)
    r = k // 2
    h, w = x.shape[-2:]
    assert min(h, w) >= k
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)], mode="symmetric")
    stack = np.stack([p[..., dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)])
    return np.sort(stack, axis=0)[k * k // 2]


def erode_numpy(x, n, level=0.0):
    """n erosions with the 4-neighbour cross of x > level, zero outside: one AND over the L1 ball of radius n.  fp32 0 / 1."""
    b = np.asarray(x) > np.float32(level)
    h, w = b.shape[-2:]
    p = np.pad(b, [(0, 0)] * (b.ndim - 2) + [(n, n), (n, n)], mode="constant", constant_values=False)
    out = np.ones(b.shape, bool)
    for dy in range(-n, n + 1):
        for dx in range(-(n - abs(dy)), n - abs(dy) + 1):
            out &= p[..., n + dy:n + dy + h, n + dx:n + dx + w]
    return out.astype(np.float32)


def labels_numpy(b, connectivity):
    """Root index per pixel (-1 on the background) of an [H][W] boolean plane: a host union-find with path halving."""
    h, w = b.shape
    fg = np.asarray(b, bool).reshape(-1)
    parent = list(range(h * w))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    steps = [(0, 1), (1, 0)] + ([(1, -1), (1, 1)] if connectivity == 2 else [])
    for i in np.flatnonzero(fg).tolist():
        y, x = divmod(i, w)
        for dy, dx in steps:
            yy, xx = y + dy, x + dx
            if yy < h and 0 <= xx < w and fg[yy * w + xx]:
                ra, rb = find(i), find(yy * w + xx)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) if fg[i] else -1 for i in range(h * w)], np.int64).reshape(h, w)


def components_numpy(x, min_size, connectivity, level=0.0, labels=None):
    """(fp32 0 / 1 plane without the components of x > level below min_size pixels, (components found, components kept))."""
    b = np.asarray(x) > np.float32(level)
    lab = labels_numpy(b, connectivity) if labels is None else labels
    sizes = np.bincount(lab[lab >= 0], minlength=lab.size)
    keep = b & (sizes[np.maximum(lab, 0)] >= min_size)
    return keep.astype(np.float32), (int((sizes > 0).sum()), int(((sizes > 0) & (sizes >= min_size)).sum()))


def mkey(name, k):
    return f"{name}_k{k}"


def ekey(name, n):
    return f"{name}_n{n}"


def ckey(name, connectivity, min_size):
    return f"{name}_c{connectivity}_m{min_size}"
