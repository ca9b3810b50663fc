"""Shared by the volume post-processing tests and their fixture generator (tests/golden/make_postproc3d_golden.py): the seeded
input recipes of the cases and plain-numpy restatements of the steps of csrc/postproc3d.hip,
  `median3d_numpy`      symmetric pad on three axes, stack the k^3 shifts, sort, take index k^3 // 2   (scipy.ndimage.median_filter)
  `erode3d_numpy`       AND over the L1 ball (octahedron) of radius n on a zero-padded volume          (scipy.ndimage.binary_erosion)
  `labels3d_numpy`      a host union-find over the forward-neighbour list of the connectivity          (scipy.ndimage.label)
  `components3d_numpy`  sizes by bincount, the size cut
The fixture tests/golden/postproc3d_kat.npz holds what scipy itself returns.  Every step selects or counts, so everything is
compared bit for bit: there is no tolerance anywhere.  Neither scipy nor a device is needed here.  Inputs are built from
elementwise IEEE arithmetic on seeded PCG64 draws only (no libm calls), so that their SHA-256 is the same on every platform.
Each restatement takes the one parameter a planted defect of tests/test_postproc3d_reference.py changes."""
import hashlib

import numpy as np

WINDOWS = (3, 5)
ERODE_N = (1, 3, 8)
CONNECTIVITY = (1, 2, 3)

# ---------------------------------------------------------------------------------- median cases
# name -> (shape, quantised to 1/64): one slice (the depth border reflects repeatedly), the window equal to the plane, W across a
# 32-wide tile, ragged in every axis, and exact ties in every window with several tiles per axis
MEDIAN = {
    "m1x7x9": ((1, 7, 9), False),
    "m2x5x5": ((2, 5, 5), False),
    "m3x9x40": ((3, 9, 40), False),
    "m6x20x37": ((6, 20, 37), False),
    "m9x40x70": ((9, 40, 70), True),
}
MEDIAN_FULL = ("m1x7x9", "m2x5x5", "m3x9x40")                # expected outputs stored in full; the others as SHA-256 + crops
BATCH_SHAPE, BATCH_PAD = (3, 5, 12, 40), 24                  # three volumes inside rows of 5 * 12 * 40 + 24 words
BAD_SHAPE = (4, 3, 8, 12)
BAD_VOLUMES = {0: "nan", 1: "inf", 2: "negative"}            # volume -> what breaks the precondition; volume 3 is clean


def field3(rng, d, h, w, quantise):
    """A squared-error-like volume: the square of (blocky structure - fine noise), smoothed by a 2 x 2 x 2 box, small values cut
    to exact zeros; `quantise` rounds down to multiples of 1/64 (many exact ties inside every window)."""
    fine = rng.random((d, h, w), dtype=np.float32)
    coarse = rng.random((-(-d // 2), -(-h // 8), -(-w // 8)), dtype=np.float32)
    coarse = np.repeat(np.repeat(np.repeat(coarse, 2, axis=0), 8, axis=1), 8, axis=2)[:d, :h, :w]
    t = coarse - np.float32(0.5) * fine
    s = (t * t).astype(np.float32)
    s = (s + np.roll(s, 1, 0)) * np.float32(0.5)
    s = ((s + np.roll(s, 1, 1)) + (np.roll(s, 1, 2) + np.roll(s, (1, 1), (1, 2)))) * np.float32(0.25)
    s = np.where(s < np.float32(0.03), np.float32(0), s).astype(np.float32)
    if quantise:
        s = (np.floor(s * np.float32(64)) / np.float32(64)).astype(np.float32)
    return s


def make_median_case(name):
    (d, h, w), quantise = MEDIAN[name]
    return field3(np.random.default_rng(9500 + sorted(MEDIAN).index(name)), d, h, w, quantise)


def make_batch():
    """(buffer [3][5 * 12 * 40 + 24], volumes [3][5][12][40] as a view into the buffer's rows, roi plane [12][40], roi volume
    [5][12][40], roi batch [3][5][12][40]): the padding holds values that must never be read or written."""
    rng = np.random.default_rng(9550)
    S, d, h, w = BATCH_SHAPE
    n = d * h * w
    buf = rng.random((S, n + BATCH_PAD), dtype=np.float32)
    for j in range(S):
        buf[j, :n] = field3(rng, d, h, w, j == 1).reshape(-1)
    roi = (rng.random((S, d, h, w), dtype=np.float32) < np.float32(0.7)).astype(np.float32)
    plane = np.zeros((h, w), np.float32)
    plane[2:h - 1, 3:w - 5] = 1
    plane[5, 20] = 0
    return buf, buf[:, :n].reshape(S, d, h, w), plane, roi[0].copy(), roi


def make_bad_batch():
    """[4][3][8][12]: volume 0 holds one NaN, 1 one inf, 2 one negative value; 3 is clean."""
    rng = np.random.default_rng(9560)
    S, d, h, w = BAD_SHAPE
    x = np.stack([field3(rng, d, h, w, False) for _ in range(S)])
    x[0, 1, 5, 7], x[1, 2, 7, 11], x[2, 0, 0, 0] = np.nan, np.inf, np.float32(-0.25)
    return x


# ---------------------------------------------------------------------------------- erosion cases
# name -> (shape, level).  `ERODE_EMPTY`: the (case, n) whose result is empty by the case's own extents; every other result is
# neither empty nor full (the generator checks it).
ERODE = {
    "ones19x21x40": ((19, 21, 40), 0.0),
    "holes9x24x40": ((9, 24, 40), 0.25),
    "ones1x9x9": ((1, 9, 9), 0.0),
}
ERODE_EMPTY = {("ones1x9x9", 1), ("ones1x9x9", 3), ("ones1x9x9", 8),           # one slice: zero above and below, everything goes
               ("holes9x24x40", 8)}                                           # 9 slices < 2 * 8 + 1


def make_erode_case(name):
    (d, h, w), level = ERODE[name]
    rng = np.random.default_rng(9600 + sorted(ERODE).index(name))
    x = rng.random((d, h, w), dtype=np.float32) * np.float32(0.5) + np.float32(0.5)        # in [0.5, 1): above both levels
    if name.startswith("holes"):
        holes = rng.random((d, h, w), dtype=np.float32) < np.float32(0.004)
        x = np.where(holes, np.float32(0.25), x).astype(np.float32)                       # exactly AT the level: not above
    return x, level


# ---------------------------------------------------------------------------------- component cases
# name -> min_size values (they straddle the sizes present); every case runs at connectivity 1, 2 and 3
COMPONENTS = {
    "empty": (1, 7),
    "full": (1, 4096, 4097),
    "checker": (1, 2, 768, 769),
    "edge": (1, 27, 28, 54, 55),
    "corner": (1, 27, 28, 54, 55),
    "path": (1, 7, 2112, 2113),
    "blobs": (1, 7, 30, 400),
}
COMPONENTS_FULL = ("edge", "corner", "blobs")                # expected map stored in full (bit-packed); the others as SHA-256


def winding_path(d, n):
    """A one-voxel-wide path through every slice of [d][n][n]: an even slice holds a serpentine (every other row, joined at
    alternating ends), an odd slice the one voxel that hands the path on to the next serpentine, at alternating ends."""
    s = np.zeros((n, n), np.float32)
    s[0::2] = 1
    for j, y in enumerate(range(1, n - 1, 2)):
        s[y, n - 1 if j % 2 == 0 else 0] = 1
    rows = list(range(0, n, 2))
    last = (rows[-1], 0 if len(rows) % 2 == 0 else n - 1)            # where the serpentine that starts at (0, 0) ends
    g = np.zeros((d, n, n), np.float32)
    for z in range(d):
        if z % 2 == 0:
            g[z] = s
        else:
            g[(z,) + (last if z % 4 == 1 else (0, 0))] = 1
    return g


def make_components_case(name):
    if name == "empty":
        return np.zeros((4, 32, 32), np.float32)
    if name == "full":
        return np.ones((4, 32, 32), np.float32)
    if name == "checker":
        i, j, k = np.meshgrid(np.arange(6), np.arange(16), np.arange(16), indexing="ij")
        return ((i + j + k) % 2 == 0).astype(np.float32)
    if name in ("edge", "corner"):
        g = np.zeros((8, 8, 8), np.float32)
        g[1:4, 1:4, 1:4] = 1
        if name == "edge":
            g[1:4, 4:7, 4:7] = 1                                         # (z, 3, 3) and (z, 4, 4): 18-neighbours, not 6-neighbours
        else:
            g[4:7, 4:7, 4:7] = 1                                         # (3, 3, 3) and (4, 4, 4): 26-neighbours only
        return g
    if name == "path":
        return winding_path(8, 32)
    f = median3d_numpy(field3(np.random.default_rng(9700), 8, 48, 56, False), 3)
    return (f > np.float32(0.2)).astype(np.float32)


# ---------------------------------------------------------------------------------- the scene of anomaly_metrics_volume
SCENE_SHAPE = (2, 6, 48, 40)
SCENE_LESION = ((0, slice(2, 5), slice(20, 23), slice(15, 18)), (1, slice(1, 4), slice(25, 28), slice(20, 23)))   # 3 x 3 x 3 each
SCENE_SPECK = ((0, slice(3, 4), slice(30, 33), slice(25, 28)), (1, slice(4, 5), slice(12, 15), slice(10, 13)))    # 1 x 3 x 3 each
SCENE_ROI_LEVEL = -0.95


def make_scene():
    """(real, recon, mask) [2][6][48][40] in [-1, 1]: an elliptic "brain" on a -1 background, a reconstruction that differs by
    small noise, by +1.0 on a lesion of 3 x 3 pixels on three neighbouring slices (in the mask; 9 pixels a slice, 27 voxels) and
    by +1.0 on a 3 x 3 speck on ONE slice and on isolated voxels (not in the mask)."""
    rng = np.random.default_rng(9800)
    V, d, h, w = SCENE_SHAPE
    i, j = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    e = ((i - np.float32(23.5)) / np.float32(20)) ** 2 + ((j - np.float32(19.5)) / np.float32(16)) ** 2
    brain = e <= np.float32(1)
    tissue = rng.random((V, d, h, w), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)
    real = np.where(brain, tissue, np.float32(-1)).astype(np.float32)
    noise = (rng.random((V, d, h, w), dtype=np.float32) - np.float32(0.5)) * np.float32(0.125)
    recon = np.where(brain, real + noise, real).astype(np.float32)
    mask = np.zeros((V, d, h, w), np.float32)
    for sl in SCENE_LESION:
        recon[sl] = real[sl] + np.float32(1)
        mask[sl] = 1
    for sl in SCENE_SPECK:
        recon[sl] = real[sl] + np.float32(1)
    dots = (rng.random((V, d, h, w), dtype=np.float32) < np.float32(0.002)) & brain & (mask == 0)
    recon = np.where(dots, real + np.float32(1), recon).astype(np.float32)
    return real, recon, mask


# ---------------------------------------------------------------------------------- fixture helpers
def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def crops(d, h, w):
    """The pieces of a big expected volume kept in the fixture for diagnosis: name -> (slices)."""
    e = min(4, h, w)
    return {"first_tl": (0, slice(0, e), slice(0, e)), "first_br": (0, slice(h - e, h), slice(w - e, w)),
            "last_tr": (d - 1, slice(0, e), slice(w - e, w)), "last_bl": (d - 1, slice(h - e, h), slice(0, e)),
            "mid": (d // 2, slice(h // 2 - 4, h // 2 + 4), slice(w // 2 - 4, w // 2 + 4))}


def check_volume(kat, key, got, full):
    """`got` against the fixture's entry: its SHA-256 always, the stored array or crops for a readable failure."""
    assert got.dtype == np.float32
    if full:
        want = kat[key]
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{key}: {int((got != want).sum())} elements differ"
    else:
        for cname, sl in crops(*got.shape[-3:]).items():
            assert got[sl].tobytes() == kat[f"{key}_{cname}"].tobytes(), f"{key}: crop {cname} differs"
    assert sha(got) == str(kat[key + "_sha"]), key


def unpack(kat, key, shape):
    return np.unpackbits(kat[key + "_bits"])[:int(np.prod(shape))].reshape(shape).astype(np.float32)


# ---------------------------------------------------------------------------------- restatements
def median3d_numpy(x, k, depth_mode="symmetric", rank_offset=0):
    """The k x k x k median of a [..., D, H, W] fp32 array, border rule d c b a | a b c d | d c b a on all three axes, repeated as
    often as the pad asks (numpy's "symmetric").  `depth_mode` / `rank_offset`: what a planted defect changes."""
    x = np.asarray(x, np.float32)
    r = k // 2
    d, h, w = x.shape[-3:]
    assert min(h, w) >= k
    lead = [(0, 0)] * (x.ndim - 3)
    p = np.pad(x, lead + [(r, r), (0, 0), (0, 0)], mode=depth_mode)
    p = np.pad(p, lead + [(0, 0), (r, r), (r, r)], mode="symmetric")
    stack = np.stack([p[..., dz:dz + d, dy:dy + h, dx:dx + w] for dz in range(k) for dy in range(k) for dx in range(k)])
    return np.sort(stack, axis=0)[k ** 3 // 2 + rank_offset]


def erode3d_numpy(x, n, level=0.0, ball="l1"):
    """n erosions with the 6-neighbour cross of x > level, zero outside: one AND over the L1 ball of radius n.  fp32 0 / 1."""
    b = np.asarray(x) > np.float32(level)
    d, h, w = b.shape[-3:]
    p = np.pad(b, [(0, 0)] * (b.ndim - 3) + [(n, n)] * 3, mode="constant", constant_values=False)
    out = np.ones(b.shape, bool)
    for dz in range(-n, n + 1):
        for dy in range(-n, n + 1):
            for dx in range(-n, n + 1):
                if ball == "linf" or abs(dz) + abs(dy) + abs(dx) <= n:
                    out &= p[..., n + dz:n + dz + d, n + dy:n + dy + h, n + dx:n + dx + w]
    return out.astype(np.float32)


def forward_neighbours(connectivity):
    """The offsets (dz, dy, dx) > (0, 0, 0) in lexicographic order with |dz| + |dy| + |dx| <= connectivity: 3 / 9 / 13 of them."""
    return [(dz, dy, dx) for dz in (0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) > (0, 0, 0) and abs(dz) + abs(dy) + abs(dx) <= connectivity]


def labels3d_numpy(b, connectivity, steps=None):
    """Root index per voxel (-1 on the background) of a [D][H][W] boolean volume: a host union-find with path halving."""
    d, h, w = b.shape
    fg = np.asarray(b, bool).reshape(-1)
    parent = list(range(d * h * w))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    steps = forward_neighbours(connectivity) if steps is None else steps
    for i in np.flatnonzero(fg).tolist():
        z, rem = divmod(i, h * w)
        y, x = divmod(rem, w)
        for dz, dy, dx in steps:
            zz, yy, xx = z + dz, y + dy, x + dx
            if zz < d and 0 <= yy < h and 0 <= xx < w and fg[(zz * h + yy) * w + xx]:
                ra, rb = find(i), find((zz * h + yy) * w + xx)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) if fg[i] else -1 for i in range(d * h * w)], np.int64).reshape(d, h, w)


def components3d_numpy(x, min_size, connectivity, level=0.0, labels=None):
    """(fp32 0 / 1 volume without the components of x > level below min_size voxels, (components found, components kept))."""
    b = np.asarray(x) > np.float32(level)
    lab = labels3d_numpy(b, connectivity) if labels is None else labels
    sizes = np.bincount(lab[lab >= 0], minlength=lab.size)
    keep = b & (sizes[np.maximum(lab, 0)] >= min_size)
    return keep.astype(np.float32), (int((sizes > 0).sum()), int(((sizes > 0) & (sizes >= min_size)).sum()))


def areas3d_numpy(x, connectivity, level=0.0):
    """(int32 size of every voxel's component, 0 on the background; number of components)."""
    b = np.asarray(x) > np.float32(level)
    lab = labels3d_numpy(b, connectivity)
    sizes = np.bincount(lab[lab >= 0], minlength=lab.size)
    return np.where(b, sizes[np.maximum(lab, 0)], 0).astype(np.int32), int((sizes > 0).sum())


def mkey(name, k):
    return f"{name}_k{k}"


def ekey(name, n):
    return f"{name}_n{n}"


def ckey(name, connectivity, min_size):
    return f"{name}_c{connectivity}_m{min_size}"
