"""Cases and numpy / scipy restatements shared by test_surface3d_reference.py (CPU) and test_gpu_surface3d.py: the exact Euclidean
distance transform and the boundary distances of whole volumes, csrc/surface3d.hip (include/anoddpm_hip.h has the definitions).

  edt3_brute       the squared distance to the nearest background voxel as an integer minimum over ALL background voxels, chunked
  edt3_separable   the kernel's own decomposition: z sweep, y search into a second buffer, x search; its keywords plant defects
                   and it counts the steps its walks take
  border6          m & ~binary_erosion(m) with the 6 face neighbours; its keywords plant defects
  surface3d_ref    scipy erosion -> border, scipy's transform -> integer squared distances from the feature indices, the header's
                   percentile, math.fsum means.  Every keyword that is not at its default is a planted defect
  surface3d_fp64   the same with the mean summed in the kernel's order: ranks t, t + 1024, ... per thread, the two halving trees
  slicewise_hd95   the plane-by-plane answer (mean of the planes' HD95): what a user gets from `surface_distance` slice by slice
The hostile-buffer calls of the three entry points are built on contract_cases (its table is extended for the duration of a
`registered()` block only, never edited)."""
import contextlib
import functools
import math

import numpy as np
from scipy import ndimage

import contract_cases as cc
import surface_cases as sfc

Y_TILE = 128                                                 # rows of the y pass's LDS tile (csrc/surface3d.hip: Y_LDS)
FACES = ndimage.generate_binary_structure(3, 1)
CUBE = ndimage.generate_binary_structure(3, 3)
IN_PLANE = FACES.copy()
IN_PLANE[0], IN_PLANE[2] = False, False
FAR = np.int64(1) << 40
EMPTY_PRED, EMPTY_REF = sfc.EMPTY_PRED, sfc.EMPTY_REF


# ---------------------------------------------------------------------------------- distance transform
def edt3_brute(fg):
    """[D, H, W] bool -> int64 squared distance to the nearest False voxel (0 on False); -1 everywhere when there is none."""
    fg = np.asarray(fg, bool)
    b = np.argwhere(~fg).astype(np.int64)
    if b.shape[0] == 0:
        return np.full(fg.shape, -1, np.int64)
    p = np.argwhere(np.ones(fg.shape, bool)).astype(np.int64)
    out = np.empty(p.shape[0], np.int64)
    step = max(1, (1 << 21) // b.shape[0])
    for i in range(0, p.shape[0], step):
        out[i:i + step] = ((p[i:i + step, None, :] - b[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    return out.reshape(fg.shape)


def edt3_scipy(fg):
    return ndimage.distance_transform_edt(np.asarray(fg, bool))


def edt3_scipy_exact(fg):
    """Integer squared distances from scipy's transform: the feature indices it returns, squared in integers."""
    fg = np.asarray(fg, bool)
    if fg.all():
        return np.full(fg.shape, -1, np.int64)
    idx = ndimage.distance_transform_edt(fg, return_distances=False, return_indices=True)
    grid = np.indices(fg.shape)
    return ((idx.astype(np.int64) - grid) ** 2).sum(axis=0)


def _sweep(fg):
    """g^2 along axis 0: the squared distance to the nearest False of the own column, FAR where it has none."""
    g = np.full(fg.shape, FAR, np.int64)
    d = np.full(fg.shape[1:], FAR, np.int64)
    for z in range(fg.shape[0]):
        d = np.where(fg[z], np.minimum(d + 1, FAR), 0)
        g[z] = d
    d = np.full(fg.shape[1:], FAR, np.int64)
    for z in range(fg.shape[0] - 1, -1, -1):
        d = np.where(fg[z], np.minimum(d + 1, FAR), 0)
        g[z] = np.minimum(g[z], d)
    return np.where(g >= FAR, FAR, g * g)


def _search(g2, axis, cap=None, bound="k2"):
    """min over |i - i'| <= cap of (i - i')^2 + g2 along `axis`, walking outwards while the bound lets a lane go on -> (result,
    steps): a step is one lane looking at distance k.  bound "k2": k^2 < best (the kernel's); "k": k < best (walks on for nothing)."""
    v = np.moveaxis(g2, axis, -1)
    n = v.shape[-1]
    best, steps = v.copy(), 0
    for k in range(1, n if cap is None else min(cap + 1, n)):
        active = (k * k < best) if bound == "k2" else (k < best)
        if not active.any():
            break
        steps += int(active.sum())
        cand = np.full(v.shape, 4 * FAR, np.int64)
        cand[..., k:] = v[..., :-k] + k * k
        cand[..., :-k] = np.minimum(cand[..., :-k], v[..., k:] + k * k)
        best = np.where(active, np.minimum(best, cand), best)
    return np.moveaxis(best, -1, axis), steps


def edt3_separable(fg, cap=None, inplace_y=False, skip_y=False, bound="k2", return_steps=False):
    """The kernel's decomposition; int64, -1 where nothing is in reach.  Defects: `cap` bounds every search, `inplace_y` lets the y
    search overwrite the buffer it reads (rows in ascending order, unstaged), `skip_y` leaves the y search out (the slice-wise
    transform plus the z sweep), `bound="k"` walks while k < best."""
    fg = np.asarray(fg, bool)
    g2 = _sweep(fg)
    steps_y = 0
    if skip_y:
        h2 = g2
    elif inplace_y:
        h2 = g2.copy()
        H = fg.shape[1]
        yy = np.arange(H, dtype=np.int64)
        for y in range(H):
            h2[:, y, :] = (h2 + ((yy - y) ** 2)[None, :, None]).min(axis=1)
    else:
        h2, steps_y = _search(g2, 1, cap, bound)
    d2, steps_x = _search(h2, 2, cap, bound)
    out = np.where(d2 >= FAR, -1, d2)
    return (out, steps_y, steps_x) if return_steps else out


def foreground(vol, level):
    return sfc.foreground(vol, level)


@functools.lru_cache(maxsize=None)
def transform_cases():
    """name -> (volumes [S, D, H, W] fp32, level).  Background is sparse in the larger ones: the brute force is volume x background."""
    rng = np.random.default_rng(43)
    c = {}
    c["one_fg"] = (np.ones((1, 1, 1, 1), np.float32), 0.0)                                    # no background: -1 / inf
    c["plane1x9x70"] = ((rng.random((1, 1, 9, 70)) > 0.3).astype(np.float32), 0.0)            # equals the plane transform
    c["flat5x1x7"] = ((rng.random((1, 5, 1, 7)) > 0.3).astype(np.float32), 0.0)
    c["flat7x5x1"] = ((rng.random((1, 7, 5, 1)) > 0.3).astype(np.float32), 0.0)
    c["dense3x4x5"] = ((rng.random((1, 3, 4, 5)) > 0.5).astype(np.float32), 0.0)
    sparse = np.ones((1, 9, 12, 33), np.float32)
    sparse.reshape(-1)[rng.choice(sparse.size, max(1, sparse.size // 200), replace=False)] = 0          # 0.5 % zeros: long walks
    c["sparse9x12x33"] = (sparse, 0.0)
    corner = np.ones((1, 17, 19, 23), np.float32)
    corner[0, 0, 0, 0] = 0                                                                    # largest value 16^2 + 18^2 + 22^2
    c["corner17x19x23"] = (corner, 0.0)
    wide = np.ones((1, 6, 37, 300), np.float32)                                               # W above the 256 threads of a row
    wide.reshape(-1)[rng.choice(wide.size, 40, replace=False)] = 0
    c["wide6x37x300"] = (wide, 0.0)
    long = np.ones((1, 2, 3, 4100), np.float32)                                               # a row too long for the staged path
    long[0, 0, 0, 5] = long[0, 1, 2, 4000] = long[0, 1, 1, 2050] = 0
    c["long2x3x4100"] = (long, 0.0)
    for H in (Y_TILE - 1, Y_TILE, Y_TILE + 1):                                                # around the y tile: staged / through L2
        v = np.ones((1, 2, H, 9), np.float32)
        v.reshape(-1)[rng.choice(v.size, max(2, v.size // 100), replace=False)] = 0
        v[0, 0, 0, 0] = v[0, 1, H - 1, 3] = 0                                                 # the first and the last row take part
        c[f"ytile2x{H}x9"] = (v, 0.0)
    mid = (rng.random((3, 4, 9, 11)) > 0.2).astype(np.float32)
    mid[1] = 1                                                                                # all foreground between two others
    c["all_fg_mid"] = (mid, 0.0)
    img = rng.random((2, 5, 8, 13)).astype(np.float32)
    img[0, 3, 4, 2] = img[1, 0, 0, 0] = img[1, 4, 7, 12] = np.nan                             # NaN is background
    c["level_nan"] = (img, 0.25)
    return c


def corner_closed_form(shape):
    z, y, x = np.indices(shape).astype(np.int64)
    return z * z + y * y + x * x


# ---------------------------------------------------------------------------------- boundary distances
def border6(m, structure=FACES, z_outside=True):
    """m & ~binary_erosion(m) on the 3-D array.  Defects: `structure=CUBE` (26 neighbours), `structure=IN_PLANE` (no z
    neighbours), `z_outside=False` (the slices beyond the two z faces repeat the faces instead of counting as background)."""
    m = np.asarray(m, bool)
    if z_outside:
        return m & ~ndimage.binary_erosion(m, structure=structure, iterations=1, border_value=0)
    p = np.concatenate([m[:1], m, m[-1:]], axis=0)
    return m & ~ndimage.binary_erosion(p, structure=structure, iterations=1, border_value=0)[1:-1]


def directed(pred, ref, structure=FACES, z_outside=True, transform=None):
    """(bp, br, d2_pr, d2_rp): the borders [D, H, W] bool and the int64 squared distances on them in voxel-index order.
    transform: None (scipy's, exact) or keywords of `edt3_separable` (a planted defect)."""
    bp, br = border6(pred, structure, z_outside), border6(ref, structure, z_outside)
    if transform is None:
        fp, fr = edt3_scipy_exact(~bp), edt3_scipy_exact(~br)
    else:
        fp, fr = edt3_separable(~bp, **transform), edt3_separable(~br, **transform)
        fp, fr = np.where(fp < 0, 2 ** 31 - 1, fp), np.where(fr < 0, 2 ** 31 - 1, fr)
    return bp, br, fr[bp], fp[br]


def _mean_fsum(d, b):
    return math.fsum(np.sqrt(d.astype(np.float64))) / d.size


def _mean_ranks(d, b):
    """The header's order: the border voxels ranked by voxel index; thread t adds ranks t, t + 1024, ...; two halving trees."""
    return sfc.kernel_sum(np.sqrt(d.astype(np.float64))) / np.float64(d.size)


def _mean_voxel_strided(d, b):
    """The plane kernel's order carried over (a defect here): thread t adds the VOXELS t, t + 1024, ... of the volume."""
    terms = np.zeros(b.size, np.float64)
    terms[b.reshape(-1)] = np.sqrt(d.astype(np.float64))
    return sfc.kernel_sum(terms) / np.float64(d.size)


def surface3d_ref(pred, ref, structure=FACES, z_outside=True, transform=None, pooled="pool", mean=_mean_fsum):
    """One pair of [D, H, W] bool volumes -> dict(counts, max2, mean, p95, status, hd, hd95, assd).  The defaults are the
    definition (with math.fsum means); every other value of a keyword is a planted defect."""
    bp, br, d_pr, d_rp = directed(pred, ref, structure, z_outside, transform)
    counts = np.array([d_pr.size, d_rp.size], np.int32)
    status = (EMPTY_PRED if d_pr.size == 0 else 0) | (EMPTY_REF if d_rp.size == 0 else 0)
    nan = float("nan")
    if status:
        return dict(counts=counts, max2=np.array([-1, -1], np.int32), mean=np.array([nan, nan]), p95=np.array([nan, nan, nan]),
                    status=status, hd=nan, hd95=nan, assd=nan)
    max2 = np.array([d_pr.max(), d_rp.max()], np.int32)
    m = np.array([mean(d_pr, bp), mean(d_rp, br)])
    p = [sfc.percentile95(np.sort(d)) for d in (d_pr, d_rp)]
    p.append(p[0] if pooled == "one_direction" else sfc.percentile95(np.sort(np.r_[d_pr, d_rp])))
    return dict(counts=counts, max2=max2, mean=m, p95=np.array(p), status=0, hd=float(np.sqrt(np.float64(max2.max()))), hd95=p[2],
                assd=float((m[0] + m[1]) / 2))


def surface3d_fp64(pred, ref):
    return surface3d_ref(pred, ref, mean=_mean_ranks)


def numpy_percentiles(pred, ref):
    """numpy.percentile(..., 95) of d_pr, d_rp and the two pooled, as a user computes them on the host."""
    _, _, d_pr, d_rp = directed(pred, ref)
    a, b = np.sqrt(d_pr.astype(np.float64)), np.sqrt(d_rp.astype(np.float64))
    return [float(np.percentile(v, 95)) for v in (a, b, np.r_[a, b])]


def slicewise_hd95(pred, ref):
    """Mean over the slices where both plane borders exist of the plane HD95 (NaN when there is none): NOT the volume's HD95."""
    v = [sfc.surface_ref(p, r) for p, r in zip(np.asarray(pred, bool), np.asarray(ref, bool))]
    v = [r["hd95"] for r in v if r["status"] == 0]
    return float(np.mean(v)) if v else float("nan")


def _blobs(rng, shape, sigma, cut):
    return (ndimage.gaussian_filter(rng.random(shape), sigma) > cut).astype(np.float32)


@functools.lru_cache(maxsize=None)
def surface_cases():
    """name -> (pred [S, D, H, W], ref [S, D, H, W] or one shared [D, H, W]), fp32 0 / 1."""
    c = {}
    rng = np.random.default_rng(47)
    shape = (12, 20, 24)
    r = _blobs(rng, shape, 2.0, 0.5)
    p = ((np.roll(r, (1, 1, 2), (0, 1, 2)) * (rng.random(shape) > 0.03) + _blobs(rng, shape, 2.0, 0.54)) > 0).astype(np.float32)
    c["blobs12x20x24"] = (p[None], r[None])
    shared = _blobs(rng, (6, 14, 17), 1.5, 0.5)
    three = np.stack([(np.roll(shared, (i - 1, 1, -i), (0, 1, 2)) * (rng.random(shared.shape) > 0.05)).astype(np.float32) for i in range(3)])
    c["batch3_shared"] = (three, shared)
    box = np.zeros((4, 5, 6, 7), np.float32)
    box[:, 1:4, 2:5, 1:5] = 1
    e_pred, e_ref = box.copy(), box.copy()
    e_pred[1] = 0                                                                             # status 1
    e_ref[2] = 0                                                                              # status 2
    e_pred[3] = e_ref[3] = 0                                                                  # status 3; pair 0 is intact
    c["empties"] = (e_pred, e_ref)
    c["identical"] = (box[:1].copy(), box[:1].copy())                                         # every distance 0
    a, b = np.zeros((1, 7, 9, 11), np.float32), np.zeros((1, 7, 9, 11), np.float32)
    a[0, 0, 0, 0] = b[0, 6, 8, 10] = 1
    c["corners"] = (a, b)                                                                     # n = 1 on both sides; max2 = 36 + 64 + 100
    c["all_fg"] = (np.ones((1, 5, 6, 7), np.float32), box[:1].copy())                         # border = the six faces
    flat = _blobs(rng, (1, 18, 21), 1.5, 0.5)
    c["one_slice"] = (flat[None], np.roll(flat, (2, 1), (1, 2))[None])                        # D = 1: every foreground voxel is border
    c["noise8x32x40"] = ((rng.random((1, 8, 32, 40)) > 0.5).astype(np.float32), (rng.random((1, 8, 32, 40)) > 0.5).astype(np.float32))
    lo, hi = np.zeros((1, 6, 12, 12), np.float32), np.zeros((1, 6, 12, 12), np.float32)
    lo[0, 1:4, 3:9, 3:9] = 1
    hi[0, 2:5, 3:9, 3:9] = 1                                                                  # the same box one slice up
    c["slice_shift"] = (lo, hi)
    return c


def pairs_of(pred, ref):
    return [(pred[s] > 0, (ref if ref.ndim == 3 else ref[s]) > 0) for s in range(pred.shape[0])]


@functools.lru_cache(maxsize=None)
def surface_expected(name):
    """(surface3d_fp64, surface3d_ref, numpy percentiles or None) of every pair of a case, computed once."""
    out = []
    for p, r in pairs_of(*surface_cases()[name]):
        k, f = surface3d_fp64(p, r), surface3d_ref(p, r)
        out.append((k, f, None if k["status"] else numpy_percentiles(p, r)))
    return out


# ---------------------------------------------------------------------------------- hostile buffers (contract_cases' method)
S = cc.S

TABLE = {
    "distance_transform3d": {
        "struct": "anoddpm_distance3d_args", "status": None, "ws_align": 4,
        "ws_fn": None, "ws_args": None, "ws_min": lambda c: 8 * c["S"] * c["D"] * c["H"] * c["W"],          # the header's formula
        "too_small": b"distance_transform3d: workspace too small",
        "fields": {"src": cc.inp("f4", "D*H*W", "src_stride", level=True), "sq": cc.out("i4", "[S][D][H][W]"),
                   "dist": cc.opt(cc.out("f8", "[S][D][H][W]")), "workspace": cc.WS}},
    "surface_distance3d": {
        "struct": "anoddpm_surface3d_args", "status": "status", "ws_align": 4,
        "ws_fn": "anoddpm_surface3d_workspace_bytes", "ws_args": lambda c: (c["S"], c["D"], c["H"], c["W"]),
        "ws_min": lambda c: 16 * c["S"] * c["D"] * c["H"] * c["W"] + 16 * c["S"] * c["D"] * c["H"] + 8 * c["S"],
        "too_small": b"surface_distance3d: workspace too small",
        "fields": {"pred": cc.inp("f4", "D*H*W", "pred_stride", level=True), "ref": cc.inp("f4", "D*H*W", "ref_stride", zero_ok=True, level=True),
                   "workspace": cc.WS, "counts": cc.out("i4", "[S][2]"), "max2": cc.out("i4", "[S][2]"), "mean": cc.out("f8", "[S][2]"),
                   "p95": cc.out("f8", "[S][3]"), "status": cc.out("i4", "[S]")}},
}


@contextlib.contextmanager
def registered():
    """contract_cases' table with the two entries above, for the duration of the block."""
    assert not set(TABLE) & set(cc.TABLE)
    cc.TABLE.update(TABLE)
    try:
        yield
    finally:
        for k in TABLE:
            cc.TABLE.pop(k, None)


def _restate_distance3d(call, inputs):
    c = call["scalars"]
    sq = np.stack([edt3_brute(foreground(v, c["level"])) for v in cc._planes(call, inputs)])
    out_ = {"sq": cc._e(sq, "i4")}
    if call["variant"]["dist"]:
        out_["dist"] = cc._e(np.where(sq < 0, np.inf, np.sqrt(np.maximum(sq, 0).astype(np.float64))), "f8")
    return out_


def _restate_surface3d(call, inputs):
    c = call["scalars"]
    pred, ref = cc._planes(call, inputs, "pred"), cc._planes(call, inputs, "ref")
    want = [surface3d_fp64(foreground(p, c["level"]), foreground(r, c["level"])) for p, r in zip(pred, ref)]
    return {k: cc._e([w[k] for w in want], t) for k, t in (("counts", "i4"), ("max2", "i4"), ("mean", "f8"), ("p95", "f8"), ("status", "i4"))}


@functools.lru_cache(maxsize=None)
def contract_calls():
    """entry -> the hostile-buffer calls of the two launching entry points (S = 3 segments; the middle one differs in kind)."""
    calls = {"distance_transform3d": [], "surface_distance3d": []}
    for (D, H, W), dist in (((3, 9, 33), True), ((3, 9, 33), False), ((2, 1, 4100), True), ((2, Y_TILE + 1, 5), True)):
        x = (cc._rng(15, D, H, W).random((S, D, H, W)) * np.float32(0.9) + np.float32(0.05)).astype(np.float32)
        if W == 4100:
            x[:] = 1
            x[0, 0, 0, 5] = x[0, 1, 0, 4000] = x[2, 1, 0, 2050] = 0
        x[1] = 1                                             # the middle volume: no background (sq -1, dist +inf)
        calls["distance_transform3d"].append(cc._call("distance_transform3d", f"{D}x{H}x{W}-{'dist' if dist else 'nodist'}-allfg-middle",
                                                      {"D": D, "H": H, "W": W, "level": 0.25}, {"src": cc._flat(x)}, _restate_distance3d,
                                                      {"dist": dist}))
    for shared in (False, True):
        rng = cc._rng(16, shared)
        mk = lambda: np.stack([ndimage.gaussian_filter(rng.random((4, 12, 19)), 1.2) for _ in range(S)])       # noqa: E731
        pred, ref = mk(), mk()
        pred, ref = [((v - v.min()) / (v.max() - v.min())).astype(np.float32) for v in (pred, ref)]
        pred[1] = np.float32(0.125)                          # the middle pair: an empty prediction
        calls["surface_distance3d"].append(cc._call("surface_distance3d", f"4x12x19-{'shared' if shared else 'own'}ref-emptypred-middle",
                                                    {"D": 4, "H": 12, "W": 19, "level": 0.5},
                                                    {"pred": cc._flat(pred), "ref": ref[0].reshape(-1) if shared else cc._flat(ref)},
                                                    _restate_surface3d))
    with registered():
        for cs in calls.values():
            for c in cs:
                cc.expected_of(c)
    return calls
