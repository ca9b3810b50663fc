"""Shared by the keep-mask tests (anoddpm_keep_mask, csrc/keepmask.hip) and tools/bench_keepmask.py:
  `CASES`              the case list: seeded recipes, every parameter of the entry point at every value its code distinguishes
  `make_case`          the host arrays of a case
  `restate`            a numpy restatement by brute force: OR over the seeds with |dy| + |dx| <= r, nothing outside the plane
  `compare`            the ONE comparison the GPU tests use: keep bytes, stitched words, counts and status words, bit for bit
  `composition_torch`  what the library could do before the entry point existed, all on the device (leg B of the bench tool)
Everything compares, selects or counts: there is no tolerance anywhere.  Neither scipy nor a device is needed to import this."""
import numpy as np

ROC_NAN, ROC_BAD_MASK = 1, 8                                  # include/anoddpm_hip.h (the tests check them against _lib)
R_MAX = 8
SHAPES = ((1, 1), (1, 40), (5, 3), (16, 32), (17, 33), (40, 70))
# single pixel; one row; narrower than the radius; exactly one tile; one pixel past a tile both ways; several ragged tiles
PATTERNS = ("sparse", "corners", "border_row", "all_above", "none_above", "strict", "negzero", "nan_score", "nan_thr",
            "roi_outside", "isolation", "bad_roi")
DEFECTS = ("ge_for_gt", "border_ones", "chebyshev", "roi_before_only", "roi_after_only", "keep_inverted", "stitch_swapped",
           "thr_stride_ignored")


def _cases():
    """Every shape at every radius with seeded draws of the other parameters, then every pattern at the two ragged shapes with
    three planes, three channels, per-plane thresholds and every roi form, then two wide planes: 54 + 24 + 2 cases."""
    out, rng = [], np.random.default_rng(9700)
    for H, W in SHAPES:
        for r in range(R_MAX + 1):
            i = len(out)
            out.append(dict(H=H, W=W, r=r, pattern=PATTERNS[i % len(PATTERNS)], S=(1, 3)[int(rng.integers(2))], C=(1, 3)[int(rng.integers(2))],
                            thr_stride=int(rng.integers(2)), roi=(None, "shared", "plane")[int(rng.integers(3))],
                            real_per_plane=bool(rng.integers(2)), pad=(0, 5)[int(rng.integers(2))], stitch=i % 5 != 4, seed=9701 + i))
    for j, pattern in enumerate(PATTERNS):
        for k, (H, W, r) in enumerate(((17, 33, 2), (40, 70, 8))):
            out.append(dict(H=H, W=W, r=r, pattern=pattern, S=3, C=(3, 1)[k], thr_stride=1, roi=(None, "shared", "plane")[(j + k) % 3],
                            real_per_plane=k == 0, pad=(5, 0)[k], stitch=True, seed=9800 + 2 * j + k))
    # past 2048 workgroups a workgroup takes `span` tiles of a tile row: span 3 with a ragged last strip on two tile rows, span 2
    out.append(dict(H=17, W=32760, r=8, pattern="sparse", S=3, C=1, thr_stride=1, roi=None, real_per_plane=True, pad=5, stitch=True, seed=9900))
    out.append(dict(H=2, W=43700, r=1, pattern="roi_outside", S=3, C=1, thr_stride=0, roi="plane", real_per_plane=False, pad=0, stitch=True, seed=9901))
    for c in out:
        if c["pattern"] in ("roi_outside", "bad_roi") and c["roi"] is None:
            c["roi"] = "plane"
        if c["pattern"] == "isolation":
            c["stitch"] = True
        c["name"] = "{pattern}-{H}x{W}-r{r}-S{S}C{C}-t{thr_stride}-roi{roi}-rs{real_per_plane:d}-p{pad}-st{stitch:d}".format(**c)
    return out


CASES = _cases()


def make_roi(h, w, rng):
    """A 0 / 1 plane: an ellipse that leaves the corners outside (a plane too small for one: a seeded draw), with a few holes."""
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    inside = ((i - (h - 1) / 2.0) / (0.45 * h + 0.5)) ** 2 + ((j - (w - 1) / 2.0) / (0.4 * w + 0.5)) ** 2 <= 1.0
    if min(h, w) < 4:
        inside = rng.random((h, w)) < 0.7
    return (inside & ~(rng.random((h, w)) < 0.01)).astype(np.float32)


def make_case(c):
    """-> dict of host arrays: `buf` [S][H*W + pad] (the planes inside rows with garbage between them), `score` [S][H][W] (a view
    of buf), `thr` [S] (thr_stride 1) or [1], `roi` None / [H][W] / [S][H][W], `real` [S or 1][C][H][W], `recon` [S][C][H][W]."""
    rng = np.random.default_rng(c["seed"])
    S, C, H, W, pat = c["S"], c["C"], c["H"], c["W"], c["pattern"]
    f32 = np.float32
    buf = (rng.random((S, H * W + c["pad"]), dtype=np.float32) * f32(4) - f32(2)).astype(np.float32)   # the garbage: above and below everything
    score = buf[:, :H * W].reshape(S, H, W)
    score[...] = rng.random((S, H, W), dtype=np.float32)
    thr = np.full((S,), 0.97, np.float32) - f32(0.02) * np.arange(S, dtype=np.float32)       # a different one per plane
    if pat in ("corners", "border_row", "roi_outside", "isolation", "bad_roi"):
        score[...] *= f32(0.25)
        thr[:] = f32(0.5)
        if pat == "corners":
            score[:, 0, 0] = score[:, 0, W - 1] = score[:, H - 1, 0] = score[:, H - 1, W - 1] = f32(1)
        elif pat == "border_row":
            for p in range(S):
                if p % 2 == 0:
                    score[p, (0, H - 1)[(p // 2) % 2], :] = f32(1)
                else:
                    score[p, :, (0, W - 1)[(p // 2) % 2]] = f32(1)
        else:
            score[rng.random((S, H, W)) < 0.04] = f32(1)              # roi_outside: some of them land outside the roi
            score[:, H // 2, W // 2] = f32(1)
    elif pat == "all_above":
        thr[:] = f32(-1)
    elif pat == "none_above":
        thr[:] = f32(2)
    elif pat == "strict":                                            # the threshold is a value of the plane: AT it is not above it
        score[...] = np.floor(score * f32(8)) / f32(8)
        score[:, 0, 0] = f32(0.625)
        score[:, H // 2, W // 2] = f32(0.5)
        thr[:] = f32(0.5)
    elif pat == "negzero":                                           # plane 0: -0.0 / +0.0 against +0.0; others: +0.0 against -0.0
        score[...] = np.where(rng.random((S, H, W)) < 0.5, f32(-0.0), f32(0.0))
        score[0][rng.random((H, W)) < 0.05] = f32(1e-30)
        thr[:] = f32(-0.0)
        thr[0] = f32(0.0)
    elif pat == "nan_score":
        score[S // 2][rng.random((H, W)) < 0.1] = np.nan
        score[S // 2, H - 1, W - 1] = np.nan
    elif pat == "nan_thr":
        thr[S // 2] = np.nan
    if c["thr_stride"] == 0:
        thr = thr[S // 2:S // 2 + 1].copy()
    roi = None
    if c["roi"] is not None:
        roi = np.stack([make_roi(H, W, rng) for _ in range(S if c["roi"] == "plane" else 1)])
        if pat == "roi_outside":
            roi[:, H // 2, W // 2] = f32(0)                          # a certain seed outside
            roi[:, 0, :] = f32(0)
        if pat == "bad_roi":
            roi[-1, H - 1, 0] = f32(0.5)
            roi[0, 0, W - 1] = f32(2) if roi.shape[0] > 1 else roi[0, 0, W - 1]
        roi = roi[0] if c["roi"] == "shared" else roi
    real = (rng.random((S if c["real_per_plane"] else 1, C, H, W), dtype=np.float32) * f32(2) - f32(1)).astype(np.float32)
    recon = (rng.random((S, C, H, W), dtype=np.float32) * f32(2) - f32(1)).astype(np.float32)
    d = dict(buf=buf, score=score, thr=thr, roi=roi, real=real, recon=recon)
    if pat == "isolation":                                           # NaN where the select must NOT look
        regen = restate(c, d)["keep"] == 0
        if real.shape[0] == 1:
            real[0][:, regen.all(axis=0)] = np.nan
        else:
            real[np.broadcast_to(regen[:, None], real.shape)] = np.nan
        recon[np.broadcast_to(~regen[:, None], recon.shape)] = np.nan
    return d


def dilate_numpy(seed, r, metric="l1", outside=False):
    """[..., H, W] boolean: OR over the ball of radius r (|dy| + |dx| <= r; "chebyshev": max(|dy|, |dx|) <= r), the outside of the
    plane contributing `outside`.  r = 0: seed itself."""
    seed = np.asarray(seed, bool)
    h, w = seed.shape[-2:]
    p = np.pad(seed, [(0, 0)] * (seed.ndim - 2) + [(r, r), (r, r)], mode="constant", constant_values=outside)
    out = np.zeros(seed.shape, bool)
    for dy in range(-r, r + 1):
        span = r - abs(dy) if metric == "l1" else r
        for dx in range(-span, span + 1):
            out |= p[..., r + dy:r + dy + h, r + dx:r + dx + w]
    return out


def restate(c, d, defect=None):
    """What anoddpm_keep_mask must write for case `c` with arrays `d`: keep uint8 [S][H][W], stitched fp32 [S][C][H][W] or None,
    regen int32 [S], status int32 [S].  `defect`: one of DEFECTS, planted on purpose -- what `compare` has to catch."""
    assert defect is None or defect in DEFECTS
    S, r = c["S"], c["r"]
    score, roi = d["score"], d["roi"]
    thr = np.broadcast_to(d["thr"][:1] if defect == "thr_stride_ignored" else d["thr"], (S,))
    with np.errstate(invalid="ignore"):
        above = score >= thr[:, None, None] if defect == "ge_for_gt" else score > thr[:, None, None]
    inside = np.ones(score.shape, bool) if roi is None else np.broadcast_to(roi == np.float32(1), score.shape)
    seed = above if defect == "roi_after_only" else above & inside
    grown = dilate_numpy(seed, r, "chebyshev" if defect == "chebyshev" else "l1", outside=defect == "border_ones")
    regen = grown if defect == "roi_before_only" else grown & inside
    keep = (regen if defect == "keep_inverted" else ~regen).astype(np.uint8)
    stitched = None
    if c["stitch"]:
        real = np.broadcast_to(d["real"], d["recon"].shape)
        a, b = (real, d["recon"]) if defect == "stitch_swapped" else (d["recon"], real)
        stitched = np.where(regen[:, None], a, b).astype(np.float32)
    status = np.zeros((S,), np.int32)
    status[np.isnan(score).any(axis=(1, 2)) | np.isnan(thr)] |= ROC_NAN
    if roi is not None:
        bad = ~((roi == 0) | (roi == 1))
        status[np.broadcast_to(bad.any(axis=(-2, -1)), (S,))] |= ROC_BAD_MASK
    return dict(keep=keep, stitched=stitched, regen=(keep == 0).sum(axis=(1, 2)).astype(np.int32), status=status)


def compare(got, want, what=""):
    """Bit for bit and word for word; `got` / `want`: dicts of numpy arrays as `restate` returns them (keep may carry the channel
    dimension of 1 that metrics.keep_mask adds)."""
    gk, wk = np.asarray(got["keep"]), np.asarray(want["keep"])
    assert gk.dtype == np.uint8 and gk.size == wk.size, f"{what}: keep {gk.dtype} {gk.shape} against {wk.shape}"
    gk = gk.reshape(wk.shape)
    assert np.array_equal(gk, wk), f"{what}: {int((gk != wk).sum())} keep bytes differ, first at {tuple(np.argwhere(gk != wk)[0])}"
    assert (got["stitched"] is None) == (want["stitched"] is None), f"{what}: stitched present / absent"
    if want["stitched"] is not None:
        gs, ws = np.ascontiguousarray(got["stitched"]), np.ascontiguousarray(want["stitched"])
        assert gs.dtype == np.float32 and gs.shape == ws.shape, f"{what}: stitched {gs.dtype} {gs.shape} against {ws.shape}"
        diff = gs.view(np.uint32) != ws.view(np.uint32)
        assert not diff.any(), f"{what}: {int(diff.sum())} stitched words differ, first at {tuple(np.argwhere(diff)[0])}"
    for key in ("regen", "status"):
        g, w = np.asarray(got[key]).reshape(-1), np.asarray(want[key]).reshape(-1)
        assert g.dtype == np.int32 and np.array_equal(g, w), f"{what}: {key} {g.tolist()} against {w.tolist()}"


def composition_torch(score, thr, r, real=None, recon=None):
    """The composition the library offered before anoddpm_keep_mask, all on the device, without a roi: ATen `score > thr`; the
    complement padded by r with ones through `erode_mask(iterations=r)`, cropped and complemented again -- the only way the
    erosion (zero outside under an AND) yields a dilation with nothing outside; ATen `where`; the cast to bytes; `count_nonzero`.
    score [S, H, W], thr [S] or [1] on the device, real [S or 1, C, H, W], recon [S, C, H, W] -> (keep uint8 [S, H, W], stitched
    or None, regen int32 [S])."""
    import torch
    from anoddpm_amd import metrics
    seed = score > thr.reshape(-1, 1, 1)
    grown = seed
    if r > 0:
        comp = torch.nn.functional.pad(1.0 - seed.float(), (r, r, r, r), value=1.0)
        grown = metrics.erode_mask(comp, iterations=r)[:, r:-r, r:-r] == 0
    stitched = torch.where(grown[:, None], recon, real) if real is not None else None
    return (~grown).to(torch.uint8), stitched, torch.count_nonzero(grown, dim=(1, 2)).to(torch.int32)
