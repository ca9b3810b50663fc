"""Anomaly-map metrics on the device -- the build's counterpart of the reference's `evaluation.py`
(same function names, argument meaning and return types) on top of ONE fused HIP pass
(`anoddpm_anomaly_map`, csrc/metrics.hip) instead of ~20 ATen dispatches and several D2H copies per image.

Reference call sites: detection.py:229-250 (per test image: squared error -> threshold 0.5 -> dice / precision /
recall / IoU / FPR), GaussianDiffusion.py:517-520, 572-583 (mean of the averaged chains, `mse` / threshold images).

SSIM (evaluation.py:46-47: skimage's `structural_similarity`) runs on the device too (`anoddpm_ssim`, csrc/ssim.hip): a workgroup
stages a tile and its window halo of both images in LDS, forms the five window means in fp64 with separable passes in a fixed
order and sums the interior of the similarity map; a second tiny launch folds the per-tile sums.  `ssim` returns the `[S]` fp64
means of a batch (one `real` may be shared by all reconstructions) without a host synchronisation, deterministic, within 1e-10 of
skimage on fp64 copies of the same images; `SSIM` on device tensors returns a Python float as skimage does.  `data_range`
defaults to 2.0: the images live in [-1, 1], and that is what older skimage releases took from the float dtype for the
upstream call (current releases refuse float images without it).  Host arguments of `SSIM` go through skimage as upstream.

ROC / AUC (evaluation.py:78-87: sklearn's `roc_curve` + `auc` on the flattened mask and squared error) run on the device
(`anoddpm_roc_auc`, csrc/roc.hip): per segment one workgroup sorts 32-bit keys `(bits(score) << 1) | label`, walks the runs of equal
score and forms the AUC as the integer Mann-Whitney statistic `twoU / (2 P N)` -- exactly the trapezoid area under sklearn's curve,
deterministic, no host sort.  `roc_auc` returns the `[S]` AUCs of a batch without a host synchronisation, `roc_points` the curve
points sklearn keeps (`drop_intermediate`), `ROC_AUC` on device tensors sklearn's `(fpr, tpr, thresholds)` triple bit for bit
(the host only prepends `(0, 0, inf)` and divides the integer counts in fp64).  Scores must be finite and >= 0 (squared errors
are; -0.0 is reported as +0.0) and masks 0 / 1: anything else sets a status word, which `ROC_AUC` / `roc_points` turn into
`ValueError` and `roc_auc` / `anomaly_metrics` / the detection records into `NaN` beside the status.  Host (numpy / CPU tensor)
arguments of `ROC_AUC` and `AUC_score` go through sklearn as upstream; sklearn's UndefinedMetricWarning for an empty class is not
re-issued by the native path (the arrays are NaN as sklearn's are).

Precision-recall (sklearn's `precision_recall_curve` / `average_precision_score`, and the best Dice over all thresholds, which the
reference has no counterpart of: it scores every map at the one cut 0.5) come from the SAME launch and the same sort: one more walk
over the runs of equal score.  `average_precision` returns the `[S]` fp64 APs (fixed summation order: same input, same bits; within
n * 2^-52 of sklearn), `best_dice` the largest `2 tp / (tp + fp + P)` over all thresholds -- found by exact integer comparison,
ties to the highest threshold -- with that threshold and its `tp` / `fp`, both without a host synchronisation; `pr_points` every
point of the curve as integer counts, `PR_curve` on device tensors sklearn's `(precision, recall, thresholds)` triple bit for bit.
A segment without positives has AP = NaN and best Dice = NaN (sklearn: AP 0.0 after a warning); one without negatives has AP = 1.0.

One curve pooled over a whole test set (detection.py:538-643 `roc_data`: mask and squared error of every scored slice, one
`ROC_AUC` call on the lot; 22 volumes x 4 slices x 256^2 = 5 767 168 pixels with `iterateKnown_restricted`).  One workgroup per
segment is the right shape for the maps of a sweep and leaves all but one compute unit idle on such a segment:
`anoddpm_roc_auc_wide` (csrc/roc_wide.hip) sorts and walks ONE segment with the whole chip, as 16 to 18 launches with one workgroup
per tile of keys, and writes the same bits.  `_roc_launch` takes it for a single segment of at least `ROC_WIDE_MIN_N` elements
(environment `ANODDPM_ROC_WIDE_MIN_N`), so nothing the functions above return changes.  `PooledCurves` collects the maps of a
run in two preallocated device buffers without a host synchronisation and scores the pooled segment; `ROC_AUC` and `PR_curve`
also take a list of device tensors on each side, meaning the pooled segment of all of them.
The per-region overlap score pools the same way and is a data-set score by definition: `anoddpm_pro_auc_wide` (csrc/pro_wide.hip)
sorts (key, area) pairs and walks ONE segment with the whole chip, as 18 launches, and writes the bits of `anoddpm_pro_auc`;
`_pro_launch` takes it for a single segment of at least `PRO_WIDE_MIN_N` elements (environment `ANODDPM_PRO_WIDE_MIN_N`).
`PooledRegionCurves` is a `PooledCurves` that also keeps the region areas, so one pool yields AUPRO beside AUROC, AP and best
Dice; `AUPRO` takes a list of device tensors on each side too.

Post-processing (the reference has none: it scores the raw squared error).  Published brain-MRI anomaly-segmentation pipelines
median-filter the residual, restrict it to an eroded brain mask and drop tiny components from the binary prediction before they
report AP and Dice.  `median_filter` (scipy.ndimage.median_filter, windows 3 / 5 / 7, reflect border), `erode_mask`
(scipy.ndimage.binary_erosion, cross, 1 ... 8 iterations) and `remove_small_components` (scipy.ndimage.label + bincount) do that
on the device (csrc/postproc.hip), batched over all maps of a sweep, bit for bit what scipy returns and without a host
synchronisation.  `PostProcess` holds the settings; the `_pp` results stand beside the raw ones.  Everything is opt-in: without it nothing changes.

Per-region overlap (Bergmann et al., "The MVTec Anomaly Detection Dataset", IJCV 2021; the reference has no counterpart).  Every
score above is pixel-wise, so one large lesion decides it; the PRO curve gives every connected ground-truth region the same weight
and AUPRO integrates it up to a false-positive rate of 0.3.  `component_areas` (csrc/postproc.hip) gives every mask pixel the size
of its region, `aupro` sorts `(score, area)` pairs and walks the curve in ONE launch per batch (`anoddpm_pro_auc`, csrc/pro.hip: one
workgroup per segment, fp64 sums in a fixed order -- same input, same bits), `pro_points` returns the curve, `AUPRO` a Python float.

Boundary distances (the reference has no counterpart): how far the predicted outline lies from the true one, which no overlap score
says.  `distance_transform` is `scipy.ndimage.distance_transform_edt(plane > level)` of every plane of a batch (csrc/surface.hip: a
sweep down and up every column, then per row the integer minimum over `(x - x')^2 + g^2`), bit for bit; `surface_distance` gives the
Hausdorff distance, its 95th percentile (`hd95`, medpy's pooled form) and the average symmetric surface distance of every
prediction against its reference or against one shared reference, in four launches whatever the batch: the order statistics are
selected on the integer squared distances and the means are fp64 sums in a fixed order, so the same input gives the same bits.
`HD95` returns a Python float.  Pixel units only (no `sampling=`), 2-D planes only, one threshold per call.

Volume-wise post-processing (csrc/postproc3d.hip).  The protocols the defaults above come from report one Dice per volume:
they filter the residual volume, erode the brain mask and drop small components in 3-D, which is not the plane-wise result slice
by slice.  `median_filter3d` (windows 3 / 5, reflect border on all three axes, any depth), `erode_mask3d` (the 6-neighbour cross)
and `remove_small_components3d` / `component_areas3d` (6 / 18 / 26 neighbours) are scipy's results bit for bit on `[..., D, H, W]`
tensors; `VolumePostProcess` holds the settings, `postprocess_volumes` applies them and `anomaly_metrics_volume` scores every
volume as ONE segment.  Nothing above changes when they are not called.  `gaussian_filter3d` (csrc/gauss3d.hip) is
`scipy.ndimage.gaussian_filter` of a volume with a sigma per axis, bit for bit; `VolumePostProcess(gaussian=)` puts it first.
Boundary distances of whole volumes (csrc/surface3d.hip), in voxel units: `distance_transform3d` is scipy's
`distance_transform_edt` of a volume bit for bit, `surface_distance3d` gives one `hd` / `hd95` / `assd` per volume (6-neighbour
border; not the planes' numbers averaged), `HD95_volume` a float, and `anomaly_metrics_volume_surface` is `anomaly_metrics_volume`
with `HD`, `HD95`, `ASSD`, `surface_status` added to every record.

Texture protocol (Bergmann et al.; the reference evaluates DAGM carpet and MVTec leather with the brain-MRI code path).  Published
pipelines smooth the anomaly map with `scipy.ndimage.gaussian_filter(map, sigma=4)` before AUROC / PRO and report an image-level
AUROC of one score per image first.  `gaussian_filter` is that filter on the device (`anoddpm_gauss2d`, csrc/smooth.hip: one launch
over all planes of a batch, scipy's fp64 taps in scipy's order, bit for bit scipy's for finite inputs), `image_scores` the maximum,
mean and top-k mean of every image from ONE launch (`anoddpm_map_scores`: the k-th largest value is selected on the bit pattern,
the sums are fp64 in a fixed order), `image_auc` the AUROC of N such scores against N image labels (`roc_auc` of one segment).
`PostProcess(gaussian=sigma)` puts the filter in front of the median; `score_maps(..., image_top=)` adds the image scores.

Operating thresholds (the reference cuts every map at 0.5; `best_dice` needs the ground truth).  Unsupervised pipelines calibrate on
healthy data: the operating threshold is the value that a chosen share of the pixels of a healthy validation set exceeds.
`HealthyPool` collects those maps on the device, `HealthyPool.thresholds(fpr)` selects the values with the whole chip
(`anoddpm_select_wide`, csrc/select_wide.hip: up to 16 order statistics of one segment of up to 2^31 - 1 values, integer counts only
between workgroups, the fp64 sums in `image_scores`' order; `order_stats` is the primitive), and `counts_at` / `scores_at` /
`anomaly_metrics_at` score maps at thresholds that stay on the device (`anoddpm_threshold_counts`: exact tp / fp for up to 16
thresholds from one pass).  No result is copied to the host, and no threshold is read there.

Keep mask of a two-pass detection.  `keep_mask` turns a first-pass score plane and such a device-resident threshold into
the bytes a `KnownRegion` stores -- threshold, scipy's `binary_dilation` by 0 ... 8 pixels inside an optional roi -- with the stitched
start image of the second pass and the size of the region, in one launch (`anoddpm_keep_mask`, csrc/keepmask.hip);
`GaussianDiffusionModel.detection_two_pass` is its caller.

`score_maps` states the scoring pipeline once: R stacks of maps in, one launch per step whatever R is -- curve scores, SSIM, and
opt-in the post-processing with its own curve scores, AUPRO and the boundary distances -- a dict of device tensors with a leading
R axis out, without a host synchronisation; a score that cannot be computed has no key.  Its callers only say how a result
leaves: `anomaly_metrics` (with `postprocess`), `anomaly_metrics_pro` (`pro_limit`) and `anomaly_metrics_surface` run it with
R = 1 behind one fused `anomaly_maps` pass, copy every number to the host at once and return Python floats (NaN where there is no
score); `GaussianDiffusionModel._score_settings` (with `postprocess`, `pro_limit`, `surface_metrics`) runs it once over all
settings of a sweep and puts row j into record j as device tensors (None where there is no score).
The individual functions accept the reference's arguments; they use the fused pass when handed device tensors of
the shapes the reference passes and raise `AnoddpmError` otherwise (no CPU path)."""
import ctypes
import numbers
import os

import torch

from . import _lib
from ._lib import (AnomalyArgs, ComponentAreasArgs, ComponentsArgs, DistanceArgs, ErodeArgs, GaussArgs, KeepMaskArgs, MapScoresArgs, MedianArgs, ProArgs, RocArgs, SelectArgs,
                   SsimArgs, SurfaceArgs, ThresholdCountsArgs, check, current_stream, lib)

__all__ = ["anomaly_maps", "score_maps", "anomaly_metrics", "anomaly_metrics_pro", "roc_auc", "roc_points", "curve_scores", "average_precision", "best_dice", "pr_points", "PR_curve", "PooledCurves", "PooledRegionCurves", "ssim", "median_filter", "erode_mask", "keep_mask",
           "remove_small_components", "PostProcess", "postprocess_maps", "component_areas", "median_filter3d", "erode_mask3d", "remove_small_components3d",
           "component_areas3d", "gaussian_filter3d", "VolumePostProcess", "postprocess_volumes", "anomaly_metrics_volume", "anomaly_metrics_volume_surface", "distance_transform3d", "surface_distance3d", "HD95_volume", "aupro", "pro_points", "AUPRO", "distance_transform",
           "surface_distance", "HD95", "anomaly_metrics_surface", "gaussian_filter", "image_scores", "image_auc", "anomaly_metrics_image", "order_stats", "counts_at", "scores_at",
           "anomaly_metrics_at", "HealthyPool", "heatmap", "dice_coeff", "PSNR", "SSIM", "IoU", "precision", "recall",
           "FPR", "ROC_AUC", "AUC_score", "testing"]

NC = _lib.ANOMALY_NCOUNTS


def _f32c(x, name):
    _lib.require_cuda(x, name)
    if x.dtype != torch.float32:
        x = x.float()
    return x.contiguous()


def _launch(name, a, dev, workspace=None):
    """The tail of every wrapper: `anoddpm_<name>(a)` on dev's current stream.  `workspace`: `(nbytes, dtype, text)` -- what the
    entry point's `*_workspace_bytes` answered (negative: ValueError(text)), allocated as `dtype` elements into `a.workspace` /
    `a.workspace_bytes`."""
    if workspace is not None:
        nbytes, dtype, text = workspace
        if nbytes < 0:
            raise ValueError(text)
        ws = torch.empty((nbytes // dtype.itemsize,), dtype=dtype, device=dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    with torch.cuda.device(dev):
        check(getattr(lib(), "anoddpm_" + name)(ctypes.byref(a), current_stream()), name)


def _nan_where_status(o, key):
    """`o[key]` of a launch's results with NaN where its status word is non-zero."""
    return torch.where(o["status"] != 0, torch.full_like(o[key], float("nan")), o[key])


def _curve_buffers(out, second, dtype, S, cap, dev):
    """The curve arrays of a ROC / PRO launch into `out` -- `fps`, `second` (`tps` / `pro`, of `dtype`), `thresholds` [S, cap] and
    `len` [S] -- and their pointers with `cap`, in the order of the `curve_*` fields of the argument structs."""
    out["fps"] = torch.empty((S, cap), dtype=torch.int32, device=dev)
    out[second] = torch.empty((S, cap), dtype=dtype, device=dev)
    out["thresholds"] = torch.empty((S, cap), dtype=torch.float32, device=dev)
    out["len"] = torch.empty((S,), dtype=torch.int32, device=dev)
    return out["fps"].data_ptr(), out[second].data_ptr(), out["thresholds"].data_ptr(), out["len"].data_ptr(), cap


def anomaly_maps(real, recon, mask=None, threshold=0.5, want=("mean", "sqerr", "mse_img", "thr_img", "pred")):
    """One fused pass.  real: [B,C,H,W]; recon: [B,C,H,W] (one reconstruction per image) or [navg,B,C,H,W] /
    ([navg,C,H,W] with B == 1: the `output` tensor of detection_A/B); mask like real or None.
    Returns (maps dict of [B,C,H,W] tensors, counts [B,12] float64 on the device)."""
    real = _f32c(real, "anomaly_maps(real)")
    recon = _f32c(recon, "anomaly_maps(recon)")
    B = real.shape[0]
    n = real[0].numel()
    if recon.dim() == real.dim() + 1:
        navg = recon.shape[0]
    elif recon.shape == real.shape:
        navg = 1
    elif B == 1 and recon.dim() == real.dim() and recon.shape[1:] == real.shape[1:]:
        navg = recon.shape[0]                      # [navg,C,H,W] for a single image
    else:
        raise ValueError(f"recon shape {tuple(recon.shape)} does not match real {tuple(real.shape)}")
    if recon.numel() != navg * B * n:
        raise ValueError("recon size mismatch")
    if mask is not None:
        mask = _f32c(mask, "anomaly_maps(mask)")
        if mask.numel() != B * n:
            raise ValueError("mask size mismatch")
    dev = real.device
    maps = {k: torch.empty_like(real) for k in want}
    counts = torch.zeros((B, NC), dtype=torch.float64, device=dev)       # the pass leaves the reserved column 11 alone: 0
    ws = torch.empty((_lib.ANOMALY_BLOCKS * B * NC,), dtype=torch.float64, device=dev)
    a = AnomalyArgs()
    a.recon, a.real, a.mask = recon.data_ptr(), real.data_ptr(), (mask.data_ptr() if mask is not None else None)
    for k in ("mean", "sqerr", "mse_img", "thr_img", "pred"):
        setattr(a, k, maps[k].data_ptr() if k in maps else None)
    a.counts, a.workspace, a.workspace_doubles = counts.data_ptr(), ws.data_ptr(), ws.numel()
    a.n, a.recon_as, a.recon_bs = n, B * n, n
    a.navg, a.B, a.threshold = navg, B, float(threshold)
    check(lib().anoddpm_anomaly_map(ctypes.byref(a), current_stream()), "anomaly_map")
    return maps, counts


def _ratios(c, smooth=0.000001):
    """The reference's formulas (evaluation.py:33-36, 50-76) on the summed counts; c: [B,12] float64 (host)."""
    out = {}
    out["dice_per_image"] = (2.0 * c[:, 2] + smooth) / (c[:, 0] + c[:, 1] + smooth)
    out["dice"] = out["dice_per_image"].mean()
    tp, fp_ref, fn_ref, tn = c[:, 3].sum(), c[:, 4].sum(), c[:, 5].sum(), c[:, 6].sum()
    out["precision"] = tp / (tp + fp_ref + 1e-6)            # evaluation.py:58-61 (its "FP" is mask==1 & recon==0)
    out["recall"] = tp / (tp + fn_ref + 1e-6)               # evaluation.py:65-68
    out["FPR"] = fp_ref / (fp_ref + tn + 1e-6)              # evaluation.py:71-74
    out["IoU"] = c[:, 7].sum() / (c[:, 8].sum() + 1e-8)     # evaluation.py:50-55
    return out


# ---------------------------------------------------------------------------------- ROC / AUC on the device
_ROC_STATUS_TEXT = ((_lib.ROC_NAN, "NaN score"), (_lib.ROC_INF, "infinite score"), (_lib.ROC_NEGATIVE, "negative score"),
                    (_lib.ROC_BAD_MASK, "mask value other than 0 and 1"), (_lib.ROC_CURVE_TRUNCATED, "curve buffer too small"))


def _roc_status_text(status):
    return ", ".join(t for bit, t in _ROC_STATUS_TEXT if status & bit)


def _raise_on_status(prefix, status):
    """ValueError for the first segment of `status` (host tensor of the kernels' words) that is non-zero."""
    for s, st in enumerate(status.tolist()):
        if st:
            raise ValueError(f"{prefix}: segment {s}: {_roc_status_text(st)} (scores must be finite and >= 0, masks 0 or 1)")


def _curve_arrays(o, names, s, L):
    """The first L points of segment s of the launch's curve arrays `names` on the host; the counts `fps` / `tps` as int64."""
    arrays = {k: o[k][s, :L].cpu().numpy() for k in names}
    return {k: a.astype("int64") if k in ("fps", "tps") else a for k, a in arrays.items()}


def _segments(x, S, name):
    """x as fp32 rows of a [S, n] view with unit element stride: (tensor that owns the memory, n, row stride in elements)."""
    _lib.require_cuda(x, name)
    if x.dtype != torch.float32:
        x = x.float()
    x = x.reshape(S, -1)
    n = x.shape[1]
    if S == 1 or n == 1 or x.stride(1) != 1 or x.stride(0) < n:
        x = x.contiguous()
        return x, n, n
    return x, n, x.stride(0)


_ROC_WIDE_NEVER = 1 << 31                                            # no segment is that long
# A single segment of at least this many elements is scored by the whole chip (anoddpm_roc_auc_wide); the outputs have the same
# bits.  65536 is the smallest measured power of two from which, at every larger measured size, the slowest wide repetition was
# below the fastest one-workgroup repetition (profiles/roc_wide_ab.txt); 2147483648 switches the path off.
ROC_WIDE_MIN_N = int(os.environ.get("ANODDPM_ROC_WIDE_MIN_N", "") or 65536)


def _roc_launch(mask, score, batched, curve, pr=False, wide=None, tile=None):
    """One `anoddpm_roc_auc` launch.  score: [S, ...] when batched, else one segment; mask: like score, or the shape of one
    segment (one mask shared by every segment).  `pr` adds the average precision and the best Dice (`ap`, `best_dice`,
    `best_threshold`, `best_counts`) and makes `curve` every run of equal score instead of the points sklearn's roc_curve keeps.
    `wide`: score the segments one after another with the whole chip (`anoddpm_roc_auc_wide`, `tile` keys per workgroup; None:
    the library's choice); None takes that path for one segment of at least `ROC_WIDE_MIN_N` elements.  Both paths write the same
    bits; `path` says which one ran ("wide" / "workgroup").  Returns a dict of device tensors; nothing is copied to the host."""
    if not isinstance(score, torch.Tensor) or not isinstance(mask, torch.Tensor):
        raise TypeError("roc: mask and score must be device tensors")
    S = score.shape[0] if batched else 1
    if score.numel() == 0 or S < 1:
        raise ValueError("roc: empty score")
    sc, n, s_stride = _segments(score, S, "roc(score)")
    if mask.numel() == S * n:
        mk, _, m_stride = _segments(mask, S, "roc(mask)")
    elif mask.numel() == n:
        mk, _, _ = _segments(mask, 1, "roc(mask)")
        m_stride = 0
    else:
        raise ValueError(f"roc: mask of {mask.numel()} elements does not match score {tuple(score.shape)}")
    if mk.device != sc.device:
        raise ValueError("roc: mask and score are on different devices")
    dev = sc.device
    if wide is None:
        wide = S == 1 and n >= ROC_WIDE_MIN_N
    out = {"auc": torch.empty((S,), dtype=torch.float64, device=dev),
           "counts": torch.empty((S, 4), dtype=torch.int64, device=dev),
           "status": torch.empty((S,), dtype=torch.int32, device=dev), "n": n, "path": "wide" if wide else "workgroup"}
    a = RocArgs()
    a.score, a.mask = sc.data_ptr(), mk.data_ptr()
    a.auc, a.counts, a.status = out["auc"].data_ptr(), out["counts"].data_ptr(), out["status"].data_ptr()
    a.n, a.score_stride, a.mask_stride, a.S = n, s_stride, m_stride, S
    if curve:                                                        # a segment has at most n distinct scores
        a.curve_fps, a.curve_tps, a.curve_thr, a.curve_len, a.curve_cap = _curve_buffers(out, "tps", torch.int32, S, max(n, 2), dev)
        a.curve_mode = _lib.ROC_CURVE_ALL if pr else _lib.ROC_CURVE_DROP
    if pr:
        out["ap"] = torch.empty((S,), dtype=torch.float64, device=dev)
        out["best_dice"] = torch.empty((S,), dtype=torch.float64, device=dev)
        out["best_threshold"] = torch.empty((S,), dtype=torch.float32, device=dev)
        out["best_counts"] = torch.empty((S, 2), dtype=torch.int64, device=dev)
        a.ap, a.best_dice = out["ap"].data_ptr(), out["best_dice"].data_ptr()
        a.best_thr, a.best_counts = out["best_threshold"].data_ptr(), out["best_counts"].data_ptr()
    if wide:
        tile = 0 if tile is None else int(tile)
        nbytes = lib().anoddpm_roc_wide_workspace_bytes(S, n, tile)
        if nbytes < 0:
            raise ValueError(f"roc: segment length {n} is outside [1, 2^31), or tile {tile} is not a multiple of 256 that cuts it into "
                             f"at most {_lib.ROC_WIDE_MAX_TILES} tiles")
        ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        with torch.cuda.device(dev):
            check(lib().anoddpm_roc_auc_wide(ctypes.byref(a), tile, current_stream()), "roc_auc_wide")
        return out
    _launch("roc_auc", a, dev, (lib().anoddpm_roc_workspace_bytes(S, n), torch.int32, f"roc: segment length {n} is outside [1, 2^31)"))
    return out


def _is_batched(score, batched):
    return score.dim() >= 3 if batched is None else bool(batched)


def roc_auc(mask, score, batched=None, return_status=False):
    """AUC of the ROC curve of every segment: score [S, ...] (`batched`; the default takes tensors of three or more dimensions
    as batches and anything smaller as one map), mask of the same shape or of one segment's shape (shared by all).  Returns an
    [S] fp64 device tensor -- `auc(*roc_curve(mask_s.flatten(), score_s.flatten())[:2])` per segment -- without a host
    synchronisation: NaN where a class is empty, and NaN where the inputs break the precondition (`return_status=True` also
    returns the [S] int32 status words)."""
    o = _roc_launch(mask, score, _is_batched(score, batched), curve=False)
    auc = _nan_where_status(o, "auc")
    return (auc, o["status"]) if return_status else auc


def roc_points(mask, score, batched=None):
    """The ROC points sklearn's `roc_curve` keeps (`drop_intermediate=True`), per segment, from the highest threshold down and
    without the `(0, 0, inf)` point it prepends: a list of dicts with `fps`, `tps` (int64 counts), `thresholds` (fp32), `auc`,
    `P`, `N`, `twoU` (Python numbers).  Copies to the host; raises ValueError for inputs outside the precondition."""
    o = _roc_launch(mask, score, _is_batched(score, batched), curve=True)
    status, lens, counts, auc = o["status"].cpu(), o["len"].cpu(), o["counts"].cpu(), o["auc"].cpu()
    _raise_on_status("roc", status)
    return [dict(_curve_arrays(o, ("fps", "tps", "thresholds"), s, L), auc=float(auc[s]),
                 P=int(counts[s, 0]), N=int(counts[s, 1]), twoU=int(counts[s, 2])) for s, L in enumerate(lens.tolist())]


def curve_scores(mask, score, batched):
    """Every score of a map from ONE launch and one sort (arguments as `_roc_launch`): a dict of [S] device tensors, no host
    synchronisation -- `auc`, `ap`, `best_dice` (fp64; NaN where `status`, the kernel's int32 word, is non-zero or the class they
    need is empty), `best_threshold` (fp32) and `best_counts` (int64 [S, 2]: tp and fp at that threshold)."""
    o = _roc_launch(mask, score, batched, curve=False, pr=True)
    out = {k: _nan_where_status(o, k) for k in ("auc", "ap", "best_dice")}
    out.update(best_threshold=o["best_threshold"], best_counts=o["best_counts"], status=o["status"])
    return out


def average_precision(mask, score, batched=None, return_status=False):
    """Average precision (area under the precision-recall curve as sklearn's `average_precision_score` defines it: the step sum
    `sum_k (R_k - R_{k-1}) P_k` over the distinct scores) of every segment; arguments as `roc_auc`.  Returns an [S] fp64 device
    tensor without a host synchronisation.  NaN where the segment has no positive: sklearn returns 0.0 after a warning there,
    which would silently pull down a mean over slices, most of which have no lesion.  1.0 where it has no negative.  NaN where
    the inputs break the precondition (`return_status=True` also returns the [S] int32 status words)."""
    o = curve_scores(mask, score, _is_batched(score, batched))
    return (o["ap"], o["status"]) if return_status else o["ap"]


def best_dice(mask, score, batched=None):
    """The largest Dice `2 tp / (tp + fp + P)` the prediction `score >= threshold` reaches over all thresholds (the plain
    definition, without the reference's 1e-6 smoothing), per segment; arguments as `roc_auc`.  Returns a dict of device tensors,
    no host synchronisation: `dice` [S] fp64, `threshold` [S] fp32 (the highest one when several reach it), `tp` / `fp` [S] int64
    at that threshold (precision, recall and IoU there follow from them and P), `status` [S] int32.  `dice` is NaN where the
    segment has no positive and where the status is non-zero."""
    o = curve_scores(mask, score, _is_batched(score, batched))
    return {"dice": o["best_dice"], "threshold": o["best_threshold"], "tp": o["best_counts"][:, 0], "fp": o["best_counts"][:, 1], "status": o["status"]}


def pr_points(mask, score, batched=None):
    """Every point of the precision-recall curve, per segment: one per distinct score, from the highest threshold down, as the
    integer counts of the prediction `score >= threshold`.  A list of dicts with `fps`, `tps` (int64), `thresholds` (fp32), `P`,
    `N`, `ap`, `best_dice`, `best_threshold`, `best_tp`, `best_fp` (Python numbers).  Copies to the host; raises ValueError for
    inputs outside the precondition."""
    o = _roc_launch(mask, score, _is_batched(score, batched), curve=True, pr=True)
    status, lens, counts = o["status"].cpu(), o["len"].cpu(), o["counts"].cpu()
    _raise_on_status("pr", status)
    ap, bd, bt, bc = o["ap"].cpu(), o["best_dice"].cpu(), o["best_threshold"].cpu(), o["best_counts"].cpu()
    return [dict(_curve_arrays(o, ("fps", "tps", "thresholds"), s, L), P=int(counts[s, 0]), N=int(counts[s, 1]),
                 ap=float(ap[s]), best_dice=float(bd[s]), best_threshold=float(bt[s]),
                 best_tp=int(bc[s, 0]), best_fp=int(bc[s, 1])) for s, L in enumerate(lens.tolist())]


# ---------------------------------------------------------------------------------- SSIM on the device
SSIM_K1, SSIM_K2 = 0.01, 0.03                                            # skimage's constants


def _ssim_window(win_size, gaussian_weights):
    """(win, mode, cn) as skimage derives them: gaussian weights fix the window at 2 * int(3.5 * 1.5 + 0.5) + 1 = 11 and use the
    population covariance; the uniform window uses the sample covariance."""
    if gaussian_weights:
        return 11, _lib.SSIM_GAUSSIAN, 1.0
    win = int(win_size)
    if win != win_size or win < 3 or win > _lib.SSIM_MAX_WIN or win % 2 == 0:
        raise ValueError(f"ssim: win_size must be odd and in 3 ... {_lib.SSIM_MAX_WIN}, got {win_size!r}")
    return win, _lib.SSIM_UNIFORM, win * win / (win * win - 1.0)


def _ssim_images(x, lead):
    """x as [*lead dims][C][H][W] -> (S, C, H, W); a 2-D image is one channel."""
    shape = tuple(x.shape)
    if len(shape) - lead == 2:
        return shape[:lead], 1, shape[-2], shape[-1]
    if len(shape) - lead == 3:
        return shape[:lead], shape[-3], shape[-2], shape[-1]
    raise ValueError(f"ssim: an image is [H, W] or [C, H, W], got shape {shape} with {lead} leading batch dimension(s)")


def ssim(real, recon, batched=None, data_range=2.0, win_size=7, gaussian_weights=False, full=False):
    """Mean structural similarity of every reconstruction with its image, as `skimage.metrics.structural_similarity(real_s,
    recon_s, channel_axis=0, data_range=..., win_size=..., gaussian_weights=...)` on fp64 copies: recon `[S, C, H, W]` (`batched`;
    the default takes tensors of four or more dimensions as batches of `[C, H, W]` images -- all leading dimensions flattened
    -- and `[C, H, W]` / `[H, W]` tensors as one image), real of the same shape or one image shared by every reconstruction.
    Returns an `[S]` fp64 device tensor, with `full=True` also the fp32 similarity map shaped like recon, without a host
    synchronisation.  NaN / inf in an image make that segment's value NaN.  ValueError for images smaller than the window."""
    if not isinstance(real, torch.Tensor) or not isinstance(recon, torch.Tensor):
        raise TypeError("ssim: real and recon must be device tensors")
    if batched is None:
        lead = max(recon.dim() - 3, 0)
    else:
        lead = 1 if batched else 0
    lead_shape, C, H, W = _ssim_images(recon, lead)
    S = 1
    for d in lead_shape:
        S *= d
    if S < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError(f"ssim: empty input {tuple(recon.shape)}")
    win, mode, cn = _ssim_window(win_size, gaussian_weights)
    if min(H, W) < win:
        raise ValueError(f"ssim: window of {win} exceeds the {H} x {W} image")
    n = C * H * W
    rc = _f32c(recon, "ssim(recon)")
    rl = _f32c(real, "ssim(real)")
    if rl.device != rc.device:
        raise ValueError("ssim: real and recon are on different devices")
    if rl.numel() == S * n:
        real_stride = n
    elif rl.numel() == n:
        real_stride = 0
    else:
        raise ValueError(f"ssim: real {tuple(real.shape)} does not match recon {tuple(recon.shape)}")
    dev = rc.device
    out = torch.empty((S,), dtype=torch.float64, device=dev)
    smap = torch.empty(tuple(recon.shape), dtype=torch.float32, device=dev) if full else None
    a = SsimArgs()
    a.real, a.recon = rl.data_ptr(), rc.data_ptr()
    a.mssim, a.map = out.data_ptr(), (smap.data_ptr() if full else None)
    a.real_stride, a.recon_stride = real_stride, n
    a.cn, a.data_range, a.K1, a.K2 = cn, float(data_range), SSIM_K1, SSIM_K2
    a.S, a.C, a.H, a.W, a.win, a.mode = S, C, H, W, win, mode
    _launch("ssim", a, dev, (lib().anoddpm_ssim_workspace_bytes(S, C, H, W), torch.float64, f"ssim: {S} x {C} x {H} x {W} is too large for one launch"))
    return (out, smap) if full else out

# ---------------------------------------------------------------------------------- post-processing on the device
def _planes(x, batched, what):
    """Shape bookkeeping of [S][C...][H][W]: (S, C, H, W); all dimensions between the batch axis and the plane are channels."""
    lead = 1 if batched else 0
    if x.dim() - lead < 2:
        raise ValueError(f"{what}: a segment is [..., H, W], got shape {tuple(x.shape)}" + (" as a batch" if batched else ""))
    S = x.shape[0] if batched else 1
    C = 1
    for d in x.shape[lead:-2]:
        C *= d
    H, W = x.shape[-2], x.shape[-1]
    if S < 1 or C < 1 or H < 1 or W < 1:
        raise ValueError(f"{what}: empty input {tuple(x.shape)}")
    return S, C, H, W


def _plane_rows(x, S, C, H, W, name):
    """x as S * C planes of H * W contiguous fp32: (tensor that owns the memory, plane stride in elements)."""
    t, n, stride = _segments(x, S, name)
    if C > 1 and stride != n:
        t, stride = t.contiguous(), n
    return t, (H * W if C > 1 else stride)


def median_filter(score, size=5, roi=None, batched=None, return_status=False):
    """`scipy.ndimage.median_filter(plane, size=size)` (reflect border) of every H x W plane of score: [S, ..., H, W] (`batched`;
    the default is `roc_auc`'s: three or more dimensions are a batch, a 2-D tensor is one map), every dimension before the last
    two a stack of planes.  size 3, 5 or 7, at most min(H, W).  `roi`: a 0 / 1 tensor shaped like one plane (shared by all), one
    segment or score; the result is +0.0 where it is 0 (the filter itself sees the unmasked map).  Returns a device tensor
    shaped like score, bit for bit scipy's, without a host synchronisation.  Scores must be finite and >= 0 as for `roc_auc`: a
    plane that is not gets a non-zero status word (`return_status=True` also returns them, int32, shaped like score without its
    last two dimensions) and an unspecified result."""
    if not isinstance(score, torch.Tensor):
        raise TypeError("median_filter: score must be a device tensor")
    if size not in _lib.MEDIAN_SIZES:
        raise ValueError(f"median_filter: size must be one of {_lib.MEDIAN_SIZES}, got {size!r}")
    S, C, H, W = _planes(score, _is_batched(score, batched), "median_filter")
    if min(H, W) < size:
        raise ValueError(f"median_filter: window of {size} exceeds the {H} x {W} plane")
    sc, s_stride = _plane_rows(score, S, C, H, W, "median_filter(score)")
    dev = sc.device
    a = MedianArgs()
    if roi is not None:
        if not isinstance(roi, torch.Tensor):
            raise TypeError("median_filter: roi must be a device tensor")
        if roi.numel() == H * W:
            a.roi_stride = 0
        elif roi.numel() == C * H * W:
            roi = roi.reshape(1, C, H, W).expand(S, C, H, W)
            a.roi_stride = H * W
        elif roi.numel() == S * C * H * W:
            a.roi_stride = H * W
        else:
            raise ValueError(f"median_filter: roi {tuple(roi.shape)} is neither a plane, a segment nor the shape of score {tuple(score.shape)}")
        rt = _f32c(roi, "median_filter(roi)")
        if rt.device != dev:
            raise ValueError("median_filter: roi and score are on different devices")
        a.roi = rt.data_ptr()
    out = torch.empty(tuple(score.shape), dtype=torch.float32, device=dev)
    status = torch.empty(tuple(score.shape[:-2]), dtype=torch.int32, device=dev)
    a.src, a.dst, a.status, a.src_stride = sc.data_ptr(), out.data_ptr(), status.data_ptr(), s_stride
    a.S, a.H, a.W, a.k = S * C, H, W, int(size)
    _launch("median2d", a, dev)
    return (out, status) if return_status else out


def erode_mask(x, iterations=3, level=0.0):
    """`scipy.ndimage.binary_erosion(plane > level, iterations=iterations)` (the 4-neighbour cross, zero outside the image) of
    every H x W plane of x ([..., H, W]); 1 ... 8 iterations.  Returns an fp32 0 / 1 device tensor shaped like x, no host
    synchronisation.  With the default level a 0 / 1 mask is eroded; with `level` an image is thresholded and eroded at once."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("erode_mask: x must be a device tensor")
    if int(iterations) != iterations or not 1 <= iterations <= _lib.ERODE_MAX:
        raise ValueError(f"erode_mask: iterations must be in 1 ... {_lib.ERODE_MAX}, got {iterations!r}")
    S, C, H, W = _planes(x, False, "erode_mask")
    xt = _f32c(x, "erode_mask(x)")
    out = torch.empty(tuple(x.shape), dtype=torch.float32, device=xt.device)
    a = ErodeArgs()
    a.src, a.dst, a.src_stride = xt.data_ptr(), out.data_ptr(), H * W
    a.S, a.H, a.W, a.n, a.level = C, H, W, int(iterations), float(level)
    _launch("erode2d", a, xt.device)
    return out


def keep_mask(score, threshold, dilate=2, roi=None, real=None, recon=None, return_status=False):
    """The step between the two passes of a two-pass detection, ONE launch (`anoddpm_keep_mask`, csrc/keepmask.hip), per
    H x W plane of score ([..., H, W]; the leading dimensions are the S planes):
      seed  = (plane > threshold) & roi;  grown = scipy.ndimage.binary_dilation(seed, iterations=dilate)  (the 4-neighbour cross,
      nothing outside the image; dilate 0 ... 8);  regen = grown & roi;  keep = ~regen;  stitched = where(regen, recon, real)
    `threshold`: a Python number (becomes a device fill, not a synchronising copy), a 1-element device tensor or a [S] device
    tensor -- e.g. `HealthyPool.thresholds`; it is never read on the host.  Strictly greater; NaN is above nothing, and a NaN
    threshold marks nothing.  `roi`: a 0 / 1 tensor of H * W (shared by all planes) or S * H * W values.  `real` [S or 1, C, H, W]
    and `recon` [S, C, H, W] come together; the C channels share the plane's mask.  Returns a dict of device tensors, no host
    synchronisation, the same bits every run: `keep` uint8, shaped like score with a channel dimension of 1 ([S, 1, H, W]: what
    `KnownRegion` takes), `stitched` fp32 [S, C, H, W] or None, `regen` int32 [S] (the pixels with keep == 0) and, with
    `return_status=True`, `status` int32 [S] (`ROC_NAN`: a NaN in the plane or its threshold; `ROC_BAD_MASK`: a roi value other
    than 0 / 1).  What the mask does to detection quality has not been measured."""
    if not isinstance(score, torch.Tensor):
        raise TypeError("keep_mask: score must be a device tensor")
    if isinstance(dilate, bool) or int(dilate) != dilate or not 0 <= dilate <= _lib.KEEP_DILATE_MAX:
        raise ValueError(f"keep_mask: dilate must be an integer in 0 ... {_lib.KEEP_DILATE_MAX}, got {dilate!r}")
    if score.dim() < 2 or score.numel() == 0:
        raise ValueError(f"keep_mask: score must be [..., H, W] and not empty, got shape {tuple(score.shape)}")
    if (real is None) != (recon is None):
        raise ValueError("keep_mask: real and recon come together (the stitch needs both)")
    H, W = score.shape[-2:]
    S = score.numel() // (H * W)
    if isinstance(threshold, torch.Tensor):
        if threshold.numel() not in (1, S):
            raise ValueError(f"keep_mask: threshold must hold 1 or {S} values (one per plane), got shape {tuple(threshold.shape)}")
    elif isinstance(threshold, bool) or not isinstance(threshold, numbers.Real):
        raise TypeError(f"keep_mask: threshold must be a number or a device tensor, got {type(threshold).__name__}")
    for name, x in (("roi", roi), ("real", real), ("recon", recon)):
        if x is not None and not isinstance(x, torch.Tensor):
            raise TypeError(f"keep_mask: {name} must be a device tensor")
    if roi is not None and roi.numel() not in (H * W, S * H * W):
        raise ValueError(f"keep_mask: roi {tuple(roi.shape)} is neither one plane nor the shape of score {tuple(score.shape)}")
    C = 1
    if real is not None:
        if recon.dim() != 4 or recon.shape[0] != S or tuple(recon.shape[2:]) != (H, W):
            raise ValueError(f"keep_mask: recon must be [{S}, C, {H}, {W}], got {tuple(recon.shape)}")
        C = recon.shape[1]
        if real.dim() != 4 or real.shape[0] not in (1, S) or tuple(real.shape[1:]) != (C, H, W):
            raise ValueError(f"keep_mask: real must be [{S} or 1, {C}, {H}, {W}], got {tuple(real.shape)}")
    sc = _f32c(score, "keep_mask(score)")
    dev = sc.device
    a = KeepMaskArgs()
    if isinstance(threshold, torch.Tensor):
        thr = _f32c(threshold, "keep_mask(threshold)").reshape(-1)
    else:
        thr = torch.full((1,), float(threshold), dtype=torch.float32, device=dev)
    hold = [sc, thr]                                                 # the fp32 copies live until the launch is enqueued
    for name, x in (("roi", roi), ("real", real), ("recon", recon), ("threshold", thr)):
        if x is not None:
            x = _f32c(x, f"keep_mask({name})")
            if x.device != dev:
                raise ValueError(f"keep_mask: {name} and score are on different devices")
            hold.append(x)
            setattr(a, name, x.data_ptr())
    out = {"keep": torch.empty((S, 1, H, W), dtype=torch.uint8, device=dev),
           "stitched": torch.empty((S, C, H, W), dtype=torch.float32, device=dev) if real is not None else None,
           "regen": torch.empty((S,), dtype=torch.int32, device=dev)}
    status = torch.empty((S,), dtype=torch.int32, device=dev)
    a.score, a.keep, a.regen_count, a.status = sc.data_ptr(), out["keep"].data_ptr(), out["regen"].data_ptr(), status.data_ptr()
    a.stitched = out["stitched"].data_ptr() if real is not None else None
    a.score_stride, a.thr_stride = H * W, (1 if thr.numel() == S and S > 1 else 0)
    a.roi_stride = H * W if roi is not None and roi.numel() == S * H * W and S > 1 else 0
    a.real_stride = C * H * W if real is not None and real.shape[0] == S and S > 1 else 0
    a.S, a.H, a.W, a.C, a.r = S, H, W, C, int(dilate)
    _launch("keep_mask", a, dev)
    if return_status:
        out["status"] = status
    return out


def _check_connectivity(connectivity, what):
    if connectivity not in (1, 2):
        raise ValueError(f"{what}: connectivity must be 1 (4 neighbours) or 2 (8 neighbours), got {connectivity!r}")


def _small_components(x, level, min_size, connectivity):
    """One `anoddpm_small_components` run on the planes of x > level: (fp32 0 / 1 map shaped like x, int64 counts [..., 2])."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("remove_small_components: pred must be a device tensor")
    if int(min_size) != min_size or min_size < 0:
        raise ValueError(f"remove_small_components: min_size must be an integer >= 0, got {min_size!r}")
    _check_connectivity(connectivity, "remove_small_components")
    S, C, H, W = _planes(x, False, "remove_small_components")
    xt = _f32c(x, "remove_small_components(pred)")
    dev = xt.device
    out = torch.empty(tuple(x.shape), dtype=torch.float32, device=dev)
    counts = torch.empty(tuple(x.shape[:-2]) + (2,), dtype=torch.int64, device=dev)
    a = ComponentsArgs()
    a.src, a.dst, a.counts = xt.data_ptr(), out.data_ptr(), counts.data_ptr()
    a.src_stride, a.S, a.H, a.W = H * W, C, H, W
    a.min_size, a.connectivity, a.level = int(min_size), int(connectivity), float(level)
    _launch("small_components", a, dev, (lib().anoddpm_small_components_workspace_bytes(C, H, W), torch.int32,
                                         f"remove_small_components: {tuple(x.shape)} has 2^31 pixels or more"))
    return out, counts


def remove_small_components(pred, min_size=7, connectivity=1, return_counts=False):
    """The binary prediction `pred` ([..., H, W], fp32 0 / 1) without its connected components of fewer than `min_size` pixels:
    `lab, _ = scipy.ndimage.label(plane); keep = numpy.bincount(lab.ravel()) >= min_size; keep[0] = False; keep[lab]` per plane.
    connectivity 1: 4 neighbours (label's default), 2: 8 neighbours.  Returns an fp32 0 / 1 device tensor shaped like pred,
    with `return_counts=True` also int64 `[..., 2]`: components found and components kept per plane.  No host synchronisation;
    the same bits every run."""
    out, counts = _small_components(pred, 0.0, min_size, connectivity)
    return (out, counts) if return_counts else out


def _gauss_radius(sigma, truncate, what):
    """scipy's radius `int(truncate * sigma + 0.5)` of positive finite floats; ValueError unless it is in 1 ... GAUSS_MAX_RADIUS."""
    ok = all(isinstance(v, (int, float)) and not isinstance(v, bool) and 0.0 < float(v) < float("inf") for v in (sigma, truncate))
    radius = int(float(truncate) * float(sigma) + 0.5) if ok else 0
    if not 1 <= radius <= _lib.GAUSS_MAX_RADIUS:
        raise ValueError(f"{what}: sigma and truncate must be positive finite numbers whose radius int(truncate * sigma + 0.5) is in "
                         f"1 ... {_lib.GAUSS_MAX_RADIUS}, got sigma={sigma!r}, truncate={truncate!r}")
    return radius


_GAUSS_TABLES = {}                                                   # (sigma, truncate, device) -> fp64 [radius + 1] on that device


def _gauss_table(sigma, truncate, radius, dev):
    """The taps `anoddpm_gauss2d` reads, outermost first, as scipy's `_gaussian_kernel1d` computes them with numpy in fp64.  Made
    and copied to the device once per (sigma, truncate, device): the first call allocates and copies, later ones only launch."""
    key = (float(sigma), float(truncate), dev)
    if key not in _GAUSS_TABLES:
        import numpy as np
        x = np.arange(-radius, radius + 1)
        w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
        w = w / w.sum()
        _GAUSS_TABLES[key] = torch.from_numpy(w[:radius + 1].copy()).to(dev)
    return _GAUSS_TABLES[key]


def gaussian_filter(score, sigma=4.0, truncate=4.0, batched=None):
    """`scipy.ndimage.gaussian_filter(plane, sigma, truncate=truncate)` (order 0, reflect border, the same sigma on both axes) of
    every H x W plane of score: [S, ..., H, W], batching and strides as `median_filter`.  Returns an fp32 device tensor shaped
    like score, bit for bit scipy's on the fp32 planes for finite inputs, in ONE launch and without a host synchronisation; a
    plane may be narrower than the radius.  `sigma` and `truncate`: positive finite numbers whose radius `int(truncate * sigma +
    0.5)` is in 1 ... 32 (sigma 4: 16), else ValueError.  NaN / inf spread within their radius by IEEE rules; no other plane is
    touched.  The tap table is cached per (sigma, truncate, device): after its first use a call only launches (graph-capture-safe)."""
    if not isinstance(score, torch.Tensor):
        raise TypeError("gaussian_filter: score must be a device tensor")
    radius = _gauss_radius(sigma, truncate, "gaussian_filter")
    S, C, H, W = _planes(score, _is_batched(score, batched), "gaussian_filter")
    sc, s_stride = _plane_rows(score, S, C, H, W, "gaussian_filter(score)")
    dev = sc.device
    out = torch.empty(tuple(score.shape), dtype=torch.float32, device=dev)
    a = GaussArgs()
    a.src, a.dst, a.w, a.src_stride = sc.data_ptr(), out.data_ptr(), _gauss_table(sigma, truncate, radius, dev).data_ptr(), s_stride
    a.S, a.H, a.W, a.radius = S * C, H, W, radius
    _launch("gauss2d", a, dev)
    return out


def image_scores(score, top=0.01, batched=None, return_status=False):
    """One score per image: score [S, ...] (`batched`; the default is `roc_auc`'s), every value of `score[s]` -- all channels
    -- pooled into image s.  Returns a dict of [S] device tensors from ONE launch, no host synchronisation, the same bits every
    run: `max` (fp32), `mean` (fp64) and `topk` (fp64): the mean of the k largest values (as a multiset: ties cannot matter).
    `top`: an int is k; a float in (0, 1] the fraction of the n values of an image, `k = max(1, int(top * n))`.  Values must be
    finite and >= 0 as for `roc_auc` (-0.0 counts as +0.0): an image that breaks this gets NaN and a non-zero status word
    (`return_status=True` returns `(dict, status)`, status int32 [S]).  n is at most 2^24 (one workgroup per image)."""
    if not isinstance(score, torch.Tensor):
        raise TypeError("image_scores: score must be a device tensor")
    S = score.shape[0] if _is_batched(score, batched) else 1
    if score.numel() == 0 or S < 1:
        raise ValueError("image_scores: empty score")
    sc, n, s_stride = _segments(score, S, "image_scores(score)")
    if isinstance(top, bool) or not isinstance(top, (int, float)):
        raise ValueError(f"image_scores: top must be an int k or a float fraction in (0, 1], got {top!r}")
    if isinstance(top, int):
        k = top
    elif 0.0 < top <= 1.0:
        k = max(1, int(top * n))
    else:
        raise ValueError(f"image_scores: a float top must be in (0, 1], got {top!r}")
    if not 1 <= k <= n:
        raise ValueError(f"image_scores: k = {k} is outside 1 ... n = {n}")
    if n > _lib.MAP_SCORES_MAX_N:
        raise ValueError(f"image_scores: an image of {n} values exceeds {_lib.MAP_SCORES_MAX_N}")
    dev = sc.device
    out = {"max": torch.empty((S,), dtype=torch.float32, device=dev), "mean": torch.empty((S,), dtype=torch.float64, device=dev),
           "topk": torch.empty((S,), dtype=torch.float64, device=dev), "status": torch.empty((S,), dtype=torch.int32, device=dev)}
    a = MapScoresArgs()
    a.src, a.max, a.mean, a.topk_mean, a.status = sc.data_ptr(), out["max"].data_ptr(), out["mean"].data_ptr(), out["topk"].data_ptr(), out["status"].data_ptr()
    a.src_stride, a.n, a.k, a.S = s_stride, n, k, S
    _launch("map_scores", a, dev)
    status = out.pop("status")
    for key in tuple(out):
        out[key] = torch.where(status != 0, torch.full_like(out[key], float("nan")), out[key])
    return (out, status) if return_status else out


def image_auc(labels, scores, return_status=False):
    """Image-level AUROC: `roc_auc` of ONE segment of N image scores (a device tensor of N values, e.g. `image_scores(...)["max"]`
    of a test set; ranked as fp32) against N 0 / 1 image labels.  Returns a [1] fp64 device tensor without a host synchronisation:
    NaN when a class is empty or the scores break `roc_auc`'s precondition (`return_status=True` also returns the status word)."""
    if not isinstance(labels, torch.Tensor) or not isinstance(scores, torch.Tensor):
        raise TypeError("image_auc: labels and scores must be device tensors")
    if labels.numel() != scores.numel():
        raise ValueError(f"image_auc: {labels.numel()} labels for {scores.numel()} scores")
    return roc_auc(labels.reshape(-1), scores.reshape(-1), batched=False, return_status=return_status)


# ---------------------------------------------------------------------------------- operating thresholds
def _rank_table(ranks, n, dev, what):
    """-> (int32 device tensor [Q] whose bits are the uint32 ranks, ctypes host copy or None).  A list (or a host tensor) is checked
    here; a device tensor is never read on the host."""
    if isinstance(ranks, torch.Tensor) and ranks.is_cuda:
        if ranks.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8, torch.int8):
            raise TypeError(f"{what}: a rank tensor holds integers, got {ranks.dtype}")
        Q = ranks.numel()
        if not 1 <= Q <= _lib.SELECT_MAX_RANKS:
            raise ValueError(f"{what}: 1 ... {_lib.SELECT_MAX_RANKS} ranks per call, got {Q}")
        if ranks.device != dev:
            raise ValueError(f"{what}: ranks and score are on different devices")
        # a rank outside [0, 2^31) becomes a pattern that is >= n: the kernel sets SELECT_BAD_RANK
        return ranks.reshape(-1).to(torch.int64).clamp(min=-1, max=0x7fffffff).to(torch.int32).contiguous(), None
    if isinstance(ranks, torch.Tensor):
        ranks = ranks.reshape(-1).tolist()
    ranks = [ranks] if isinstance(ranks, int) and not isinstance(ranks, bool) else list(ranks)
    if not 1 <= len(ranks) <= _lib.SELECT_MAX_RANKS:
        raise ValueError(f"{what}: 1 ... {_lib.SELECT_MAX_RANKS} ranks per call, got {len(ranks)}")
    for r in ranks:
        if isinstance(r, bool) or not isinstance(r, int) or not 0 <= r < n:
            raise ValueError(f"{what}: rank {r!r} is outside 0 ... n - 1 = {n - 1}")
    return torch.tensor(ranks, dtype=torch.int32, device=dev), (ctypes.c_uint32 * len(ranks))(*ranks)


def order_stats(score, ranks, batched=None, tile=None, return_status=False):
    """Order statistics of every segment, each selected by the whole chip (`anoddpm_select_wide`, csrc/select_wide.hip): score
    [S, ...] (`batched`; the default is `roc_auc`'s), every value of `score[s]` pooled into segment s, 1 <= n < 2^31.  `ranks`: up
    to 16 0-based positions from the top (0 is the maximum, k - 1 the k-th largest value), one table for all segments -- a list
    of ints, checked here (ValueError for a rank outside 0 ... n - 1), or an integer device tensor, which is never read on the
    host (a rank outside sets the status bit `SELECT_BAD_RANK`).  Returns a dict of device tensors, no host synchronisation, the
    same bits every run: `value` [S, Q] fp32 (selected on the bit pattern; -0.0 counts as +0.0), `above` / `equal` [S, Q] int64
    (`#{v > value}`, `#{v == value}`; `above <= rank < above + equal`), `topk` [S, Q] fp64 (the mean of the rank + 1 largest
    values as a multiset), `max` [S] fp32, `mean` [S] fp64.  Sums in `image_scores`' order: up to 2^24 values and for one rank,
    `topk`, `max` and `mean` have the bits `image_scores` returns for k = rank + 1.  Values must be finite and >= 0: the float
    entries of a segment that breaks this are NaN and its status word is non-zero (`return_status=True` returns `(dict, status)`,
    int32 [S]).  `tile`: values per workgroup, a multiple of 256 (None: the library's choice).  With a device `ranks` the call
    only allocates and launches (graph-capture-safe)."""
    if not isinstance(score, torch.Tensor):
        raise TypeError("order_stats: score must be a device tensor")
    S = score.shape[0] if _is_batched(score, batched) else 1
    if score.numel() == 0 or S < 1:
        raise ValueError("order_stats: empty score")
    sc, n, s_stride = _segments(score, S, "order_stats(score)")
    dev = sc.device
    table, host = _rank_table(ranks, n, dev, "order_stats")
    Q = table.numel()
    tile = 0 if tile is None else int(tile)
    nbytes = lib().anoddpm_select_wide_workspace_bytes(n, Q, tile)
    if nbytes < 0:
        raise ValueError(f"order_stats: segment length {n} is outside [1, 2^31), or tile {tile} is not a multiple of 256")
    ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=dev)
    out = {"value": torch.empty((S, Q), dtype=torch.float32, device=dev), "above": torch.empty((S, Q), dtype=torch.int64, device=dev),
           "equal": torch.empty((S, Q), dtype=torch.int64, device=dev), "topk": torch.empty((S, Q), dtype=torch.float64, device=dev),
           "max": torch.empty((S,), dtype=torch.float32, device=dev), "mean": torch.empty((S,), dtype=torch.float64, device=dev)}
    status = torch.empty((S,), dtype=torch.int32, device=dev)
    a = SelectArgs()
    a.src, a.ranks, a.ranks_host = sc.data_ptr(), table.data_ptr(), (ctypes.addressof(host) if host is not None else None)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.value, a.above, a.equal, a.topk_mean = out["value"].data_ptr(), out["above"].data_ptr(), out["equal"].data_ptr(), out["topk"].data_ptr()
    a.max, a.mean, a.status = out["max"].data_ptr(), out["mean"].data_ptr(), status.data_ptr()
    a.src_stride, a.n, a.S, a.Q = s_stride, n, S, Q
    with torch.cuda.device(dev):
        check(lib().anoddpm_select_wide(ctypes.byref(a), tile, current_stream()), "select_wide")
    for key in ("value", "topk", "max", "mean"):
        bad = (status != 0).reshape((S,) + (1,) * (out[key].dim() - 1))
        out[key] = torch.where(bad, torch.full_like(out[key], float("nan")), out[key])
    return (out, status) if return_status else out


def counts_at(mask, score, thresholds, batched=None):
    """True and false positives of the predictions `score > thresholds[j]` -- strict, as the reference's `sqerr > 0.5` -- for up
    to 16 thresholds that live on the DEVICE, from one pass over the data (`anoddpm_threshold_counts`): score [S, ...] (`batched`
    as `roc_auc`), mask of the same shape or of one segment's shape (shared), `thresholds` an fp32 device tensor [T] (one table
    for all segments) or [S, T]; it is never read on the host.  Returns a dict of device tensors without a host synchronisation:
    `tp`, `fp` [S, T] and `P`, `N` [S] (the mask's positives and negatives), int64 and exact, and `status` [S] int32
    (`ROC_BAD_MASK`, `ROC_NAN`; a NaN score is never predicted)."""
    if not isinstance(score, torch.Tensor) or not isinstance(mask, torch.Tensor) or not isinstance(thresholds, torch.Tensor):
        raise TypeError("counts_at: mask, score and thresholds must be device tensors")
    S = score.shape[0] if _is_batched(score, batched) else 1
    if score.numel() == 0 or S < 1:
        raise ValueError("counts_at: empty score")
    sc, n, s_stride = _segments(score, S, "counts_at(score)")
    if mask.numel() == S * n:
        mk, _, m_stride = _segments(mask, S, "counts_at(mask)")
    elif mask.numel() == n:
        mk, _, _ = _segments(mask, 1, "counts_at(mask)")
        m_stride = 0
    else:
        raise ValueError(f"counts_at: mask of {mask.numel()} elements does not match score {tuple(score.shape)}")
    th = _f32c(thresholds, "counts_at(thresholds)")
    if th.dim() == 2 and th.shape[0] == S and S > 1:
        T, t_stride = th.shape[1], th.shape[1]
    elif th.dim() <= 1 or (th.dim() == 2 and th.shape[0] == 1):
        th = th.reshape(-1)
        T, t_stride = th.numel(), 0
    else:
        raise ValueError(f"counts_at: thresholds {tuple(thresholds.shape)} are neither [T] nor [S, T] for S = {S}")
    if not 1 <= T <= _lib.THRESHOLD_COUNTS_MAX:
        raise ValueError(f"counts_at: 1 ... {_lib.THRESHOLD_COUNTS_MAX} thresholds per call, got {T}")
    if mk.device != sc.device or th.device != sc.device:
        raise ValueError("counts_at: mask, score and thresholds are on different devices")
    dev = sc.device
    counts = torch.empty((S, T, 2), dtype=torch.int64, device=dev)
    totals = torch.empty((S, 2), dtype=torch.int64, device=dev)
    status = torch.empty((S,), dtype=torch.int32, device=dev)
    a = ThresholdCountsArgs()
    a.score, a.mask, a.thr = sc.data_ptr(), mk.data_ptr(), th.data_ptr()
    a.counts, a.totals, a.status = counts.data_ptr(), totals.data_ptr(), status.data_ptr()
    a.n, a.score_stride, a.mask_stride, a.thr_stride, a.S, a.T = n, s_stride, m_stride, t_stride, S, T
    _launch("threshold_counts", a, dev)
    return {"tp": counts[:, :, 0], "fp": counts[:, :, 1], "P": totals[:, 0], "N": totals[:, 1], "status": status}


def scores_at(mask, score, thresholds, batched=None):
    """`counts_at` and the scores that follow from its counts, as fp64 device tensors [S, T] without a host synchronisation:
    `dice` = 2 tp / (tp + fp + P) (`best_dice`'s definition, so never above it; NaN when P = 0), `precision` = tp / (tp + fp) (NaN
    when nothing is predicted), `recall` = tp / P and `fpr` = fp / N (NaN for an empty class).  All four are NaN in a segment
    whose status word is non-zero."""
    o = counts_at(mask, score, thresholds, batched)
    tp, fp = o["tp"].double(), o["fp"].double()
    P, N = o["P"].double()[:, None], o["N"].double()[:, None]
    nan = torch.full_like(tp, float("nan"))
    bad = (o["status"] != 0)[:, None]
    ratios = {"dice": ((2 * o["tp"]).double() / (o["tp"] + o["fp"] + o["P"][:, None]).double(), P == 0),
              "precision": (tp / (tp + fp), (tp + fp) == 0), "recall": (tp / P, P == 0), "fpr": (fp / N, N == 0)}
    o.update({k: torch.where(empty | bad, nan, v) for k, (v, empty) in ratios.items()})
    return o


class _PostProcessType(type):
    """`PostProcess(..., gaussian=sigma)`: the trailing keyword is taken here, by the call of the class, and `__init__` keeps the
    five positional settings and the signature it has had since it was written (callers and tests read it with `inspect`)."""

    def __call__(cls, *args, gaussian=None, **kw):
        self = super().__call__(*args, **kw)
        if gaussian is not None:
            _gauss_radius(gaussian, 4.0, "PostProcess: gaussian")
            object.__setattr__(self, "gaussian", float(gaussian))
        return self


class PostProcess(metaclass=_PostProcessType):
    """Settings of the post-processing between the squared error and its scores; immutable.  `median`: window of the median
    filter (3, 5, 7; None: off).  `erode`: erosions of the region of interest (0 ... 8; 0: used as it is).  `roi_level`: when not
    None the region of interest is `real > roi_level` (the images live in [-1, 1] with a -1 background) unless the caller hands
    one in.  `min_size` / `connectivity`: components of the thresholded map below that many pixels are dropped (0: off).  The
    defaults are the values common in published pipelines.  `gaussian` (keyword only; None: off): sigma of a Gaussian filter
    (`gaussian_filter`, truncate 4.0) applied before the median -- the smoothing of the texture protocol."""
    __slots__ = ("median", "erode", "roi_level", "min_size", "connectivity", "gaussian")

    def __init__(self, median=5, erode=3, roi_level=None, min_size=7, connectivity=1):
        if median is not None and median not in _lib.MEDIAN_SIZES:
            raise ValueError(f"PostProcess: median must be None or one of {_lib.MEDIAN_SIZES}, got {median!r}")
        if isinstance(erode, bool) or int(erode) != erode or not 0 <= erode <= _lib.ERODE_MAX:
            raise ValueError(f"PostProcess: erode must be in 0 ... {_lib.ERODE_MAX}, got {erode!r}")
        if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 0:
            raise ValueError(f"PostProcess: min_size must be an integer >= 0, got {min_size!r}")
        if connectivity not in (1, 2):
            raise ValueError(f"PostProcess: connectivity must be 1 or 2, got {connectivity!r}")
        object.__setattr__(self, "gaussian", None)                   # _PostProcessType.__call__ sets it
        for k, v in (("median", median), ("erode", int(erode)), ("roi_level", None if roi_level is None else float(roi_level)),
                     ("min_size", int(min_size)), ("connectivity", int(connectivity))):
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("PostProcess is immutable")

    def __delattr__(self, name):
        raise AttributeError("PostProcess is immutable")

    def _settings(self):
        """The settings that are spelled out: `gaussian` only when it is set, so that key, hash, repr and pickle of everything from
        before it existed are what they were."""
        return [k for k in self.__slots__ if k != "gaussian" or self.gaussian is not None]

    def _key(self):
        return tuple(getattr(self, k) for k in self._settings())

    def __eq__(self, other):
        return isinstance(other, PostProcess) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "PostProcess(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self._settings()) + ")"

    def __reduce__(self):
        if self.gaussian is None:
            return PostProcess, self._key()
        return _postprocess_from, ({k: getattr(self, k) for k in self.__slots__},)


def _postprocess_from(settings):
    return PostProcess(**settings)


def postprocess_maps(sqerr, pp, real=None, roi=None):
    """The squared-error maps `sqerr` ([S, ..., H, W]; batching as `median_filter`) after `pp`'s median filter inside the region
    of interest.  The region is `roi` (a 0 / 1 tensor) when given, else `real > pp.roi_level` when `pp.roi_level` is set, else
    everything; it has the shape of one plane (shared by all maps), one segment or sqerr, and is eroded `pp.erode` times in ONE
    launch before the ONE median launch applies it.  Returns a device tensor shaped like sqerr, no host synchronisation.  With
    `pp.median` None the region is applied by an elementwise product.  `pp.gaussian` runs first: the median and the region see
    the smoothed maps (ONE more launch)."""
    if not isinstance(pp, PostProcess):
        raise TypeError("postprocess_maps: pp must be a PostProcess")
    level = 0.0
    if roi is None and pp.roi_level is not None:
        if real is None:
            raise ValueError("postprocess_maps: PostProcess.roi_level needs the real image")
        roi, level = real, pp.roi_level
    if roi is not None:
        roi = erode_mask(roi, pp.erode, level) if pp.erode else (_f32c(roi, "postprocess_maps(roi)") > level).float()
    smoothed = pp.gaussian is not None
    if smoothed:
        sqerr = gaussian_filter(sqerr, pp.gaussian)
    if pp.median is not None:
        return median_filter(sqerr, pp.median, roi=roi)
    out = _f32c(sqerr, "postprocess_maps(sqerr)")
    if roi is None:
        return out if smoothed else out.clone()
    S, C, H, W = _planes(out, _is_batched(out, None), "postprocess_maps")
    if roi.numel() not in (H * W, C * H * W, S * C * H * W):
        raise ValueError(f"postprocess_maps: roi {tuple(roi.shape)} does not match sqerr {tuple(sqerr.shape)}")
    shape = (1, 1, H, W) if roi.numel() == H * W else ((1, C, H, W) if roi.numel() == C * H * W else (S, C, H, W))
    return (out.reshape(S, C, H, W) * roi.reshape(shape)).reshape(out.shape)


# ---------------------------------------------------------------------------------- per-region overlap (PRO / AUPRO) on the device
def component_areas(mask, connectivity=2, level=0.0, batched=None):
    """The size of every pixel's connected component of `plane > level`, per H x W plane of mask ([S, ..., H, W]; batching as
    `median_filter`, every dimension before the last two a stack of independent planes): `lab, m = scipy.ndimage.label(plane >
    level, structure); numpy.bincount(lab.ravel())[lab]` with 0 on the background.  connectivity 2: 8 neighbours (the choice of
    the PRO score), 1: 4 neighbours.  Returns `(areas, counts)`: int32 shaped like mask and int64 shaped like mask without its
    last two dimensions (the `m` of every plane), device tensors, no host synchronisation, the same bits every run."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError("component_areas: mask must be a device tensor")
    _check_connectivity(connectivity, "component_areas")
    S, C, H, W = _planes(mask, _is_batched(mask, batched), "component_areas")
    xt = _f32c(mask, "component_areas(mask)")
    dev = xt.device
    areas = torch.empty(tuple(mask.shape), dtype=torch.int32, device=dev)
    counts = torch.empty(tuple(mask.shape[:-2]), dtype=torch.int64, device=dev)
    a = ComponentAreasArgs()
    a.src, a.area, a.counts = xt.data_ptr(), areas.data_ptr(), counts.data_ptr()
    a.src_stride, a.S, a.H, a.W = H * W, S * C, H, W
    a.connectivity, a.level = int(connectivity), float(level)
    _launch("component_areas", a, dev, (lib().anoddpm_small_components_workspace_bytes(S * C, H, W), torch.int32,
                                        f"component_areas: {tuple(mask.shape)} has 2^31 pixels or more"))
    return areas, counts


# A single segment of at least this many elements is sorted and walked by the whole chip (anoddpm_pro_auc_wide); the outputs have
# the same bits.  65536 is the smallest measured power of two from which, at every larger measured size, the slowest wide repetition
# was below the fastest one-workgroup repetition (profiles/pro_wide_ab.txt); 2147483648 switches the path off.
PRO_WIDE_MIN_N = int(os.environ.get("ANODDPM_PRO_WIDE_MIN_N", "") or 65536)


def _pro_call(a, out, S, n, dev, wide, tile):
    """The launch of a filled `ProArgs`: `anoddpm_pro_auc_wide` (`tile` elements per workgroup; None: the library's choice) or
    `anoddpm_pro_auc`, with the workspace of either.  Sets `out["path"]`."""
    out["path"] = "wide" if wide else "workgroup"
    if wide:
        tile = 0 if tile is None else int(tile)
        nbytes = lib().anoddpm_pro_wide_workspace_bytes(S, n, tile)
        if nbytes < 0:
            raise ValueError(f"pro: segment length {n} is outside [1, 2^31), or tile {tile} is not a multiple of 256 that cuts it into "
                             f"at most {_lib.ROC_WIDE_MAX_TILES} tiles")
        ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        with torch.cuda.device(dev):
            check(lib().anoddpm_pro_auc_wide(ctypes.byref(a), tile, current_stream()), "pro_auc_wide")
        return out
    _launch("pro_auc", a, dev, (lib().anoddpm_pro_workspace_bytes(S, n), torch.float64, f"pro: segment length {n} is outside [1, 2^31)"))
    return out


def _pro_launch(mask, score, limit, connectivity, batched, curve, wide=None, tile=None):
    """One `anoddpm_component_areas` run on the mask and one `anoddpm_pro_auc` launch.  score: [S, ..., H, W] when batched, else
    one segment [..., H, W]; every plane of `score[s]` belongs to segment s.  mask: like score, or the shape of one segment (its
    areas are computed once and shared).  `wide`: sort and walk the segments one after another with the whole chip
    (`anoddpm_pro_auc_wide`, `tile` elements per workgroup; None: the library's choice); None takes that path for one segment of
    at least `PRO_WIDE_MIN_N` elements.  Both paths write the same bits; `path` says which one ran ("wide" / "workgroup").
    Returns a dict of device tensors; nothing is copied to the host."""
    if not isinstance(score, torch.Tensor) or not isinstance(mask, torch.Tensor):
        raise TypeError("pro: mask and score must be device tensors")
    if isinstance(limit, bool) or not 0.0 < float(limit) <= 1.0:
        raise ValueError(f"pro: limit must be in (0, 1], got {limit!r}")
    _check_connectivity(connectivity, "pro")
    S, C, H, W = _planes(score, batched, "pro")
    n = C * H * W
    if mask.numel() not in (n, S * n) or tuple(mask.shape[-2:]) != (H, W):
        raise ValueError(f"pro: mask {tuple(mask.shape)} is neither the shape of score {tuple(score.shape)} nor of one segment")
    sc, n, s_stride = _segments(score, S, "pro(score)")
    shared = mask.numel() == n and S > 1
    mk = _f32c(mask, "pro(mask)")
    if mk.device != sc.device:
        raise ValueError("pro: mask and score are on different devices")
    dev = sc.device
    areas, regions = component_areas(mk.reshape(-1, H, W), connectivity, batched=True)
    out = {"aupro": torch.empty((S,), dtype=torch.float64, device=dev),
           "counts": torch.empty((S, 4), dtype=torch.int64, device=dev),
           "status": torch.empty((S,), dtype=torch.int32, device=dev), "n": n}
    a = ProArgs()
    a.score, a.area, a.region_counts, a.mask = sc.data_ptr(), areas.data_ptr(), regions.data_ptr(), mk.data_ptr()
    a.aupro, a.counts, a.status = out["aupro"].data_ptr(), out["counts"].data_ptr(), out["status"].data_ptr()
    a.score_stride, a.area_stride, a.mask_stride = s_stride, (0 if shared else n), (0 if shared else n)
    a.limit, a.S, a.planes_per_segment, a.H, a.W = float(limit), S, C, H, W
    if curve:                                                        # a segment has at most n distinct scores
        a.curve_fps, a.curve_pro, a.curve_thr, a.curve_len, a.curve_cap = _curve_buffers(out, "pro", torch.float64, S, n, dev)
    if wide is None:
        wide = S == 1 and n >= PRO_WIDE_MIN_N
    return _pro_call(a, out, S, n, dev, wide, tile)


def aupro(mask, score, limit=0.3, connectivity=2, batched=None, return_status=False):
    """Area under the per-region overlap curve up to the false-positive rate `limit`, divided by `limit` (Bergmann et al., IJCV
    2021), of every segment: score `[S, ..., H, W]` (`batched`; the default is `roc_auc`'s), all planes of `score[s]` one segment
    -- several planes pool a data set into one curve -- and mask of the same shape or of one segment's shape (shared by all
    segments).  A region is a connected component of one mask plane (`connectivity` 2: 8 neighbours); for every distinct score v
    the curve holds `FPR = fps / N` over the pixels outside every region and `PRO` = the mean over the regions of the fraction
    of the region with `score >= v`.  Returns an `[S]` fp64 device tensor without a host synchronisation, the same bits every
    run.  NaN where the mask has no region or no background, and where the inputs break the precondition of `roc_auc`
    (`return_status=True` also returns the [S] int32 status words)."""
    o = _pro_launch(mask, score, limit, connectivity, _is_batched(score, batched), curve=False)
    val = _nan_where_status(o, "aupro")
    return (val, o["status"]) if return_status else val


def pro_points(mask, score, limit=0.3, connectivity=2, batched=None):
    """Every point of the per-region overlap curve, per segment (arguments as `aupro`): one per distinct score, from the highest
    threshold down and without the `(0, 0)` point in front.  A list of dicts with `fps` (int64 counts; `FPR = fps / N`), `pro`
    (fp64), `thresholds` (fp32), `K` (regions), `N`, `P` (pixels outside / inside the regions) and `aupro` (Python numbers).
    Copies to the host; raises ValueError for inputs outside the precondition."""
    return _pro_points_of(_pro_launch(mask, score, limit, connectivity, _is_batched(score, batched), curve=True))


def _pro_points_of(o):
    """The host form of a `_pro_launch` dict with curve outputs: the list `pro_points` returns."""
    status, lens, counts, val = o["status"].cpu(), o["len"].cpu(), o["counts"].cpu(), o["aupro"].cpu()
    _raise_on_status("pro", status)
    return [dict(_curve_arrays(o, ("fps", "pro", "thresholds"), s, L), K=int(counts[s, 0]), N=int(counts[s, 1]),
                 P=int(counts[s, 2]), aupro=float(val[s])) for s, L in enumerate(lens.tolist())]


# ---------------------------------------------------------------------------------- distance transform and boundary distances
def _surface_workspace(S, H, W, what, share=1):
    """`_launch`'s workspace of the two entry points of csrc/surface.hip: `1 / share` of what `anoddpm_surface_workspace_bytes` answers."""
    return (lib().anoddpm_surface_workspace_bytes(S, H, W) // share, torch.int32,
            f"{what}: {S} planes of {H} x {W} are too large: (H-1)^2 + (W-1)^2, H*W and 2 * planes * H*W must stay below 2^31")


def distance_transform(x, level=0.0, squared=False, batched=None):
    """`scipy.ndimage.distance_transform_edt(plane > level)` of every H x W plane of x ([..., H, W]: every dimension before the
    last two a stack of independent planes, so `batched` changes nothing but is accepted as by the sibling functions; NaN is
    background): an fp64 device tensor shaped like x, bit for bit scipy's wherever the plane has a background pixel, without a
    host synchronisation.  `squared=True`: the exact int32 squared distance instead.  A plane without a background pixel has no
    defined answer: +inf (squared: -1) everywhere in it."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("distance_transform: x must be a device tensor")
    S, C, H, W = _planes(x, False, "distance_transform")
    xt = _f32c(x, "distance_transform(x)")
    dev = xt.device
    sq = torch.empty(tuple(x.shape), dtype=torch.int32, device=dev)
    dist = None if squared else torch.empty(tuple(x.shape), dtype=torch.float64, device=dev)
    a = DistanceArgs()
    a.src, a.sq, a.dist = xt.data_ptr(), sq.data_ptr(), (None if squared else dist.data_ptr())
    a.src_stride, a.S, a.H, a.W, a.level = H * W, C, H, W, float(level)
    _launch("distance_transform", a, dev, _surface_workspace(C, H, W, "distance_transform", share=4))    # 4 * S * H * W bytes: a quarter
    return sq if squared else dist


def surface_distance(pred, ref, level=0.0, return_status=False):
    """Boundary distances of every H x W plane of pred ([..., H, W]) against the plane of ref at the same place, or against ONE
    `[H, W]` reference shared by all (its border is computed once).  With `m = plane > level`, the border of m is `m &
    ~scipy.ndimage.binary_erosion(m)` (4 neighbours, the image edge counts as background), `d_pr` the distances from the pixels of
    pred's border to the nearest pixel of ref's border and `d_rp` the reverse, in pixels.  Returns a dict of device tensors shaped
    like pred without its last two dimensions (plus the trailing axis named), no host synchronisation, the same bits every run:
    `hd` (Hausdorff distance), `hd95` (the 95th percentile of `d_pr` and `d_rp` pooled: medpy's `hd95`), `assd` (the mean of the
    two directions' means), all fp64; `p95` [..., 3] (of `d_pr`, of `d_rp`, pooled), `mean` [..., 2], `max2` [..., 2] (int32, the
    largest squared distances), `counts` [..., 2] (int32 border sizes) and `status` (int32: bit 0 pred's border is empty, bit 1
    ref's).  Where the status is non-zero every fp64 value is NaN and `max2` is -1.  `return_status=True` returns `(dict, status)`."""
    if not isinstance(pred, torch.Tensor) or not isinstance(ref, torch.Tensor):
        raise TypeError("surface_distance: pred and ref must be device tensors")
    S, C, H, W = _planes(pred, False, "surface_distance")
    if tuple(ref.shape) != tuple(pred.shape) and tuple(ref.shape) != (H, W):
        raise ValueError(f"surface_distance: ref {tuple(ref.shape)} is neither the shape of pred {tuple(pred.shape)} nor one [H, W] plane")
    pt = _f32c(pred, "surface_distance(pred)")
    rt = _f32c(ref, "surface_distance(ref)")
    if rt.device != pt.device:
        raise ValueError("surface_distance: pred and ref are on different devices")
    dev = pt.device
    lead = tuple(pred.shape[:-2])
    out = {"counts": torch.empty(lead + (2,), dtype=torch.int32, device=dev), "max2": torch.empty(lead + (2,), dtype=torch.int32, device=dev),
           "mean": torch.empty(lead + (2,), dtype=torch.float64, device=dev), "p95": torch.empty(lead + (3,), dtype=torch.float64, device=dev),
           "status": torch.empty(lead, dtype=torch.int32, device=dev)}
    a = SurfaceArgs()
    a.pred, a.ref = pt.data_ptr(), rt.data_ptr()
    for k in ("counts", "max2", "mean", "p95", "status"):
        setattr(a, k, out[k].data_ptr())
    a.pred_stride, a.ref_stride = H * W, (H * W if rt.numel() == C * H * W and C > 1 else 0)
    a.S, a.H, a.W, a.level = C, H, W, float(level)
    _launch("surface_distance", a, dev, _surface_workspace(C, H, W, "surface_distance"))
    out["hd"] = torch.sqrt(out["max2"].max(dim=-1).values.double())              # max2 is -1 where the status is set: NaN
    out["hd95"] = out["p95"][..., 2]
    out["assd"] = (out["mean"][..., 0] + out["mean"][..., 1]) / 2
    return (out, out["status"]) if return_status else out


def _valid_mean(values, status):
    """Mean of `values` over the entries of the last axis whose status is 0 (NaN when there is none), and their number."""
    ok = status == 0
    n = ok.sum(dim=-1)
    total = torch.where(ok, values, torch.zeros_like(values)).sum(dim=-1)
    return torch.where(n > 0, total / n.clamp(min=1), torch.full_like(total, float("nan"))), n


def score_maps(real, mean, sqerr, pred, mask, postprocess=None, roi=None, pro_limit=None, surface=False, threshold=0.5, pred_pp=False,
               image_top=None):
    """Every score of R stacks of anomaly maps, one launch per step whatever R is.  real: [B, C, H, W]; mean (the averaged
    reconstructions), sqerr and pred: [R, B, C, H, W], `pred > 0` being the thresholded map (the 0 / 1 `pred` and the -1 / 1
    `thr_img` of `anomaly_maps` both do); mask: like real, or None.  Setting r pools its B images into one curve, as
    detection.py:230-231 does.  Returns a dict of device tensors with a leading R axis; never synchronises, never copies to the
    host, and the same bits in row r whatever the other rows hold.  A score that cannot be computed has no key:

    `ssim` [R, B] (7 x 7 uniform window, data_range 2.0; `real[0]` is read in place by every setting when B == 1) -- for
    non-empty `[B, C, H, W]` images of at least the window's size.
    With a mask: `auc`, `ap`, `best_dice`, `best_threshold`, `auc_status` [R] (`curve_scores` of sqerr).
    With `postprocess` (a `PostProcess`; `roi`: see `postprocess_maps`): `sqerr_pp` like sqerr -- one erosion and one median
    launch -- with a mask `auc_pp`, `ap_pp`, `best_dice_pp`, `best_threshold_pp`, `auc_pp_status` [R] of it, and, when `pred_pp`
    or `surface` asks for it, `pred_pp`: `sqerr_pp > threshold` without its components below `postprocess.min_size` pixels.
    With `pro_limit` and a mask: `aupro` (and `aupro_pp`) [R] as `aupro(..., connectivity=2)`, `aupro_regions` (int64) and
    `aupro_status` [R] of the raw maps -- one component run on the mask and one PRO launch.
    With `surface` and a mask: `hd`, `hd95`, `assd` (and their `_pp` forms) [R]: `surface_distance` of every plane of pred (and
    pred_pp) against its mask plane in one call (a mask of one plane is shared), each the mean over the setting's planes whose
    status is 0, NaN when there is none; `surface_status` [R, B * C], the planes' status words for pred.
    With `image_top` (`image_scores`' `top`; no mask needed): `image_max`, `image_mean`, `image_topk` (and their `_pp` forms) [R, B],
    the scores of every image's sqerr (all its channels pooled), and `image_status` [R, B] of the raw maps -- ONE launch over all
    R * B images (2 R B with `postprocess`)."""
    R, have_mask = sqerr.shape[0], mask is not None
    out, stacks = {}, [("", sqerr)]

    def curves(sfx, sq):
        o = curve_scores(mask, sq.reshape(R, -1), batched=True)
        out.update({k + sfx: o[k] for k in ("auc", "ap", "best_dice", "best_threshold")})
        out["auc" + sfx + "_status"] = o["status"]

    if have_mask:
        curves("", sqerr)
    if real.dim() == 4 and min(real.shape[-2:]) >= 7 and real.numel() > 0:
        B = real.shape[0]
        out["ssim"] = ssim(real[0] if B == 1 else real.unsqueeze(0).expand_as(mean), mean).reshape(R, B)
    if postprocess is not None:
        out["sqerr_pp"] = postprocess_maps(sqerr, postprocess, real=real, roi=roi)
        stacks.append(("_pp", out["sqerr_pp"]))
        if have_mask:
            curves("_pp", out["sqerr_pp"])
    if have_mask and pro_limit is not None:
        o = _pro_launch(mask, torch.cat([sq for _, sq in stacks]), pro_limit, 2, batched=True, curve=False)
        out["aupro_regions"], out["aupro_status"] = o["counts"][:R, 0], o["status"][:R]
        for (sfx, _), val in zip(stacks, _nan_where_status(o, "aupro").reshape(-1, R)):
            out["aupro" + sfx] = val
    if image_top is not None:
        B = sqerr.shape[1]
        o, status = image_scores(torch.cat([sq for _, sq in stacks]).reshape(len(stacks) * R * B, -1), image_top, batched=True, return_status=True)
        out["image_status"] = status[:R * B].reshape(R, B)
        for k in ("max", "mean", "topk"):
            for (sfx, _), val in zip(stacks, o[k].reshape(-1, R, B)):
                out["image_" + k + sfx] = val
    preds = [pred]
    if postprocess is not None and (pred_pp or (surface and have_mask)):
        out["pred_pp"] = _small_components(out["sqerr_pp"], float(threshold), postprocess.min_size, postprocess.connectivity)[0]
        preds.append(out["pred_pp"])
    if have_mask and surface:
        H, W = pred.shape[-2:]
        planes = torch.cat(preds).reshape(len(preds) * R, -1, H, W)
        ref = mask.reshape(-1, H, W)
        o = surface_distance(planes, ref[0] if ref.shape[0] == 1 else ref.unsqueeze(0).expand(planes.shape))
        out["surface_status"] = o["status"][:R]
        for k in ("hd", "hd95", "assd"):
            for (sfx, _), val in zip(stacks, _valid_mean(o[k], o["status"])[0].reshape(-1, R)):
                out[k + sfx] = val
    return out


NAN = float("nan")
# anomaly_metrics*: (key, key of score_maps, value when score_maps has none, options that bring the key)
_METRIC_KEYS = (("AUC", "auc", NAN, ()), ("AP", "ap", NAN, ()), ("best_dice", "best_dice", NAN, ()), ("best_threshold", "best_threshold", NAN, ()),
                ("AUC_status", "auc_status", 0, ()), ("SSIM", "ssim", NAN, ()),
                ("AUC_pp", "auc_pp", NAN, ("pp",)), ("AP_pp", "ap_pp", NAN, ("pp",)), ("best_dice_pp", "best_dice_pp", NAN, ("pp",)),
                ("best_threshold_pp", "best_threshold_pp", NAN, ("pp",)), ("AUC_pp_status", "auc_pp_status", 0, ("pp",)),
                ("AUPRO", "aupro", NAN, ("pro",)), ("AUPRO_regions", "aupro_regions", 0, ("pro",)), ("AUPRO_status", "aupro_status", 0, ("pro",)),
                ("AUPRO_pp", "aupro_pp", NAN, ("pro", "pp")),
                ("HD", "hd", NAN, ("surface",)), ("HD95", "hd95", NAN, ("surface",)), ("ASSD", "assd", NAN, ("surface",)),
                ("HD_pp", "hd_pp", NAN, ("surface", "pp")), ("HD95_pp", "hd95_pp", NAN, ("surface", "pp")), ("ASSD_pp", "assd_pp", NAN, ("surface", "pp")),
                ("image_max", "image_max", [], ("image",)), ("image_mean", "image_mean", [], ("image",)), ("image_topk", "image_topk", [], ("image",)),
                ("image_status", "image_status", [], ("image",)),
                ("image_max_pp", "image_max_pp", [], ("image", "pp")), ("image_mean_pp", "image_mean_pp", [], ("image", "pp")),
                ("image_topk_pp", "image_topk_pp", [], ("image", "pp")))               # a list: one entry per image of the batch


def _to_host(tensors):
    """The device tensors of a dict on the host from ONE copy, as fp64 (counts, status words and fp32 values are exact in it)."""
    flat = torch.cat([t.reshape(-1).double() for t in tensors.values()]).cpu()
    parts = flat.split([t.numel() for t in tensors.values()])
    return {k: p.reshape(t.shape) for (k, t), p in zip(tensors.items(), parts)}


def _metrics(real, recon, mask, threshold, postprocess, roi, pro_limit=None, surface=False, image_top=None):
    """`anomaly_metrics`, `anomaly_metrics_pro` and `anomaly_metrics_surface`: `anomaly_maps`, `score_maps` of the one stack, one
    copy of every number to the host, `_METRIC_KEYS`."""
    maps, counts = anomaly_maps(real, recon, mask, threshold)
    o = score_maps(real, maps["mean"][None], maps["sqerr"][None], maps["pred"][None], mask, postprocess=postprocess, roi=roi,
                   pro_limit=pro_limit, surface=surface, threshold=threshold, pred_pp=True, image_top=image_top)
    dev = {src: o[src][0] for _, src, _, _ in _METRIC_KEYS if src in o}
    dev["counts"] = counts
    if "ssim" in o:
        dev["ssim"] = o["ssim"].mean()
    if "surface_status" in o:
        dev["surface_status"] = o["surface_status"][0]
    if postprocess is not None:
        maps["sqerr_pp"], maps["pred_pp"] = o["sqerr_pp"][0], o["pred_pp"][0]
        dev["counts_pp"] = anomaly_maps(torch.zeros_like(maps["pred_pp"]), maps["pred_pp"], mask, threshold=0.5, want=())[1]    # (pred - 0)^2 > 0.5 is pred itself
    h = _to_host(dev)
    c = h["counts"]
    r = {k: float(v) for k, v in _ratios(c).items() if k != "dice_per_image"}
    mse = float(c[:, 9].sum()) / real.numel()
    r["mse"] = mse
    r["PSNR"] = float(20.0 * torch.log10(torch.tensor(float(c[:, 10].max())) / torch.sqrt(torch.tensor(mse)))) if mse > 0 else float("inf")
    on = {"pp": postprocess is not None, "pro": pro_limit is not None, "surface": surface, "image": image_top is not None}
    for key, src, absent, options in _METRIC_KEYS:
        if all(on[k] for k in options):
            if isinstance(absent, list):
                r[key] = [int(v) if key.endswith("status") else v for v in h[src].tolist()] if src in h else []
            else:
                r[key] = type(absent)(h[src]) if src in h else absent
    for sfx in ("", "_pp") if on["pp"] else ("",):
        if r["best_dice" + sfx] != r["best_dice" + sfx]:
            r["best_threshold" + sfx] = NAN                          # no positive: no threshold is better than another
    if surface:
        status = [int(st) for st in h["surface_status"].tolist()] if "surface_status" in h else []
        r["HD95_valid"], r["surface_status"] = sum(st == 0 for st in status), 0
        for st in status:
            r["surface_status"] |= st
    if on["pp"]:
        ratios = _ratios(h["counts_pp"])
        for key in ("dice", "precision", "recall"):
            r[key + "_pp"] = float(ratios[key])
    r["maps"] = maps
    return r


def anomaly_metrics(real, recon, mask, threshold=0.5, postprocess=None, roi=None):
    """dice / IoU / precision / recall / FPR / mse / PSNR of detection.py:229-250 from one launch, the AUC of
    detection.py:230-231 (the whole batch flattened into one curve, evaluation.py:81) from a second one -- which also gives `AP`
    (average precision), `best_dice` and `best_threshold` (the largest Dice over all thresholds and the highest threshold that
    reaches it; NaN like `AUC`, and NaN when the mask has no positive) of that same flattened curve -- and the SSIM of
    detection.py:241-246 (mean over the batch of the per-image SSIM of `real` against the `mean` map, i.e. the reconstruction
    averaged over `navg`) from a third.  Returns a dict of Python floats plus the maps (device tensors).  `AUC` is NaN when a
    class is empty or when `AUC_status` (the status word of the ROC kernel) is non-zero; without a mask there is no AUC (NaN,
    status 0).  `SSIM` is NaN when the inputs are not `[B, C, H, W]` or are smaller than the 7 x 7 window.

    `postprocess` (a `PostProcess`; `roi`: its region of interest, see `postprocess_maps`) ADDS, and changes nothing else:
    `AUC_pp`, `AP_pp`, `best_dice_pp`, `best_threshold_pp`, `AUC_pp_status` -- the same launch on the filtered map
    `maps["sqerr_pp"]` -- and `dice_pp`, `precision_pp`, `recall_pp`: the filtered map cut at `threshold`, without its
    components below `postprocess.min_size` pixels (`maps["pred_pp"]`), counted by the same pass as `dice` / `precision` /
    `recall`.  The inputs must be `[..., H, W]` images then."""
    return _metrics(real, recon, mask, threshold, postprocess, roi)


def anomaly_metrics_pro(real, recon, mask, threshold=0.5, postprocess=None, roi=None, pro_limit=0.3):
    """`anomaly_metrics` with the per-region overlap score beside its results -- a function of its own, so that `anomaly_metrics`
    keeps its signature, its keys and its launches.  `pro_limit` (a false-positive rate in (0, 1], 0.3 in the literature) ADDS
    `AUPRO` (`aupro` of the whole batch pooled into one curve, as `AUC` is), `AUPRO_regions` (the mask's connected regions, 8
    neighbours) and `AUPRO_status`, and with `postprocess` also `AUPRO_pp` on the filtered map, all from one component run on
    the mask and one PRO launch; NaN as `AUC`.  The inputs must be `[..., H, W]` images.  `pro_limit=None`: exactly
    `anomaly_metrics(...)`, no key and no launch more."""
    return _metrics(real, recon, mask, threshold, postprocess, roi, pro_limit=pro_limit)


def anomaly_metrics_surface(real, recon, mask, threshold=0.5, postprocess=None, roi=None):
    """`anomaly_metrics` with the boundary distances beside its results -- a function of its own, as `anomaly_metrics_pro` is, so
    that `anomaly_metrics` keeps its signature, its keys and its launches.  ADDS `HD`, `HD95`, `ASSD`: `surface_distance` of the
    thresholded map `maps["pred"]` against the mask, plane by plane, each the mean over the planes whose status is 0 (both borders
    exist; NaN when there is none), `HD95_valid`, the number of those planes, and `surface_status`, the OR of the planes' status
    words; with `postprocess` also `HD_pp`, `HD95_pp`, `ASSD_pp` from `maps["pred_pp"]`, from the same launch.  Without a mask:
    NaN, 0, 0.  The inputs must be `[..., H, W]` images."""
    return _metrics(real, recon, mask, threshold, postprocess, roi, surface=True)


def anomaly_metrics_image(real, recon, mask, threshold=0.5, postprocess=None, roi=None, image_top=0.01):
    """`anomaly_metrics` with the image-level scores beside its results -- a function of its own, as `anomaly_metrics_pro` is, so
    that `anomaly_metrics` keeps its signature, its keys and its launches.  `image_top` (`image_scores`' `top`: an int k or a
    fraction in (0, 1]) ADDS `image_max`, `image_mean`, `image_topk` -- lists of B Python floats, the scores of every image's
    squared-error map, NaN where `image_status` (B ints) is non-zero -- and with `postprocess` their `_pp` forms on the filtered
    map, all from one launch.  `image_top=None`: exactly `anomaly_metrics(...)`, no key and no launch more."""
    return _metrics(real, recon, mask, threshold, postprocess, roi, image_top=image_top)


_AT_KEYS = ("dice", "precision", "recall", "fpr")


def anomaly_metrics_at(real, recon, mask, thresholds, postprocess=None, roi=None):
    """`anomaly_metrics` with the scores at calibrated operating thresholds beside its results -- a function of its own, as
    `anomaly_metrics_pro` is.  `thresholds`: an fp32 device tensor [T] (`HealthyPool.thresholds`), never read on the host.  ADDS
    `dice_at`, `precision_at`, `recall_at`, `fpr_at` -- fp64 device tensors [T], `scores_at` of `maps["sqerr"]` with the whole
    batch pooled into one segment, as `AUC` pools it -- and `tp_at`, `fp_at` (int64 [T]), the counts behind them; with
    `postprocess` also their `_pp` forms on `maps["sqerr_pp"]` (the filtered map cut at every threshold; small components are not
    removed, that step takes one host threshold).  Without a mask every pixel is a negative: only `fpr_at` is a number."""
    r = _metrics(real, recon, mask, 0.5, postprocess, roi)
    for sfx in ("", "_pp") if postprocess is not None else ("",):
        sq = r["maps"]["sqerr" + sfx]
        mk = mask if mask is not None else torch.zeros_like(sq)
        o = scores_at(mk.reshape(1, -1), sq.reshape(1, -1), thresholds.reshape(-1), batched=True)
        for k in _AT_KEYS + ("tp", "fp"):
            r[k + "_at" + sfx] = o[k][0]
    return r


# ---------------------------------------------------------------------------------- volume-wise post-processing (csrc/postproc3d.hip)
def _volumes(x, batched, what, name):
    """Shape bookkeeping of [..., D, H, W]: (V, D, H, W), every dimension before the last three a stack of independent volumes.  A
    3-D tensor is one volume; `batched=True` asks for at least one leading dimension."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a device tensor")
    if x.dim() < 3 or (batched and x.dim() < 4):
        raise ValueError(f"{what}: a volume is [..., D, H, W], got {name} of shape {tuple(x.shape)}" + (" as a batch" if batched else ""))
    if x.numel() == 0:
        raise ValueError(f"{what}: empty {name} {tuple(x.shape)}")
    D, H, W = x.shape[-3:]
    return x.numel() // (D * H * W), D, H, W


def median_filter3d(score, size=5, roi=None, batched=None, return_status=False):
    """`scipy.ndimage.median_filter(vol, size=size)` (reflect border on all three axes) of every D x H x W volume of score:
    [..., D, H, W] -- a 3-D tensor is one volume, four or more dimensions a batch of volumes (`batched=False`: the leading
    dimensions are still a stack of independent volumes; `batched=True` refuses a 3-D tensor).  size 3 or 5, at most min(H, W);
    any D >= 1 (the border is reflected as often as the window asks).  `roi`: a 0 / 1 tensor shaped like one plane (shared by
    every slice), one volume (shared by the batch) or score; the result is +0.0 where it is 0 (the filter itself sees the
    unmasked volume).  Returns a device tensor shaped like score, bit for bit scipy's, without a host synchronisation.  Scores
    must be finite and >= 0 as for `median_filter`: a volume that is not gets a non-zero status word (`return_status=True` also
    returns them, int32, shaped like score without its last three dimensions) and an unspecified result."""
    V, D, H, W = _volumes(score, batched, "median_filter3d", "score")
    if size not in _lib.MEDIAN3D_SIZES:
        raise ValueError(f"median_filter3d: size must be one of {_lib.MEDIAN3D_SIZES}, got {size!r}")
    if min(H, W) < size:
        raise ValueError(f"median_filter3d: window of {size} exceeds the {H} x {W} slices")
    sc, _, s_stride = _segments(score, V, "median_filter3d(score)")
    dev = sc.device
    a = _lib.Median3dArgs()
    if roi is not None:
        if not isinstance(roi, torch.Tensor):
            raise TypeError("median_filter3d: roi must be a device tensor")
        if roi.numel() == H * W:
            a.roi_slice_stride, a.roi_stride = 0, 0
        elif roi.numel() == D * H * W:
            a.roi_slice_stride, a.roi_stride = H * W, 0
        elif roi.numel() == V * D * H * W:
            a.roi_slice_stride, a.roi_stride = H * W, D * H * W
        else:
            raise ValueError(f"median_filter3d: roi {tuple(roi.shape)} is neither a plane, a volume nor the shape of score {tuple(score.shape)}")
        rt = _f32c(roi, "median_filter3d(roi)")
        if rt.device != dev:
            raise ValueError("median_filter3d: roi and score are on different devices")
        a.roi = rt.data_ptr()
    out = torch.empty(tuple(score.shape), dtype=torch.float32, device=dev)
    status = torch.empty(tuple(score.shape[:-3]), dtype=torch.int32, device=dev)
    a.src, a.dst, a.status, a.src_stride = sc.data_ptr(), out.data_ptr(), status.data_ptr(), s_stride
    a.S, a.D, a.H, a.W, a.k = V, D, H, W, int(size)
    _launch("median3d", a, dev)
    return (out, status) if return_status else out


def erode_mask3d(x, iterations=3, level=0.0):
    """`scipy.ndimage.binary_erosion(vol > level, iterations=iterations)` (the 6-neighbour cross, zero outside the volume) of
    every D x H x W volume of x ([..., D, H, W]); 1 ... 8 iterations.  Returns an fp32 0 / 1 device tensor shaped like x, no host
    synchronisation.  With the default level a 0 / 1 mask is eroded; with `level` a volume is thresholded and eroded at once."""
    V, D, H, W = _volumes(x, None, "erode_mask3d", "x")
    if isinstance(iterations, bool) or int(iterations) != iterations or not 1 <= iterations <= _lib.ERODE_MAX:
        raise ValueError(f"erode_mask3d: iterations must be in 1 ... {_lib.ERODE_MAX}, got {iterations!r}")
    xt, _, stride = _segments(x, V, "erode_mask3d(x)")
    out = torch.empty(tuple(x.shape), dtype=torch.float32, device=xt.device)
    a = _lib.Erode3dArgs()
    a.src, a.dst, a.src_stride = xt.data_ptr(), out.data_ptr(), stride
    a.S, a.D, a.H, a.W, a.n, a.level = V, D, H, W, int(iterations), float(level)
    _launch("erode3d", a, xt.device)
    return out


def _check_connectivity3d(connectivity, what):
    if connectivity not in (1, 2, 3):
        raise ValueError(f"{what}: connectivity must be 1 (6 neighbours), 2 (18) or 3 (26), got {connectivity!r}")


def _small_components3d(x, level, min_size, connectivity):
    """One `anoddpm_small_components3d` run on the volumes of x > level: (fp32 0 / 1 map shaped like x, int64 counts [..., 2])."""
    V, D, H, W = _volumes(x, None, "remove_small_components3d", "pred")
    if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 0:
        raise ValueError(f"remove_small_components3d: min_size must be an integer >= 0, got {min_size!r}")
    _check_connectivity3d(connectivity, "remove_small_components3d")
    xt, _, stride = _segments(x, V, "remove_small_components3d(pred)")
    dev = xt.device
    out = torch.empty(tuple(x.shape), dtype=torch.float32, device=dev)
    counts = torch.empty(tuple(x.shape[:-3]) + (2,), dtype=torch.int64, device=dev)
    a = _lib.Components3dArgs()
    a.src, a.dst, a.counts = xt.data_ptr(), out.data_ptr(), counts.data_ptr()
    a.src_stride, a.S, a.D, a.H, a.W = stride, V, D, H, W
    a.min_size, a.connectivity, a.level = int(min_size), int(connectivity), float(level)
    _launch("small_components3d", a, dev, (lib().anoddpm_components3d_workspace_bytes(V, D, H, W), torch.int32,
                                           f"remove_small_components3d: {tuple(x.shape)} has 2^31 voxels or more"))
    return out, counts


def remove_small_components3d(pred, min_size=7, connectivity=1, return_counts=False):
    """The binary prediction `pred` ([..., D, H, W], fp32 0 / 1) without its connected components of fewer than `min_size`
    voxels: `lab, _ = scipy.ndimage.label(vol, generate_binary_structure(3, connectivity)); keep =
    numpy.bincount(lab.ravel()) >= min_size; keep[0] = False; keep[lab]` per volume.  connectivity 1: 6 neighbours (label's
    default), 2: 18, 3: 26.  Returns an fp32 0 / 1 device tensor shaped like pred, with `return_counts=True` also int64
    `[..., 2]`: components found and components kept per volume.  No host synchronisation; the same bits every run."""
    out, counts = _small_components3d(pred, 0.0, min_size, connectivity)
    return (out, counts) if return_counts else out


def component_areas3d(mask, connectivity=3, level=0.0, batched=None):
    """The size of every voxel's connected component of `vol > level`, per D x H x W volume of mask ([..., D, H, W]; batching as
    `median_filter3d`): `lab, m = scipy.ndimage.label(vol > level, generate_binary_structure(3, connectivity));
    numpy.bincount(lab.ravel())[lab]` with 0 on the background.  connectivity 3: 26 neighbours (the 3-D counterpart of the PRO
    score's 8), 2: 18, 1: 6.  Returns `(areas, counts)`: int32 shaped like mask and int64 shaped like mask without its last three
    dimensions (the `m` of every volume), device tensors, no host synchronisation, the same bits every run."""
    V, D, H, W = _volumes(mask, batched, "component_areas3d", "mask")
    _check_connectivity3d(connectivity, "component_areas3d")
    xt, _, stride = _segments(mask, V, "component_areas3d(mask)")
    dev = xt.device
    areas = torch.empty(tuple(mask.shape), dtype=torch.int32, device=dev)
    counts = torch.empty(tuple(mask.shape[:-3]), dtype=torch.int64, device=dev)
    a = _lib.ComponentAreas3dArgs()
    a.src, a.area, a.counts = xt.data_ptr(), areas.data_ptr(), counts.data_ptr()
    a.src_stride, a.S, a.D, a.H, a.W = stride, V, D, H, W
    a.connectivity, a.level = int(connectivity), float(level)
    _launch("component_areas3d", a, dev, (lib().anoddpm_components3d_workspace_bytes(V, D, H, W), torch.int32,
                                          f"component_areas3d: {tuple(mask.shape)} has 2^31 voxels or more"))
    return areas, counts


# ---------------------------------------------------------------------------------- smoothing of whole volumes (csrc/gauss3d.hip)
def _gauss3d_radii(sigma, truncate, what):
    """`sigma`: one number or three in (z, y, x) order, each finite and >= 0; `truncate`: a positive finite number.  Returns
    (the three sigmas as floats, scipy's radius `int(truncate * sigma + 0.5)` of each axis -- 0 where scipy skips the axis (sigma
    <= 1e-15) or applies the one-tap kernel).  ValueError for anything else and for a radius above GAUSS_MAX_RADIUS."""
    def number(v):
        return isinstance(v, numbers.Real) and not isinstance(v, bool)

    sig = (sigma,) * 3 if number(sigma) else (tuple(sigma) if isinstance(sigma, (tuple, list)) else None)
    if sig is None or len(sig) != 3 or not all(number(s) and 0.0 <= float(s) < float("inf") for s in sig):
        raise ValueError(f"{what}: sigma must be a finite number >= 0 or a sequence of three in (z, y, x) order, got {sigma!r}")
    if not number(truncate) or not 0.0 < float(truncate) < float("inf"):
        raise ValueError(f"{what}: truncate must be a positive finite number, got {truncate!r}")
    sig = tuple(float(s) for s in sig)
    radii = tuple(0 if s <= 1e-15 else int(float(truncate) * s + 0.5) for s in sig)
    if max(radii) > _lib.GAUSS_MAX_RADIUS:
        raise ValueError(f"{what}: the radius int(truncate * sigma + 0.5) of every axis must be at most {_lib.GAUSS_MAX_RADIUS}, got "
                         f"{radii} for sigma={sigma!r}, truncate={truncate!r}")
    return sig, radii


def gaussian_filter3d(score, sigma=4.0, truncate=4.0, batched=None):
    """`scipy.ndimage.gaussian_filter(vol, sigma, truncate=truncate)` (order 0, reflect border) of every D x H x W volume of
    score: [..., D, H, W], batching and strides as `median_filter3d`.  `sigma`: one number, or three in (z, y, x) order -- slices
    are usually thicker than the pixels in them, and a sigma in millimetres is `sigma_mm / spacing` per axis; each finite and >=
    0.  The radius of an axis is `int(truncate * sigma + 0.5)`, at most 32 (else ValueError); an axis of radius 0 is skipped, as
    scipy's one-tap kernel leaves it.  Returns an fp32 device tensor shaped like score, bit for bit scipy's on the fp32 volumes for
    finite inputs, without a host synchronisation: the z pass of all volumes in one launch and the two in-plane passes in another
    (`anoddpm_gauss3d`; one launch when the z axis, or both others, are skipped).  Any D >= 1: the border reflects as often as the
    radius asks.  With all three axes skipped the result is an fp32 copy and nothing is launched.  NaN / inf spread within the
    radii by IEEE rules; no other volume is touched.  The tap tables are `gaussian_filter`'s, cached per (sigma, truncate,
    device); the workspace of the z pass is allocated per call (the caching allocator: capturable after the first use)."""
    V, D, H, W = _volumes(score, batched, "gaussian_filter3d", "score")
    sig, radii = _gauss3d_radii(sigma, truncate, "gaussian_filter3d")
    if not any(radii):
        return score.to(dtype=torch.float32, copy=True, memory_format=torch.contiguous_format)
    sc, _, s_stride = _segments(score, V, "gaussian_filter3d(score)")
    dev = sc.device
    out = torch.empty(tuple(score.shape), dtype=torch.float32, device=dev)
    a = _lib.Gauss3dArgs()
    a.src, a.dst, a.src_stride = sc.data_ptr(), out.data_ptr(), s_stride
    if radii[0] and (radii[1] or radii[2]):
        tmp = torch.empty((V * D * H * W,), dtype=torch.float32, device=dev)
        a.tmp = tmp.data_ptr()
    for axis, s, r in zip("zyx", sig, radii):
        setattr(a, "r" + axis, r)
        if r:
            setattr(a, "w" + axis, _gauss_table(s, truncate, r, dev).data_ptr())
    a.S, a.D, a.H, a.W = V, D, H, W
    _launch("gauss3d", a, dev)
    return out


# ---------------------------------------------------------------------------------- distances on whole volumes (csrc/surface3d.hip)
def _surface3d_workspace(S, D, H, W, what, transform=False):
    """`_launch`'s workspace of the two entry points of csrc/surface3d.hip: what `anoddpm_surface3d_workspace_bytes` answers, or
    the transform's stated share of it (8 * S * D * H * W bytes: half of its voxel part)."""
    nbytes = lib().anoddpm_surface3d_workspace_bytes(S, D, H, W)
    return (8 * S * D * H * W if transform and nbytes >= 0 else nbytes, torch.int32,
            f"{what}: {S} volumes of {D} x {H} x {W} are too large: (D-1)^2 + (H-1)^2 + (W-1)^2, D*H*W and 2 * volumes * D*H must stay below 2^31")


def distance_transform3d(x, level=0.0, squared=False, batched=None):
    """`scipy.ndimage.distance_transform_edt(vol > level)` of every D x H x W volume of x ([..., D, H, W]; a 3-D tensor is one
    volume, `batched=True` refuses it; NaN is background), in voxels: an fp64 device tensor shaped like x, bit for bit scipy's
    wherever the volume has a background voxel, without a host synchronisation.  `squared=True`: the exact int32 squared distance
    instead.  A volume without a background voxel has no defined answer: +inf (squared: -1) everywhere in it."""
    V, D, H, W = _volumes(x, batched, "distance_transform3d", "x")
    xt = _f32c(x, "distance_transform3d(x)")
    dev = xt.device
    sq = torch.empty(tuple(x.shape), dtype=torch.int32, device=dev)
    dist = None if squared else torch.empty(tuple(x.shape), dtype=torch.float64, device=dev)
    a = _lib.Distance3dArgs()
    a.src, a.sq, a.dist = xt.data_ptr(), sq.data_ptr(), (None if squared else dist.data_ptr())
    a.src_stride, a.S, a.D, a.H, a.W, a.level = D * H * W, V, D, H, W, float(level)
    _launch("distance_transform3d", a, dev, _surface3d_workspace(V, D, H, W, "distance_transform3d", transform=True))
    return sq if squared else dist


def surface_distance3d(pred, ref, level=0.0, return_status=False):
    """Boundary distances of every D x H x W volume of pred ([..., D, H, W]) against the volume of ref at the same place, or against
    ONE `[D, H, W]` reference shared by all (its border is computed once), in voxels.  With `m = vol > level`, the border of m is
    `m & ~scipy.ndimage.binary_erosion(m)` on the 3-D array (6 face neighbours, everything outside the volume counts as
    background -- so in a volume of ONE slice every foreground voxel is border; `surface_distance` is the function for planes).
    Returns the dict of `surface_distance` -- `hd`, `hd95`, `assd`, `p95` [..., 3], `mean` [..., 2], `max2` [..., 2], `counts`
    [..., 2], `status` -- as device tensors shaped like pred without its last three dimensions, no host synchronisation (usable
    inside a captured graph), the same bits every run.  Where the status is non-zero every fp64 value is NaN and `max2` is -1.
    `return_status=True` returns `(dict, status)`."""
    V, D, H, W = _volumes(pred, None, "surface_distance3d", "pred")
    if not isinstance(ref, torch.Tensor):
        raise TypeError("surface_distance3d: ref must be a device tensor")
    if tuple(ref.shape) != tuple(pred.shape) and tuple(ref.shape) != (D, H, W):
        raise ValueError(f"surface_distance3d: ref {tuple(ref.shape)} is neither the shape of pred {tuple(pred.shape)} nor one [D, H, W] volume")
    pt = _f32c(pred, "surface_distance3d(pred)")
    rt = _f32c(ref, "surface_distance3d(ref)")
    if rt.device != pt.device:
        raise ValueError("surface_distance3d: pred and ref are on different devices")
    dev = pt.device
    lead = tuple(pred.shape[:-3])
    out = {"counts": torch.empty(lead + (2,), dtype=torch.int32, device=dev), "max2": torch.empty(lead + (2,), dtype=torch.int32, device=dev),
           "mean": torch.empty(lead + (2,), dtype=torch.float64, device=dev), "p95": torch.empty(lead + (3,), dtype=torch.float64, device=dev),
           "status": torch.empty(lead, dtype=torch.int32, device=dev)}
    a = _lib.Surface3dArgs()
    a.pred, a.ref = pt.data_ptr(), rt.data_ptr()
    for k in ("counts", "max2", "mean", "p95", "status"):
        setattr(a, k, out[k].data_ptr())
    n = D * H * W
    a.pred_stride, a.ref_stride = n, (n if rt.numel() == V * n and V > 1 else 0)
    a.S, a.D, a.H, a.W, a.level = V, D, H, W, float(level)
    _launch("surface_distance3d", a, dev, _surface3d_workspace(V, D, H, W, "surface_distance3d"))
    out["hd"] = torch.sqrt(out["max2"].max(dim=-1).values.double())              # max2 is -1 where the status is set: NaN
    out["hd95"] = out["p95"][..., 2]
    out["assd"] = (out["mean"][..., 0] + out["mean"][..., 1]) / 2
    return (out, out["status"]) if return_status else out


def HD95_volume(real_mask, pred_mask):
    """`HD95` for whole volumes: the 95th-percentile Hausdorff distance (both directions pooled) between the 0 / 1 masks
    `[..., D, H, W]` in voxels as a Python float, `surface_distance3d(pred_mask, real_mask)["hd95"]`, and for several volumes its
    mean over the volumes where both borders exist.  NaN when there is no such volume."""
    o = surface_distance3d(pred_mask, real_mask)
    return float(_valid_mean(o["hd95"].reshape(-1), o["status"].reshape(-1))[0])


class _VolumePostProcessType(type):
    """`VolumePostProcess(..., gaussian=sigma)`: `_PostProcessType`'s arrangement -- the trailing keyword is taken by the call of
    the class, and `__init__` keeps its five positional settings and its signature."""

    def __call__(cls, *args, gaussian=None, **kw):
        self = super().__call__(*args, **kw)
        if gaussian is not None:
            object.__setattr__(self, "gaussian", _gauss3d_radii(gaussian, 4.0, "VolumePostProcess: gaussian")[0])
        return self


class VolumePostProcess(metaclass=_VolumePostProcessType):
    """Settings of the volume-wise post-processing between the squared error of a volume and its scores; immutable, hashable,
    picklable.  `median`: window of the 3-D median filter (3, 5; None: off).  `erode`: 3-D erosions of the region of interest
    (0 ... 8; 0: used as it is).  `roi_level`: when not None the region of interest is `real > roi_level` unless the caller hands
    one in.  `min_size` / `connectivity` (1, 2, 3: 6 / 18 / 26 neighbours): 3-D components of the thresholded volume below that
    many voxels are dropped (0: off).  The defaults are `PostProcess`'s.  `gaussian` (keyword only; None: off): sigma in voxels of
    a Gaussian filter (`gaussian_filter3d`, truncate 4.0) applied before the median, one number or three in (z, y, x) order --
    for a sigma in millimetres divide by the spacing of each axis; kept as a tuple of three floats."""
    __slots__ = ("median", "erode", "roi_level", "min_size", "connectivity", "gaussian")

    def __init__(self, median=5, erode=3, roi_level=None, min_size=7, connectivity=1):
        if median is not None and median not in _lib.MEDIAN3D_SIZES:
            raise ValueError(f"VolumePostProcess: median must be None or one of {_lib.MEDIAN3D_SIZES}, got {median!r}")
        if isinstance(erode, bool) or int(erode) != erode or not 0 <= erode <= _lib.ERODE_MAX:
            raise ValueError(f"VolumePostProcess: erode must be in 0 ... {_lib.ERODE_MAX}, got {erode!r}")
        if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 0:
            raise ValueError(f"VolumePostProcess: min_size must be an integer >= 0, got {min_size!r}")
        if connectivity not in (1, 2, 3):
            raise ValueError(f"VolumePostProcess: connectivity must be 1, 2 or 3, got {connectivity!r}")
        object.__setattr__(self, "gaussian", None)                   # _VolumePostProcessType.__call__ sets it
        for k, v in (("median", median), ("erode", int(erode)), ("roi_level", None if roi_level is None else float(roi_level)),
                     ("min_size", int(min_size)), ("connectivity", int(connectivity))):
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("VolumePostProcess is immutable")

    def __delattr__(self, name):
        raise AttributeError("VolumePostProcess is immutable")

    def _settings(self):
        """The settings that are spelled out: `gaussian` only when it is set, so that key, hash, repr and pickle of everything from
        before it existed are what they were."""
        return [k for k in self.__slots__ if k != "gaussian" or self.gaussian is not None]

    def _key(self):
        return tuple(getattr(self, k) for k in self._settings())

    def __eq__(self, other):
        return isinstance(other, VolumePostProcess) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "VolumePostProcess(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self._settings()) + ")"

    def __reduce__(self):
        if self.gaussian is None:
            return VolumePostProcess, self._key()
        return _volume_postprocess_from, ({k: getattr(self, k) for k in self.__slots__},)


def _volume_postprocess_from(settings):
    return VolumePostProcess(**settings)


def postprocess_volumes(sqerr, pp, real=None, roi=None):
    """The squared-error volumes `sqerr` ([..., D, H, W]; batching as `median_filter3d`) after `pp`'s 3-D median filter inside the
    region of interest.  The region is `roi` (a 0 / 1 tensor) when given, else `real > pp.roi_level` when `pp.roi_level` is set,
    else everything; it has the shape of one plane (the same column through every slice), one volume (shared by the batch) or sqerr,
    and is thresholded and eroded `pp.erode` times in 3-D in ONE launch -- with nothing outside the volume, so the erosion also
    takes `pp.erode` slices off either end of the column.  ONE median launch then applies it.  Returns a
    device tensor shaped like sqerr, no host synchronisation.  With `pp.median` None the region is applied by an elementwise
    product.  `pp.gaussian` runs first (`gaussian_filter3d`): the median and the region see the smoothed volumes."""
    if not isinstance(pp, VolumePostProcess):
        raise TypeError("postprocess_volumes: pp must be a VolumePostProcess")
    V, D, H, W = _volumes(sqerr, None, "postprocess_volumes", "sqerr")
    level = 0.0
    if roi is None and pp.roi_level is not None:
        if real is None:
            raise ValueError("postprocess_volumes: VolumePostProcess.roi_level needs the real volume")
        roi, level = real, pp.roi_level
    if roi is not None:
        if not isinstance(roi, torch.Tensor):
            raise TypeError("postprocess_volumes: roi must be a device tensor")
        if roi.numel() not in (H * W, D * H * W, V * D * H * W):
            raise ValueError(f"postprocess_volumes: roi {tuple(roi.shape)} does not match sqerr {tuple(sqerr.shape)}")
        if not pp.erode:
            roi = (_f32c(roi, "postprocess_volumes(roi)") > level).float()
        else:                                                        # one plane: the same column through every slice, eroded as that volume
            roi = erode_mask3d(roi.reshape(1, H, W).expand(D, H, W) if roi.numel() == H * W else roi.reshape((-1, D, H, W)), pp.erode, level)
    smoothed = pp.gaussian is not None
    if smoothed:
        sqerr = gaussian_filter3d(sqerr, pp.gaussian)
    if pp.median is not None:
        return median_filter3d(sqerr, pp.median, roi=roi)
    out = _f32c(sqerr, "postprocess_volumes(sqerr)")
    if roi is None:
        return out if smoothed else out.clone()
    shape = (1, 1, H, W) if roi.numel() == H * W else ((1, D, H, W) if roi.numel() == D * H * W else (V, D, H, W))
    return (out.reshape(V, D, H, W) * roi.reshape(shape)).reshape(out.shape)


_VOLUME_KEYS = (("dice", "dice"), ("precision", "precision"), ("recall", "recall"), ("FPR", "fpr"), ("AUC", "auc"), ("AP", "ap"),
                ("best_dice", "best_dice"), ("best_threshold", "best_threshold"), ("AUC_status", "status"))
_VOLUME_SURFACE_KEYS = (("HD", "hd"), ("HD95", "hd95"), ("ASSD", "assd"), ("surface_status", "status"))


def anomaly_metrics_volume(real, recon, mask, threshold=0.5, postprocess=None, roi=None):
    """The scores of whole volumes: real, recon and mask `[D, H, W]` (one volume; returns one record) or `[V, D, H, W]` (returns a
    list of V records).  Nothing of a volume is averaged over its slices: per volume, the squared error `(recon - real)^2` of the
    fused `anomaly_maps` pass is ONE segment of D * H * W voxels, and a record holds
      `dice`, `precision`, `recall`, `FPR`       of the prediction `sqerr > threshold` (`scores_at`: 2 tp / (tp + fp + P), tp / (tp + fp),
                                                 tp / P, fp / N; NaN for an empty class)
      `AUC`, `AP`, `best_dice`, `best_threshold` of `curve_scores` over the volume (the chip-wide sort from 65 536 voxels on), and
      `AUC_status`, the status word of that launch
    as Python numbers from one copy to the host, and `maps`: `sqerr` and `pred` of the volume as device tensors [D, H, W].
    `postprocess` (a `VolumePostProcess`; `roi`: see `postprocess_volumes`) ADDS the `_pp` twin of every key: the curve scores of
    `maps["sqerr_pp"]` (`postprocess_volumes`) and the scores at `threshold` of `maps["pred_pp"]`, the filtered volume cut at
    `threshold` without its 3-D components below `postprocess.min_size` voxels.
    `anomaly_metrics_volume_surface` is this function with the boundary distances of every volume added."""
    return _metrics_volume(real, recon, mask, threshold, postprocess, roi, False)


def anomaly_metrics_volume_surface(real, recon, mask, threshold=0.5, postprocess=None, roi=None):
    """`anomaly_metrics_volume` (same arguments, same records, same bits) with `HD`, `HD95`, `ASSD` (voxels; NaN where a border is
    empty) and `surface_status` ADDED to every record: `surface_distance3d` between `maps["pred"]` and the mask, one launch
    sequence for all V volumes, and with `postprocess` their `_pp` twins from `maps["pred_pp"]`.  They reach the host in the same
    single copy as the other scores.  (A function of its own, as `anomaly_metrics_surface` is beside `anomaly_metrics`.)"""
    return _metrics_volume(real, recon, mask, threshold, postprocess, roi, True)


def _metrics_volume(real, recon, mask, threshold, postprocess, roi, surface):
    if not all(isinstance(x, torch.Tensor) for x in (real, recon, mask)):
        raise TypeError("anomaly_metrics_volume: real, recon and mask must be device tensors")
    if postprocess is not None and not isinstance(postprocess, VolumePostProcess):
        raise TypeError("anomaly_metrics_volume: postprocess must be a VolumePostProcess")
    if real.dim() not in (3, 4) or real.numel() == 0:
        raise ValueError(f"anomaly_metrics_volume: real must be [D, H, W] or [V, D, H, W], got shape {tuple(real.shape)}")
    if recon.shape != real.shape or mask.shape != real.shape:
        raise ValueError(f"anomaly_metrics_volume: recon {tuple(recon.shape)} and mask {tuple(mask.shape)} must have real's shape {tuple(real.shape)}")
    single = real.dim() == 3
    D, H, W = real.shape[-3:]
    V = 1 if single else real.shape[0]
    rl, mk = real.reshape(V, D, H, W), _f32c(mask, "anomaly_metrics_volume(mask)").reshape(V, D, H, W)
    maps = anomaly_maps(rl, recon.reshape(V, D, H, W), mk, threshold, want=("sqerr", "pred"))[0]
    stacks = [("", maps["sqerr"], maps["sqerr"], float(threshold))]
    if postprocess is not None:
        maps["sqerr_pp"] = postprocess_volumes(maps["sqerr"], postprocess, real=rl, roi=roi)
        maps["pred_pp"] = _small_components3d(maps["sqerr_pp"], float(threshold), postprocess.min_size, postprocess.connectivity)[0]
        stacks.append(("_pp", maps["sqerr_pp"], maps["pred_pp"], 0.5))                    # a 0 / 1 volume cut at 0.5 is itself
    dev = {}
    for sfx, sq, cut, thr in stacks:
        at = scores_at(mk.reshape(V, -1), cut.reshape(V, -1), torch.full((1,), thr, dtype=torch.float32, device=sq.device), batched=True)
        for v in range(V):                                           # one segment per launch: a volume goes to the chip-wide sort
            o = curve_scores(mk[v].reshape(-1), sq[v].reshape(-1), batched=False)
            dev.update({f"{k}{sfx}/{v}": o[src] for k, src in _VOLUME_KEYS if src in o})
            dev.update({f"{k}{sfx}/{v}": at[src][v] for k, src in _VOLUME_KEYS if src not in o})
        if surface:
            sd = surface_distance3d(maps["pred" + sfx], mk)
            dev.update({f"{k}{sfx}/{v}": sd[src][v] for k, src in _VOLUME_SURFACE_KEYS for v in range(V)})
    keys = _VOLUME_KEYS + (_VOLUME_SURFACE_KEYS if surface else ())
    h = _to_host(dev)
    records = []
    for v in range(V):
        r = {}
        for sfx, _, _, _ in stacks:
            for k, _ in keys:
                x = float(h[f"{k}{sfx}/{v}"].reshape(-1)[0])
                r[k + sfx] = int(x) if k in ("AUC_status", "surface_status") else x
            if r["best_dice" + sfx] != r["best_dice" + sfx]:
                r["best_threshold" + sfx] = NAN                      # no positive: no threshold is better than another
        r["maps"] = {k: m[v] for k, m in maps.items()}
        records.append(r)
    return records[0] if single else records


# ---------------------------------------------------------------------------------- evaluation.py surface
def heatmap(real, recon, mask, filename, save=True):
    """evaluation.py:12-22 computes the squared-error / threshold images, plots them and returns None.  The images come from the
    fused pass (anomaly_maps); writing the figure is plot I/O, out of scope: `filename` / `save` are accepted and ignored."""
    anomaly_maps(real, recon, None, want=("mse_img", "thr_img"))
    return None


def dice_coeff(real, recon, real_mask, smooth=0.000001, mse=None):
    """evaluation.py:26-36.  `mse`, when given, is used as it is, like upstream (evaluation.py:34-35: `sum(mse * real_mask)` and
    `sum(mse) + sum(real_mask)` per image): the thresholded map of detection.py:232, or any real-valued map -- the three sums are
    then plain fp64 reductions on the device (no threshold pass, no host synchronisation), so the value is the reference's for
    every `mse`, not only for a {0,1} one."""
    if mse is None:
        _, counts = anomaly_maps(real, recon, real_mask, threshold=0.5, want=())
        d = (2.0 * counts[:, 2] + smooth) / (counts[:, 0] + counts[:, 1] + smooth)
    else:
        m = _f32c(mse, "dice_coeff(mse)")
        k = _f32c(real_mask, "dice_coeff(real_mask)")
        if m.dim() < 1 or k.numel() != m.numel():
            raise ValueError(f"dice_coeff: mse shape {tuple(m.shape)} does not match real_mask {tuple(k.shape)}")
        m, k = m.reshape(m.shape[0], -1).double(), k.reshape(m.shape[0], -1).double()
        d = (2.0 * (m * k).sum(dim=1) + smooth) / (m.sum(dim=1) + k.sum(dim=1) + smooth)
    return d.mean(dim=0).float()


def PSNR(recon, real):
    """evaluation.py:39-44 (returns a numpy scalar like upstream)."""
    _, counts = anomaly_maps(real, recon, None, want=())
    c = counts.cpu()
    mse = c[:, 9].sum() / real.numel()
    return (20 * torch.log10(c[:, 10].max() / torch.sqrt(mse))).float().numpy()


def SSIM(real, recon):
    """evaluation.py:46-47.  Device tensors: the native kernel (`ssim`, 7 x 7 uniform window, data_range 2.0) on `(H, W, C)`
    images as detection.py:241-246 passes them (channels last, upstream's `channel_axis=2`) and on `(H, W)` images as
    detection.py:361, 767 pass them, read as ONE single-channel image; returns a Python float like skimage.  Host inputs (numpy
    arrays, CPU tensors): skimage, as upstream."""
    if isinstance(real, torch.Tensor) and isinstance(recon, torch.Tensor) and real.is_cuda and recon.is_cuda:
        if real.shape != recon.shape or real.dim() not in (2, 3):
            raise ValueError(f"SSIM: expected two (H, W, C) or two (H, W) images, got {tuple(real.shape)} and {tuple(recon.shape)}")
        if real.dim() == 3:
            real, recon = real.permute(2, 0, 1), recon.permute(2, 0, 1)
        return float(ssim(real, recon, batched=False)[0])
    from skimage.metrics import structural_similarity               # raises ImportError when skimage is absent
    if isinstance(real, torch.Tensor):
        real, recon = real.detach().cpu().numpy(), recon.detach().cpu().numpy()
    return structural_similarity(real, recon, channel_axis=2)


def _mask_counts(real_mask, recon_mask):
    zeros = torch.zeros_like(_f32c(recon_mask, "metrics(recon_mask)"))
    m = _f32c(recon_mask, "metrics(recon_mask)")
    if not bool(((m == 0) | (m == 1)).all()):
        raise ValueError("recon_mask must be a {0,1} map (detection.py:232)")
    _, counts = anomaly_maps(zeros.reshape(1, -1), m.reshape(1, -1), real_mask.reshape(1, -1), threshold=0.5, want=())
    return counts[0]


def IoU(real, recon):
    """evaluation.py:50-55."""
    c = _mask_counts(real, recon).cpu()
    return float(c[7] / (c[8] + 1e-8))


def precision(real_mask, recon_mask):
    """evaluation.py:58-61."""
    c = _mask_counts(real_mask, recon_mask)
    return (c[3] / (c[3] + c[4] + 1e-6)).float()


def recall(real_mask, recon_mask):
    """evaluation.py:65-68."""
    c = _mask_counts(real_mask, recon_mask)
    return (c[3] / (c[3] + c[5] + 1e-6)).float()


def FPR(real_mask, recon_mask):
    """evaluation.py:71-74."""
    c = _mask_counts(real_mask, recon_mask)
    return (c[4] / (c[4] + c[6] + 1e-6)).float()


def _pooled(real_mask, square_error, what):
    """Lists / tuples of device tensors on both sides -> the pooled segment of all of them (mask, score), else None."""
    if not isinstance(real_mask, (list, tuple)) and not isinstance(square_error, (list, tuple)):
        return None
    if not (isinstance(real_mask, (list, tuple)) and isinstance(square_error, (list, tuple))) or len(real_mask) != len(square_error) or not real_mask:
        raise TypeError(f"{what}: a pooled call takes two non-empty lists of device tensors of the same length")
    for x in (*real_mask, *square_error):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise TypeError(f"{what}: a pooled call takes device tensors only")
    pool = PooledCurves(sum(s.numel() for s in square_error), device=square_error[0].device)
    for m, s in zip(real_mask, square_error):
        pool.add(m, s)
    return pool._mask, pool._score


class PooledCurves:
    """The masks and scores of a run collected into ONE segment -- the curve pooled over a whole test set (detection.py:538-643
    `roc_data`) -- in two preallocated fp32 device buffers of `capacity` pixels.  `add(mask, score)` appends device tensors of
    equal `numel`, or one mask plane shared by several score planes (the mask is written out once per plane), without a host
    synchronisation; it raises ValueError, from the count kept on the host, when the buffers would overflow.  `len()` is the
    number of pixels held, `reset()` empties the pool.  `scores()` is the dict `curve_scores` returns for the pooled segment
    (S = 1, device tensors, no synchronisation), `roc_curve()` / `pr_curve()` what `ROC_AUC` / `PR_curve` return for it."""

    def __init__(self, capacity, device=None):
        capacity = int(capacity)
        if capacity < 1 or capacity >= _ROC_WIDE_NEVER:
            raise ValueError(f"PooledCurves: capacity must be in [1, 2^31), got {capacity}")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise ValueError("PooledCurves: the buffers live on the device")
        self._mask = torch.empty((capacity,), dtype=torch.float32, device=device)
        self._score = torch.empty((capacity,), dtype=torch.float32, device=device)
        self._n = 0

    capacity = property(lambda self: self._mask.numel())

    def __len__(self):
        return self._n

    def reset(self):
        self._n = 0

    def add(self, mask, score):
        if not isinstance(mask, torch.Tensor) or not isinstance(score, torch.Tensor) or not mask.is_cuda or not score.is_cuda:
            raise TypeError("PooledCurves.add: mask and score must be device tensors")
        k, km = score.numel(), mask.numel()
        if k == 0 or km == 0 or k % km != 0:
            raise ValueError(f"PooledCurves.add: mask of {km} elements does not match score {tuple(score.shape)}")
        if self._n + k > self.capacity:
            raise ValueError(f"PooledCurves.add: {self._n} + {k} pixels exceed the capacity {self.capacity}")
        self._score[self._n:self._n + k].copy_(score.reshape(-1))
        self._mask[self._n:self._n + k].view(k // km, km).copy_(mask.reshape(1, km).expand(k // km, km))
        self._n += k

    def _segment(self, what):
        if self._n == 0:
            raise ValueError(f"PooledCurves.{what}: the pool is empty")
        return self._mask[:self._n], self._score[:self._n]

    def scores(self):
        return curve_scores(*self._segment("scores"), batched=False)

    def roc_curve(self):
        return ROC_AUC(*self._segment("roc_curve"))

    def pr_curve(self):
        return PR_curve(*self._segment("pr_curve"))


class PooledRegionCurves(PooledCurves):
    """`PooledCurves` that also keeps what the per-region overlap score needs, so that one pool yields every pooled score of a
    run: beside mask and score the int32 area of every pixel's connected ground-truth region (`component_areas`, `connectivity`
    2: 8 neighbours) and, in a one-element int64 device accumulator, the number of regions.  `add(mask, score)`: mask
    `[..., H, W]`, score of the same shape or k stacked copies' worth of planes for the one mask; planes of different adds may
    differ in H x W.  One component run per `add` on the mask planes, no host synchronisation.  Every (mask plane, score plane)
    pair is an image of the set, so a mask shared by k score planes counts its regions k times.  Overflow raises ValueError from
    the count kept on the host, as `PooledCurves.add` does.  `aupro(limit)` is a `[1]` fp64 device tensor without a
    synchronisation (NaN under the status rule of `metrics.aupro`; `return_status=True` also returns the status word),
    `pro_curve(limit)` the dict `pro_points` returns for the pooled segment.  `scores()` / `roc_curve()` / `pr_curve()` are
    inherited.  The pooled segment goes to the kernels as one plane of 1 x n: they read the plane shape only through n, and the
    region counts only through their sum."""

    def __init__(self, capacity, connectivity=2, device=None):
        _check_connectivity(connectivity, "PooledRegionCurves")
        super().__init__(capacity, device=device)
        self._connectivity = int(connectivity)
        self._area = torch.empty((self.capacity,), dtype=torch.int32, device=self._mask.device)
        self._regions = torch.zeros((1,), dtype=torch.int64, device=self._mask.device)

    def reset(self):
        super().reset()
        self._regions.zero_()

    def add(self, mask, score):
        if not isinstance(mask, torch.Tensor) or not isinstance(score, torch.Tensor) or not mask.is_cuda or not score.is_cuda:
            raise TypeError("PooledRegionCurves.add: mask and score must be device tensors")
        k, km = score.numel(), mask.numel()
        if mask.dim() < 2 or score.dim() < 2 or k == 0 or km == 0 or k % km != 0 or tuple(score.shape[-2:]) != tuple(mask.shape[-2:]):
            raise ValueError(f"PooledRegionCurves.add: mask {tuple(mask.shape)} does not match score {tuple(score.shape)}")
        if self._n + k > self.capacity:
            raise ValueError(f"PooledRegionCurves.add: {self._n} + {k} pixels exceed the capacity {self.capacity}")
        H, W = mask.shape[-2:]
        areas, regions = component_areas(mask.reshape(-1, H, W), self._connectivity, batched=True)
        n0 = self._n
        super().add(mask, score)
        self._area[n0:n0 + k].view(k // km, km).copy_(areas.reshape(1, km).expand(k // km, km))
        self._regions += regions.sum() * (k // km)

    def _pro(self, limit, curve, what):
        if isinstance(limit, bool) or not 0.0 < float(limit) <= 1.0:
            raise ValueError(f"pro: limit must be in (0, 1], got {limit!r}")
        mk, sc = self._segment(what)
        n, dev = self._n, sc.device
        out = {"aupro": torch.empty((1,), dtype=torch.float64, device=dev),
               "counts": torch.empty((1, 4), dtype=torch.int64, device=dev),
               "status": torch.empty((1,), dtype=torch.int32, device=dev), "n": n}
        a = ProArgs()
        a.score, a.area, a.region_counts, a.mask = sc.data_ptr(), self._area.data_ptr(), self._regions.data_ptr(), mk.data_ptr()
        a.aupro, a.counts, a.status = out["aupro"].data_ptr(), out["counts"].data_ptr(), out["status"].data_ptr()
        a.score_stride, a.area_stride, a.mask_stride = n, n, n
        a.limit, a.S, a.planes_per_segment, a.H, a.W = float(limit), 1, 1, 1, n
        if curve:
            a.curve_fps, a.curve_pro, a.curve_thr, a.curve_len, a.curve_cap = _curve_buffers(out, "pro", torch.float64, 1, n, dev)
        return _pro_call(a, out, 1, n, dev, n >= PRO_WIDE_MIN_N, None)

    def aupro(self, limit=0.3, return_status=False):
        o = self._pro(limit, False, "aupro")
        val = _nan_where_status(o, "aupro")
        return (val, o["status"]) if return_status else val

    def pro_curve(self, limit=0.3):
        return _pro_points_of(self._pro(limit, True, "pro_curve"))[0]


class HealthyPool:
    """The score maps of a HEALTHY validation run collected into one segment, to calibrate operating thresholds without ground
    truth: an fp32 device buffer of `capacity` pixels (`PooledCurves`' buffer handling, without a mask).  `add(score)` appends a
    device tensor of any shape without a host synchronisation and raises ValueError, from the count kept on the host, when the
    buffer would overflow; `len()` is the number of pixels held, `reset()` empties the pool.
    `thresholds(fpr, negatives=None)`: for every requested false-positive rate (a number or up to 16 of them) the operating
    threshold as a [Q] fp32 device tensor -- with `k = floor(fpr * negatives)` in Python floats (`negatives` defaults to
    `len(pool)`), the pooled value of descending rank k: the smallest pooled value that at most k pooled values exceed, so the
    prediction `score > threshold` marks at most that share of the healthy pixels.  `fpr = 0` gives the pool's maximum; a rate
    whose k reaches `len(pool)` is a ValueError.  Pass the number of region-of-interest pixels as `negatives` when the maps were
    zeroed outside it: the zeros sit at the bottom and do not move the k-th largest value.  `order_stats(ranks)` is the primitive
    underneath: `metrics.order_stats` of the pooled segment."""

    def __init__(self, capacity, device=None):
        capacity = int(capacity)
        if capacity < 1 or capacity >= _ROC_WIDE_NEVER:
            raise ValueError(f"HealthyPool: capacity must be in [1, 2^31), got {capacity}")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise ValueError("HealthyPool: the buffer lives on the device")
        self._score = torch.empty((capacity,), dtype=torch.float32, device=device)
        self._n = 0

    capacity = property(lambda self: self._score.numel())

    def __len__(self):
        return self._n

    def reset(self):
        self._n = 0

    def add(self, score):
        if not isinstance(score, torch.Tensor) or not score.is_cuda:
            raise TypeError("HealthyPool.add: score must be a device tensor")
        k = score.numel()
        if k == 0:
            raise ValueError("HealthyPool.add: empty score")
        if self._n + k > self.capacity:
            raise ValueError(f"HealthyPool.add: {self._n} + {k} pixels exceed the capacity {self.capacity}")
        self._score[self._n:self._n + k].copy_(score.reshape(-1))
        self._n += k

    def order_stats(self, ranks, tile=None, return_status=False):
        if self._n == 0:
            raise ValueError("HealthyPool.order_stats: the pool is empty")
        return order_stats(self._score[:self._n], ranks, batched=False, tile=tile, return_status=return_status)

    def thresholds(self, fpr, negatives=None):
        rates = [fpr] if isinstance(fpr, (int, float)) else list(fpr)
        negatives = self._n if negatives is None else negatives
        if isinstance(negatives, bool) or not isinstance(negatives, int) or negatives < 1:
            raise ValueError(f"HealthyPool.thresholds: negatives must be a positive int, got {negatives!r}")
        ranks = []
        for f in rates:
            if isinstance(f, bool) or not isinstance(f, (int, float)) or not 0.0 <= float(f) <= 1.0:
                raise ValueError(f"HealthyPool.thresholds: a false-positive rate is a number in [0, 1], got {f!r}")
            k = int(float(f) * float(negatives))
            if k >= self._n:
                raise ValueError(f"HealthyPool.thresholds: rate {f!r} of {negatives} pixels is rank {k}, the pool holds {self._n}")
            ranks.append(k)
        return self.order_stats(ranks)["value"][0]


def ROC_AUC(real_mask, square_error):
    """evaluation.py:78-82.  Device tensors: the native sort (`roc_points` of the flattened inputs); the host prepends the
    `(0, 0, inf)` point and divides the integer counts in fp64, which gives sklearn's `(fpr, tpr, thresholds)` bit for bit
    (NaN arrays when a class is empty).  A list or tuple of device tensors on each side is the pooled segment of all of them.
    Host inputs (numpy arrays, CPU tensors): sklearn, as upstream."""
    pooled = _pooled(real_mask, square_error, "ROC_AUC")
    if pooled is not None:
        real_mask, square_error = pooled
    if isinstance(real_mask, torch.Tensor) and isinstance(square_error, torch.Tensor) and real_mask.is_cuda and square_error.is_cuda:
        import numpy as np
        p = roc_points(real_mask, square_error, batched=False)[0]
        fps = np.r_[0.0, p["fps"].astype(np.float64)]
        tps = np.r_[0.0, p["tps"].astype(np.float64)]
        thresholds = np.r_[np.float32(np.inf), p["thresholds"]].astype(np.float32)
        fpr = fps / fps[-1] if fps[-1] > 0 else np.repeat(np.nan, fps.shape)
        tpr = tps / tps[-1] if tps[-1] > 0 else np.repeat(np.nan, tps.shape)
        return fpr, tpr, thresholds
    from sklearn.metrics import roc_curve
    if isinstance(real_mask, torch.Tensor):
        return roc_curve(real_mask.detach().cpu().numpy().flatten(), square_error.detach().cpu().numpy().flatten())
    return roc_curve(real_mask.flatten(), square_error.flatten())


def PR_curve(real_mask, square_error):
    """sklearn's `precision_recall_curve(real_mask.flatten(), square_error.flatten())`: `(precision, recall, thresholds)` in
    ascending threshold order with the final `(1, 0)` point appended.  Device tensors: the native sort (`pr_points` of the
    flattened inputs); the host divides the integer counts in fp64, which gives sklearn's arrays bit for bit.  Recall is all
    ones when the mask has no positive, as sklearn's is; its warning is not re-issued.  A list or tuple of device tensors on
    each side is the pooled segment of all of them.  Host inputs (numpy arrays, CPU tensors): sklearn."""
    pooled = _pooled(real_mask, square_error, "PR_curve")
    if pooled is not None:
        real_mask, square_error = pooled
    if isinstance(real_mask, torch.Tensor) and isinstance(square_error, torch.Tensor) and real_mask.is_cuda and square_error.is_cuda:
        import numpy as np
        p = pr_points(real_mask, square_error, batched=False)[0]
        tps, fps = p["tps"].astype(np.float64), p["fps"].astype(np.float64)
        prec = tps / (tps + fps)                                         # tps + fps >= 1: every point predicts something
        rec = tps / tps[-1] if tps[-1] > 0 else np.ones_like(tps)
        return np.hstack((prec[::-1], 1)), np.hstack((rec[::-1], 0)), p["thresholds"][::-1]
    from sklearn.metrics import precision_recall_curve
    if isinstance(real_mask, torch.Tensor):
        return precision_recall_curve(real_mask.detach().cpu().numpy().flatten(), square_error.detach().cpu().numpy().flatten())
    return precision_recall_curve(real_mask.flatten(), square_error.flatten())


def AUPRO(real_mask, square_error, limit=0.3):
    """Area under the per-region overlap curve of the mask's connected regions (8 neighbours) up to the false-positive rate
    `limit`, normalised to [0, 1] (Bergmann et al., IJCV 2021), as a Python float: `aupro` with all planes of the inputs pooled
    into one curve.  NaN without a region or without background; ValueError for inputs outside the precondition of `ROC_AUC`.
    A list or tuple of device tensors on each side is the pooled curve of all of them, `[..., H, W]` each, planes of mixed
    shapes allowed (`PooledRegionCurves`).  Device tensors only: the reference has no host implementation to fall back to."""
    if isinstance(real_mask, (list, tuple)) or isinstance(square_error, (list, tuple)):
        if not (isinstance(real_mask, (list, tuple)) and isinstance(square_error, (list, tuple))) or len(real_mask) != len(square_error) or not real_mask:
            raise TypeError("AUPRO: a pooled call takes two non-empty lists of device tensors of the same length")
        for x in (*real_mask, *square_error):
            if not isinstance(x, torch.Tensor) or not x.is_cuda:
                raise TypeError("AUPRO: a pooled call takes device tensors only")
        pool = PooledRegionCurves(sum(x.numel() for x in square_error), device=square_error[0].device)
        for m, x in zip(real_mask, square_error):
            pool.add(m, x)
        return pool.pro_curve(limit)["aupro"]
    return pro_points(real_mask, square_error, limit=limit, batched=False)[0]["aupro"]


def HD95(real_mask, pred_mask):
    """The 95th-percentile Hausdorff distance (medpy's `hd95`: the 95th percentile of the border-to-border distances of both
    directions pooled) between the 0 / 1 masks, in pixels, as a Python float: `surface_distance(pred_mask, real_mask)["hd95"]`,
    and for inputs of several planes its mean over the planes where both borders exist.  NaN when there is no such plane.
    Device tensors only: the reference has no host implementation to fall back to."""
    o = surface_distance(pred_mask, real_mask)
    return float(_valid_mean(o["hd95"].reshape(-1), o["status"].reshape(-1))[0])


def AUC_score(fpr, tpr):
    """evaluation.py:85-86."""
    from sklearn.metrics import auc
    return auc(fpr, tpr)


def testing(testing_dataset_loader, diffusion, args, ema, model, test_iters=40, sequences=True):
    """evaluation.py:90-186: the test-set pass `diffusion_training.train` ends with (diffusion_training.py:153).

    Compute kept, in upstream's order and with its draw counts: (1) for `i in range(100, sample_distance, 100)` one
    `forward_backward(ema, x, "half", t_distance=i)` (upstream turns the returned sequence into an mp4 -- the video
    dump is plot I/O and is skipped, the chain itself runs so the loader and the RNG streams advance as upstream;
    `sequences=False`, an extension, skips these chains); (2) `test_iters // Batch_Size + 5` batches of
    `calc_total_vlb(x, model, args)`; (3) as many batches of `PSNR(forward_backward(ema, x, None, T // 2), x)`.
    Prints upstream's six summary lines and (extension) returns them as a dict of (mean, std) pairs.

    Upstream reads the module globals `device`, `np` and `animation`, which only exist when evaluation.py runs as
    `__main__` (evaluation.py:222-232), so its call from diffusion_training.py:153 ends in NameError; here the
    device is the model's."""
    import numpy as np

    device = next(model.parameters()).device
    ema.eval()
    model.eval()

    def batch(pairs=("cifar",)):
        # upstream's own rule per loop: the sequence loop reads data[0] for "cifar" AND "carpet" (evaluation.py:118-120), the VLB
        # and PSNR loops only for "cifar" (:144-149, :155-160) -- the carpet loader yields dicts, and with sequences=False or
        # sample_distance <= 100 upstream runs on it
        data = next(testing_dataset_loader)
        if args["dataset"] in pairs:
            return data[0].to(device)                      # [data, class] pairs
        return data["image"].to(device)

    seq_lens = []
    if sequences:
        for i in range(100, args['sample_distance'], 100):
            out = diffusion.forward_backward(ema, batch(("cifar", "carpet")), see_whole_sequence="half", t_distance=i)
            seq_lens.append(len(out))
    rounds = test_iters // args["Batch_Size"] + 5
    vlb = [diffusion.calc_total_vlb(batch(), model, args) for _ in range(rounds)]
    psnr = []
    for _ in range(rounds):
        x = batch()
        out = diffusion.forward_backward(ema, x, see_whole_sequence=None, t_distance=args["T"] // 2)
        psnr.append(PSNR(out, x))

    def ms(vals):
        return float(np.mean(vals)), float(np.std(vals))

    k = min(199, diffusion.num_timesteps - 1)              # upstream indexes [0][199] (T >= 200 in every config)
    res = {
        "total_vlb": ms([v['total_vlb'].mean(dim=-1).cpu().item() for v in vlb]),
        "prior_vlb": ms([v['prior_vlb'].mean(dim=-1).cpu().item() for v in vlb]),
        "vb@200": ms([v['vb'][0][k].cpu().item() for v in vlb]),
        "x_0_mse@200": ms([v['x_0_mse'][0][k].cpu().item() for v in vlb]),
        "mse@200": ms([v['mse'][0][k].cpu().item() for v in vlb]),
        "PSNR": ms(psnr),
        "sequence_lengths": seq_lens,
    }
    print(f"Test set total VLB: {res['total_vlb'][0]} +- {res['total_vlb'][1]}")
    print(f"Test set prior VLB: {res['prior_vlb'][0]} +- {res['prior_vlb'][1]}")
    print(f"Test set vb @ t=200: {res['vb@200'][0]} +- {res['vb@200'][1]}")
    print(f"Test set x_0_mse @ t=200: {res['x_0_mse@200'][0]} +- {res['x_0_mse@200'][1]}")
    print(f"Test set mse @ t=200: {res['mse@200'][0]} +- {res['mse@200'][1]}")
    print(f"Test set PSNR: {res['PSNR'][0]} +- {res['PSNR'][1]}")
    return res
