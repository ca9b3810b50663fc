"""-m gpu: the native volume post-processing (csrc/postproc3d.hip through metrics.median_filter3d / erode_mask3d /
remove_small_components3d / component_areas3d, postprocess_volumes and anomaly_metrics_volume) against the fixture
tests/golden/postproc3d_kat.npz (what scipy.ndimage returns on volumes) and the numpy restatements of tests/postproc3d_cases.py.
Every step selects or counts, so every comparison is `tobytes()` equality: there is no tolerance in this file.  scipy is not
needed.  The shapes are the smallest at which each kernel can go wrong: one slice, a window equal to the plane, extents across
and short of the 4 x 8 x 32 and 8 x 16 x 32 tiles, several tiles per axis."""
import gc
import os

import numpy as np
import pytest
import torch

import postproc3d_cases as pc
from conftest import GOLDEN
from score_cases import bits as _bits, host as _host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEDIAN_CASES = [(name, k) for name in sorted(pc.MEDIAN) for k in pc.WINDOWS]
ERODE_CASES = [(name, n) for name in sorted(pc.ERODE) for n in pc.ERODE_N]
COMPONENT_CASES = [(name, c) for name in sorted(pc.COMPONENTS) for c in pc.CONNECTIVITY]


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "postproc3d_kat.npz"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _is_f32_on_device(t, like):
    return t.dtype == torch.float32 and t.shape == like.shape and t.is_cuda and t.device == like.device


# ---------------------------------------------------------------------------------- median
@pytest.mark.parametrize("name,k", MEDIAN_CASES)
def test_median3d_matches_fixture_and_restatement(kat, name, k):
    from anoddpm_amd import metrics
    x = pc.make_median_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    d = _dev(x)
    out, status = metrics.median_filter3d(d, size=k, return_status=True)               # a 3-D tensor: one volume
    assert _is_f32_on_device(out, d) and status.dtype == torch.int32 and status.shape == () and int(status) == 0
    got = _host(out)
    pc.check_volume(kat, pc.mkey(name, k), got, name in pc.MEDIAN_FULL)
    assert _bits(got, pc.median3d_numpy(x, k))
    assert _bits(_host(metrics.median_filter3d(d, size=k)), got)                       # two runs
    assert _bits(_host(metrics.median_filter3d(d[None, None], size=k))[0, 0], got)     # [1, 1, D, H, W]
    assert _bits(_host(metrics.median_filter3d(d.double(), size=k)), got)              # other dtypes are converted


@pytest.mark.parametrize("k", pc.WINDOWS)
def test_median3d_batch_behind_a_volume_stride_with_every_roi_shape(kat, k):
    from anoddpm_amd import metrics
    buf, vols, plane, roi_vol, roi_batch = pc.make_batch()
    assert pc.sha(buf, plane, roi_vol, roi_batch) == str(kat["batch_in_sha"])
    S, d, h, w = pc.BATCH_SHAPE
    dbuf = _dev(buf)
    view = dbuf[:, :d * h * w].view(S, d, h, w)
    assert not view.is_contiguous() and view.stride(0) == d * h * w + pc.BATCH_PAD and view.data_ptr() == dbuf.data_ptr()
    plain, status = metrics.median_filter3d(view, size=k, return_status=True)
    assert _is_f32_on_device(plain, view) and plain.is_contiguous() and status.shape == (S,) and not bool(status.any())
    plain = _host(plain)
    assert pc.sha(plain) == str(kat[f"batch_k{k}_sha"]) and [pc.sha(v) for v in plain] == [str(s) for s in kat[f"batch_k{k}_volume_sha"]]
    assert _bits(plain, pc.median3d_numpy(vols, k))
    for roi, shape in ((plane, (1, 1, h, w)), (roi_vol, (1, d, h, w)), (roi_batch, (S, d, h, w))):
        out, status = metrics.median_filter3d(view, size=k, roi=_dev(roi), return_status=True)
        got = _host(out)
        full = np.broadcast_to(roi.reshape(shape), (S, d, h, w))
        assert not bool(status.any()) and _bits(got, plain * full), shape
        assert (got.view(np.uint32)[full == 0] == 0).all() and (got[full == 1] > 0).any()      # +0.0 outside: every bit zero
    for j in range(S):                                                                 # a stack equals per-volume calls
        assert _bits(_host(metrics.median_filter3d(view[j], size=k, roi=_dev(roi_batch[j]))), plain[j] * roi_batch[j])
    assert _bits(_host(dbuf), buf)                                                     # the input, padding included, is untouched


def test_a_bad_volume_sets_its_own_status_only(kat):
    from anoddpm_amd import _lib, metrics
    bad = pc.make_bad_batch()
    assert pc.sha(bad) == str(kat["bad_in_sha"])
    want = {"nan": _lib.ROC_NAN, "inf": _lib.ROC_INF, "negative": _lib.ROC_NEGATIVE}
    expect = [want[pc.BAD_VOLUMES[j]] if j in pc.BAD_VOLUMES else 0 for j in range(pc.BAD_SHAPE[0])]
    for k in pc.WINDOWS:
        out, status = metrics.median_filter3d(_dev(bad), size=k, return_status=True)
        assert status.tolist() == expect
        assert _bits(_host(out)[3], kat[f"bad_k{k}_clean"])
    roi = np.ones(pc.BAD_SHAPE[1:], np.float32)                                        # a region of interest that is not 0 / 1
    roi[1, 4, 4] = 0.5
    _, status = metrics.median_filter3d(_dev(bad), size=3, roi=_dev(roi), return_status=True)
    assert [s & _lib.ROC_BAD_MASK for s in status.tolist()] == [_lib.ROC_BAD_MASK] * 4
    assert [s & ~_lib.ROC_BAD_MASK for s in status.tolist()] == expect
    z = torch.full((2, 9, 9), -0.0, device=DEV)                                        # -0.0 is a valid score, reported as +0.0
    out, status = metrics.median_filter3d(z, size=3, return_status=True)
    assert int(status) == 0 and (_host(out).view(np.uint32) == 0).all()


# ---------------------------------------------------------------------------------- erosion
@pytest.mark.parametrize("name,n", ERODE_CASES)
def test_erode3d_matches_fixture_and_restatement(kat, name, n):
    from anoddpm_amd import metrics
    x, level = pc.make_erode_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"])
    d = _dev(x)
    out = metrics.erode_mask3d(d, iterations=n, level=level)
    assert _is_f32_on_device(out, d)
    got = _host(out)
    key = pc.ekey(name, n)
    assert _bits(got, pc.unpack(kat, key, x.shape)), f"{int((got != pc.unpack(kat, key, x.shape)).sum())} voxels differ"
    assert pc.sha(got) == str(kat[key + "_sha"]) and _bits(got, pc.erode3d_numpy(x, n, level))
    assert (not got.any()) == ((name, n) in pc.ERODE_EMPTY)
    b = (x > np.float32(level)).astype(np.float32)                                     # the 0 / 1 mask at the default level, and a stack
    assert _bits(_host(metrics.erode_mask3d(_dev(np.stack([b, b])), iterations=n)), np.stack([got, got]))


def test_erode3d_nan_is_above_no_level():
    from anoddpm_amd import metrics
    x, level = pc.make_erode_case("holes9x24x40")
    x[4, 12, 20] = np.nan
    got = _host(metrics.erode_mask3d(_dev(x), iterations=1, level=level))
    assert _bits(got, pc.erode3d_numpy(x, 1, level)) and got[4, 12, 20] == 0 and got[3, 12, 20] == 0 and got.any()


# ---------------------------------------------------------------------------------- components
@pytest.mark.parametrize("name,c", COMPONENT_CASES)
def test_components3d_match_fixture_and_restatement(kat, name, c):
    from anoddpm_amd import metrics
    x = pc.make_components_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"])
    d = _dev(x)
    lab = pc.labels3d_numpy(x > 0, c)
    for m in pc.COMPONENTS[name]:
        key = pc.ckey(name, c, m)
        out, counts = metrics.remove_small_components3d(d, min_size=m, connectivity=c, return_counts=True)
        assert _is_f32_on_device(out, d) and counts.dtype == torch.int64 and counts.shape == (2,)
        got = _host(out)
        assert counts.tolist() == [int(v) for v in kat[key + "_counts"]], key
        assert pc.sha(got) == str(kat[key + "_sha"]), key
        want, wcounts = pc.components3d_numpy(x, m, c, labels=lab)
        assert _bits(got, want) and tuple(counts.tolist()) == wcounts
        out2, counts2 = metrics.remove_small_components3d(d, min_size=m, connectivity=c, return_counts=True)
        assert _bits(_host(out2), got) and counts2.tolist() == counts.tolist()         # two runs give the same bits
    areas, found = metrics.component_areas3d(d, connectivity=c)
    want, wfound = pc.areas3d_numpy(x, c)
    assert areas.dtype == torch.int32 and areas.shape == d.shape and found.dtype == torch.int64 and found.shape == ()
    assert _bits(_host(areas), want) and int(found) == wfound == int(kat[f"{name}_c{c}_areas_count"])
    assert pc.sha(_host(areas)) == str(kat[f"{name}_c{c}_areas_sha"])


@pytest.mark.parametrize("c", pc.CONNECTIVITY)
def test_a_stack_of_volumes_equals_per_volume_calls(c):
    from anoddpm_amd import metrics
    names = ("edge", "corner")                                                         # both [8, 8, 8]
    stack = np.stack([pc.make_components_case(n) for n in names] + [pc.make_components_case("corner")[::-1].copy()])
    d = _dev(stack)
    out, counts = metrics.remove_small_components3d(d, min_size=28, connectivity=c, return_counts=True)
    areas, found = metrics.component_areas3d(d, connectivity=c)
    assert counts.shape == (3, 2) and found.shape == (3,)
    for j in range(3):
        o, cn = metrics.remove_small_components3d(d[j], min_size=28, connectivity=c, return_counts=True)
        a, f = metrics.component_areas3d(d[j], connectivity=c)
        assert _bits(_host(out[j]), _host(o)) and counts[j].tolist() == cn.tolist()
        assert _bits(_host(areas[j]), _host(a)) and int(found[j]) == int(f)
        assert _bits(_host(o), pc.components3d_numpy(stack[j], 28, c)[0])
    assert counts[:, 0].tolist() == [2 if c == 1 else 1, 2 if c < 3 else 1, 2 if c < 3 else 1]


# ---------------------------------------------------------------------------------- graph capture
def test_graph_replay_gives_the_eager_bits():
    from anoddpm_amd import metrics
    rng = np.random.default_rng(9900)
    a, b = (np.stack([pc.field3(rng, 6, 20, 37, False) for _ in range(2)]) for _ in range(2))
    roi = np.ones((6, 20, 37), np.float32)
    x, r = _dev(a).clone(), _dev(roi)

    def run():
        f = metrics.median_filter3d(x, size=3, roi=metrics.erode_mask3d(r, iterations=1))
        p, c = metrics._small_components3d(f, 0.1, 7, 2)
        return f, p, c

    eager = [_host(t) for t in run()]
    assert _bits(eager[0], pc.median3d_numpy(a, 3) * pc.erode3d_numpy(roi, 1)) and eager[1].any()
    x.copy_(_dev(b))
    other = [_host(t) for t in run()]
    x.copy_(_dev(a))
    assert not _bits(other[0], eager[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()                                                        # no collection of older graphs inside the capture
    try:
        with torch.cuda.graph(g):
            captured = run()
    finally:
        if was_enabled:
            gc.enable()
    g.replay()
    torch.cuda.synchronize()
    assert all(_bits(_host(t), e) for t, e in zip(captured, eager))
    x.copy_(_dev(b))                                                    # new contents in the captured input, replayed
    g.replay()
    torch.cuda.synchronize()
    assert all(_bits(_host(t), e) for t, e in zip(captured, other))


# ---------------------------------------------------------------------------------- anomaly_metrics_volume
def _same_number(a, b):
    return (a != a and b != b) or np.float64(a).tobytes() == np.float64(b).tobytes()


RAW_KEYS = ("dice", "precision", "recall", "FPR", "AUC", "AP", "best_dice", "best_threshold", "AUC_status")


def _expected_scores(metrics, mask_v, sq_v, cut_v, thr):
    """The existing functions on one volume as ONE segment: (curve scores of sq_v, scores of cut_v > thr)."""
    mk = _dev(mask_v).reshape(-1)
    o = metrics.curve_scores(mk, _dev(sq_v).reshape(-1), batched=False)
    at = metrics.scores_at(mk, _dev(cut_v).reshape(-1), torch.full((1,), thr, device=DEV), batched=False)
    want = {"AUC": o["auc"], "AP": o["ap"], "best_dice": o["best_dice"], "best_threshold": o["best_threshold"], "AUC_status": o["status"],
            "dice": at["dice"], "precision": at["precision"], "recall": at["recall"], "FPR": at["fpr"]}
    return {k: float(v.reshape(-1)[0]) for k, v in want.items()}


def test_anomaly_metrics_volume_scores_volumes_as_one_segment(kat):
    from anoddpm_amd import metrics
    real, recon, mask = pc.make_scene()
    assert pc.sha(real, recon, mask) == str(kat["scene_in_sha"])
    dr, dc, dm = _dev(real), _dev(recon), _dev(mask)
    raw = metrics.anomaly_metrics_volume(dr, dc, dm)
    assert isinstance(raw, list) and len(raw) == 2
    diff = recon - real
    sq = (diff * diff).astype(np.float32)
    for v, r in enumerate(raw):
        assert set(r) == set(RAW_KEYS) | {"maps"} and set(r["maps"]) == {"sqerr", "pred"}
        assert _bits(_host(r["maps"]["sqerr"]), sq[v]) and _bits(_host(r["maps"]["pred"]) > 0, sq[v] > np.float32(0.5))
        want = _expected_scores(metrics, mask[v], sq[v], sq[v], 0.5)
        assert all(_same_number(r[k], want[k]) for k in RAW_KEYS), (v, {k: (r[k], want[k]) for k in RAW_KEYS})
        assert r["AUC_status"] == 0 and 0 < r["recall"] <= 1 and 0 < r["AUC"] <= 1
    one = metrics.anomaly_metrics_volume(dr[1], dc[1], dm[1])                          # [D, H, W]: one record
    assert isinstance(one, dict) and all(_same_number(one[k], raw[1][k]) for k in RAW_KEYS)

    pp = metrics.VolumePostProcess(median=3, erode=1, roi_level=pc.SCENE_ROI_LEVEL, min_size=7, connectivity=1)
    out = metrics.anomaly_metrics_volume(dr, dc, dm, postprocess=pp)
    sq_pp = pc.median3d_numpy(sq, 3) * pc.erode3d_numpy(real, 1, pc.SCENE_ROI_LEVEL)
    pred_pp = np.stack([pc.components3d_numpy(s, 7, 1, level=0.5)[0] for s in sq_pp])
    assert pc.sha(sq_pp) == str(kat["scene_sqerr_pp_sha"]) and _bits(pred_pp, pc.unpack(kat, "scene_pred_pp", real.shape))
    for v, r in enumerate(out):
        assert set(r) == set(RAW_KEYS) | {k + "_pp" for k in RAW_KEYS} | {"maps"}
        assert set(r["maps"]) == {"sqerr", "pred", "sqerr_pp", "pred_pp"}
        assert all(_same_number(r[k], raw[v][k]) for k in RAW_KEYS)                    # the raw keys and bits are untouched
        assert _bits(_host(r["maps"]["sqerr"]), sq[v])
        assert _bits(_host(r["maps"]["sqerr_pp"]), sq_pp[v]) and _bits(_host(r["maps"]["pred_pp"]), pred_pp[v])
        want = _expected_scores(metrics, mask[v], sq_pp[v], pred_pp[v], 0.5)
        assert all(_same_number(r[k + "_pp"], want[k]) for k in RAW_KEYS), (v, {k: (r[k + "_pp"], want[k]) for k in RAW_KEYS})
        assert r["precision_pp"] == 1.0 and r["FPR_pp"] == 0.0 and r["recall_pp"] == 7 / 27   # only lesion voxels survive

    # the reason this exists: the plane-wise pipeline with the same settings drops the lesion, the volume-wise one keeps it
    pp2 = metrics.PostProcess(median=3, erode=1, roi_level=pc.SCENE_ROI_LEVEL, min_size=7, connectivity=1)
    planes = (-1, 1) + real.shape[-2:]
    f2 = metrics.postprocess_maps(_dev(sq).reshape(planes), pp2, real=dr.reshape(planes))
    pred2 = _host(metrics._small_components(f2, 0.5, 7, 1)[0]).reshape(real.shape)
    pred3 = np.stack([_host(r["maps"]["pred_pp"]) for r in out])
    for sl in pc.SCENE_LESION:
        assert pred3[sl].sum() == 7 and pred2[sl].sum() == 0
    assert pred2.sum() == 0 and pred3.sum() == 14
    for sl in pc.SCENE_SPECK:                                                          # the one-slice speck is alive after the 2-D median only
        assert (_host(f2).reshape(real.shape)[sl] > 0.5).sum() == 5 and not (sq_pp[sl] > 0.5).any()


def test_postprocess_volumes_roi_forms():
    from anoddpm_amd import metrics
    real, recon, mask = pc.make_scene()
    diff = recon - real
    sq = (diff * diff).astype(np.float32)
    d = _dev(sq)
    brain = (real[0, 0] > np.float32(-0.95)).astype(np.float32)                        # one plane: the same column through every slice
    pp = metrics.VolumePostProcess(median=5, erode=2, min_size=0)
    column = np.broadcast_to(brain, real.shape[1:])
    assert _bits(_host(metrics.postprocess_volumes(d, pp, roi=_dev(brain))), pc.median3d_numpy(sq, 5) * pc.erode3d_numpy(column, 2))
    assert _bits(_host(metrics.postprocess_volumes(d, pp)), pc.median3d_numpy(sq, 5))
    off = metrics.VolumePostProcess(median=None, erode=0, min_size=0)
    assert _bits(_host(metrics.postprocess_volumes(d, off, roi=_dev(brain))), sq * brain)
    assert _bits(_host(metrics.postprocess_volumes(d[0], off)), sq[0])


# ---------------------------------------------------------------------------------- argument errors
def test_argument_errors_on_device_tensors():
    from anoddpm_amd import metrics
    x = torch.zeros(2, 4, 16, 16, device=DEV)
    with pytest.raises(ValueError, match="size"):
        metrics.median_filter3d(x, size=7)
    with pytest.raises(ValueError, match="window"):
        metrics.median_filter3d(torch.zeros(8, 4, 16, device=DEV), size=5)
    with pytest.raises(ValueError, match="roi"):
        metrics.median_filter3d(x, roi=torch.ones(3, 16, 16, device=DEV))
    with pytest.raises(TypeError, match="roi"):
        metrics.median_filter3d(x, roi=np.ones((16, 16), np.float32))
    with pytest.raises(ValueError, match="iterations"):
        metrics.erode_mask3d(x, iterations=0)
    with pytest.raises(ValueError, match="connectivity"):
        metrics.remove_small_components3d(x, connectivity=4)
    with pytest.raises(ValueError, match="connectivity"):
        metrics.component_areas3d(x, connectivity=0)
    with pytest.raises(ValueError, match="D, H, W"):
        metrics.erode_mask3d(x[0, 0])
    with pytest.raises(ValueError, match="roi"):
        metrics.postprocess_volumes(x, metrics.VolumePostProcess(), roi=torch.ones(5, 5, device=DEV))
    with pytest.raises(ValueError, match="recon"):
        metrics.anomaly_metrics_volume(x, x[0], x)
