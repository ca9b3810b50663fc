"""-m gpu: the native post-processing (csrc/postproc.hip through metrics.median_filter / erode_mask / remove_small_components,
anomaly_metrics and the detection records) against the fixture tests/golden/postproc_kat.npz (what scipy.ndimage returns) and
the numpy restatements of tests/postproc_cases.py.  Every step selects or counts, so every comparison is `tobytes()` equality:
there is no tolerance in this file.  scipy is not needed."""
import gc
import os

import numpy as np
import pytest
import torch

import postproc_cases as pc
from conftest import GOLDEN
from score_cases import PARENT_RECORD_KEYS, PP_RECORD_KEYS, bits as _bits, host as _host, tiny as _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEDIAN_CASES = [(name, k) for name in sorted(pc.MEDIAN) for k in pc.WINDOWS]
ERODE_CASES = [(name, n) for name in sorted(pc.ERODE) for n in pc.ERODE_N]
COMPONENT_CASES = [(name, c) for name in sorted(pc.COMPONENTS) for c in (1, 2)]


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "postproc_kat.npz"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _is_f32_on_device(t, like):
    return t.dtype == torch.float32 and t.shape == like.shape and t.is_cuda and t.device == like.device


# ---------------------------------------------------------------------------------- median
@pytest.mark.parametrize("name,k", MEDIAN_CASES)
def test_median_matches_fixture_and_restatement(kat, name, k):
    from anoddpm_amd import metrics
    x = pc.make_median_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    d = _dev(x)
    out, status = metrics.median_filter(d, size=k, return_status=True)                 # a 2-D tensor: one map
    assert _is_f32_on_device(out, d) and status.dtype == torch.int32 and status.shape == () and int(status) == 0
    got = _host(out)
    pc.check_plane(kat, pc.mkey(name, k), got, name in pc.MEDIAN_FULL)
    assert _bits(got, pc.median_numpy(x, k))
    assert _bits(_host(metrics.median_filter(d, size=k)), got)                         # two runs
    assert _bits(_host(metrics.median_filter(d[None, None], size=k))[0, 0], got)       # [1, 1, H, W]
    assert _bits(_host(metrics.median_filter(d.double(), size=k)), got)                # other dtypes are converted


def test_median_of_planes_behind_a_row_stride(kat):
    from anoddpm_amd import metrics
    buf, planes = pc.make_strided()
    assert pc.sha(buf) == str(kat["strided_in_sha"])
    S, h, w = pc.STRIDED_SHAPE
    dbuf = _dev(buf)
    view = dbuf[:, :h * w].view(S, h, w)
    assert not view.is_contiguous() and view.stride(0) == h * w + pc.STRIDED_PAD and view.data_ptr() == dbuf.data_ptr()
    for k in pc.WINDOWS:
        out = metrics.median_filter(view, size=k)
        assert _is_f32_on_device(out, view) and out.is_contiguous()
        pc.check_plane(kat, pc.mkey("strided", k), _host(out), True)
        assert _bits(_host(out), pc.median_numpy(planes, k))
    assert _bits(_host(dbuf), buf)                                                     # the input, padding included, is untouched


def test_median_batch_of_55_with_one_shared_roi(kat):
    from anoddpm_amd import metrics
    maps, roi = pc.make_batch()
    assert pc.sha(maps, roi) == str(kat["batch_in_sha"])
    d, r = _dev(maps), _dev(roi)
    out, status = metrics.median_filter(d, size=5, roi=r, return_status=True)
    assert _is_f32_on_device(out, d) and status.shape == (pc.BATCH, 1) and not bool(status.any())
    got = _host(out)
    assert [pc.sha(g) for g in got] == [str(s) for s in kat["batch_k5_plane_sha"]] and pc.sha(got) == str(kat["batch_k5_sha"])
    for j in (0, 27, 54):
        for cname, sl in pc.crops(256, 256).items():
            assert _bits(got[j, 0][sl], kat[f"batch_k5_{j}_{cname}"]), (j, cname)
    assert _bits(got, pc.median_numpy(maps, 5) * roi)
    # +0.0 outside the region of interest: every bit zero
    assert (got.view(np.uint32)[:, 0][:, roi == 0] == 0).all() and (got[:, 0][:, roi == 1] > 0).any()
    # the same bits from per-plane calls, from the ROI in the other two shapes, and from a second run
    for j in (0, 27, 54):
        assert _bits(_host(metrics.median_filter(d[j], size=5, roi=r)), got[j])
        assert _bits(_host(metrics.median_filter(d[j, 0], size=5, roi=r)), got[j, 0])
    assert _bits(_host(metrics.median_filter(d, size=5, roi=r[None])), got)            # one segment [1, 256, 256]
    assert _bits(_host(metrics.median_filter(d, size=5, roi=r.expand(pc.BATCH, 1, 256, 256))), got)
    assert _bits(_host(metrics.median_filter(d, size=5, roi=r)), got)
    # without the ROI the inside is the same and the outside is the plain median
    plain = _host(metrics.median_filter(d, size=5))
    assert _bits(plain * roi, got) and _bits(plain[3], pc.median_numpy(maps[3], 5))


def test_a_bad_plane_sets_its_own_status_only(kat):
    from anoddpm_amd import _lib, metrics
    bad = pc.make_bad_batch()
    assert pc.sha(bad) == str(kat["bad_in_sha"])
    out, status = metrics.median_filter(_dev(bad), size=5, return_status=True)         # [6, 32, 48]: six segments of one plane
    want = {"nan": _lib.ROC_NAN, "inf": _lib.ROC_INF, "negative": _lib.ROC_NEGATIVE}
    assert status.tolist() == [want[pc.BAD_PLANES[j]] if j in pc.BAD_PLANES else 0 for j in range(6)]
    clean = [j for j in range(6) if j not in pc.BAD_PLANES]
    assert _bits(_host(out)[clean], kat["bad_k5_clean"])
    # a region of interest that is not 0 / 1: its own bit, on every plane that shares it
    roi = np.ones((32, 48), np.float32)
    roi[4, 4] = 0.5
    _, status = metrics.median_filter(_dev(bad), size=3, roi=_dev(roi), return_status=True)
    assert [s & _lib.ROC_BAD_MASK for s in status.tolist()] == [_lib.ROC_BAD_MASK] * 6
    assert [s & ~_lib.ROC_BAD_MASK for s in status.tolist()] == [want[pc.BAD_PLANES[j]] if j in pc.BAD_PLANES else 0 for j in range(6)]
    # -0.0 is a valid score and is reported as +0.0
    z = torch.full((9, 9), -0.0, device=DEV)
    out, status = metrics.median_filter(z, size=3, return_status=True)
    assert int(status) == 0 and (_host(out).view(np.uint32) == 0).all()


def test_median_argument_errors():
    from anoddpm_amd import metrics
    x = torch.zeros(2, 16, 16, device=DEV)
    with pytest.raises(ValueError, match="size"):
        metrics.median_filter(x, size=9)
    with pytest.raises(ValueError, match="window"):
        metrics.median_filter(torch.zeros(6, 40, device=DEV), size=7)
    with pytest.raises(ValueError, match="roi"):
        metrics.median_filter(x, roi=torch.ones(16, 8, device=DEV))
    with pytest.raises(ValueError, match="segment"):
        metrics.median_filter(torch.zeros(4, 256, device=DEV), batched=True)
    assert metrics.median_filter(x, size=3, batched=False).shape == x.shape


# ---------------------------------------------------------------------------------- erosion
@pytest.mark.parametrize("name,n", ERODE_CASES)
def test_erosion_matches_fixture_and_restatement(kat, name, n):
    from anoddpm_amd import metrics
    x, level = pc.make_erode_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    d = _dev(x)
    out = metrics.erode_mask(d, iterations=n, level=level)
    assert _is_f32_on_device(out, d)
    got = _host(out)
    want = np.unpackbits(kat[pc.ekey(name, n) + "_bits"])[:x.size].reshape(x.shape).astype(np.float32)
    assert _bits(got, want), f"{int((got != want).sum())} pixels differ"
    assert pc.sha(got) == str(kat[pc.ekey(name, n) + "_sha"]) and _bits(got, pc.erode_numpy(x, n, level))
    assert _bits(_host(metrics.erode_mask(d, iterations=n, level=level)), got)
    # the thresholded mask itself, eroded at the default level, is the same thing
    assert _bits(_host(metrics.erode_mask((d > level).float(), iterations=n)), got)


def test_erosion_of_a_stack_equals_per_plane_calls():
    from anoddpm_amd import metrics
    planes = [pc.make_erode_case("e64")[0], pc.make_erode_case("e64")[0][::-1].copy(), np.ones((64, 64), np.float32),
              np.zeros((64, 64), np.float32)]
    d = _dev(np.stack(planes).reshape(2, 2, 64, 64))
    out = metrics.erode_mask(d, iterations=3, level=0.25)
    assert _is_f32_on_device(out, d)
    for j, p in enumerate(planes):
        assert _bits(_host(out).reshape(4, 64, 64)[j], pc.erode_numpy(p, 3, 0.25))
    assert _bits(_host(metrics.erode_mask(d, iterations=3)).reshape(4, 64, 64)[2], pc.erode_numpy(planes[2], 3))
    nan = torch.full((16, 16), float("nan"), device=DEV)
    assert not bool(metrics.erode_mask(nan, iterations=1).any())                       # NaN is above no level
    with pytest.raises(ValueError, match="iterations"):
        metrics.erode_mask(d, iterations=9)


# ---------------------------------------------------------------------------------- small components
@pytest.mark.parametrize("name,connectivity", COMPONENT_CASES)
def test_small_components_match_fixture_and_restatement(kat, name, connectivity):
    from anoddpm_amd import metrics
    x = pc.make_components_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    d = _dev(x)
    lab = pc.labels_numpy(x > 0, connectivity)
    for m in pc.COMPONENTS[name]:
        key = pc.ckey(name, connectivity, m)
        out, counts = metrics.remove_small_components(d, min_size=m, connectivity=connectivity, return_counts=True)
        assert _is_f32_on_device(out, d) and counts.dtype == torch.int64 and counts.shape == (2,) and counts.is_cuda
        got = _host(out)
        print(f"{key}: components found / kept {counts.tolist()}, fixture {kat[key + '_counts'].tolist()}, pixels kept {int(got.sum())}")
        assert counts.tolist() == kat[key + "_counts"].tolist(), key
        assert pc.sha(got) == str(kat[key + "_sha"]), key
        want, wcounts = pc.components_numpy(x, m, connectivity, labels=lab)
        assert _bits(got, want) and tuple(counts.tolist()) == wcounts
        if name in pc.COMPONENTS_FULL:
            assert _bits(got, np.unpackbits(kat[key + "_bits"])[:x.size].reshape(x.shape).astype(np.float32))
        again, counts2 = metrics.remove_small_components(d, min_size=m, connectivity=connectivity, return_counts=True)
        assert _bits(_host(again), got) and counts2.tolist() == counts.tolist()         # two runs
    assert _bits(_host(metrics.remove_small_components(d, min_size=1)), x)              # min_size 1 keeps everything
    assert _bits(_host(d), x)                                                           # the input is untouched


def test_small_components_of_a_stack_equal_per_plane_calls(kat):
    from anoddpm_amd import metrics
    names = ("empty", "full", "spiral", "blobs")
    planes = [pc.make_components_case(n) for n in names]
    d = _dev(np.stack(planes).reshape(2, 2, 256, 256))
    for connectivity in (1, 2):
        out, counts = metrics.remove_small_components(d, min_size=7, connectivity=connectivity, return_counts=True)
        assert _is_f32_on_device(out, d) and counts.shape == (2, 2, 2)
        for j, n in enumerate(names):
            key = pc.ckey(n, connectivity, 7)
            assert pc.sha(_host(out).reshape(4, 256, 256)[j]) == str(kat[key + "_sha"]), key
            assert counts.reshape(4, 2)[j].tolist() == kat[key + "_counts"].tolist(), key
    one = torch.ones(1, 1, device=DEV)
    out, counts = metrics.remove_small_components(one, min_size=1, return_counts=True)
    assert out.tolist() == [[1.0]] and counts.tolist() == [1, 1]
    out, counts = metrics.remove_small_components(one, min_size=2, return_counts=True)
    assert out.tolist() == [[0.0]] and counts.tolist() == [1, 0]


def test_graph_replay_gives_the_eager_bits(kat):
    from anoddpm_amd import metrics
    maps, roi = pc.make_batch()
    x, r = _dev(maps[:8]).clone(), _dev(roi)

    def run():
        f = metrics.median_filter(x, size=5, roi=metrics.erode_mask(r, iterations=3))
        p, c = metrics._small_components(f, 0.05, 7, 1)
        return f, p, c

    eager = [_host(t) for t in run()]
    x.copy_(_dev(maps[8:16]))
    other = [_host(t) for t in run()]
    x.copy_(_dev(maps[:8]))
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
    x.copy_(_dev(maps[8:16]))                                           # new contents in the captured input, replayed
    g.replay()
    torch.cuda.synchronize()
    assert all(_bits(_host(t), e) for t, e in zip(captured, other))


# ---------------------------------------------------------------------------------- anomaly_metrics
def _float_bits(v):
    return np.float64(v).tobytes()


def _scene():
    """real / recon / mask [2, 1, 96, 80]: a -1 background round an ellipse, a lesion the reconstruction misses, speckle."""
    rng = np.random.default_rng(9500)
    i, j = np.meshgrid(np.arange(96, dtype=np.float64), np.arange(80, dtype=np.float64), indexing="ij")
    inside = ((i - 47.5) / 42.0) ** 2 + ((j - 39.5) / 33.0) ** 2 <= 1.0
    real = np.where(inside, rng.random((2, 1, 96, 80), dtype=np.float32) * np.float32(0.6) - np.float32(0.3), np.float32(-1)).astype(np.float32)
    recon = (real + (rng.random(real.shape, dtype=np.float32) - np.float32(0.5)) * np.float32(0.3)).astype(np.float32)
    mask = np.zeros(real.shape, np.float32)
    mask[0, 0, 30:44, 25:41] = 1
    mask[1, 0, 50:70, 30:38] = 1
    real = np.where(mask == 1, np.float32(0.9), real).astype(np.float32)               # bright lesion, reconstructed as healthy tissue
    speckle = rng.random(real.shape, dtype=np.float32) < np.float32(0.01)
    recon = np.where(speckle, np.float32(1.0), recon).astype(np.float32)               # isolated large errors
    return real, recon, mask


def _check_pp(r0, r1, real, mask, pp, roi_np, threshold):
    """r1 = anomaly_metrics(..., postprocess=pp) against r0 (without): old keys bit-equal, new ones from the restatement."""
    from anoddpm_amd import metrics
    for k, v in r0.items():
        if k == "maps":
            assert set(r1["maps"]) == set(v) | {"sqerr_pp", "pred_pp"}
            for name, t in v.items():
                assert torch.equal(t, r1["maps"][name]) and t.dtype == r1["maps"][name].dtype, name
        else:
            assert type(v) is type(r1[k]) and _float_bits(v) == _float_bits(r1[k]), k
    assert set(r1) == set(r0) | {"AUC_pp", "AP_pp", "best_dice_pp", "best_threshold_pp", "AUC_pp_status", "dice_pp", "precision_pp",
                                "recall_pp"}
    sq = _host(r0["maps"]["sqerr"])
    filt = pc.median_numpy(sq, pp.median) if pp.median is not None else sq.copy()
    if roi_np is not None:
        filt = (filt * roi_np).astype(np.float32)
    got = r1["maps"]["sqerr_pp"]
    assert _is_f32_on_device(got, r0["maps"]["sqerr"]) and _bits(_host(got), filt)
    pred = np.stack([pc.components_numpy(p, pp.min_size, pp.connectivity, level=threshold)[0] for p in filt.reshape(-1, *filt.shape[-2:])])
    pred = pred.reshape(filt.shape)
    assert _is_f32_on_device(r1["maps"]["pred_pp"], got) and _bits(_host(r1["maps"]["pred_pp"]), pred)
    # the existing functions on the restatement's maps
    f, m = _dev(filt), _dev(mask)
    assert _float_bits(r1["AUC_pp"]) == _float_bits(float(metrics.roc_auc(m, f, batched=False)[0]))
    assert _float_bits(r1["AP_pp"]) == _float_bits(float(metrics.average_precision(m, f, batched=False)[0]))
    best = metrics.best_dice(m, f, batched=False)
    assert _float_bits(r1["best_dice_pp"]) == _float_bits(float(best["dice"][0]))
    assert _float_bits(r1["best_threshold_pp"]) == _float_bits(float(best["threshold"][0])) and r1["AUC_pp_status"] == 0
    _, counts = metrics.anomaly_maps(_dev(np.zeros_like(pred)), _dev(pred), m, threshold=0.5, want=())
    ratios = metrics._ratios(counts.cpu())
    for key in ("dice", "precision", "recall"):
        assert isinstance(r1[key + "_pp"], float) and _float_bits(r1[key + "_pp"]) == _float_bits(float(ratios[key])), key
    print({k: v for k, v in r1.items() if k != "maps"})


def test_anomaly_metrics_adds_the_postprocessed_scores_and_keeps_the_rest():
    from anoddpm_amd import metrics
    real, recon, mask = _scene()
    x, y, m = _dev(real), _dev(recon), _dev(mask)
    r0 = metrics.anomaly_metrics(x, y, m)
    # region of interest from the image itself: real > -0.9, eroded three times
    pp = metrics.PostProcess(median=5, erode=3, roi_level=-0.9, min_size=7, connectivity=1)
    r1 = metrics.anomaly_metrics(x, y, m, postprocess=pp)
    _check_pp(r0, r1, real, mask, pp, pc.erode_numpy(real, 3, -0.9), 0.5)
    assert r1["dice_pp"] > r0["dice"] and r1["AP_pp"] > r0["AP"]                       # the speckle is gone
    # a region of interest handed in, other settings, another threshold
    roi = pc.make_roi(96, 80, 9501)
    pp2 = metrics.PostProcess(median=3, erode=1, min_size=30, connectivity=2)
    r0b = metrics.anomaly_metrics(x, y, m, threshold=0.3)
    r2 = metrics.anomaly_metrics(x, y, m, threshold=0.3, postprocess=pp2, roi=_dev(roi))
    _check_pp(r0b, r2, real, mask, pp2, pc.erode_numpy(roi, 1), 0.3)
    # everything switched off: the raw map again
    off = metrics.PostProcess(median=None, erode=0, min_size=0)
    r3 = metrics.anomaly_metrics(x, y, m, postprocess=off)
    _check_pp(r0, r3, real, mask, off, None, 0.5)
    assert _float_bits(r3["AUC_pp"]) == _float_bits(r0["AUC"]) and _float_bits(r3["dice_pp"]) == _float_bits(r0["dice"])
    assert torch.equal(r3["maps"]["pred_pp"], r0["maps"]["pred"])
    with pytest.raises(ValueError, match="real image|roi_level"):
        metrics.postprocess_maps(r0["maps"]["sqerr"], pp)


def test_postprocess_maps_launches_once_per_step(monkeypatch):
    """One erosion launch and one median launch for a whole sweep, whatever its size."""
    from anoddpm_amd import _lib, metrics
    maps, roi = pc.make_batch()
    d, r = _dev(maps[:6]), _dev(roi)
    L = _lib.lib()
    calls = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(L, name)
            if name in ("anoddpm_median2d", "anoddpm_erode2d", "anoddpm_small_components", "anoddpm_roc_auc"):
                def wrapped(*a):
                    calls.append(name)
                    return fn(*a)
                return wrapped
            return fn

    monkeypatch.setattr(metrics, "lib", Spy)
    out = metrics.postprocess_maps(d, metrics.PostProcess(5, 3), roi=r)
    monkeypatch.undo()
    assert calls == ["anoddpm_erode2d", "anoddpm_median2d"]
    assert _bits(_host(out), pc.median_numpy(maps[:6], 5) * pc.erode_numpy(roi, 3))


# ---------------------------------------------------------------------------------- detection records
def test_detection_records_carry_the_postprocessed_scores(tmp_path, monkeypatch):
    from anoddpm_amd import metrics
    GD, m, d = _tiny(32)
    monkeypatch.chdir(tmp_path)
    g = torch.Generator().manual_seed(5)
    x_0 = (torch.rand(1, 1, 32, 32, generator=g) * 2 - 1).to(DEV)
    x_0[:, :, :3] = -1.0                                                 # some background for the ROI level to cut
    mask = (torch.rand(1, 1, 32, 32, generator=g) > 0.7).float().to(DEV)
    args = {"arg_num": 9, "T": 200, "img_size": [32, 32]}                # settings 50, 100, 150

    # unset: exactly the keys of the parent commit
    assert d.postprocess is None and d.postprocess_roi is None
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    plain = d.last_detection
    assert [r["t_distance"] for r in plain] == [50, 100, 150] and all(set(r) == PARENT_RECORD_KEYS for r in plain)

    d.postprocess = pp = metrics.PostProcess(median=3, erode=2, roi_level=-0.95)
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    recs = d.last_detection
    roi = pc.erode_numpy(_host(x_0)[0, 0], 2, -0.95)
    assert 0 < roi.sum() < roi.size
    for rec, old in zip(recs, plain):
        assert set(rec) == PARENT_RECORD_KEYS | PP_RECORD_KEYS
        for k in ("mean", "mse", "threshold", "counts", "auc", "ap", "best_dice", "best_threshold", "ssim", "output"):
            assert _bits(_host(rec[k]), _host(old[k])), k                 # the same chains, the same raw results
        sq = metrics.anomaly_maps(x_0, rec["output"], mask)[0]["sqerr"]
        want = (pc.median_numpy(_host(sq), 3) * roi).astype(np.float32)
        assert _is_f32_on_device(rec["sqerr_pp"], sq) and _bits(_host(rec["sqerr_pp"]), want)
        f = _dev(want)
        for key, fn in (("auc_pp", metrics.roc_auc), ("ap_pp", metrics.average_precision)):
            assert rec[key].is_cuda and rec[key].dtype == torch.float64 and rec[key].shape == ()
            assert _bits(_host(rec[key]), _host(fn(mask, f, batched=False)[0])), key
        best = metrics.best_dice(mask, f, batched=False)
        assert _bits(_host(rec["best_dice_pp"]), _host(best["dice"][0])) and _bits(_host(rec["best_threshold_pp"]), _host(best["threshold"][0]))
        print(rec["t_distance"], float(rec["auc"]), float(rec["auc_pp"]), float(rec["ap"]), float(rec["ap_pp"]))

    # a region of interest handed in wins over the level; without a mask the map is still there and the scores are None
    d.postprocess_roi = torch.ones(32, 32, device=DEV)
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), None, denoise_fn="gauss", total_avg=2)
    for rec in d.last_detection:
        assert set(rec) == PARENT_RECORD_KEYS | PP_RECORD_KEYS
        assert rec["auc_pp"] is None and rec["ap_pp"] is None and rec["best_dice_pp"] is None and rec["best_threshold_pp"] is None
        sq = metrics.anomaly_maps(x_0, rec["output"], None)[0]["sqerr"]
        assert _bits(_host(rec["sqerr_pp"]), (pc.median_numpy(_host(sq), 3) * pc.erode_numpy(np.ones((32, 32), np.float32), 2)).astype(np.float32))

    # unset again: the parent's keys again
    d.postprocess = None
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert all(set(r) == PARENT_RECORD_KEYS for r in d.last_detection)
    assert not os.listdir(tmp_path)
