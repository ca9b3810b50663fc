"""-m gpu: the Gaussian filter and the image-level scores (csrc/smooth.hip through metrics.gaussian_filter / image_scores /
image_auc, PostProcess(gaussian=), score_maps(image_top=) and the detection records) against the fixture
tests/golden/smooth_kat.npz (what scipy.ndimage.gaussian_filter returns) and the numpy restatements of tests/smooth_cases.py.
Filter outputs, maxima and the sums in the kernel's order are compared by `tobytes()` equality, no tolerance; the means also
against math.fsum within n * 2^-52 / k * 2^-52.  scipy is not needed."""
import ctypes
import gc
import math
import os

import numpy as np
import pytest
import torch

import smooth_cases as sm
from conftest import GOLDEN
from postproc_cases import erode_numpy, make_roi, median_numpy
from score_cases import PARENT_RECORD_KEYS, bits as _bits, host as _host, tiny as _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IMAGE_RECORD_KEYS = {"image_max", "image_topk"}


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "smooth_kat.npz"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _is_f32_on_device(t, like):
    return t.dtype == torch.float32 and t.shape == like.shape and t.is_cuda and t.device == like.device


# ---------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize("name", sorted(sm.GAUSS))
def test_gaussian_matches_fixture_and_restatement(kat, name):
    from anoddpm_amd import metrics
    _, sigma, truncate, kind = sm.GAUSS[name]
    x = sm.make_gauss_case(name)
    assert sm.sha(x) == str(kat[name + "_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    d = _dev(x)
    out = metrics.gaussian_filter(d, sigma, truncate)                                  # a 2-D tensor: one map
    assert _is_f32_on_device(out, d) and out.is_contiguous()
    got = _host(out)
    sm.check_fixture(kat, name, got)
    assert _bits(got, sm.gaussian_numpy(x, sigma, truncate))
    if kind == "constant":
        assert (got == np.float32(0.7)).all()
    assert _bits(_host(metrics.gaussian_filter(d, sigma, truncate)), got)              # two runs
    assert _bits(_host(metrics.gaussian_filter(d[None, None], sigma, truncate))[0, 0], got)       # [1, 1, H, W]
    assert _bits(_host(metrics.gaussian_filter(d.double(), sigma, truncate)), got)     # other dtypes are converted
    assert _bits(_host(d), x)


def test_gaussian_defaults_are_sigma_4_truncate_4(kat):
    from anoddpm_amd import metrics
    x = sm.make_gauss_case("g37x53")
    sm.check_fixture(kat, "g37x53", _host(metrics.gaussian_filter(_dev(x))))


def test_gaussian_of_planes_behind_a_row_stride(kat):
    from anoddpm_amd import metrics
    buf, planes = sm.make_strided()
    assert sm.sha(buf) == str(kat["strided_in_sha"])
    S, h, w = planes.shape
    dbuf = _dev(buf)
    view = dbuf[:, :h * w].view(S, h, w)
    assert not view.is_contiguous() and view.stride(0) == buf.shape[1] and view.data_ptr() == dbuf.data_ptr()
    out = metrics.gaussian_filter(view, 4.0)
    assert _is_f32_on_device(out, view) and out.is_contiguous()
    sm.check_fixture(kat, "strided", _host(out))
    assert _bits(_host(out), sm.gaussian_numpy(planes, 4.0))
    assert _bits(_host(dbuf), buf)                                                     # the input, padding included, is untouched


def test_gaussian_batch_of_55_equals_single_calls(kat):
    from anoddpm_amd import metrics
    batch = sm.make_batch()
    assert sm.sha(batch) == str(kat["batch_in_sha"])
    d = _dev(batch)
    got = _host(metrics.gaussian_filter(d, 4.0))
    assert got.shape == sm.BATCH_SHAPE and sm.sha(got) == str(kat["batch_out_sha"])
    assert [sm.sha(g) for g in got] == kat["batch_out_plane_sha"].tolist()
    singles = np.stack([_host(metrics.gaussian_filter(d[j, 0], 4.0)) for j in range(sm.BATCH_SHAPE[0])])[:, None]
    assert _bits(singles, got)


def test_a_nan_stays_inside_its_plane(kat):
    from anoddpm_amd import metrics
    bad = sm.make_poison()
    assert sm.sha(bad) == str(kat["poison_in_sha"])
    got = _host(metrics.gaussian_filter(_dev(bad), 4.0))
    clean = [j for j in range(bad.shape[0]) if j != sm.POISON_PLANE]
    assert _bits(got[clean], kat["poison_clean_out"])
    want = sm.gaussian_numpy(bad[sm.POISON_PLANE], 4.0)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert (np.isnan(got[sm.POISON_PLANE]) == np.isnan(want)).all()                    # within its radius, by IEEE rules
    assert _bits(np.nan_to_num(got[sm.POISON_PLANE], nan=-1.0), np.nan_to_num(want, nan=-1.0))


def test_gaussian_argument_errors():
    from anoddpm_amd import _lib, metrics
    d = _dev(sm.make_gauss_case("g5x7"))
    for sigma in (0, 0.0, -4.0, float("nan"), float("inf"), 0.1, 8.2):               # radius 0 at 0.1, 33 at 8.2
        with pytest.raises(ValueError, match="radius"):
            metrics.gaussian_filter(d, sigma)
    with pytest.raises(ValueError, match="radius"):
        metrics.gaussian_filter(d, 4.0, truncate=0.0)
    with pytest.raises(ValueError, match="H, W"):
        metrics.gaussian_filter(d[0], 4.0)
    with pytest.raises(TypeError):
        metrics.gaussian_filter(_host(d), 4.0)
    with pytest.raises(_lib.AnoddpmError):
        metrics.gaussian_filter(d.cpu(), 4.0)

    # direct calls: null pointers and dst == src are refused, nothing is launched and dst keeps its bits
    out = torch.full_like(d, 7.0)
    w = _dev(sm.weights_numpy(4.0)[:17])
    L = _lib.lib()

    def call(**kw):
        a = _lib.GaussArgs()
        a.src, a.dst, a.w, a.src_stride, a.S, a.H, a.W, a.radius = d.data_ptr(), out.data_ptr(), w.data_ptr(), 35, 1, 5, 7, 16
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.anoddpm_gauss2d(ctypes.byref(a), _lib.current_stream())
        return rc, L.anoddpm_last_error().decode()

    for kw, text in (({"src": None}, "null"), ({"dst": None}, "null"), ({"w": None}, "null"), ({"dst": d.data_ptr()}, "overlaps"),
                     ({"dst": d.data_ptr() + 4 * 34}, "overlaps"), ({"radius": 0}, "radius"), ({"radius": 33}, "radius"), ({"H": 0}, "S, H, W")):
        rc, msg = call(**kw)
        assert rc != 0 and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    rc, msg = call()
    assert rc == 0, msg
    assert _bits(_host(out), sm.gaussian_numpy(_host(d), 4.0))


def test_gaussian_graph_replay_gives_the_eager_bits():
    from anoddpm_amd import metrics
    batch = sm.make_batch()
    x = _dev(batch[:8]).clone()
    eager = _host(metrics.gaussian_filter(x, 4.0))                                     # first use: the tap table is on the device now
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()                                                        # no collection of older graphs inside the capture
    try:
        with torch.cuda.graph(g):
            captured = metrics.gaussian_filter(x, 4.0)
    finally:
        if was_enabled:
            gc.enable()
    g.replay()
    torch.cuda.synchronize()
    assert _bits(_host(captured), eager)
    x.copy_(_dev(batch[8:16]))                                          # new contents in the captured input, replayed
    g.replay()
    torch.cuda.synchronize()
    assert _bits(_host(captured), sm.gaussian_numpy(batch[8:16], 4.0))


# ---------------------------------------------------------------------------------- the image scores
def _exact(x, k):
    """(max, mean, top-k mean) with correctly rounded sums (math.fsum); partition, not a full sort: n may be 2^24."""
    v = np.abs(np.asarray(x, np.float32).reshape(-1)).astype(np.float64)
    top = np.partition(v, v.size - k)[v.size - k:]
    return np.float32(v.max()), math.fsum(v) / v.size, math.fsum(top) / k


def _check_scores(o, status, j, x, k):
    n = x.size
    mx, mean, topk = sm.scores_numpy(x, k)
    emx, emean, etopk = _exact(x, k)
    got = {key: _host(o[key])[j] for key in ("max", "mean", "topk")}
    print(n, k, got, emean, etopk)
    assert int(status[j]) == 0
    assert got["max"].dtype == np.float32 and got["mean"].dtype == np.float64 and got["topk"].dtype == np.float64
    assert got["max"].tobytes() == np.float32(mx).tobytes() == emx.tobytes()
    assert got["mean"].tobytes() == np.float64(mean).tobytes() and got["topk"].tobytes() == np.float64(topk).tobytes()
    assert sm.within(float(got["mean"]), emean, n) and sm.within(float(got["topk"]), etopk, k)
    return got


@pytest.mark.parametrize("name", sorted(sm.SCORES))
def test_image_scores_match_restatement_and_exact_sums(name):
    from anoddpm_amd import metrics
    x, k = sm.make_score_case(name)
    d = _dev(x)
    o, status = metrics.image_scores(d, top=k, batched=False, return_status=True)
    assert all(o[key].shape == (1,) and o[key].is_cuda for key in ("max", "mean", "topk")) and set(o) == {"max", "mean", "topk"}
    assert status.dtype == torch.int32 and status.shape == (1,)
    got = _check_scores(o, status, 0, x, k)
    if k == 1:
        assert float(got["topk"]) == float(got["max"])
    if k == x.size:
        assert sm.within(float(got["topk"]), _exact(x, k)[1], x.size)
    if name in ("constant", "zeros"):
        assert float(got["topk"]) == float(got["max"]) == float(x.reshape(-1)[0])
    if name == "tie_at_k":
        assert float(got["topk"]) == (2.0 + 1.75 + 1.5 + 1.5) / 4
    again = metrics.image_scores(d, top=k, batched=False)
    assert all(_bits(_host(again[key]), _host(o[key])) for key in o)                   # two runs


def test_image_scores_batch_fraction_and_stride():
    from anoddpm_amd import metrics
    x = sm._errors(np.random.default_rng(9950), (5, 3, 10, 10))                        # five images of three channels, pooled
    d = _dev(x)
    o, status = metrics.image_scores(d, top=0.05, return_status=True)                  # k = int(0.05 * 300) = 15
    assert o["max"].shape == (5,)
    for j in range(5):
        _check_scores(o, status, j, x[j], 15)
    x50 = sm._errors(np.random.default_rng(9951), (2, 50))
    o, status = metrics.image_scores(_dev(x50), top=0.01, batched=True, return_status=True)       # int(0.5) = 0 -> k = 1
    for j in range(2):
        got = _check_scores(o, status, j, x50[j], 1)
        assert float(got["topk"]) == float(got["max"])
    buf, planes = sm.make_strided()
    dbuf = _dev(buf)
    view = dbuf[:, :planes[0].size]
    o, status = metrics.image_scores(view, top=7, batched=True, return_status=True)
    for j in range(planes.shape[0]):
        _check_scores(o, status, j, planes[j], 7)
    for bad in (0, 51, 0.0, 1.5, -0.1, True, "1"):
        with pytest.raises(ValueError):
            metrics.image_scores(_dev(x50), top=bad, batched=True)


def test_image_scores_largest_segment_and_one_more():
    from anoddpm_amd import metrics
    x = sm._errors(np.random.default_rng(9960), (sm.MAX_N + 1,))
    d = _dev(x)
    k = 4099
    o, status = metrics.image_scores(d[:sm.MAX_N], top=k, batched=False, return_status=True)
    _check_scores(o, status, 0, x[:sm.MAX_N], k)
    with pytest.raises(ValueError, match="exceeds"):
        metrics.image_scores(d, top=k, batched=False)


def test_a_bad_segment_sets_its_own_status_only():
    from anoddpm_amd import _lib, metrics
    bad, which = sm.make_bad_segments()
    clean = np.where(np.isfinite(bad) & (bad >= 0), bad, np.float32(0.5)).astype(np.float32)
    ob, sb = metrics.image_scores(_dev(bad), top=9, return_status=True)
    oc, sc = metrics.image_scores(_dev(clean), top=9, return_status=True)
    bit = {"nan": _lib.ROC_NAN, "inf": _lib.ROC_INF, "negative": _lib.ROC_NEGATIVE}
    assert _host(sc).tolist() == [0] * 6
    assert _host(sb).tolist() == [bit[which[j]] if j in which else 0 for j in range(6)]
    for key in ("max", "mean", "topk"):
        b, c = _host(ob[key]), _host(oc[key])
        for j in range(6):
            if j in which:
                assert np.isnan(b[j])
            else:
                assert b[j].tobytes() == c[j].tobytes(), (key, j)


# ---------------------------------------------------------------------------------- integration
def test_postprocess_maps_with_gaussian():
    from anoddpm_amd import metrics
    x = sm._errors(np.random.default_rng(9970), (3, 1, 40, 48))
    d = _dev(x)
    smooth = metrics.gaussian_filter(d, 4.0)
    assert _bits(_host(smooth), sm.gaussian_numpy(x, 4.0))
    only = metrics.PostProcess(gaussian=4, median=None, erode=0, min_size=0)
    assert _bits(_host(metrics.postprocess_maps(d, only)), _host(smooth))
    both = metrics.PostProcess(gaussian=4, median=3, erode=0, min_size=0)
    got = _host(metrics.postprocess_maps(d, both))
    assert _bits(got, _host(metrics.median_filter(smooth, 3))) and _bits(got, median_numpy(_host(smooth), 3))
    roi = make_roi(40, 48, 9971)
    eroded = erode_numpy(roi, 2)
    assert 0 < eroded.sum() < roi.sum()
    for pp in (metrics.PostProcess(gaussian=4, median=None, erode=2, min_size=0), metrics.PostProcess(gaussian=4, median=3, erode=2, min_size=0)):
        got = _host(metrics.postprocess_maps(d, pp, roi=_dev(roi)))
        inner = _host(smooth) if pp.median is None else median_numpy(_host(smooth), 3)
        assert (got[:, :, eroded == 0] == 0).all() and _bits(got, (inner * eroded).astype(np.float32))
    assert _bits(_host(d), x)


def _stacks(R=3, B=2):
    rng = np.random.default_rng(9980)
    real = (rng.random((B, 1, 32, 32), dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
    mean = (rng.random((R, B, 1, 32, 32), dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
    sqerr = ((mean - real) * (mean - real)).astype(np.float32)
    pred = (sqerr > np.float32(0.5)).astype(np.float32)
    mask = (rng.random((B, 1, 32, 32), dtype=np.float32) > np.float32(0.7)).astype(np.float32)
    return real, mean, sqerr, pred, mask


def test_score_maps_adds_the_image_scores():
    from anoddpm_amd import metrics
    real, mean, sqerr, pred, mask = _stacks()
    R, B = sqerr.shape[:2]
    args = [_dev(a) for a in (real, mean, sqerr, pred, mask)]
    plain = metrics.score_maps(*args)
    o = metrics.score_maps(*args, image_top=0.01)                                      # k = int(0.01 * 1024) = 10
    new = {"image_max", "image_mean", "image_topk", "image_status"}
    assert set(o) == set(plain) | new
    for key in plain:
        assert _bits(_host(o[key]), _host(plain[key])), key
    assert all(o[key].shape == (R, B) for key in new) and (_host(o["image_status"]) == 0).all()
    for r in range(R):
        each = metrics.image_scores(_dev(sqerr[r]), top=0.01, batched=True)
        alone = metrics.score_maps(args[0], *(a[r:r + 1] for a in args[1:4]), args[4], image_top=0.01)
        for key in ("max", "mean", "topk"):
            assert _bits(_host(o["image_" + key][r]), _host(each[key])), (r, key)
            assert _bits(_host(alone["image_" + key][0]), _host(each[key])), (r, key)    # row r whatever the other rows hold
        for b in range(B):
            mx, mn, tk = sm.scores_numpy(sqerr[r, b], 10)
            assert _host(o["image_topk"])[r, b] == tk and _host(o["image_max"])[r, b] == mx and _host(o["image_mean"])[r, b] == mn
    pp = metrics.PostProcess(gaussian=2.0, median=None, erode=0, min_size=0)
    o2 = metrics.score_maps(*args, postprocess=pp, image_top=5)
    base = metrics.score_maps(*args, postprocess=pp)
    assert set(o2) == set(base) | new | {"image_max_pp", "image_mean_pp", "image_topk_pp"}
    smooth = sm.gaussian_numpy(sqerr, 2.0)
    assert _bits(_host(o2["sqerr_pp"]), smooth)
    for r in range(R):
        for b in range(B):
            mx, mn, tk = sm.scores_numpy(smooth[r, b], 5)
            assert _host(o2["image_topk_pp"])[r, b] == tk and _host(o2["image_max_pp"])[r, b] == mx and _host(o2["image_mean_pp"])[r, b] == mn
    # without a mask the image scores are still there
    nomask = metrics.score_maps(*args[:4], None, image_top=0.01)
    assert _bits(_host(nomask["image_topk"]), _host(o["image_topk"]))


def test_anomaly_metrics_image_adds_its_keys_only():
    from anoddpm_amd import metrics
    real, mean, _, _, mask = _stacks()
    x, y, m = _dev(real), _dev(mean[0]), _dev(mask)
    r0 = metrics.anomaly_metrics(x, y, m)
    assert metrics.anomaly_metrics_image(x, y, m, image_top=None).keys() == r0.keys()
    r1 = metrics.anomaly_metrics_image(x, y, m)
    assert set(r1) == set(r0) | {"image_max", "image_mean", "image_topk", "image_status"}
    for k, v in r0.items():
        if k != "maps":
            assert np.float64(v).tobytes() == np.float64(r1[k]).tobytes(), k
    sq = _host(r0["maps"]["sqerr"])
    want = [sm.scores_numpy(sq[b], 10) for b in range(sq.shape[0])]
    assert r1["image_max"] == [float(w[0]) for w in want] and r1["image_mean"] == [w[1] for w in want]
    assert r1["image_topk"] == [w[2] for w in want] and r1["image_status"] == [0, 0]
    r2 = metrics.anomaly_metrics_image(x, y, m, postprocess=metrics.PostProcess(gaussian=4.0), image_top=3)
    assert {"image_max_pp", "image_mean_pp", "image_topk_pp", "AUC_pp"} <= set(r2) and len(r2["image_topk_pp"]) == 2


def test_image_auc_is_the_mann_whitney_count():
    from anoddpm_amd import metrics
    scores = np.array([0.9, 0.1, 0.4, 0.4, 0.7, 0.2], np.float32)
    labels = np.array([1, 0, 1, 0, 0, 1], np.float32)
    two_u = sum(2 * (p > q) + (p == q) for p, lp in zip(scores.tolist(), labels.tolist()) if lp == 1
                for q, lq in zip(scores.tolist(), labels.tolist()) if lq == 0)
    auc, status = metrics.image_auc(_dev(labels), _dev(scores), return_status=True)
    assert auc.shape == (1,) and auc.dtype == torch.float64 and int(status[0]) == 0
    assert two_u == 11 and float(auc[0]) == two_u / (2 * 3 * 3)
    assert float(metrics.image_auc(_dev(labels), _dev(scores.astype(np.float64)))[0]) == float(auc[0])
    for empty in (np.zeros(6, np.float32), np.ones(6, np.float32)):
        assert math.isnan(float(metrics.image_auc(_dev(empty), _dev(scores))[0]))
    with pytest.raises(ValueError):
        metrics.image_auc(_dev(labels[:5]), _dev(scores))


def test_detection_records_carry_the_image_scores(tmp_path, monkeypatch):
    from anoddpm_amd import metrics
    GD, m, d = _tiny(32)
    monkeypatch.chdir(tmp_path)
    g = torch.Generator().manual_seed(5)
    x_0 = (torch.rand(1, 1, 32, 32, generator=g) * 2 - 1).to(DEV)
    mask = (torch.rand(1, 1, 32, 32, generator=g) > 0.7).float().to(DEV)
    args = {"arg_num": 9, "T": 200, "img_size": [32, 32]}                # settings 50, 100, 150

    assert d.image_top is None and "image_top" not in d.__dict__
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    plain = d.last_detection
    assert [r["t_distance"] for r in plain] == [50, 100, 150] and all(set(r) == PARENT_RECORD_KEYS for r in plain)

    d.image_top = 0.01
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    for rec, old in zip(d.last_detection, plain):
        assert set(rec) == PARENT_RECORD_KEYS | IMAGE_RECORD_KEYS
        for k in ("mean", "mse", "threshold", "counts", "auc", "ap", "best_dice", "best_threshold", "ssim", "output"):
            assert _bits(_host(rec[k]), _host(old[k])), k                 # the same chains, the same raw results
        sq = _host(metrics.anomaly_maps(x_0, rec["output"], mask)[0]["sqerr"])
        mx, _, tk = sm.scores_numpy(sq[0], 10)
        assert rec["image_max"].shape == (1,) and rec["image_max"].is_cuda and rec["image_topk"].dtype == torch.float64
        assert float(rec["image_max"][0]) == float(mx) and float(rec["image_topk"][0]) == tk

    d.postprocess = metrics.PostProcess(gaussian=2.0, median=None, erode=0, min_size=0)
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), None, denoise_fn="gauss", total_avg=2)
    for rec in d.last_detection:
        assert IMAGE_RECORD_KEYS | {"image_max_pp", "image_topk_pp", "sqerr_pp"} <= set(rec)
        mx, _, tk = sm.scores_numpy(_host(rec["sqerr_pp"])[0], 10)
        assert float(rec["image_max_pp"][0]) == float(mx) and float(rec["image_topk_pp"][0]) == tk
