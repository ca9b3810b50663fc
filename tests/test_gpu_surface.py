"""-m gpu: the native distance transform and boundary distances (anoddpm_distance_transform / anoddpm_surface_distance of
csrc/surface.hip through metrics.distance_transform / surface_distance / HD95, anomaly_metrics_surface and the detection records)
against the restatements of tests/surface_cases.py: squared distances equal to the integer brute-force minimum, distances bit-equal
to scipy.ndimage.distance_transform_edt, border counts and largest squared distances equal, percentiles bit-equal to the header's
definition and within 8 ulp of numpy.percentile, means bit-equal to the kernel-order restatement and within n * 2^-52 * dmax of
the math.fsum value, the same bits on every launch and wherever a plane sits in a batch."""
import os

import numpy as np
import pytest
import torch

import surface_cases as sc
from conftest import GOLDEN
from score_cases import PARENT_METRIC_KEYS, PARENT_RECORD_KEYS, PP_METRIC_KEYS, PP_RECORD_KEYS, bits_any_nan as _bits, host as _host, tiny as _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SURFACE_METRIC_KEYS = {"HD", "HD95", "ASSD", "HD95_valid", "surface_status"}


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "surface_kat.npz"))


@pytest.fixture(scope="module")
def transform_cases():
    return sc.transform_cases()


@pytest.fixture(scope="module")
def surface_cases():
    return sc.surface_cases()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ---------------------------------------------------------------------------------- distance transform
@pytest.mark.parametrize("name", sc.SMALL_TRANSFORM + sc.LARGE_TRANSFORM)
def test_transform_equals_brute_force_and_scipy(kat, transform_cases, name):
    from anoddpm_amd import metrics
    planes, level = transform_cases[name]
    fg = sc.foreground(planes, level)
    if name in sc.SMALL_TRANSFORM:
        assert _bits(fg.astype(np.uint8), kat[f"dt_{name}_fg"])
        want_sq = kat[f"dt_{name}_sq"]
    else:
        want_sq = np.stack([sc.edt2_brute(f) for f in fg]).astype(np.int32)
    want = np.stack([sc.edt_scipy(f) if not f.all() else np.full(f.shape, np.inf) for f in fg])
    assert sc.sha(fg.astype(np.uint8), want_sq, want) == str(kat[f"dt_{name}_sha"])          # what the fixture froze
    x = _dev(planes)
    sq = metrics.distance_transform(x, level=level, squared=True)
    dist = metrics.distance_transform(x, level=level)
    assert sq.dtype == torch.int32 and dist.dtype == torch.float64 and sq.is_cuda and dist.is_cuda
    assert tuple(sq.shape) == planes.shape == tuple(dist.shape)
    bad = np.flatnonzero(_host(sq).reshape(-1) != want_sq.reshape(-1))
    assert bad.size == 0, (name, bad[:8], _host(sq).reshape(-1)[bad[:8]], want_sq.reshape(-1)[bad[:8]])
    assert _bits(_host(dist), want), (name, np.abs(_host(dist) - want).max())
    again = metrics.distance_transform(x, level=level)
    assert _bits(_host(again), _host(dist))
    if name == "all_fg_mid":
        assert (_host(sq)[1] == -1).all() and np.isinf(_host(dist)[1]).all() and (_host(sq)[[0, 2]] >= 0).all()
        # a plane on its own, as a 2-D tensor, gives what it gives inside the batch
        for s in (0, 2):
            assert _bits(_host(metrics.distance_transform(x[s], level=level)), _host(dist)[s])
    if name == "corner64":
        assert int(sq.max()) == 2 * 63 * 63


def test_transform_takes_any_stack_of_planes_and_other_dtypes(transform_cases):
    from anoddpm_amd import metrics
    planes, level = transform_cases["rand40x33"]
    x = _dev(planes)
    want = _host(metrics.distance_transform(x))
    assert _bits(_host(metrics.distance_transform(x.reshape(2, 1, 40, 33))).reshape(2, 40, 33), want)
    assert _bits(_host(metrics.distance_transform(x.bool())), want) and _bits(_host(metrics.distance_transform(x.double(), batched=True)), want)
    with pytest.raises(ValueError):
        metrics.distance_transform(x.reshape(-1))


# ---------------------------------------------------------------------------------- boundary distances
def _check_pair(got, s, p, r, tag):
    """Entry s of a surface_distance result against the restatements of the pair (p, r)."""
    want, order = sc.surface_ref(p, r), sc.surface_fp64(p, r)
    g = {k: _host(v)[s] for k, v in got.items()}
    print(tag, {k: g[k].tolist() for k in ("counts", "max2", "mean", "p95", "status")})
    assert int(g["status"]) == want["status"], tag
    assert np.array_equal(g["counts"], want["counts"]) and np.array_equal(g["max2"], want["max2"]), (tag, g["counts"], want["counts"], g["max2"], want["max2"])
    if want["status"]:
        assert np.isnan(g["mean"]).all() and np.isnan(g["p95"]).all() and all(np.isnan(g[k]) for k in ("hd", "hd95", "assd")), tag
        return
    assert _bits(g["p95"], want["p95"]), (tag, g["p95"], want["p95"])
    assert _bits(g["mean"], order["mean"]), (tag, g["mean"], order["mean"])
    _, _, d_pr, d_rp = sc.directed(p, r)
    for d, gm, wm in zip((d_pr, d_rp), g["mean"], want["mean"]):
        assert abs(gm - wm) <= d.size * 2.0 ** -52 * np.sqrt(np.float64(d.max())), (tag, gm, wm)
    for d, q in zip((d_pr, d_rp, np.r_[d_pr, d_rp]), g["p95"]):
        assert sc.ulps(q, np.percentile(np.sqrt(d.astype(np.float64)), 95)) <= 8, tag
    assert _bits(g["hd"], np.float64(want["hd"])) and _bits(g["hd95"], np.float64(want["hd95"])) and _bits(g["assd"], np.float64(order["assd"])), tag


@pytest.mark.parametrize("name", sc.SMALL_SURFACE + sc.LARGE_SURFACE)
def test_surface_distance_against_the_restatements(kat, surface_cases, name):
    from anoddpm_amd import metrics
    pred, ref = surface_cases[name]
    if name in sc.SMALL_SURFACE:
        assert _bits(pred.astype(np.uint8), kat[f"sd_{name}_pred"]) and _bits(ref.astype(np.uint8), kat[f"sd_{name}_ref"])
    else:
        assert sc.sha(pred, ref) == str(kat[f"sd_{name}_sha"])
    got, status = metrics.surface_distance(_dev(pred), _dev(ref), return_status=True)
    S = pred.shape[0]
    assert set(got) == {"hd", "hd95", "assd", "p95", "mean", "max2", "counts", "status"} and status is got["status"]
    assert all(v.is_cuda for v in got.values())
    assert [tuple(got[k].shape) for k in ("hd", "hd95", "assd", "status", "p95", "mean", "max2", "counts")] == [(S,)] * 4 + [(S, 3), (S, 2), (S, 2), (S, 2)]
    assert [got[k].dtype for k in ("hd", "p95", "mean", "max2", "counts", "status")] == [torch.float64] * 3 + [torch.int32] * 3
    for s, (p, r) in enumerate(sc.pairs_of(pred, ref)):
        _check_pair(got, s, p, r, f"{name}[{s}]")
        for k in ("counts", "max2", "p95"):                                                # what the fixture froze
            assert _bits(_host(got[k])[s], kat[f"sd_{name}_{k}"][s]), (name, s, k)
    again = metrics.surface_distance(_dev(pred), _dev(ref))
    assert all(_bits(_host(again[k]), _host(got[k])) for k in got), name
    if name == "identical":
        assert not _host(got["max2"]).any() and float(got["hd"][0]) == 0.0 and float(got["assd"][0]) == 0.0
    if name == "corners64":
        assert _host(got["max2"]).tolist() == [[2 * 63 * 63] * 2]
    if name == "batch6_shared":
        assert _host(status).tolist() == [0, 0, 1, 0, 0, 0]
        # every plane on its own, and the batch with its reference repeated: the same bits
        for s in range(S):
            alone = metrics.surface_distance(_dev(pred[s]), _dev(ref))
            assert all(tuple(alone[k].shape) == tuple(got[k].shape[1:]) for k in got)
            assert all(_bits(_host(alone[k]), _host(got[k])[s]) for k in got), s
        own = metrics.surface_distance(_dev(pred), _dev(np.repeat(ref[None], S, axis=0)))
        assert all(_bits(_host(own[k]), _host(got[k])) for k in got)
        lead = metrics.surface_distance(_dev(pred).reshape(2, 3, 24, 20), _dev(ref))      # any stack of planes
        assert all(_bits(_host(lead[k]).reshape(_host(got[k]).shape), _host(got[k])) for k in got)
    if name == "empty_ref":
        assert _host(status).tolist() == [2] and _host(got["counts"])[0, 0] > 0
        both = metrics.surface_distance(torch.zeros(16, 16, device=DEV), torch.zeros(16, 16, device=DEV))
        assert int(both["status"]) == 3 and _host(both["counts"]).tolist() == [0, 0]


def test_level_thresholds_an_image_and_HD95_is_a_python_float(surface_cases):
    from anoddpm_amd import metrics
    pred, ref = surface_cases["blobs40x33"]
    rng = np.random.default_rng(3)
    img = np.where(pred > 0, 0.6 + 0.4 * rng.random(pred.shape), 0.6 * rng.random(pred.shape)).astype(np.float32)
    img_ref = np.where(ref > 0, 0.61, 0.3).astype(np.float32)
    want = metrics.surface_distance(_dev(pred), _dev(ref))
    got = metrics.surface_distance(_dev(img), _dev(img_ref), level=0.6)
    assert all(_bits(_host(got[k]), _host(want[k])) for k in want)
    h = metrics.HD95(_dev(ref), _dev(pred))
    assert isinstance(h, float) and _bits(np.float64(h), _host(want["hd95"])[0])
    six, shared = surface_cases["batch6_shared"]
    o = metrics.surface_distance(_dev(six), _dev(shared))
    valid = _host(o["hd95"])[[0, 1, 3, 4, 5]]
    h = metrics.HD95(_dev(shared), _dev(six))
    assert abs(h - valid.mean()) <= 4 * np.spacing(valid.max())
    assert np.isnan(metrics.HD95(torch.zeros(8, 8, device=DEV), torch.ones(8, 8, device=DEV)))


def test_wrong_arguments_raise_as_the_sibling_functions_do():
    from anoddpm_amd import _lib, metrics
    x = torch.zeros(2, 8, 8, device=DEV)
    with pytest.raises(TypeError):
        metrics.surface_distance(x, np.zeros((8, 8), np.float32))
    with pytest.raises(TypeError):
        metrics.distance_transform([[0.0]])
    with pytest.raises(_lib.AnoddpmError, match="no CPU fallback"):
        metrics.surface_distance(x, torch.zeros(8, 8))
    with pytest.raises(_lib.AnoddpmError, match="no CPU fallback"):
        metrics.distance_transform(torch.zeros(8, 8))
    with pytest.raises(ValueError, match="neither the shape"):
        metrics.surface_distance(x, torch.zeros(3, 8, 8, device=DEV))
    with pytest.raises(ValueError, match="neither the shape"):
        metrics.surface_distance(x, torch.zeros(8, 9, device=DEV))
    with pytest.raises(ValueError):
        metrics.surface_distance(torch.zeros(8, device=DEV), torch.zeros(8, device=DEV))
    # another dtype is converted, as the sibling functions do
    m = torch.zeros(8, 8, device=DEV)
    m[2:6, 2:6] = 1
    a, b = metrics.surface_distance(m, m.roll(1, 0)), metrics.surface_distance(m.bool(), m.roll(1, 0).to(torch.int64))
    assert all(_bits(_host(a[k]), _host(b[k])) for k in a) and float(a["hd"]) == 1.0


# ---------------------------------------------------------------------------------- anomaly_metrics_surface
def _scene():
    """real / recon / mask [2, 1, 48, 40]: a lesion the reconstruction misses in image 0, none in image 1 (an empty reference)."""
    rng = np.random.default_rng(21)
    real = (rng.random((2, 1, 48, 40)) * 1.6 - 0.8).astype(np.float32)
    mask = np.zeros_like(real)
    mask[0, 0, 5:25, 4:22] = 1
    mask[0, 0, 40:42, 30:33] = 1
    shifted = np.roll(mask, (2, 3), (2, 3))
    shifted[1, 0, 20:24, 10:14] = 1
    recon = real + (rng.random(real.shape).astype(np.float32) - 0.5) * 0.2 + shifted * (0.9 + 0.3 * rng.random(real.shape).astype(np.float32))
    return _dev(real), _dev(recon.astype(np.float32)), _dev(mask)


def test_anomaly_metrics_surface_adds_keys_and_nothing_else():
    from anoddpm_amd import metrics
    real, recon, mask = _scene()
    plain = metrics.anomaly_metrics(real, recon, mask)
    assert set(plain) == PARENT_METRIC_KEYS
    r = metrics.anomaly_metrics_surface(real, recon, mask)
    assert set(r) == PARENT_METRIC_KEYS | SURFACE_METRIC_KEYS
    for k in PARENT_METRIC_KEYS - {"maps"}:
        assert _bits(np.float64(r[k]), np.float64(plain[k])), k
    pred = r["maps"]["pred"]
    o = metrics.surface_distance(pred, mask)
    assert _host(o["status"]).reshape(-1).tolist() == [0, 2]
    assert (r["HD95_valid"], r["surface_status"]) == (1, 2)
    for key, src in (("HD", "hd"), ("HD95", "hd95"), ("ASSD", "assd")):
        assert isinstance(r[key], float) and _bits(np.float64(r[key]), _host(o[src])[0, 0]), key
    want = sc.surface_ref(_host(pred)[0, 0], _host(mask)[0, 0])
    assert _bits(np.float64(r["HD"]), np.float64(want["hd"])) and _bits(np.float64(r["HD95"]), np.float64(want["hd95"])) and r["HD"] > 0
    # the filtered prediction beside the raw one
    pp = metrics.PostProcess(median=3, erode=0, min_size=2)
    r = metrics.anomaly_metrics_surface(real, recon, mask, postprocess=pp)
    assert set(r) == PARENT_METRIC_KEYS | PP_METRIC_KEYS | SURFACE_METRIC_KEYS | {"HD_pp", "HD95_pp", "ASSD_pp"}
    with_pp = metrics.anomaly_metrics(real, recon, mask, postprocess=pp)
    for k in (PARENT_METRIC_KEYS | PP_METRIC_KEYS) - {"maps"}:
        assert _bits(np.float64(r[k]), np.float64(with_pp[k])), k
    o = metrics.surface_distance(r["maps"]["pred_pp"], mask)
    for key, src in (("HD_pp", "hd"), ("HD95_pp", "hd95"), ("ASSD_pp", "assd")):
        assert _bits(np.float64(r[key]), _host(o[src])[0, 0]), key
    assert _bits(np.float64(r["HD95"]), np.float64(want["hd95"]))
    # no mask, and no plane with both borders: NaN, nothing valid
    r = metrics.anomaly_metrics_surface(real, recon, None)
    assert all(np.isnan(r[k]) for k in ("HD", "HD95", "ASSD")) and (r["HD95_valid"], r["surface_status"]) == (0, 0)
    r = metrics.anomaly_metrics_surface(real, recon, torch.zeros_like(mask))
    assert all(np.isnan(r[k]) for k in ("HD", "HD95", "ASSD")) and (r["HD95_valid"], r["surface_status"]) == (0, 2)


# ---------------------------------------------------------------------------------- detection records
def test_detection_records_carry_boundary_distances_when_asked(tmp_path, monkeypatch):
    from anoddpm_amd import _lib, metrics
    GD, m, d = _tiny(32)
    monkeypatch.chdir(tmp_path)
    g = torch.Generator().manual_seed(5)
    x_0 = (torch.rand(1, 1, 32, 32, generator=g) * 2 - 1).to(DEV)
    mask = torch.zeros(1, 1, 32, 32)
    mask[0, 0, 4:14, 5:20] = 1
    mask[0, 0, 25:27, 26:28] = 1
    mask = mask.to(DEV)
    args = {"arg_num": 9, "T": 200, "img_size": [32, 32]}                # settings 50, 100, 150

    assert d.surface_metrics is False
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    plain = d.last_detection
    assert [r["t_distance"] for r in plain] == [50, 100, 150] and all(set(r) == PARENT_RECORD_KEYS for r in plain)

    calls = []
    L = _lib.lib()
    fn = L.anoddpm_surface_distance
    monkeypatch.setattr(L, "anoddpm_surface_distance", lambda *a: (calls.append("surface"), fn(*a))[1])
    d.surface_metrics = True
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert calls == ["surface"]                                           # one batched call for the whole sweep
    recs = d.last_detection
    for rec, old in zip(recs, plain):
        assert set(rec) == PARENT_RECORD_KEYS | {"hd", "hd95", "assd"}
        for k in ("mean", "mse", "threshold", "counts", "auc", "ap", "best_dice", "best_threshold", "ssim", "output"):
            assert _bits(_host(rec[k]), _host(old[k])), k                 # the same chains, the same raw results
        del calls[:]
        o = metrics.surface_distance(rec["threshold"], mask)
        for k in ("hd", "hd95", "assd"):
            assert rec[k].is_cuda and rec[k].dtype == torch.float64 and rec[k].shape == ()
            assert _bits(_host(rec[k]), _host(o[k])[0, 0]), k
        print(rec["t_distance"], float(rec["hd"]), float(rec["hd95"]), float(rec["assd"]), int(o["status"]))

    # with post-processing: the _pp forms from the same call
    del calls[:]
    d.postprocess = metrics.PostProcess(median=3, erode=0, min_size=3)
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert calls == ["surface"]
    for rec, old in zip(d.last_detection, recs):
        assert set(rec) == PARENT_RECORD_KEYS | PP_RECORD_KEYS | {"hd", "hd95", "assd", "hd_pp", "hd95_pp", "assd_pp"}
        cut = metrics.remove_small_components((rec["sqerr_pp"] > 0.5).float(), min_size=3)
        o = metrics.surface_distance(cut, mask)
        for k in ("hd", "hd95", "assd"):
            assert _bits(_host(rec[k]), _host(old[k])), k
            assert _bits(_host(rec[k + "_pp"]), _host(o[k])[0, 0]), k

    # without a mask, and with the default: the parent's keys
    d.postprocess = None
    d.detection_B(m, x_0, args, ("vol", "slice"), None, denoise_fn="gauss", total_avg=2)
    assert all(set(r) == PARENT_RECORD_KEYS for r in d.last_detection)
    d.surface_metrics = False
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert all(set(r) == PARENT_RECORD_KEYS for r in d.last_detection)
    assert not os.listdir(tmp_path)
