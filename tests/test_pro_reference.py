"""Per-region overlap curve and AUPRO without a device: the three CPU restatements of tests/pro_cases.py agree -- fp64 in the
kernel's summation order and the cumulative-sum form of the published evaluation code against exact rational arithmetic over
scipy.ndimage.label, within n * 2^-50 -- the fixture tests/golden/pro_kat.npz regenerates bit for bit, and the host side of the
native path: validation of anoddpm_component_areas / anoddpm_pro_auc through the ABI, struct sizes, exports, and the opt-in hooks
leaving the defaults alone.  CPU only."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

import pro_cases as pc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "pro_kat.npz"))


def _segments(name):
    mask, score, limit, conn = pc.make_case(name)
    for s in range(score.shape[0]):
        yield s, pc.segment_mask(mask, score, s), score[s], limit, conn


@pytest.mark.parametrize("name", pc.SMALL + pc.LARGE)
def test_fp64_restatement_and_published_form_against_exact(kat, name):
    for s, mask, score, limit, conn in _segments(name):
        exact = pc.pro_exact(mask, score, limit, conn)
        assert (exact["K"], exact["N"], exact["P"]) == tuple(int(kat[f"{name}_{k}"][s]) for k in ("K", "N", "P"))
        assert pc.sha(exact["fps"], exact["thresholds"], exact["pro"]) == str(kat[f"{name}_curve_sha"][s])
        assert np.array_equal(np.float64(exact["aupro"]).view(np.uint64), kat[f"{name}_aupro"][s].view(np.uint64))
        pc.check_against_exact(pc.pro_fp64(mask, score, limit, conn), exact, f"{name}[{s}] fp64")
        fpr, pro, val = pc.pro_cumsum(mask, score, limit, conn)
        tol = pc.tolerance(score.size) - 2.0 ** -53
        if exact["K"] == 0 or exact["N"] == 0:
            assert np.isnan(val) and np.isnan(exact["aupro"])
            continue
        print(f"{name}[{s}] published form: aupro {val!r} exact {exact['aupro']!r} |diff| {abs(val - exact['aupro']):.3g} bound {tol:.3g}")
        assert abs(val - exact["aupro"]) <= tol
        assert fpr[0] == 0 and pro[0] == 0 and np.max(np.abs(fpr[1:] - exact["fps"] / np.float64(exact["N"]))) <= tol   # a cumsum of 1 / N
        assert np.max(np.abs(pro[1:] - exact["pro"])) <= tol


def test_ragged_case_is_what_it_is_for():
    mask, score, limit, conn = pc.make_case(pc.RAGGED)
    assert score.shape == (1, 1, 50, 100)
    exact = pc.pro_exact(mask, score[0], limit, conn)
    assert (exact["K"], exact["P"]) == (5, 1 + 6 + 62 + 200 + 600) and exact["N"] > 0 and exact["fps"].size <= 8
    pc.check_against_exact(pc.pro_fp64(mask, score[0], limit, conn), exact, "ragged fp64")
    # at every border of the 320-element wave chunks in the rows 10 to 24, one key carries several areas on both sides
    area = pc.regions(mask, conn)[0].reshape(-1)
    bits = (score.reshape(-1) + np.float32(0)).view(np.uint32)

    def mixed(lo):
        a, b = area[lo:lo + 320], bits[lo:lo + 320]
        return {k for k in np.unique(b[a != 0]) if np.unique(a[(b == k) & (a != 0)]).size > 1}

    for border in (1280, 1600, 1920, 2240):
        assert mixed(border - 320) & mixed(border), border


def test_hand_cases(kat):
    aupro = {name: float(kat[f"{name}_aupro"][0]) for name in pc.SMALL}
    assert aupro["first_beyond"] == 0.35 and int(kat["first_beyond_N"][0]) == 56      # the first point (24 / 56, 1) lies beyond 0.3
    mask, score, limit, conn = pc.make_case("first_beyond")
    e = pc.pro_exact(mask, score[0], limit, conn)
    assert e["fps"][0] == 24 and e["pro"][0] == 1.0
    assert abs(e["aupro_fraction"] - pc.Fraction(35, 100)) < pc.Fraction(1, 10 ** 15)
    assert aupro["perfect"] == 1.0 and aupro["all_equal"] == 0.15
    assert np.isnan(aupro["mask_all0"]) and int(kat["mask_all0_K"][0]) == 0
    assert np.isnan(aupro["mask_all1"]) and int(kat["mask_all1_N"][0]) == 0
    assert (int(kat["diag_c2_K"][0]), int(kat["diag_c1_K"][0])) == (1, 2)
    assert int(kat["pooled4_K"][0]) == 4                                              # the regions of planes 1 and 2 stay apart
    # N = 10 and the point with three negatives above the cut sits on the limit: fl(3 / 10) is the literal 0.3
    mask, score, limit, conn = pc.make_case("at_limit")
    e = pc.pro_exact(mask, score[0], limit, conn)
    assert e["N"] == 10 and 3 in e["fps"].tolist() and np.float64(3) / np.float64(10) == limit
    # -0.0 and +0.0 are one score: the lowest threshold is +0.0 and holds every zero
    mask, score, limit, conn = pc.make_case("neg_zero")
    assert np.signbit(score).any() and (score == 0).sum() > np.signbit(score).sum()
    e = pc.pro_exact(mask, score[0], limit, conn)
    assert e["thresholds"][-1].view(np.uint32) == 0 and e["fps"].size == np.unique(score + np.float32(0)).size
    # limit 1.0 integrates the whole curve
    assert aupro["limit1"] > aupro["plane16"]


def test_fixture_regenerates_bit_equal(kat):
    sys.path.insert(0, GOLDEN)
    try:
        import make_pro_golden
    finally:
        sys.path.remove(GOLDEN)
    fresh = make_pro_golden.build()
    assert sorted(fresh) == sorted(kat.files)
    for k, v in fresh.items():
        v = np.asarray(v)
        assert v.dtype == kat[k].dtype and v.shape == kat[k].shape and v.tobytes() == kat[k].tobytes(), k
    assert os.path.getsize(os.path.join(GOLDEN, "pro_kat.npz")) <= os.path.getsize(os.path.join(GOLDEN, "pr_kat.npz"))


def test_kernel_order_scan_is_a_scan():
    rng = np.random.default_rng(4)
    rows = rng.random((3, 64))
    assert np.max(np.abs(pc._group_scan(rows) - np.cumsum(rows, axis=1))) <= 64 * 2.0 ** -52 * 64
    assert np.array_equal(pc._group_scan(np.ones((1, 64))), np.arange(1.0, 65.0)[None])
    x, y = np.array([0.1, 0.2, 0.5, 1.0]), np.array([0.5, 0.5, 1.0, 1.0])
    # cut inside the third segment: (0.1 * 0.5 / 2) + 0.1 * 0.5 + 0.1 * (0.5 + 2 / 3) / 2
    t = pc.trapezoid_terms(x, y, 0.3)
    assert t[3] == 0 and abs(t.sum() - (0.025 + 0.05 + 0.1 * (0.5 + 0.5 + 0.5 / 3) / 2)) < 1e-15


def test_abi_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_abi_version() == _lib.ABI_VERSION
    for name, st in ((b"anoddpm_component_areas_args", _lib.ComponentAreasArgs), (b"anoddpm_pro_args", _lib.ProArgs)):
        assert st in _lib._STRUCTS and L.anoddpm_struct_size(name) == ctypes.sizeof(st)
    assert {"anoddpm_component_areas", "anoddpm_pro_auc", "anoddpm_pro_workspace_bytes"} <= set(_lib.SYMBOLS)
    # host memory stands in for the device pointers: every case below is rejected before anything is launched
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    err = L.anoddpm_last_error

    assert L.anoddpm_component_areas(None, None) == -1 and b"null args" in err()
    c = _lib.ComponentAreasArgs()
    c.S, c.H, c.W, c.connectivity, c.src_stride = 1, 4, 4, 2, 16
    c.workspace_bytes = L.anoddpm_small_components_workspace_bytes(1, 4, 4)
    for missing in ("src", "area", "counts", "workspace"):
        c.src = c.area = c.counts = c.workspace = p
        setattr(c, missing, None)
        assert L.anoddpm_component_areas(ctypes.byref(c), None) == -1 and b"null pointer" in err(), missing
    c.src = c.area = c.counts = c.workspace = p
    for conn in (0, 3, -1):
        c.connectivity = conn
        assert L.anoddpm_component_areas(ctypes.byref(c), None) == -1 and b"connectivity must be" in err()
    c.connectivity = 1
    c.workspace_bytes -= 1
    assert L.anoddpm_component_areas(ctypes.byref(c), None) == -1 and b"workspace too small" in err()
    c.H = 0
    assert L.anoddpm_component_areas(ctypes.byref(c), None) == -1 and b"must be >= 1" in err()

    assert L.anoddpm_pro_workspace_bytes(1, 1 << 31) == -1 and L.anoddpm_pro_workspace_bytes(0, 16) == -1
    assert L.anoddpm_pro_workspace_bytes(1, 0) == -1 and L.anoddpm_pro_workspace_bytes(1, (1 << 31) - 1) > 0
    assert L.anoddpm_pro_workspace_bytes(3, 16) == 3 * 6 * 64 * 4
    assert L.anoddpm_pro_auc(None, None) == -1 and b"null args" in err()
    a = _lib.ProArgs()
    required = ("score", "area", "region_counts", "workspace", "aupro", "counts", "status")

    def fill():
        for k in required:
            setattr(a, k, p)
        a.S, a.planes_per_segment, a.H, a.W, a.limit = 1, 1, 4, 4, 0.3
        a.workspace_bytes = L.anoddpm_pro_workspace_bytes(1, 16)

    for missing in required:
        fill()
        setattr(a, missing, None)
        assert L.anoddpm_pro_auc(ctypes.byref(a), None) == -1 and b"null pointer" in err(), missing
    for limit in (0.0, -0.3, 1.0000001, float("nan"), float("inf")):
        fill()
        a.limit = limit
        assert L.anoddpm_pro_auc(ctypes.byref(a), None) == -1 and b"limit must be in (0, 1]" in err(), limit
    fill()
    a.workspace_bytes -= 1
    assert L.anoddpm_pro_auc(ctypes.byref(a), None) == -1 and b"workspace too small" in err()
    fill()
    a.planes_per_segment, a.H, a.W = 2, 1 << 15, 1 << 15
    assert L.anoddpm_pro_auc(ctypes.byref(a), None) == -1 and b"below 2^31" in err()
    fill()
    a.S, a.score_stride, a.workspace_bytes = 2, 15, L.anoddpm_pro_workspace_bytes(2, 16)
    assert L.anoddpm_pro_auc(ctypes.byref(a), None) == -1 and b"score segments overlap" in err()
    a.score_stride, a.area_stride = 16, 8
    assert L.anoddpm_pro_auc(ctypes.byref(a), None) == -1 and b"area_stride must be 0" in err()
    fill()
    a.curve_fps = a.curve_thr = p
    assert L.anoddpm_pro_auc(ctypes.byref(a), None) == -1 and b"curve output needs" in err()
    a.curve_pro = a.curve_len = p
    a.curve_cap = 0
    assert L.anoddpm_pro_auc(ctypes.byref(a), None) == -1 and b"curve capacity" in err()


def test_python_argument_validation_without_gpu():
    import torch
    from anoddpm_amd import metrics
    from anoddpm_amd._lib import AnoddpmError
    m, s = torch.zeros(4, 4), torch.zeros(4, 4)
    with pytest.raises(AnoddpmError):
        metrics.aupro(m, s)                                              # CPU tensors: there is no host path
    with pytest.raises(AnoddpmError):
        metrics.component_areas(m)
    for limit in (0.0, 1.5, -1, True):
        with pytest.raises(ValueError):
            metrics.aupro(m, s, limit=limit)
    with pytest.raises(ValueError):
        metrics.aupro(m, s, connectivity=3)
    with pytest.raises(ValueError):
        metrics.component_areas(m, connectivity=0)
    with pytest.raises(ValueError):
        metrics.aupro(torch.zeros(3, 4), s)
    with pytest.raises(TypeError):
        metrics.aupro(np.zeros((4, 4)), s)


def test_new_names_are_exported_and_defaults_add_nothing(monkeypatch):
    import evaluation
    from anoddpm_amd import metrics
    from anoddpm_amd.diffusion import GaussianDiffusionModel
    new = {"component_areas", "aupro", "pro_points", "AUPRO", "anomaly_metrics_pro"}
    assert new <= set(metrics.__all__)
    assert all(getattr(evaluation, k) is getattr(metrics, k) for k in new)
    E = inspect.Parameter.empty
    parent = [("real", E), ("recon", E), ("mask", E), ("threshold", 0.5), ("postprocess", None), ("roi", None)]
    assert [(k, v.default) for k, v in inspect.signature(metrics.anomaly_metrics).parameters.items()] == parent
    assert [(k, v.default) for k, v in inspect.signature(metrics.anomaly_metrics_pro).parameters.items()] == parent + [("pro_limit", 0.3)]
    assert inspect.signature(metrics.aupro).parameters["limit"].default == 0.3
    assert inspect.signature(metrics.aupro).parameters["connectivity"].default == 2
    assert inspect.signature(metrics.AUPRO).parameters["limit"].default == 0.3
    # the record template: unset, `_score_settings` asks for no PRO launch and a record has no new key
    assert GaussianDiffusionModel.pro_limit is None
    import torch
    from score_cases import PARENT_RECORD_KEYS
    model, asked = object.__new__(GaussianDiffusionModel), []
    image = torch.zeros(1, 1, 8, 8)
    monkeypatch.setattr(metrics, "anomaly_maps", lambda *a, **kw: ({k: image for k in ("mean", "sqerr", "mse_img", "thr_img", "pred")}, torch.zeros(1, 12)))
    monkeypatch.setattr(metrics, "score_maps", lambda *a, **kw: (asked.append(kw["pro_limit"]), {})[1])
    model._score_settings([{"t_distance": 50}], torch.zeros(2, 1, 8, 8), 2, image, None)
    assert asked == [None] and set(model.last_detection[0]) == PARENT_RECORD_KEYS
    model.pro_limit = 0.3
    model._score_settings([{"t_distance": 50}], torch.zeros(2, 1, 8, 8), 2, image, None)
    assert asked == [None, 0.3] and model.last_detection[0]["aupro"] is None
