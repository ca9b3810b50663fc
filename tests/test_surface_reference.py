"""Distance transform and boundary distances without a device: the restatements of tests/surface_cases.py agree -- the integer
brute-force minimum, scipy's transform and the kernel's own decomposition -- the fixture tests/golden/surface_kat.npz regenerates
bit for bit, the percentile the header defines stays within 8 ulp of numpy.percentile, every planted defect changes the result
of at least one case (otherwise the case list would prove nothing), and the host side of the native path: validation of
anoddpm_distance_transform / anoddpm_surface_distance through the ABI, struct sizes, exports, and the opt-in hooks leaving the
defaults alone.  CPU only."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import surface_cases as sc
from conftest import GOLDEN
from score_cases import bits as _bits


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "surface_kat.npz"))


@pytest.fixture(scope="module")
def surface_results():
    """name -> the `surface_ref` of every pair of the case; computed once, read by every test."""
    return {name: [sc.surface_ref(p, r) for p, r in sc.pairs_of(pred, ref)] for name, (pred, ref) in sc.surface_cases().items()}


# ---------------------------------------------------------------------------------- distance transform
@pytest.mark.parametrize("name", sc.SMALL_TRANSFORM + sc.LARGE_TRANSFORM)
def test_brute_force_equals_scipy_squared_and_the_fixture(kat, name):
    planes, level = sc.transform_cases()[name]
    fg = sc.foreground(planes, level)
    sq = np.stack([sc.edt2_brute(f) for f in fg]).astype(np.int32)
    dist = np.stack([sc.edt_scipy(f) if not f.all() else np.full(f.shape, np.inf) for f in fg])
    for f, s, d in zip(fg, sq, dist):
        if f.all():
            assert (s == -1).all()
            continue
        assert _bits(d, np.sqrt(s.astype(np.float64))), name                  # scipy = the correctly rounded root of the integer
        assert np.array_equal(sc.edt2_separable(f), s), name                  # the kernel's decomposition
        assert (s[~f] == 0).all() and (s[f] > 0).all()
    if name in sc.SMALL_TRANSFORM:
        assert _bits(fg.astype(np.uint8), kat[f"dt_{name}_fg"]) and _bits(sq, kat[f"dt_{name}_sq"])
    assert sc.sha(fg.astype(np.uint8), sq, dist) == str(kat[f"dt_{name}_sha"])


def test_transform_cases_reach_what_they_are_for():
    c = sc.transform_cases()
    assert sc.edt2_brute(c["corner64"][0][0] > 0).max() == 2 * 63 * 63
    wide = sc.edt2_brute(c["wide17x300"][0][0] > 0)
    assert wide.max() > 64 * 64 and not np.array_equal(sc.edt2_separable(c["wide17x300"][0][0] > 0, cap=64), wide)
    assert c["long2x4100"][0].shape[-1] > 4096 and c["all_fg_mid"][0][1].all() and not c["all_fg_mid"][0][0].all()
    assert np.isnan(c["level_nan"][0]).sum() == 3 and c["level_nan"][1] != 0.0
    assert c["rand40x33"][0].shape[-1] % 2 == 1


# ---------------------------------------------------------------------------------- boundary distances
@pytest.mark.parametrize("name", sc.SMALL_SURFACE + sc.LARGE_SURFACE)
def test_fixture_is_reproduced(kat, surface_results, name):
    pred, ref = sc.surface_cases()[name]
    if name in sc.SMALL_SURFACE:
        assert _bits(pred.astype(np.uint8), kat[f"sd_{name}_pred"]) and _bits(ref.astype(np.uint8), kat[f"sd_{name}_ref"])
    else:
        assert sc.sha(pred, ref) == str(kat[f"sd_{name}_sha"])
    res = surface_results[name]
    for k in ("counts", "max2", "mean", "p95"):
        assert _bits(np.stack([r[k] for r in res]), kat[f"sd_{name}_{k}"]), (name, k)
    assert [r["status"] for r in res] == kat[f"sd_{name}_status"].tolist()


def test_cases_state_what_they_are_for(surface_results):
    r = surface_results
    assert r["identical"][0]["hd"] == 0.0 and r["identical"][0]["assd"] == 0.0 and r["identical"][0]["hd95"] == 0.0
    assert r["single_pixel"][0]["counts"][0] == 1
    assert r["full_image"][0]["counts"][0] == 2 * 12 + 2 * 15 - 4                            # the frame
    assert r["nested"][0]["max2"].min() >= 36 and r["nested"][0]["hd95"] > 0                 # border to border, not to the foreground
    assert r["corners64"][0]["max2"].tolist() == [2 * 63 * 63] * 2
    assert r["blobs17x300"][0]["max2"].max() > 64 * 64
    assert [x["status"] for x in r["batch6_shared"]] == [0, 0, sc.EMPTY_PRED, 0, 0, 0]
    assert r["empty_ref"][0]["status"] == sc.EMPTY_REF and np.isnan(r["empty_ref"][0]["p95"]).all() and r["empty_ref"][0]["max2"].tolist() == [-1, -1]
    assert r["empty_ref"][0]["counts"][0] > 0
    assert r["pair256"][0]["counts"].min() > 1024                                            # more than one round of the strided sum


@pytest.mark.parametrize("name", sc.SMALL_SURFACE + sc.LARGE_SURFACE)
def test_kernel_order_sum_against_fsum_and_percentile_against_numpy(surface_results, name):
    pred, ref = sc.surface_cases()[name]
    for (p, r), want in zip(sc.pairs_of(pred, ref), surface_results[name]):
        got = sc.surface_fp64(p, r)
        assert got["status"] == want["status"] and np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["max2"], want["max2"])
        if want["status"]:
            assert np.isnan(got["mean"]).all()
            continue
        assert _bits(got["p95"], want["p95"])
        _, _, d_pr, d_rp = sc.directed(p, r)
        for d, gm, wm in zip((d_pr, d_rp), got["mean"], want["mean"]):
            bound = d.size * 2.0 ** -52 * np.sqrt(np.float64(d.max()))
            assert abs(gm - wm) <= bound, (name, gm, wm, bound)
        for d, q in zip((d_pr, d_rp, np.r_[d_pr, d_rp]), want["p95"]):
            ref95 = np.percentile(np.sqrt(d.astype(np.float64)), 95)
            assert sc.ulps(q, ref95) <= 8, (name, q, ref95)


def test_percentile_within_8_ulp_of_numpy_on_random_multisets():
    rng = np.random.default_rng(17)
    worst = 0.0
    for _ in range(2000):
        n = int(rng.integers(1, 400))
        sq = np.sort(rng.integers(0, int(rng.choice([4, 100, 20000, 2 * 63 * 63, 2 ** 31 - 1])), n).astype(np.int64))
        worst = max(worst, sc.ulps(sc.percentile95(sq), np.percentile(np.sqrt(sq.astype(np.float64)), 95)))
    print(f"worst distance from numpy.percentile: {worst} ulp")
    assert worst <= 8
    assert sc.percentile95(np.array([9], np.int64)) == 3.0                                  # n = 1: lo = hi = 0
    assert sc.percentile95(np.arange(21, dtype=np.int64) ** 2) == 19.0                      # r = 0: no interpolation


DEFECTS = {"8-neighbour erosion": dict(structure=sc.FULL),
           "image edge not a border": dict(border_value=1),
           "distance to the foreground": dict(to_foreground=True),
           "one direction only": dict(one_direction=True),
           "nearest-rank percentile": dict(percentile="nearest"),
           "row search capped at 64 columns": dict(row_cap=64),
           "per-direction percentiles maxed": dict(pooled="max")}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_every_planted_defect_changes_a_case(surface_results, defect):
    seen = []
    for name, (pred, ref) in sc.surface_cases().items():
        if name in sc.LARGE_SURFACE:
            continue
        bad = [sc.surface_ref(p, r, **DEFECTS[defect]) for p, r in sc.pairs_of(pred, ref)]
        if sc.summary(bad) != sc.summary(surface_results[name]):
            seen.append(name)
    print(defect, "->", seen)
    assert seen, f"no case notices: {defect}"


def test_capped_search_without_a_cap_is_the_transform():
    for name in ("blobs16", "blobs40x33", "blobs17x300"):
        pred, ref = sc.surface_cases()[name]
        a = sc.directed(pred[0], ref[0])
        b = sc.directed(pred[0], ref[0], row_cap=300)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------- the host side of the native path
def _distance_args(L, keep):
    from anoddpm_amd import _lib
    a = _lib.DistanceArgs()
    a.src, a.sq, a.workspace = 64, 64, 64                                   # never dereferenced: validation comes first
    a.workspace_bytes, a.src_stride, a.S, a.H, a.W = 1 << 40, 16, 1, 4, 4
    for k, v in keep.items():
        setattr(a, k, v)
    return a


def _surface_args(L, keep):
    from anoddpm_amd import _lib
    a = _lib.SurfaceArgs()
    for k in ("pred", "ref", "workspace", "counts", "max2", "mean", "p95", "status"):
        setattr(a, k, 64)
    a.workspace_bytes, a.pred_stride, a.ref_stride, a.S, a.H, a.W = 1 << 40, 16, 16, 2, 4, 4
    for k, v in keep.items():
        setattr(a, k, v)
    return a


def test_argument_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_distance_transform(None, None) == -1 and b"null args" in L.anoddpm_last_error()
    assert L.anoddpm_surface_distance(None, None) == -1 and b"null args" in L.anoddpm_last_error()
    for k in ("src", "sq", "workspace"):
        assert L.anoddpm_distance_transform(ctypes.byref(_distance_args(L, {k: None})), None) == -1
        assert b"distance_transform: null pointer" in L.anoddpm_last_error()
    for k in ("pred", "ref", "workspace", "counts", "max2", "mean", "p95", "status"):
        assert L.anoddpm_surface_distance(ctypes.byref(_surface_args(L, {k: None})), None) == -1
        assert b"surface_distance: null pointer" in L.anoddpm_last_error()
    # sizes whose squared distance, plane or batch leaves int32
    big = (dict(H=46342, W=2), dict(H=2, W=46342), dict(H=32769, W=32769), dict(H=40000, W=60000), dict(S=1 << 20, H=64, W=64),
           dict(S=0), dict(H=0), dict(W=-1))
    for over in big:
        assert L.anoddpm_distance_transform(ctypes.byref(_distance_args(L, over)), None) == -1, over
        assert b"below 2^31" in L.anoddpm_last_error()
        assert L.anoddpm_surface_distance(ctypes.byref(_surface_args(L, over)), None) == -1, over
        assert b"below 2^31" in L.anoddpm_last_error()
        assert L.anoddpm_surface_workspace_bytes(over.get("S", 1), over.get("H", 4), over.get("W", 4)) == -1
    assert L.anoddpm_surface_workspace_bytes(1, 46341, 1) == 16 * 46341                      # (H - 1)^2 = 46340^2 < 2^31
    assert L.anoddpm_surface_workspace_bytes(55, 256, 256) == 16 * 55 * 65536
    # strides and workspace
    assert L.anoddpm_distance_transform(ctypes.byref(_distance_args(L, dict(S=2, src_stride=15))), None) == -1
    assert b"planes overlap" in L.anoddpm_last_error()
    assert L.anoddpm_distance_transform(ctypes.byref(_distance_args(L, dict(workspace_bytes=63))), None) == -1
    assert b"workspace too small" in L.anoddpm_last_error()
    assert L.anoddpm_surface_distance(ctypes.byref(_surface_args(L, dict(pred_stride=15))), None) == -1
    assert b"planes overlap" in L.anoddpm_last_error()
    assert L.anoddpm_surface_distance(ctypes.byref(_surface_args(L, dict(ref_stride=3))), None) == -1
    assert b"ref_stride" in L.anoddpm_last_error()
    assert L.anoddpm_surface_distance(ctypes.byref(_surface_args(L, dict(workspace_bytes=16 * 2 * 16 - 1))), None) == -1
    assert b"workspace too small" in L.anoddpm_last_error()


def test_abi_moves_together():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_abi_version() == _lib.ABI_VERSION
    for name, st in ((b"anoddpm_distance_args", _lib.DistanceArgs), (b"anoddpm_surface_args", _lib.SurfaceArgs)):
        assert st in _lib._STRUCTS and L.anoddpm_struct_size(name) == ctypes.sizeof(st)
    for name in ("anoddpm_distance_transform", "anoddpm_surface_distance", "anoddpm_surface_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert (_lib.SURFACE_EMPTY_PRED, _lib.SURFACE_EMPTY_REF) == (sc.EMPTY_PRED, sc.EMPTY_REF)


def test_public_names_and_untouched_defaults():
    import evaluation
    from anoddpm_amd import diffusion, metrics
    for name in ("distance_transform", "surface_distance", "HD95", "anomaly_metrics_surface"):
        assert name in metrics.__all__ and callable(getattr(evaluation, name))
    assert evaluation.HD95 is metrics.HD95 and evaluation.surface_distance is metrics.surface_distance and evaluation.AUPRO is metrics.AUPRO
    assert str(inspect.signature(metrics.distance_transform)) == "(x, level=0.0, squared=False, batched=None)"
    assert str(inspect.signature(metrics.surface_distance)) == "(pred, ref, level=0.0, return_status=False)"
    assert str(inspect.signature(metrics.HD95)) == "(real_mask, pred_mask)"
    assert str(inspect.signature(metrics.anomaly_metrics_surface)) == "(real, recon, mask, threshold=0.5, postprocess=None, roi=None)"
    assert str(inspect.signature(metrics.anomaly_metrics)) == "(real, recon, mask, threshold=0.5, postprocess=None, roi=None)"
    assert str(inspect.signature(metrics.anomaly_metrics_pro)) == "(real, recon, mask, threshold=0.5, postprocess=None, roi=None, pro_limit=0.3)"
    assert diffusion.GaussianDiffusionModel.surface_metrics is False
    import torch
    with pytest.raises(TypeError):
        metrics.distance_transform(np.zeros((4, 4), np.float32))
    with pytest.raises(TypeError):
        metrics.surface_distance(torch.zeros(4, 4), np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="neither the shape"):
        metrics.surface_distance(torch.zeros(2, 4, 4), torch.zeros(3, 4, 4))
    from anoddpm_amd._lib import AnoddpmError
    with pytest.raises(AnoddpmError):
        metrics.surface_distance(torch.zeros(4, 4), torch.zeros(4, 4))                      # host tensors: no CPU path
    with pytest.raises(AnoddpmError):
        metrics.distance_transform(torch.zeros(4, 4))
