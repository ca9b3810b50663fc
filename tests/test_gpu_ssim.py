"""-m gpu: the native SSIM (csrc/ssim.hip through metrics.ssim / SSIM, anomaly_metrics and the detection records) against the
fixture tests/golden/ssim_kat.npz (the definition with scipy's filters, the ones skimage calls): |mssim - expected| <= 1e-10, the
fp32 map within 2^-24 + 1e-10, real == recon exactly 1.0, NaN segments NaN (tests/ssim_cases.py derives the bounds).  Neither
skimage nor scipy is needed."""
import gc
import os

import numpy as np
import pytest
import torch

import ssim_cases as sc
from conftest import GOLDEN
from score_cases import bits as _bits, tiny as _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(name, window) for name, windows in sorted(sc.SINGLE.items()) for window in windows]


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "ssim_kat.npz"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _kw(window):
    return dict(gaussian_weights=True) if window == "gauss" else dict(win_size=window)


def _check(got, want, what):
    print(f"{what}: mssim {got!r} fixture {want!r} |diff| {abs(got - want):.3g} bound {sc.MSSIM_TOL:.3g}")
    if np.isnan(want):
        assert np.isnan(got), what
    else:
        assert abs(got - want) <= sc.MSSIM_TOL, what


@pytest.mark.parametrize("name,window", CASES)
def test_mssim_and_map_match_fixture(kat, name, window):
    from anoddpm_amd import metrics
    real, recon = sc.make_case(name)
    assert sc.sha_inputs(real, recon) == str(kat[f"{name}_sha"]), f"{name}: regenerated input differs from the fixture's"
    x, y = _dev(real), _dev(recon)
    got, smap = metrics.ssim(x, y, full=True, **_kw(window))
    assert got.shape == (1,) and got.dtype == torch.float64 and got.is_cuda
    assert smap.shape == x.shape and smap.dtype == torch.float32
    _check(float(got[0]), float(kat[f"{sc.key(name, window)}_mssim"]), sc.key(name, window))
    assert _bits(metrics.ssim(x, y, **_kw(window)).cpu().numpy(), got.cpu().numpy())          # with and without the map
    # the restatement of the kernel's arrangement: the same IEEE fp64 operations in the same order (no contraction, correctly
    # rounded division), so with the exact 1/win weights the bits agree; the gaussian table goes through two exp() libraries
    want_b, map_b = sc.ssim_kernel_numpy(real, recon, window)
    host_map = smap.cpu().numpy()
    print(f"  against the kernel-arrangement restatement: |mssim diff| {abs(float(got[0]) - want_b):.3g}, "
          f"map elements that differ from its fp32 rounding: {int((host_map != map_b.astype(np.float32)).sum())} of {host_map.size}")
    assert abs(float(got[0]) - want_b) <= sc.MSSIM_TOL and np.abs(host_map.astype(np.float64) - map_b).max() <= sc.MAP_TOL
    if window != "gauss":
        assert float(got[0]) == want_b and _bits(host_map, map_b.astype(np.float32))
    if (name, window) in sc.MAP_CASES:
        for cname, sl in sc.crops(host_map).items():
            want = kat[f"{sc.key(name, window)}_map_{cname}"]
            diff = float(np.abs(host_map[sl].astype(np.float64) - want).max())
            print(f"  map crop {cname} {want.shape}: largest |diff| {diff:.3g} bound {sc.MAP_TOL:.3g}")
            assert diff <= sc.MAP_TOL, (name, window, cname)
    if name == "equal256":
        assert float(got[0]) == 1.0 and bool((smap == 1.0).all())
    if name == "const256":
        assert float(got[0]) < 0.0


def test_batch_of_55_with_shared_real(kat):
    from anoddpm_amd import metrics
    real, recons = sc.make_batch()
    assert sc.sha_inputs(real, recons) == str(kat["batch_sha"]), "batch: regenerated input differs from the fixture's"
    x, y = _dev(real), _dev(recons)
    got = metrics.ssim(x, y)                                            # one [1, 256, 256] image against [55, 1, 256, 256]
    assert got.shape == (sc.BATCH,)
    host = got.cpu().numpy()
    for j in range(sc.BATCH):
        _check(float(host[j]), float(kat["batch_mssim"][j]), f"batch[{j}]")
    # the same numbers from per-segment calls, from a repeated real, and from other dtypes / layouts of the inputs
    for j in (0, 27, 54):
        assert _bits(metrics.ssim(x, y[j]).cpu().numpy(), host[j:j + 1])
    assert _bits(metrics.ssim(x.expand(sc.BATCH, -1, -1, -1), y).cpu().numpy(), host)
    assert _bits(metrics.ssim(x[0], y[:, 0], batched=True).cpu().numpy(), host)          # [H, W] against [S, H, W]
    assert _bits(metrics.ssim(x.double(), y[:3].double()).cpu().numpy(), host[:3])
    yt = y[:3].transpose(-1, -2).contiguous().transpose(-1, -2)         # same values, other strides
    assert not yt.is_contiguous() and _bits(metrics.ssim(x, yt).cpu().numpy(), host[:3])


def test_nan_stays_in_its_segment(kat):
    from anoddpm_amd import metrics
    real, recon = sc.make_nan_batch()
    assert sc.sha_inputs(real, recon) == str(kat["nan_sha"]), "nan: regenerated input differs from the fixture's"
    got, smap = metrics.ssim(_dev(real), _dev(recon), full=True)
    host = got.cpu().numpy()
    assert np.isnan(host).tolist() == [j == sc.NAN_SEGMENT for j in range(3)]
    for j in range(3):
        _check(float(host[j]), float(kat["nan_mssim"][j]), f"nan[{j}]")
    nan_map = torch.isnan(smap).cpu().numpy()
    assert nan_map[sc.NAN_SEGMENT].sum() == 49 and not nan_map[[0, 2]].any()            # the 7 x 7 windows that hold the NaN


def test_two_runs_and_a_graph_replay_give_identical_bits(kat):
    from anoddpm_amd import metrics
    real, recons = sc.make_batch()
    x, y = _dev(real), _dev(recons[:8]).clone()
    a, amap = metrics.ssim(x, y, full=True)
    b, bmap = metrics.ssim(x, y, full=True)
    assert _bits(a.cpu().numpy(), b.cpu().numpy()) and _bits(amap.cpu().numpy(), bmap.cpu().numpy())
    eager_other = metrics.ssim(x, _dev(recons[8:16])).cpu().numpy()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()                                                        # no collection of older graphs inside the capture
    try:
        with torch.cuda.graph(g):
            c, cmap = metrics.ssim(x, y, full=True)
    finally:
        if was_enabled:
            gc.enable()
    g.replay()
    torch.cuda.synchronize()
    assert _bits(a.cpu().numpy(), c.cpu().numpy()) and _bits(amap.cpu().numpy(), cmap.cpu().numpy())
    y.copy_(_dev(recons[8:16]))                                         # new contents in the captured input, replayed
    g.replay()
    torch.cuda.synchronize()
    assert _bits(c.cpu().numpy(), eager_other)
    for j in range(8):
        _check(float(c[j]), float(kat["batch_mssim"][8 + j]), f"replayed batch[{8 + j}]")


def test_SSIM_in_both_upstream_call_forms(kat):
    import evaluation
    real, recon = sc.make_case("rgb64")
    x, y = _dev(real).permute(1, 2, 0), _dev(recon).permute(1, 2, 0)    # (H, W, C) as detection.py:241-246 passes it
    got = evaluation.SSIM(x, y)
    assert isinstance(got, float)
    _check(got, float(kat["rgb64_w7_mssim"]), "SSIM (H, W, C)")
    assert got == evaluation.SSIM(x.contiguous(), y.contiguous())
    real, recon = sc.make_case("mri256")
    got = evaluation.SSIM(_dev(real[0]), _dev(recon[0]))                # (H, W) as detection.py:361, 767: one single-channel image
    assert isinstance(got, float)
    _check(got, float(kat["mri256_w7_mssim"]), "SSIM (H, W)")
    with pytest.raises(ValueError, match="SSIM"):
        evaluation.SSIM(_dev(real[None]), _dev(recon[None]))


def test_anomaly_metrics_has_the_ssim(kat):
    from anoddpm_amd import metrics
    real, recons = sc.make_batch()
    x = _dev(np.stack([real, recons[40]]))                              # [2, 1, 256, 256]
    y = _dev(recons[[3, 20]])
    mask = (torch.rand(2, 1, 256, 256, device=DEV) > 0.9).float()
    before = metrics.anomaly_maps(x, y, mask)[1].cpu()
    r = metrics.anomaly_metrics(x, y, mask)
    per_image = metrics.ssim(x, y).cpu().numpy()
    assert isinstance(r["SSIM"], float) and r["SSIM"] == float(per_image.mean())
    _check(float(per_image[0]), float(kat["batch_mssim"][3]), "anomaly_metrics image 0")
    assert r["dice"] == float(metrics._ratios(before)["dice"]) and r["mse"] == float(before[:, 9].sum()) / x.numel()
    # a reconstruction with the navg axis: the SSIM is the one of the mean map
    stack = _dev(np.stack([recons[3], recons[5]]))                      # [navg = 2, C, H, W] for one image
    r2 = metrics.anomaly_metrics(x[:1], stack, mask[:1])
    assert r2["SSIM"] == float(metrics.ssim(x[:1], r2["maps"]["mean"])[0])
    want = sc.ssim_kernel_numpy(real, r2["maps"]["mean"][0].cpu().numpy(), 7)[0]
    _check(r2["SSIM"], want, "anomaly_metrics navg = 2 against the restatement")
    # smaller than the window, or not [B, C, H, W]: NaN, and every other key as before
    small = metrics.anomaly_metrics(x[:, :, :6, :40].contiguous(), y[:, :, :6, :40].contiguous(), mask[:, :, :6, :40].contiguous())
    assert np.isnan(small["SSIM"]) and 0.0 <= small["dice"] <= 1.0
    flat = metrics.anomaly_metrics(x.reshape(2, -1), y.reshape(2, -1), mask.reshape(2, -1))
    assert np.isnan(flat["SSIM"]) and flat["dice"] == r["dice"]


def test_too_small_images_raise():
    from anoddpm_amd import metrics
    x = torch.zeros(1, 6, 40, device=DEV)
    with pytest.raises(ValueError, match="window"):
        metrics.ssim(x, x)
    with pytest.raises(ValueError, match="window"):
        metrics.ssim(torch.zeros(1, 10, 40, device=DEV), torch.zeros(1, 10, 40, device=DEV), gaussian_weights=True)
    assert float(metrics.ssim(x, x, win_size=3)[0]) == 1.0
    with pytest.raises(ValueError, match="does not match"):
        metrics.ssim(torch.zeros(2, 1, 8, 8, device=DEV), torch.zeros(3, 1, 8, 8, device=DEV))
    with pytest.raises(ValueError, match="win_size"):
        metrics.ssim(torch.zeros(1, 32, 32, device=DEV), torch.zeros(1, 32, 32, device=DEV), win_size=8)
    with pytest.raises(ValueError, match="SSIM|window"):
        import evaluation
        evaluation.SSIM(torch.zeros(5, 5, device=DEV), torch.zeros(5, 5, device=DEV))


def test_detection_records_carry_the_ssim(tmp_path, monkeypatch):
    from anoddpm_amd import metrics
    GD, m, d = _tiny(32)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(1)
    x_0 = torch.rand(1, 1, 32, 32, device=DEV) * 2 - 1
    mask = (torch.rand(1, 1, 32, 32, device=DEV) > 0.7).float()
    args = {"arg_num": 9, "T": 200, "img_size": [32, 32]}                # settings 50, 100, 150
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert [r["t_distance"] for r in d.last_detection] == [50, 100, 150]
    for rec in d.last_detection:
        assert rec["ssim"].is_cuda and rec["ssim"].dtype == torch.float64 and rec["ssim"].shape == (1,)
        want = metrics.ssim(x_0, rec["mean"])
        assert _bits(rec["ssim"].cpu().numpy(), want.cpu().numpy())
        restated = sc.ssim_kernel_numpy(x_0[0].cpu().numpy(), rec["mean"][0].cpu().numpy(), 7)[0]
        _check(float(rec["ssim"][0]), restated, f"detection_B t_distance {rec['t_distance']}")
        assert -1.0 <= float(rec["ssim"][0]) <= 1.0
    # without a mask the SSIM is still there (it needs none)
    d.detection_B(m, x_0, args, ("vol", "slice"), None, denoise_fn="gauss", total_avg=2)
    assert all(r["ssim"] is not None and r["auc"] is None for r in d.last_detection)
    # an image smaller than the 7 x 7 window: no SSIM
    small = torch.zeros(2, 1, 1, 6, 6, device=DEV)
    assert "ssim" not in metrics.score_maps(torch.zeros(1, 1, 6, 6, device=DEV), small, small, small, None)
    # a batch of images: [B] per setting, the real images repeated per setting
    xb = torch.rand(2, 1, 32, 32, device=DEV) * 2 - 1
    means = torch.stack([(xb + 0.1 * (j + 1) * torch.rand_like(xb)).clamp(-1, 1) for j in range(3)])
    val = metrics.score_maps(xb, means, torch.zeros_like(means), torch.zeros_like(means), None)["ssim"]
    for j in range(3):
        assert val[j].shape == (2,) and _bits(val[j].cpu().numpy(), metrics.ssim(xb, means[j]).cpu().numpy())
    assert not os.listdir(tmp_path)
