"""-m gpu: `detection_two_pass` on the small UNet of the detection tests (32^2, base 32, T = 100), seeded owner,
total_avg = 2, t_first = 6, t_second = [3, 5]: the two trivial thresholds, a threshold taken on the device, the records, smoothing
and a roi, and detection_B around a call."""
import numpy as np
import pytest
import torch

import keepmask_cases as kc
from test_gpu_detection import DEV, tiny

pytestmark = pytest.mark.gpu

_TINY = []
AVG, T1, T2 = 2, 6, [3, 5]
BASE_KEYS = ["output", "mean", "mse", "threshold", "counts", "auc", "auc_status", "ap", "best_dice", "best_threshold", "ssim", "keep", "regen"]


def shared():
    """One model for the file; a fresh diffusion owner per test."""
    if not _TINY:
        _TINY.append(tiny())
    GD, m, _ = _TINY[0]
    return GD, m, GD.GaussianDiffusionModel([32, 32], GD.get_beta_schedule(100, "linear"), noise="gauss")


def image():
    g = torch.Generator().manual_seed(21)
    x_0 = (torch.rand(1, 1, 32, 32, generator=g) * 2 - 1).to(DEV)
    mask = (torch.rand(1, 1, 32, 32, generator=g) > 0.7).float().to(DEV)
    return x_0, mask


def two_pass(d, m, x_0, mask, threshold, seed=4, **kw):
    d.seed_gauss(seed)
    assert d.detection_two_pass(m, x_0, mask, threshold, T1, T2, total_avg=AVG, **kw) is None
    return d.last_detection


def first_pass(d, m, x_0, seed=4):
    """Pass 1 run alone on the same seed and stream position: (outputs, mean, sqerr) -- the bits the call itself works on."""
    from anoddpm_amd import metrics
    d.seed_gauss(seed)
    out = d._run_chains(m, x_0, [T1] * AVG, None)
    maps, _ = metrics.anomaly_maps(x_0, out, None, want=("mean", "sqerr"))
    return out, maps["mean"], maps["sqerr"]


def want_keep(score, thr, r, roi=None):
    """The restatement on a downloaded [H][W] score plane -> uint8 [1][1][H][W]."""
    inside = np.ones(score.shape, bool) if roi is None else roi == 1
    regen = kc.dilate_numpy((score > np.float32(thr)) & inside, r) & inside
    return (~regen).astype(np.uint8)[None, None]


def test_threshold_inf_keeps_everything_and_returns_the_input():
    from anoddpm_amd import metrics
    GD, m, d = shared()
    x_0, mask = image()
    recs = two_pass(d, m, x_0, mask, float("inf"))
    assert [r["pass"] for r in recs] == [1, 2, 2]
    for r in recs:
        assert r["keep"].dtype == torch.uint8 and r["keep"].shape == (1, 1, 32, 32) and bool((r["keep"] == 1).all())
        assert r["regen"].dtype == torch.int32 and r["regen"].tolist() == [0]
    _, mean1, sq1 = first_pass(d, m, x_0)
    assert torch.equal(metrics.keep_mask(sq1[:, 0], float("inf"), 2, real=x_0, recon=mean1)["stitched"], x_0)
    for r in recs[1:]:
        assert r["output"].shape == (AVG, 1, 32, 32) and all(torch.equal(o, x_0[0]) for o in r["output"])
    d.release_chains()


def test_threshold_below_everything_is_an_unconditioned_second_pass():
    from anoddpm_amd import metrics
    GD, m, d = shared()
    x_0, mask = image()
    recs = two_pass(d, m, x_0, mask, -1.0)
    for r in recs:
        assert bool((r["keep"] == 0).all()) and r["regen"].tolist() == [32 * 32]
    out1, mean1, sq1 = first_pass(d, m, x_0)                         # streams 0, 1; the owner now stands at stream 2
    assert torch.equal(recs[0]["output"], out1) and torch.equal(recs[0]["mean"], mean1)
    assert torch.equal(metrics.keep_mask(sq1[:, 0], -1.0, 2, real=x_0, recon=mean1)["stitched"], mean1)
    plain = d._run_chains(m, mean1, [t for t in T2 for _ in range(AVG)], None)
    got = torch.cat([r["output"] for r in recs[1:]])
    assert torch.isfinite(got).all()
    print("max |two-pass - unconditioned|:", float((got - plain).abs().max()))
    assert torch.allclose(got, plain, atol=1e-4, rtol=0), float((got - plain).abs().max())
    d.release_chains()


def test_threshold_taken_on_the_device():
    from anoddpm_amd import metrics
    from scipy import ndimage as ndi
    GD, m, d = shared()
    x_0, mask = image()
    out1, mean1, sq1 = first_pass(d, m, x_0)
    thr = metrics.order_stats(sq1, [sq1.numel() // 10], batched=True)["value"].reshape(1)      # stays on the device
    recs = two_pass(d, m, x_0, mask, thr)
    assert d.last_chain_schedule["chain_steps"] == AVG * sum(T2)
    assert len([ch for ch in d._chains.values() if getattr(ch, "slot_chain", False)]) == 2      # neither pass dropped the other's graph
    assert torch.equal(recs[0]["output"], out1)
    seed = sq1[0, 0].cpu().numpy() > thr.cpu().numpy()[0]
    keep = (~ndi.binary_dilation(seed, iterations=2)).astype(np.uint8)
    assert 0 < seed.sum() < seed.size and 0 < keep.sum() < keep.size
    kept = torch.from_numpy(keep.astype(bool)).to(DEV)
    for r in recs:
        assert np.array_equal(r["keep"].cpu().numpy()[0, 0], keep) and r["regen"].tolist() == [int((keep == 0).sum())]
    for r in recs[1:]:
        assert torch.isfinite(r["output"]).all()
        assert all(torch.equal(o[0][kept], x_0[0, 0][kept]) for o in r["output"])
        assert not torch.equal(r["output"][0], x_0[0])               # and the rest was regenerated
    again = two_pass(d, m, x_0, mask, float(thr.item()))
    assert [list(r) for r in again] == [list(r) for r in recs]
    for a, b in zip(again, recs):
        assert all(torch.equal(a[k], b[k]) for k in ("output", "mean", "mse", "threshold", "counts", "keep", "regen"))
        assert all(torch.equal(a[k], b[k]) for k in ("auc", "ap", "best_dice"))
    res = GD.Resampling(2, 2)
    jumped = two_pass(d, m, x_0, mask, thr, resampling=res)
    assert d.last_chain_schedule["chain_steps"] == AVG * sum(res.steps(t) for t in T2) > AVG * sum(T2)
    assert all(torch.equal(a["keep"], b["keep"]) for a, b in zip(jumped, recs)) and torch.equal(jumped[0]["output"], out1)
    for r in jumped[1:]:
        assert torch.isfinite(r["output"]).all() and all(torch.equal(o[0][kept], x_0[0, 0][kept]) for o in r["output"])
    d.resampling = res                                               # the attribute serves where the argument is absent
    two_pass(d, m, x_0, mask, thr)
    assert d.last_chain_schedule["chain_steps"] == AVG * sum(res.steps(t) for t in T2)
    d.release_chains()


def test_records_smoothing_and_roi():
    from anoddpm_amd import metrics
    GD, m, d = shared()
    x_0, mask = image()
    out1, mean1, sq1 = first_pass(d, m, x_0)
    thr = float(metrics.order_stats(sq1, [sq1.numel() // 10], batched=True)["value"].item())
    base = d.gauss_next_stream
    recs = two_pass(d, m, x_0, mask, thr, dilate=1)
    assert d.gauss_next_stream == AVG * (1 + len(T2))                 # pass 1's streams first, then pass 2's in setting order
    assert base == AVG
    assert [list(r) for r in recs] == [["t_distance", "pass"] + BASE_KEYS] + [["t_distance", "pass", "t_first"] + BASE_KEYS] * 2
    assert [(r["t_distance"], r["pass"], r.get("t_first")) for r in recs] == [(T1, 1, None), (T2[0], 2, T1), (T2[1], 2, T1)]
    assert all(r["keep"] is recs[0]["keep"] and r["regen"] is recs[0]["regen"] for r in recs)
    plain = want_keep(sq1[0, 0].cpu().numpy(), thr, 1)
    assert np.array_equal(recs[0]["keep"].cpu().numpy(), plain)
    smooth = metrics.gaussian_filter(sq1, sigma=1.0)[0, 0].cpu().numpy()
    thr_s = float(np.sort(smooth.reshape(-1))[::-1][smooth.size // 10])
    recs = two_pass(d, m, x_0, mask, thr_s, dilate=1, smooth=1.0)
    smoothed = want_keep(smooth, thr_s, 1)
    assert np.array_equal(recs[0]["keep"].cpu().numpy(), smoothed) and not np.array_equal(smoothed, plain)
    roi = torch.zeros(32, 32, device=DEV)
    roi[:, :16] = 1
    recs = two_pass(d, m, x_0, mask, thr, dilate=1, roi=roi)
    with_roi = want_keep(sq1[0, 0].cpu().numpy(), thr, 1, roi.cpu().numpy())
    assert np.array_equal(recs[0]["keep"].cpu().numpy(), with_roi) and not np.array_equal(with_roi, plain)
    assert with_roi[0, 0, :, 16:].all() and all(torch.equal(o[:, :, 16:], x_0[0][:, :, 16:]) for r in recs[1:] for o in r["output"])
    d.release_chains()


def test_detection_B_around_a_two_pass_call(tmp_path, monkeypatch):
    """With the method not called, detection_B gives the records, keys and output bits of a run made before it ever ran."""
    GD, m, d = shared()
    monkeypatch.chdir(tmp_path)
    x_0, mask = image()
    args = {"arg_num": 9, "T": 100, "img_size": [32, 32]}
    d.seed_gauss(4)
    assert d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2) == [None]
    before = d.last_detection
    keys, images = [list(r) for r in before], [r["output"].clone() for r in before]
    assert keys == [["t_distance"] + BASE_KEYS[:-2]]
    two_pass(d, m, x_0, mask, 0.05)
    d.seed_gauss(4)
    assert d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2) == [None]
    assert [list(r) for r in d.last_detection] == keys
    assert all(torch.equal(r["output"], img) for r, img in zip(d.last_detection, images))
    assert d.detection_keep is None and d.resampling is None
    d.release_chains()
