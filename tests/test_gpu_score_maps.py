"""-m gpu: metrics.score_maps, the one statement of the scoring pipeline behind anomaly_metrics* and the detection records: every
row of a stack of settings carries the bits the setting gives alone, the whole stack costs one launch per step, and a score that
cannot be computed has no key."""
import numpy as np
import pytest
import torch

from score_cases import DEV, bits, host

pytestmark = pytest.mark.gpu

R = 3
LAUNCHES = ["anoddpm_roc_auc", "anoddpm_ssim", "anoddpm_median2d", "anoddpm_roc_auc", "anoddpm_component_areas", "anoddpm_pro_auc",
            "anoddpm_small_components", "anoddpm_surface_distance"]
CURVE_KEYS = {"auc", "ap", "best_dice", "best_threshold", "auc_status"}
PRO_KEYS = {"aupro", "aupro_regions", "aupro_status"}
SURFACE_KEYS = {"hd", "hd95", "assd", "surface_status"}


def _stacks():
    """real, mask [2, 1, 48, 40] (two regions in image 0, none in image 1: that plane has no reference border) and the mean /
    sqerr / pred stacks [3, 2, 1, 48, 40] of three reconstructions that miss the regions by different amounts."""
    from anoddpm_amd import metrics
    rng = np.random.default_rng(21)
    real = (rng.random((2, 1, 48, 40)) * 1.6 - 0.8).astype(np.float32)
    mask = np.zeros_like(real)
    mask[0, 0, 5:25, 4:22] = 1
    mask[0, 0, 40:42, 30:33] = 1
    shifted = np.roll(mask, (2, 3), (2, 3))
    shifted[1, 0, 20:24, 10:14] = 1
    real_d, mask_d = torch.from_numpy(real).to(DEV), torch.from_numpy(mask).to(DEV)
    maps = []
    for j in range(R):
        noise = (rng.random(real.shape).astype(np.float32) - 0.5) * (0.2 + 0.2 * j)
        recon = real + noise + shifted * (0.9 + 0.3 * rng.random(real.shape).astype(np.float32))
        maps.append(metrics.anomaly_maps(real_d, torch.from_numpy(recon.astype(np.float32)).to(DEV), mask_d)[0])
    return real_d, mask_d, [torch.stack([m[k] for m in maps]) for k in ("mean", "sqerr", "pred")]


def test_score_maps_rows_are_independent_of_the_batch(monkeypatch):
    from anoddpm_amd import _lib, metrics
    real, mask, stacks = _stacks()
    options = dict(postprocess=metrics.PostProcess(median=3, erode=0, min_size=2), pro_limit=0.3, surface=True)
    L = _lib.lib()
    calls = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(L, name)
            if name.endswith("_workspace_bytes"):
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped

    monkeypatch.setattr(metrics, "lib", Spy)
    whole = metrics.score_maps(real, *stacks, mask, **options)
    monkeypatch.undo()
    assert calls == LAUNCHES                                              # one launch per step for the three settings; no erosion without a region of interest
    pp_keys = {"sqerr_pp", "pred_pp"} | {k + "_pp" for k in ("auc", "ap", "best_dice", "best_threshold", "aupro", "hd", "hd95", "assd")} | {"auc_pp_status"}
    assert set(whole) == CURVE_KEYS | PRO_KEYS | SURFACE_KEYS | pp_keys | {"ssim"}
    assert host(whole["surface_status"]).tolist() == [[0, 2]] * R and host(whole["aupro_regions"]).tolist() == [2] * R
    for j in range(R):
        alone = metrics.score_maps(real, *(s[j:j + 1] for s in stacks), mask, **options)
        assert set(alone) == set(whole)
        for k, v in whole.items():
            assert v.is_cuda and v.shape[0] == R and alone[k].shape == (1,) + v.shape[1:], k
            assert bits(host(v[j]), host(alone[k][0])), (j, k)
    assert all(np.isfinite(host(whole[k])).all() for k in ("auc", "ap", "best_dice", "aupro", "hd", "hd95", "assd", "ssim"))
    # without a mask: what needs none is still there
    bare = metrics.score_maps(real, *stacks, None, **options)
    assert set(bare) == {"ssim", "sqerr_pp"}
    assert bits(host(bare["ssim"]), host(whole["ssim"])) and bits(host(bare["sqerr_pp"]), host(whole["sqerr_pp"]))
