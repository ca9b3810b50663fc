"""Precision-recall curve, average precision and best Dice without a device: the numpy restatement of step 6 of csrc/roc.hip
(tests/pr_cases.py: the walk over the runs of equal score) reproduces the fixture tests/golden/pr_kat.npz -- sklearn's precision /
recall / thresholds bit for bit, its average precision within n * 2^-52, the brute-force best Dice, threshold and counts exactly
-- and the host-side pieces of the native path: validation of the new fields of anoddpm_roc_args through the ABI, and the host
path of metrics.PR_curve.  CPU only."""
import ctypes
import os

import numpy as np
import pytest

import pr_cases as pc
import roc_cases as rc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "pr_kat.npz"))


@pytest.mark.parametrize("name", pc.SMALL)
def test_restatement_reproduces_sklearn_curve_ap_and_brute_force_best_dice(kat, name):
    mask, score = kat[f"{name}_mask"], kat[f"{name}_score"]
    assert rc.bits_equal(mask, pc.make_case(name)[0]) and rc.bits_equal(score, pc.make_case(name)[1])
    r = pc.pr_numpy(mask, score)
    prec, rec, thr = pc.sklearn_triple(r["fps"], r["tps"], r["thresholds"])
    assert rc.bits_equal(prec, kat[f"{name}_prec"])
    assert rc.bits_equal(rec, kat[f"{name}_rec"])
    assert rc.bits_equal(thr, kat[f"{name}_thr"])
    pc.check_ap(r["ap"], float(kat[f"{name}_ap"]), r["P"], score.size, name)
    pc.check_best(kat, name, None, r, name)
    assert r["P"] == int((mask != 0).sum()) and r["R"] == np.unique(score + np.float32(0)).size == prec.size - 1


@pytest.mark.parametrize("name", pc.SUMMARISED)
def test_restatement_maps_and_long_segment(kat, name):
    mask, score = pc.make_case(name)
    assert rc.sha_inputs(mask, score) == str(kat[f"{name}_sha"]), \
        f"{name}: the regenerated input differs from the one the fixture was made from (a numpy that draws differently?)"
    pc.check_summary(kat, name, 0, pc.pr_numpy(mask, score), score.size)


def test_restatement_batch_of_55(kat):
    masks, scores = rc.make_batch()
    assert rc.sha_inputs(masks, scores) == str(kat["batch_sha"]), "batch: the regenerated input differs from the fixture's"
    for j in range(rc.BATCH):
        pc.check_summary(kat, "batch", j, pc.pr_numpy(masks[j], scores[j]), scores[j].size)
    assert np.isnan(kat["batch_best_dice"][rc.BATCH_ALL_ZERO_MASK]) and np.isnan(kat["batch_best_dice"]).sum() == 1


def test_special_cases(kat):
    # one score only: a single point, precision = prevalence, AP = prevalence; Dice = 2 P / (n + P)
    r = pc.pr_numpy(kat["all_equal_mask"], kat["all_equal_score"])
    P, n = r["P"], 4096
    assert r["R"] == 1 and r["ap"] == P / n and r["best_dice"] == 2 * P / (n + P) and (r["best_tp"], r["best_fp"]) == (P, n - P)
    # no positive: NaN, recall all ones as sklearn's; the threshold that is left is the highest score
    r = pc.pr_numpy(kat["mask_all0_mask"], kat["mask_all0_score"])
    assert np.isnan(r["ap"]) and np.isnan(r["best_dice"]) and r["best_tp"] == 0 and r["best_threshold"] == kat["mask_all0_score"].max()
    assert (kat["mask_all0_rec"][:-1] == 1).all() and (kat["mask_all0_prec"][:-1] == 0).all() and float(kat["mask_all0_ap"]) == 0.0
    # no negative: AP is exactly 1, the best cut keeps everything
    r = pc.pr_numpy(kat["mask_all1_mask"], kat["mask_all1_score"])
    assert r["ap"] == 1.0 and r["best_dice"] == 1.0 and (r["best_tp"], r["best_fp"]) == (4096, 0)
    assert r["best_threshold"] == kat["mask_all1_score"].min()
    # n == 1
    r = pc.pr_numpy(kat["n1_mask"], kat["n1_score"])
    assert r["R"] == 1 and r["fps"].size == 1
    # two thresholds reach the best Dice 1 / 2: the higher one is reported
    r = pc.pr_numpy(kat["tie_dice_mask"], kat["tie_dice_score"])
    assert (r["best_dice"], float(r["best_threshold"]), r["best_tp"], r["best_fp"]) == (0.5, 4.0, 1, 1)
    tps, fps = r["tps"], r["fps"]
    assert sorted(np.flatnonzero(2 * tps * 2 == (tps + fps + 2)).tolist()) == [1, 5]      # Dice == 1/2 at scores 4 and 0.5
    # -0.0 counts as +0.0
    r = pc.pr_numpy(np.array([0, 1, 1, 0], np.float32), np.array([0.0, -0.0, 0.0, -0.0], np.float32))
    assert r["R"] == 1 and r["ap"] == 0.5 and r["thresholds"].view(np.uint32)[0] == 0


def test_kernel_order_sum_is_a_sum():
    rng = np.random.default_rng(3)
    for size in (1, 63, 1024, 1025, 5000):
        t = rng.random(size)
        assert abs(pc._kernel_sum(t) - float(np.sum(t))) <= size * 2.0 ** -52 * max(1.0, float(np.sum(t)))
    assert pc._kernel_sum(np.array([0.25, 0.5])) == 0.75


def test_pr_abi_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 27 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    assert L.anoddpm_struct_size(b"anoddpm_roc_args") == ctypes.sizeof(_lib.RocArgs)
    names = [f[0] for f in _lib.RocArgs._fields_]
    assert {"ap", "best_dice", "best_thr", "best_counts", "curve_mode"} <= set(names)
    assert names.index("S") < min(names.index(k) for k in ("ap", "best_dice", "best_thr", "best_counts", "curve_mode"))      # appended
    # host memory stands in for the device pointers: every case below is rejected before anything is launched
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    a = _lib.RocArgs()
    a.score = a.mask = a.workspace = a.auc = a.counts = a.status = p
    a.S, a.n, a.workspace_bytes = 1, 16, L.anoddpm_roc_workspace_bytes(1, 16)
    a.curve_mode = 2
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"unknown curve_mode" in L.anoddpm_last_error()
    a.curve_mode = -1
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"unknown curve_mode" in L.anoddpm_last_error()
    a.curve_mode = _lib.ROC_CURVE_ALL                                   # the full curve without anywhere to write it
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"curve_mode needs" in L.anoddpm_last_error()
    a.curve_mode = _lib.ROC_CURVE_DROP
    for some in (("best_dice",), ("best_thr",), ("best_counts",), ("best_dice", "best_thr"), ("best_thr", "best_counts")):
        a.best_dice = a.best_thr = a.best_counts = None
        for k in some:
            setattr(a, k, p)
        assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"best Dice output needs" in L.anoddpm_last_error(), some
    # the existing checks still come first
    a.best_dice = a.best_thr = a.best_counts = a.ap = p
    a.workspace_bytes -= 1
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"workspace too small" in L.anoddpm_last_error()
    assert (_lib.ROC_CURVE_DROP, _lib.ROC_CURVE_ALL) == (0, 1)


def test_host_inputs_of_PR_curve_go_through_sklearn(kat):
    pytest.importorskip("sklearn")
    import torch
    from sklearn.metrics import precision_recall_curve
    from anoddpm_amd import metrics
    mask, score = kat["round4_4096_mask"], kat["round4_4096_score"]
    want = precision_recall_curve(mask, score)
    for got in (metrics.PR_curve(mask.reshape(64, 64), score.reshape(64, 64)),
                metrics.PR_curve(torch.from_numpy(mask).reshape(1, 1, 64, 64), torch.from_numpy(score).reshape(1, 1, 64, 64))):
        assert all(rc.bits_equal(g, w) for g, w in zip(got, want))
    assert rc.bits_equal(want[0], kat["round4_4096_prec"]) and rc.bits_equal(want[1], kat["round4_4096_rec"])


def test_new_names_are_exported():
    import evaluation
    from anoddpm_amd import metrics
    new = {"average_precision", "best_dice", "pr_points", "PR_curve"}
    assert new <= set(metrics.__all__)
    assert all(getattr(evaluation, k) is getattr(metrics, k) for k in new)
