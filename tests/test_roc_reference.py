"""ROC / AUC without a device: the numpy restatement of csrc/roc.hip (tests/roc_cases.py: keys, sort, runs, integer twoU, sklearn's
drop rule) reproduces the sklearn fixture tests/golden/roc_kat.npz -- fpr / tpr / thresholds bit for bit, AUC within n * 2^-52 --
and the host-side pieces of the native path: argument validation of anoddpm_roc_auc through the ABI, the workspace-size function,
and the unchanged host path of metrics.ROC_AUC.  CPU only."""
import ctypes
import os

import numpy as np
import pytest

import roc_cases as rc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "roc_kat.npz"))


def _inputs(kat, name):
    if name in rc.SMALL:
        return kat[f"{name}_mask"], kat[f"{name}_score"]
    mask, score = rc.make_case(name)
    assert rc.sha_inputs(mask, score) == str(kat[f"{name}_sha"]), \
        f"{name}: the regenerated input differs from the one the fixture was made from (a numpy that draws differently?)"
    return mask, score


def _check_auc(got, want, n, what):
    print(f"{what}: auc {got!r} fixture {want!r} |diff| {abs(got - want):.3g} bound {rc.auc_tolerance(n):.3g}")
    if np.isnan(want):
        assert np.isnan(got), what
    else:
        assert abs(got - want) <= rc.auc_tolerance(n), what


@pytest.mark.parametrize("name", rc.SMALL + rc.MAPS)
def test_restatement_reproduces_sklearn_curve_and_auc(kat, name):
    mask, score = _inputs(kat, name)
    r = rc.roc_numpy(mask, score)
    fpr, tpr, thr = rc.sklearn_triple(r["fps"], r["tps"], r["thresholds"])
    assert rc.bits_equal(fpr, kat[f"{name}_fpr"])
    assert rc.bits_equal(tpr, kat[f"{name}_tpr"])
    assert rc.bits_equal(thr, kat[f"{name}_thr"])
    _check_auc(r["auc"], float(kat[f"{name}_auc"]), score.size, name)
    assert r["P"] + r["N"] == score.size and r["P"] == int((mask != 0).sum())


def test_restatement_special_values(kat):
    assert float(kat["all_equal_auc"]) == 0.5 and kat["all_equal_fpr"].size == 2
    assert rc.roc_numpy(kat["all_equal_mask"], kat["all_equal_score"])["twoU"] == \
        int(kat["all_equal_mask"].sum()) * int((kat["all_equal_mask"] == 0).sum())
    assert np.isnan(kat["mask_all0_auc"]) and np.isnan(kat["mask_all0_tpr"]).all()
    assert np.isnan(kat["mask_all1_auc"]) and np.isnan(kat["mask_all1_fpr"]).all()
    # -0.0 counts as +0.0: one run, threshold +0.0
    r = rc.roc_numpy(np.array([0, 1, 1, 0], np.float32), np.array([0.0, -0.0, 0.0, -0.0], np.float32))
    assert r["R"] == 1 and r["auc"] == 0.5 and r["thresholds"].view(np.uint32)[0] == 0


def _check_summary(kat, prefix, masks, scores):
    assert rc.sha_inputs(masks, scores) == str(kat[f"{prefix}_sha"]), \
        f"{prefix}: the regenerated input differs from the one the fixture was made from (a numpy that draws differently?)"
    for j, (mask, score) in enumerate(zip(masks, scores)):
        r = rc.roc_numpy(mask, score)
        fpr, tpr, thr = rc.sklearn_triple(r["fps"], r["tps"], r["thresholds"])
        assert (r["P"], r["N"], r["twoU"]) == (int(kat[f"{prefix}_P"][j]), int(kat[f"{prefix}_N"][j]), int(kat[f"{prefix}_twoU"][j]))
        assert fpr.size == int(kat[f"{prefix}_len"][j])
        assert rc.sha_curve(fpr, tpr, thr) == str(kat[f"{prefix}_curve_sha"][j]), (prefix, j)
        _check_auc(r["auc"], float(kat[f"{prefix}_auc"][j]), score.size, f"{prefix}[{j}]")


def test_restatement_long_segment(kat):
    mask, score = rc.make_case("long")
    _check_summary(kat, "long", mask[None], score[None])


def test_restatement_batch_of_55(kat):
    masks, scores = rc.make_batch()
    _check_summary(kat, "batch", masks, scores)
    assert np.isnan(kat["batch_auc"][rc.BATCH_ALL_ZERO_MASK]) and np.isnan(kat["batch_auc"]).sum() == 1


def test_ragged_case_is_what_it_is_for():
    mask, score = rc.make_ragged()
    assert score.size == rc.RAGGED_N == 5000 and 0 < mask.sum() < mask.size
    bits = (score + np.float32(0)).view(np.uint32)
    for border in range(320, 5000, 320):                                 # the 320-element wave chunks: a tie across every border
        assert np.intersect1d(bits[border - 64:border], bits[border:border + 64]).size, border


def test_roc_abi_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 25 and L.anoddpm_struct_size(b"anoddpm_roc_args") == ctypes.sizeof(_lib.RocArgs)
    assert L.anoddpm_roc_auc(None, None) == -1 and b"null args" in L.anoddpm_last_error()
    a = _lib.RocArgs()
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"null pointer" in L.anoddpm_last_error()
    # host memory stands in for the device pointers: every case below is rejected before anything is launched
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    a.score = a.mask = a.workspace = a.auc = a.counts = a.status = p
    a.S, a.n = 0, 16
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"S must be" in L.anoddpm_last_error()
    a.S, a.n = 1, 0
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"n must be >= 1" in L.anoddpm_last_error()
    a.n = 1 << 31
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"2^31" in L.anoddpm_last_error()
    a.S, a.n, a.score_stride, a.mask_stride = 2, 16, 8, 0
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"score_stride" in L.anoddpm_last_error()
    a.score_stride, a.mask_stride = 16, 8
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"mask_stride" in L.anoddpm_last_error()
    a.mask_stride, a.workspace_bytes = 0, L.anoddpm_roc_workspace_bytes(2, 16) - 1
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"workspace too small" in L.anoddpm_last_error()
    a.workspace_bytes += 1
    a.curve_fps = p                                                     # some but not all of the curve outputs
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"curve output needs" in L.anoddpm_last_error()
    a.curve_tps = a.curve_thr = a.curve_len = p
    a.curve_cap = 1
    assert L.anoddpm_roc_auc(ctypes.byref(a), None) == -1 and b"curve capacity" in L.anoddpm_last_error()


def test_roc_workspace_bytes():
    from anoddpm_amd import _lib
    L = _lib.lib()
    for S, n in ((1, 1), (1, 63), (1, 64), (55, 65536), (1, 1 << 22), (3, (1 << 31) - 1)):
        words = (n + 1 + 63) // 64 * 64                                 # keys, and run records with their sentinel
        assert L.anoddpm_roc_workspace_bytes(S, n) == S * 3 * words * 4
    for S, n in ((0, 8), (-1, 8), (1, 0), (1, -5), (1, 1 << 31)):
        assert L.anoddpm_roc_workspace_bytes(S, n) == -1


def test_host_inputs_of_ROC_AUC_still_go_through_sklearn(kat):
    pytest.importorskip("sklearn")
    import torch
    from sklearn.metrics import auc, roc_curve
    from anoddpm_amd import metrics
    mask, score = kat["round4_4096_mask"], kat["round4_4096_score"]
    want = roc_curve(mask, score)
    for got in (metrics.ROC_AUC(mask.reshape(64, 64), score.reshape(64, 64)),
                metrics.ROC_AUC(torch.from_numpy(mask).reshape(1, 1, 64, 64), torch.from_numpy(score).reshape(1, 1, 64, 64))):
        assert all(rc.bits_equal(g, w) for g, w in zip(got, want))
    assert metrics.AUC_score(want[0], want[1]) == auc(want[0], want[1])
    assert {"roc_auc", "roc_points"} <= set(metrics.__all__)
