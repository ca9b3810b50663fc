"""-m gpu: the native precision-recall curve, average precision and best Dice (step 6 of csrc/roc.hip through metrics.pr_points /
PR_curve / average_precision / best_dice, anomaly_metrics and the detection records) against the fixture tests/golden/pr_kat.npz
with the criteria of tests/test_pr_reference.py: curve arrays bit-equal to sklearn's, AP within n * 2^-52 of sklearn's (and bit-equal
to the numpy restatement, which adds in the kernel's order), best Dice / threshold / counts equal to the brute-force search.  The
ROC outputs of a launch that also asks for the new ones are bit-equal to a plain launch.  sklearn itself is not needed."""
import os

import numpy as np
import pytest
import torch

import pr_cases as pc
import roc_cases as rc
from conftest import GOLDEN
from score_cases import tiny as _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "pr_kat.npz"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same_as_restatement(p, want, what):
    assert (p["P"], p["N"]) == (want["P"], want["N"]), what
    assert np.array_equal(p["fps"], want["fps"]) and np.array_equal(p["tps"], want["tps"]), what
    assert rc.bits_equal(p["thresholds"], np.ascontiguousarray(want["thresholds"])), what
    assert rc.bits_equal(np.float64(p["ap"]), np.float64(want["ap"])), (what, p["ap"], want["ap"])      # same summation order
    assert pc.same_float(p["best_dice"], want["best_dice"]) and p["best_threshold"] == float(want["best_threshold"]), what
    assert (p["best_tp"], p["best_fp"]) == (want["best_tp"], want["best_fp"]), what


def _check_functions_equal_points(m, s, p, what):
    """average_precision / best_dice: device tensors with the values pr_points copies out."""
    from anoddpm_amd import metrics
    ap = metrics.average_precision(m, s, batched=False)
    assert ap.shape == (1,) and ap.dtype == torch.float64 and ap.is_cuda
    assert rc.bits_equal(ap.cpu().numpy(), np.array([p["ap"]], np.float64)), what
    b = metrics.best_dice(m, s, batched=False)
    assert b["dice"].dtype == torch.float64 and b["threshold"].dtype == torch.float32 and b["tp"].dtype == b["fp"].dtype == torch.int64
    assert all(b[k].shape == (1,) and b[k].is_cuda for k in ("dice", "threshold", "tp", "fp"))
    assert rc.bits_equal(b["dice"].cpu().numpy(), np.array([p["best_dice"]], np.float64)), what
    assert float(b["threshold"][0]) == p["best_threshold"] and (int(b["tp"][0]), int(b["fp"][0])) == (p["best_tp"], p["best_fp"]), what


def _check_dice_dominates_fixed_cuts(m, s, p, what):
    """Property: the best Dice is at least the plain Dice 2 c[2] / (c[0] + c[1]) of anomaly_maps' counts at any fixed cut.
    real = 0 and recon = sqrt(score) make sqerr = fl(fl(sqrt(score))^2), a non-decreasing function of the score, so the
    prediction sqerr > cut is `score >= v` for one of the distinct scores v (or empty): one of the cuts the maximum runs over."""
    from anoddpm_amd import metrics
    real, recon = torch.zeros_like(s).reshape(1, -1), s.sqrt().reshape(1, -1)
    for cut in (0.25, 0.5, 1.0):
        c = metrics.anomaly_maps(real, recon, m.reshape(1, -1), threshold=cut, want=())[1].cpu().numpy()[0]
        if c[0] + c[1] == 0 or p["P"] == 0:
            continue                                                    # 0 / 0, or NaN by convention: nothing to compare
        fixed = 2.0 * c[2] / (c[0] + c[1])
        print(f"{what}: best dice {p['best_dice']!r} at {p['best_threshold']!r}; dice at the cut {cut}: {fixed!r}")
        assert p["best_dice"] >= fixed, (what, cut)


@pytest.mark.parametrize("name", pc.SMALL)
def test_small_cases_match_fixture(kat, name):
    from anoddpm_amd import metrics
    mask, score = kat[f"{name}_mask"], kat[f"{name}_score"]
    m, s = _dev(mask), _dev(score)
    prec, rec, thr = metrics.PR_curve(m, s)
    assert rc.bits_equal(prec, kat[f"{name}_prec"])
    assert rc.bits_equal(rec, kat[f"{name}_rec"])
    assert rc.bits_equal(thr, kat[f"{name}_thr"])
    p = metrics.pr_points(m, s)[0]
    pc.check_ap(p["ap"], float(kat[f"{name}_ap"]), p["P"], score.size, name)
    pc.check_best(kat, name, None, p, name)
    _same_as_restatement(p, pc.pr_numpy(mask, score), name)
    _check_functions_equal_points(m, s, p, name)
    _check_dice_dominates_fixed_cuts(m, s, p, name)


@pytest.mark.parametrize("name", pc.SUMMARISED)
def test_maps_and_long_segment_match_fixture(kat, name):
    from anoddpm_amd import metrics
    mask, score = pc.make_case(name)
    assert rc.sha_inputs(mask, score) == str(kat[f"{name}_sha"]), f"{name}: regenerated input differs from the fixture's"
    m, s = _dev(mask), _dev(score)
    p = metrics.pr_points(m, s)[0]
    pc.check_summary(kat, name, 0, p, score.size)
    _same_as_restatement(p, pc.pr_numpy(mask, score), name)
    _check_functions_equal_points(m, s, p, name)
    _check_dice_dominates_fixed_cuts(m, s, p, name)
    side = int(round(score.size ** 0.5))                                # the reference's shapes: [1, 1, H, W] tensors are flattened
    prec, rec, thr = metrics.PR_curve(m.reshape(1, 1, side, -1), s.reshape(1, 1, side, -1))
    assert rc.sha_curve(prec, rec, thr) == str(kat[f"{name}_curve_sha"][0])


def test_chunk_with_a_ragged_second_scatter_group():
    from anoddpm_amd import metrics
    mask, score = rc.make_ragged()
    assert score.size == 5000 and 0 < mask.sum() < mask.size
    _same_as_restatement(metrics.pr_points(_dev(mask), _dev(score))[0], pc.pr_numpy(mask, score), "ragged")


def test_batch_of_55_strided_rows_and_shared_mask(kat):
    from anoddpm_amd import metrics
    masks, scores = rc.make_batch()
    assert rc.sha_inputs(masks, scores) == str(kat["batch_sha"]), "batch: regenerated input differs from the fixture's"
    m, s = _dev(masks).reshape(rc.BATCH, 1, rc.SIDE, rc.SIDE), _dev(scores).reshape(rc.BATCH, 1, rc.SIDE, rc.SIDE)
    pts = metrics.pr_points(m, s)                                       # dim >= 3: one segment per leading index, mask rows strided
    ap = metrics.average_precision(m, s)
    best = metrics.best_dice(m, s)
    assert ap.shape == (rc.BATCH,) and best["dice"].shape == (rc.BATCH,)
    ap_h, bd_h, bt_h = ap.cpu().numpy(), best["dice"].cpu().numpy(), best["threshold"].cpu().numpy()
    for j in range(rc.BATCH):
        pc.check_summary(kat, "batch", j, pts[j], rc.N256)
        assert rc.bits_equal(ap_h[j], np.float64(pts[j]["ap"])) and rc.bits_equal(bd_h[j], np.float64(pts[j]["best_dice"])), j
        assert float(bt_h[j]) == pts[j]["best_threshold"], j
        assert (int(best["tp"][j]), int(best["fp"][j])) == (pts[j]["best_tp"], pts[j]["best_fp"]), j
        _check_dice_dominates_fixed_cuts(m[j].reshape(-1), s[j].reshape(-1), pts[j], f"batch[{j}]")
    assert np.isnan(ap_h[rc.BATCH_ALL_ZERO_MASK]) and np.isnan(ap_h).sum() == 1
    assert np.isnan(bd_h[rc.BATCH_ALL_ZERO_MASK]) and np.isnan(bd_h).sum() == 1
    for j in (0, 7, 54):                                                # a single-segment launch gives the same bits
        single = metrics.pr_points(m[j], s[j], batched=False)[0]
        _same_as_restatement(single, pts[j], f"single[{j}]")
    # rows of a wider matrix: segment stride 65536, length 5000 (ragged against waves and the workgroup)
    n = 5000
    wide_m, wide_s = _dev(masks[:4]), _dev(scores[:4])
    assert wide_s[:, :n].stride(0) == rc.N256
    got = metrics.pr_points(wide_m[:, :n], wide_s[:, :n], batched=True)
    for j in range(4):
        _same_as_restatement(got[j], pc.pr_numpy(masks[j, :n], scores[j, :n]), f"strided[{j}]")
    # one mask shared by every segment (mask_stride 0: what the detection sweep passes)
    shared = metrics.pr_points(m[3], s)
    ap_s, best_s = metrics.average_precision(m[3], s).cpu().numpy(), metrics.best_dice(m[3], s)
    for j in (0, 3, 21, 54):
        _same_as_restatement(shared[j], pc.pr_numpy(masks[3], scores[j]), f"shared[{j}]")
        assert rc.bits_equal(ap_s[j], np.float64(shared[j]["ap"])) and int(best_s["tp"][j]) == shared[j]["best_tp"]
    pc.check_summary(kat, "batch", 3, shared[3], rc.N256)


def test_roc_outputs_are_unchanged_by_the_new_outputs(kat):
    """AUC, counts and the dropped ROC curve of a launch that also computes AP and best Dice are those of a plain launch."""
    from anoddpm_amd import metrics
    masks, scores = rc.make_batch()
    m, s = _dev(masks[:8]), _dev(scores[:8])
    plain = metrics._roc_launch(m, s, True, True)
    plain_nocurve = metrics._roc_launch(m, s, True, False)
    full = metrics._roc_launch(m, s, True, False, pr=True)              # AP + best Dice, no curve
    for k in ("auc", "counts", "status"):
        assert rc.bits_equal(plain[k].cpu().numpy(), full[k].cpu().numpy()), k
        assert rc.bits_equal(plain[k].cpu().numpy(), plain_nocurve[k].cpu().numpy()), k
    assert rc.bits_equal(metrics.roc_auc(m, s, batched=True).cpu().numpy(), full["auc"].cpu().numpy())
    # the dropped curve beside the new outputs: curve_mode stays 0 while ap / best_* are requested
    mixed = _launch_dropped_curve_with_extras(m, s)
    for k in ("auc", "counts", "status", "len"):
        assert rc.bits_equal(plain[k].cpu().numpy(), mixed[k].cpu().numpy()), k
    for j, L in enumerate(plain["len"].tolist()):
        for k in ("fps", "tps", "thresholds"):
            assert rc.bits_equal(plain[k][j, :L].cpu().numpy(), mixed[k][j, :L].cpu().numpy()), (k, j)
    assert rc.bits_equal(mixed["ap"].cpu().numpy(), full["ap"].cpu().numpy())
    # and the host-facing functions
    want = metrics.roc_points(m, s, batched=True)
    for j in range(8):
        r = rc.roc_numpy(masks[j], scores[j])
        assert (want[j]["P"], want[j]["N"], want[j]["twoU"]) == (r["P"], r["N"], r["twoU"])
        assert int(mixed["counts"][j, 2]) == r["twoU"]


def _launch_dropped_curve_with_extras(m, s):
    """One anoddpm_roc_auc call with sklearn's dropped ROC curve AND ap / best_*: metrics has no caller of that combination."""
    import ctypes
    from anoddpm_amd import _lib
    S, n = m.shape
    nbytes = _lib.lib().anoddpm_roc_workspace_bytes(S, n)
    ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=DEV)
    o = {"auc": torch.empty((S,), dtype=torch.float64, device=DEV), "counts": torch.empty((S, 4), dtype=torch.int64, device=DEV),
         "status": torch.empty((S,), dtype=torch.int32, device=DEV), "fps": torch.empty((S, n), dtype=torch.int32, device=DEV),
         "tps": torch.empty((S, n), dtype=torch.int32, device=DEV), "thresholds": torch.empty((S, n), dtype=torch.float32, device=DEV),
         "len": torch.empty((S,), dtype=torch.int32, device=DEV), "ap": torch.empty((S,), dtype=torch.float64, device=DEV),
         "best_dice": torch.empty((S,), dtype=torch.float64, device=DEV), "best_thr": torch.empty((S,), dtype=torch.float32, device=DEV),
         "best_counts": torch.empty((S, 2), dtype=torch.int64, device=DEV)}
    a = _lib.RocArgs()
    a.score, a.mask, a.workspace, a.workspace_bytes = s.data_ptr(), m.data_ptr(), ws.data_ptr(), nbytes
    a.auc, a.counts, a.status = o["auc"].data_ptr(), o["counts"].data_ptr(), o["status"].data_ptr()
    a.curve_fps, a.curve_tps, a.curve_thr = o["fps"].data_ptr(), o["tps"].data_ptr(), o["thresholds"].data_ptr()
    a.curve_len, a.curve_cap, a.curve_mode = o["len"].data_ptr(), n, _lib.ROC_CURVE_DROP
    a.ap, a.best_dice, a.best_thr, a.best_counts = (o[k].data_ptr() for k in ("ap", "best_dice", "best_thr", "best_counts"))
    a.n, a.score_stride, a.mask_stride, a.S = n, s.stride(0), m.stride(0), S
    _lib.check(_lib.lib().anoddpm_roc_auc(ctypes.byref(a), _lib.current_stream()), "roc_auc")
    torch.cuda.synchronize()
    return o


def test_two_launches_give_the_same_bits(kat):
    from anoddpm_amd import metrics
    masks, scores = rc.make_batch()
    m, s = _dev(masks[:6]), _dev(scores[:6])
    a, b = metrics._roc_launch(m, s, True, True, pr=True), metrics._roc_launch(m, s, True, True, pr=True)
    for k in ("ap", "best_dice", "best_threshold", "best_counts", "auc", "counts", "status", "len"):
        assert rc.bits_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    for j, L in enumerate(a["len"].tolist()):
        assert L == int(a["counts"][j, 3])                              # the full curve: one point per distinct score
        for k in ("fps", "tps", "thresholds"):
            assert rc.bits_equal(a[k][j, :L].cpu().numpy(), b[k][j, :L].cpu().numpy()), (k, j)
    mask, score = pc.make_case("long")
    ml, sl = _dev(mask), _dev(score)
    assert rc.bits_equal(metrics.average_precision(ml, sl).cpu().numpy(), metrics.average_precision(ml, sl).cpu().numpy())


BAD = (("nan", float("nan"), None, "NaN"), ("inf", float("inf"), None, "infinite"), ("negative", -0.25, None, "negative"),
       ("mask2", None, 2.0, "mask value"))


@pytest.mark.parametrize("what,bad_score,bad_mask,text", BAD)
def test_status_word_and_nan_for_inputs_outside_the_precondition(kat, what, bad_score, bad_mask, text):
    from anoddpm_amd import _lib, metrics
    mask, score = kat["n1025_mask"].copy(), kat["n1025_score"].copy()
    if bad_score is not None:
        score[700] = bad_score
    if bad_mask is not None:
        mask[700] = bad_mask
    m, s = _dev(mask), _dev(score)
    with pytest.raises(ValueError, match=text):
        metrics.PR_curve(m, s)
    with pytest.raises(ValueError, match=text):
        metrics.pr_points(m, s)
    bit = {"nan": _lib.ROC_NAN, "inf": _lib.ROC_INF, "negative": _lib.ROC_NEGATIVE, "mask2": _lib.ROC_BAD_MASK}[what]
    ap, status = metrics.average_precision(m, s, return_status=True)    # no exception, no synchronisation: NaN beside the status
    assert np.isnan(float(ap[0])) and int(status[0]) == bit
    b = metrics.best_dice(m, s)
    assert np.isnan(float(b["dice"][0])) and int(b["status"][0]) == bit
    # only the bad segment of a batch is affected
    good_m, good_s = _dev(kat["n1025_mask"]), _dev(kat["n1025_score"])
    ap2, status2 = metrics.average_precision(torch.stack([good_m, m]), torch.stack([good_s, s]), batched=True, return_status=True)
    assert status2.tolist() == [0, bit] and np.isnan(float(ap2[1]))
    pc.check_ap(float(ap2[0]), float(kat["n1025_ap"]), 1, 1025, "good segment beside a bad one")
    b2 = metrics.best_dice(torch.stack([good_m, m]), torch.stack([good_s, s]), batched=True)
    assert float(b2["dice"][0]) == float(kat["n1025_best_dice"]) and np.isnan(float(b2["dice"][1]))
    if what in ("nan", "mask2"):                                        # anomaly_metrics keeps working: NaN beside AUC_status
        real = torch.zeros(1, 1, 25, 41, device=DEV)
        recon = s.clamp_min(0).sqrt().reshape(1, 1, 25, 41) if what == "mask2" else s.reshape(1, 1, 25, 41)
        r = metrics.anomaly_metrics(real, recon, m.reshape(1, 1, 25, 41))
        assert r["AUC_status"] == bit and all(np.isnan(r[k]) for k in ("AUC", "AP", "best_dice", "best_threshold"))


def test_negative_zero_counts_as_zero():
    from anoddpm_amd import metrics
    m = torch.tensor([0, 1, 1, 0], dtype=torch.float32, device=DEV)
    s = torch.tensor([0.0, -0.0, 0.0, -0.0], dtype=torch.float32, device=DEV)
    p = metrics.pr_points(m, s)[0]
    assert p["ap"] == 0.5 and p["thresholds"].view(np.uint32).tolist() == [0] and p["fps"].tolist() == [2] and p["tps"].tolist() == [2]
    assert (p["best_dice"], p["best_tp"], p["best_fp"]) == (2 * 2 / (4 + 2), 2, 2)


def test_anomaly_metrics_ap_and_best_dice_come_with_the_auc(kat):
    from anoddpm_amd import metrics
    torch.manual_seed(5)
    real = torch.rand(3, 1, 64, 64, device=DEV) * 2 - 1
    recon = real + torch.randn(3, 1, 64, 64, device=DEV) * 0.3
    mask = (torch.rand(3, 1, 64, 64, device=DEV) > 0.9).float()
    recon = recon + mask * 0.4
    r = metrics.anomaly_metrics(real, recon, mask)
    sq = r["maps"]["sqerr"].reshape(-1)
    assert r["AUC_status"] == 0 and r["AUC"] == float(metrics.roc_auc(mask.reshape(-1), sq)[0])      # the value it had
    assert r["AP"] == float(metrics.average_precision(mask.reshape(-1), sq)[0]) and 0.1 < r["AP"] < 1.0
    b = metrics.best_dice(mask.reshape(-1), sq)
    assert r["best_dice"] == float(b["dice"][0]) and r["best_threshold"] == float(b["threshold"][0])
    want = pc.pr_numpy(mask.cpu().numpy(), sq.cpu().numpy())
    assert rc.bits_equal(np.float64(r["AP"]), np.float64(want["ap"])) and r["best_dice"] == want["best_dice"]
    c = metrics.anomaly_maps(real, recon, mask)[1].cpu().numpy()        # the reference's cut 0.5, over the whole batch
    assert r["best_dice"] >= 2.0 * c[:, 2].sum() / (c[:, 0].sum() + c[:, 1].sum())
    no_mask = metrics.anomaly_metrics(real, recon, None)
    assert all(np.isnan(no_mask[k]) for k in ("AUC", "AP", "best_dice", "best_threshold")) and no_mask["AUC_status"] == 0
    no_pos = metrics.anomaly_metrics(real, recon, torch.zeros_like(mask))
    assert all(np.isnan(no_pos[k]) for k in ("AUC", "AP", "best_dice", "best_threshold")) and no_pos["AUC_status"] == 0


def test_detection_records_carry_ap_and_best_dice(tmp_path, monkeypatch):
    from anoddpm_amd import metrics
    GD, m, d = _tiny()
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(1)
    x_0 = torch.rand(1, 1, 32, 32, device=DEV) * 2 - 1
    mask = (torch.rand(1, 1, 32, 32, device=DEV) > 0.7).float()
    args = {"arg_num": 9, "T": 200, "img_size": [32, 32]}                # settings 50, 100, 150: one launch of three segments
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert [r["t_distance"] for r in d.last_detection] == [50, 100, 150]
    for rec in d.last_detection:
        for k, dt in (("ap", torch.float64), ("best_dice", torch.float64), ("best_threshold", torch.float32), ("auc", torch.float64)):
            assert rec[k].is_cuda and rec[k].dtype == dt and rec[k].dim() == 0, k
        sqerr = metrics.anomaly_maps(x_0, rec["output"], mask)[0]["sqerr"]       # rec["mse"] is sqerr * 2 - 1, not the score
        assert rc.bits_equal(rec["auc"].cpu().numpy().reshape(1), metrics.roc_auc(mask, sqerr).cpu().numpy())
        assert rc.bits_equal(rec["ap"].cpu().numpy().reshape(1), metrics.average_precision(mask, sqerr).cpu().numpy())
        b = metrics.best_dice(mask, sqerr)
        assert rc.bits_equal(rec["best_dice"].cpu().numpy().reshape(1), b["dice"].cpu().numpy())
        assert rc.bits_equal(rec["best_threshold"].cpu().numpy().reshape(1), b["threshold"].cpu().numpy())
        assert int(rec["auc_status"]) == 0 and 0.0 < float(rec["ap"]) <= 1.0 and 0.0 < float(rec["best_dice"]) <= 1.0
        want = pc.pr_numpy(mask.cpu().numpy(), sqerr.cpu().numpy())
        assert rc.bits_equal(np.float64(float(rec["ap"])), np.float64(want["ap"])) and float(rec["best_dice"]) == want["best_dice"]
    # an all-zero mask: NaN, status 0
    d.detection_B(m, x_0, args, ("vol", "slice"), torch.zeros_like(mask), denoise_fn="gauss", total_avg=2)
    assert all(np.isnan(float(r["ap"])) and np.isnan(float(r["best_dice"])) and int(r["auc_status"]) == 0 for r in d.last_detection)
    # no mask: the new keys are None, as auc is
    d.detection_B(m, x_0, args, ("vol", "slice"), None, denoise_fn="gauss", total_avg=2)
    assert all(r["auc"] is None and r["ap"] is None and r["best_dice"] is None and r["best_threshold"] is None for r in d.last_detection)
    assert not os.listdir(tmp_path)
