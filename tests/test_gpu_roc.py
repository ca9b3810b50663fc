"""-m gpu: the native ROC / AUC (csrc/roc.hip through metrics.roc_auc / roc_points / ROC_AUC, anomaly_metrics and the detection
records) against the sklearn fixture tests/golden/roc_kat.npz: curve arrays bit-equal, AUC within n * 2^-52 (tests/roc_cases.py
derives the bound), integer counts equal to the numpy restatement.  sklearn itself is not needed."""
import os

import numpy as np
import pytest
import torch

import roc_cases as rc
from conftest import GOLDEN
from score_cases import tiny as _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "roc_kat.npz"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


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
def test_curve_and_auc_match_sklearn_fixture(kat, name):
    from anoddpm_amd import metrics
    mask, score = _inputs(kat, name)
    m, s = _dev(mask), _dev(score)
    fpr, tpr, thr = metrics.ROC_AUC(m, s)
    assert rc.bits_equal(fpr, kat[f"{name}_fpr"])
    assert rc.bits_equal(tpr, kat[f"{name}_tpr"])
    assert rc.bits_equal(thr, kat[f"{name}_thr"])
    auc = metrics.roc_auc(m, s)
    assert auc.shape == (1,) and auc.dtype == torch.float64 and auc.is_cuda
    _check_auc(float(auc[0]), float(kat[f"{name}_auc"]), score.size, name)
    # the integer counts behind it
    want = rc.roc_numpy(mask, score)
    p = metrics.roc_points(m, s)[0]
    assert (p["P"], p["N"], p["twoU"]) == (want["P"], want["N"], want["twoU"])
    assert np.array_equal(p["fps"], want["fps"]) and np.array_equal(p["tps"], want["tps"])
    assert rc.bits_equal(p["thresholds"], want["thresholds"])
    # the reference's shapes: [1, 1, H, W] tensors are flattened (evaluation.py:81)
    if score.size == rc.N256:
        got = metrics.ROC_AUC(m.reshape(1, 1, rc.SIDE, rc.SIDE), s.reshape(1, 1, rc.SIDE, rc.SIDE))
        assert all(rc.bits_equal(g, w) for g, w in zip(got, (fpr, tpr, thr)))


def test_chunk_with_a_ragged_second_scatter_group():
    from anoddpm_amd import metrics
    mask, score = rc.make_ragged()
    assert score.size == 5000 and 0 < mask.sum() < mask.size
    want = rc.roc_numpy(mask, score)
    p = metrics.roc_points(_dev(mask), _dev(score))[0]
    assert (p["P"], p["N"], p["twoU"]) == (want["P"], want["N"], want["twoU"])
    assert np.array_equal(p["fps"], want["fps"]) and np.array_equal(p["tps"], want["tps"])
    assert rc.bits_equal(p["thresholds"], want["thresholds"])
    assert rc.bits_equal(np.float64(p["auc"]), np.float64(want["auc"]))


def _check_summary(kat, prefix, j, p, mask, score):
    fpr, tpr, thr = rc.sklearn_triple(p["fps"], p["tps"], p["thresholds"])
    assert (p["P"], p["N"], p["twoU"]) == (int(kat[f"{prefix}_P"][j]), int(kat[f"{prefix}_N"][j]), int(kat[f"{prefix}_twoU"][j]))
    assert fpr.size == int(kat[f"{prefix}_len"][j])
    assert rc.sha_curve(fpr, tpr, thr) == str(kat[f"{prefix}_curve_sha"][j]), (prefix, j)
    _check_auc(p["auc"], float(kat[f"{prefix}_auc"][j]), score.size, f"{prefix}[{j}]")


def test_long_segment(kat):
    from anoddpm_amd import metrics
    mask, score = rc.make_case("long")
    assert rc.sha_inputs(mask[None], score[None]) == str(kat["long_sha"]), "long: regenerated input differs from the fixture's"
    m, s = _dev(mask), _dev(score)
    _check_summary(kat, "long", 0, metrics.roc_points(m, s)[0], mask, score)
    _check_auc(float(metrics.roc_auc(m, s)[0]), float(kat["long_auc"][0]), score.size, "long roc_auc")
    fpr, tpr, thr = metrics.ROC_AUC(m, s)
    assert rc.sha_curve(fpr, tpr, thr) == str(kat["long_curve_sha"][0])


def test_batch_of_55_equals_single_calls_and_fixture(kat):
    from anoddpm_amd import metrics
    masks, scores = rc.make_batch()
    assert rc.sha_inputs(masks, scores) == str(kat["batch_sha"]), "batch: regenerated input differs from the fixture's"
    m, s = _dev(masks).reshape(rc.BATCH, 1, rc.SIDE, rc.SIDE), _dev(scores).reshape(rc.BATCH, 1, rc.SIDE, rc.SIDE)
    auc = metrics.roc_auc(m, s)                                         # dim >= 3: one segment per leading index
    assert auc.shape == (rc.BATCH,)
    pts = metrics.roc_points(m, s)
    host = auc.cpu().numpy()
    for j in range(rc.BATCH):
        _check_summary(kat, "batch", j, pts[j], masks[j], scores[j])
        single = metrics.roc_auc(m[j], s[j], batched=False)
        assert rc.bits_equal(single.cpu().numpy(), host[j:j + 1]), j
        assert rc.bits_equal(np.float64(pts[j]["auc"]), host[j]), j
    assert np.isnan(host[rc.BATCH_ALL_ZERO_MASK]) and np.isnan(host).sum() == 1
    # one mask shared by every segment (what the detection sweep passes)
    shared = metrics.roc_auc(m[3], s).cpu().numpy()
    for j in (0, 3, 54):
        assert rc.bits_equal(shared[j:j + 1], metrics.roc_auc(m[3], s[j], batched=False).cpu().numpy())


def test_two_runs_are_bit_identical(kat):
    from anoddpm_amd import metrics
    masks, scores = rc.make_batch()
    m, s = _dev(masks[:6]), _dev(scores[:6])
    a, b = metrics._roc_launch(m, s, True, True), metrics._roc_launch(m, s, True, True)
    for k in ("auc", "counts", "status", "len"):
        assert rc.bits_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    for j, L in enumerate(a["len"].tolist()):
        for k in ("fps", "tps", "thresholds"):
            assert rc.bits_equal(a[k][j, :L].cpu().numpy(), b[k][j, :L].cpu().numpy()), (k, j)


def test_strided_and_non_contiguous_segments(kat):
    from anoddpm_amd import metrics
    masks, scores = rc.make_batch()
    n = 5000                                                            # ragged against waves and the workgroup
    want = [rc.roc_numpy(masks[j, :n], scores[j, :n]) for j in range(4)]
    big_m, big_s = _dev(masks[:4]), _dev(scores[:4])
    got = metrics.roc_auc(big_m[:, :n], big_s[:, :n], batched=True)     # rows of a wider matrix: segment stride 65536, length 5000
    assert big_s[:, :n].stride(0) == rc.N256
    for j in range(4):
        _check_auc(float(got[j]), want[j]["auc"], n, f"strided[{j}]")
        p = metrics.roc_points(big_m[j, :n], big_s[j, :n])[0]
        assert (p["P"], p["N"], p["twoU"]) == (want[j]["P"], want[j]["N"], want[j]["twoU"])
    # element stride 2 (copied to unit stride inside), and a transposed map
    ev = metrics.roc_auc(big_m[0, ::2], big_s[0, ::2])
    _check_auc(float(ev[0]), rc.roc_numpy(masks[0, ::2], scores[0, ::2])["auc"], rc.N256 // 2, "every other element")
    t_m, t_s = big_m[1].reshape(rc.SIDE, rc.SIDE).t(), big_s[1].reshape(rc.SIDE, rc.SIDE).t()
    assert rc.bits_equal(metrics.roc_auc(t_m, t_s).cpu().numpy(), metrics.roc_auc(big_m[1], big_s[1]).cpu().numpy())
    # other dtypes of the mask are converted
    assert rc.bits_equal(metrics.roc_auc(big_m[1].bool(), big_s[1]).cpu().numpy(), metrics.roc_auc(big_m[1], big_s[1]).cpu().numpy())


BAD = (("nan", float("nan"), None, "NaN"), ("inf", float("inf"), None, "infinite"), ("negative", -0.25, None, "negative"),
       ("mask2", None, 2.0, "mask value"))


@pytest.mark.parametrize("what,bad_score,bad_mask,text", BAD)
def test_status_word_for_inputs_outside_the_precondition(kat, what, bad_score, bad_mask, text):
    from anoddpm_amd import _lib, metrics
    mask, score = kat["n1025_mask"].copy(), kat["n1025_score"].copy()
    if bad_score is not None:
        score[700] = bad_score
    if bad_mask is not None:
        mask[700] = bad_mask
    m, s = _dev(mask), _dev(score)
    with pytest.raises(ValueError, match=text):
        metrics.ROC_AUC(m, s)
    with pytest.raises(ValueError, match=text):
        metrics.roc_points(m, s)
    auc, status = metrics.roc_auc(m, s, return_status=True)             # no exception, no synchronisation: NaN beside the status
    assert np.isnan(float(auc[0])) and int(status[0]) != 0
    bit = {"nan": _lib.ROC_NAN, "inf": _lib.ROC_INF, "negative": _lib.ROC_NEGATIVE, "mask2": _lib.ROC_BAD_MASK}[what]
    assert int(status[0]) == bit
    # only the bad segment of a batch is affected
    good_m, good_s = _dev(kat["n1025_mask"]), _dev(kat["n1025_score"])
    auc2, status2 = metrics.roc_auc(torch.stack([good_m, m]), torch.stack([good_s, s]), batched=True, return_status=True)
    assert status2.tolist() == [0, bit] and np.isnan(float(auc2[1]))
    _check_auc(float(auc2[0]), float(kat["n1025_auc"]), 1025, "good segment beside a bad one")
    # anomaly_metrics keeps working: sqerr = (recon - real)^2 = score needs real = 0, recon = sqrt(score); a bad mask value
    # or a NaN reconstruction gives AUC nan + AUC_status
    if what in ("nan", "mask2"):
        real = torch.zeros(1, 1, 25, 41, device=DEV)
        recon = s.clamp_min(0).sqrt().reshape(1, 1, 25, 41) if what == "mask2" else s.reshape(1, 1, 25, 41)
        r = metrics.anomaly_metrics(real, recon, m.reshape(1, 1, 25, 41))
        assert np.isnan(r["AUC"]) and r["AUC_status"] == bit


def test_negative_zero_counts_as_zero():
    from anoddpm_amd import metrics
    m = torch.tensor([0, 1, 1, 0], dtype=torch.float32, device=DEV)
    s = torch.tensor([0.0, -0.0, 0.0, -0.0], dtype=torch.float32, device=DEV)
    p = metrics.roc_points(m, s)[0]
    assert p["auc"] == 0.5 and p["thresholds"].view(np.uint32).tolist() == [0] and p["fps"].tolist() == [2] and p["tps"].tolist() == [2]


def test_anomaly_metrics_auc_is_the_flattened_batch(kat):
    from anoddpm_amd import metrics
    torch.manual_seed(5)
    real = torch.rand(3, 1, 64, 64, device=DEV) * 2 - 1
    recon = real + torch.randn(3, 1, 64, 64, device=DEV) * 0.3
    mask = (torch.rand(3, 1, 64, 64, device=DEV) > 0.9).float()
    recon = recon + mask * 0.4
    before = metrics.anomaly_maps(real, recon, mask)
    r = metrics.anomaly_metrics(real, recon, mask)
    assert r["AUC_status"] == 0
    flat = metrics.roc_auc(mask.reshape(-1), r["maps"]["sqerr"].reshape(-1))
    assert r["AUC"] == float(flat[0]) and 0.5 < r["AUC"] < 1.0
    want = rc.roc_numpy(mask.cpu().numpy(), before[0]["sqerr"].cpu().numpy())
    _check_auc(r["AUC"], want["auc"], real.numel(), "anomaly_metrics")
    per_image = metrics.roc_auc(mask, r["maps"]["sqerr"])               # [3]: NOT what the reference computes
    assert per_image.shape == (3,) and float(per_image.mean()) != r["AUC"]
    # the keys that existed keep their values
    c = before[1].cpu()
    assert r["mse"] == float(c[:, 9].sum()) / real.numel() and r["dice"] == float(metrics._ratios(c)["dice"])
    no_mask = metrics.anomaly_metrics(real, recon, None)
    assert np.isnan(no_mask["AUC"]) and no_mask["AUC_status"] == 0


def test_detection_records_carry_the_auc(tmp_path, monkeypatch):
    from anoddpm_amd import metrics
    GD, m, d = _tiny()
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(1)
    x_0 = torch.rand(1, 1, 32, 32, device=DEV) * 2 - 1
    mask = (torch.rand(1, 1, 32, 32, device=DEV) > 0.7).float()
    args = {"arg_num": 9, "T": 200, "img_size": [32, 32]}                # settings 50, 100, 150
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert [r["t_distance"] for r in d.last_detection] == [50, 100, 150]
    for rec in d.last_detection:
        assert rec["auc"].is_cuda and rec["auc"].dtype == torch.float64 and rec["auc"].dim() == 0
        sqerr = metrics.anomaly_maps(x_0, rec["output"], mask)[0]["sqerr"]       # rec["mse"] is sqerr * 2 - 1, not the score
        want = metrics.roc_auc(mask, sqerr)
        assert rc.bits_equal(rec["auc"].cpu().numpy().reshape(1), want.cpu().numpy())
        assert int(rec["auc_status"]) == 0 and 0.0 <= float(rec["auc"]) <= 1.0
        _check_auc(float(rec["auc"]), rc.roc_numpy(mask.cpu().numpy(), sqerr.cpu().numpy())["auc"], 1024, "detection_B")
    # an all-zero mask (what the existing detection tests pass): NaN, as sklearn gives
    d.detection_B(m, x_0, args, ("vol", "slice"), torch.zeros_like(mask), denoise_fn="gauss", total_avg=2)
    assert all(np.isnan(float(r["auc"])) and int(r["auc_status"]) == 0 for r in d.last_detection)
    # no mask: no AUC
    d.detection_B(m, x_0, args, ("vol", "slice"), None, denoise_fn="gauss", total_avg=2)
    assert all(r["auc"] is None and r["auc_status"] is None for r in d.last_detection)
    assert not os.listdir(tmp_path)
