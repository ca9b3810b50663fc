"""-m gpu: the native per-region overlap curve and AUPRO (anoddpm_component_areas of csrc/postproc.hip and anoddpm_pro_auc of
csrc/pro.hip through metrics.component_areas / aupro / pro_points / AUPRO, anomaly_metrics_pro and the detection records) against
the restatements of tests/pro_cases.py: areas and region counts equal to scipy.ndimage.label + bincount, K / N / P / fps /
thresholds equal, PRO values and AUPRO within n * 2^-50 of the exact rational value (and bit-equal to the fp64 restatement, which
adds in the kernel's order), the same bits on every launch and wherever a segment sits in a batch."""
import gc
import os

import numpy as np
import pytest
import torch

import pro_cases as pc
from conftest import GOLDEN
from score_cases import PARENT_METRIC_KEYS, PARENT_RECORD_KEYS, PP_METRIC_KEYS, PP_RECORD_KEYS, bits as _bits, host as _host, tiny as _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "pro_kat.npz"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _points(mask, score, limit, conn):
    """metrics.pro_points of a case: score [S, m, H, W], mask like it or [m, H, W]."""
    from anoddpm_amd import metrics
    return metrics.pro_points(_dev(mask), _dev(score), limit=limit, connectivity=conn, batched=True)


# ---------------------------------------------------------------------------------- component areas
def _area_masks():
    rng = np.random.default_rng(11)
    yield "noise40x33", (rng.random((3, 40, 33)) > 0.55).astype(np.float32)          # odd width, winding components, three planes
    yield "dense17x300", (rng.random((2, 17, 300)) > 0.35).astype(np.float32)         # more than one block per plane
    yield "single", np.ones((1, 1, 1), np.float32)
    for name in ("border", "pooled4", "diag_c2", "mask_all0", "mask_all1", "map256"):
        yield name, pc.make_case(name)[0]


@pytest.mark.parametrize("conn", (1, 2))
def test_component_areas_equal_scipy_label_and_bincount(conn):
    from anoddpm_amd import metrics
    for name, mask in _area_masks():
        want_area, want_counts = pc.regions(mask, conn)
        area, counts = metrics.component_areas(_dev(mask), connectivity=conn)
        assert area.dtype == torch.int32 and counts.dtype == torch.int64 and area.is_cuda and counts.is_cuda
        assert tuple(area.shape) == mask.shape and tuple(counts.shape) == mask.shape[:1]
        assert np.array_equal(_host(area), want_area), (name, conn)
        assert np.array_equal(_host(counts), want_counts), (name, conn)
    # a level other than 0 thresholds an image; a 2-D tensor is one plane
    img = np.random.default_rng(12).random((24, 24)).astype(np.float32)
    want_area, want_counts = pc.regions((img > 0.5)[None].astype(np.float32), conn)
    area, counts = metrics.component_areas(_dev(img), connectivity=conn, level=0.5)
    assert tuple(area.shape) == (24, 24) and tuple(counts.shape) == ()
    assert np.array_equal(_host(area), want_area[0]) and int(counts) == int(want_counts[0])


# ---------------------------------------------------------------------------------- the curve and its area
@pytest.mark.parametrize("name", pc.SMALL + pc.LARGE)
def test_curve_and_aupro_against_exact_and_kernel_order(kat, name):
    from anoddpm_amd import metrics
    mask, score, limit, conn = pc.make_case(name)
    if name in pc.SMALL:
        assert _bits(mask.astype(np.uint8), kat[f"{name}_mask"]) and _bits(score, kat[f"{name}_score"])
    else:
        assert pc.sha(mask, score) == str(kat[f"{name}_sha"]), f"{name}: the regenerated input differs from the fixture's"
    pts = _points(mask, score, limit, conn)
    val, status = metrics.aupro(_dev(mask), _dev(score), limit=limit, connectivity=conn, batched=True, return_status=True)
    assert val.dtype == torch.float64 and val.is_cuda and tuple(val.shape) == (score.shape[0],) and not _host(status).any()
    for s, p in enumerate(pts):
        m = pc.segment_mask(mask, score, s)
        exact = pc.pro_exact(m, score[s], limit, conn)
        assert pc.sha(exact["fps"], exact["thresholds"], exact["pro"]) == str(kat[f"{name}_curve_sha"][s])      # what the fixture froze
        assert _bits(np.float64(exact["aupro"]), kat[f"{name}_aupro"][s])
        pc.check_against_exact(p, exact, f"{name}[{s}]")
        order = pc.pro_fp64(m, score[s], limit, conn)
        assert _bits(p["pro"], order["pro"]), (name, s)                                 # the same additions in the same order
        assert _bits(np.float64(p["aupro"]), np.float64(order["aupro"])), (name, s, p["aupro"], order["aupro"])
        assert _bits(_host(val)[s], np.float64(p["aupro"])), (name, s)                  # aupro() is pro_points()' value
    if name == "perfect":
        assert pts[0]["aupro"] == 1.0
    if name == "first_beyond":
        assert abs(pts[0]["aupro"] - 0.35) <= pc.tolerance(64) and pts[0]["fps"][0] == 24 and pts[0]["pro"][0] == 1.0
    if name in ("mask_all0", "mask_all1"):
        assert np.isnan(pts[0]["aupro"]) and np.isnan(_host(val)[0])
        assert (pts[0]["K"] == 0) if name == "mask_all0" else (pts[0]["N"] == 0 and pts[0]["K"] == 1)


def test_chunk_with_a_ragged_second_scatter_group_keeps_the_payload_order():
    mask, score, limit, conn = pc.make_case(pc.RAGGED)
    p = _points(mask, score, limit, conn)[0]
    pc.check_against_exact(p, pc.pro_exact(mask, score[0], limit, conn), pc.RAGGED)
    order = pc.pro_fp64(mask, score[0], limit, conn)
    assert _bits(p["pro"], order["pro"])
    assert _bits(np.float64(p["aupro"]), np.float64(order["aupro"])), (p["aupro"], order["aupro"])


def test_AUPRO_is_a_python_float_of_the_pooled_curve():
    from anoddpm_amd import metrics
    mask, score, limit, conn = pc.make_case("pooled4")
    want = _points(mask, score, limit, conn)[0]["aupro"]
    got = metrics.AUPRO(_dev(mask).reshape(4, 1, 16, 24), _dev(score).reshape(4, 1, 16, 24))
    assert isinstance(got, float) and _bits(np.float64(got), np.float64(want))
    mask, score, limit, conn = pc.make_case("limit1")
    assert _bits(np.float64(metrics.AUPRO(_dev(mask[0]), _dev(score[0, 0]), limit=1.0)), np.float64(_points(mask, score, 1.0, conn)[0]["aupro"]))


# ---------------------------------------------------------------------------------- determinism
def test_same_bits_on_every_launch_and_wherever_the_segment_sits():
    from anoddpm_amd import metrics
    names = ("plane32", "odd40x33", "map256")
    for name in names:
        mask, score, limit, conn = pc.make_case(name)
        alone = _points(mask, score, limit, conn)[0]
        again = _points(mask, score, limit, conn)[0]
        assert all(_bits(np.asarray(alone[k]), np.asarray(again[k])) for k in alone), name
        # as segment 2 of 3, with its own mask and with other maps around it
        rng = np.random.default_rng(3)
        others = [(rng.random(score.shape[1:]) ** 2).astype(np.float32) for _ in range(2)]
        batch = np.stack([others[0], score[0], others[1]])
        masks = np.stack([np.roll(mask, 3, axis=-1), mask, np.zeros_like(mask)])
        mid = _points(masks, batch, limit, conn)[1]
        assert all(_bits(np.asarray(alone[k]), np.asarray(mid[k])) for k in alone), name
        shared = _points(mask, batch, limit, conn)[1]
        assert all(_bits(np.asarray(alone[k]), np.asarray(shared[k])) for k in alone), name
        a1 = metrics.aupro(_dev(mask), _dev(batch), limit=limit, batched=True)
        assert _bits(_host(a1)[1], np.float64(alone["aupro"]))


# ---------------------------------------------------------------------------------- NaN and status
def test_status_bits_stay_on_their_own_segment():
    from anoddpm_amd import _lib, metrics
    mask, score = pc.status_batch()
    val, status = metrics.aupro(_dev(mask), _dev(score), batched=True, return_status=True)
    assert _host(status).tolist() == [_lib.ROC_NAN, _lib.ROC_NEGATIVE, _lib.ROC_BAD_MASK]
    assert np.isnan(_host(val)).all()
    with pytest.raises(ValueError, match="segment 0: NaN score"):
        metrics.pro_points(_dev(mask), _dev(score), batched=True)
    with pytest.raises(ValueError, match="negative score"):
        metrics.AUPRO(_dev(mask[1]), _dev(score[1]))
    with pytest.raises(ValueError, match="mask value other than 0 and 1"):
        metrics.AUPRO(_dev(mask[2]), _dev(score[2]))
    # each violation mended in turn: that segment alone changes, and it equals the restatement
    clean_mask, clean_score = mask.copy(), score.copy()
    clean_score[0, 0, 3, 4], clean_score[1, 0, 7, 1], clean_mask[2, 0, 2, 2] = 0.5, 0.5, 1.0
    val, status = metrics.aupro(_dev(clean_mask), _dev(clean_score), batched=True, return_status=True)
    assert not _host(status).any()
    for s in range(3):
        exact = pc.pro_exact(clean_mask[s], clean_score[s], 0.3, 2)
        assert abs(_host(val)[s] - exact["aupro"]) <= pc.tolerance(256) - 2.0 ** -53
    mixed = score.copy()
    mixed[0], mixed[1] = clean_score[0], clean_score[1]
    v2, s2 = metrics.aupro(_dev(mask), _dev(mixed), batched=True, return_status=True)
    assert _host(s2).tolist() == [0, 0, _lib.ROC_BAD_MASK] and _bits(_host(v2)[:2], _host(val)[:2]) and np.isnan(_host(v2)[2])
    # an infinite score
    inf = clean_score.copy()
    inf[1, 0, 0, 0] = np.inf
    assert _host(metrics.aupro(_dev(clean_mask), _dev(inf), batched=True, return_status=True)[1]).tolist() == [0, _lib.ROC_INF, 0]


def test_truncated_curve_keeps_its_first_points():
    import ctypes
    from anoddpm_amd import _lib, metrics
    mask, score, limit, conn = pc.make_case("plane16")
    full = _points(mask, score, limit, conn)[0]
    areas, regions = metrics.component_areas(_dev(mask), connectivity=conn)
    sc = _dev(score).reshape(-1)
    cap = 10
    L = _lib.lib()
    nbytes = L.anoddpm_pro_workspace_bytes(1, 256)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    out = {"aupro": torch.empty(1, dtype=torch.float64, device=DEV), "counts": torch.empty(4, dtype=torch.int64, device=DEV),
           "status": torch.empty(1, dtype=torch.int32, device=DEV), "fps": torch.full((cap + 2,), -7, dtype=torch.int32, device=DEV),
           "pro": torch.full((cap + 2,), -7.0, dtype=torch.float64, device=DEV), "thr": torch.full((cap + 2,), -7.0, device=DEV),
           "len": torch.empty(1, dtype=torch.int32, device=DEV)}
    a = _lib.ProArgs()
    a.score, a.area, a.region_counts, a.workspace, a.workspace_bytes = sc.data_ptr(), areas.data_ptr(), regions.data_ptr(), ws.data_ptr(), nbytes
    a.aupro, a.counts, a.status = out["aupro"].data_ptr(), out["counts"].data_ptr(), out["status"].data_ptr()
    a.curve_fps, a.curve_pro, a.curve_thr, a.curve_len = out["fps"].data_ptr(), out["pro"].data_ptr(), out["thr"].data_ptr(), out["len"].data_ptr()
    a.curve_cap, a.limit, a.S, a.planes_per_segment, a.H, a.W = cap, limit, 1, 1, 16, 16
    _lib.check(L.anoddpm_pro_auc(ctypes.byref(a), _lib.current_stream()), "pro_auc")
    torch.cuda.synchronize()
    assert int(out["status"][0]) == _lib.ROC_CURVE_TRUNCATED and int(out["len"][0]) == full["fps"].size
    assert np.array_equal(_host(out["fps"])[:cap], full["fps"][:cap]) and _bits(_host(out["pro"])[:cap], full["pro"][:cap])
    assert (_host(out["fps"])[cap:] == -7).all() and (_host(out["pro"])[cap:] == -7).all() and (_host(out["thr"])[cap:] == -7).all()
    assert _bits(np.float64(_host(out["aupro"])[0]), np.float64(full["aupro"]))          # the area does not depend on the buffer
    assert _host(out["counts"]).tolist() == [full["K"], full["N"], full["P"], full["fps"].size]


# ---------------------------------------------------------------------------------- graph capture
def test_both_entry_points_replay_from_a_captured_graph():
    from anoddpm_amd import metrics
    mask, score, limit, conn = pc.make_case("shared3")
    other = (np.random.default_rng(8).random(score.shape) ** 2).astype(np.float32)
    m, x = _dev(mask), _dev(score).clone()

    def run():
        areas, counts = metrics.component_areas(m, connectivity=conn)
        return areas, counts, metrics.aupro(m, x, limit=limit, connectivity=conn, batched=True)

    eager = [_host(t) for t in run()]
    x.copy_(_dev(other))
    eager_other = [_host(t) for t in run()]
    x.copy_(_dev(score))
    assert not _bits(eager[2], eager_other[2])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()                                                        # no collection of older graphs inside the capture
    try:
        with torch.cuda.graph(g):
            captured = run()
    finally:
        if was_enabled:
            gc.enable()
    g.replay()
    torch.cuda.synchronize()
    assert all(_bits(_host(t), e) for t, e in zip(captured, eager))
    x.copy_(_dev(other))                                                # new contents in the captured input, replayed
    g.replay()
    torch.cuda.synchronize()
    assert all(_bits(_host(t), e) for t, e in zip(captured, eager_other))


# ---------------------------------------------------------------------------------- anomaly_metrics
def _scene():
    """real / recon / mask [2, 1, 48, 40]: two lesions of very different size in image 0, one in image 1, speckle everywhere."""
    rng = np.random.default_rng(21)
    real = (rng.random((2, 1, 48, 40)) * 1.6 - 0.8).astype(np.float32)
    mask = np.zeros_like(real)
    mask[0, 0, 5:25, 4:22] = 1
    mask[0, 0, 40:42, 30:33] = 1
    mask[1, 0, 20:28, 10:18] = 1
    recon = real + (rng.random(real.shape).astype(np.float32) - 0.5) * 0.6 + mask * rng.random(real.shape).astype(np.float32) * 0.9
    return _dev(real), _dev(recon.astype(np.float32)), _dev(mask)


def test_anomaly_metrics_pro_adds_keys_and_nothing_else():
    from anoddpm_amd import metrics
    real, recon, mask = _scene()
    plain = metrics.anomaly_metrics(real, recon, mask)
    assert set(plain) == PARENT_METRIC_KEYS
    none = metrics.anomaly_metrics_pro(real, recon, mask, pro_limit=None)
    assert set(none) == PARENT_METRIC_KEYS and all(_bits(np.float64(none[k]), np.float64(plain[k])) for k in PARENT_METRIC_KEYS - {"maps"})
    r = metrics.anomaly_metrics_pro(real, recon, mask)
    assert set(r) == PARENT_METRIC_KEYS | {"AUPRO", "AUPRO_regions", "AUPRO_status"}
    for k in PARENT_METRIC_KEYS - {"maps"}:
        assert _bits(np.float64(r[k]), np.float64(plain[k])), k
    sq = r["maps"]["sqerr"]
    assert _bits(np.float64(r["AUPRO"]), np.float64(metrics.AUPRO(mask, sq))) and isinstance(r["AUPRO"], float)
    exact = pc.pro_exact(_host(mask).reshape(2, 48, 40), _host(sq).reshape(2, 48, 40), 0.3, 2)
    assert (r["AUPRO_regions"], r["AUPRO_status"]) == (3, 0) == (exact["K"], 0)
    assert abs(r["AUPRO"] - exact["aupro"]) <= pc.tolerance(sq.numel()) - 2.0 ** -53
    # another limit, and the filtered map beside the raw one
    pp = metrics.PostProcess(median=3, erode=0, min_size=2)
    with_pp = metrics.anomaly_metrics(real, recon, mask, postprocess=pp)
    assert set(with_pp) == PARENT_METRIC_KEYS | PP_METRIC_KEYS
    assert set(metrics.anomaly_metrics_pro(real, recon, mask, postprocess=pp, pro_limit=None)) == PARENT_METRIC_KEYS | PP_METRIC_KEYS
    r = metrics.anomaly_metrics_pro(real, recon, mask, postprocess=pp, pro_limit=0.1)
    assert set(r) == PARENT_METRIC_KEYS | PP_METRIC_KEYS | {"AUPRO", "AUPRO_pp", "AUPRO_regions", "AUPRO_status"}
    assert _bits(np.float64(r["AUPRO"]), np.float64(metrics.AUPRO(mask, r["maps"]["sqerr"], limit=0.1)))
    assert _bits(np.float64(r["AUPRO_pp"]), np.float64(metrics.AUPRO(mask, r["maps"]["sqerr_pp"], limit=0.1)))
    assert r["AUPRO_pp"] != r["AUPRO"]
    # no mask: no curve; no region: NaN
    r = metrics.anomaly_metrics_pro(real, recon, None, pro_limit=0.3)
    assert np.isnan(r["AUPRO"]) and (r["AUPRO_regions"], r["AUPRO_status"]) == (0, 0)
    r = metrics.anomaly_metrics_pro(real, recon, torch.zeros_like(mask), pro_limit=0.3)
    assert np.isnan(r["AUPRO"]) and (r["AUPRO_regions"], r["AUPRO_status"]) == (0, 0)


# ---------------------------------------------------------------------------------- detection records
def test_detection_records_carry_aupro_when_asked(tmp_path, monkeypatch):
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

    assert d.pro_limit is None
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    plain = d.last_detection
    assert [r["t_distance"] for r in plain] == [50, 100, 150] and all(set(r) == PARENT_RECORD_KEYS for r in plain)

    calls = []
    L = _lib.lib()
    for name in ("anoddpm_component_areas", "anoddpm_pro_auc"):
        fn = getattr(L, name)
        monkeypatch.setattr(L, name, lambda *a, _fn=fn, _name=name: (calls.append(_name), _fn(*a))[1])
    d.pro_limit = 0.3
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert calls == ["anoddpm_component_areas", "anoddpm_pro_auc"]        # one of each for the whole sweep
    recs = d.last_detection
    for rec, old in zip(recs, plain):
        assert set(rec) == PARENT_RECORD_KEYS | {"aupro"}
        for k in ("mean", "mse", "threshold", "counts", "auc", "ap", "best_dice", "best_threshold", "ssim", "output"):
            assert _bits(_host(rec[k]), _host(old[k])), k                 # the same chains, the same raw results
        sq = metrics.anomaly_maps(x_0, rec["output"], mask)[0]["sqerr"]
        assert rec["aupro"].is_cuda and rec["aupro"].dtype == torch.float64 and rec["aupro"].shape == ()
        assert _bits(_host(rec["aupro"]), _host(metrics.aupro(mask, sq, batched=False)[0]))
        print(rec["t_distance"], float(rec["auc"]), float(rec["aupro"]))

    # with post-processing: aupro_pp on the filtered map, still one launch of each
    del calls[:]
    d.postprocess = metrics.PostProcess(median=3, erode=0)
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert calls == ["anoddpm_component_areas", "anoddpm_pro_auc"]
    for rec, old in zip(d.last_detection, recs):
        assert set(rec) == PARENT_RECORD_KEYS | PP_RECORD_KEYS | {"aupro", "aupro_pp"}
        assert _bits(_host(rec["aupro"]), _host(old["aupro"]))
        assert _bits(_host(rec["aupro_pp"]), _host(metrics.aupro(mask, rec["sqerr_pp"], batched=False)[0]))

    # without a mask the keys are there and empty; unset again: the parent's keys again
    d.postprocess = None
    d.detection_B(m, x_0, args, ("vol", "slice"), None, denoise_fn="gauss", total_avg=2)
    assert all(set(r) == PARENT_RECORD_KEYS | {"aupro"} and r["aupro"] is None for r in d.last_detection)
    d.pro_limit = None
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert all(set(r) == PARENT_RECORD_KEYS for r in d.last_detection)
    assert not os.listdir(tmp_path)
