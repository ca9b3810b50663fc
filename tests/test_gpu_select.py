"""-m gpu: order statistics of pooled segments and counts at device thresholds (csrc/select_wide.hip through its C ABI and through
metrics.order_stats / HealthyPool / counts_at / scores_at / anomaly_metrics_at and the detection records) against the numpy
restatements of tests/select_cases.py and against anoddpm_map_scores.  Values, counts, maxima, status words and the sums in the
kernel's order are compared by `tobytes()` equality, no tolerance; the means also against math.fsum within n * 2^-52 / k * 2^-52."""
import ctypes
import math

import numpy as np
import pytest
import torch

import select_cases as sc
import smooth_cases as sm
from score_cases import PARENT_RECORD_KEYS, bits as _bits, bits_any_nan, host as _host, tiny as _tiny

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SELECT_CASES = sorted(sc.SELECT)
COUNT_CASES = sorted(sc.COUNTS)
AT_RECORD_KEYS = {"dice_at", "precision_at", "recall_at", "fpr_at"}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def select_abi(buf, n, ranks, tile, S=1, stride=None, host_ranks=True):
    """anoddpm_select_wide on the device tensor `buf` ([S][stride] fp32), every output poisoned first (NaN / -1) and allocated with
    one guard row behind it.  -> (rc, dict of host arrays with the guard row, Q)"""
    from anoddpm_amd import _lib
    L = _lib.lib()
    Q = len(ranks)
    table = torch.tensor([r if r < (1 << 31) else r - (1 << 32) for r in ranks], dtype=torch.int32, device=DEV)
    host = (ctypes.c_uint32 * Q)(*ranks)
    nbytes = L.anoddpm_select_wide_workspace_bytes(n, Q, tile)
    assert nbytes > 0
    ws = torch.empty((nbytes // 4,), dtype=torch.int32, device=DEV)
    out = {"value": torch.full((S + 1, Q), float("nan"), dtype=torch.float32, device=DEV), "above": torch.full((S + 1, Q), -1, dtype=torch.int64, device=DEV),
           "equal": torch.full((S + 1, Q), -1, dtype=torch.int64, device=DEV), "topk": torch.full((S + 1, Q), float("nan"), dtype=torch.float64, device=DEV),
           "max": torch.full((S + 1,), float("nan"), dtype=torch.float32, device=DEV), "mean": torch.full((S + 1,), float("nan"), dtype=torch.float64, device=DEV),
           "status": torch.full((S + 1,), -1, dtype=torch.int32, device=DEV)}
    a = _lib.SelectArgs()
    a.src, a.ranks, a.ranks_host = buf.data_ptr(), table.data_ptr(), (ctypes.addressof(host) if host_ranks else None)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.value, a.above, a.equal, a.topk_mean = out["value"].data_ptr(), out["above"].data_ptr(), out["equal"].data_ptr(), out["topk"].data_ptr()
    a.max, a.mean, a.status = out["max"].data_ptr(), out["mean"].data_ptr(), out["status"].data_ptr()
    a.src_stride, a.n, a.S, a.Q = (n if stride is None else stride), n, S, Q
    rc = L.anoddpm_select_wide(ctypes.byref(a), tile, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, {k: _host(v) for k, v in out.items()}, Q


def guards_intact(o, S):
    return (np.isnan(o["value"][S]).all() and (o["above"][S] == -1).all() and (o["equal"][S] == -1).all() and np.isnan(o["topk"][S]).all()
            and np.isnan(o["max"][S]) and np.isnan(o["mean"][S]) and o["status"][S] == -1)


def map_scores_abi(buf, n, k):
    from anoddpm_amd import _lib
    out = {"max": torch.empty((1,), dtype=torch.float32, device=DEV), "mean": torch.empty((1,), dtype=torch.float64, device=DEV),
           "topk": torch.empty((1,), dtype=torch.float64, device=DEV), "status": torch.empty((1,), dtype=torch.int32, device=DEV)}
    a = _lib.MapScoresArgs()
    a.src, a.max, a.mean, a.topk_mean, a.status = buf.data_ptr(), out["max"].data_ptr(), out["mean"].data_ptr(), out["topk"].data_ptr(), out["status"].data_ptr()
    a.src_stride, a.n, a.k, a.S = n, n, k, 1
    assert _lib.lib().anoddpm_map_scores(ctypes.byref(a), _lib.current_stream()) == 0
    torch.cuda.synchronize()
    return {k_: _host(v) for k_, v in out.items()}


def check_against(o, s, want, n, ranks):
    """Segment s of a select_abi result against a select_numpy result."""
    assert int(o["status"][s]) == want["status"]
    for k in ("value", "above", "equal"):
        assert _bits(o[k][s], want[k]), (k, o[k][s], want[k])
    assert _bits(o["max"][s], np.float32(want["max"])) or (np.isnan(o["max"][s]) and np.isnan(want["max"]))
    for q, r in enumerate(ranks):
        assert int(o["above"][s, q]) <= r < int(o["above"][s, q]) + int(o["equal"][s, q])
    if want["status"] == 0:
        print("mean", o["mean"][s], want["mean"], "topk", o["topk"][s].tolist(), want["topk"].tolist())
        assert _bits(o["mean"][s], np.float64(want["mean"])) and _bits(o["topk"][s], want["topk"])


# ---------------------------------------------------------------------------------- the select
@pytest.fixture(scope="module")
def restated():
    """name -> select_numpy of the case: computed once, shared, never written to."""
    return {name: sc.select_numpy(*sc.make_select_case(name)) for name in SELECT_CASES}


@pytest.mark.parametrize("name", SELECT_CASES)
def test_select_matches_the_restatement(restated, name):
    from anoddpm_amd import metrics
    x, ranks, tile = sc.make_select_case(name)
    n, want = x.size, restated[name]
    d = _dev(x)
    rc, o, Q = select_abi(d, n, ranks, tile)
    assert rc == 0 and guards_intact(o, 1)
    check_against(o, 0, want, n, ranks)
    if want["status"] == 0:
        v = np.sort(np.abs(x).astype(np.float64))[::-1]
        assert sm.within(float(o["mean"][0]), math.fsum(v) / n, n)
        for q, r in enumerate(ranks):
            assert sm.within(float(o["topk"][0, q]), math.fsum(v[:r + 1]) / (r + 1), r + 1)
    rc2, o2, _ = select_abi(d, n, ranks, tile)                                         # two runs
    assert rc2 == 0 and all(o[k].tobytes() == o2[k].tobytes() for k in o)
    got, status = metrics.order_stats(d, list(ranks), tile=tile or None, return_status=True)
    assert int(status[0]) == want["status"] and got["value"].shape == (1, Q) and got["max"].shape == (1,) and got["above"].dtype == torch.int64
    assert _bits(_host(got["above"])[0], want["above"]) and _bits(_host(got["equal"])[0], want["equal"])
    if want["status"] == 0:
        for k in ("value", "topk", "max", "mean"):
            assert _bits(_host(got[k])[0], np.asarray(want[k]))
    else:
        assert all(np.isnan(_host(got[k])).all() for k in ("value", "topk", "max", "mean"))
    assert _bits(_host(d), x)


@pytest.mark.parametrize("name", SELECT_CASES)
def test_select_of_one_rank_has_the_bits_of_map_scores(name):
    x, ranks, tile = sc.make_select_case(name)
    d = _dev(x)
    for r in sorted(set(ranks)):
        rc, o, _ = select_abi(d, x.size, (r,), tile)
        ms = map_scores_abi(d, x.size, r + 1)
        assert rc == 0
        assert int(o["status"][0]) == int(ms["status"][0])
        assert bits_any_nan(o["max"][:1], ms["max"]) and bits_any_nan(o["mean"][:1], ms["mean"]) and bits_any_nan(o["topk"][0], ms["topk"]), (r, o, ms)


def test_select_beyond_the_limit_of_map_scores():
    from anoddpm_amd import _lib
    x, ranks, tile = sc.make_big()
    n = x.size
    assert n == (1 << 24) + 4097 > _lib.MAP_SCORES_MAX_N and ranks == (0, 167772, n - 1) and tile == 0
    want = sc.select_numpy(x, ranks, tile)
    d = _dev(x)
    rc, o, _ = select_abi(d, n, ranks, tile)
    assert rc == 0 and guards_intact(o, 1)
    check_against(o, 0, want, n, ranks)


def test_select_of_strided_segments_leaves_its_neighbours_alone():
    buf, ranks, tile, n = sc.make_strided()
    S, stride = buf.shape
    d = _dev(buf)
    rc, o, _ = select_abi(d, n, ranks, tile, S=S, stride=stride)
    assert rc == 0 and guards_intact(o, S)
    for s in range(S):
        want = sc.select_numpy(buf[s, :n], ranks, tile)
        assert want["status"] == (sc.INF_BIT if s == 1 else 0)
        check_against(o, s, want, n, ranks)
    assert _bits(_host(d), buf)                                                        # the input, gaps included, is untouched


def test_a_device_rank_past_the_end_sets_the_status_bit():
    from anoddpm_amd import metrics
    x, _, tile = sc.make_select_case("n257")
    n = x.size
    d = _dev(x)
    rc, o, _ = select_abi(d, n, (0, n, 5, 0xffffffff), tile, host_ranks=False)
    want = sc.select_numpy(x, (0, 5), tile)
    assert rc == 0 and guards_intact(o, 1) and int(o["status"][0]) == sc.BAD_RANK_BIT
    assert _bits(o["value"][0, [0, 2]], want["value"]) and _bits(o["topk"][0, [0, 2]], want["topk"]) and _bits(o["above"][0, [0, 2]], want["above"])
    rc, _, _ = select_abi(d, n, (0, n), tile, host_ranks=True)                          # the same table, checked on the host: refused
    assert rc != 0
    got, status = metrics.order_stats(d, torch.tensor([0, n], device=DEV), return_status=True)
    assert int(status[0]) == sc.BAD_RANK_BIT and np.isnan(_host(got["value"])).all()
    for bad in ([n], [-1], [0.5], [], list(range(17))):
        with pytest.raises(ValueError):
            metrics.order_stats(d, bad)


# ---------------------------------------------------------------------------------- counts at thresholds
def counts_abi(mask, score, thr):
    from anoddpm_amd import _lib
    S, n = score.shape
    T = thr.shape[-1]
    dm, ds, dt = _dev(mask), _dev(score), _dev(thr)
    counts = torch.full((S + 1, T, 2), -1, dtype=torch.int64, device=DEV)
    totals = torch.full((S + 1, 2), -1, dtype=torch.int64, device=DEV)
    status = torch.full((S + 1,), -1, dtype=torch.int32, device=DEV)
    a = _lib.ThresholdCountsArgs()
    a.score, a.mask, a.thr, a.counts, a.totals, a.status = ds.data_ptr(), dm.data_ptr(), dt.data_ptr(), counts.data_ptr(), totals.data_ptr(), status.data_ptr()
    a.n, a.score_stride, a.mask_stride, a.thr_stride, a.S, a.T = n, n, (n if mask.ndim == 2 else 0), (T if thr.ndim == 2 else 0), S, T
    rc = _lib.lib().anoddpm_threshold_counts(ctypes.byref(a), _lib.current_stream())
    torch.cuda.synchronize()
    c, t, st = _host(counts), _host(totals), _host(status)
    assert (c[S] == -1).all() and (t[S] == -1).all() and st[S] == -1                   # the guard rows
    return rc, {"tp": c[:S, :, 0], "fp": c[:S, :, 1], "P": t[:S, 0], "N": t[:S, 1], "status": st[:S]}


@pytest.mark.parametrize("name", COUNT_CASES)
def test_threshold_counts_equal_the_restatement(name):
    from anoddpm_amd import metrics
    mask, score, thr = sc.make_count_case(name)
    want = sc.counts_numpy(mask, score, thr)
    rc, got = counts_abi(mask, score, thr)
    assert rc == 0 and sc.same_counts(got, want), (got, want)
    o = metrics.scores_at(_dev(mask), _dev(score), _dev(thr), batched=True)
    assert sc.same_counts({k: _host(o[k]) for k in ("tp", "fp", "P", "N", "status")}, want)
    tp, fp, P, N = (want[k].astype(np.float64) for k in ("tp", "fp", "P", "N"))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratios = {"dice": np.where(P[:, None] == 0, np.nan, 2 * tp / (tp + fp + P[:, None])), "precision": np.where(tp + fp == 0, np.nan, tp / (tp + fp)),
                  "recall": np.where(P[:, None] == 0, np.nan, tp / P[:, None]), "fpr": np.where(N[:, None] == 0, np.nan, fp / N[:, None])}
    for k, v in ratios.items():
        v = np.where(want["status"][:, None] != 0, np.nan, v)
        assert o[k].dtype == torch.float64 and o[k].is_cuda and bits_any_nan(_host(o[k]), v), k


def test_dice_at_a_threshold_never_exceeds_best_dice():
    from anoddpm_amd import metrics
    rng = np.random.default_rng(9980)
    S, n = 3, 3001
    score = sm._errors(rng, (S, n))
    mask = ((score > 0.4) ^ (rng.random((S, n)) < 0.1)).astype(np.float32)             # a mask the score predicts, with 10 % flips
    thr = np.sort(sm._errors(rng, (16,)))
    dm, ds = _dev(mask), _dev(score)
    best = metrics.best_dice(dm, ds, batched=True)
    at = metrics.scores_at(dm, ds, _dev(thr), batched=True)
    d, b = _host(at["dice"]), _host(best["dice"])
    print(d.max(axis=1), b)
    assert np.isfinite(d).all() and (d <= b[:, None]).all()
    assert (_host(best["threshold"]) > 0).all()
    below = torch.nextafter(best["threshold"], torch.zeros_like(best["threshold"]))[:, None]      # score >= t  <=>  score > the value below t
    o = metrics.counts_at(dm, ds, below, batched=True)
    assert _bits(_host(o["tp"])[:, 0], _host(best["tp"])) and _bits(_host(o["fp"])[:, 0], _host(best["fp"]))
    assert _bits(_host(metrics.scores_at(dm, ds, below, batched=True)["dice"])[:, 0], b)


# ---------------------------------------------------------------------------------- the pool
def test_healthy_pool_collects_and_calibrates():
    from anoddpm_amd import metrics
    rng = np.random.default_rng(9981)
    parts = [sm._errors(rng, shape) for shape in ((2, 1, 32, 32), (40, 50), (777,))]
    flat = np.concatenate([p.reshape(-1) for p in parts])
    n = flat.size
    pool = metrics.HealthyPool(n)
    assert len(pool) == 0 and pool.capacity == n
    with pytest.raises(ValueError, match="empty"):
        pool.order_stats([0])
    for p in parts:
        pool.add(_dev(p))
    assert len(pool) == n
    with pytest.raises(ValueError, match="exceed"):
        pool.add(_dev(parts[2][:1]))
    one = metrics.HealthyPool(n + 5)
    one.add(_dev(flat))
    ranks = [0, 3, n // 100, n - 1]
    a, b = pool.order_stats(ranks), one.order_stats(ranks)
    assert all(_bits(_host(a[k]), _host(b[k])) for k in a)
    rates = [0, 0.001, 0.05]
    thr = pool.thresholds(rates)
    assert thr.shape == (3,) and thr.dtype == torch.float32 and thr.is_cuda
    want = np.array([sc.threshold_numpy(flat, f) for f in rates], np.float32)
    assert _bits(_host(thr), want) and want[0] == flat.max()
    for t, f in zip(want, rates):
        assert int((flat > t).sum()) <= sc.rank_of(f, n)
    assert _bits(_host(pool.thresholds(0.05)), want[2:])
    for bad in (1.0, [0.5, 1.0], -0.1, 1.5, "0.1"):
        with pytest.raises(ValueError):
            pool.thresholds(bad)
    roi = rng.random(n) < 0.6                                                          # maps zeroed outside a region of interest
    pool.reset()
    assert len(pool) == 0
    pool.add(_dev(np.where(roi, flat, np.float32(0))))
    inside = np.array([sc.threshold_numpy(flat[roi], f) for f in (0.001, 0.05)], np.float32)
    assert _bits(_host(pool.thresholds([0.001, 0.05], negatives=int(roi.sum()))), inside)


def test_order_stats_and_counts_at_replay_from_a_graph():
    from anoddpm_amd import metrics
    rng = np.random.default_rng(9982)
    n = 70001
    score, mask = sm._errors(rng, (n,)), (rng.random(n) < 0.1).astype(np.float32)
    pool = metrics.HealthyPool(n)
    pool.add(_dev(score))
    dm, ds = _dev(mask), _dev(score)
    ranks = torch.tensor([0, 70, 3500], dtype=torch.int32, device=DEV)

    def run():
        st = pool.order_stats(ranks)
        return st, metrics.counts_at(dm, ds, st["value"][0], batched=False)

    eager = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for e, c in zip(eager, captured):
        assert all(_bits(_host(e[k]), _host(c[k])) for k in e)
    want = sc.select_numpy(score, (0, 70, 3500))
    assert _bits(_host(captured[0]["value"])[0], want["value"])
    cn = sc.counts_numpy(mask, score[None], want["value"])
    assert _bits(_host(captured[1]["tp"]), cn["tp"]) and _bits(_host(captured[1]["fp"]), cn["fp"])


# ---------------------------------------------------------------------------------- anomaly_metrics_at and the detection records
@pytest.mark.parametrize("pp", [False, True])
def test_anomaly_metrics_at_equals_scores_at_on_the_returned_maps(pp):
    from anoddpm_amd import metrics
    g = torch.Generator().manual_seed(11)
    real = (torch.rand(2, 1, 32, 32, generator=g) * 2 - 1).to(DEV)
    recon = (torch.rand(3, 2, 1, 32, 32, generator=g) * 2 - 1).to(DEV)
    mask = (torch.rand(2, 1, 32, 32, generator=g) > 0.7).float().to(DEV)
    thr = torch.tensor([0.5, 0.1, 1.2], device=DEV)
    post = metrics.PostProcess(median=3, erode=0, min_size=0) if pp else None
    plain = metrics.anomaly_metrics(real, recon, mask, postprocess=post)
    r = metrics.anomaly_metrics_at(real, recon, mask, thr, postprocess=post)
    new = {k + "_at" + sfx for k in ("dice", "precision", "recall", "fpr", "tp", "fp") for sfx in (("", "_pp") if pp else ("",))}
    assert set(r) == set(plain) | new
    for k in plain:
        if k != "maps":
            assert plain[k] == r[k] or (plain[k] != plain[k] and r[k] != r[k]), k
    for sfx in ("", "_pp") if pp else ("",):
        o = metrics.scores_at(mask.reshape(1, -1), r["maps"]["sqerr" + sfx].reshape(1, -1), thr, batched=True)
        for k in ("dice", "precision", "recall", "fpr", "tp", "fp"):
            got = r[k + "_at" + sfx]
            assert got.shape == (3,) and got.is_cuda and bits_any_nan(_host(got), _host(o[k])[0]), k
    pred = r["maps"]["pred"]                                                           # sqerr > 0.5, what `dice` is counted on
    assert int(r["tp_at"][0]) == int((pred * mask).sum()) and int(r["fp_at"][0]) == int((pred * (1 - mask)).sum())
    assert _bits(_host(r["maps"]["pred"]), _host((r["maps"]["sqerr"] > 0.5).float()))


def test_detection_records_carry_the_scores_at_the_operating_thresholds(tmp_path, monkeypatch):
    from anoddpm_amd import metrics
    GD, m, d = _tiny(32)
    monkeypatch.chdir(tmp_path)
    g = torch.Generator().manual_seed(5)
    x_0 = (torch.rand(1, 1, 32, 32, generator=g) * 2 - 1).to(DEV)
    mask = (torch.rand(1, 1, 32, 32, generator=g) > 0.7).float().to(DEV)
    args = {"arg_num": 9, "T": 200, "img_size": [32, 32]}                # settings 50, 100, 150

    assert d.operating_thresholds is None and "operating_thresholds" not in d.__dict__
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    plain = d.last_detection
    assert [r["t_distance"] for r in plain] == [50, 100, 150] and all(set(r) == PARENT_RECORD_KEYS for r in plain)

    d.operating_thresholds = torch.tensor([0.5, 0.05], device=DEV)
    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    for rec, old in zip(d.last_detection, plain):
        assert set(rec) == PARENT_RECORD_KEYS | AT_RECORD_KEYS
        for k in ("mean", "mse", "threshold", "counts", "auc", "ap", "best_dice", "best_threshold", "ssim", "output"):
            assert _bits(_host(rec[k]), _host(old[k])), k                 # the same chains, the same raw results
        sq = metrics.anomaly_maps(x_0, rec["output"], mask)[0]["sqerr"]
        o = metrics.scores_at(mask.reshape(1, -1), sq.reshape(1, -1), d.operating_thresholds, batched=True)
        for k in ("dice", "precision", "recall", "fpr"):
            got = rec[k + "_at"]
            assert got.shape == (2,) and got.is_cuda and got.dtype == torch.float64 and bits_any_nan(_host(got), _host(o[k])[0]), k
        assert float(rec["dice_at"][0]) <= float(rec["best_dice"]) and float(rec["dice_at"][1]) <= float(rec["best_dice"])

    torch.manual_seed(1)
    d.detection_B(m, x_0, args, ("vol", "slice"), None, denoise_fn="gauss", total_avg=2)            # no mask: every pixel is a negative
    for rec in d.last_detection:
        assert AT_RECORD_KEYS <= set(rec) and np.isnan(_host(rec["dice_at"])).all() and np.isfinite(_host(rec["fpr_at"])).all()
