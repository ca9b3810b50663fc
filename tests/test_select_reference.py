"""-m "not gpu": the numpy restatements of tests/select_cases.py -- what the device tests compare csrc/select_wide.hip with --
against `numpy.sort`, exact arithmetic and `smooth_cases.scores_numpy`; the calibration rule; the planted defects; the header,
the binding and the host-side argument checks of both entry points."""
import ctypes
import math

import numpy as np
import pytest

import select_cases as sc
import smooth_cases as sm

SELECT_CASES = sorted(sc.SELECT)
COUNT_CASES = sorted(sc.COUNTS)


@pytest.fixture(scope="module")
def restated():
    """name -> select_numpy of the case: computed once, shared, never written to."""
    out = {}
    for name in SELECT_CASES:
        x, ranks, tile = sc.make_select_case(name)
        out[name] = sc.select_numpy(x, ranks, tile)
        for v in out[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def counted():
    return {name: sc.counts_numpy(*sc.make_count_case(name)) for name in COUNT_CASES}


# ---------------------------------------------------------------------------------- the select
@pytest.mark.parametrize("name", SELECT_CASES)
def test_restatement_against_sort_and_exact_arithmetic(restated, name):
    x, ranks, _ = sc.make_select_case(name)
    got, n = restated[name], x.size
    assert got["status"] == sc.STATUS.get(name, 0)
    bits = np.sort(x.view(np.uint32) & sc.ABS)[::-1]
    v = bits.view(np.float32).astype(np.float64)
    for q, r in enumerate(ranks):
        assert got["value"][q].tobytes() == bits[r].tobytes() and not np.signbit(got["value"][q])
        above, equal = int(got["above"][q]), int(got["equal"][q])
        assert above == int((bits > bits[r]).sum()) and equal == int((bits == bits[r]).sum())
        assert above <= r < above + equal                                             # the invariant of the issue
        if got["status"] == 0:
            assert sm.within(float(got["topk"][q]), math.fsum(v[:r + 1]) / (r + 1), r + 1)
    if got["status"] == 0:
        assert np.float32(got["max"]).tobytes() == bits[0].tobytes() and sm.within(got["mean"], math.fsum(v) / n, n)


@pytest.mark.parametrize("name", [c for c in SELECT_CASES if c not in sc.STATUS])
def test_restatement_equals_scores_numpy_for_every_rank_alone(restated, name):
    x, ranks, tile = sc.make_select_case(name)
    for q, r in enumerate(ranks):
        mx, mean, topk = sm.scores_numpy(x, r + 1)
        one = sc.select_numpy(x, (r,), tile)
        for got in ((one["max"], one["mean"], one["topk"][0]), (restated[name]["max"], restated[name]["mean"], restated[name]["topk"][q])):
            assert np.float32(got[0]).tobytes() == np.float32(mx).tobytes()
            assert np.float64(got[1]).tobytes() == np.float64(mean).tobytes() and np.float64(got[2]).tobytes() == np.float64(topk).tobytes()


def test_cases_are_what_their_names_say(restated):
    sizes = {sc.SELECT[c][0] for c in SELECT_CASES}
    assert {1, 63, 64, 65, 255, 256, 257, 3001, 70001} <= sizes
    assert sc.SELECT["n70001_t0"][1] == 0 and sc.default_tile(70001) == 1024 and all(sc.SELECT[c][1] == 256 for c in SELECT_CASES if c != "n70001_t0")
    assert -(-3001 // 256) == 12 and 3001 % 256 != 0
    assert (sc.default_tile(1), sc.default_tile(5767168), sc.default_tile(1 << 24), sc.default_tile((1 << 31) - 1)) == (1024, 2816, 8192, 16384)
    ranks = {c: sc.make_select_case(c)[1] for c in SELECT_CASES}
    assert ranks["n63_top"] == (0,) and ranks["n64_bottom"] == (63,) and ranks["n65_both"] == (0, 64)
    assert len(ranks["n3001_16ranks"]) == sc.MAX_RANKS and len(set(ranks["n3001_16ranks"])) < sc.MAX_RANKS
    assert (restated["constant"]["equal"] == 3001).all() and (restated["constant"]["above"] == 0).all()
    x = sc.make_select_case("lowbyte")[0].view(np.uint32)
    assert len(set((x >> 8).tolist())) == 1 and len(set((x & 255).tolist())) > 100
    x = sc.make_select_case("topbyte")[0]
    assert len(set((x.view(np.uint32) & 0xffffff).tolist())) == 1 and np.isfinite(x).all() and len(set((x.view(np.uint32) >> 24).tolist())) > 50
    x = sc.make_select_case("halfzero")[0]
    assert (x == 0).sum() >= 1500 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    t = restated["tie_run"]
    assert t["value"].tolist() == [2.0, 1.5, 1.5, 1.5, t["value"][4]] and t["value"][4] < 1.5 and t["equal"].tolist()[:4] == [5, 40, 40, 40]
    assert t["above"].tolist() == [0, 5, 5, 5, 45]
    v = restated["n3001_16ranks"]["value"].view(np.uint32)
    assert any(a != b and a >> 16 == b >> 16 and (a >> 8) & 255 != (b >> 8) & 255 for a in v[1:] for b in v[:1]), "no two ranks part ways in pass 2"
    for name in sc.STATUS:                                                            # the bad value sits in the last tile
        x, _, tile = sc.make_select_case(name)
        bad = np.flatnonzero(~np.isfinite(x) | (x < 0))
        assert bad.size == 1 and bad[0] >= (x.size - 1) // tile * tile
    buf, ranks, tile, n = sc.make_strided()
    assert np.isnan(buf[:, n:]).all() and np.isfinite(buf[[0, 2], :n]).all() and np.isinf(buf[1, :n]).sum() == 1 and buf.shape[1] > n


@pytest.mark.parametrize("defect", sc.SELECT_DEFECTS)
def test_planted_select_defect_changes_some_case(restated, defect):
    hit = []
    for name in SELECT_CASES:
        x, ranks, tile = sc.make_select_case(name)
        if not sc.same_select(sc.select_numpy(x, ranks, tile, defect=defect), restated[name], floats=name not in sc.STATUS):
            hit.append(name)
    print(defect, hit)
    assert hit, f"no case notices the defect {defect!r}"


# ---------------------------------------------------------------------------------- counts at thresholds
@pytest.mark.parametrize("name", COUNT_CASES)
def test_counts_restatement_against_loops(counted, name):
    mask, score, thr = sc.make_count_case(name)
    got = counted[name]
    S, n = score.shape
    T = thr.shape[-1]
    assert got["tp"].shape == got["fp"].shape == (S, T) and got["P"].shape == (S,)
    for s in range(S):
        m = mask if mask.ndim == 1 else mask[s]
        t = thr if thr.ndim == 1 else thr[s]
        assert got["P"][s] == int((m != 0).sum()) and got["P"][s] + got["N"][s] == n
        for j in range(T):
            pred = [bool(v > t[j]) for v in score[s].tolist()] if n <= 300 else (score[s] > t[j])
            assert got["tp"][s, j] == int((np.asarray(pred) & (m != 0)).sum()) and got["fp"][s, j] == int((np.asarray(pred) & (m == 0)).sum())


def test_count_cases_are_what_their_names_say(counted):
    assert {sc.COUNTS[c][2] for c in COUNT_CASES} >= {1, 16} and sc.MAX_THRESHOLDS == 16
    mask, score, thr = sc.make_count_case("t1_equal")
    assert (score[0] == thr[0]).any() and counted["t1_equal"]["tp"][0, 0] + counted["t1_equal"]["fp"][0, 0] == int((score[0] > thr[0]).sum())
    mask, score, thr = sc.make_count_case("t16_shared")
    assert mask.ndim == 1 and thr.ndim == 1 and thr[-1] > score.max() and (score[1] == thr[1]).any()
    assert counted["t16_shared"]["tp"][:, -1].tolist() == [0, 0, 0] and counted["t16_shared"]["fp"][:, -1].tolist() == [0, 0, 0]
    mask, score, thr = sc.make_count_case("t4_per_segment")
    assert mask.shape == score.shape and thr.shape == (3, 4) and (score[2] == thr[2, 1]).any()
    mask, score, thr = sc.make_count_case("zeros")
    zero = score[0] == 0
    assert np.signbit(score[0][zero]).any() and not np.signbit(score[0][zero]).all() and np.signbit(thr).tolist() == [False, True]
    c = counted["zeros"]
    assert (c["tp"] + c["fp"])[0].tolist() == [int((~zero).sum())] * 2                # neither zero is above either zero
    assert counted["bad_mask"]["status"].tolist() == [0, sc.BAD_MASK_BIT] and counted["nan_score"]["status"].tolist() == [sc.NAN_BIT, 0]
    mask, score, thr = sc.make_count_case("nan_score")
    assert np.isnan(score[0, -1]) and mask[0, -1] == 1 and counted["nan_score"]["tp"][0, 0] == int(((score[0] > 0) & (mask[0] != 0)).sum())
    assert sc.COUNTS["n70001"][1] > sc.COUNT_TILE and sc.COUNTS["n70001"][1] % sc.COUNT_TILE != 0


@pytest.mark.parametrize("defect", sc.COUNT_DEFECTS)
def test_planted_count_defect_changes_some_case(counted, defect):
    hit = [name for name in COUNT_CASES if not sc.same_counts(sc.counts_numpy(*sc.make_count_case(name), defect=defect), counted[name])]
    print(defect, hit)
    assert hit, f"no case notices the defect {defect!r}"


def test_every_defect_of_the_issue_is_planted():
    assert set(sc.DEFECTS) == set(sc.SELECT_DEFECTS) | set(sc.COUNT_DEFECTS) and len(sc.DEFECTS) == 7


# ---------------------------------------------------------------------------------- the calibration rule
@pytest.mark.parametrize("seed", range(10))
def test_calibration_rule(seed):
    rng = np.random.default_rng(7700 + seed)
    n = int(rng.integers(50, 5000))
    v = sm._errors(rng, (n,))
    if seed % 3 == 0:
        v[rng.integers(0, n, n // 4)] = v[0]                                          # ties around the ranks
    desc = np.sort(v)[::-1]
    for fpr in (0.0, 0.001, 0.01, 0.05, 0.5):
        k = sc.rank_of(fpr, n)
        assert k == math.floor(fpr * n) and k < n
        thr = sc.threshold_numpy(v, fpr)
        assert thr == desc[k] and int((v > thr).sum()) <= k
        assert sc.select_numpy(v, (k,))["value"][0] == thr
        if k > 0 and desc[k - 1] > thr:
            assert int((v > np.nextafter(thr, np.float32(0))).sum()) > k              # the smallest such value
    assert sc.threshold_numpy(v, 0.0) == v.max()
    roi = rng.random(n) < 0.6                                                         # zeroed outside a region of interest
    z = np.where(roi, v, np.float32(0))
    for fpr in (0.001, 0.05):
        assert sc.threshold_numpy(z, fpr, negatives=int(roi.sum())) == sc.threshold_numpy(v[roi], fpr)


# ---------------------------------------------------------------------------------- header, binding, host checks
def test_header_and_binding():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 37 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    assert _lib.SELECT_MAX_RANKS == sc.MAX_RANKS == 16 and _lib.THRESHOLD_COUNTS_MAX == sc.MAX_THRESHOLDS and _lib.SELECT_BAD_RANK == sc.BAD_RANK_BIT
    assert (_lib.ROC_NAN, _lib.ROC_INF, _lib.ROC_NEGATIVE, _lib.ROC_BAD_MASK) == (sc.NAN_BIT, sc.INF_BIT, sc.NEGATIVE_BIT, sc.BAD_MASK_BIT)
    assert _lib.SELECT_BAD_RANK & (_lib.ROC_NAN | _lib.ROC_INF | _lib.ROC_NEGATIVE | _lib.ROC_BAD_MASK | _lib.ROC_CURVE_TRUNCATED) == 0
    for name, st in (("select", _lib.SelectArgs), ("threshold_counts", _lib.ThresholdCountsArgs)):
        assert st in _lib._STRUCTS and L.anoddpm_struct_size(b"anoddpm_%s_args" % name.encode()) == ctypes.sizeof(st)
    for sym in ("anoddpm_select_wide", "anoddpm_select_wide_workspace_bytes", "anoddpm_threshold_counts"):
        assert sym in _lib.SYMBOLS and hasattr(L, sym)
    assert L.anoddpm_select_wide_workspace_bytes.restype is ctypes.c_int64
    assert [n for n, _ in _lib.SelectArgs._fields_][:3] == ["src", "ranks", "ranks_host"]
    import evaluation
    from anoddpm_amd import metrics
    for name in ("order_stats", "counts_at", "scores_at", "anomaly_metrics_at", "HealthyPool"):
        assert getattr(evaluation, name) is getattr(metrics, name) and name in metrics.__all__
    from anoddpm_amd.diffusion import GaussianDiffusionModel
    assert GaussianDiffusionModel.operating_thresholds is None


def test_workspace_bytes_refuses_exactly_what_the_call_refuses():
    from anoddpm_amd import _lib
    L = _lib.lib()
    ws = L.anoddpm_select_wide_workspace_bytes
    host = (ctypes.c_uint32 * 16)(*([0] * 16))

    def call(n, Q, tile):
        a = _lib.SelectArgs()
        a.src, a.ranks, a.ranks_host, a.workspace, a.workspace_bytes = 0x10000, 0x20000, ctypes.addressof(host), 0x30000, 0   # too small: never launches
        a.value, a.above, a.equal, a.topk_mean, a.max, a.mean, a.status = 0x40000, 0x41000, 0x42000, 0x43000, 0x44000, 0x45000, 0x46000
        a.src_stride, a.n, a.S, a.Q = n, n, 1, Q
        rc = L.anoddpm_select_wide(ctypes.byref(a), tile, None)
        return rc, L.anoddpm_last_error().decode()

    for n in (0, -1, 1, 255, 256, 3001, 1 << 24, (1 << 24) + 1, (1 << 31) - 1, 1 << 31, 1 << 40):
        for Q in (0, 1, 16, 17):
            for tile in (-256, 0, 100, 256, 4096, 1 << 20):
                b = ws(n, Q, tile)
                rc, msg = call(n, Q, tile)
                assert rc != 0
                assert (b == -1) == ("workspace too small" not in msg), (n, Q, tile, b, msg)   # accepted up to the workspace check, or refused before it
                assert b == -1 or b > 0
    for tile in (0, 256, 4096):
        for Q in (1, 4, 16):
            sizes = [ws(n, Q, tile) for n in (1, 256, 257, 70001, 1 << 20, 1 << 24, (1 << 24) + 4097, 1 << 30, (1 << 31) - 1)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0, (tile, Q, sizes)
    assert ws(1 << 30, 16, 0) < (1 << 20)                                             # O(Q), not O(n)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call here is refused by the argument checks: nothing reaches the device (the pointers are made-up addresses)."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    good = (ctypes.c_uint32 * 3)(0, 5, 99)
    past = (ctypes.c_uint32 * 3)(0, 100, 99)

    def select(tile=0, **kw):
        a = _lib.SelectArgs()
        a.src, a.ranks, a.ranks_host, a.workspace, a.workspace_bytes = 0x10000, 0x20000, ctypes.addressof(good), 0x30000, 1 << 20
        a.value, a.above, a.equal, a.topk_mean, a.max, a.mean, a.status = 0x40000, 0x41000, 0x42000, 0x43000, 0x44000, 0x45000, 0x46000
        a.src_stride, a.n, a.S, a.Q = 100, 100, 2, 3
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.anoddpm_select_wide(ctypes.byref(a), tile, None)
        return rc, L.anoddpm_last_error().decode()

    for kw, text in ([({p: None}, "null") for p in ("src", "ranks", "workspace", "value", "above", "equal", "topk_mean", "max", "mean", "status")]
                     + [({"S": 0}, "S must"), ({"n": 0}, "n must"), ({"n": 1 << 31, "src_stride": 1 << 31}, "n must"), ({"Q": 0}, "Q must"),
                        ({"Q": 17}, "Q must"), ({"tile": 100}, "tile"), ({"tile": -256}, "tile"), ({"src_stride": 99}, "src_stride"),
                        ({"workspace_bytes": 64}, "workspace too small"), ({"workspace": 0x30008}, "aligned"),
                        ({"ranks_host": ctypes.addressof(past)}, "not below n"), ({"n": 99, "src_stride": 99}, "not below n")]):
        rc, msg = select(**kw)
        assert rc != 0 and text in msg, (kw, rc, msg)
    assert L.anoddpm_select_wide(None, 0, None) != 0

    def counts(**kw):
        a = _lib.ThresholdCountsArgs()
        a.score, a.mask, a.thr, a.counts, a.totals, a.status = 0x10000, 0x20000, 0x30000, 0x40000, 0x41000, 0x42000
        a.n, a.score_stride, a.mask_stride, a.thr_stride, a.S, a.T = 100, 100, 100, 4, 2, 4
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.anoddpm_threshold_counts(ctypes.byref(a), None)
        return rc, L.anoddpm_last_error().decode()

    for kw, text in ([({p: None}, "null") for p in ("score", "mask", "thr", "counts", "totals", "status")]
                     + [({"S": 0}, "S must"), ({"n": 0}, "n must"), ({"n": 1 << 31, "score_stride": 1 << 31, "mask_stride": 0}, "n must"),
                        ({"T": 0}, "T must"), ({"T": 17, "thr_stride": 17}, "T must"), ({"score_stride": 99}, "score_stride"),
                        ({"mask_stride": 50}, "mask_stride"), ({"thr_stride": 3}, "thr_stride"),
                        ({"n": (1 << 31) - 1, "score_stride": 1 << 31, "mask_stride": 0, "S": 1 << 20}, "S * tiles")]):
        rc, msg = counts(**kw)
        assert rc != 0 and text in msg, (kw, rc, msg)
    assert L.anoddpm_threshold_counts(None, None) != 0
