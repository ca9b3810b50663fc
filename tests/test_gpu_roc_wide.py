"""-m gpu: the chip-wide ROC / PR path (csrc/roc_wide.hip: anoddpm_roc_auc_wide, and metrics._roc_launch's dispatch to it,
PooledCurves, the pooled form of ROC_AUC) against the one-workgroup launch anoddpm_roc_auc -- every output bit for bit, through
the C ABI with the outputs pre-filled and guard words around the workspace -- and against the sklearn fixtures
tests/golden/roc_kat.npz / pr_kat.npz through the default tile."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import pr_cases as pc
import roc_cases as rc
import roc_wide_cases as wc
from conftest import GOLDEN
from score_cases import tiny as _tiny
from test_gpu_roc import BAD

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                                                   # int32 words on both sides of the workspace (keeps it 16-byte aligned)
GUARD_WORD = 0x5A5A5A5A
PLAIN, FULL = "plain", "full"                                # ROC only with the DROP curve / AP, best Dice and the ALL curve


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "roc_kat.npz"))


@pytest.fixture(scope="module")
def pr_kat():
    return np.load(os.path.join(GOLDEN, "pr_kat.npz"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _raw(mask, score, n, mode, tile=None, S=1, s_stride=None, m_stride=None, cap=None):
    """One launch through the C ABI on device tensors mask / score: anoddpm_roc_auc (tile None) or anoddpm_roc_auc_wide.  Every
    output is filled with NaN / -1 first; returns them as numpy arrays.  The wide workspace stands between guard words."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    cap = max(n, 2) if cap is None else cap
    out = {"auc": torch.full((S,), float("nan"), dtype=torch.float64, device=DEV),
           "counts": torch.full((S, 4), -1, dtype=torch.int64, device=DEV),
           "status": torch.full((S,), -1, dtype=torch.int32, device=DEV),
           "fps": torch.full((S, cap), -1, dtype=torch.int32, device=DEV),
           "tps": torch.full((S, cap), -1, dtype=torch.int32, device=DEV),
           "thr": torch.full((S, cap), float("nan"), dtype=torch.float32, device=DEV),
           "len": torch.full((S,), -1, dtype=torch.int32, device=DEV)}
    a = _lib.RocArgs()
    a.score, a.mask = score.data_ptr(), mask.data_ptr()
    a.auc, a.counts, a.status = out["auc"].data_ptr(), out["counts"].data_ptr(), out["status"].data_ptr()
    a.curve_fps, a.curve_tps, a.curve_thr, a.curve_len, a.curve_cap = (out["fps"].data_ptr(), out["tps"].data_ptr(), out["thr"].data_ptr(),
                                                                     out["len"].data_ptr(), cap)
    a.n, a.S = n, S
    a.score_stride = n if s_stride is None else s_stride
    a.mask_stride = n if m_stride is None else m_stride
    if mode == FULL:
        out["ap"] = torch.full((S,), float("nan"), dtype=torch.float64, device=DEV)
        out["best_dice"] = torch.full((S,), float("nan"), dtype=torch.float64, device=DEV)
        out["best_thr"] = torch.full((S,), float("nan"), dtype=torch.float32, device=DEV)
        out["best_counts"] = torch.full((S, 2), -1, dtype=torch.int64, device=DEV)
        a.ap, a.best_dice, a.best_thr, a.best_counts = (out["ap"].data_ptr(), out["best_dice"].data_ptr(), out["best_thr"].data_ptr(),
                                                        out["best_counts"].data_ptr())
        a.curve_mode = _lib.ROC_CURVE_ALL
    nbytes = L.anoddpm_roc_workspace_bytes(S, n) if tile is None else L.anoddpm_roc_wide_workspace_bytes(S, n, tile)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr() + 4 * GUARD, nbytes
    stream = _lib.current_stream()
    rc_ = L.anoddpm_roc_auc(ctypes.byref(a), stream) if tile is None else L.anoddpm_roc_auc_wide(ctypes.byref(a), tile, stream)
    assert rc_ == 0, L.anoddpm_last_error()
    torch.cuda.synchronize()
    assert bool((ws[:GUARD] == GUARD_WORD).all()) and bool((ws[-GUARD:] == GUARD_WORD).all()), "a guard word of the workspace was written"
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, what, status_only=False):
    for k in (("status",) if status_only else want):
        assert rc.bits_equal(got[k], want[k]), (what, k, got[k].reshape(-1)[:8], want[k].reshape(-1)[:8])


def _compare_all(mask, score, what, tiles=(256, 1024, 0)):
    n = score.size
    m, s = _dev(mask), _dev(score)
    for mode in (PLAIN, FULL):
        want = _raw(m, s, n, mode)
        assert want["len"][0] >= 1 and want["counts"][0, 0] + want["counts"][0, 1] == n
        for tile in tiles:
            _assert_same(_raw(m, s, n, mode, tile=tile), want, (what, mode, tile))


# ---- 1. bit equality with the one-workgroup launch
@pytest.mark.parametrize("name", pc.SMALL + ("ragged",))
def test_every_output_equals_the_one_workgroup_launch(name):
    mask, score = wc.make_case(name)
    _compare_all(mask, score, name)


def test_truncated_curve_equals_the_one_workgroup_launch():
    mask, score = rc.make_ragged()
    m, s = _dev(mask), _dev(score)
    from anoddpm_amd import _lib
    for mode in (PLAIN, FULL):
        want = _raw(m, s, score.size, mode, cap=7)
        assert want["status"][0] == _lib.ROC_CURVE_TRUNCATED and want["len"][0] > 7
        for tile in (256, 0):
            _assert_same(_raw(m, s, score.size, mode, tile=tile, cap=7), want, ("truncated", mode, tile))


# ---- 2. constructed borders, n = 1024 at tile 256
@pytest.mark.parametrize("name", wc.BORDERS)
def test_constructed_borders(name):
    mask, score = wc.make_case(name)
    assert score.size == 1024
    _compare_all(mask, score, name, tiles=(256,))


# ---- 3. the fixtures through the default tile and the dispatch
@pytest.mark.parametrize("name", rc.MAPS + ("long",))
def test_fixtures_through_the_default_tile(kat, pr_kat, name, monkeypatch):
    from anoddpm_amd import metrics
    monkeypatch.setattr(metrics, "ROC_WIDE_MIN_N", 1)
    mask, score = rc.make_case(name)
    sha = rc.sha_inputs(mask[None], score[None]) if name == "long" else rc.sha_inputs(mask, score)
    assert sha == str(kat[f"{name}_sha"]), f"{name}: regenerated input differs from the fixture's"
    m, s = _dev(mask), _dev(score)
    assert metrics._roc_launch(m, s, False, curve=False)["path"] == "wide"
    fpr, tpr, thr = metrics.ROC_AUC(m, s)
    p = metrics.roc_points(m, s)[0]
    if name == "long":
        assert (p["P"], p["N"], p["twoU"]) == (int(kat["long_P"][0]), int(kat["long_N"][0]), int(kat["long_twoU"][0]))
        assert fpr.size == int(kat["long_len"][0]) and rc.sha_curve(fpr, tpr, thr) == str(kat["long_curve_sha"][0])
        want_auc = float(kat["long_auc"][0])
    else:
        assert rc.bits_equal(fpr, kat[f"{name}_fpr"]) and rc.bits_equal(tpr, kat[f"{name}_tpr"]) and rc.bits_equal(thr, kat[f"{name}_thr"])
        want_auc = float(kat[f"{name}_auc"])
    print(f"{name}: auc {p['auc']!r} fixture {want_auc!r} bound {rc.auc_tolerance(score.size):.3g}")
    assert abs(p["auc"] - want_auc) <= rc.auc_tolerance(score.size)
    pc.check_summary(pr_kat, name, 0, metrics.pr_points(m, s)[0], score.size)


# ---- 4. several segments: a strided score view and one shared mask
def test_three_segments_strided_with_a_shared_mask():
    masks, scores = rc.make_batch()
    n, stride = 5000, rc.N256
    big_s, m = _dev(scores[:3]), _dev(masks[1, :n])
    assert big_s[:, :n].stride(0) == stride
    for mode in (PLAIN, FULL):
        got = _raw(m, big_s, n, mode, tile=256, S=3, s_stride=stride, m_stride=0)
        for j in range(3):
            single = _raw(m, big_s[j], n, mode, tile=256)
            for k in got:
                assert rc.bits_equal(got[k][j:j + 1], single[k]), (mode, j, k)
        _assert_same(got, _raw(m, big_s, n, mode, S=3, s_stride=stride, m_stride=0), ("three segments", mode))


# ---- 5. precondition: the offending element sits in the last tile
@pytest.mark.parametrize("what,bad_score,bad_mask,text", BAD)
def test_status_word_of_the_last_tile(kat, what, bad_score, bad_mask, text):
    from anoddpm_amd import _lib
    mask, score = kat["n1025_mask"].copy(), kat["n1025_score"].copy()
    if bad_score is not None:
        score[1024] = bad_score                              # tile 256: the last tile is this one key
    if bad_mask is not None:
        mask[1024] = bad_mask
    m, s = _dev(mask), _dev(score)
    bit = {"nan": _lib.ROC_NAN, "inf": _lib.ROC_INF, "negative": _lib.ROC_NEGATIVE, "mask2": _lib.ROC_BAD_MASK}[what]
    for mode in (PLAIN, FULL):
        want = _raw(m, s, 1025, mode)
        assert want["status"][0] == bit
        for tile in (256, 0):
            _assert_same(_raw(m, s, 1025, mode, tile=tile), want, (what, mode, tile), status_only=True)


# ---- 6. determinism
def test_two_runs_are_bit_identical():
    mask, score = rc.make_ragged()
    m, s = _dev(mask), _dev(score)
    _assert_same(_raw(m, s, score.size, FULL, tile=256), _raw(m, s, score.size, FULL, tile=256), "two runs")


# ---- 7. PooledCurves and the pooled form of ROC_AUC
def test_pooled_curves():
    from anoddpm_amd import metrics
    import evaluation
    side = inspect.signature(_tiny).parameters["size"].default
    assert side == 32
    px, maps = side * side, 88
    rng = np.random.default_rng(600)
    mask, score = rc._variant("round1024", rng, maps * px, 0.05)
    mask, score = mask.reshape(maps, 1, side, side), score.reshape(maps, 1, side, side)
    mask[40:70] = mask[40]                                   # the second call shares one mask plane
    m, s = _dev(mask), _dev(score)
    pool = evaluation.PooledCurves(maps * px, device=DEV)
    assert len(pool) == 0
    pool.add(m[:40], s[:40])
    pool.add(m[40, 0], s[40:70])
    pool.add(m[70:], s[70:])
    assert len(pool) == maps * px
    with pytest.raises(ValueError, match="capacity"):
        pool.add(m[0], s[0])
    with pytest.raises(ValueError, match="does not match"):
        pool.add(m[0, 0, :3], s[0])
    got, want = pool.scores(), metrics.curve_scores(m.reshape(-1), s.reshape(-1), batched=False)
    assert set(got) == set(want)
    for k in want:
        assert rc.bits_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), k
    r = rc.roc_numpy(mask, score)
    for g, w in zip(pool.roc_curve(), rc.sklearn_triple(r["fps"], r["tps"], r["thresholds"])):
        assert rc.bits_equal(g, w)
    p = pc.pr_numpy(mask, score)
    for g, w in zip(pool.pr_curve(), pc.sklearn_triple(p["fps"], p["tps"], p["thresholds"])):
        assert rc.bits_equal(g, w)
    pool.reset()
    assert len(pool) == 0
    with pytest.raises(ValueError, match="empty"):
        pool.scores()
    pool.add(m[:2], s[:2])
    assert len(pool) == 2 * px
    # lists on both sides: the pooled segment of all of them
    cat_m, cat_s = torch.cat([m[3].reshape(-1), m[50].reshape(-1)]), torch.cat([s[3].reshape(-1), s[50].reshape(-1)])
    for f in (metrics.ROC_AUC, metrics.PR_curve):
        for g, w in zip(f([m[3], m[50]], [s[3], s[50]]), f(cat_m, cat_s)):
            assert rc.bits_equal(g, w)
    with pytest.raises(TypeError, match="pooled"):
        metrics.ROC_AUC([m[3]], [s[3], s[50]])


# ---- 8. dispatch
def test_dispatch(monkeypatch):
    from anoddpm_amd import metrics
    mask, score = rc.make_ragged()
    m, s = _dev(mask), _dev(score)

    def everything():
        cs = metrics.curve_scores(m, s, batched=False)
        return ({"auc": metrics.roc_auc(m, s).cpu().numpy(), **{k: v.cpu().numpy() for k, v in cs.items()}},
                metrics.roc_points(m, s)[0], metrics.pr_points(m, s)[0], metrics._roc_launch(m, s, False, curve=False)["path"])

    monkeypatch.setattr(metrics, "ROC_WIDE_MIN_N", 1 << 31)
    off = everything()
    monkeypatch.setattr(metrics, "ROC_WIDE_MIN_N", 1024)
    on = everything()
    assert (off[3], on[3]) == ("workgroup", "wide")
    for k in off[0]:
        assert rc.bits_equal(on[0][k], off[0][k]), k
    for a, b in ((on[1], off[1]), (on[2], off[2])):
        assert set(a) == set(b)
        for k in a:
            assert rc.bits_equal(np.asarray(a[k]), np.asarray(b[k])), k
    # a batch stays on the one-workgroup path, a short segment too
    masks, scores = rc.make_batch()
    assert metrics._roc_launch(_dev(masks[:2]), _dev(scores[:2]), True, curve=False)["path"] == "workgroup"
    assert metrics._roc_launch(m[:1000], s[:1000], False, curve=False)["path"] == "workgroup"
    # the explicit keywords: wide on a batch processes its segments one after another
    a = metrics._roc_launch(_dev(masks[:2, :5000]), _dev(scores[:2, :5000]), True, curve=True, pr=True, wide=True, tile=256)
    b = metrics._roc_launch(_dev(masks[:2, :5000]), _dev(scores[:2, :5000]), True, curve=True, pr=True, wide=False)
    assert (a["path"], b["path"]) == ("wide", "workgroup")
    for k in ("auc", "counts", "status", "len", "ap", "best_dice", "best_threshold", "best_counts"):
        assert rc.bits_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    with pytest.raises(ValueError, match="tile"):
        metrics._roc_launch(m, s, False, curve=False, wide=True, tile=100)
