"""-m gpu: the chip-wide AUPRO path (csrc/pro_wide.hip: anoddpm_pro_auc_wide, metrics._pro_launch's dispatch to it,
PooledRegionCurves, the list form of AUPRO) against the one-workgroup launch anoddpm_pro_auc -- every output bit for bit, through
the C ABI with the outputs pre-filled and guard words around the workspace -- against the numpy restatement of
tests/pro_wide_cases.py for pools of mixed plane shapes, and against the fixture tests/golden/pro_kat.npz through the default tile."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pro_cases as pc
import pro_wide_cases as pw
import roc_cases as rc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                                                   # int32 words on both sides of the workspace (keeps it 16-byte aligned)
GUARD_WORD = 0x5A5A5A5A
TILES = (256, 1024, 0)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _areas(mask, conn):
    from anoddpm_amd import metrics
    m = _dev(mask)
    areas, counts = metrics.component_areas(m.reshape(-1, *mask.shape[-2:]), connectivity=conn, batched=True)
    return m, areas, counts


def _raw(score, areas, counts, n, limit, tile=None, S=1, s_stride=None, a_stride=None, mask=None, m_stride=None, cap=None, dims=None,
         expect=0):
    """One launch through the C ABI on device tensors: anoddpm_pro_auc (tile None) or anoddpm_pro_auc_wide.  Every output is
    filled with NaN / -1 first; returns them as numpy arrays.  The workspace stands between guard words."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    cap = n if cap is None else cap
    out = {"aupro": torch.full((S,), float("nan"), dtype=torch.float64, device=DEV),
           "counts": torch.full((S, 4), -1, dtype=torch.int64, device=DEV),
           "status": torch.full((S,), -1, dtype=torch.int32, device=DEV),
           "fps": torch.full((S, cap), -1, dtype=torch.int32, device=DEV),
           "pro": torch.full((S, cap), float("nan"), dtype=torch.float64, device=DEV),
           "thr": torch.full((S, cap), float("nan"), dtype=torch.float32, device=DEV),
           "len": torch.full((S,), -1, dtype=torch.int32, device=DEV)}
    a = _lib.ProArgs()
    a.score, a.area, a.region_counts = score.data_ptr(), areas.data_ptr(), counts.data_ptr()
    if mask is not None:
        a.mask = mask.data_ptr()
    a.aupro, a.counts, a.status = out["aupro"].data_ptr(), out["counts"].data_ptr(), out["status"].data_ptr()
    a.curve_fps, a.curve_pro, a.curve_thr, a.curve_len, a.curve_cap = (out["fps"].data_ptr(), out["pro"].data_ptr(), out["thr"].data_ptr(),
                                                                     out["len"].data_ptr(), cap)
    a.score_stride = n if s_stride is None else s_stride
    a.area_stride = n if a_stride is None else a_stride
    a.mask_stride = a.area_stride if m_stride is None else m_stride
    a.limit, a.S = float(limit), S
    a.planes_per_segment, a.H, a.W = dims if dims is not None else (1, 1, n)
    assert a.planes_per_segment * a.H * a.W == n
    nbytes = L.anoddpm_pro_workspace_bytes(S, n) if tile is None else L.anoddpm_pro_wide_workspace_bytes(S, n, tile if expect == 0 else 0)
    assert nbytes > 0 and nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr() + 4 * GUARD, nbytes
    stream = _lib.current_stream()
    got = L.anoddpm_pro_auc(ctypes.byref(a), stream) if tile is None else L.anoddpm_pro_auc_wide(ctypes.byref(a), tile, stream)
    assert got == expect, L.anoddpm_last_error()
    torch.cuda.synchronize()
    assert bool((ws[:GUARD] == GUARD_WORD).all()) and bool((ws[-GUARD:] == GUARD_WORD).all()), "a guard word of the workspace was written"
    if expect != 0:
        assert bool((ws == GUARD_WORD).all()), "a refused call wrote into the workspace"
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, want, what, status_only=False):
    for k in (("status",) if status_only else want):
        assert rc.bits_equal(got[k], want[k]), (what, k, got[k].reshape(-1)[:8], want[k].reshape(-1)[:8])


def _compare_case(name, tiles=TILES, limit=None, cap=None):
    """Both entry points on every segment layout of a case: score [S, m, H, W]; a mask of one segment's shape is shared."""
    mask, score, case_limit, conn = pw.make_case(name)
    limit = case_limit if limit is None else limit
    S, n = score.shape[0], score[0].size
    m, areas, counts = _areas(mask, conn)
    shared = mask.ndim == 3 and S > 1
    stride = 0 if shared else n
    s = _dev(score)
    dims = (score.shape[1], score.shape[2], score.shape[3])
    want = _raw(s, areas, counts, n, limit, S=S, a_stride=stride, mask=m, cap=cap, dims=dims)
    assert (want["len"] >= 1).all() and (want["counts"][:, 1] + want["counts"][:, 2] == n).all()
    for tile in tiles:
        # the wide entry point reads the plane shape only through n: the flat form of the same segment gives the same bits
        for d in (dims, None) if counts.numel() == 1 else (dims,):
            _assert_same(_raw(s, areas, counts, n, limit, tile=tile, S=S, a_stride=stride, mask=m, cap=cap, dims=d), want, (name, tile, d))
    return want


# ---- 1. bit equality with the one-workgroup launch
@pytest.mark.parametrize("name", pw.CPU_CASES)
def test_every_output_equals_the_one_workgroup_launch(name):
    want = _compare_case(name)
    if name in ("mask_all0", "mask_all1"):
        assert np.isnan(want["aupro"][0]) and (want["counts"][0, 0] == 0 if name == "mask_all0" else want["counts"][0, 1] == 0)
    if name in ("odd40x33", "last_one", "full_curve"):
        assert want["len"][0] > 1024                         # several rounds of the lane sum


@pytest.mark.parametrize("name", (pc.RAGGED, "many_ties"))
def test_other_limits_and_a_truncated_curve(name):
    from anoddpm_amd import _lib
    _compare_case(name, limit=1.0)
    want = _compare_case(name, tiles=(256, 0), cap=7)
    assert want["status"][0] == _lib.ROC_CURVE_TRUNCATED and want["len"][0] > 7


def test_limit_exactly_on_a_curve_point():
    want = _compare_case("at_limit")
    assert (want["fps"][0, :want["len"][0]] == 3).any() and want["counts"][0, 1] == 10       # FPR 3 / 10 = the limit


def test_chains_longer_than_one_staging_round():
    """walk_carry stages 256 group totals per chain and round: 16 * 256 * 64 = 262144 elements fit in one round.  300 x 900 =
    270000 elements give chains of 264 groups (the last of 260), so a second round of 8 -- the smallest size that takes it, and
    only the two entry points are compared."""
    rng = np.random.default_rng(740)
    mask = np.zeros((1, 300, 900), np.float32)
    for y, x, h, w in pw.ODD_RECTS + ((50, 100, 40, 43), (200, 500, 61, 77), (120, 700, 9, 11)):
        mask[0, y:y + h, x:x + w] = 1
    score = pc._scores(rng, mask, levels=4000)
    m, areas, counts = _areas(mask, 2)
    s = _dev(score)
    want = _raw(s, areas, counts, 270000, 0.3, mask=m)
    assert want["len"][0] > 1024 and want["counts"][0, 0] == 9
    for tile in (1024, 0):
        _assert_same(_raw(s, areas, counts, 270000, 0.3, tile=tile, mask=m), want, ("two rounds", tile))


# ---- 2. several segments: strided scores, a shared mask and masks of their own
def test_three_segments_strided():
    mask, score, limit, conn = pw.make_case(pc.RAGGED)
    n, stride = score[0].size, 8192
    rng = np.random.default_rng(720)
    scores = np.zeros((3, stride), np.float32)
    for j in range(3):
        scores[j, :n] = pc._scores(rng, mask, shift=0.2 * (j + 1), levels=(8, None, 40)[j]).reshape(-1)
    s = _dev(scores)
    m, areas, counts = _areas(mask, conn)
    want = _raw(s, areas, counts, n, limit, S=3, s_stride=stride, a_stride=0, mask=m)
    for tile in (256, 0):
        got = _raw(s, areas, counts, n, limit, tile=tile, S=3, s_stride=stride, a_stride=0, mask=m)
        _assert_same(got, want, ("shared mask", tile))
        for j in range(3):
            single = _raw(s[j], areas, counts, n, limit, tile=tile, mask=m)
            for k in got:
                assert rc.bits_equal(got[k][j:j + 1], single[k]), (tile, j, k)
    # three masks of their own: area_stride = n, one region count per segment
    masks = np.stack([np.roll(mask, 7 * j, axis=-1) for j in range(3)])
    m3, areas3, counts3 = _areas(masks, conn)
    want = _raw(s, areas3, counts3, n, limit, S=3, s_stride=stride, mask=m3)
    _assert_same(_raw(s, areas3, counts3, n, limit, tile=256, S=3, s_stride=stride, mask=m3), want, "own masks")


# ---- 3. precondition: the offending element sits in the last tile of the input
@pytest.mark.parametrize("what", ("nan", "inf", "negative", "mask"))
def test_status_word_of_the_last_tile(what):
    from anoddpm_amd import _lib
    mask, score, limit, conn = pw.make_case("last_one")
    m, areas, counts = _areas(mask, conn)
    score, check = score.copy().reshape(-1), mask.copy().reshape(-1)
    if what == "mask":
        check[1024] = 0.5                                    # tile 256: the last tile is this one element
    else:
        score[1024] = {"nan": np.nan, "inf": np.inf, "negative": -0.5}[what]
    bit = {"nan": _lib.ROC_NAN, "inf": _lib.ROC_INF, "negative": _lib.ROC_NEGATIVE, "mask": _lib.ROC_BAD_MASK}[what]
    s, mk = _dev(score), _dev(check)
    want = _raw(s, areas, counts, 1025, limit, mask=mk)
    assert want["status"][0] == bit
    for tile in (256, 0):
        _assert_same(_raw(s, areas, counts, 1025, limit, tile=tile, mask=mk), want, (what, tile), status_only=True)


# ---- 4. refused calls launch nothing
def test_refused_calls_write_nothing():
    from anoddpm_amd import _lib
    mask, score, limit, conn = pw.make_case("plane16")
    m, areas, counts = _areas(mask, conn)
    s = _dev(score)
    for kw, text in ((dict(tile=100), b"multiple of 256"), (dict(tile=256, limit=0.0), b"limit"), (dict(tile=256, cap=0), b"curve capacity"),
                     (dict(tile=256, S=2, s_stride=8), b"score_stride")):
        args = dict(limit=limit, expect=-1)
        args.update(kw)
        lim = args.pop("limit")
        cap = args.pop("cap", None)
        if cap == 0:                                         # a curve buffer of one point, declared as none
            out = _raw_zero_cap(s, areas, counts, 256, lim)
        else:
            out = _raw(s, areas, counts, 256, lim, **args)
            assert np.isnan(out["aupro"]).all() and (out["counts"] == -1).all() and (out["status"] == -1).all() and (out["len"] == -1).all()
        assert text in _lib.lib().anoddpm_last_error(), text


def _raw_zero_cap(s, areas, counts, n, limit):
    from anoddpm_amd import _lib
    L = _lib.lib()
    out = torch.full((8,), -1, dtype=torch.int64, device=DEV)
    a = _lib.ProArgs()
    a.score, a.area, a.region_counts = s.data_ptr(), areas.data_ptr(), counts.data_ptr()
    a.aupro = a.counts = a.status = a.curve_fps = a.curve_pro = a.curve_thr = a.curve_len = out.data_ptr()
    a.curve_cap, a.limit, a.S, a.planes_per_segment, a.H, a.W = 0, limit, 1, 1, 1, n
    nbytes = L.anoddpm_pro_wide_workspace_bytes(1, n, 256)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 256, _lib.current_stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == -1).all())
    return out


# ---- 5. dispatch
def test_dispatch(monkeypatch):
    from anoddpm_amd import metrics
    mask, score, limit, conn = pw.make_case(pc.RAGGED)
    m, s = _dev(mask), _dev(score[0])

    def everything():
        val, status = metrics.aupro(m, s, batched=False, return_status=True)
        return ({"aupro": val.cpu().numpy(), "status": status.cpu().numpy()}, metrics.pro_points(m, s, batched=False)[0],
                metrics.AUPRO(m, s), metrics._pro_launch(m, s, limit, conn, False, curve=False)["path"])

    monkeypatch.setattr(metrics, "PRO_WIDE_MIN_N", 1 << 31)
    off = everything()
    monkeypatch.setattr(metrics, "PRO_WIDE_MIN_N", 1024)
    on = everything()
    assert (off[3], on[3]) == ("workgroup", "wide")
    for k in off[0]:
        assert rc.bits_equal(on[0][k], off[0][k]), k
    assert set(on[1]) == set(off[1])
    for k in on[1]:
        assert rc.bits_equal(np.asarray(on[1][k]), np.asarray(off[1][k])), k
    assert rc.bits_equal(np.float64(on[2]), np.float64(off[2]))
    # a batch stays on the one-workgroup path, a short segment too
    batch = _dev(np.stack([score[0], score[0]]))
    assert metrics._pro_launch(m, batch, limit, conn, True, curve=False)["path"] == "workgroup"
    assert metrics._pro_launch(m[:, :10], s[:, :10], limit, conn, False, curve=False)["path"] == "workgroup"
    # the explicit keywords: wide on a batch processes its segments one after another
    a = metrics._pro_launch(m, batch, limit, conn, True, curve=True, wide=True, tile=256)
    b = metrics._pro_launch(m, batch, limit, conn, True, curve=True, wide=False)
    assert (a["path"], b["path"]) == ("wide", "workgroup")
    for k in ("aupro", "counts", "status", "len"):
        assert rc.bits_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    for j, L in enumerate(a["len"].tolist()):                           # the buffers are not initialised past the curve's end
        for k in ("fps", "pro", "thresholds"):
            assert rc.bits_equal(a[k][j, :L].cpu().numpy(), b[k][j, :L].cpu().numpy()), (j, k)
    with pytest.raises(ValueError, match="tile"):
        metrics._pro_launch(m, s, limit, conn, False, curve=False, wide=True, tile=100)


# ---- 6. PooledRegionCurves and the list form of AUPRO
def test_pool_of_one_plane_shape_equals_aupro(monkeypatch):
    from anoddpm_amd import metrics
    import evaluation
    rng = np.random.default_rng(730)
    mask = np.stack([pc._blobs(rng, 16, 16, 3, 5)[None] for _ in range(6)])                # [6, 1, 16, 16]
    score = pc._scores(rng, mask)
    m, s = _dev(mask), _dev(score)
    for min_n in (1 << 31, 1):
        monkeypatch.setattr(metrics, "PRO_WIDE_MIN_N", min_n)
        pool = evaluation.PooledRegionCurves(6 * 256, device=DEV)
        pool.add(m[:2], s[:2])
        pool.add(m[2], s[2])
        pool.add(m[3:], s[3:])
        assert len(pool) == 6 * 256
        want, wstatus = metrics.aupro(m, s, batched=False, return_status=True)
        got, status = pool.aupro(return_status=True)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (1,)
        assert rc.bits_equal(got.cpu().numpy(), want.cpu().numpy()) and rc.bits_equal(status.cpu().numpy(), wstatus.cpu().numpy())
        p, q = pool.pro_curve(), metrics.pro_points(m, s, batched=False)[0]
        assert set(p) == set(q)
        for k in q:
            assert rc.bits_equal(np.asarray(p[k]), np.asarray(q[k])), k
        # the inherited scores are those of a PooledCurves fed the same adds
        plain = metrics.PooledCurves(6 * 256, device=DEV)
        plain.add(m[:2], s[:2])
        plain.add(m[2], s[2])
        plain.add(m[3:], s[3:])
        a, b = pool.scores(), plain.scores()
        assert set(a) == set(b)
        for k in b:
            assert rc.bits_equal(a[k].cpu().numpy(), b[k].cpu().numpy()), k
        with pytest.raises(ValueError, match="capacity"):
            pool.add(m[0], s[0])
        with pytest.raises(ValueError, match="does not match"):
            pool.add(m[0, 0, :3], s[0])
        # reset: the accumulator too
        pool.reset()
        assert len(pool) == 0 and int(pool._regions[0]) == 0
        with pytest.raises(ValueError, match="empty"):
            pool.aupro()
        pool.add(m, s)
        assert rc.bits_equal(pool.aupro().cpu().numpy(), want.cpu().numpy())


def test_pool_of_mixed_shapes_and_a_shared_mask_equals_the_restatement(monkeypatch):
    from anoddpm_amd import metrics
    adds = pw.pool_adds()
    n = sum(score.size for _, score in adds)
    for limit in (0.3, 1.0):
        want = pw.pool_numpy(adds, limit, 2, pw.default_tile(n))
        assert want["K"] > 0 and want["N"] > 0
        for min_n in (1 << 31, 1):
            monkeypatch.setattr(metrics, "PRO_WIDE_MIN_N", min_n)
            pool = metrics.PooledRegionCurves(n + 5, device=DEV)
            for mask, score in adds:
                pool.add(_dev(mask), _dev(score))
            assert len(pool) == n
            got = pool.pro_curve(limit)
            assert pw.differences(got, want) == [], (limit, min_n, pw.differences(got, want))
            assert rc.bits_equal(pool.aupro(limit).cpu().numpy(), np.array([want["aupro"]]))
            listed = metrics.AUPRO([_dev(mask) for mask, _ in adds], [_dev(score) for _, score in adds], limit=limit)
            assert isinstance(listed, float) and rc.bits_equal(np.float64(listed), np.float64(got["aupro"]))
    with pytest.raises(TypeError, match="pooled"):
        metrics.AUPRO([_dev(adds[0][0])], [_dev(adds[0][1]), _dev(adds[1][1])])


# ---- 7. the one workload-sized case through the default tile, against the fixture
def test_map256_through_the_default_tile(monkeypatch):
    from anoddpm_amd import metrics
    kat = np.load(os.path.join(GOLDEN, "pro_kat.npz"))
    name = "map256"
    mask, score, limit, conn = pc.make_case(name)
    assert pc.sha(mask, score) == str(kat[f"{name}_sha"]), f"{name}: the regenerated input differs from the fixture's"
    monkeypatch.setattr(metrics, "PRO_WIDE_MIN_N", 1)
    m, s = _dev(mask), _dev(score[0])
    assert metrics._pro_launch(m, s, limit, conn, False, curve=False)["path"] == "wide"
    p = metrics.pro_points(m, s, limit=limit, connectivity=conn, batched=False)[0]
    exact = pc.pro_exact(mask, score[0], limit, conn)
    assert pc.sha(exact["fps"], exact["thresholds"], exact["pro"]) == str(kat[f"{name}_curve_sha"][0])
    assert rc.bits_equal(np.float64(exact["aupro"]), np.float64(kat[f"{name}_aupro"][0]))
    pc.check_against_exact(p, exact, name)
    order = pc.pro_fp64(mask, score[0], limit, conn)
    assert rc.bits_equal(p["pro"], order["pro"]) and rc.bits_equal(np.float64(p["aupro"]), np.float64(order["aupro"]))
