"""The chip-wide AUPRO path without a device: the numpy restatement of the launch sequence of csrc/pro_wide.hip
(tests/pro_wide_cases.py) equals the restatement of the one-workgroup kernel (pro_cases.pro_fp64) bit for bit on every case at
tiles 256, 1024 and the default, each planted defect of that restatement is caught by the case list, and the host side of the two
new entry points: refusals before anything is launched, workspace sizes.  CPU only."""
import ctypes

import numpy as np
import pytest

import pro_cases as pc
import pro_wide_cases as pw

ALL_TILES = pw.TILES + (0,)


def _tile(tile, n):
    return tile if tile else pw.default_tile(n)


@pytest.mark.parametrize("tile", ALL_TILES)
@pytest.mark.parametrize("name", pw.CPU_CASES)
def test_restatement_equals_the_one_workgroup_restatement(name, tile):
    n = pw.make_case(name)[1][0].size
    assert pw.case_differences(name, _tile(tile, n)) == []


def test_cases_are_what_they_are_for():
    sizes = {name: pw.make_case(name)[1][0].size for name in pw.CPU_CASES}
    chunk = lambda n: ((n + 15) // 16 + 63) & ~63
    # a chunk border inside a 256-tile and n no multiple of 64; two chunks per tile with eleven of sixteen waves used; a chunk
    # that is a multiple of both tiles; one group; a last tile of one element
    assert sizes[pc.RAGGED] == 5000 and chunk(5000) == 320 and 5000 % 64
    assert sizes["odd40x33"] == 1320 and chunk(1320) == 128 and -(-1320 // 128) == 11
    assert sizes["chunk_is_tile"] == 16384 and chunk(16384) == 1024
    assert sizes["tiny5x7"] <= 64 and sizes["last_one"] == 1025
    # weights that are inexact in fp64 beside exact ones, in every case that is there for the order of the additions
    for name in (pc.RAGGED, "last_one", "chunk_is_tile", "many_ties", "long_run"):
        mask, score, limit, conn = pw.make_case(name)
        sizes_of = set(np.unique(pc.regions(mask, conn)[0]).tolist()) - {0}
        assert sizes_of & {3, 6, 7, 15} and sizes_of & {1, 2}, (name, sizes_of)
    pooled = [set(np.unique(pc.regions(mask.reshape(-1, *mask.shape[-2:]), 2)[0]).tolist()) for mask, score in pw.pool_adds()]
    assert all(s & {1, 2, 3, 7} for s in pooled) and sum(bool(s & {3, 7}) for s in pooled) >= 3
    # a run that covers two whole tiles of the walk: tiles 1 and 2 hold no run end
    mask, score, limit, conn = pw.make_case("long_run")
    s = np.sort(score.reshape(-1))[::-1]
    end = np.r_[s[1:] != s[:-1], True]
    assert not end[256:768].any() and end[:256].any() and end[768:].any()
    # more than 1024 runs: several rounds of the lane sum; K == 0 and N == 0
    assert pc.pro_fp64(*[x[0] if i == 1 else x for i, x in enumerate(pw.make_case("odd40x33"))])["fps"].size > 1024
    assert pw.wide_case(pw.make_case("mask_all0")[0], pw.make_case("mask_all0")[1][0], 0.3, 2, 256)["K"] == 0
    assert pw.wide_case(pw.make_case("mask_all1")[0], pw.make_case("mask_all1")[1][0], 0.3, 2, 256)["N"] == 0
    # one tile of one digit in a pass where the segment has several
    mask, score, limit, conn = pw.make_case("tile_digit")
    key = pw.keys_of(pc.regions(mask, conn)[0], score)
    assert np.unique(key[:256] & 255).size == 1 and np.unique(key & 255).size > 1


CAUGHT_BY = {"carry_per_tile": ("chunk_is_tile", 256), "totals_tile_major": (pc.RAGGED, 256), "groups_in_i": ("odd40x33", 256),
             "payload_own_rank": (pc.RAGGED, 1024), "run_end_blind": ("long_run", 256), "term_blind": ("last_one", 256),
             "trapezoid_per_tile": ("full_curve", 1024)}


@pytest.mark.parametrize("defect", [d for d in pw.DEFECTS if d != "shared_once"])
def test_planted_defect_is_caught(defect):
    name, tile = CAUGHT_BY[defect]
    bad = pw.case_differences(name, tile, defect)
    print(defect, name, tile, bad)
    assert bad, f"{defect} passes {name} at tile {tile}"


def test_shared_mask_regions_counted_once_is_caught():
    adds = pw.pool_adds()
    good, bad = pw.pool_numpy(adds, 0.3, 2, 256), pw.pool_numpy(adds, 0.3, 2, 256, "shared_once")
    assert good["K"] == bad["K"] + 2 * 3 and pw.differences(bad, good)
    # the pool at every tile is one curve
    assert pw.differences(pw.pool_numpy(adds, 0.3, 2, 1024), good) == []


def test_wide_abi_refusals_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 36 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    assert L.anoddpm_pro_auc_wide.argtypes == [ctypes.POINTER(_lib.ProArgs), ctypes.c_int32, ctypes.c_void_p]
    assert L.anoddpm_pro_wide_workspace_bytes.restype is ctypes.c_int64
    assert L.anoddpm_pro_auc_wide(None, 0, None) == -1 and b"null args" in L.anoddpm_last_error()
    a = _lib.ProArgs()
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 0, None) == -1 and b"null pointer" in L.anoddpm_last_error()
    # host memory stands in for the device pointers: every case below is rejected before anything is launched
    buf = (ctypes.c_char * 128)()
    p = (ctypes.addressof(buf) + 15) & ~15
    a.score = a.area = a.region_counts = a.workspace = a.aupro = a.counts = a.status = p
    a.S, a.planes_per_segment, a.H, a.W, a.limit = 0, 1, 4, 4, 0.3
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 0, None) == -1 and b"S must be" in L.anoddpm_last_error()
    a.S, a.H = 1, 0
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 0, None) == -1 and b"must be >= 1" in L.anoddpm_last_error()
    a.planes_per_segment, a.H, a.W = 2, 1 << 15, 1 << 15
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 0, None) == -1 and b"2^31" in L.anoddpm_last_error()
    a.planes_per_segment, a.H, a.W, a.limit = 1, 4, 4, 0.0
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 0, None) == -1 and b"limit" in L.anoddpm_last_error()
    a.limit, a.S, a.score_stride = 0.3, 2, 8
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 0, None) == -1 and b"score_stride" in L.anoddpm_last_error()
    a.score_stride, a.area_stride = 16, 8
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 0, None) == -1 and b"area_stride" in L.anoddpm_last_error()
    a.area_stride, a.mask, a.mask_stride = 0, p, 8
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 0, None) == -1 and b"mask_stride" in L.anoddpm_last_error()
    a.mask_stride = 0
    a.workspace_bytes = 1 << 40
    for tile in (-256, 100, 255, 257, 1000):
        assert L.anoddpm_pro_auc_wide(ctypes.byref(a), tile, None) == -1 and b"multiple of 256" in L.anoddpm_last_error(), tile
    a.H, a.W = 1, 256 * _lib.ROC_WIDE_MAX_TILES + 1
    a.score_stride = a.W
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 256, None) == -1 and b"tiles" in L.anoddpm_last_error()
    a.H, a.W, a.score_stride = 4, 4, 16
    for tile in (0, 256, 1024):
        a.workspace_bytes = L.anoddpm_pro_wide_workspace_bytes(2, 16, tile) - 1
        assert a.workspace_bytes > 0
        assert L.anoddpm_pro_auc_wide(ctypes.byref(a), tile, None) == -1 and b"workspace too small" in L.anoddpm_last_error()
    a.workspace_bytes += 1
    a.workspace = p + 4
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 1024, None) == -1 and b"aligned" in L.anoddpm_last_error()
    a.workspace = p
    a.curve_fps = p                                                     # some but not all of the curve outputs
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 1024, None) == -1 and b"curve output needs" in L.anoddpm_last_error()
    a.curve_pro = a.curve_thr = a.curve_len = p
    a.curve_cap = 0
    assert L.anoddpm_pro_auc_wide(ctypes.byref(a), 1024, None) == -1 and b"curve capacity" in L.anoddpm_last_error()


def test_wide_workspace_bytes():
    from anoddpm_amd import _lib
    L = _lib.lib()
    cap = _lib.ROC_WIDE_MAX_TILES
    for S, n, tile in ((0, 8, 0), (-1, 8, 0), (1, 0, 0), (1, -5, 0), (1, 1 << 31, 0), (1, 1000, 100), (1, 1000, 255), (1, 1000, 384 + 1),
                       (1, 1000, -256), (1, 256 * cap + 1, 256), (1, 1 << 22, 1024), (1, (1 << 31) - 1, 1 << 19)):
        assert L.anoddpm_pro_wide_workspace_bytes(S, n, tile) == -1, (S, n, tile)
    assert L.anoddpm_pro_wide_workspace_bytes(1, 256 * cap, 256) > 0 and L.anoddpm_pro_wide_workspace_bytes(1, (1 << 31) - 1, 1 << 20) > 0
    # the segments are processed one after another in ONE segment's workspace
    assert L.anoddpm_pro_wide_workspace_bytes(7, 5000, 256) == L.anoddpm_pro_wide_workspace_bytes(1, 5000, 256)
    # every n < 2^31 is accepted at the default tile, and a larger n never needs less -- also where the default tile grows
    ns = sorted({1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65536, 1 << 22, 5767168, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 23) + 4096,
                 9000000, 1 << 24, (1 << 24) + 1, 1 << 28, (1 << 31) - 2, (1 << 31) - 1} | set(range((1 << 23) - 3000, (1 << 23) + 9000, 500)))
    for tile in (0, 1 << 20):
        sizes = [L.anoddpm_pro_wide_workspace_bytes(1, n, tile) for n in ns]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:])), tile
        assert sizes[-1] > sizes[0]
    sizes = [L.anoddpm_pro_wide_workspace_bytes(1, n, 256) for n in range(1, 256 * cap, 4099)]
    assert all(s > 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:]))
    # the documented bound: 28 W + W / 4 bytes with W = n rounded up to 64, 1044 bytes per tile, less than 1 KB beside them
    for n, tile in ((1, 0), (5000, 256), (5000, 0), (1 << 22, 0), (1 << 22, 4096)):
        W, T = (n + 63) // 64 * 64, -(-n // (tile or 4096))
        size = L.anoddpm_pro_wide_workspace_bytes(1, n, tile)
        assert 28 * W <= size <= 28 * W + W // 4 + 1044 * ((T + 3) // 4 * 4) + 1024, (n, tile, size)


def test_python_surface_without_gpu():
    import evaluation
    from anoddpm_amd import metrics
    assert "PooledRegionCurves" in metrics.__all__ and evaluation.PooledRegionCurves is metrics.PooledRegionCurves
    assert issubclass(metrics.PooledRegionCurves, metrics.PooledCurves)
    assert isinstance(metrics.PRO_WIDE_MIN_N, int) and metrics.PRO_WIDE_MIN_N >= 1
    m, s = np.zeros((4, 4), np.float32), np.ones((4, 4), np.float32)
    with pytest.raises(TypeError, match="pooled"):
        metrics.AUPRO([m, m], [s, s])                                   # host arrays in a list: not a pooled device call
    with pytest.raises(TypeError, match="pooled"):
        metrics.AUPRO([m], s)
