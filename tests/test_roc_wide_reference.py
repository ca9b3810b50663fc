"""The chip-wide ROC / PR path without a device: the numpy restatement of the launch sequence of csrc/roc_wide.hip
(tests/roc_wide_cases.py) equals the restatements of the one-workgroup kernel (rc.roc_numpy, pc.pr_numpy) on every case at tiles
256 and 1024 -- integers and curves exactly, AP by pc.same_float -- each planted defect of that restatement is caught by the case
list, and the host side of the two new entry points: refusals before anything is launched, workspace sizes.  CPU only."""
import ctypes

import numpy as np
import pytest

import pr_cases as pc
import roc_cases as rc
import roc_wide_cases as wc


@pytest.fixture(scope="module")
def cases():
    return {name: wc.make_case(name) for name in wc.CPU_CASES}


@pytest.mark.parametrize("tile", wc.TILES)
@pytest.mark.parametrize("name", wc.CPU_CASES)
def test_restatement_equals_the_one_workgroup_restatements(cases, name, tile):
    mask, score = cases[name]
    assert wc.differences(mask, score, tile) == []


def test_cases_are_what_they_are_for(cases):
    # n = 1025 at tile 256: a last tile of one key; n = 63: one partial tile
    assert cases["n1025"][1].size == 1025 and cases["n63"][1].size == 63
    # a run that covers two whole tiles: tiles 1 and 2 of the sorted keys hold no run start
    key = np.sort(wc.keys_of(*cases["long_run"]))
    s = key >> np.uint32(1)
    bnd = np.r_[True, s[1:] != s[:-1]]
    assert not bnd[256:768].any() and bnd[:256].any() and bnd[768:].any()
    # every pass skips when all keys share every digit but the label bit ... which splits the first one: passes 1 to 3 skip
    w = wc.wide_numpy(*cases["all_equal_1024"], 256)
    assert w["skipped"] == [False, True, True, True] and w["R"] == 1
    assert wc.wide_numpy(np.zeros(1024, np.float32), cases["all_equal_1024"][1], 256)["skipped"] == [True] * 4
    # one tile of one digit in a pass where the segment has several: the pass is not skipped
    assert wc.wide_numpy(*cases["tile_digit"], 256)["skipped"][0] is False
    # tiles of runs: several at both tile sizes, with dropped points on both sides of their borders
    r = rc.roc_numpy(*cases["border_keep"])
    assert r["R"] == 2304 and r["fps"].size < 16
    assert wc.default_tile(1) == wc.default_tile(1 << 23) == 4096 and wc.default_tile((1 << 23) + 1) == 4352
    assert -(-((1 << 31) - 1) // wc.default_tile((1 << 31) - 1)) <= wc.MAX_TILES


CAUGHT_BY = {"scan_tile_major": ("ragged", 256), "reverse_rank": ("ragged", 1024), "tile_first_blind": ("long_run", 256),
             "keep_blind": ("border_keep", 1024), "ap_per_tile": ("continuous", 1024), "skip_from_tile": ("tile_digit", 256)}


@pytest.mark.parametrize("defect", wc.DEFECTS)
def test_planted_defect_is_caught(cases, defect):
    """The named (case, tile) exposes the defect; tile_digit and border_keep were constructed for theirs."""
    name, tile = CAUGHT_BY[defect]
    bad = wc.differences(*cases[name], tile, defect)
    print(defect, name, tile, bad)
    assert bad, f"{defect} passes {name} at tile {tile}"
    caught = [(n, t) for n in wc.CPU_CASES if n not in rc.MAPS for t in wc.TILES if wc.differences(*cases[n], t, defect)]
    print(defect, "caught by", caught)
    assert caught, f"{defect}: only a 256^2 map exposes it"


def test_wide_abi_refusals_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 34 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    assert L.anoddpm_roc_auc_wide.argtypes == [ctypes.POINTER(_lib.RocArgs), ctypes.c_int32, ctypes.c_void_p]
    assert L.anoddpm_roc_wide_workspace_bytes.restype is ctypes.c_int64
    assert L.anoddpm_roc_auc_wide(None, 0, None) == -1 and b"null args" in L.anoddpm_last_error()
    a = _lib.RocArgs()
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 0, None) == -1 and b"null pointer" in L.anoddpm_last_error()
    # host memory stands in for the device pointers: every case below is rejected before anything is launched
    buf = (ctypes.c_char * 128)()
    p = (ctypes.addressof(buf) + 15) & ~15
    a.score = a.mask = a.workspace = a.auc = a.counts = a.status = p
    a.S, a.n = 0, 16
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 0, None) == -1 and b"S must be" in L.anoddpm_last_error()
    a.S, a.n = 1, 0
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 0, None) == -1 and b"n must be >= 1" in L.anoddpm_last_error()
    a.n = 1 << 31
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 0, None) == -1 and b"2^31" in L.anoddpm_last_error()
    a.S, a.n, a.score_stride, a.mask_stride = 2, 16, 8, 0
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 0, None) == -1 and b"score_stride" in L.anoddpm_last_error()
    a.score_stride, a.mask_stride = 16, 8
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 0, None) == -1 and b"mask_stride" in L.anoddpm_last_error()
    a.mask_stride = 0
    a.workspace_bytes = 1 << 40
    for tile in (-256, 100, 255, 257, 1000):
        assert L.anoddpm_roc_auc_wide(ctypes.byref(a), tile, None) == -1 and b"multiple of 256" in L.anoddpm_last_error(), tile
    a.n = 256 * _lib.ROC_WIDE_MAX_TILES + 1
    a.score_stride = a.n
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 256, None) == -1 and b"tiles" in L.anoddpm_last_error()
    a.n = a.score_stride = 16
    for tile in (0, 256, 1024):
        a.workspace_bytes = L.anoddpm_roc_wide_workspace_bytes(2, 16, tile) - 1
        assert a.workspace_bytes > 0
        assert L.anoddpm_roc_auc_wide(ctypes.byref(a), tile, None) == -1 and b"workspace too small" in L.anoddpm_last_error()
    a.workspace_bytes += 1
    a.workspace = p + 4
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 1024, None) == -1 and b"aligned" in L.anoddpm_last_error()
    a.workspace = p
    a.curve_fps = p                                                     # some but not all of the curve outputs
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 1024, None) == -1 and b"curve output needs" in L.anoddpm_last_error()
    a.curve_tps = a.curve_thr = a.curve_len = p
    a.curve_cap = 1
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 1024, None) == -1 and b"curve capacity" in L.anoddpm_last_error()
    a.curve_cap, a.curve_mode = 16, 2
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 1024, None) == -1 and b"curve_mode" in L.anoddpm_last_error()
    a.curve_fps = a.curve_tps = a.curve_thr = a.curve_len = None
    a.curve_mode = _lib.ROC_CURVE_ALL
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 1024, None) == -1 and b"curve_mode needs" in L.anoddpm_last_error()
    a.curve_mode, a.best_dice = _lib.ROC_CURVE_DROP, p
    assert L.anoddpm_roc_auc_wide(ctypes.byref(a), 1024, None) == -1 and b"best Dice output needs" in L.anoddpm_last_error()


def test_wide_workspace_bytes():
    from anoddpm_amd import _lib
    L = _lib.lib()
    cap = _lib.ROC_WIDE_MAX_TILES
    assert cap == wc.MAX_TILES
    for S, n, tile in ((0, 8, 0), (-1, 8, 0), (1, 0, 0), (1, -5, 0), (1, 1 << 31, 0), (1, 1000, 100), (1, 1000, 255), (1, 1000, 384 + 1),
                       (1, 1000, -256), (1, 256 * cap + 1, 256), (1, 1 << 22, 1024), (1, (1 << 31) - 1, 1 << 19)):
        assert L.anoddpm_roc_wide_workspace_bytes(S, n, tile) == -1, (S, n, tile)
    assert L.anoddpm_roc_wide_workspace_bytes(1, 256 * cap, 256) > 0 and L.anoddpm_roc_wide_workspace_bytes(1, (1 << 31) - 1, 1 << 20) > 0
    # the segments are processed one after another in ONE segment's workspace
    assert L.anoddpm_roc_wide_workspace_bytes(7, 5000, 256) == L.anoddpm_roc_wide_workspace_bytes(1, 5000, 256)
    # every n < 2^31 is accepted at the default tile, and a larger n never needs less -- also where the default tile grows
    ns = sorted({1, 2, 63, 64, 255, 256, 257, 4095, 4096, 4097, 65536, 1 << 22, 5767168, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 23) + 4096,
                 9000000, 1 << 24, (1 << 24) + 1, 1 << 28, (1 << 31) - 2, (1 << 31) - 1} | set(range((1 << 23) - 3000, (1 << 23) + 9000, 500)))
    for tile in (0, 1 << 20):
        sizes = [L.anoddpm_roc_wide_workspace_bytes(1, n, tile) for n in ns]
        assert all(s > 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:])), tile
        assert sizes[-1] > sizes[0]
    sizes = [L.anoddpm_roc_wide_workspace_bytes(1, n, 256) for n in range(1, 256 * cap, 4099)]
    assert all(s > 0 for s in sizes) and all(b >= a for a, b in zip(sizes, sizes[1:]))
    # room for the keys, the run records with their sentinel and one fp64 term per run
    for n in (1, 5000, 1 << 22):
        assert L.anoddpm_roc_wide_workspace_bytes(1, n, 0) >= (3 * 4 + 8) * (n + 1)


def test_python_surface_without_gpu():
    import evaluation
    from anoddpm_amd import metrics
    assert "PooledCurves" in metrics.__all__ and evaluation.PooledCurves is metrics.PooledCurves
    assert isinstance(metrics.ROC_WIDE_MIN_N, int) and metrics.ROC_WIDE_MIN_N >= 1
    m, s = np.zeros(4, np.float32), np.ones(4, np.float32)
    for f in (metrics.ROC_AUC, metrics.PR_curve):
        with pytest.raises(TypeError, match="pooled"):
            f([m, m], [s, s])                                           # host arrays in a list: not a pooled device call
        with pytest.raises(TypeError, match="pooled"):
            f([m], s)
