"""-m "not gpu": the numpy restatements of tests/smooth_cases.py -- what the device tests compare csrc/smooth.hip with -- against
scipy itself (when it is installed), against the fixture tests/golden/smooth_kat.npz (always) and, for the image scores, against
exact arithmetic; the six planted defects; the `PostProcess(gaussian=)` setting and the host-side argument checks."""
import copy
import math
import os
import pickle

import numpy as np
import pytest

import smooth_cases as sm
from conftest import GOLDEN

GAUSS_CASES = sorted(sm.GAUSS)


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "smooth_kat.npz"))


@pytest.fixture(scope="module")
def restated():
    """name -> gaussian_numpy of the case: computed once, shared, never written to."""
    out = {}
    for name, (_, sigma, truncate, _) in sm.GAUSS.items():
        out[name] = sm.gaussian_numpy(sm.make_gauss_case(name), sigma, truncate)
        out[name].setflags(write=False)
    return out


# ---------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize("name", GAUSS_CASES)
def test_restatement_equals_the_fixture(kat, restated, name):
    x = sm.make_gauss_case(name)
    assert x.dtype == np.float32 and x.shape == sm.GAUSS[name][0]
    assert sm.sha(x) == str(kat[name + "_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    sm.check_fixture(kat, name, restated[name])


def test_restatement_equals_the_fixture_on_batches(kat):
    buf, planes = sm.make_strided()
    assert sm.sha(buf) == str(kat["strided_in_sha"])
    sm.check_fixture(kat, "strided", sm.gaussian_numpy(planes, 4.0))
    batch = sm.make_batch()
    assert sm.sha(batch) == str(kat["batch_in_sha"])
    got = sm.gaussian_numpy(batch, 4.0)
    assert sm.sha(got) == str(kat["batch_out_sha"]) and [sm.sha(g) for g in got] == kat["batch_out_plane_sha"].tolist()
    bad = sm.make_poison()
    assert sm.sha(bad) == str(kat["poison_in_sha"])
    clean = [j for j in range(bad.shape[0]) if j != sm.POISON_PLANE]
    assert sm.gaussian_numpy(bad[clean], 4.0).tobytes() == kat["poison_clean_out"].tobytes()
    assert np.isnan(sm.gaussian_numpy(bad[sm.POISON_PLANE], 4.0)).any()


@pytest.mark.parametrize("name", GAUSS_CASES)
def test_restatement_equals_scipy(restated, name):
    ndimage = pytest.importorskip("scipy.ndimage")
    _, sigma, truncate, _ = sm.GAUSS[name]
    want = ndimage.gaussian_filter(sm.make_gauss_case(name), sigma, truncate=truncate)
    assert want.dtype == np.float32 and want.tobytes() == restated[name].tobytes()


def test_constant_plane_stays_constant(restated):
    assert (restated["g64x64_const"] == np.float32(0.7)).all()


def test_case_set_covers_what_the_issue_lists():
    shapes = {(shape, sigma, truncate) for shape, sigma, truncate, _ in sm.GAUSS.values()}
    for want in (((5, 7), 4.0, 4.0), ((3, 3), 4.0, 4.0), ((1, 40), 4.0, 4.0), ((40, 1), 4.0, 4.0), ((2, 2), 8.0, 4.0), ((37, 53), 4.0, 4.0),
                 ((sm.TILE, sm.TILE), 4.0, 4.0), ((sm.TILE + 1, sm.TILE + 1), 4.0, 4.0), ((9, 70), 8.0, 4.0), ((70, 9), 8.0, 4.0),
                 ((17, 33), 0.5, 4.0), ((20, 20), 3.0, 3.0), ((33, 20), 2.5, 4.0), ((256, 256), 4.0, 4.0)):
        assert want in shapes, want
    assert sm.radius_of(8.0) == sm.MAX_RADIUS == 32 and sm.radius_of(4.0) == 16


@pytest.mark.parametrize("sigma,truncate", sorted(sm.WEIGHTS))
def test_weights_equal_the_fixture_and_scipy(kat, sigma, truncate):
    w, r = sm.weights_numpy(sigma, truncate), sm.WEIGHTS[(sigma, truncate)]
    assert sm.radius_of(sigma, truncate) == r and w.dtype == np.float64 and w.shape == (2 * r + 1,)
    assert w.tobytes() == kat[f"w_s{sigma}_t{truncate}"].tobytes()
    assert w[:r].tobytes() == w[:r:-1].tobytes()                                     # symmetric bit for bit: r + 1 entries say it all
    filters = pytest.importorskip("scipy.ndimage._filters")
    assert w.tobytes() == filters._gaussian_kernel1d(sigma, 0, r).tobytes()


@pytest.mark.parametrize("defect", sm.DEFECTS)
def test_planted_defect_changes_some_case(restated, defect):
    hit = [name for name, (_, sigma, truncate, _) in sm.GAUSS.items()
           if sm.gaussian_numpy(sm.make_gauss_case(name), sigma, truncate, defect=defect).tobytes() != restated[name].tobytes()]
    print(defect, hit)
    assert hit, f"no case notices the defect {defect!r}"


# ---------------------------------------------------------------------------------- the image scores
def exact_scores(x, k):
    """(max, mean, top-k mean) with correctly rounded sums: math.fsum over the sorted values."""
    v = np.sort(np.abs(np.asarray(x, np.float32).reshape(-1)).astype(np.float64))[::-1]
    return np.float32(v[0]), math.fsum(v) / v.size, math.fsum(v[:k]) / k


@pytest.mark.parametrize("name", sorted(sm.SCORES))
def test_scores_restatement_against_exact_arithmetic(name):
    x, k = sm.make_score_case(name)
    n = x.size
    mx, mean, topk = sm.scores_numpy(x, k)
    emx, emean, etopk = exact_scores(x, k)
    print(name, n, k, mx, mean, emean, topk, etopk)
    assert np.float32(mx).tobytes() == emx.tobytes() and not np.signbit(mx)
    assert sm.within(mean, emean, n) and sm.within(topk, etopk, k)
    if k == 1:
        assert topk == float(mx)
    if k == n:
        assert sm.within(topk, emean, n)


def test_score_cases_are_what_their_names_say():
    x, k = sm.make_score_case("tie_at_k")
    v = np.sort(x.reshape(-1))[::-1]
    assert v[k - 1] == v[k] and int((v > v[k - 1]).sum()) == 2
    x, _ = sm.make_score_case("negzero_denormal")
    tiny = np.finfo(np.float32).tiny
    assert np.signbit(x[x == 0]).any() and ((x > 0) & (x < tiny)).any() and (x >= 0).all()
    assert sm.k_of(0.01, 50) == 1 and sm.k_of(0.01, 256 * 256) == 655 and sm.k_of(7, 50) == 7 and sm.k_of(1.0, 50) == 50
    bad, which = sm.make_bad_segments()
    assert np.isnan(bad[1]).any() and np.isinf(bad[3]).any() and (bad[4] < 0).any() and sorted(which) == [1, 3, 4]
    assert all(np.isfinite(bad[j]).all() and (bad[j] >= 0).all() for j in (0, 2, 5))


def test_tree_sum_is_the_stated_order():
    rng = np.random.default_rng(5)
    v = rng.random(3000)
    partial = [0.0] * sm.THREADS
    for i, t in enumerate(v.tolist()):
        partial[i % sm.THREADS] += t                                                  # thread t adds t, t + 1024, ... in that order
    waves = []
    for wv in range(sm.THREADS // sm.WAVE):
        p = partial[wv * sm.WAVE:(wv + 1) * sm.WAVE]
        off = sm.WAVE // 2
        while off:
            p = [p[i] + p[i + off] for i in range(off)]
            off //= 2
        waves.append(p[0])
    off = len(waves) // 2
    while off:
        waves = [waves[i] + waves[i + off] for i in range(off)]
        off //= 2
    assert sm.tree_sum(v) == waves[0]


# ---------------------------------------------------------------------------------- host side
def test_postprocess_gaussian_setting():
    from anoddpm_amd.metrics import PostProcess
    pp = PostProcess()
    assert pp.gaussian is None and pp == PostProcess(gaussian=None) and hash(pp) == hash(PostProcess(gaussian=None))
    assert "gaussian" not in repr(pp) and repr(pp) == "PostProcess(median=5, erode=3, roi_level=None, min_size=7, connectivity=1)"
    assert pp.__reduce__() == (PostProcess, (5, 3, None, 7, 1))
    g = PostProcess(gaussian=4)
    assert g.gaussian == 4.0 and isinstance(g.gaussian, float) and g != pp and g == PostProcess(5, 3, gaussian=4.0)
    assert hash(g) == hash(PostProcess(gaussian=4.0)) and g != PostProcess(gaussian=2.0)
    assert repr(g).endswith("connectivity=1, gaussian=4.0)") and eval(repr(g), {"PostProcess": PostProcess}) == g
    texture = PostProcess(median=None, erode=0, min_size=0, gaussian=4.0)
    for obj in (g, texture):
        back = pickle.loads(pickle.dumps(obj))
        assert back == obj and back.gaussian == obj.gaussian and copy.deepcopy(obj) == obj
    with pytest.raises(TypeError):
        PostProcess(5, 3, None, 7, 1, 4.0)                                            # keyword only: the positional order stays
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 0.1, 8.2, "4", True):     # radius 0 at 0.1, 33 at 8.2
        with pytest.raises(ValueError, match="gaussian"):
            PostProcess(gaussian=bad)
    with pytest.raises(AttributeError):
        g.gaussian = 2.0


def test_radius_check_of_the_host_wrapper():
    from anoddpm_amd import _lib
    from anoddpm_amd.metrics import _gauss_radius
    assert _lib.GAUSS_MAX_RADIUS == sm.MAX_RADIUS and _lib.MAP_SCORES_MAX_N == sm.MAX_N and _lib.ABI_VERSION >= 33
    for (sigma, truncate), r in sm.WEIGHTS.items():
        assert _gauss_radius(sigma, truncate, "t") == r
    assert _gauss_radius(4, 4, "t") == 16
    for sigma, truncate in ((0.0, 4.0), (-4.0, 4.0), (float("nan"), 4.0), (float("inf"), 4.0), (0.1, 4.0), (8.2, 4.0), (4.0, 0.0), (4.0, -1.0),
                            (4.0, float("nan")), (4.0, 9.0), ("4", 4.0), (None, 4.0)):
        with pytest.raises(ValueError, match="radius"):
            _gauss_radius(sigma, truncate, "t")


def test_struct_sizes_and_entry_points():
    import ctypes
    from anoddpm_amd import _lib
    L = _lib.lib()
    for name, st in (("gauss", _lib.GaussArgs), ("map_scores", _lib.MapScoresArgs)):
        assert st in _lib._STRUCTS and L.anoddpm_struct_size(b"anoddpm_%s_args" % name.encode()) == ctypes.sizeof(st)
    assert "anoddpm_gauss2d" in _lib.SYMBOLS and "anoddpm_map_scores" in _lib.SYMBOLS
    assert [n for n, _ in _lib.GaussArgs._fields_] == ["src", "dst", "w", "src_stride", "S", "H", "W", "radius"]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call here is refused by the argument checks: nothing reaches the device (the pointers are made-up addresses)."""
    import ctypes
    from anoddpm_amd import _lib
    L = _lib.lib()

    def gauss(**kw):
        a = _lib.GaussArgs()
        a.src, a.dst, a.w, a.src_stride, a.S, a.H, a.W, a.radius = 0x10000, 0x90000, 0x8000, 64, 2, 8, 8, 16
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.anoddpm_gauss2d(ctypes.byref(a), None)
        return rc, L.anoddpm_last_error().decode()

    for kw, text in (({"radius": 0}, "radius"), ({"radius": 33}, "radius"), ({"S": 0}, "S, H, W"), ({"H": 0}, "S, H, W"), ({"W": -1}, "S, H, W"),
                     ({"src": None}, "null"), ({"dst": None}, "null"), ({"w": None}, "null"), ({"dst": 0x10000}, "overlaps"),
                     ({"dst": 0x10000 + 4 * 100}, "overlaps"), ({"dst": 0x10000 - 4 * 100}, "overlaps"), ({"src_stride": 63}, "src_stride")):
        rc, msg = gauss(**kw)
        assert rc != 0 and text in msg, (kw, rc, msg)
    assert L.anoddpm_gauss2d(None, None) != 0

    def scores(**kw):
        a = _lib.MapScoresArgs()
        a.src, a.max, a.mean, a.topk_mean, a.status = 0x10000, 0x90000, 0x91000, 0x92000, 0x93000
        a.src_stride, a.n, a.k, a.S = 100, 100, 3, 2
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.anoddpm_map_scores(ctypes.byref(a), None)
        return rc, L.anoddpm_last_error().decode()

    for kw, text in (({"n": 0}, "n must"), ({"n": sm.MAX_N + 1, "src_stride": sm.MAX_N + 1}, "n must"), ({"k": 0}, "k must"), ({"k": 101}, "k must"),
                     ({"S": 0}, "S must"), ({"src_stride": 99}, "src_stride"), ({"src": None}, "null"), ({"max": None}, "null"),
                     ({"mean": None}, "null"), ({"topk_mean": None}, "null"), ({"status": None}, "null")):
        rc, msg = scores(**kw)
        assert rc != 0 and text in msg, (kw, rc, msg)
    assert L.anoddpm_map_scores(None, None) != 0
