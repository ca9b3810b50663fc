"""-m "not gpu": the numpy restatement of tests/gauss3d_cases.py -- what the device tests compare csrc/gauss3d.hip with -- against
scipy itself (when it is installed) and against the fixture tests/golden/gauss3d.npz (always); the six planted defects; the
cross-check with the plane filter's restatement; the host-side argument checks of `gaussian_filter3d`, the
`VolumePostProcess(gaussian=)` setting and what `anoddpm_gauss3d` refuses before any launch."""
import copy
import ctypes
import inspect
import os
import pickle

import numpy as np
import pytest

import gauss3d_cases as gc
import smooth_cases as sm
from conftest import GOLDEN

NAMES = sorted(gc.CASES)


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "gauss3d.npz"))


@pytest.fixture(scope="module")
def restated():
    """name -> gaussian3d_numpy of the case: computed once, shared, never written to."""
    out = {}
    for name, (_, sigma) in gc.CASES.items():
        out[name] = gc.gaussian3d_numpy(gc.make_case(name), sigma)
        out[name].setflags(write=False)
    return out


# ---------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_fixture(kat, restated, name):
    x = gc.make_case(name)
    assert x.dtype == np.float32 and x.shape == gc.CASES[name][0] and np.isfinite(x).all() and (x >= 0).all()
    assert gc.sha(x) == str(kat[name + "_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    assert (name + "_out" in kat.files) == (x.size <= gc.FULL_LIMIT)
    gc.check_fixture(kat, name, restated[name])


def test_restatement_equals_the_fixture_on_batches(kat):
    buf, vols = gc.make_strided()
    assert gc.sha(buf) == str(kat["strided_in_sha"])
    gc.check_fixture(kat, "strided", gc.gaussian3d_numpy(vols, gc.BATCH5[1]))
    b5 = gc.make_batch5()
    assert gc.sha(b5) == str(kat["batch5_in_sha"])
    gc.check_fixture(kat, "batch5", gc.gaussian3d_numpy(b5, gc.BATCH5[1]))
    bad = gc.make_poison()
    shape, sigma, v, where = gc.POISON
    assert gc.sha(bad) == str(kat["poison_in_sha"])
    clean = [j for j in range(shape[0]) if j != v]
    assert gc.sha(gc.gaussian3d_numpy(bad[clean], sigma)) == str(kat["poison_clean_out_sha"])
    got = gc.gaussian3d_numpy(bad[v], sigma)
    assert np.isnan(got).any() and not np.isnan(got).all()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_scipy(restated, name):
    ndimage = pytest.importorskip("scipy.ndimage")
    shape, sigma = gc.CASES[name]
    x = gc.make_case(name).reshape((-1,) + shape[-3:])
    want = np.stack([ndimage.gaussian_filter(v, gc.sigmas_of(sigma), truncate=gc.TRUNCATE) for v in x]).reshape(shape)
    assert want.dtype == np.float32 and want.tobytes() == restated[name].tobytes()


@pytest.mark.parametrize("sigma,truncate", gc.tables_used())
def test_tap_tables_equal_the_fixture(kat, sigma, truncate):
    w, r = sm.weights_numpy(sigma, truncate), gc.radius_of(sigma, truncate)
    assert 1 <= r <= gc.MAX_RADIUS and w.dtype == np.float64 and w.shape == (2 * r + 1,)
    assert w.tobytes() == kat[f"w_s{sigma}_t{truncate}"].tobytes()


def test_case_set_is_the_table_of_the_issue():
    want = {((1, 5, 7), (1, 1, 1)), ((3, 33, 65), (4, 4, 4)), ((33, 3, 5), (8, 0.4, 8)), ((9, 34, 31), (1, 4, 4)), ((4, 40, 70), (0, 2, 2)),
            ((70, 3, 5), (2, 0, 0)), ((5, 6, 40), (0.5, 3, 0)), ((2, 2, 2, 16, 16), (1.5, 1.5, 1.5))}
    assert {(shape, gc.sigmas_of(sigma)) for shape, sigma in gc.CASES.values()} == want
    radii = {name: tuple(gc.radius_of(s) for s in gc.sigmas_of(sigma)) for name, (_, sigma) in gc.CASES.items()}
    assert radii["rz32_tiny_plane"] == (32, 2, 32) and radii["z_skipped"] == (0, 8, 8) and radii["z_only"] == (8, 0, 0)
    assert radii["x_skipped"] == (2, 12, 0) and radii["d_below_rz"] == (16, 16, 16) and radii["anisotropic"] == (4, 16, 16)
    assert gc.CASES["d_below_rz"][0][0] < 16 and gc.CASES["rz32_tiny_plane"][0][0] > gc.TILE and gc.CASES["z_only"][0][0] > 2 * gc.TILE
    assert gc.radius_of(1e-16) == 0 and gc.radius_of(0.1) == 0 and gc.radius_of(0.13) == 1


@pytest.mark.parametrize("defect", gc.DEFECTS)
def test_planted_defect_changes_some_case(restated, defect):
    hit = [name for name, (_, sigma) in gc.CASES.items()
           if gc.gaussian3d_numpy(gc.make_case(name), sigma, defect=defect).tobytes() != restated[name].tobytes()]
    print(defect, hit)
    assert hit, f"no case notices the defect {defect!r}"


def test_z_skipped_equals_the_plane_filter_slice_by_slice(restated):
    x = gc.make_case("z_skipped")
    assert gc.CASES["z_skipped"][1] == (0.0, 2.0, 2.0)
    assert sm.gaussian_numpy(x, 2.0).tobytes() == restated["z_skipped"].tobytes()
    for d in range(x.shape[0]):
        assert sm.gaussian_numpy(x[d], 2.0).tobytes() == restated["z_skipped"][d].tobytes()


def test_a_spike_reaches_the_next_slice_only_under_the_volume_filter():
    x = np.zeros((5, 9, 9), np.float32)
    x[2, 4, 4] = 1.0
    vol, planes = gc.gaussian3d_numpy(x, 1.0), sm.gaussian_numpy(x, 1.0)
    assert abs(float(vol[1, 4, 4]) - 0.0385) < 5e-5 and planes[1, 4, 4] == 0.0


# ---------------------------------------------------------------------------------- host side
def test_sigma_and_radius_checks_of_the_host_wrapper():
    import torch
    from anoddpm_amd import _lib, metrics
    assert _lib.GAUSS_MAX_RADIUS == gc.MAX_RADIUS
    E = inspect.Parameter.empty
    assert [(k, v.default) for k, v in inspect.signature(metrics.gaussian_filter3d).parameters.items()] == \
        [("score", E), ("sigma", 4.0), ("truncate", 4.0), ("batched", None)]
    assert metrics._gauss3d_radii(4, 4.0, "t") == ((4.0, 4.0, 4.0), (16, 16, 16))
    assert metrics._gauss3d_radii((1, 4.0, 4), 4.0, "t") == ((1.0, 4.0, 4.0), (4, 16, 16))
    assert metrics._gauss3d_radii([8, 0.4, 0], 4.0, "t")[1] == (32, 2, 0)
    assert metrics._gauss3d_radii((1e-16, 0.1, 0.13), 4.0, "t")[1] == (0, 0, 1)
    assert metrics._gauss3d_radii(3.0, 3.0, "t")[1] == (9, 9, 9)
    for name, (_, sigma) in gc.CASES.items():
        assert metrics._gauss3d_radii(sigma, gc.TRUNCATE, "t")[1] == tuple(gc.radius_of(s) for s in gc.sigmas_of(sigma)), name
    x = torch.zeros(3, 4, 5)                                          # on the host: every refusal below comes before any device work
    for bad in (-1.0, float("nan"), float("inf"), True, "4", None, (1, 2), (1, 2, 3, 4), (1, -2, 3), (1, float("nan"), 1), (1, True, 1), 8.2,
                (1, 1, 8.2), ((1, 2, 3),)):
        with pytest.raises(ValueError, match="sigma"):
            metrics.gaussian_filter3d(x, bad)
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, "4"):
        with pytest.raises(ValueError, match="truncate"):
            metrics.gaussian_filter3d(x, 1.0, truncate=bad)
    with pytest.raises(ValueError, match="radius"):
        metrics.gaussian_filter3d(x, 4.0, truncate=9.0)
    with pytest.raises(ValueError, match=r"\[\.\.\., D, H, W\]"):
        metrics.gaussian_filter3d(torch.zeros(4, 5), 1.0)
    with pytest.raises(ValueError, match="as a batch"):
        metrics.gaussian_filter3d(x, 1.0, batched=True)
    with pytest.raises(TypeError):
        metrics.gaussian_filter3d(np.zeros((3, 4, 5), np.float32), 1.0)
    with pytest.raises(_lib.AnoddpmError):
        metrics.gaussian_filter3d(x, 1.0)                             # no CPU path
    # every axis skipped: what scipy returns, an fp32 copy; nothing is launched
    src = torch.arange(60, dtype=torch.float64).reshape(3, 4, 5)
    for sigma in (0, 0.0, (0, 0, 0), 0.1, (1e-16, 0.1, 0)):
        got = metrics.gaussian_filter3d(src, sigma)
        assert got.dtype == torch.float32 and got.shape == src.shape and got.is_contiguous() and got.data_ptr() != src.data_ptr()
        assert torch.equal(got, src.float())
    same = torch.ones(2, 2, 2)
    assert metrics.gaussian_filter3d(same, 0).data_ptr() != same.data_ptr()


def test_python_surface():
    import evaluation
    from anoddpm_amd import metrics
    assert "gaussian_filter3d" in metrics.__all__ and evaluation.gaussian_filter3d is metrics.gaussian_filter3d
    params = [(k, v.default) for k, v in inspect.signature(metrics.VolumePostProcess.__init__).parameters.items()]
    assert params[1:] == [("median", 5), ("erode", 3), ("roi_level", None), ("min_size", 7), ("connectivity", 1)]
    assert [k for k in inspect.signature(metrics.postprocess_volumes).parameters] == ["sqerr", "pp", "real", "roi"]


def test_volume_postprocess_gaussian_setting():
    from anoddpm_amd.metrics import VolumePostProcess
    pp = VolumePostProcess()
    assert pp.gaussian is None and pp == VolumePostProcess(gaussian=None) and hash(pp) == hash(VolumePostProcess(gaussian=None))
    # what the parent commit's object answers
    assert pp._key() == (5, 3, None, 7, 1) and hash(pp) == hash((5, 3, None, 7, 1))
    assert repr(pp) == "VolumePostProcess(median=5, erode=3, roi_level=None, min_size=7, connectivity=1)"
    assert pp.__reduce__() == (VolumePostProcess, (5, 3, None, 7, 1))
    off = VolumePostProcess(median=None, erode=0, min_size=0)
    assert off.__reduce__() == (VolumePostProcess, (None, 0, None, 0, 1)) and pickle.loads(pickle.dumps(off)) == off
    g = VolumePostProcess(gaussian=(1, 2, 2))
    assert g.gaussian == (1.0, 2.0, 2.0) and all(isinstance(s, float) for s in g.gaussian)
    assert g != pp and hash(g) != hash(pp) and g == VolumePostProcess(5, 3, gaussian=[1.0, 2, 2]) and g != VolumePostProcess(gaussian=(2, 2, 1))
    assert VolumePostProcess(gaussian=2) == VolumePostProcess(gaussian=(2, 2, 2)) and VolumePostProcess(gaussian=2).gaussian == (2.0, 2.0, 2.0)
    assert g._key() == (5, 3, None, 7, 1, (1.0, 2.0, 2.0)) and hash(g) == hash(VolumePostProcess(gaussian=(1, 2, 2)))
    assert repr(g).endswith("connectivity=1, gaussian=(1.0, 2.0, 2.0))") and eval(repr(g), {"VolumePostProcess": VolumePostProcess}) == g
    assert g.__reduce__() != pp.__reduce__()
    only = VolumePostProcess(median=None, erode=0, min_size=0, gaussian=(1.0, 4.0, 4.0))
    for obj in (g, only, VolumePostProcess(gaussian=(0, 2, 2))):
        back = pickle.loads(pickle.dumps(obj))
        assert back == obj and back.gaussian == obj.gaussian and hash(back) == hash(obj)
        deep = copy.deepcopy(obj)
        assert deep == obj and deep.gaussian == obj.gaussian
    with pytest.raises(TypeError):
        VolumePostProcess(5, 3, None, 7, 1, 2.0)                                       # keyword only: the positional order stays
    for bad in (-1.0, float("nan"), float("inf"), True, "4", (1, 2), (1, 2, 3, 4), (1, -1, 1), (1, 1, True), 8.2, (8.2, 1, 1)):
        with pytest.raises(ValueError, match="gaussian"):
            VolumePostProcess(gaussian=bad)
    with pytest.raises(AttributeError):
        g.gaussian = (2.0, 2.0, 2.0)
    with pytest.raises(AttributeError):
        del g.gaussian


# ---------------------------------------------------------------------------------- the library, without a device
def test_struct_size_entry_point_and_abi():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 43 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    assert _lib.Gauss3dArgs in _lib._STRUCTS and L.anoddpm_struct_size(b"anoddpm_gauss3d_args") == ctypes.sizeof(_lib.Gauss3dArgs)
    assert "anoddpm_gauss3d" in _lib.SYMBOLS
    assert [n for n, _ in _lib.Gauss3dArgs._fields_] == ["src", "dst", "tmp", "wz", "wy", "wx", "src_stride", "S", "D", "H", "W", "rz", "ry", "rx"]


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every call here is refused by the argument checks: nothing reaches the device (the pointers are made-up addresses)."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    vol = 4 * 8 * 8

    def call(**kw):
        a = _lib.Gauss3dArgs()
        a.src, a.dst, a.tmp, a.wz, a.wy, a.wx = 0x100000, 0x200000, 0x300000, 0x8000, 0x9000, 0xa000
        a.src_stride, a.S, a.D, a.H, a.W, a.rz, a.ry, a.rx = vol, 2, 4, 8, 8, 4, 16, 16
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.anoddpm_gauss3d(ctypes.byref(a), None)
        return rc, L.anoddpm_last_error().decode()

    span = 4 * 2 * vol                                                                 # bytes of the two volumes
    for kw, text in (({"rz": 0, "ry": 0, "rx": 0}, "all three radii"), ({"rz": 33}, "radius"), ({"ry": 33}, "radius"), ({"rx": 33}, "radius"),
                     ({"rz": -1}, "radius"), ({"rx": -1}, "radius"),
                     ({"S": 0}, "S, D, H, W"), ({"D": 0}, "S, D, H, W"), ({"H": 0}, "S, D, H, W"), ({"W": -1}, "S, D, H, W"),
                     ({"S": 1 << 7, "D": 1 << 8, "H": 256, "W": 256, "src_stride": 1 << 24}, "2^31"),
                     ({"S": 1, "D": 1 << 11, "H": 1 << 10, "W": 1 << 10}, "2^31"),
                     ({"S": 1, "D": 1 << 30, "H": 1 << 30, "W": 1 << 30}, "2^31"),
                     ({"src": None}, "null"), ({"dst": None}, "null"), ({"tmp": None}, "null"),
                     ({"wz": None}, "null"), ({"wy": None}, "null"), ({"wx": None}, "null"),
                     ({"src_stride": vol - 1}, "src_stride"),
                     ({"dst": 0x100000}, "dst overlaps src"), ({"dst": 0x100000 + span - 4}, "dst overlaps src"),
                     ({"dst": 0x100000 - span + 4}, "dst overlaps src"),
                     ({"tmp": 0x100000}, "tmp overlaps src"), ({"tmp": 0x100000 + span - 4}, "tmp overlaps src"),
                     ({"tmp": 0x200000}, "tmp overlaps dst"), ({"tmp": 0x200000 - span + 4}, "tmp overlaps dst"),
                     ({"rz": 0, "tmp": 0x100000}, "tmp overlaps src")):
        rc, msg = call(**kw)
        assert rc != 0 and text in msg and msg.startswith("gauss3d:"), (kw, rc, msg)
    assert L.anoddpm_gauss3d(None, None) != 0 and "null args" in L.anoddpm_last_error().decode()
