"""Post-processing without a device: the plain-numpy restatements of tests/postproc_cases.py (symmetric pad + sort; L1 ball over a
zero pad; a host union-find) reproduce the fixture tests/golden/postproc_kat.npz -- what scipy.ndimage's median_filter,
binary_erosion and label + bincount return -- bit for bit, every case; where scipy imports they are also compared live.  And
the host-side pieces of the native path: argument validation of anoddpm_median2d / anoddpm_erode2d / anoddpm_small_components
through the ABI, the workspace-size function, the signatures of the metrics functions, PostProcess.  CPU only."""
import copy
import ctypes
import inspect
import os
import pickle

import numpy as np
import pytest

import postproc_cases as pc
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "postproc_kat.npz")
MEDIAN_CASES = [(name, k) for name in sorted(pc.MEDIAN) for k in pc.WINDOWS]
ERODE_CASES = [(name, n) for name in sorted(pc.ERODE) for n in pc.ERODE_N]
COMPONENT_CASES = [(name, c) for name in sorted(pc.COMPONENTS) for c in (1, 2)]


@pytest.fixture(scope="module")
def kat():
    return np.load(FIXTURE)


def _scipy():
    try:
        from scipy import ndimage
        return ndimage
    except ImportError:
        return None


@pytest.mark.parametrize("name,k", MEDIAN_CASES)
def test_median_restatement_reproduces_fixture(kat, name, k):
    x = pc.make_median_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: the regenerated input differs from the one the fixture was made from"
    got = pc.median_numpy(x, k)
    pc.check_plane(kat, pc.mkey(name, k), got, name in pc.MEDIAN_FULL)
    nd = _scipy()
    if nd is not None:
        assert got.tobytes() == nd.median_filter(x, size=k).tobytes()


def test_median_cases_have_ties_and_zeros():
    for name in ("m25x41", "m256"):
        x = pc.make_median_case(name)
        assert len(np.unique(x)) <= 64 and (x == 0).mean() > 0.05 and (x * 64 == np.floor(x * 64)).all(), name
    assert (pc.make_median_case("m8x300") == 0).any()


def test_strided_and_batch_reproduce_fixture(kat):
    buf, planes = pc.make_strided()
    assert pc.sha(buf) == str(kat["strided_in_sha"]) and not planes.flags["C_CONTIGUOUS"] and np.shares_memory(buf, planes)
    for k in pc.WINDOWS:
        pc.check_plane(kat, pc.mkey("strided", k), pc.median_numpy(planes, k), True)
    maps, roi = pc.make_batch()
    assert pc.sha(maps, roi) == str(kat["batch_in_sha"]) and maps.shape == (pc.BATCH, 1, 256, 256)
    assert set(np.unique(roi)) == {0.0, 1.0} and 0.3 < roi.mean() < 0.7
    got = pc.median_numpy(maps, 5) * roi
    assert pc.sha(got) == str(kat["batch_k5_sha"])
    assert [pc.sha(g) for g in got] == [str(s) for s in kat["batch_k5_plane_sha"]]
    assert (got[:, 0][:, roi == 0] == 0).all() and not np.signbit(got).any()
    for j in (0, 27, 54):
        for cname, sl in pc.crops(256, 256).items():
            assert got[j, 0][sl].tobytes() == kat[f"batch_k5_{j}_{cname}"].tobytes()


def test_bad_batch_clean_planes(kat):
    bad = pc.make_bad_batch()
    assert pc.sha(bad) == str(kat["bad_in_sha"])
    assert np.isnan(bad[1]).sum() == 1 and np.isinf(bad[3]).sum() == 1 and (bad[4] < 0).sum() == 1
    clean = [j for j in range(bad.shape[0]) if j not in pc.BAD_PLANES]
    assert clean == [0, 2, 5] and np.isfinite(bad[clean]).all() and (bad[clean] >= 0).all()
    assert pc.median_numpy(bad[clean], 5).tobytes() == kat["bad_k5_clean"].tobytes()


@pytest.mark.parametrize("name,n", ERODE_CASES)
def test_erosion_restatement_reproduces_fixture(kat, name, n):
    x, level = pc.make_erode_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    b = x > np.float32(level)
    assert b[0].any() and b[-1].any() and b[:, 0].any() and b[:, -1].any()            # the mask touches every border
    got = pc.erode_numpy(x, n, level)
    want = np.unpackbits(kat[pc.ekey(name, n) + "_bits"])[:x.size].reshape(x.shape).astype(np.float32)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), f"{int((got != want).sum())} pixels differ"
    assert pc.sha(got) == str(kat[pc.ekey(name, n) + "_sha"]) and int(got.sum()) == int(kat[pc.ekey(name, n) + "_sum"])
    assert not got[0].any() and not got[:, -1].any()                                   # zero outside: the border always goes
    nd = _scipy()
    if nd is not None:
        assert got.tobytes() == nd.binary_erosion(b, iterations=n).astype(np.float32).tobytes()


def test_erosion_special_values(kat):
    x, level = pc.make_erode_case("e7x7")
    want = np.zeros((7, 7), np.float32)
    want[3, 3] = 1
    assert pc.erode_numpy(x, 3, level).tobytes() == want.tobytes() and not pc.erode_numpy(x, 8, level).any()
    x, level = pc.make_erode_case("e64")
    assert level == 0.25 and (x == np.float32(0.25)).any() and not (x < np.float32(0.25)).any()    # AT the level is not above it


@pytest.mark.parametrize("name,connectivity", COMPONENT_CASES)
def test_components_restatement_reproduces_fixture(kat, name, connectivity):
    x = pc.make_components_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    lab = pc.labels_numpy(x > 0, connectivity)
    nd = _scipy()
    for m in pc.COMPONENTS[name]:
        key = pc.ckey(name, connectivity, m)
        got, counts = pc.components_numpy(x, m, connectivity, labels=lab)
        assert counts == tuple(int(v) for v in kat[key + "_counts"]), key
        assert got.dtype == np.float32 and pc.sha(got) == str(kat[key + "_sha"]), key
        if name in pc.COMPONENTS_FULL:
            want = np.unpackbits(kat[key + "_bits"])[:x.size].reshape(x.shape).astype(np.float32)
            assert got.tobytes() == want.tobytes()
        if nd is not None:
            sl, found = nd.label(x > 0, structure=nd.generate_binary_structure(2, connectivity))
            keep = np.bincount(sl.ravel(), minlength=found + 1) >= m
            keep[0] = False
            assert got.tobytes() == keep[sl].astype(np.float32).tobytes() and counts == (found, int(keep.sum()))


def test_component_special_values(kat):
    assert tuple(kat["empty_c1_m1_counts"]) == (0, 0) and tuple(kat["full_c2_m65537_counts"]) == (1, 0)
    assert tuple(kat["checker_c1_m1_counts"]) == (2048, 2048) and tuple(kat["checker_c1_m2_counts"]) == (2048, 0)
    assert tuple(kat["checker_c2_m7_counts"]) == (1, 1) and tuple(kat["checker_c2_m2049_counts"]) == (1, 0)
    s = pc.make_components_case("spiral")
    assert tuple(kat["spiral_c1_m7_counts"]) == (1, 1) and int(s.sum()) > 30000 and tuple(kat["spiral_c1_m40000_counts"]) == (1, 0)
    for name in ("blobs", "blobs40x56"):
        x = pc.make_components_case(name)
        big = max(pc.COMPONENTS[name])
        found, kept = (int(v) for v in kat[pc.ckey(name, 1, 7) + "_counts"])
        assert 0 < kept < found, name                                               # min_size 7 removes some, keeps some
        assert pc.components_numpy(x, 1, 1)[0].tobytes() == x.tobytes()             # min_size 1 keeps everything
    assert tuple(kat["blobs_c1_m5000_counts"])[1] == 0 and tuple(kat["blobs_c2_m5000_counts"])[1] == 0 and big >= 100


def test_fixture_says_how_it_was_produced(kat):
    text = str(kat["produced_with"])
    assert "scipy" in text and "median_filter" in text and "binary_erosion" in text and "label" in text
    assert os.path.getsize(FIXTURE) < 108 * 1024


# ---------------------------------------------------------------------------------- the ABI without a GPU
def _host_pointer():
    buf = (ctypes.c_char * 64)()
    return buf, ctypes.addressof(buf)


def _rejecter(fn, args, defaults):
    from anoddpm_amd import _lib
    L = _lib.lib()

    def rejected(text, **kw):
        vals = dict(defaults)
        vals.update(kw)
        for k, v in vals.items():
            setattr(args, k, v)
        assert fn(ctypes.byref(args), None) == -1, text
        assert text in L.anoddpm_last_error(), (text, L.anoddpm_last_error())
    return rejected


def test_struct_sizes_and_version():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 28
    assert L.anoddpm_abi_version() == _lib.ABI_VERSION
    for name, st in (("median", _lib.MedianArgs), ("erode", _lib.ErodeArgs), ("components", _lib.ComponentsArgs), ("ssim", _lib.SsimArgs)):
        assert st in _lib._STRUCTS and L.anoddpm_struct_size(b"anoddpm_%s_args" % name.encode()) == ctypes.sizeof(st)


def test_median_abi_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_median2d(None, None) == -1 and b"median2d: null args" in L.anoddpm_last_error()
    a = _lib.MedianArgs()
    assert L.anoddpm_median2d(ctypes.byref(a), None) == -1 and b"median2d: null pointer" in L.anoddpm_last_error()
    # host memory stands in for the device pointers: every case below is rejected before anything is launched
    buf, p = _host_pointer()
    a.src = a.dst = a.status = a.roi = p
    rejected = _rejecter(L.anoddpm_median2d, a, dict(S=2, H=32, W=32, k=5, src_stride=1024, roi_stride=0))
    rejected(b"S, H, W must be", S=0)
    rejected(b"S, H, W must be", H=0)
    rejected(b"S, H, W must be", W=-4)
    rejected(b"S, H, W must be", S=1 << 30, H=256, W=256)
    for k in (0, 1, 2, 4, 6, 8, 9, -3):
        rejected(b"k must be 3, 5 or 7", k=k)
    rejected(b"k exceeds the plane", H=4)
    rejected(b"k exceeds the plane", W=6, k=7)
    rejected(b"planes overlap", src_stride=1023)
    rejected(b"roi_stride must be 0", roi_stride=512)
    a.status = None
    rejected(b"null pointer")


def test_erode_abi_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_erode2d(None, None) == -1 and b"erode2d: null args" in L.anoddpm_last_error()
    a = _lib.ErodeArgs()
    assert L.anoddpm_erode2d(ctypes.byref(a), None) == -1 and b"erode2d: null pointer" in L.anoddpm_last_error()
    buf, p = _host_pointer()
    a.src = a.dst = p
    rejected = _rejecter(L.anoddpm_erode2d, a, dict(S=2, H=16, W=16, n=3, src_stride=256, level=0.0))
    rejected(b"S, H, W must be", S=0)
    rejected(b"S, H, W must be", H=-1)
    rejected(b"S, H, W must be", W=0)
    for n in (0, 9, -1, 100):
        rejected(b"n must be in 1 ... 8", n=n)
    rejected(b"planes overlap", src_stride=255)


def test_small_components_abi_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_small_components(None, None) == -1 and b"small_components: null args" in L.anoddpm_last_error()
    a = _lib.ComponentsArgs()
    assert L.anoddpm_small_components(ctypes.byref(a), None) == -1 and b"small_components: null pointer" in L.anoddpm_last_error()
    buf, p = _host_pointer()
    a.src = a.dst = a.counts = a.workspace = p
    need = L.anoddpm_small_components_workspace_bytes(2, 16, 16)
    rejected = _rejecter(L.anoddpm_small_components, a, dict(S=2, H=16, W=16, min_size=7, connectivity=1, src_stride=256, level=0.0,
                                                              workspace_bytes=need))
    rejected(b"S, H, W must be", S=0)
    rejected(b"S, H, W must be", H=0)
    rejected(b"S, H, W must be", S=1 << 15, H=256, W=256)
    rejected(b"min_size must be", min_size=-1)
    for c in (0, 3, -1):
        rejected(b"connectivity must be", connectivity=c)
    rejected(b"planes overlap", src_stride=255)
    rejected(b"workspace too small", workspace_bytes=need - 1)
    rejected(b"workspace too small", workspace_bytes=0)


def test_small_components_workspace_bytes():
    from anoddpm_amd import _lib
    L = _lib.lib()
    for S, H, W in ((1, 1, 1), (1, 7, 7), (55, 256, 256), (48, 512, 512), (1, 8, 300), (1, 32767, 65536)):
        assert L.anoddpm_small_components_workspace_bytes(S, H, W) == 8 * S * H * W
    for S, H, W in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -3), (1 << 15, 256, 256), (1, 32768, 65536), (2, 32768, 32768)):
        assert L.anoddpm_small_components_workspace_bytes(S, H, W) == -1


# ---------------------------------------------------------------------------------- the Python surface
def test_python_surface():
    import evaluation
    from anoddpm_amd import metrics

    def params(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert params(metrics.median_filter) == [("score", E), ("size", 5), ("roi", None), ("batched", None), ("return_status", False)]
    assert params(metrics.erode_mask) == [("x", E), ("iterations", 3), ("level", 0.0)]
    assert params(metrics.remove_small_components) == [("pred", E), ("min_size", 7), ("connectivity", 1), ("return_counts", False)]
    assert params(metrics.PostProcess.__init__)[1:] == [("median", 5), ("erode", 3), ("roi_level", None), ("min_size", 7), ("connectivity", 1)]
    assert params(metrics.postprocess_maps) == [("sqerr", E), ("pp", E), ("real", None), ("roi", None)]
    assert params(metrics.anomaly_metrics) == [("real", E), ("recon", E), ("mask", E), ("threshold", 0.5), ("postprocess", None), ("roi", None)]
    for name in ("median_filter", "erode_mask", "remove_small_components", "PostProcess", "postprocess_maps"):
        assert name in metrics.__all__ and getattr(evaluation, name) is getattr(metrics, name), name
    assert evaluation.median_filter is metrics.median_filter


def test_postprocess_settings_object():
    from anoddpm_amd.metrics import PostProcess
    pp = PostProcess()
    assert (pp.median, pp.erode, pp.roi_level, pp.min_size, pp.connectivity) == (5, 3, None, 7, 1)
    off = PostProcess(median=None, erode=0, min_size=0)
    assert off.median is None and off.erode == 0 and off.min_size == 0
    assert PostProcess(3, 8, -0.95, 20, 2).roi_level == -0.95
    for bad in (4, 6, 1, 9, 0, 5.5, "5"):
        with pytest.raises(ValueError, match="median"):
            PostProcess(median=bad)
    for bad in (-1, 9, 2.5):
        with pytest.raises(ValueError, match="erode"):
            PostProcess(erode=bad)
    for bad in (-1, -7, 1.5):
        with pytest.raises(ValueError, match="min_size"):
            PostProcess(min_size=bad)
    for bad in (0, 3, 4, -1):
        with pytest.raises(ValueError, match="connectivity"):
            PostProcess(connectivity=bad)
    with pytest.raises(AttributeError):
        pp.median = 3
    with pytest.raises(AttributeError):
        del pp.erode
    assert pp == PostProcess(5, 3) and pp != off and hash(pp) == hash(PostProcess()) and "median=5" in repr(pp)
    assert pickle.loads(pickle.dumps(off)) == off and copy.deepcopy(pp) == pp


def test_diffusion_model_attributes_are_plain():
    import GaussianDiffusion as GD
    from anoddpm_amd.metrics import PostProcess
    d = GD.GaussianDiffusionModel([32, 32], GD.get_beta_schedule(100, "linear"), noise="gauss")
    assert d.postprocess is None and d.postprocess_roi is None
    assert "postprocess" not in d.__getstate__()                         # unset: nothing new in the state
    d.postprocess = PostProcess(3, 1, -0.9)
    d.noise_fn = d._default_noise_fn = None                              # the lambdas of __init__ do not pickle (nor do upstream's)
    for other in (copy.deepcopy(d), pickle.loads(pickle.dumps(d))):
        assert other.postprocess == d.postprocess and other.postprocess_roi is None


def test_host_arguments_are_refused():
    """No CPU path: host tensors raise instead of computing somewhere else."""
    import torch
    from anoddpm_amd import _lib, metrics
    x = torch.zeros(1, 16, 16)
    with pytest.raises(_lib.AnoddpmError):
        metrics.median_filter(x)
    with pytest.raises(_lib.AnoddpmError):
        metrics.erode_mask(x)
    with pytest.raises(_lib.AnoddpmError):
        metrics.remove_small_components(x)
    with pytest.raises(ValueError, match="size"):
        metrics.median_filter(x, size=4)
    with pytest.raises(ValueError, match="window"):
        metrics.median_filter(torch.zeros(4, 16), size=5)
    with pytest.raises(ValueError, match="iterations"):
        metrics.erode_mask(x, iterations=0)
    with pytest.raises(ValueError, match="connectivity"):
        metrics.remove_small_components(x, connectivity=3)
    with pytest.raises(TypeError):
        metrics.postprocess_maps(x, None)
