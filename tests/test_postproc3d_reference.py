"""Volume post-processing without a device: the plain-numpy restatements of tests/postproc3d_cases.py (symmetric pad on three axes +
sort; octahedron over a zero pad; a host union-find over the forward neighbours) reproduce the fixture
tests/golden/postproc3d_kat.npz -- what scipy.ndimage's median_filter, binary_erosion and label + bincount return on volumes --
bit for bit, every case; where scipy imports they are also compared live.  Planted defects in the restatements each break a
case, so the cases can tell a volume result from its look-alikes.  And the host-side pieces of the native path: argument
validation of the four entry points through the ABI, the workspace-size function, the Python surface.  CPU only."""
import copy
import ctypes
import inspect
import os
import pickle

import numpy as np
import pytest

import postproc3d_cases as pc
import postproc_cases as pc2
from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "postproc3d_kat.npz")
MEDIAN_CASES = [(name, k) for name in sorted(pc.MEDIAN) for k in pc.WINDOWS]
ERODE_CASES = [(name, n) for name in sorted(pc.ERODE) for n in pc.ERODE_N]
COMPONENT_CASES = [(name, c) for name in sorted(pc.COMPONENTS) for c in pc.CONNECTIVITY]


@pytest.fixture(scope="module")
def kat():
    return np.load(FIXTURE)


def _scipy():
    try:
        from scipy import ndimage
        return ndimage
    except ImportError:
        return None


# ---------------------------------------------------------------------------------- restatements against the fixture
@pytest.mark.parametrize("name,k", MEDIAN_CASES)
def test_median_restatement_reproduces_fixture(kat, name, k):
    x = pc.make_median_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: the regenerated input differs from the one the fixture was made from"
    got = pc.median3d_numpy(x, k)
    pc.check_volume(kat, pc.mkey(name, k), got, name in pc.MEDIAN_FULL)
    nd = _scipy()
    if nd is not None:
        assert got.tobytes() == nd.median_filter(x, size=k).tobytes()


def test_median_cases_are_what_they_claim():
    x = pc.make_median_case("m9x40x70")
    assert len(np.unique(x)) <= 64 and (x == 0).mean() > 0.02 and (x * 64 == np.floor(x * 64)).all()
    assert pc.make_median_case("m1x7x9").shape[0] == 1 and pc.make_median_case("m2x5x5").shape[1:] == (5, 5)
    # a volume result is not the stack of its slices' results
    y = pc.make_median_case("m6x20x37")
    assert not np.array_equal(pc.median3d_numpy(y, 3), np.stack([pc2.median_numpy(s, 3) for s in y]))


def test_batch_and_bad_volumes_reproduce_fixture(kat):
    buf, vols, plane, roi_vol, roi_batch = pc.make_batch()
    assert pc.sha(buf, plane, roi_vol, roi_batch) == str(kat["batch_in_sha"])
    assert not vols.flags["C_CONTIGUOUS"] and np.shares_memory(buf, vols) and vols.shape == pc.BATCH_SHAPE
    for roi in (plane, roi_vol, roi_batch):
        assert set(np.unique(roi)) == {0.0, 1.0}
    for k in pc.WINDOWS:
        got = pc.median3d_numpy(vols, k)
        assert pc.sha(got) == str(kat[f"batch_k{k}_sha"])
        assert [pc.sha(g) for g in got] == [str(s) for s in kat[f"batch_k{k}_volume_sha"]]
    bad = pc.make_bad_batch()
    assert pc.sha(bad) == str(kat["bad_in_sha"]) and bad.shape == pc.BAD_SHAPE
    assert np.isnan(bad[0]).sum() == 1 and np.isinf(bad[1]).sum() == 1 and (bad[2] < 0).sum() == 1
    assert np.isfinite(bad[3]).all() and (bad[3] >= 0).all() and np.isfinite(bad[2]).all() and (bad[:2][np.isfinite(bad[:2])] >= 0).all()
    for k in pc.WINDOWS:
        assert pc.median3d_numpy(bad[3], k).tobytes() == kat[f"bad_k{k}_clean"].tobytes()


@pytest.mark.parametrize("name,n", ERODE_CASES)
def test_erosion_restatement_reproduces_fixture(kat, name, n):
    x, level = pc.make_erode_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    got = pc.erode3d_numpy(x, n, level)
    key = pc.ekey(name, n)
    want = pc.unpack(kat, key, x.shape)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), f"{int((got != want).sum())} voxels differ"
    assert pc.sha(got) == str(kat[key + "_sha"]) and int(got.sum()) == int(kat[key + "_sum"])
    assert (not got.any()) == ((name, n) in pc.ERODE_EMPTY) and not got.all()
    nd = _scipy()
    if nd is not None:
        assert got.tobytes() == nd.binary_erosion(x > np.float32(level), iterations=n).astype(np.float32).tobytes()


def test_erosion_special_values(kat):
    assert int(kat["ones19x21x40_n8_sum"]) == 3 * 5 * 24
    got = pc.unpack(kat, "ones19x21x40_n8", (19, 21, 40))
    assert got[8:11, 8:13, 8:32].all() and int(got.sum()) == got[8:11, 8:13, 8:32].size
    x, level = pc.make_erode_case("holes9x24x40")
    assert level == 0.25 and (x == np.float32(0.25)).any() and not (x < np.float32(0.25)).any()    # AT the level is not above it
    y = x.copy()
    y[4, 12, 20] = np.nan                                                                          # NaN is above no level
    assert pc.erode3d_numpy(y, 1, level)[4, 12, 20] == 0 and pc.erode3d_numpy(y, 1, level)[4, 12, 21] == 0


@pytest.mark.parametrize("name,connectivity", COMPONENT_CASES)
def test_components_restatement_reproduces_fixture(kat, name, connectivity):
    x = pc.make_components_case(name)
    assert pc.sha(x) == str(kat[f"{name}_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    lab = pc.labels3d_numpy(x > 0, connectivity)
    nd = _scipy()
    for m in pc.COMPONENTS[name]:
        key = pc.ckey(name, connectivity, m)
        got, counts = pc.components3d_numpy(x, m, connectivity, labels=lab)
        assert counts == tuple(int(v) for v in kat[key + "_counts"]), key
        assert got.dtype == np.float32 and pc.sha(got) == str(kat[key + "_sha"]), key
        if name in pc.COMPONENTS_FULL:
            assert got.tobytes() == pc.unpack(kat, key, x.shape).tobytes()
        if nd is not None:
            sl, found = nd.label(x > 0, structure=nd.generate_binary_structure(3, connectivity))
            keep = np.bincount(sl.ravel(), minlength=found + 1) >= m
            keep[0] = False
            assert got.tobytes() == keep[sl].astype(np.float32).tobytes() and counts == (found, int(keep.sum()))
    areas, found = pc.areas3d_numpy(x, connectivity)
    assert pc.sha(areas) == str(kat[f"{name}_c{connectivity}_areas_sha"]) and found == int(kat[f"{name}_c{connectivity}_areas_count"])


def test_component_special_values(kat):
    def counts(name, c, m):
        return tuple(int(v) for v in kat[pc.ckey(name, c, m) + "_counts"])

    assert [len(pc.forward_neighbours(c)) for c in pc.CONNECTIVITY] == [3, 9, 13]
    assert counts("empty", 1, 1) == (0, 0) and counts("full", 3, 4096) == (1, 1) and counts("full", 1, 4097) == (1, 0)
    assert counts("checker", 1, 1) == (768, 768) and counts("checker", 1, 2) == (768, 0)          # all singletons with 6 neighbours
    assert counts("checker", 2, 768) == (1, 1) and counts("checker", 2, 769) == (1, 0)            # one component with 18
    assert counts("edge", 1, 27) == (2, 2) and counts("edge", 2, 28) == (1, 1) and counts("edge", 1, 28) == (2, 0)
    assert counts("corner", 2, 27) == (2, 2) and counts("corner", 3, 54) == (1, 1) and counts("corner", 2, 28) == (2, 0)
    p = pc.make_components_case("path")
    assert int(p.sum()) == 2112 and all(p[z].any() for z in range(8))
    assert all(counts("path", c, 2112) == (1, 1) and counts("path", c, 2113) == (1, 0) for c in pc.CONNECTIVITY)
    found, kept = counts("blobs", 1, 7)
    assert 0 < kept < found and counts("blobs", 1, 1)[1] == found


def test_scene_is_what_it_claims(kat):
    """The lesion spans three slices and is small on each; the 3-D steps keep it, the plane-wise ones with the same settings drop it."""
    real, recon, mask = pc.make_scene()
    assert pc.sha(real, recon, mask) == str(kat["scene_in_sha"]) and real.shape == pc.SCENE_SHAPE
    d = recon - real
    sq = (d * d).astype(np.float32)
    sq_pp = pc.median3d_numpy(sq, 3) * pc.erode3d_numpy(real, 1, pc.SCENE_ROI_LEVEL)
    assert pc.sha(sq_pp) == str(kat["scene_sqerr_pp_sha"])
    pred3 = np.stack([pc.components3d_numpy(v, 7, 1, level=0.5)[0] for v in sq_pp])
    assert pred3.tobytes() == pc.unpack(kat, "scene_pred_pp", real.shape).tobytes()
    flat = sq.reshape(-1, *sq.shape[-2:])
    roi2 = pc2.erode_numpy(real.reshape(flat.shape), 1, pc.SCENE_ROI_LEVEL)
    pred2 = np.stack([pc2.components_numpy(p, 7, 1, level=0.5)[0] for p in pc2.median_numpy(flat, 3) * roi2]).reshape(real.shape)
    for sl in pc.SCENE_LESION:
        assert int(mask[sl].sum()) == 27 and all(int(mask[sl][z].sum()) == 9 for z in range(3))
        assert pred3[sl].sum() == 7 and pred2[sl].sum() == 0
    assert pred3.sum() == 14 and pred2.sum() == 0                       # nothing but the two lesions survives in 3-D, nothing at all in 2-D
    for sl in pc.SCENE_SPECK:                                           # the one-slice speck: alive after the 2-D median, gone after the 3-D one
        z = sl[1].start
        assert (pc2.median_numpy(sq[sl[0], z], 3)[sl[2], sl[3]] > 0.5).sum() == 5 and not (pc.median3d_numpy(sq, 3)[sl] > 0.5).any()


def test_fixture_says_how_it_was_produced(kat):
    text = str(kat["produced_with"])
    assert "scipy" in text and "median_filter" in text and "binary_erosion" in text and "label" in text
    assert os.path.getsize(FIXTURE) < 160 * 1024


# ---------------------------------------------------------------------------------- planted defects
def _median_breaks(**defect):
    return [(name, k) for name, k in MEDIAN_CASES if not np.array_equal(pc.median3d_numpy(pc.make_median_case(name), k, **defect),
                                                                        pc.median3d_numpy(pc.make_median_case(name), k))]


def test_planted_clamp_along_depth_is_caught():
    broken = _median_breaks(depth_mode="edge")
    assert ("m1x7x9", 5) not in broken                                  # one slice: clamping and reflecting read the same slice
    assert ("m3x9x40", 5) in broken and ("m6x20x37", 5) in broken and len(broken) >= 3
    # k = 3 reads one slice past the border, where clamp and reflect agree: only the window of 5 tells them apart
    assert all(k == 5 for _, k in broken)


def test_planted_rank_off_by_one_is_caught():
    """Where reflection repeats every value of a window (one slice, two slices) the neighbouring ranks can hold the same value;
    the cases with depth tell the ranks apart at both windows."""
    for offset in (1, -1):
        broken = _median_breaks(rank_offset=offset)
        assert {(name, k) for name in ("m3x9x40", "m6x20x37", "m9x40x70") for k in pc.WINDOWS} <= set(broken), (offset, broken)


def test_planted_linf_ball_is_caught(kat):
    """A box eroded by the cube is the box eroded by the octahedron, so the all-ones cases cannot tell; the holes can: the cube's
    corners see holes the octahedron does not."""
    broken = []
    for name, n in ERODE_CASES:
        x, level = pc.make_erode_case(name)
        if not np.array_equal(pc.erode3d_numpy(x, n, level, ball="linf"), pc.unpack(kat, pc.ekey(name, n), x.shape)):
            broken.append((name, n))
    assert broken == [("holes9x24x40", 1), ("holes9x24x40", 3)]


def test_planted_slice_wise_labelling_is_caught(kat):
    """2-D labelling of every slice: the lesion of the scene and the winding path fall apart."""
    for name in ("path", "blobs", "full"):
        x = pc.make_components_case(name)
        lab2 = np.stack([np.where(l >= 0, l + z * l.size, -1) for z, l in enumerate(pc2.labels_numpy(s > 0, 1) for s in x)])
        m = pc.COMPONENTS[name][1]
        got, counts = pc.components3d_numpy(x, m, 1, labels=lab2)
        assert counts != tuple(int(v) for v in kat[pc.ckey(name, 1, m) + "_counts"]), name


def test_planted_connectivity_2_as_3_is_caught(kat):
    x = pc.make_components_case("corner")
    got, counts = pc.components3d_numpy(x, 28, 2, labels=pc.labels3d_numpy(x > 0, 2, steps=pc.forward_neighbours(3)))
    assert counts == (1, 1) and counts != tuple(int(v) for v in kat[pc.ckey("corner", 2, 28) + "_counts"])
    x = pc.make_components_case("edge")                                  # and 1 treated as 2
    assert pc.components3d_numpy(x, 28, 1, labels=pc.labels3d_numpy(x > 0, 1, steps=pc.forward_neighbours(2)))[1] != \
        tuple(int(v) for v in kat[pc.ckey("edge", 1, 28) + "_counts"])


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
    assert _lib.ABI_VERSION >= 41 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    for name, st in (("median3d", _lib.Median3dArgs), ("erode3d", _lib.Erode3dArgs), ("components3d", _lib.Components3dArgs),
                     ("component_areas3d", _lib.ComponentAreas3dArgs)):
        assert st in _lib._STRUCTS and L.anoddpm_struct_size(b"anoddpm_%s_args" % name.encode()) == ctypes.sizeof(st)
    for name in ("median3d", "erode3d", "small_components3d", "component_areas3d", "components3d_workspace_bytes"):
        assert "anoddpm_" + name in _lib.SYMBOLS


def test_median3d_abi_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_median3d(None, None) == -1 and b"median3d: null args" in L.anoddpm_last_error()
    a = _lib.Median3dArgs()
    assert L.anoddpm_median3d(ctypes.byref(a), None) == -1 and b"median3d: null pointer" in L.anoddpm_last_error()
    # host memory stands in for the device pointers: every case below is rejected before anything is launched
    buf, p = _host_pointer()
    a.src = a.dst = a.status = a.roi = p
    rejected = _rejecter(L.anoddpm_median3d, a, dict(S=2, D=4, H=32, W=32, k=5, src_stride=4096, roi_stride=0, roi_slice_stride=0))
    rejected(b"S, D, H, W must be", S=0)
    rejected(b"S, D, H, W must be", D=0)
    rejected(b"S, D, H, W must be", H=0)
    rejected(b"S, D, H, W must be", W=-4)
    rejected(b"S, D, H, W must be", S=1 << 30, D=64, H=256, W=256)
    for k in (0, 1, 2, 4, 6, 7, 9, -3):
        rejected(b"k must be 3 or 5", k=k)
    rejected(b"k exceeds the plane", H=4)
    rejected(b"k exceeds the plane", W=2, k=3)
    rejected(b"volumes overlap", src_stride=4095)
    rejected(b"roi_slice_stride must be 0", roi_slice_stride=512)
    rejected(b"one plane is shared", roi_stride=4096)
    rejected(b"roi_stride must be 0", roi_slice_stride=1024, roi_stride=1024)
    a.status = None
    rejected(b"null pointer")


def test_erode3d_abi_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_erode3d(None, None) == -1 and b"erode3d: null args" in L.anoddpm_last_error()
    a = _lib.Erode3dArgs()
    assert L.anoddpm_erode3d(ctypes.byref(a), None) == -1 and b"erode3d: null pointer" in L.anoddpm_last_error()
    buf, p = _host_pointer()
    a.src = a.dst = p
    rejected = _rejecter(L.anoddpm_erode3d, a, dict(S=2, D=4, H=16, W=16, n=3, src_stride=1024, level=0.0))
    rejected(b"S, D, H, W must be", S=0)
    rejected(b"S, D, H, W must be", D=-1)
    rejected(b"S, D, H, W must be", W=0)
    for n in (0, 9, -1, 100):
        rejected(b"n must be in 1 ... 8", n=n)
    rejected(b"volumes overlap", src_stride=1023)


@pytest.mark.parametrize("entry", ["small_components3d", "component_areas3d"])
def test_components3d_abi_validation_without_gpu(entry):
    from anoddpm_amd import _lib
    L = _lib.lib()
    fn = getattr(L, "anoddpm_" + entry)
    assert fn(None, None) == -1 and entry.encode() + b": null args" in L.anoddpm_last_error()
    a = _lib.Components3dArgs() if entry == "small_components3d" else _lib.ComponentAreas3dArgs()
    assert fn(ctypes.byref(a), None) == -1 and entry.encode() + b": null pointer" in L.anoddpm_last_error()
    buf, p = _host_pointer()
    a.src = a.counts = a.workspace = p
    if entry == "small_components3d":
        a.dst = p
    else:
        a.area = p
    need = L.anoddpm_components3d_workspace_bytes(2, 4, 16, 16)
    rejected = _rejecter(fn, a, dict(S=2, D=4, H=16, W=16, connectivity=1, src_stride=1024, level=0.0, workspace_bytes=need))
    rejected(b"S, D, H, W must be", S=0)
    rejected(b"S, D, H, W must be", D=0)
    rejected(b"S, D, H, W must be", S=1 << 7, D=1 << 8, H=256, W=256)                     # S * D * H * W = 2^31
    rejected(b"S, D, H, W must be", S=1, D=1 << 11, H=1 << 10, W=1 << 10)
    for c in (0, 4, -1):
        rejected(b"connectivity must be", connectivity=c)
    rejected(b"volumes overlap", src_stride=1023)
    rejected(b"workspace too small", workspace_bytes=need - 1)
    rejected(b"workspace too small", workspace_bytes=0)
    if entry == "small_components3d":
        rejected(b"min_size must be", min_size=-1)


def test_components3d_workspace_bytes():
    from anoddpm_amd import _lib
    L = _lib.lib()
    for S, D, H, W in ((1, 1, 1, 1), (1, 4, 256, 256), (4, 155, 240, 240), (1, 1, 32767, 65536), (3, 7, 9, 11)):
        assert L.anoddpm_components3d_workspace_bytes(S, D, H, W) == 8 * S * D * H * W
    for S, D, H, W in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, -3), (1 << 7, 1 << 8, 256, 256), (1, 2, 32768, 32768),
                       (1, 1 << 30, 1 << 30, 1 << 30)):
        assert L.anoddpm_components3d_workspace_bytes(S, D, H, W) == -1


# ---------------------------------------------------------------------------------- the Python surface
def test_python_surface():
    import evaluation
    from anoddpm_amd import metrics

    def params(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert params(metrics.median_filter3d) == [("score", E), ("size", 5), ("roi", None), ("batched", None), ("return_status", False)]
    assert params(metrics.erode_mask3d) == [("x", E), ("iterations", 3), ("level", 0.0)]
    assert params(metrics.remove_small_components3d) == [("pred", E), ("min_size", 7), ("connectivity", 1), ("return_counts", False)]
    assert params(metrics.component_areas3d)[:2] == [("mask", E), ("connectivity", 3)]
    assert params(metrics.VolumePostProcess.__init__)[1:] == [("median", 5), ("erode", 3), ("roi_level", None), ("min_size", 7), ("connectivity", 1)]
    assert params(metrics.postprocess_volumes) == [("sqerr", E), ("pp", E), ("real", None), ("roi", None)]
    assert params(metrics.anomaly_metrics_volume) == [("real", E), ("recon", E), ("mask", E), ("threshold", 0.5), ("postprocess", None), ("roi", None)]
    for name in ("median_filter3d", "erode_mask3d", "remove_small_components3d", "component_areas3d", "VolumePostProcess",
                 "postprocess_volumes", "anomaly_metrics_volume"):
        assert name in metrics.__all__ and getattr(evaluation, name) is getattr(metrics, name), name
    # the plane-wise settings object is what it was
    assert params(metrics.PostProcess.__init__)[1:] == [("median", 5), ("erode", 3), ("roi_level", None), ("min_size", 7), ("connectivity", 1)]


def test_volume_postprocess_settings_object():
    from anoddpm_amd.metrics import PostProcess, VolumePostProcess
    pp = VolumePostProcess()
    assert (pp.median, pp.erode, pp.roi_level, pp.min_size, pp.connectivity) == (5, 3, None, 7, 1)
    off = VolumePostProcess(median=None, erode=0, min_size=0)
    assert off.median is None and off.erode == 0 and off.min_size == 0
    assert VolumePostProcess(3, 8, -0.95, 20, 3).connectivity == 3
    for bad in (4, 6, 7, 1, 0, 5.5, "5"):
        with pytest.raises(ValueError, match="median"):
            VolumePostProcess(median=bad)
    for bad in (-1, 9, 2.5):
        with pytest.raises(ValueError, match="erode"):
            VolumePostProcess(erode=bad)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="min_size"):
            VolumePostProcess(min_size=bad)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="connectivity"):
            VolumePostProcess(connectivity=bad)
    with pytest.raises(AttributeError):
        pp.median = 3
    with pytest.raises(AttributeError):
        del pp.erode
    assert pp == VolumePostProcess(5, 3) and pp != off and hash(pp) == hash(VolumePostProcess()) and "median=5" in repr(pp)
    assert pp != PostProcess() and PostProcess() != pp and len({pp, VolumePostProcess(), off}) == 2
    assert pickle.loads(pickle.dumps(off)) == off and copy.deepcopy(pp) == pp


def test_host_arguments_are_refused():
    """No CPU path: host tensors raise instead of computing somewhere else; argument errors name the argument."""
    import torch
    from anoddpm_amd import _lib, metrics
    x = torch.zeros(2, 16, 16)
    for fn in (metrics.median_filter3d, metrics.erode_mask3d, metrics.remove_small_components3d, metrics.component_areas3d):
        with pytest.raises(_lib.AnoddpmError):
            fn(x)
        with pytest.raises(ValueError, match=r"\[\.\.\., D, H, W\]"):
            fn(torch.zeros(16, 16))
        with pytest.raises(TypeError):
            fn(np.zeros((2, 16, 16), np.float32))
    with pytest.raises(ValueError, match="size"):
        metrics.median_filter3d(x, size=7)
    with pytest.raises(ValueError, match="window"):
        metrics.median_filter3d(torch.zeros(8, 4, 16), size=5)
    with pytest.raises(ValueError, match="as a batch"):
        metrics.median_filter3d(x, batched=True)
    with pytest.raises(ValueError, match="iterations"):
        metrics.erode_mask3d(x, iterations=9)
    with pytest.raises(ValueError, match="connectivity"):
        metrics.remove_small_components3d(x, connectivity=4)
    with pytest.raises(ValueError, match="min_size"):
        metrics.remove_small_components3d(x, min_size=-1)
    with pytest.raises(ValueError, match="connectivity"):
        metrics.component_areas3d(x, connectivity=0)
    with pytest.raises(TypeError):
        metrics.postprocess_volumes(x, metrics.PostProcess())
    with pytest.raises(ValueError, match="roi_level"):
        metrics.postprocess_volumes(x, metrics.VolumePostProcess(roi_level=-0.9))
    with pytest.raises(TypeError):
        metrics.anomaly_metrics_volume(x, x, x, postprocess=metrics.PostProcess())
    with pytest.raises(ValueError, match="real"):
        metrics.anomaly_metrics_volume(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(4, 4))
    with pytest.raises(ValueError, match="mask"):
        metrics.anomaly_metrics_volume(x, x, torch.zeros(3, 16, 16))
