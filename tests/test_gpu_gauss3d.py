"""-m gpu: Gaussian smoothing of whole volumes (csrc/gauss3d.hip through metrics.gaussian_filter3d, VolumePostProcess(gaussian=),
postprocess_volumes and anomaly_metrics_volume) against the fixture tests/golden/gauss3d.npz (what scipy.ndimage.gaussian_filter
returns) and the numpy restatement of tests/gauss3d_cases.py evaluated here.  Every comparison is `tobytes()` equality, no
tolerance.  scipy is not needed."""
import ctypes
import gc as _gc
import os

import numpy as np
import pytest
import torch

import gauss3d_cases as gc
from conftest import GOLDEN
from score_cases import bits as _bits, host as _host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "gauss3d.npz"))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _is_f32_on_device(t, like):
    return t.dtype == torch.float32 and t.shape == like.shape and t.is_cuda and t.device == like.device and t.is_contiguous()


# ---------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_volume_filter_matches_fixture_and_restatement(kat, name):
    from anoddpm_amd import metrics
    _, sigma = gc.CASES[name]
    x = gc.make_case(name)
    assert gc.sha(x) == str(kat[name + "_in_sha"]), f"{name}: regenerated input differs from the fixture's"
    d = _dev(x)
    out = metrics.gaussian_filter3d(d, sigma)
    assert _is_f32_on_device(out, d)
    got = _host(out)
    gc.check_fixture(kat, name, got)
    assert _bits(got, gc.gaussian3d_numpy(x, sigma))
    assert _bits(_host(metrics.gaussian_filter3d(d, sigma, gc.TRUNCATE)), got)         # two runs
    assert _bits(_host(metrics.gaussian_filter3d(d.double(), sigma)), got)             # other dtypes are converted
    if x.ndim == 3:
        assert _bits(_host(metrics.gaussian_filter3d(d[None, None], sigma))[0, 0], got)           # [1, 1, D, H, W]
    assert _bits(_host(d), x)


def test_z_skipped_is_the_plane_kernel_slice_by_slice(kat):
    from anoddpm_amd import metrics
    x = gc.make_case("z_skipped")
    d = _dev(x)
    vol = metrics.gaussian_filter3d(d, (0, 2, 2))
    planes = metrics.gaussian_filter(d, 2.0)                                           # the same tensor: its slices as a stack of planes
    assert _bits(_host(vol), _host(planes))
    gc.check_fixture(kat, "z_skipped", _host(planes))


def test_strided_batch_and_batch_of_five_equal_single_calls(kat):
    from anoddpm_amd import metrics
    sigma = gc.BATCH5[1]
    buf, vols = gc.make_strided()
    assert gc.sha(buf) == str(kat["strided_in_sha"])
    V, D, H, W = vols.shape
    dbuf = _dev(buf)
    view = dbuf[:, :D * H * W].view(V, D, H, W)
    assert not view.is_contiguous() and view.stride(0) == buf.shape[1] > D * H * W and view.data_ptr() == dbuf.data_ptr()
    out = metrics.gaussian_filter3d(view, sigma)
    assert _is_f32_on_device(out, view)
    gc.check_fixture(kat, "strided", _host(out))
    singles = np.stack([_host(metrics.gaussian_filter3d(view[v].contiguous(), sigma)) for v in range(V)])
    assert _bits(singles, _host(out)) and _bits(_host(out), gc.gaussian3d_numpy(vols, sigma))
    assert _bits(_host(dbuf), buf)                                                     # the input, padding included, is untouched

    b5 = gc.make_batch5()
    assert gc.sha(b5) == str(kat["batch5_in_sha"])
    d5 = _dev(b5)
    got = _host(metrics.gaussian_filter3d(d5, sigma))
    gc.check_fixture(kat, "batch5", got)
    assert _bits(np.stack([_host(metrics.gaussian_filter3d(d5[v], sigma)) for v in range(b5.shape[0])]), got)
    assert _bits(_host(metrics.gaussian_filter3d(d5, sigma, batched=True)), got)


def test_a_nan_stays_inside_its_volume(kat):
    from anoddpm_amd import metrics
    shape, sigma, v, _ = gc.POISON
    bad = gc.make_poison()
    assert gc.sha(bad) == str(kat["poison_in_sha"])
    got = _host(metrics.gaussian_filter3d(_dev(bad), sigma))
    clean = [j for j in range(shape[0]) if j != v]
    assert gc.sha(got[clean]) == str(kat["poison_clean_out_sha"])
    filled = bad.copy()
    filled[v] = np.float32(1.0)                                                        # other contents in the poisoned volume
    assert _bits(_host(metrics.gaussian_filter3d(_dev(filled), sigma))[clean], got[clean])
    want = gc.gaussian3d_numpy(bad[v], sigma)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert (np.isnan(got[v]) == np.isnan(want)).all()                                  # within the radii, by IEEE rules
    assert _bits(np.nan_to_num(got[v], nan=-1.0), np.nan_to_num(want, nan=-1.0))


@pytest.mark.parametrize("name", ["anisotropic", "rz32_tiny_plane", "z_skipped", "z_only", "x_skipped", "one_slice"])
def test_every_output_element_is_written(name):
    """Output and workspace start as NaN; a direct call, with no workspace where one launch runs."""
    from anoddpm_amd import _lib, metrics
    shape, sigma = gc.CASES[name]
    x = gc.make_case(name)
    d = _dev(x)
    sig, radii = metrics._gauss3d_radii(sigma, gc.TRUNCATE, "t")
    two = radii[0] > 0 and (radii[1] > 0 or radii[2] > 0)
    out = torch.full_like(d, float("nan"))
    tmp = torch.full_like(d, float("nan")) if two else None
    a = _lib.Gauss3dArgs()
    a.src, a.dst, a.tmp, a.src_stride = d.data_ptr(), out.data_ptr(), (tmp.data_ptr() if two else None), x.size
    a.S, a.D, a.H, a.W = (1,) + shape
    a.rz, a.ry, a.rx = radii
    tables = [metrics._gauss_table(s, gc.TRUNCATE, r, d.device) if r else None for s, r in zip(sig, radii)]
    a.wz, a.wy, a.wx = [None if t is None else t.data_ptr() for t in tables]
    L = _lib.lib()
    rc = L.anoddpm_gauss3d(ctypes.byref(a), _lib.current_stream())
    assert rc == 0, L.anoddpm_last_error().decode()
    got = _host(out)
    assert not np.isnan(got).any() and _bits(got, gc.gaussian3d_numpy(x, sigma))
    if two:
        z_only = gc.gaussian3d_numpy(x, (gc.sigmas_of(sigma)[0], 0.0, 0.0))
        assert _bits(_host(tmp), z_only)                                               # the workspace: the volume after the z pass, in fp32
    assert _bits(_host(d), x)


def test_refused_calls_launch_nothing():
    from anoddpm_amd import _lib, metrics
    x = gc.make_case("one_slice")
    d = _dev(x)
    out, tmp = torch.full_like(d, 7.0), torch.full_like(d, 7.0)
    w = metrics._gauss_table(1.0, gc.TRUNCATE, 4, d.device)
    L = _lib.lib()

    def call(**kw):
        a = _lib.Gauss3dArgs()
        a.src, a.dst, a.tmp, a.wz, a.wy, a.wx = d.data_ptr(), out.data_ptr(), tmp.data_ptr(), w.data_ptr(), w.data_ptr(), w.data_ptr()
        a.src_stride, a.S, a.D, a.H, a.W, a.rz, a.ry, a.rx = x.size, 1, 1, 5, 7, 4, 4, 4
        for k, v in kw.items():
            setattr(a, k, v)
        rc = L.anoddpm_gauss3d(ctypes.byref(a), _lib.current_stream())
        return rc, L.anoddpm_last_error().decode()

    for kw, text in (({"src": None}, "null"), ({"dst": None}, "null"), ({"tmp": None}, "null"), ({"wy": None}, "null"),
                     ({"dst": d.data_ptr()}, "dst overlaps src"), ({"tmp": d.data_ptr() + 4 * 34}, "tmp overlaps src"),
                     ({"tmp": out.data_ptr()}, "tmp overlaps dst"), ({"rz": 0, "ry": 0, "rx": 0}, "all three radii"), ({"rx": 33}, "radius"),
                     ({"D": 0}, "S, D, H, W")):
        rc, msg = call(**kw)
        assert rc != 0 and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (tmp == 7.0).all()
    rc, msg = call()
    assert rc == 0, msg
    assert _bits(_host(out), gc.gaussian3d_numpy(x, 1.0))
    with pytest.raises(ValueError, match="sigma"):
        metrics.gaussian_filter3d(d, (1, 2))
    with pytest.raises(ValueError, match="radius"):
        metrics.gaussian_filter3d(d, 8.2)
    copy = metrics.gaussian_filter3d(d, 0)                                             # every axis skipped: a copy, as scipy returns
    assert _is_f32_on_device(copy, d) and copy.data_ptr() != d.data_ptr() and _bits(_host(copy), x)


def test_graph_replay_gives_the_eager_bits():
    from anoddpm_amd import metrics
    sigma = (1.0, 2.0, 2.0)
    b5 = gc.make_batch5()
    x = _dev(b5[:2]).clone()
    eager = _host(metrics.gaussian_filter3d(x, sigma))                                 # first use: the tap tables are on the device now
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    _gc.collect()
    _gc.collect()
    was_enabled = _gc.isenabled()
    _gc.disable()                                                       # no collection of older graphs inside the capture
    try:
        with torch.cuda.graph(g):
            captured = metrics.gaussian_filter3d(x, sigma)
    finally:
        if was_enabled:
            _gc.enable()
    g.replay()
    torch.cuda.synchronize()
    assert _bits(_host(captured), eager)
    x.copy_(_dev(b5[2:4]))                                              # new contents in the captured input, replayed
    g.replay()
    torch.cuda.synchronize()
    assert _bits(_host(captured), gc.gaussian3d_numpy(b5[2:4], sigma))


# ---------------------------------------------------------------------------------- integration
def _scene(V=2, D=6, H=20, W=24):
    rng = np.random.default_rng(9395)
    real = (rng.random((V, D, H, W), dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
    recon = (rng.random((V, D, H, W), dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
    mask = (rng.random((V, D, H, W), dtype=np.float32) > np.float32(0.7)).astype(np.float32)
    return real, recon, mask


def test_postprocess_volumes_smooths_first():
    from anoddpm_amd import metrics
    real, recon, _ = _scene()
    sq = ((recon - real) * (recon - real)).astype(np.float32)
    d = _dev(sq)
    g = (1, 2, 2)
    smooth = metrics.gaussian_filter3d(d, g)
    assert _bits(_host(smooth), gc.gaussian3d_numpy(sq, g))
    for settings in (dict(median=3, erode=1, roi_level=-0.5, min_size=7), dict(median=None, erode=0, min_size=0),
                     dict(median=None, erode=2, roi_level=-2.0, min_size=0), dict(median=5, erode=0, min_size=0)):   # -2: all of it, less 2 voxels a side
        with_g = metrics.VolumePostProcess(gaussian=g, **settings)
        without = metrics.VolumePostProcess(**settings)
        got = metrics.postprocess_volumes(d, with_g, real=_dev(real))
        assert _bits(_host(got), _host(metrics.postprocess_volumes(smooth, without, real=_dev(real)))), settings
        assert not _bits(_host(got), _host(metrics.postprocess_volumes(d, without, real=_dev(real)))), settings
    assert _bits(_host(metrics.postprocess_volumes(d[0], metrics.VolumePostProcess(median=None, erode=0, min_size=0, gaussian=2.0))),
                 gc.gaussian3d_numpy(sq[0], 2.0))
    assert _bits(_host(d), sq)


def _numbers_equal(a, b):
    return a.keys() == b.keys() and all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() or (a[k] != a[k] and b[k] != b[k])
                                        for k in a if k != "maps")


@pytest.mark.parametrize("surface", [False, True])
def test_anomaly_metrics_volume_with_and_without_gaussian(surface):
    from anoddpm_amd import metrics
    fn = metrics.anomaly_metrics_volume_surface if surface else metrics.anomaly_metrics_volume
    real, recon, mask = _scene()
    dr, dc, dm = _dev(real), _dev(recon), _dev(mask)
    settings = dict(median=3, erode=0, min_size=7, connectivity=1)
    base = fn(dr, dc, dm, postprocess=metrics.VolumePostProcess(**settings))
    none = fn(dr, dc, dm, postprocess=metrics.VolumePostProcess(gaussian=None, **settings))
    raw = fn(dr, dc, dm)
    g = (0.5, 1.0, 1.0)
    pp = metrics.VolumePostProcess(gaussian=g, **settings)
    out = fn(dr, dc, dm, postprocess=pp)
    for v in range(real.shape[0]):
        assert _numbers_equal(none[v], base[v]) and none[v]["maps"].keys() == base[v]["maps"].keys()      # gaussian=None: no key, no bit changes
        assert all(_bits(_host(none[v]["maps"][k]), _host(base[v]["maps"][k])) for k in base[v]["maps"])
        assert out[v].keys() == base[v].keys() and out[v]["maps"].keys() == base[v]["maps"].keys()          # no new keys with it either
        assert all(np.float64(out[v][k]).tobytes() == np.float64(raw[v][k]).tobytes() or raw[v][k] != raw[v][k] for k in raw[v] if k != "maps")
    # the _pp values: the composed device calls
    sq = torch.stack([r["maps"]["sqerr"] for r in raw])
    sq_pp = metrics.postprocess_volumes(metrics.gaussian_filter3d(sq, g), metrics.VolumePostProcess(**settings), real=dr)
    pred_pp = metrics._small_components3d(sq_pp, 0.5, 7, 1)[0]
    half = torch.full((1,), 0.5, dtype=torch.float32, device=DEV)
    for v in range(real.shape[0]):
        assert _bits(_host(out[v]["maps"]["sqerr_pp"]), _host(sq_pp[v])) and _bits(_host(out[v]["maps"]["pred_pp"]), _host(pred_pp[v]))
        assert not _bits(_host(out[v]["maps"]["sqerr_pp"]), _host(base[v]["maps"]["sqerr_pp"]))
        cs = metrics.curve_scores(dm[v].reshape(-1), sq_pp[v].reshape(-1), batched=False)
        at = metrics.scores_at(dm[v].reshape(1, -1), pred_pp[v].reshape(1, -1), half, batched=True)
        for key, src in metrics._VOLUME_KEYS:
            want = float(_host(cs[src]).reshape(-1)[0]) if src in cs else float(_host(at[src]).reshape(-1)[0])
            have = out[v][key + "_pp"]
            assert np.float64(have).tobytes() == np.float64(want).tobytes() or (have != have and (want != want or key == "best_threshold")), (v, key)
        if surface:
            sd = metrics.surface_distance3d(pred_pp[v], dm[v])
            for key, src in metrics._VOLUME_SURFACE_KEYS:
                want, have = float(_host(sd[src]).reshape(-1)[0]), out[v][key + "_pp"]
                assert np.float64(have).tobytes() == np.float64(want).tobytes() or (have != have and want != want), (v, key)
