"""SSIM without a device: the numpy restatement of csrc/ssim.hip's arrangement (tests/ssim_cases.py: reflect halo, separable
weight-table passes, tile / thread / tree partial sums) reproduces the fixture tests/golden/ssim_kat.npz -- the definition with
scipy's filters, the ones skimage calls -- within the derived bounds (|mssim| 1e-10, map 2^-24 + 1e-10 after the fp32 rounding
the kernel applies), and the host-side pieces of the native path: argument validation of anoddpm_ssim through the ABI, the
workspace-size function, the signature of metrics.ssim.  CPU only."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import ssim_cases as sc
from conftest import GOLDEN

CASES = [(name, window) for name, windows in sorted(sc.SINGLE.items()) for window in windows]


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "ssim_kat.npz"))


def _inputs(kat, name):
    real, recon = sc.make_case(name)
    assert sc.sha_inputs(real, recon) == str(kat[f"{name}_sha"]), \
        f"{name}: the regenerated input differs from the one the fixture was made from (a numpy that draws differently?)"
    return real, recon


def _check(got, want, what):
    print(f"{what}: mssim {got!r} fixture {want!r} |diff| {abs(got - want):.3g} bound {sc.MSSIM_TOL:.3g}")
    if np.isnan(want):
        assert np.isnan(got), what
    else:
        assert abs(got - want) <= sc.MSSIM_TOL, what


def test_every_size_has_every_window_that_fits():
    for name in ("s25x41", "s7x7", "s8x300"):
        h, w = (int(v) for v in name[1:].split("x"))
        assert tuple(sc.SINGLE[name]) == tuple(x for x in sc.WINDOWS if sc.win_of(x) <= min(h, w)), name


@pytest.mark.parametrize("name,window", CASES)
def test_kernel_arrangement_reproduces_fixture(kat, name, window):
    real, recon = _inputs(kat, name)
    got, gmap = sc.ssim_kernel_numpy(real, recon, window)
    _check(got, float(kat[f"{sc.key(name, window)}_mssim"]), sc.key(name, window))
    if (name, window) in sc.MAP_CASES:
        for cname, sl in sc.crops(gmap).items():
            want = kat[f"{sc.key(name, window)}_map_{cname}"]
            diff = float(np.abs(gmap[sl].astype(np.float32).astype(np.float64) - want).max())
            print(f"  map crop {cname} {want.shape}: largest |diff| {diff:.3g} bound {sc.MAP_TOL:.3g}")
            assert diff <= sc.MAP_TOL, (name, window, cname)


def test_special_values(kat):
    assert float(kat["equal256_w7_mssim"]) == 1.0 and float(kat["equal256_wgauss_mssim"]) == 1.0
    for window in sc.SINGLE["equal256"]:
        real, recon = sc.make_case("equal256")
        got, gmap = sc.ssim_kernel_numpy(real, recon, window)
        assert got == 1.0 and (gmap == 1.0).all()                       # exactly: uxx, uyy and uxy are the same sums in the same order
    assert float(kat["const256_w7_mssim"]) < 0.0 and float(kat["const256_wgauss_mssim"]) < 0.0
    # one interior pixel: the mean is that pixel's S
    real, recon = sc.make_case("s7x7")
    got, gmap = sc.ssim_kernel_numpy(real, recon, 7)
    assert got == gmap[0, 3, 3]


def test_batch_of_55_with_shared_real(kat):
    real, recons = sc.make_batch()
    assert sc.sha_inputs(real, recons) == str(kat["batch_sha"]), "batch: regenerated input differs from the fixture's"
    assert kat["batch_mssim"].shape == (sc.BATCH,) and (np.diff(kat["batch_mssim"]) < 0).all()     # more noise, less similar
    for j, recon in enumerate(recons):
        _check(sc.ssim_kernel_numpy(real, recon, 7)[0], float(kat["batch_mssim"][j]), f"batch[{j}]")


def test_nan_stays_in_its_segment(kat):
    real, recon = sc.make_nan_batch()
    assert sc.sha_inputs(real, recon) == str(kat["nan_sha"]), "nan: regenerated input differs from the fixture's"
    assert np.isnan(kat["nan_mssim"]).tolist() == [j == sc.NAN_SEGMENT for j in range(3)]
    for j in range(3):
        _check(sc.ssim_kernel_numpy(real[j], recon[j], 7)[0], float(kat["nan_mssim"][j]), f"nan[{j}]")


def test_fixture_says_how_it_was_produced(kat):
    text = str(kat["produced_with"])
    assert "scipy" in text and ("checked against skimage" in text or "NOT cross-checked" in text)
    assert os.path.getsize(os.path.join(GOLDEN, "ssim_kat.npz")) < 108 * 1024


def test_ssim_abi_validation_without_gpu():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 26 and L.anoddpm_struct_size(b"anoddpm_ssim_args") == ctypes.sizeof(_lib.SsimArgs)
    assert L.anoddpm_ssim(None, None) == -1 and b"null args" in L.anoddpm_last_error()
    a = _lib.SsimArgs()
    assert L.anoddpm_ssim(ctypes.byref(a), None) == -1 and b"null pointer" in L.anoddpm_last_error()
    # host memory stands in for the device pointers: every case below is rejected before anything is launched
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    a.real = a.recon = a.workspace = a.mssim = p
    a.cn, a.data_range, a.K1, a.K2 = 49.0 / 48.0, 2.0, 0.01, 0.03

    def rejected(text, **kw):
        vals = dict(S=2, C=1, H=32, W=32, win=7, mode=_lib.SSIM_UNIFORM, real_stride=0, recon_stride=1024,
                    workspace_bytes=L.anoddpm_ssim_workspace_bytes(2, 1, 32, 32))
        vals.update(kw)
        for k, v in vals.items():
            setattr(a, k, v)
        assert L.anoddpm_ssim(ctypes.byref(a), None) == -1, text
        assert text in L.anoddpm_last_error(), (text, L.anoddpm_last_error())

    rejected(b"S must be", S=0)
    rejected(b"C, H, W", C=0)
    rejected(b"C, H, W", H=0)
    for win in (1, 2, 8, 17, -7):
        rejected(b"win must be odd", win=win)
    rejected(b"win exceeds the image", H=5)
    rejected(b"win exceeds the image", W=14, win=15)
    rejected(b"mode must be", mode=2)
    rejected(b"gaussian window", mode=_lib.SSIM_GAUSSIAN, win=7)
    rejected(b"recon segments overlap", recon_stride=1023)
    rejected(b"real_stride", real_stride=512)
    rejected(b"workspace too small", workspace_bytes=L.anoddpm_ssim_workspace_bytes(2, 1, 32, 32) - 1)


def test_ssim_workspace_bytes():
    from anoddpm_amd import _lib
    L = _lib.lib()
    for S, C, H, W in ((1, 1, 7, 7), (1, 1, 16, 32), (1, 1, 17, 33), (55, 1, 256, 256), (16, 3, 512, 512), (1, 1, 8, 300)):
        assert L.anoddpm_ssim_workspace_bytes(S, C, H, W) == S * C * (-(-H // sc.TH)) * (-(-W // sc.TW)) * 8
    for S, C, H, W in ((0, 1, 8, 8), (-1, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, -3), (1 << 20, 1 << 10, 256, 256)):
        assert L.anoddpm_ssim_workspace_bytes(S, C, H, W) == -1


def test_python_surface():
    import evaluation
    from anoddpm_amd import metrics
    sig = inspect.signature(metrics.ssim)
    assert list(sig.parameters) == ["real", "recon", "batched", "data_range", "win_size", "gaussian_weights", "full"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["batched"], d["data_range"], d["win_size"], d["gaussian_weights"], d["full"]) == (None, 2.0, 7, False, False)
    assert "ssim" in metrics.__all__ and evaluation.ssim is metrics.ssim and evaluation.SSIM is metrics.SSIM
    for bad in (2, 8, 17, 1, 7.5):
        with pytest.raises(ValueError, match="win_size"):
            metrics._ssim_window(bad, False)
    assert metrics._ssim_window(7, False) == (7, 0, 49.0 / 48.0) and metrics._ssim_window(3, True) == (11, 1, 1.0)
    # the weight table of the restatement sums to one and is symmetric
    for window in sc.WINDOWS:
        w = sc.weights(window)
        assert abs(w.sum() - 1.0) < 1e-15 and (w == w[::-1]).all() and w.size == sc.win_of(window)
