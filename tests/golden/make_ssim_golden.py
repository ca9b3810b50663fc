"""Writes tests/golden/ssim_kat.npz: the mean structural similarity -- and a few crops of the similarity map -- of the cases of
tests/ssim_cases.py, computed by the definition in fp64 with scipy.ndimage.uniform_filter / gaussian_filter(sigma=1.5,
truncate=3.5), the filters skimage.metrics.structural_similarity calls (`ssim_cases.ssim_expected`).  Run by hand:
    python tests/golden/make_ssim_golden.py
Inputs are not stored: the fixture pins the SHA-256 of the regenerated fp32 inputs.  Where skimage can be imported the generator
also asserts that structural_similarity on fp64 copies of the inputs agrees with the restatement to 1e-12; the fixture's
`produced_with` entry says whether that happened.  Before anything is written, the restatement of the kernel's own arrangement
(`ssim_cases.ssim_kernel_numpy`) has to agree with the expected values within the asserted bounds."""
import os
import sys

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ssim_cases as sc  # noqa: E402


def skimage_ssim():
    try:
        import skimage
        from skimage.metrics import structural_similarity
    except ImportError:
        return None, None
    return structural_similarity, skimage.__version__


def main():
    sk, sk_version = skimage_ssim()
    out, worst = {}, {"mssim": 0.0, "map": 0.0, "skimage": 0.0}

    def one(real, recon, window):
        want, smap = sc.ssim_expected(real, recon, window)
        got, gmap = sc.ssim_kernel_numpy(real, recon, window)
        if np.isnan(want):
            assert np.isnan(got)
            return want, smap
        worst["mssim"] = max(worst["mssim"], abs(got - want))
        worst["map"] = max(worst["map"], float(np.abs(gmap - smap).max()))
        assert abs(got - want) <= sc.MSSIM_TOL and np.abs(gmap - smap).max() <= 1e-10, (window, got, want)
        if sk is not None:
            kw = dict(gaussian_weights=True) if window == "gauss" else dict(win_size=sc.win_of(window))
            ref = sk(real.astype(np.float64), recon.astype(np.float64), channel_axis=0, data_range=sc.DATA_RANGE, **kw)
            worst["skimage"] = max(worst["skimage"], abs(ref - want))
            assert abs(ref - want) <= 1e-12, (window, ref, want)
        return want, smap

    for name, windows in sorted(sc.SINGLE.items()):
        real, recon = sc.make_case(name)
        out[f"{name}_sha"] = np.array(sc.sha_inputs(real, recon))
        for window in windows:
            want, smap = one(real, recon, window)
            out[f"{sc.key(name, window)}_mssim"] = np.float64(want)
            if (name, window) in sc.MAP_CASES:
                for cname, sl in sc.crops(smap).items():
                    out[f"{sc.key(name, window)}_map_{cname}"] = smap[sl]
    assert out["equal256_w7_mssim"] == 1.0 and out["equal256_wgauss_mssim"] == 1.0 and out["const256_w7_mssim"] < 0.0

    real, recons = sc.make_batch()
    out["batch_sha"] = np.array(sc.sha_inputs(real, recons))
    out["batch_mssim"] = np.array([one(real, r, 7)[0] for r in recons], np.float64)
    real, recon = sc.make_nan_batch()
    out["nan_sha"] = np.array(sc.sha_inputs(real, recon))
    out["nan_mssim"] = np.array([one(x, y, 7)[0] for x, y in zip(real, recon)], np.float64)
    assert np.isnan(out["nan_mssim"]).tolist() == [j == sc.NAN_SEGMENT for j in range(3)]

    checked = (f"checked against skimage {sk_version} structural_similarity on the fp64 inputs: largest difference "
               f"{worst['skimage']:.3g} (bound 1e-12)") if sk is not None else \
        "skimage was not importable where this fixture was generated: NOT cross-checked against structural_similarity"
    out["produced_with"] = np.array(f"ssim_cases.ssim_expected: numpy {np.__version__}, scipy {scipy.__version__} ndimage filters; {checked}")
    path = os.path.join(HERE, "ssim_kat.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; {out['produced_with']}")
    print(f"kernel-arrangement restatement against it: largest |mssim diff| {worst['mssim']:.3g}, largest map element diff {worst['map']:.3g}")


if __name__ == "__main__":
    main()
