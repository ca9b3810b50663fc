"""-m "not gpu": what tests/test_gpu_loader_elements.py compares the device against, checked on the CPU.  The numpy oracle
(oracle/loader_oracle.py) against Pillow's recorded outputs (tests/golden/loader_kat.npz) on every case of tests/loader_cases.py and,
where Pillow imports, against Pillow itself; the host copies in anoddpm_amd/dataset.py against the oracle's; numpy models of the
kernels with one seeded defect each, which the device test's comparison has to reject; and the measurement R was fixed from."""
import importlib.util
import os

import numpy as np
import pytest

import loader_cases as lc
from conftest import GOLDEN
from oracle import loader_oracle as lo


@pytest.fixture(scope="module")
def kat():
    g = np.load(os.path.join(GOLDEN, "loader_kat.npz"))
    return {k: g[k] for k in g.files}


def test_the_fixture_was_recorded_on_these_inputs(kat):
    assert str(kat["produced_with"]).startswith("Pillow ")
    assert kat["prep_cases"].tolist() == [f"{g}/{a}" for g, a in lc.PREPARE_CASES] and kat["resize_cases"].tolist() == lc.RESIZE_NAMES
    for gi, g in enumerate(lc.GEOMETRY_NAMES):
        assert [lc.checksum(v) for v in lc.geometry_volumes(g)] == kat["prep_input_sum"][gi].tolist(), g
    assert [lc.checksum(lc.resize_images(n)) for n in lc.RESIZE_NAMES] == kat["resize_input_sum"].tolist()
    assert os.path.getsize(os.path.join(GOLDEN, "loader_kat.npz")) < 108 * 1024


@pytest.mark.parametrize("gname", lc.GEOMETRY_NAMES)
def test_oracle_slice_preparation_equals_recorded_pillow(kat, gname):
    stride = int(kat["probe_stride"])
    for ci, (g, a) in enumerate(lc.PREPARE_CASES):
        if g != gname:
            continue
        case, want = lc.prepare_case(g, a), lc.prepare_expected(g, a)
        for b in range(len(case["items"])):
            img, aff, crop = lc.prepare_stages(case, b)
            assert lc.checksum(aff) == kat["prep_affine_sum"][ci, b], (case["name"], b, "affine")
            assert lc.checksum(crop) == kat["prep_crop_sum"][ci, b], (case["name"], b, "crop")
            assert lc.same_bits(crop, want[b])
            if a not in lc.ALL_ZERO and a != "none":
                assert aff.any() and crop.any(), case["name"]
        if f"prep_probe_{g}_{a}" in kat:
            assert lc.same_bits(want[1].reshape(-1)[::stride], kat[f"prep_probe_{g}_{a}"]), case["name"]
        if a in lc.ALL_ZERO:
            assert not want.any(), case["name"]
    assert f"prep_probe_{gname}_none" in kat and f"prep_probe_{gname}_rot+3_t++" in kat


@pytest.mark.parametrize("name", lc.RESIZE_NAMES)
def test_oracle_resize_equals_recorded_pillow(kat, name):
    ci, want = lc.RESIZE_NAMES.index(name), lc.resize_expected(name, 0)
    assert [lc.checksum(w) for w in want] == kat["resize_sum"][ci].tolist()
    (ih, iw), (oh, ow) = lc.resize_case(name)
    if oh <= 64 and ow <= 64:
        assert lc.same_bits(want[0], kat[f"resize_{name}"])
    else:
        assert lc.same_bits(want[0].reshape(-1)[::int(kat["probe_stride"])], kat[f"resize_probe_{name}"])
    norm = lc.resize_expected(name, 1)
    assert norm.dtype == np.float32 and lc.same_bits(norm, (want - np.float32(0.5)) / np.float32(0.5))


def test_oracle_equals_pillow_directly_on_every_case(kat):
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("make_loader_golden", os.path.join(GOLDEN, "make_loader_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    n = 0
    for g, a in lc.PREPARE_CASES:
        case = lc.prepare_case(g, a)
        for b in range(len(case["items"])):
            _, aff, crop = lc.prepare_stages(case, b)
            p_aff, p_crop = gen.pil_prepare(case, b)
            assert lc.same_bits(aff, p_aff) and lc.same_bits(crop, p_crop), (case["name"], b)
            n += 1
    for name in lc.RESIZE_NAMES:
        _, (oh, ow) = lc.resize_case(name)
        for img, want in zip(lc.resize_images(name), lc.resize_expected(name, 0)):
            assert lc.same_bits(gen.pil_resize(img, oh, ow), want), name
            n += 1
    # the whole default transform at the dataset shapes, Pillow's stages chained
    for (X, Z) in lc.DATASET_SHAPES:
        key = (X, lc.DATASET_Y, Z)
        geom = lo.center_crop_geometry(X, Z, lc.CROP)
        for size in lc.IMG_SIZES:
            for ang, tx, ty in lc.dataset_draws(X, Z)[:3]:
                tr = (int(round(tx)), int(round(ty)))
                img = lo.take_slice(lc.dataset_volume(*key), 80)
                p = gen.pil_affine(img, lo.inverse_affine_matrix((Z * 0.5, X * 0.5), ang, tr))
                p = lc.post_normalise(gen.pil_resize(gen.pil_center_crop(p, geom), *size))[None]
                assert lc.same_bits(p, lc.dataset_expected(key, 80, size, (ang, tr))), (key, size, ang, tr)
                n += 1
    print(f"{n} images compared with Pillow {gen.PIL.__version__} (fixture: {kat['produced_with']})")


def test_host_copies_in_the_package_equal_the_oracle():
    """resize_coeffs, center_crop_geometry and affine_fixed_coeffs of anoddpm_amd/dataset.py are separate copies of the oracle's."""
    from anoddpm_amd import dataset as D
    assert D.CROP == lc.CROP
    for (X, Z), geom, _ in lc.GEOMETRIES:
        assert D.center_crop_geometry(X, Z, lc.CROP) == lo.center_crop_geometry(X, Z, lc.CROP) == geom
        for name, params in lc.affine_sets(X, Z).items():
            for ang, tr in params or []:
                want = lo.affine_fixed_coeffs(lo.inverse_affine_matrix((Z * 0.5, X * 0.5), ang, tr))
                assert D.affine_fixed_coeffs(Z, X, ang, tr) == want, (X, Z, name)
    for (X, Z) in lc.DATASET_SHAPES:
        assert D.center_crop_geometry(X, Z, lc.CROP) == lo.center_crop_geometry(X, Z, lc.CROP)
        for ang, tx, ty in lc.dataset_draws(X, Z):
            tr = (int(round(tx)), int(round(ty)))
            assert D.affine_fixed_coeffs(Z, X, ang, tr) == lo.affine_fixed_coeffs(lo.inverse_affine_matrix((Z * 0.5, X * 0.5), ang, tr))
    pairs = {(i, o) for (ih, iw), (oh, ow) in lc.RESIZE_CASES for i, o in ((ih, oh), (iw, ow))}
    pairs |= {(lc.CROP, s) for size in lc.IMG_SIZES for s in size}
    for i, o in sorted(pairs):
        got, want = D.resize_coeffs(i, o), lo.resize_coeffs(i, o)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (i, o)
    kmax = {n: (lc.resize_tables(n)[0].shape[1], lc.resize_tables(n)[3].shape[1]) for n in lc.RESIZE_NAMES}
    assert kmax["235x235-1x1"] == (471, 471) and kmax["235x235-33x48"] == (11, 17) and kmax["235x235-512x96"] == (7, 3)


def test_models_of_the_kernels_equal_the_oracle():
    """The numpy statements of slice_prepare_kernel (with dataset.py's two signed numbers) and of the two resample launches, without a
    defect, give the oracle's bits on every case: what the seeded defects below depart from."""
    for g, a in lc.PREPARE_CASES:
        assert lc.same_bits(lc.prepare_model(lc.prepare_case(g, a)), lc.prepare_expected(g, a)), (g, a)
    for name in lc.RESIZE_NAMES:
        for img, want in zip(lc.resize_images(name), lc.resize_expected(name, 0)):
            assert lc.same_bits(lc.resize_model(img, lc.resize_tables(name)), want), name


@pytest.mark.parametrize("defect", lc.PREPARE_DEFECTS)
def test_seeded_slice_preparation_defect_is_caught(defect):
    caught = [f"{g}/{a}" for g, a in lc.PREPARE_CASES if not lc.same_bits(lc.prepare_model(lc.prepare_case(g, a), defect), lc.prepare_expected(g, a))]
    print(f"{defect}: caught by {len(caught)} of {len(lc.PREPARE_CASES)} cases")
    assert caught, defect
    geoms = {c.split("/")[0] for c in caught}
    if defect == "flip_pad_left":                                # every class with a horizontal offset
        assert geoms == {n for (_, geom, n) in lc.GEOMETRIES if geom[0] != geom[3]}
    if defect == "flip_crop_top":
        assert geoms == {n for (_, geom, n) in lc.GEOMETRIES if geom[1] != geom[2]}
    if defect == "one_ydim":
        assert geoms == set(lc.GEOMETRY_NAMES)
    if defect == "truncate":                                     # only an affine that sends a coordinate into (-1, 0)
        assert not any(c.endswith("/none") or c.endswith("/identity") for c in caught)


@pytest.mark.parametrize("defect", lc.RESIZE_DEFECTS)
def test_seeded_resize_defect_is_caught(defect):
    caught = [n for n in lc.RESIZE_NAMES
              if not lc.same_bits(np.stack([lc.resize_model(img, lc.resize_tables(n), defect) for img in lc.resize_images(n)]), lc.resize_expected(n, 0))]
    print(f"{defect}: caught by {caught}")
    assert len(caught) >= 6 and "235x235-1x1" in caught and "30x40-64x48" in caught


def test_normalisation_error_model_and_R():
    """The kernel's summation order against math.fsum: R is 16x the largest relative difference of lo, hi and hi - lo, rounded up to
    one digit.  The model of the kernel, pushed through the device test's own check, passes it; a range off by 1e-7 does not."""
    worst = {"lo": 0.0, "hi": 0.0, "hi - lo": 0.0}
    for name in lc.NORM_CASES:
        x = lc.norm_volume(name)
        l0, h0 = lc.norm_stats_fsum(x)
        l1, h1 = lc.norm_stats_kernel(x)
        rel = {"lo": abs(l1 - l0) / abs(l0), "hi": abs(h1 - h0) / abs(h0), "hi - lo": abs((h1 - l1) - (h0 - l0)) / abs(h0 - l0)}
        print(f"{name:18s} " + "  ".join(f"{k} {v:.3g}" for k, v in rel.items()) + f"   clipped below {(x < l0).sum()} above {(x > h0).sum()} of {x.size}")
        worst = {k: max(worst[k], rel[k]) for k in worst}
        assert (x < l0).any() or name.startswith("two") and (x > h0).any()
        e = lc.norm_expected(name)
        got = (np.clip(x, l1, h1) / (h1 - l1)).astype(np.float32)
        lines, ratio, firm = lc.norm_failures(name, got, e)
        assert not lines and ratio <= 1.0 and firm >= 0.99 * x.size, (lines, ratio, firm)
        off = (np.clip(x, l1, h1) / ((h1 - l1) * (1 + 1e-7))).astype(np.float32)
        assert lc.norm_failures(name, off, e)[0], name
    top = max(worst.values())
    print("largest: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"   16x = {16 * top:.3g}   R = {lc.R:g}")
    digit = 10.0 ** np.floor(np.log10(16 * top))
    assert lc.R == pytest.approx(np.ceil(16 * top / digit) * digit, rel=1e-9), (top, lc.R)
    for name in lc.NORM_NAN_CASES:
        assert np.isnan(lc.norm_expected(name)).all()
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.isnan(lo.normalise_volume(lc.norm_volume(name))).all()

