"""-m "not gpu": the numpy restatement of an `AnomalousMRIDataset` item (tests/ano_loader_cases.py) against the reference class's own
outputs (tests/golden/ano_loader_kat.npz, written by tests/golden/make_ano_loader_golden.py) and, where Pillow imports, against Pillow
itself; the (crop_h, crop_w) centre-crop geometry; planted defects in the restatement, each of which must be caught; the new entry
point in the derived binding; and the class's file / `slices=` / `slices.json` / error handling with the launch replaced.

The long modes are compared slice by slice through the recorded per-slice sums: every slice at 32 x 32, every 5th at 64 x 64 and every
13th at 256 x 256 of "iterateUnknown" (the device test compares all of them)."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

import ano_loader_cases as ac
import loader_cases as lc
from anoddpm_amd import _lib
from anoddpm_amd import dataset as D
from conftest import GOLDEN
from oracle import loader_oracle as lo

# planes of the device test: larger in both axes, the crop itself, padded / larger, differences of 1 and of 3, padded in both
PLANES = ((181, 250), (175, 240), (100, 260), (176, 241), (178, 243), (60, 70))
OUT_SIZES = ((256, 256), (64, 64), (32, 32), (175, 240), (17, 23), (1, 1))


@pytest.fixture(scope="module")
def kat():
    g = np.load(os.path.join(GOLDEN, "ano_loader_kat.npz"))
    return {k: g[k] for k in g.files}


def stride_of(run):
    return {32: 1, 64: 5, 256: 13}[run[2][0]] if run[0] == "iterateUnknown" else 1


def compare_run(kat, run, calls, stride):
    """Lines for what differs between the calls of a run (ano_loader_cases.run_expected's form) and the fixture."""
    key, bad = ac.run_key(run), []
    assert len(calls) == kat[f"{key}__slices"].shape[0]
    for c, (value, keep, img, msk) in enumerate(calls):
        if not np.array_equal(ac.slices_record(value), kat[f"{key}__slices"][c]):
            bad.append(f"{key} call {c}: slices {ac.slices_record(value).tolist()} != {kat[f'{key}__slices'][c].tolist()}")
            continue
        if [lc.checksum(p) for p in img] != kat[f"{key}__img_sum"][c][keep].tolist():
            bad.append(f"{key} call {c}: image is not the reference's")
        if (msk is not None) != (f"{key}__mask_sum" in kat):
            bad.append(f"{key} call {c}: mask present {msk is not None}")
        elif msk is not None and [lc.checksum(p) for p in msk] != kat[f"{key}__mask_sum"][c][keep].tolist():
            bad.append(f"{key} call {c}: mask is not the reference's")
    if stride == 1 and not bad:
        if not lc.same_bits(ac.probe(calls[0][2]), kat[f"{key}__img_probe"]):
            bad.append(f"{key}: image probes differ")
        if f"{key}__img" in kat and not lc.same_bits(np.stack([c[2] for c in calls]), kat[f"{key}__img"]):
            bad.append(f"{key}: full image differs")
        if f"{key}__mask" in kat and not lc.same_bits(np.stack([c[3] for c in calls]), kat[f"{key}__mask"]):
            bad.append(f"{key}: full mask differs")
    return bad


# ------------------------------------------------------------------------------------------------------ fixture and restatement
def test_fixture_is_of_these_inputs_and_small(kat):
    assert kat["runs"].tolist() == [ac.run_key(r) for r in ac.RUNS]
    assert kat["input_sum"].tolist() == [[lc.checksum(ac.volume(n)), lc.checksum(ac.mask(n))] for n in ac.SHAPES]
    assert str(kat["produced_with"]).startswith("Pillow ")
    for f in ("ano_loader_kat.npz", "ano_slices.json"):
        assert os.path.getsize(os.path.join(GOLDEN, f)) < 108 * 1024
    table = ac.slice_table()
    for vid in ac.IDS:                                            # "random" may draw the stop itself, and every mode indexes below S
        assert table[vid].stop < ac.SHAPES[vid][0]
    assert any(0 < v < 1 for v in np.unique(ac.mask("18975-resized")))          # the non-binary mask


@pytest.mark.parametrize("size", ac.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_the_reference_class_in_every_mode(kat, size):
    bad = []
    for run in ac.RUNS:
        if run[2] == size:
            bad += compare_run(kat, run, ac.run_expected(run, stride=stride_of(run)), stride_of(run))
    assert not bad, "\n".join(bad)


def test_restatement_is_loader_oracle_resize_bilinear():
    for (h, w), out in zip(PLANES, OUT_SIZES):
        plane = lc.seeded_values(h * 1000 + w, (2, h, w))
        want = np.stack([lo.resize_bilinear(ac.center_crop(plane[i:i + 1], *ac.CROP)[0], *out) for i in range(2)])
        assert lc.same_bits(ac.resized(plane, out), want), ((h, w), out)


def _pil_item(plane, out):
    from PIL import Image
    ch, cw = ac.CROP
    im = Image.fromarray(np.ascontiguousarray(plane, dtype=np.float32))
    w, h = im.size
    pl, pt = (cw - w) // 2 if cw > w else 0, (ch - h) // 2 if ch > h else 0
    pr, pb = (cw - w + 1) // 2 if cw > w else 0, (ch - h + 1) // 2 if ch > h else 0
    padded = Image.new("F", (w + pl + pr, h + pt + pb), 0.0)
    padded.paste(im, (pl, pt))
    W, H = padded.size
    top, left = int(round((H - ch) / 2.0)), int(round((W - cw) / 2.0))
    crop = padded.crop((left, top, left + cw, top + ch))
    return np.array(crop), np.array(crop.resize((out[1], out[0]), Image.BILINEAR))


def test_restatement_and_crop_geometry_equal_pillow():
    pytest.importorskip("PIL")
    # differences of 0, 1, 3 and negative ones in each axis, beside the device test's planes
    planes = PLANES + ((175, 243), (178, 240), (176, 239), (174, 241), (172, 260), (181, 237), (174, 239))
    for k, (h, w) in enumerate(planes):
        plane = lc.seeded_values(9000 + k, (1, h, w))
        geom = D.center_crop_geometry_hw(h, w, *ac.CROP)
        assert geom == ac.crop_geometry(h, w, *ac.CROP)
        crop = ac.center_crop(plane, *ac.CROP)
        for out in (OUT_SIZES if (h, w) in PLANES else OUT_SIZES[2:3]):
            pil_crop, pil_res = _pil_item(plane[0], out)
            assert lc.same_bits(crop[0], pil_crop), ((h, w), geom)
            assert lc.same_bits(ac.resized(plane, out)[0], pil_res), ((h, w), out)


def test_crop_geometry_rule():
    g = D.center_crop_geometry_hw
    assert g(176, 241, 175, 240) == (0, 0, 0, 0)                  # a difference of 1: round(0.5) = 0
    assert g(178, 243, 175, 240) == (0, 0, 2, 2)                  # a difference of 3: round(1.5) = 2
    assert g(175, 240, 175, 240) == (0, 0, 0, 0)
    assert g(100, 260, 175, 240) == (0, 37, 0, 10)
    assert g(60, 71, 175, 240) == (84, 57, 0, 0)                  # pads (c - s) // 2 before, (c - s + 1) // 2 after
    for h, w, c in ((256, 192, 235), (200, 300, 235), (238, 237, 235), (40, 30, 235), (470, 471, 235)):
        assert D.center_crop_geometry(h, w, c) == g(h, w, c, c) == lo.center_crop_geometry(h, w, c)
    for h in range(170, 182):
        for w in range(236, 246):
            assert g(h, w, 175, 240) == ac.crop_geometry(h, w, 175, 240)


def test_threshold_after_normalize_is_a_half_before_it():
    planes = [ac.mask("18975-resized")[175:190], ac.mask("19723")[145:150], ac.volume("19723")[3:6]]
    for p in planes:
        for out in ((32, 32), (64, 64), (17, 23)):
            r = ac.resized(p, out)
            assert np.array_equal(lc.post_normalise(r) > 0, r > np.float32(0.5))
    half = np.full((1, 181, 250), 0.5, np.float32)
    for out in OUT_SIZES:
        assert (ac.resized(half, out) == np.float32(0.5)).all() and not ac.mask_of(half, out).any()


# ------------------------------------------------------------------------------------------------------------ planted defects
@pytest.mark.parametrize("defect", ac.DEFECTS)
def test_planted_defect_is_caught(kat, defect):
    runs = [r for r in ac.RUNS if r[2] == (32, 32) and r[0] != "iterateUnknown"]
    assert not [b for r in runs for b in compare_run(kat, r, ac.run_expected(r), 1)]
    caught = [ac.run_key(r) for r in runs if compare_run(kat, r, ac.run_expected(r, defect=defect), 1)]
    print(defect, "caught by", caught)
    assert caught, f"no run of the fixture notices {defect}"
    if defect == "mask_ge":                                       # the reference's own output on the block of exactly 0.5
        assert caught == ["iterateKnown_restricted__18975r__32x32"]
    if defect in ("exclusive_randint",):
        assert all(k.startswith("random__") for k in caught)
    if defect == "no_margin":
        assert all(k.startswith("iterateKnown_restricted__") for k in caught)


# -------------------------------------------------------------------------------------------------------------------- binding
def test_entry_point_and_struct_are_in_the_derived_binding():
    assert "anoddpm_ano_slices" in _lib.SYMBOLS and _lib.AnoSlicesArgs in _lib._STRUCTS
    assert _lib.ABI_VERSION >= 35
    L = _lib.lib()
    assert L.anoddpm_abi_version() == _lib.ABI_VERSION
    assert L.anoddpm_struct_size(b"anoddpm_ano_slices_args") == ctypes.sizeof(_lib.AnoSlicesArgs) > 0
    names = [f[0] for f in _lib.AnoSlicesArgs._fields_]
    for n in ("vols", "masks", "slice_idx", "img", "mask", "R", "C", "crop_h", "crop_w", "crop_top", "crop_left", "out_h", "out_w", "mean", "std"):
        assert n in names, n


def test_refused_arguments_without_a_device():
    """Every refusal comes before the launch, so it can be asked for on the host: a status, and the text says why."""
    L = _lib.lib()

    def good():
        a = _lib.AnoSlicesArgs()
        for f in ("vols", "masks", "slice_idx", "img", "mask", "kx", "kx_min", "kx_n", "ky", "ky_min", "ky_n"):
            setattr(a, f, 4096)
        a.n, a.R, a.C, a.crop_h, a.crop_w, a.out_h, a.out_w, a.kmax_x, a.kmax_y, a.mean, a.std = 1, 8, 8, 8, 8, 4, 4, 5, 5, 0.5, 0.5
        return a
    changes = [(f, None) for f in ("vols", "slice_idx", "img", "mask", "kx", "kx_min", "kx_n", "ky", "ky_min", "ky_n")]
    changes += [("n", 0), ("n", -1), ("n", 65536), ("std", 0.0)]
    changes += [(f, 0) for f in ("R", "C", "crop_h", "crop_w", "out_h", "out_w", "kmax_x", "kmax_y")]
    for f, v in changes:
        a = good()
        setattr(a, f, v)
        assert L.anoddpm_ano_slices(ctypes.byref(a), None) == _lib.EINVAL, (f, v)
        assert b"ano_slices" in L.anoddpm_last_error()
    assert L.anoddpm_ano_slices(None, None) == _lib.EINVAL


# ---------------------------------------------------------------------------------------------------------------------- class
SMALL = {"va": (12, 20, 30), "vb": (9, 20, 30), "vc": (9, 21, 30)}


@pytest.fixture()
def root(tmp_path):
    r = str(tmp_path)
    os.makedirs(os.path.join(r, "raw_cleaned"))
    os.makedirs(os.path.join(r, "raw"))
    os.makedirs(os.path.join(r, "mask"))
    for k, (name, shape) in enumerate(SMALL.items()):
        v = np.arange(np.prod(shape), dtype=np.float64).reshape(shape) + 1000 * k          # float64 on disk: astype(float32) at upload
        np.save(os.path.join(r, "raw_cleaned", f"{name}.npy"), v)
        np.save(os.path.join(r, "raw", f"{name}.npy"), -v)
        np.save(os.path.join(r, "mask", f"{name}.npy"), (v % 2).astype(np.uint8))
    np.save(os.path.join(r, "raw_cleaned", "va-resized.npy"), np.full((12, 5, 6), 7.0, np.float32))
    np.save(os.path.join(r, "mask", "va-resized.npy"), np.ones((12, 5, 6), np.float32))
    return r


@pytest.fixture()
def launches(monkeypatch):
    """The launch replaced by a recorder: (volumes, masks, slice indices) of every call; zeros come back."""
    calls = []

    def fake(self, vols, masks, slice_idx):
        calls.append((vols, masks, [int(s) for s in slice_idx]))
        shape = (len(vols),) + self.img_size
        return torch.zeros(shape), (torch.ones(shape) if masks is not None else None)
    monkeypatch.setattr(D.AnomalousMRIDataset, "_launch", fake)
    return calls


TABLE = {"va": range(2, 11), "vb": (1, 8), "vc": [0, 8]}


def test_class_slices_argument_json_file_and_errors(root, launches):
    ds = D.AnomalousMRIDataset(root, device="cpu", slices=TABLE)
    assert ds.slices == {"va": range(2, 11), "vb": range(1, 8), "vc": range(0, 8)} and len(ds) == 3
    assert ds.filenames == [f"{root}/raw_cleaned/{n}.npy" for n in ("va", "vb", "vc")]
    assert ds.img_size == (32, 32) and ds.slice_selection == "random"
    assert D.AnomalousMRIDataset(root, device="cpu", slices=TABLE, cleaned=False).filenames[0] == f"{root}/raw/va.npy"
    with pytest.raises(_lib.AnoddpmError, match="slices"):
        D.AnomalousMRIDataset(root, device="cpu")
    with open(os.path.join(root, "slices.json"), "w") as f:
        json.dump({"vb": [1, 8], "va": [2, 11]}, f)
    ds2 = D.AnomalousMRIDataset(root, device="cpu")
    assert ds2.slices == {"vb": range(1, 8), "va": range(2, 11)} and ds2.filenames[0].endswith("/vb.npy")
    assert D.AnomalousMRIDataset(root, device="cpu", slices={"va": (3, 4)}).slices == {"va": range(3, 4)}      # the argument wins
    for bad in ({}, {"va": 5}, {"va": (1, 2, 3)}, {"va": range(0, 8, 2)}, {"va": (5, 2)}, [("va", (1, 2))]):
        with pytest.raises(_lib.AnoddpmError):
            D.AnomalousMRIDataset(root, device="cpu", slices=bad)
    with pytest.raises(ValueError):
        D.AnomalousMRIDataset(root, device="cpu", slices=TABLE, slice_selection="iterateUnKnown")
    missing = D.AnomalousMRIDataset(root, device="cpu", slices={"nope": (0, 3)}, slice_selection="iterateKnown")
    with pytest.raises(_lib.AnoddpmError, match="raw_cleaned/nope.npy"):
        missing[0]
    os.remove(os.path.join(root, "mask", "vb.npy"))
    with pytest.raises(_lib.AnoddpmError, match="mask/vb.npy"):
        D.AnomalousMRIDataset(root, device="cpu", slices=TABLE, slice_selection="iterateKnown")[1]
    assert not launches


def test_class_modes_index_rules_and_sample_dict(root, launches):
    mk = lambda mode, **kw: D.AnomalousMRIDataset(root, device="cpu", slices=TABLE, slice_selection=mode, img_size=(8, 6), **kw)
    random.seed(3)
    want = [random.randint(2, 11) for _ in range(40)]
    assert 11 in want and 2 in want                               # the inclusive stop is drawn
    random.seed(3)
    ds = mk("random")
    for w in want:
        s = ds[torch.tensor(0)]
        assert s["slices"] == w and type(s["slices"]) is int and "mask" not in s and s["filenames"] == ds.filenames[0]
        assert tuple(s["image"].shape) == (1, 8, 6) and launches[-1][1] is None and launches[-1][2] == [w]
    with pytest.raises(IndexError):                               # vb has 9 planes and range(1, 8): fine; a range that reaches S is not
        D.AnomalousMRIDataset(root, device="cpu", slices={"vb": (9, 9)})[0]
    s = mk("iterateKnown")[0]
    assert s["slices"] == range(2, 11) and isinstance(s["slices"], range) and launches[-1][2] == list(range(2, 11))
    assert tuple(s["image"].shape) == tuple(s["mask"].shape) == (9, 8, 6) and len(launches[-1][1]) == 9
    s = mk("iterateKnown_restricted")[1]
    want = np.linspace(1 + 5, 8 - 5, 4).astype(np.int32)
    assert isinstance(s["slices"], np.ndarray) and s["slices"].dtype == np.int32 and s["slices"].tolist() == want.tolist() == launches[-1][2]
    assert tuple(s["mask"].shape) == (4, 8, 6)
    s = mk("iterateUnknown")[2]
    assert s["slices"] == 9 and type(s["slices"]) is int and "mask" not in s and launches[-1][2] == list(range(9)) and launches[-1][1] is None
    # residency: a volume is read and converted once, as float32
    ds = mk("iterateKnown")
    ds[0], ds[0]
    v = launches[-1][0][0]
    assert v.dtype == torch.float32 and v is launches[-2][0][0] and len(ds._vols) == 2
    assert torch.equal(v, torch.from_numpy(np.load(os.path.join(root, "raw_cleaned", "va.npy")).astype(np.float32)))
    # resized=True: the -resized files where they exist (va), the plain ones elsewhere (vb)
    ds = mk("iterateKnown", resized=True)
    ds[0], ds[1]
    assert tuple(launches[-2][0][0].shape) == (12, 5, 6) and tuple(launches[-2][1][0].shape) == (12, 5, 6)
    assert tuple(launches[-1][0][0].shape) == SMALL["vb"]
    # get_slices / get_batch
    img, msk = mk("random").get_slices(1, [8, 0, 0, 3])
    assert launches[-1][2] == [8, 0, 0, 3] and tuple(img.shape) == (4, 8, 6) and msk is not None
    with pytest.raises(IndexError):
        mk("random").get_slices(1, [9])
    with pytest.raises(IndexError):
        mk("random").get_slices(1, [-1])
    random.seed(5)
    b = mk("random").get_batch([0, 1, 1])
    random.seed(5)
    assert b["slices"] == [random.randint(2, 11), random.randint(1, 8), random.randint(1, 8)] == launches[-1][2]
    assert tuple(b["image"].shape) == (3, 1, 8, 6) and b["filenames"] == [ds.filenames[i] for i in (0, 1, 1)]
    with pytest.raises(ValueError, match="plane shape"):
        mk("random").get_batch([0, 2])                            # 20 x 30 and 21 x 30 planes


def test_class_user_transform_gets_the_numpy_slice_on_the_host(root, launches):
    seen = []

    def transform(a):
        seen.append(a)
        return torch.full((1, 4, 4), float(a[0, 0]))
    ds = D.AnomalousMRIDataset(root, transform=transform, device="cpu", slices=TABLE, slice_selection="iterateKnown_restricted", img_size=(4, 4))
    s = ds[1]
    vol, msk = np.load(os.path.join(root, "raw_cleaned", "vb.npy")), np.load(os.path.join(root, "mask", "vb.npy"))
    assert not launches and len(seen) == 8 and all(isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (20, 30) for a in seen)
    assert s["image"][:, 0, 0].tolist() == [float(np.float32(vol[i, 0, 0])) for i in s["slices"]]
    assert s["mask"][:, 0, 0].tolist() == [float(msk[i, 0, 0] > 0) for i in s["slices"]]


def test_class_mask_of_another_shape_is_refused(root, launches):
    np.save(os.path.join(root, "mask", "va.npy"), np.zeros((12, 20, 31), np.float32))
    with pytest.raises(ValueError, match="mask shape"):
        D.AnomalousMRIDataset(root, device="cpu", slices=TABLE, slice_selection="iterateKnown")[0]
    assert not launches
