"""-m gpu: anoddpm_mri_slice_prepare / anoddpm_resize_bilinear_pil / anoddpm_volume_normalise straight through the C ABI, and
`MRIDataset` over temporary roots, element by element against the cases and expected values of tests/loader_cases.py (all from
oracle/loader_oracle.py, which tests/test_loader_reference.py holds to Pillow's own outputs on the same cases).

Slice preparation and resizing are held to the bits, per item, and to the recorded Pillow sums of tests/golden/loader_kat.npz; the
normalisation to |got - expected64| <= 0.5 ulp32 + R |expected64| on every element and to the bits of float32(expected64) away from
rounding midpoints (R = 2e-14, fixed on the CPU from the kernel's summation order).  Every output, the resize's intermediate and the
normalisation workspace are filled with NaN before a launch: an element the kernels do not write shows.  No Pillow here.

Observed on the MI355X (run the file with -s): no case differs in a bit.  The device's lo, hi and hi - lo differ from the fsum ones by
exactly the figures the CPU model of its summation order gives (largest 6.85e-16, brain-n1048581); every normalised element is within
its bound (the error is the one rounding to fp32), and all but one of 3.3 M elements are far enough from a rounding midpoint to be
held to the bits of float32(expected64) -- and have them.
    mri_slice_prepare 162 launches, 25.8 M elements    resize_bilinear_pil 192 launches, 7.1 M elements
    volume_normalise 17 launches, 3.3 M elements       MRIDataset 124 calls, 3.7 M elements"""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import loader_cases as lc
from anoddpm_amd import _lib
from anoddpm_amd._lib import MriSliceArgs, ResizeArgs, current_stream, lib
from conftest import GOLDEN
from oracle import loader_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEDGER = {}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                 # (a copy: the cases' arrays are read-only)


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def count(entry, cases, elements):
    c = LEDGER.setdefault(entry, [0, 0])
    c[0] += cases
    c[1] += elements


@pytest.fixture(scope="module")
def kat():
    g = np.load(os.path.join(GOLDEN, "loader_kat.npz"))
    return {k: g[k] for k in g.files}


# ------------------------------------------------------------------------------------------------- anoddpm_mri_slice_prepare
def slice_prepare(case, vols_dev, items=None):
    """One launch over the items of a case (all of them, or the listed ones): [B][235][235] from a NaN-filled buffer."""
    items = list(range(len(case["items"]))) if items is None else items
    B = len(items)
    vols = torch.tensor([vols_dev[case["items"][b][0]].data_ptr() for b in items], dtype=torch.int64).to(DEV)
    ydim, sl = dev(case["ydim"][items]), dev(case["slice_idx"][items])
    aff = None if case["coeffs"] is None else dev(case["coeffs"][items])
    out = nans(B, lc.CROP, lc.CROP)
    a = MriSliceArgs()
    a.vols, a.ydim, a.slice_idx, a.out = vols.data_ptr(), ydim.data_ptr(), sl.data_ptr(), out.data_ptr()
    a.affine = aff.data_ptr() if aff is not None else None
    a.B, a.X, a.Z, a.crop = B, case["X"], case["Z"], lc.CROP
    a.pad_left, a.crop_top = lc.fold_geometry(case["geom"])
    _lib.check(lib().anoddpm_mri_slice_prepare(ctypes.byref(a), current_stream()), "mri_slice_prepare")
    return out.cpu().numpy()


@pytest.mark.parametrize("gname", lc.GEOMETRY_NAMES)
def test_slice_prepare_every_geometry_and_affine_set_to_the_bit(kat, gname):
    vols_dev = [dev(v) for v in lc.geometry_volumes(gname)]
    stride, bad = int(kat["probe_stride"]), []
    for ci, (g, a) in enumerate(lc.PREPARE_CASES):
        if g != gname:
            continue
        case, want = lc.prepare_case(g, a), lc.prepare_expected(g, a)
        got = slice_prepare(case, vols_dev)
        assert not np.isnan(got).any(), f"{case['name']}: {int(np.isnan(got).sum())} elements were not written"
        for b in range(len(case["items"])):
            if not lc.same_bits(got[b], want[b]):
                diff = np.nonzero(got[b].view(np.uint32) != want[b].view(np.uint32))
                y, x = int(diff[0][0]), int(diff[1][0])
                bad.append(f"{case['name']} item {b}: {diff[0].size} pixels differ from the oracle, first [{y}][{x}] got {got[b, y, x]!r} want {want[b, y, x]!r}")
            if lc.checksum(got[b]) != kat["prep_crop_sum"][ci, b]:
                bad.append(f"{case['name']} item {b}: not Pillow's recorded crop")
        if f"prep_probe_{g}_{a}" in kat:
            assert lc.same_bits(got[1].reshape(-1)[::stride], kat[f"prep_probe_{g}_{a}"]), case["name"]
        if a in lc.ALL_ZERO:
            assert not got.any(), case["name"]
        count("mri_slice_prepare", 1, got.size)
    # a launch over one item, and over the items in another order, gives the same images (the per-item ydim / slice / coefficients)
    case, want = lc.prepare_case(gname, "mixed"), lc.prepare_expected(gname, "mixed")
    for items in ([2], [2, 0, 1]):
        got = slice_prepare(case, vols_dev, items)
        assert lc.same_bits(got, want[items]), (gname, items)
        count("mri_slice_prepare", 1, got.size)
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------- anoddpm_resize_bilinear_pil
def resize(imgs, tables, out_hw, normalize):
    """One launch: imgs [B][in_h][in_w] -> (out [B][out_h][out_w], tmp [B][in_h][out_w]), both from NaN-filled buffers."""
    B, ih, iw = imgs.shape
    oh, ow = out_hw
    kx, xmin, xn, ky, ymin, yn = (dev(t) for t in tables)
    inp, tmp, out = dev(imgs), nans(B, ih, ow), nans(B, oh, ow)
    r = ResizeArgs()
    r.inp, r.tmp, r.out = inp.data_ptr(), tmp.data_ptr(), out.data_ptr()
    r.kx, r.kx_min, r.kx_n, r.ky, r.ky_min, r.ky_n = kx.data_ptr(), xmin.data_ptr(), xn.data_ptr(), ky.data_ptr(), ymin.data_ptr(), yn.data_ptr()
    r.B, r.in_h, r.in_w, r.out_h, r.out_w, r.kmax_x, r.kmax_y = B, ih, iw, oh, ow, kx.shape[1], ky.shape[1]
    r.mean, r.std, r.normalize = 0.5, 0.5, normalize
    _lib.check(lib().anoddpm_resize_bilinear_pil(ctypes.byref(r), current_stream()), "resize_bilinear_pil")
    return out.cpu().numpy(), tmp.cpu().numpy()


@pytest.mark.parametrize("name", lc.RESIZE_NAMES)
def test_resize_every_case_batch_and_normalize_to_the_bit(kat, name):
    from anoddpm_amd.dataset import resize_coeffs
    (ih, iw), out_hw = lc.resize_case(name)
    imgs = lc.resize_images(name)
    ci = lc.RESIZE_NAMES.index(name)
    for tables in (lc.resize_tables(name), lc.resize_tables(name, resize_coeffs)):
        assert tables[0].shape[1] == int(np.ceil(max(iw / out_hw[1], 1.0))) * 2 + 1
        for normalize in (0, 1):
            want = lc.resize_expected(name, normalize)
            got, tmp = resize(imgs, tables, out_hw, normalize)                       # B = 3
            assert not np.isnan(got).any() and not np.isnan(tmp).any(), f"{name}: elements of out or tmp were not written"
            assert lc.same_bits(got, want), f"{name} normalize {normalize}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {got.size} elements differ"
            count("resize_bilinear_pil", 1, got.size)
            for b in range(lc.RESIZE_B):                                             # B = 1, every item on its own
                one, tmp1 = resize(imgs[b:b + 1], tables, out_hw, normalize)
                assert not np.isnan(one).any() and not np.isnan(tmp1).any()
                assert lc.same_bits(one[0], want[b]) and lc.same_bits(one[0], got[b]) and lc.same_bits(tmp1[0], tmp[b]), (name, normalize, b)
                count("resize_bilinear_pil", 1, one.size)
            if not normalize:
                assert [lc.checksum(g) for g in got] == kat["resize_sum"][ci].tolist(), f"{name}: not Pillow's recorded output"


# -------------------------------------------------------------------------------------------------- anoddpm_volume_normalise
def volume_normalise(x):
    v = dev(x)
    out, ws = nans(x.size), nans(2 * 256 + 4, dtype=torch.float64)
    _lib.check(lib().anoddpm_volume_normalise(v.data_ptr(), x.size, out.data_ptr(), ws.data_ptr(), current_stream()), "volume_normalise")
    return out.cpu().numpy(), ws.cpu().numpy()


@pytest.mark.parametrize("name", lc.NORM_CASES)
def test_volume_normalise_every_element_against_fp64(name):
    x, e = lc.norm_volume(name), lc.norm_expected(name)
    got, ws = volume_normalise(x)
    assert not np.isnan(ws).any(), "the fold reads workspace entries nobody wrote"
    l0, h0 = lc.norm_stats_fsum(x)
    print(f"{name:18s} lo rel {abs(ws[514] - l0) / abs(l0):.3g}  hi rel {abs(ws[515] - h0) / abs(h0):.3g}  hi - lo rel {abs((ws[515] - ws[514]) - (h0 - l0)) / (h0 - l0):.3g}")
    lines, ratio, firm = lc.norm_failures(name, got, e)
    print(f"{name:18s} worst err / bound {ratio:.3f}; {firm} of {x.size} elements held to the bits of float32(expected64)")
    count("volume_normalise", 1, x.size)
    assert firm >= 0.99 * x.size                                   # (the bit-for-bit half of the bar is not an empty statement)
    assert not lines, "\n".join(lines)


@pytest.mark.parametrize("name", lc.NORM_NAN_CASES)
def test_volume_normalise_of_a_range_of_zero_is_nan(name):
    got, _ = volume_normalise(lc.norm_volume(name))
    assert np.isnan(got).all()
    count("volume_normalise", 1, got.size)


def test_normalise_volume_wrapper_keeps_the_shape():
    from anoddpm_amd.dataset import normalise_volume
    x = lc.norm_volume("brain-n65539")[:65536].reshape(32, 64, 32).copy()
    got = normalise_volume(x, DEV)
    assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
    assert lc.same_bits(got.cpu().numpy().reshape(-1), volume_normalise(x.reshape(-1))[0])


# ---------------------------------------------------------------------------------------------------------------- MRIDataset
def _write(root, name, vol):
    os.makedirs(os.path.join(root, name))
    np.save(os.path.join(root, name, f"{name}.npy"), vol)


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    """(X, Z) -> (root, {name: volume key}): two volumes each; the third root mixes Y = 101 and Y = 130."""
    out = {}
    for X, Z in lc.DATASET_SHAPES:
        d = str(tmp_path_factory.mktemp(f"mri{X}x{Z}"))
        keys = {"va": (X, lc.DATASET_Y, Z, 0), "vb": (X, lc.DATASET_Y, Z, 1)}
        for n, k in keys.items():
            _write(d, n, lc.dataset_volume(*k))
        out[(X, Z)] = (d, keys)
    X, Z = lc.DATASET_SHAPES[0]
    d = str(tmp_path_factory.mktemp("mriY"))
    keys = {"y101": (X, lc.DATASET_Y, Z, 2), "y130": (X, lc.DATASET_Y2, Z, 3)}
    for n, k in keys.items():
        _write(d, n, lc.dataset_volume(*k))
    out["mixedY"] = (d, keys)
    return out


def _inject(monkeypatch, D, draws):
    """RandomAffine's three draws per item, handed out in order; the ranges the dataset asks for must hold them."""
    it = iter([v for d in draws for v in d])

    def uniform(lo_, hi_):
        v = next(it)
        assert lo_ <= v <= hi_ and lo_ == -hi_
        return v
    monkeypatch.setattr(D, "_uniform", uniform)
    return it


def _rounded(draw):
    return draw[0], (int(round(draw[1])), int(round(draw[2])))


@pytest.mark.parametrize("size", lc.IMG_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("shape", lc.DATASET_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dataset_fixed_slice_with_and_without_injected_affine_draws(roots, monkeypatch, shape, size):
    from anoddpm_amd import dataset as D
    root, keys = roots[shape]
    plain = D.MRIDataset(root, img_size=size, random_slice=False, device=DEV, augment=False)
    aug = D.MRIDataset(root, img_size=size, random_slice=False, device=DEV, augment=True)
    idx = {n: plain.filenames.index(n) for n in keys}
    assert aug.filenames == plain.filenames and len(plain) == 2
    for n, k in keys.items():
        s = plain[idx[n]]
        assert s["filenames"] == n and s["image"].is_cuda and tuple(s["image"].shape) == (1,) + size
        assert lc.same_bits(s["image"].cpu().numpy(), lc.dataset_expected(k, 80, size)), (n, size)
        count("MRIDataset", 1, s["image"].numel())
    draws = lc.dataset_draws(*shape)
    for n, k in keys.items():
        for d in draws:
            it = _inject(monkeypatch, D, [d])
            img = aug[idx[n]]["image"]
            monkeypatch.undo()
            assert next(it, None) is None, "the dataset did not take three draws"
            assert lc.same_bits(img.cpu().numpy(), lc.dataset_expected(k, 80, size, _rounded(d))), (n, size, d)
            count("MRIDataset", 1, img.numel())
    # batches over mixed indices: every item its own draws
    order = ["va", "vb", "vb", "va", "va"]
    got, names = plain.get_batch([idx[n] for n in order])
    assert names == order and tuple(got.shape) == (5, 1) + size
    assert lc.same_bits(got.cpu().numpy(), np.stack([lc.dataset_expected(keys[n], 80, size) for n in order]))
    it = _inject(monkeypatch, D, draws)
    got, names = aug.get_batch([idx[n] for n in order])
    monkeypatch.undo()
    assert next(it, None) is None and names == order
    assert lc.same_bits(got.cpu().numpy(), np.stack([lc.dataset_expected(keys[n], 80, size, _rounded(d)) for n, d in zip(order, draws)]))
    count("MRIDataset", 2, 2 * got.numel())


@pytest.mark.parametrize("where", ["40x30", "100x120", "mixedY"])
def test_dataset_random_slices_and_real_draws_follow_the_generators(roots, where):
    """random_slice=True under random.seed and RandomAffine's draws under torch.manual_seed, replayed on the host: __getitem__ and
    get_batch give the oracle's default_transform of exactly those draws, and a batch equals its per-item calls."""
    from anoddpm_amd import dataset as D
    root, keys = roots[lc.DATASET_SHAPES[["40x30", "100x120"].index(where)] if where != "mixedY" else where]
    size = (32, 48)
    for augment in (False, True):
        ds = D.MRIDataset(root, img_size=size, random_slice=True, device=DEV, augment=augment)
        order = [ds.filenames.index(n) for n in (sorted(keys) * 3)[:5]]
        random.seed(17)
        torch.manual_seed(17)
        got, names = ds.get_batch(order)
        random.seed(17)
        torch.manual_seed(17)
        items = torch.stack([ds[i]["image"] for i in order])
        assert torch.equal(got, items), "a batch is not its per-item calls under the same generator state"
        random.seed(17)
        torch.manual_seed(17)
        want, slices = [], []
        for i in order:
            k = keys[ds.filenames[i]]
            s = random.randint(40, 100)
            aff = lo.random_affine_params(k[2], k[0]) if augment else None
            want.append(lc.dataset_expected(k, s, size, aff))
            slices.append(s)
        assert len(set(slices)) > 1 and names == [ds.filenames[i] for i in order]
        assert lc.same_bits(got.cpu().numpy(), np.stack(want)), (where, augment, slices)
        count("MRIDataset", 2, 2 * got.numel())
    if where == "mixedY":                                          # the batches above did mix two Y
        assert {tuple(ds._volume(n).shape)[1] for n in keys} == {lc.DATASET_Y, lc.DATASET_Y2}


def test_zz_counts_of_this_file():
    """Prints, per entry point, the launches (or dataset calls) made and the elements compared (run the file with -s)."""
    for k in sorted(LEDGER):
        print(f"{k:22s} {LEDGER[k][0]:5d} cases  {LEDGER[k][1]:10d} elements compared")
