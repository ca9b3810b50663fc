"""Shared by the anomalous-loader tests (tests/test_ano_loader_reference.py on the CPU, tests/test_gpu_ano_loader.py on the device,
tests/golden/make_ano_loader_golden.py for the reference's own outputs): the seeded synthetic data root, the runs the fixture
records, and a numpy restatement of one `AnomalousMRIDataset` item (reference dataset.py:646-790) built on oracle/loader_oracle.py:

    plane = volume[s]                                      axis 0 is sliced
    crop  = torchvision CenterCrop((175, 240))             zero padding where the plane is smaller, half-even window offset
    r     = Pillow resize(BILINEAR)                        loader_oracle.resize_coeffs; horizontal pass, then vertical, fp64 sums in
                                                           ascending tap order, fp32 after each pass (== loader_oracle.resize_bilinear)
    image = (r - 0.5) / 0.5 in fp32                        mask = ((r_mask - 0.5) / 0.5 > 0) as 0/1

and of the four slice-selection rules.  With `defect=None` the restatement must equal the fixture (and Pillow) bit for bit; each
named defect must be caught on the cases (tests/test_ano_loader_reference.py).  No device and no Pillow here.

The synthetic root (regenerated from seeds, never stored): ids "19723" (172 planes of 178 x 243: larger than the crop by 3 in
both axes, where the half-even window offset 2 is not the truncated 1) and "18975" (196 planes of 100 x 263: padded in one axis, larger
by 23 in the other: offset 12, not 11), masks with a blob per plane inside the tumour range, and a `-resized` pair for "18975" (196
planes of 60 x 70: padded in both) whose mask is not binary: a block of exactly 0.5 (which `> 0` after Normalize maps to 0, `>=` to 1)
and a rim of 0.75.  The ranges come from tests/golden/ano_slices.json, the
reference class's `slices` attribute dumped as data."""
import functools
import json
import os
import random

import numpy as np

import loader_cases as lc
from oracle import loader_oracle as lo

CROP = (175, 240)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDS = ("19723", "18975")
SHAPES = {"19723": (172, 178, 243), "18975": (196, 100, 263), "18975-resized": (196, 60, 70)}
MODES = ("random", "iterateKnown", "iterateKnown_restricted", "iterateUnknown")
SIZES = ((32, 32), (64, 64), (256, 256))
RANDOM_SEED, RANDOM_CALLS = 23, 3
# (mode, id, img_size, resized)
RUNS = [(m, i, s, False) for s in SIZES for m in MODES for i in IDS] + \
    [("iterateKnown_restricted", "18975", (32, 32), True), ("random", "18975", (32, 32), True)]
FULL = [("random", "19723", (32, 32), False), ("iterateKnown_restricted", "19723", (32, 32), False),
        ("iterateKnown_restricted", "18975", (32, 32), True)]                  # runs whose outputs the fixture holds in full
DEFECTS = ("truncate_offset", "mask_ge", "swap_crop", "exclusive_randint", "no_margin", "vertical_first")


def run_key(run):
    m, i, (h, w), resized = run
    return f"{m}__{i}{'r' if resized else ''}__{h}x{w}"


def slice_table():
    with open(os.path.join(GOLDEN, "ano_slices.json")) as f:
        return {k: range(*v) for k, v in json.load(f).items()}


# ------------------------------------------------------------------------------------------------------------ synthetic data
@functools.lru_cache(maxsize=None)
def volume(name):
    """fp32 [S][R][C] in [0, 1) with exact zeros: a smooth ramp plus noise, so neighbouring planes and pixels all differ."""
    S, R, C = SHAPES[name]
    rng = np.random.RandomState(7000 + sum(ord(c) for c in name))
    v = rng.random_sample((S, R, C)).astype(np.float32)
    v *= (0.25 + 0.75 * np.linspace(0.0, 1.0, C, dtype=np.float32))[None, None, :]
    v[v < 0.03] = 0.0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def mask(name):
    """fp32 0/1 [S][R][C]: inside the id's tumour range a disc whose centre and radius move with the plane, elsewhere empty."""
    S, R, C = SHAPES[name]
    r = slice_table()[name.split("-")[0]]
    m = np.zeros((S, R, C), np.float32)
    yy, xx = np.mgrid[0:R, 0:C]
    for s in range(r.start, min(r.stop + 1, S)):
        k = s - r.start
        cy, cx, rad = R * (0.35 + 0.01 * (k % 17)), C * (0.4 + 0.008 * (k % 23)), 4.0 + (k % 11) * min(R, C) / 40.0
        m[s] = ((yy - cy) ** 2 + (xx - cx) ** 2 < rad * rad).astype(np.float32)
        if name.endswith("-resized"):
            m[s, 5:25, 40:65] = 0.75
            m[s, 8:22, 44:61] = 0.5
    m.setflags(write=False)
    return m


def write_root(root):
    """The data root the reference's class and ours read: raw_cleaned/, mask/, with the -resized pair of "18975"."""
    os.makedirs(os.path.join(root, "raw_cleaned"))
    os.makedirs(os.path.join(root, "mask"))
    for name in SHAPES:
        np.save(os.path.join(root, "raw_cleaned", f"{name}.npy"), volume(name))
        np.save(os.path.join(root, "mask", f"{name}.npy"), mask(name))
    return root


def data_name(run):
    return run[1] + ("-resized" if run[3] and run[1] + "-resized" in SHAPES else "")


def probe(a):
    """About 200 elements of an array at an odd stride fixed by its size."""
    flat = np.ascontiguousarray(a).reshape(-1)
    return flat[::(flat.size // 200) | 1].copy()


# ---------------------------------------------------------------------------------------------------------------- one item
def crop_geometry(h, w, crop_h, crop_w, defect=None):
    """torchvision center_crop for a (crop_h, crop_w) window: (pad_left, pad_top, crop_top, crop_left)."""
    pad_left = (crop_w - w) // 2 if crop_w > w else 0
    pad_top = (crop_h - h) // 2 if crop_h > h else 0
    pad_right = (crop_w - w + 1) // 2 if crop_w > w else 0
    pad_bottom = (crop_h - h + 1) // 2 if crop_h > h else 0
    H, W = h + pad_top + pad_bottom, w + pad_left + pad_right
    rnd = (lambda v: int(v)) if defect == "truncate_offset" else (lambda v: int(round(v)))
    return pad_left, pad_top, rnd((H - crop_h) / 2.0), rnd((W - crop_w) / 2.0)


def center_crop(planes, crop_h, crop_w, defect=None):
    """[n][h][w] -> [n][crop_h][crop_w]."""
    n, h, w = planes.shape
    pl, pt, ct, cl = crop_geometry(h, w, crop_h, crop_w, defect)
    padded = np.zeros((n, max(h, crop_h), max(w, crop_w)), planes.dtype)
    padded[:, pt:pt + h, pl:pl + w] = planes
    return np.ascontiguousarray(padded[:, ct:ct + crop_h, cl:cl + crop_w])


def _resize_stack(img, tables, defect):
    """loader_cases._pass (one pass of the resample: ascending taps, fp64, fp32 store) along the axes of a stack [n][h][w]."""
    kx, xmin, xn, ky, ymin, yn = tables
    if defect == "vertical_first":
        return lc._pass(lc._pass(img, ky, ymin, yn, 1, np.float64), kx, xmin, xn, 2, np.float64)
    return lc._pass(lc._pass(img, kx, xmin, xn, 2, np.float64), ky, ymin, yn, 1, np.float64)


def resized(planes, out_hw, crop=CROP, defect=None):
    """Centre crop and Pillow's bilinear resize of a stack of planes, fp32 [n][out_h][out_w] (before Normalize)."""
    ch, cw = crop[::-1] if defect == "swap_crop" else crop
    img = center_crop(np.asarray(planes, np.float32), ch, cw, defect)
    return _resize_stack(img, lo.resize_coeffs(cw, out_hw[1]) + lo.resize_coeffs(ch, out_hw[0]), defect)


def image_of(planes, out_hw, crop=CROP, defect=None, mean=0.5, std=0.5):
    r = resized(planes, out_hw, crop, defect)
    return (r - np.float32(mean)) / np.float32(std)


def mask_of(planes, out_hw, crop=CROP, defect=None, mean=0.5, std=0.5):
    v = image_of(planes, out_hw, crop, defect, mean, std)
    return ((v >= 0) if defect == "mask_ge" else (v > 0)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------- selection
def select(mode, rng, S, defect=None):
    """(slice indices, the sample's "slices" value, whether a mask comes with it) of one __getitem__."""
    if mode == "random":
        s = random.randrange(rng.start, rng.stop) if defect == "exclusive_randint" else random.randint(rng.start, rng.stop)
        return [s], s, False
    if mode == "iterateKnown":
        return list(rng), rng, True
    if mode == "iterateKnown_restricted":
        margin = 0 if defect == "no_margin" else 5
        sl = np.linspace(rng.start + margin, rng.stop - margin, 4).astype(np.int32)
        return [int(s) for s in sl], sl, True
    assert mode == "iterateUnknown"
    return list(range(S)), S, False


def slices_record(value):
    """The "slices" value of a sample as an int64 array: an int -> [v], a range -> [start, stop], an array as it is."""
    if isinstance(value, range):
        return np.array([value.start, value.stop], np.int64)
    return np.atleast_1d(np.asarray(value)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _expected(name, indices, out_hw, with_mask, defect):
    idx = list(indices)
    img = image_of(volume(name)[idx], out_hw, defect=defect)
    msk = mask_of(mask(name)[idx], out_hw, defect=defect) if with_mask else None
    for a in (img, msk):
        if a is not None:
            a.setflags(write=False)
    return img, msk


def run_expected(run, defect=None, stride=1):
    """The restatement of one run: list of (slices value, indices, image [n,H,W], mask or None), one entry per call (RANDOM_CALLS for
    "random" under random.seed(RANDOM_SEED), else one).  stride > 1 keeps every stride-th slice of the long modes (the indices say which)."""
    mode, vid, out_hw, _ = run
    name, rng = data_name(run), slice_table()[vid]
    S = SHAPES[name][0]
    calls = []
    if mode == "random":
        random.seed(RANDOM_SEED)
    for _ in range(RANDOM_CALLS if mode == "random" else 1):
        idx, value, with_mask = select(mode, rng, S, defect)
        keep = list(range(0, len(idx), stride))
        img, msk = _expected(name, tuple(idx[k] for k in keep), tuple(out_hw), with_mask, defect)
        calls.append((value, keep, img, msk))
    return calls
