"""Writes tests/golden/loader_kat.npz: Pillow's own outputs on the cases of tests/loader_cases.py, so that a machine without Pillow
can still hold the numpy oracle (oracle/loader_oracle.py) and the device loader to them.  Run by hand:
    python tests/golden/make_loader_golden.py
Inputs are not stored; they are regenerated from their seeds and the fixture pins 64 bits of their SHA-256.

Slice preparation (every case of `loader_cases.PREPARE_CASES`, every item): the slice as a mode-"F" image through
Image.transform((w, h), AFFINE, the six floats of the inverse matrix, NEAREST, fillcolor=0), then torchvision CenterCrop's zero
padding (Image.new + paste) and Image.crop.  Stored: 64 bits of the SHA-256 of the affine output (`prep_affine_sum`) and of the
235 x 235 crop (`prep_crop_sum`), [case][item]; and of two affine sets per geometry ("none" and "rot+3_t++") every PROBE-th pixel
of item 1's crop (`prep_probe_<geometry>_<set>`).

Resizing (every case of `loader_cases.RESIZE_CASES`, every item): Image.resize((out_w, out_h), BILINEAR).  Stored: the 64-bit sums
(`resize_sum`, [case][item]); item 0 in full where the output is at most 64 x 64 (`resize_<case>`), every PROBE-th pixel of item 0
otherwise (`resize_probe_<case>`).

`produced_with` is the Pillow version string.  Nothing here reads the reference project."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import loader_cases as lc  # noqa: E402

PROBE = 211
PROBED_SETS = ("none", "rot+3_t++")
LIMIT = 108 * 1024


def as_image(a):
    """torchvision ToPILImage of a float32 2-D array: mode "F"."""
    im = Image.fromarray(np.ascontiguousarray(a, dtype=np.float32))
    assert im.mode == "F" and im.size == (a.shape[1], a.shape[0])
    return im


def pil_affine(img, m):
    h, w = img.shape
    return np.array(as_image(img).transform((w, h), Image.AFFINE, tuple(m), Image.NEAREST, fillcolor=0))


def pil_center_crop(img, geom, crop=lc.CROP):
    """torchvision.transforms.functional.center_crop on a PIL image: pad with zeros where it is smaller, then crop."""
    h, w = img.shape
    pl, pt, ct, cl = geom
    pr = (crop - w + 1) // 2 if crop > w else 0
    pb = (crop - h + 1) // 2 if crop > h else 0
    padded = Image.new("F", (w + pl + pr, h + pt + pb), 0.0)
    padded.paste(as_image(img), (pl, pt))
    return np.array(padded.crop((cl, ct, cl + crop, ct + crop)))


def pil_resize(img, oh, ow):
    return np.array(as_image(img).resize((ow, oh), Image.BILINEAR))


def pil_prepare(case, b):
    """(after the affine, after the centre crop) of item b, by Pillow."""
    v, s = case["items"][b]
    img = np.ascontiguousarray(case["vols"][v][:, s, :])
    aff = img if case["matrices"] is None else pil_affine(img, case["matrices"][b])
    return aff, pil_center_crop(aff, case["geom"])


def probe(a):
    return a.reshape(-1)[::PROBE].copy()


def main():
    out = {"produced_with": np.array(f"Pillow {PIL.__version__}"), "probe_stride": np.int64(PROBE)}
    out["prep_cases"] = np.array([f"{g}/{a}" for g, a in lc.PREPARE_CASES])
    out["prep_input_sum"] = np.array([[lc.checksum(v) for v in lc.geometry_volumes(g)] for g in lc.GEOMETRY_NAMES], np.uint64)
    aff_sum, crop_sum = [], []
    for g, a in lc.PREPARE_CASES:
        case = lc.prepare_case(g, a)
        stages = [pil_prepare(case, b) for b in range(len(case["items"]))]
        aff_sum.append([lc.checksum(s[0]) for s in stages])
        crop_sum.append([lc.checksum(s[1]) for s in stages])
        assert all(s[1].dtype == np.float32 and s[1].shape == (lc.CROP, lc.CROP) for s in stages)
        if a in lc.ALL_ZERO:
            assert not any(s[1].any() for s in stages), (g, a)
        if a in PROBED_SETS:
            out[f"prep_probe_{g}_{a}"] = probe(stages[1][1])
    out["prep_affine_sum"], out["prep_crop_sum"] = np.array(aff_sum, np.uint64), np.array(crop_sum, np.uint64)

    out["resize_cases"] = np.array(lc.RESIZE_NAMES)
    out["resize_input_sum"] = np.array([lc.checksum(lc.resize_images(n)) for n in lc.RESIZE_NAMES], np.uint64)
    sums = []
    for n in lc.RESIZE_NAMES:
        _, (oh, ow) = lc.resize_case(n)
        res = [pil_resize(img, oh, ow) for img in lc.resize_images(n)]
        assert all(r.dtype == np.float32 and r.shape == (oh, ow) for r in res)
        sums.append([lc.checksum(r) for r in res])
        if oh <= 64 and ow <= 64:
            out[f"resize_{n}"] = res[0]
        else:
            out[f"resize_probe_{n}"] = probe(res[0])
    out["resize_sum"] = np.array(sums, np.uint64)

    path = os.path.join(HERE, "loader_kat.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes, {len(out)} entries; {out['produced_with']}")
    assert size < LIMIT, size


if __name__ == "__main__":
    main()
