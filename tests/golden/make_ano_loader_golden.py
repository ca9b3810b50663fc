"""Writes tests/golden/ano_loader_kat.npz and tests/golden/ano_slices.json: the reference's own `AnomalousMRIDataset`
(dataset.py:646-790) run over the synthetic data root of tests/ano_loader_cases.py, so that the numpy restatement there, and through
it the device loader, are held to what the reference yields.  Run by hand, where the reference tree and Pillow are present:
    python tests/golden/make_ano_loader_golden.py

The reference's module is imported with cv2 / nibabel / torchvision stubbed (as make_golden.gen_loader does).  Its default transform
needs torchvision, which is not installed; for this class torchvision's pipeline is a thin layer over Pillow, so the class is handed,
as its `transform=`, the callable `pil_transform` below: ToPILImage (Image.fromarray, mode "F") -> CenterCrop((175, 240)) (zero
padding by Image.new + paste, then Image.crop) -> Resize(img_size, BILINEAR) (Image.resize) -> ToTensor -> Normalize(0.5, 0.5).

ano_slices.json is the reference object's `slices` attribute dumped as data: {id: [start, stop]}.  It is written first; the cases
read it.  Then every run of `ano_loader_cases.RUNS` (mode, id, img_size, resized), through the reference's `__getitem__`
("random": RANDOM_CALLS calls under random.seed(RANDOM_SEED)); stored per run under `<run key>__<what>`:
    slices      the sample's "slices" value(s) (ano_loader_cases.slices_record), one row per call
    img_sum     64 bits of the SHA-256 of every output slice, [calls][n];  mask_sum the same of the 0/1 mask where the mode has one
    img_probe   about 200 strided elements of the first call's image;  mask_probe likewise
    img, mask   the outputs in full for the runs of `ano_loader_cases.FULL`
and `input_sum` (the volumes' and masks' checksums), `produced_with` (the Pillow version), `filenames` of the two ids."""
import importlib
import json
import os
import random
import sys
import tempfile
import types

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refimport  # noqa: E402

LIMIT = 108 * 1024
CROP = (175, 240)


def load_reference_dataset():
    saved = {k: sys.modules.get(k) for k in ("cv2", "nibabel", "torchvision", "dataset")}
    sys.modules["nibabel"] = types.ModuleType("nibabel")
    sys.modules["cv2"] = types.ModuleType("cv2")
    tv = types.ModuleType("torchvision")
    tv.datasets, tv.transforms = types.ModuleType("torchvision.datasets"), types.ModuleType("torchvision.transforms")
    sys.modules["torchvision"] = tv
    sys.path.insert(0, _refimport.REF)
    try:
        sys.modules.pop("dataset", None)
        ref = importlib.import_module("dataset")
    finally:
        sys.path.remove(_refimport.REF)
        for k, v in saved.items():
            if v is not None:
                sys.modules[k] = v
            else:
                sys.modules.pop(k, None)
    return ref


def pil_transform(img_size):
    """torchvision's pipeline of this class on one float32 plane, by Pillow: -> [1][H][W] float32 tensor."""
    ch, cw = CROP

    def transform(a):
        im = Image.fromarray(np.ascontiguousarray(a, dtype=np.float32))
        assert im.mode == "F"
        w, h = im.size
        if cw > w or ch > h:                                                # functional.center_crop: pad first where it is smaller
            pl, pt = (cw - w) // 2 if cw > w else 0, (ch - h) // 2 if ch > h else 0
            pr, pb = (cw - w + 1) // 2 if cw > w else 0, (ch - h + 1) // 2 if ch > h else 0
            padded = Image.new("F", (w + pl + pr, h + pt + pb), 0.0)
            padded.paste(im, (pl, pt))
            im = padded
            w, h = im.size
        top, left = int(round((h - ch) / 2.0)), int(round((w - cw) / 2.0))
        im = im.crop((left, top, left + cw, top + ch))
        im = im.resize((img_size[1], img_size[0]), Image.BILINEAR)
        t = torch.from_numpy(np.array(im))[None]                            # ToTensor of a mode-"F" image
        return (t - 0.5) / 0.5                                              # Normalize((0.5), (0.5))
    return transform


def main():
    ref = load_reference_dataset()
    with tempfile.TemporaryDirectory() as probe_root:
        table = ref.AnomalousMRIDataset(probe_root, transform=lambda a: a).slices
    with open(os.path.join(HERE, "ano_slices.json"), "w") as f:
        json.dump({k: [r.start, r.stop] for k, r in table.items()}, f, indent=0)
        f.write("\n")
    import ano_loader_cases as ac                                           # reads ano_slices.json
    import loader_cases as lc

    out = {"produced_with": np.array(f"Pillow {PIL.__version__}"), "runs": np.array([ac.run_key(r) for r in ac.RUNS])}
    out["input_sum"] = np.array([[lc.checksum(ac.volume(n)), lc.checksum(ac.mask(n))] for n in ac.SHAPES], np.uint64)
    with tempfile.TemporaryDirectory() as root:
        ac.write_root(root)
        names = None
        for run in ac.RUNS:
            mode, vid, size, resized = run
            ds = ref.AnomalousMRIDataset(root, transform=pil_transform(size), img_size=size, slice_selection=mode, resized=resized)
            idx = list(ds.slices).index(vid)
            names = names or [ds.filenames[list(ds.slices).index(i)][len(root):] for i in ac.IDS]
            if mode == "random":
                random.seed(ac.RANDOM_SEED)
            samples = [ds[idx] for _ in range(ac.RANDOM_CALLS if mode == "random" else 1)]
            key = ac.run_key(run)
            imgs = [np.asarray(s["image"], np.float32).reshape((-1,) + tuple(size)) for s in samples]
            assert all(s["filenames"] == ds.filenames[idx] for s in samples)
            out[f"{key}__slices"] = np.stack([ac.slices_record(s["slices"]) for s in samples])
            out[f"{key}__img_sum"] = np.array([[lc.checksum(p) for p in im] for im in imgs], np.uint64)
            out[f"{key}__img_probe"] = ac.probe(imgs[0])
            if "mask" in samples[0]:
                masks = [s["mask"].numpy() for s in samples]
                assert all(m.dtype == np.float32 and set(np.unique(m)) <= {0.0, 1.0} for m in masks)
                out[f"{key}__mask_sum"] = np.array([[lc.checksum(p) for p in m] for m in masks], np.uint64)
                out[f"{key}__mask_probe"] = ac.probe(masks[0])
            if run in ac.FULL:
                out[f"{key}__img"] = np.stack(imgs)
                if "mask" in samples[0]:
                    out[f"{key}__mask"] = np.stack(masks)
            print(key, out[f"{key}__slices"].tolist()[:1], out[f"{key}__img_sum"].shape, flush=True)
        out["filenames"] = np.array(names)
    path = os.path.join(HERE, "ano_loader_kat.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes, {len(out)} entries; {out['produced_with']}")
    assert size < LIMIT, size
    assert os.path.getsize(os.path.join(HERE, "ano_slices.json")) < LIMIT


if __name__ == "__main__":
    main()
