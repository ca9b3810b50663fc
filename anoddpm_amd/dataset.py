"""`MRIDataset` -- the reference's healthy-MRI slice loader (dataset.py:575-643) with the per-sample work on the MI355X.

Kept from the reference: constructor signature, `__len__`, `__getitem__(idx) -> {"image": [1,H,W] float tensor in [-1,1],
"filenames": name}`, the `.npy` cache next to each volume, `random_slice` drawing `random.randint(40, 100)`, and the default
transform RandomAffine(3, translate=(0.02, 0.09)) -> CenterCrop(235) -> Resize(img_size, BILINEAR) -> ToTensor ->
Normalize(0.5, 0.5) -- which upstream builds from torchvision (not installed here): its arithmetic is Pillow's and is
restated in csrc/loader.hip (bit-identical to Pillow 12), the parameter glue follows torchvision's functional.py.

MI355X-first: every volume is uploaded ONCE and stays resident in HBM (a normalised fp32 volume is 40 MB; the whole NFBS
set is ~5 GB of the 288 GB), a slice never touches the host again, and a whole batch costs three launches (`get_batch`).
A user-supplied `transform` callable is honoured the reference's way (it receives the numpy slice on the host).
NIfTI input needs nibabel exactly like upstream; without it only the `.npy` cache path works.

`AnomalousMRIDataset` -- the reference's test-set loader (dataset.py:646-790) the same way: volumes and masks resident, one launch
per sample for all its slices, image and mask (anoddpm_ano_slices); the slice table comes from the caller or `slices.json`.
"""
import ctypes
import os
import random

import numpy as np
import torch

from . import _lib
from ._lib import AnoSlicesArgs, MriSliceArgs, ResizeArgs, check, current_stream, lib

__all__ = ["MRIDataset", "AnomalousMRIDataset", "normalise_volume", "resize_coeffs", "center_crop_geometry", "center_crop_geometry_hw",
           "affine_fixed_coeffs", "cycle", "init_dataset_loader"]

CROP = 235


def resize_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs (bilinear) as (k [out][kmax] fp64, kmin, kn): host side, once per size pair."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    kmax = int(np.ceil(support)) * 2 + 1
    k = np.zeros((out_size, kmax), dtype=np.float64)
    kmin = np.zeros(out_size, dtype=np.int32)
    kn = np.zeros(out_size, dtype=np.int32)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ww = 0.0
        for x in range(xmax):
            v = (x + xmin - center + 0.5) * ss
            w = 1.0 - abs(v) if abs(v) < 1.0 else 0.0
            k[xx, x] = w
            ww += w
        if ww != 0.0:
            k[xx, :xmax] /= ww
        kmin[xx], kn[xx] = xmin, xmax
    return k, kmin, kn


def center_crop_geometry(h, w, crop):
    """torchvision center_crop: (pad_left, pad_top, crop_top, crop_left)."""
    pad_left = (crop - w) // 2 if crop > w else 0
    pad_top = (crop - h) // 2 if crop > h else 0
    pad_right = (crop - w + 1) // 2 if crop > w else 0
    pad_bottom = (crop - h + 1) // 2 if crop > h else 0
    H, W = h + pad_top + pad_bottom, w + pad_left + pad_right
    return pad_left, pad_top, int(round((H - crop) / 2.0)), int(round((W - crop) / 2.0))


def center_crop_geometry_hw(h, w, crop_h, crop_w):
    """torchvision center_crop to a (crop_h, crop_w) window: (pad_left, pad_top, crop_top, crop_left).  Zero padding of
    (c - s) // 2 before and (c - s + 1) // 2 after where the image is smaller, then the window at int(round((S - c) / 2.0)) of the
    padded size S: Python's round, half to even (a difference of 1 gives 0, of 3 gives 2)."""
    pad_left = (crop_w - w) // 2 if crop_w > w else 0
    pad_top = (crop_h - h) // 2 if crop_h > h else 0
    pad_right = (crop_w - w + 1) // 2 if crop_w > w else 0
    pad_bottom = (crop_h - h + 1) // 2 if crop_h > h else 0
    H, W = h + pad_top + pad_bottom, w + pad_left + pad_right
    return pad_left, pad_top, int(round((H - crop_h) / 2.0)), int(round((W - crop_w) / 2.0))


def affine_fixed_coeffs(w, h, angle, translate):
    """torchvision's inverse affine matrix (centre = image centre, scale 1, no shear) as Pillow's six 16.16 coefficients."""
    import math
    rot = math.radians(angle)
    cx, cy = w * 0.5, h * 0.5
    tx, ty = translate
    a, b, c, d = math.cos(rot), -math.sin(rot), math.sin(rot), math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def _uniform(lo, hi):
    """One draw from torch's CPU generator, the way torchvision's RandomAffine.get_params draws."""
    return float(torch.empty(1).uniform_(float(lo), float(hi)).item())


def normalise_volume(volume, device):
    """dataset.py:585-592 on the device: returns the normalised fp32 volume (device tensor, same shape)."""
    v = torch.as_tensor(np.ascontiguousarray(volume, dtype=np.float64)).to(device)
    _lib.require_cuda(v, "normalise_volume")
    out = torch.empty(v.shape, dtype=torch.float32, device=v.device)
    ws = torch.empty(2 * 256 + 4, dtype=torch.float64, device=v.device)
    check(lib().anoddpm_volume_normalise(v.data_ptr(), v.numel(), out.data_ptr(), ws.data_ptr(), current_stream()), "volume_normalise")
    return out


class MRIDataset(torch.utils.data.Dataset):
    """Healthy MRI dataset (dataset.py:575-643)."""

    def __init__(self, ROOT_DIR, transform=None, img_size=(32, 32), random_slice=False, device=None, augment=True):
        self.transform = transform
        self.img_size = tuple(int(v) for v in img_size)
        self.filenames = os.listdir(ROOT_DIR)
        if ".DS_Store" in self.filenames:
            self.filenames.remove(".DS_Store")
        self.ROOT_DIR = ROOT_DIR
        self.random_slice = random_slice
        self.augment = augment
        # default: the CALLING process's current device (one process per GPU sets it with torch.cuda.set_device(local_rank));
        # a hard-wired cuda:0 would make ranks > 0 upload their volumes to, and launch on, somebody else's GPU
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda:0")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self._vols = {}
        self._coef = {}

    def __len__(self):
        return len(self.filenames)

    # ---- volumes: one upload each, resident afterwards
    def _volume(self, name):
        v = self._vols.get(name)
        if v is not None:
            return v
        npy = os.path.join(self.ROOT_DIR, name, f"{name}.npy")
        if os.path.exists(npy):
            v = torch.from_numpy(np.ascontiguousarray(np.load(npy), dtype=np.float32)).to(self.device)
        else:
            nii = os.path.join(self.ROOT_DIR, name, f"sub-{name}_ses-NFB3_T1w.nii.gz")
            try:
                import nibabel as nib
            except ImportError as e:
                raise _lib.AnoddpmError(f"{npy} is missing and reading {nii} needs nibabel (as upstream does)") from e
            v = normalise_volume(nib.load(nii).get_fdata(), self.device)
            np.save(npy, v.cpu().numpy())                                    # dataset.py:591-595
        if v.dim() != 3:
            raise ValueError(f"{name}: expected a 3-D volume, got shape {tuple(v.shape)}")
        self._vols[name] = v
        return v

    def _tables(self, in_h, in_w):
        key = (in_h, in_w, self.img_size)
        t = self._coef.get(key)
        if t is None:
            kx, xmin, xn = resize_coeffs(in_w, self.img_size[1])
            ky, ymin, yn = resize_coeffs(in_h, self.img_size[0])
            up = lambda a: torch.from_numpy(a).to(self.device)
            t = self._coef[key] = (up(kx), up(xmin), up(xn), kx.shape[1], up(ky), up(ymin), up(yn), ky.shape[1])
        return t

    def _draw(self, idx):
        """The host-side random draws of one sample, in the reference's order: slice index, then RandomAffine's three."""
        if torch.is_tensor(idx):
            idx = idx.tolist()
        name = self.filenames[idx]
        vol = self._volume(name)
        slice_idx = random.randint(40, 100) if self.random_slice else 80
        aff = None
        if self.augment and self.transform is None:
            X, Z = vol.shape[0], vol.shape[2]
            angle = _uniform(-3.0, 3.0)
            max_dx, max_dy = float(0.02 * Z), float(0.09 * X)
            tx = int(round(_uniform(-max_dx, max_dx)))
            ty = int(round(_uniform(-max_dy, max_dy)))
            aff = affine_fixed_coeffs(Z, X, angle, (tx, ty))
        return name, vol, slice_idx, aff

    def get_batch(self, indices):
        """[B,1,H,W] device tensor + the file names: the default pipeline for a whole batch in three launches."""
        if self.transform is not None:
            items = [self[i] for i in indices]
            return torch.stack([it["image"] for it in items]), [it["filenames"] for it in items]
        with torch.cuda.device(self.device):                                 # launches go to THIS dataset's device and its stream
            return self._get_batch_on_device(indices)

    def _get_batch_on_device(self, indices):
        draws = [self._draw(i) for i in indices]
        B = len(draws)
        X, Z = draws[0][1].shape[0], draws[0][1].shape[2]
        if any(d[1].shape[0] != X or d[1].shape[2] != Z for d in draws):
            raise ValueError("volumes of one batch must share their first and last dimensions")
        dev = self.device
        vols = torch.tensor([d[1].data_ptr() for d in draws], dtype=torch.int64).to(dev)
        ydim = torch.tensor([d[1].shape[1] for d in draws], dtype=torch.int32).to(dev)
        sl = torch.tensor([d[2] for d in draws], dtype=torch.int32).to(dev)
        for d in draws:
            if not 0 <= d[2] < d[1].shape[1]:
                raise IndexError(f"slice {d[2]} is outside volume {d[0]} with {d[1].shape[1]} slices")
        aff = None
        if draws[0][3] is not None:
            aff = torch.tensor([d[3] for d in draws], dtype=torch.int64).to(dev)
        pl, pt, ct, cl = center_crop_geometry(X, Z, CROP)
        crop = torch.empty((B, CROP, CROP), dtype=torch.float32, device=dev)
        a = MriSliceArgs()
        a.vols, a.ydim, a.slice_idx, a.affine, a.out = vols.data_ptr(), ydim.data_ptr(), sl.data_ptr(), (aff.data_ptr() if aff is not None else None), crop.data_ptr()
        a.B, a.X, a.Z, a.crop, a.pad_left, a.crop_top = B, X, Z, CROP, pl - cl, ct - pt
        check(lib().anoddpm_mri_slice_prepare(ctypes.byref(a), current_stream()), "mri_slice_prepare")
        kx, xmin, xn, kmx, ky, ymin, yn, kmy = self._tables(CROP, CROP)
        H, W = self.img_size
        tmp = torch.empty((B, CROP, W), dtype=torch.float32, device=dev)
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        r = ResizeArgs()
        r.inp, r.tmp, r.out = crop.data_ptr(), tmp.data_ptr(), out.data_ptr()
        r.kx, r.kx_min, r.kx_n, r.ky, r.ky_min, r.ky_n = kx.data_ptr(), xmin.data_ptr(), xn.data_ptr(), ky.data_ptr(), ymin.data_ptr(), yn.data_ptr()
        r.B, r.in_h, r.in_w, r.out_h, r.out_w, r.kmax_x, r.kmax_y = B, CROP, CROP, H, W, kmx, kmy
        r.mean, r.std, r.normalize = 0.5, 0.5, 1
        check(lib().anoddpm_resize_bilinear_pil(ctypes.byref(r), current_stream()), "resize_bilinear_pil")
        return out, [d[0] for d in draws]

    def __getitem__(self, idx):
        if self.transform is not None:                                       # the reference's contract: numpy slice in, anything out
            with torch.cuda.device(self.device):
                name, vol, slice_idx, _ = self._draw(idx)
            image = vol[:, slice_idx:slice_idx + 1, :].reshape(vol.shape[0], vol.shape[2]).cpu().numpy()
            return {"image": self.transform(image), "filenames": name}
        out, names = self.get_batch([idx])
        return {"image": out[0], "filenames": names[0]}


ANO_CROP = (175, 240)
SLICE_SELECTIONS = ("random", "iterateKnown", "iterateKnown_restricted", "iterateUnknown")


def _slice_table(ROOT_DIR, slices):
    """id -> range from the caller's mapping or {ROOT_DIR}/slices.json; values are ranges or (start, stop) pairs."""
    if slices is None:
        path = os.path.join(ROOT_DIR, "slices.json")
        if not os.path.exists(path):
            raise _lib.AnoddpmError(
                f"AnomalousMRIDataset needs the tumour slice range of every volume: pass slices={{id: range(start, stop)}} (or "
                f"(start, stop) pairs), or put them into {path} as {{\"id\": [start, stop]}}; upstream's table is at dataset.py:675-682")
        import json
        with open(path) as f:
            slices = json.load(f)
    if not hasattr(slices, "items") or len(slices) == 0:
        raise _lib.AnoddpmError("AnomalousMRIDataset: slices must be a non-empty mapping id -> range or (start, stop)")
    table = {}
    for name, r in slices.items():
        if not isinstance(r, range):
            try:
                start, stop = (int(v) for v in r)
            except (TypeError, ValueError) as e:
                raise _lib.AnoddpmError(f"AnomalousMRIDataset: slices[{name!r}] = {r!r} is neither a range nor (start, stop)") from e
            r = range(start, stop)
        if r.step != 1 or r.start < 0 or r.stop < r.start:
            raise _lib.AnoddpmError(f"AnomalousMRIDataset: slices[{name!r}] = {r!r} is not an ascending unit-step range")
        table[str(name)] = r
    return table


class AnomalousMRIDataset(torch.utils.data.Dataset):
    """Anomalous MRI dataset (dataset.py:646-790): tumour volumes `{ROOT}/raw_cleaned/{id}.npy` (`raw/` with cleaned=False) and
    masks `{ROOT}/mask/{id}.npy`, sliced along axis 0, through CenterCrop((175, 240)) -> Resize(img_size, BILINEAR) -> ToTensor ->
    Normalize(0.5, 0.5); the mask goes through the same transform and is then `> 0`.

    Kept from the reference: the file layout (`-resized.npy` variants with resized=True where they exist), `filenames`, `slices`,
    `img_size`, `slice_selection`, `__len__`, the four modes with their index rules and the sample dict (`"slices"` has upstream's
    type per mode).  Not kept: the slice table itself -- it comes from `slices=` or `{ROOT}/slices.json` -- and the NIfTI branch
    (upstream's names always end in .npy, so its nib.load cannot succeed): a missing file raises AnoddpmError naming the path.

    MI355X-first: every volume and mask is uploaded once (astype(float32)) and stays in HBM; one `__getitem__` of any mode costs one
    upload of its pointers and slice indices and ONE launch (anoddpm_ano_slices) for all slices, image and mask.  `image` / `mask`
    are [n, H, W] device tensors ([1, H, W] for "random").  A user `transform` is honoured upstream's way (numpy slice in, host)."""

    def __init__(self, ROOT_DIR, transform=None, img_size=(32, 32), slice_selection="random", resized=False, cleaned=True, device=None,
                 slices=None):
        if slice_selection not in SLICE_SELECTIONS:
            raise ValueError(f"slice_selection {slice_selection!r} is none of {SLICE_SELECTIONS}")
        self.transform = transform
        self.img_size = tuple(int(v) for v in img_size)
        self.resized = resized
        self.slices = _slice_table(ROOT_DIR, slices)
        self._ids = list(self.slices)
        self.filenames = [f"{ROOT_DIR}/{'raw_cleaned' if cleaned else 'raw'}/{name}.npy" for name in self._ids]
        self.ROOT_DIR = ROOT_DIR
        self.slice_selection = slice_selection
        if device is None:                                                   # as MRIDataset: the calling process's current device
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda:0")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self._vols = {}
        self._coef = {}

    def __len__(self):
        return len(self.filenames)

    # ---- volumes and masks: one upload each, resident afterwards
    def _resident(self, path):
        v = self._vols.get(path)
        if v is None:
            if not os.path.exists(path):
                raise _lib.AnoddpmError(f"{path} is missing (AnomalousMRIDataset reads .npy volumes only)")
            v = torch.from_numpy(np.ascontiguousarray(np.load(path), dtype=np.float32)).to(self.device)
            if v.dim() != 3:
                raise ValueError(f"{path}: expected a 3-D volume, got shape {tuple(v.shape)}")
            self._vols[path] = v
        return v

    def _volume(self, idx):
        path = self.filenames[idx]
        alt = f"{path[:-4]}-resized.npy"
        return self._resident(alt if self.resized and os.path.exists(alt) else path)

    def _mask(self, idx):
        path = f"{self.ROOT_DIR}/mask/{self._ids[idx]}.npy"
        alt = f"{path[:-4]}-resized.npy"
        m = self._resident(alt if self.resized and os.path.exists(alt) else path)
        if m.shape != self._volume(idx).shape:
            raise ValueError(f"{path}: mask shape {tuple(m.shape)} is not the volume's {tuple(self._volume(idx).shape)}")
        return m

    def _tables(self):
        key = self.img_size
        t = self._coef.get(key)
        if t is None:
            kx, xmin, xn = resize_coeffs(ANO_CROP[1], self.img_size[1])
            ky, ymin, yn = resize_coeffs(ANO_CROP[0], self.img_size[0])
            up = lambda a: torch.from_numpy(a).to(self.device)
            t = self._coef[key] = (up(kx), up(xmin), up(xn), kx.shape[1], up(ky), up(ymin), up(yn), ky.shape[1])
        return t

    def _launch(self, vols, masks, slice_idx):
        """One upload (pointers and slice indices in one buffer) and one launch: vols / masks are lists of resident volumes of one
        plane shape, masks may be None.  -> (img [n,H,W], mask [n,H,W] or None)."""
        n = len(vols)
        R, C = int(vols[0].shape[1]), int(vols[0].shape[2])
        for v in vols:
            _lib.require_cuda(v, "AnomalousMRIDataset")
        host = np.zeros(2 * n + (n + 1) // 2, dtype=np.int64)
        host[:n] = [v.data_ptr() for v in vols]
        if masks is not None:
            host[n:2 * n] = [m.data_ptr() for m in masks]
        host[2 * n:].view(np.int32)[:n] = slice_idx
        with torch.cuda.device(self.device):                                 # launches go to THIS dataset's device and its stream
            buf = torch.from_numpy(host).to(self.device)
            kx, xmin, xn, kmx, ky, ymin, yn, kmy = self._tables()
            H, W = self.img_size
            img = torch.empty((n, H, W), dtype=torch.float32, device=self.device)
            mask = torch.empty((n, H, W), dtype=torch.float32, device=self.device) if masks is not None else None
            pl, pt, ct, cl = center_crop_geometry_hw(R, C, *ANO_CROP)
            a = AnoSlicesArgs()
            a.vols, a.masks, a.slice_idx = buf.data_ptr(), (buf.data_ptr() + 8 * n if masks is not None else None), buf.data_ptr() + 16 * n
            a.img, a.mask = img.data_ptr(), (mask.data_ptr() if mask is not None else None)
            a.kx, a.kx_min, a.kx_n, a.ky, a.ky_min, a.ky_n = kx.data_ptr(), xmin.data_ptr(), xn.data_ptr(), ky.data_ptr(), ymin.data_ptr(), yn.data_ptr()
            a.n, a.R, a.C, a.crop_h, a.crop_w, a.crop_top, a.crop_left = n, R, C, ANO_CROP[0], ANO_CROP[1], ct - pt, cl - pl
            a.out_h, a.out_w, a.kmax_x, a.kmax_y, a.mean, a.std = H, W, kmx, kmy, 0.5, 0.5
            check(lib().anoddpm_ano_slices(ctypes.byref(a), current_stream()), "ano_slices")
        return img, mask

    def _items(self, pairs, with_mask):
        """pairs: (volume index, slice index).  Checks the indices, then one launch."""
        if len(pairs) == 0:
            raise ValueError("AnomalousMRIDataset: no slices asked for")
        vol_of = {i: self._volume(i) for i in dict.fromkeys(i for i, _ in pairs)}        # each volume looked up once, not once per slice
        vols = [vol_of[i] for i, _ in pairs]
        for (i, s), v in zip(pairs, vols):
            if not 0 <= s < v.shape[0]:
                raise IndexError(f"slice {s} is outside volume {self.filenames[i]} with {v.shape[0]} slices")
        if any(v.shape[1:] != vols[0].shape[1:] for v in vol_of.values()):
            raise ValueError("volumes of one batch must share their plane shape")
        masks = None
        if with_mask:
            mask_of = {i: self._mask(i) for i in vol_of}
            masks = [mask_of[i] for i, _ in pairs]
        return self._launch(vols, masks, np.array([s for _, s in pairs], dtype=np.int32))

    def _host_slices(self, idx, slice_indices, with_mask):
        """The reference's loop for a user transform: the numpy slice goes in on the host, the results fill torch.empty(n, *img_size)."""
        vol = self._volume(idx).cpu().numpy()
        msk = self._mask(idx).cpu().numpy() if with_mask else None
        out = torch.empty(len(slice_indices), *self.img_size)
        out_mask = torch.empty(len(slice_indices), *self.img_size) if with_mask else None
        for k, s in enumerate(slice_indices):
            if not 0 <= s < vol.shape[0]:
                raise IndexError(f"slice {s} is outside volume {self.filenames[idx]} with {vol.shape[0]} slices")
            out[k, ...] = torch.as_tensor(self.transform(vol[s]))
            if with_mask:
                out_mask[k, ...] = torch.as_tensor(self.transform(msk[s]))
        return out, ((out_mask > 0).float() if with_mask else None)

    def get_slices(self, idx, slice_indices, with_mask=True):
        """(image [n,H,W], mask [n,H,W] of 0/1 or None) of the listed slices of volume idx: the primitive of every mode."""
        if torch.is_tensor(idx):
            idx = idx.tolist()
        slice_indices = [int(s) for s in slice_indices]
        if self.transform is not None:
            return self._host_slices(idx, slice_indices, with_mask)
        return self._items([(idx, s) for s in slice_indices], with_mask)

    def get_batch(self, indices):
        """"random" over several volumes (which must share R and C) in one launch: {"image": [B,1,H,W], "slices": [B ints],
        "filenames": [B names]}; one random.randint per index, in order."""
        indices = [i.tolist() if torch.is_tensor(i) else i for i in indices]
        draws = [random.randint(self.slices[self._ids[i]].start, self.slices[self._ids[i]].stop) for i in indices]
        if self.transform is not None:
            image = torch.stack([self._host_slices(i, [s], False)[0] for i, s in zip(indices, draws)])
        else:
            image = self._items(list(zip(indices, draws)), False)[0][:, None]
        return {"image": image, "slices": draws, "filenames": [self.filenames[i] for i in indices]}

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.tolist()
        temp_range = self.slices[self._ids[idx]]
        sample = {}
        if self.slice_selection == "random":
            slice_idx = random.randint(temp_range.start, temp_range.stop)    # :732, the stop is inclusive
            if self.transform is not None:                                   # :733-735, the transform's result as it is
                vol = self._volume(idx)
                if not 0 <= slice_idx < vol.shape[0]:
                    raise IndexError(f"slice {slice_idx} is outside volume {self.filenames[idx]} with {vol.shape[0]} slices")
                image = self.transform(vol[slice_idx].cpu().numpy())
            else:
                image = self.get_slices(idx, [slice_idx], with_mask=False)[0]
            sample["slices"] = slice_idx
        elif self.slice_selection == "iterateKnown":
            image, sample["mask"] = self.get_slices(idx, temp_range)
            sample["slices"] = temp_range
        elif self.slice_selection == "iterateKnown_restricted":
            slices = np.linspace(temp_range.start + 5, temp_range.stop - 5, 4).astype(np.int32)      # :761
            image, sample["mask"] = self.get_slices(idx, slices)
            sample["slices"] = slices
        else:                                                                # "iterateUnknown": the whole volume, no mask
            n = int(self._volume(idx).shape[0])
            image = self.get_slices(idx, range(n), with_mask=False)[0]
            sample["slices"] = n
        sample["image"] = image
        sample["filenames"] = self.filenames[idx]
        return sample


def cycle(iterable):
    """dataset.py:13-16"""
    while True:
        for x in iterable:
            yield x


def init_dataset_loader(mri_dataset, args, shuffle=True):
    """dataset.py:361-370: an endless DataLoader; samples are device tensors already, so no workers / pinning."""
    return cycle(torch.utils.data.DataLoader(mri_dataset, batch_size=args["Batch_Size"], shuffle=shuffle, num_workers=0, drop_last=True))
