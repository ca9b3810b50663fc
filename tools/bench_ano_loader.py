"""A/B of the anomalous-set slice loader on one device, in one process: 256 x 256 planes, CenterCrop((175, 240)) -> 256 x 256, image
and mask, at 4, 40 and 256 slices of one resident volume,
  (a) host      the path `AnomalousMRIDataset` replaces: per slice and per mask slice a numpy cut, Pillow (fromarray "F", crop,
                resize BILINEAR), Normalize / `> 0` in torch on the host, then one host-to-device copy of each stack; wall time ending
                in a synchronise.  Without Pillow this leg is reported as absent.
  (b) composed  the entry points the library had before, on the device: torch indexing for the gather and the crop,
                anoddpm_resize_bilinear_pil (two launches, image and mask each), a torch compare for the mask; HIP events
  (c) fused     anoddpm_ano_slices, one launch; HIP events.  Also its bytes (the cropped windows read once, both outputs written once)
                over its time as a share of the HBM peak, and the wall time of `get_slices` (index upload + launch + synchronise).
The legs alternate inside every repetition after a warm-up; (b) and (c) (and (a), with Pillow) are compared bit for bit before anything
is timed.  Reported: median, min, quartiles and max per leg.  The bar: the median of (c) is at most the median of (b) at 40 and 256
slices, with no margin but the spread printed next to it.

    python tools/bench_ano_loader.py [--reps 20] [--warmup 3] [--out profiles/ano_loader_ab.txt]"""
import argparse
import ctypes
import os
import platform
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
PLANE, CROP, OUT, S = (256, 256), (175, 240), (256, 256), 256


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:9.4f} ms   min {s['min']:9.4f}   q25 {s['q25']:9.4f}   q75 {s['q75']:9.4f}   max {s['max']:9.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_ano_loader.py measures on the device: no GPU visible")
    try:
        import PIL
        from PIL import Image
    except ImportError:
        PIL = Image = None
    from anoddpm_amd import _lib
    from anoddpm_amd import dataset as D
    from anoddpm_amd._lib import AnoSlicesArgs, ResizeArgs, current_stream, lib
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(77)
    vol = rng.random_sample((S,) + PLANE).astype(np.float32)
    yy, xx = np.mgrid[0:PLANE[0], 0:PLANE[1]]
    msk = np.stack([((yy - 120 - s % 9) ** 2 + (xx - 130 + s % 7) ** 2 < (20 + s % 31) ** 2) for s in range(S)]).astype(np.float32)
    pl, pt, ct, cl = D.center_crop_geometry_hw(*PLANE, *CROP)
    assert (pl, pt) == (0, 0)
    ch, cw = CROP
    lines = [f"AnomalousMRIDataset slices: {PLANE[0]} x {PLANE[1]} planes, CenterCrop({ch}, {cw}) -> {OUT[0]} x {OUT[1]}, image and mask; host path against the "
             f"composed and the fused device paths, same process, legs alternating, {args.reps} repetitions after {args.warmup} warm-up",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}; Pillow {PIL.__version__ if PIL else 'absent'}",
             f"HBM peak used for the share below: {HBM_PEAK / 1e12:.1f} TB/s", ""]
    if Image is None:
        lines += ["(a) host leg: absent (Pillow is not installed here)", ""]
    missed = []
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "raw_cleaned"))
        os.makedirs(os.path.join(root, "mask"))
        np.save(os.path.join(root, "raw_cleaned", "00001.npy"), vol)
        np.save(os.path.join(root, "mask", "00001.npy"), msk)
        ds = D.AnomalousMRIDataset(root, img_size=OUT, slice_selection="iterateKnown", device=dev, slices={"00001": (0, S - 1)})
        vol_d, msk_d = ds._volume(0), ds._mask(0)
        kx, xmin, xn, kmx, ky, ymin, yn, kmy = ds._tables()
        for n in (4, 40, 256):
            idx = [(7 * k + 3) % S for k in range(n)] if n < S else list(range(S))
            idx_d = torch.tensor(idx, dtype=torch.int64, device=dev)
            sl_d = idx_d.to(torch.int32)
            vp = torch.full((n,), vol_d.data_ptr(), dtype=torch.int64, device=dev)
            mp = torch.full((n,), msk_d.data_ptr(), dtype=torch.int64, device=dev)
            img = torch.empty((n,) + OUT, dtype=torch.float32, device=dev)
            mask = torch.empty((n,) + OUT, dtype=torch.float32, device=dev)
            a = AnoSlicesArgs()
            a.vols, a.masks, a.slice_idx, a.img, a.mask = vp.data_ptr(), mp.data_ptr(), sl_d.data_ptr(), img.data_ptr(), mask.data_ptr()
            a.kx, a.kx_min, a.kx_n, a.ky, a.ky_min, a.ky_n = kx.data_ptr(), xmin.data_ptr(), xn.data_ptr(), ky.data_ptr(), ymin.data_ptr(), yn.data_ptr()
            a.n, a.R, a.C, a.crop_h, a.crop_w, a.crop_top, a.crop_left = n, PLANE[0], PLANE[1], ch, cw, ct, cl
            a.out_h, a.out_w, a.kmax_x, a.kmax_y, a.mean, a.std = OUT[0], OUT[1], kmx, kmy, 0.5, 0.5

            def fused():
                _lib.check(lib().anoddpm_ano_slices(ctypes.byref(a), current_stream()), "ano_slices")
                return img, mask

            def composed():
                res = []
                for src in (vol_d, msk_d):
                    crop = src[idx_d][:, ct:ct + ch, cl:cl + cw].contiguous()
                    tmp = torch.empty((n, ch, OUT[1]), dtype=torch.float32, device=dev)
                    o = torch.empty((n,) + OUT, dtype=torch.float32, device=dev)
                    r = ResizeArgs()
                    r.inp, r.tmp, r.out = crop.data_ptr(), tmp.data_ptr(), o.data_ptr()
                    r.kx, r.kx_min, r.kx_n, r.ky, r.ky_min, r.ky_n = kx.data_ptr(), xmin.data_ptr(), xn.data_ptr(), ky.data_ptr(), ymin.data_ptr(), yn.data_ptr()
                    r.B, r.in_h, r.in_w, r.out_h, r.out_w, r.kmax_x, r.kmax_y = n, ch, cw, OUT[0], OUT[1], kmx, kmy
                    r.mean, r.std, r.normalize = 0.5, 0.5, 1
                    _lib.check(lib().anoddpm_resize_bilinear_pil(ctypes.byref(r), current_stream()), "resize_bilinear_pil")
                    res.append(o)
                return res[0], (res[1] > 0).float()

            def host():
                outs = []
                for src in (vol, msk):
                    stack = torch.empty((n,) + OUT)
                    for k, s in enumerate(idx):
                        im = Image.fromarray(src[s].reshape(PLANE).astype(np.float32))
                        im = im.crop((cl, ct, cl + cw, ct + ch)).resize((OUT[1], OUT[0]), Image.BILINEAR)
                        stack[k] = (torch.from_numpy(np.array(im)) - 0.5) / 0.5
                    outs.append(stack)
                res = outs[0].to(dev), (outs[1] > 0).float().to(dev)
                torch.cuda.synchronize()
                return res

            def method():
                res = ds.get_slices(0, idx)
                torch.cuda.synchronize()
                return res

            f_img, f_mask = (t.clone() for t in fused())
            for name, leg in (("composed", composed), ("get_slices", method)) + ((("host", host),) if Image else ()):
                g_img, g_mask = leg()
                assert torch.equal(g_img.view(torch.int32), f_img.view(torch.int32)) and torch.equal(g_mask, f_mask), (n, name)
            for _ in range(args.warmup):
                if Image:
                    host()
                composed(), fused(), method()
            t = {k: [] for k in ("host", "composed", "fused", "get_slices")}
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            for _ in range(args.reps):
                if Image:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    host()
                    t["host"].append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                e[0].record()
                composed()
                e[1].record()
                torch.cuda.synchronize()
                e[2].record()
                fused()
                e[3].record()
                torch.cuda.synchronize()
                t["composed"].append(e[0].elapsed_time(e[1]))
                t["fused"].append(e[2].elapsed_time(e[3]))
                t0 = time.perf_counter()
                method()
                t["get_slices"].append((time.perf_counter() - t0) * 1e3)
            st = {k: stats(v) for k, v in t.items() if v}
            nbytes = n * 2 * (ch * cw + OUT[0] * OUT[1]) * 4
            tf = st["fused"]["median"] * 1e-3
            lines.append(f"{n} slices (image + mask): all legs equal bit for bit")
            if Image:
                lines.append(f"  (a) host: numpy cut + Pillow + H2D, wall                {fmt(st['host'])}")
            lines += [f"  (b) composed: older entry points + torch, HIP events    {fmt(st['composed'])}",
                      f"  (c) fused: anoddpm_ano_slices, one launch, HIP events   {fmt(st['fused'])}",
                      f"      {nbytes / 1e6:.2f} MB needed = {nbytes / tf / 1e9:.0f} GB/s, {nbytes / tf / HBM_PEAK:.1%} of the HBM peak",
                      f"      get_slices (index upload + launch + synchronise), wall {fmt(st['get_slices'])}",
                      f"  ratio of medians (b) / (c): {st['composed']['median'] / st['fused']['median']:.2f}x"
                      + (f"; (a) / get_slices: {st['host']['median'] / st['get_slices']['median']:.0f}x" if Image else ""), ""]
            if n >= 40 and st["fused"]["median"] > st["composed"]["median"]:
                missed.append(f"{n} slices")
    lines.append("bar (c) <= (b) at 40 and 256 slices: " + ("MISSED at " + ", ".join(missed) if missed else "met"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
