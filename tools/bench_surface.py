"""Cost of the distance transform and the boundary distances (anoddpm_distance_transform / anoddpm_surface_distance of
csrc/surface.hip) on one device, in one process: for (a) 1 x 256^2, (b) the 55 maps of a detection sweep with ONE shared mask and
(c) 16 x 512^2,
  1. DEVICE time of each entry point (what metrics.distance_transform / metrics.surface_distance issue) from HIP events around a
     window of back-to-back calls that lasts at least --window seconds, divided by the calls in it.  The legs alternate, the round
     is repeated --pairs times and the spread over the repetitions is reported
  2. native against host: HOST wall time of metrics.surface_distance with its results copied to the host against what a user
     had to do without it: copy the maps to the host, then per map two scipy.ndimage.binary_erosion, two
     scipy.ndimage.distance_transform_edt and numpy.percentile.  The two results are compared before anything is timed.

    python tools/bench_surface.py [--pairs 5] [--window 0.5] [--reps 10] [--out profiles/surface_ab.txt]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_surface(pred, ref):
    """One pair on the host, medpy's way: (hd, hd95, assd); NaN when a border is empty."""
    from scipy import ndimage
    p, r = pred > 0, ref > 0
    bp, br = p & ~ndimage.binary_erosion(p), r & ~ndimage.binary_erosion(r)
    if not bp.any() or not br.any():
        return float("nan"), float("nan"), float("nan")
    d_pr, d_rp = ndimage.distance_transform_edt(~br)[bp], ndimage.distance_transform_edt(~bp)[br]
    return max(d_pr.max(), d_rp.max()), np.percentile(np.hstack((d_pr, d_rp)), 95), (d_pr.mean() + d_rp.mean()) / 2


def make(S, side, shared, dev):
    """A reference of a few blobs per plane and predictions that move and fray it."""
    from scipy import ndimage
    rng = np.random.default_rng(977 + S + side)
    sigma = side / 32.0
    ref = np.stack([ndimage.gaussian_filter(rng.random((side, side)), sigma) > 0.5 for _ in range(1 if shared else S)])
    pred = np.stack([np.roll(ref[0 if shared else s], (int(rng.integers(-4, 5)), int(rng.integers(-4, 5))), (0, 1)) & (rng.random((side, side)) > 0.02)
                     for s in range(S)])
    ref = ref[0] if shared else ref
    return torch.from_numpy(pred.astype(np.float32)).to(dev), torch.from_numpy(ref.astype(np.float32)).to(dev)


def spread(x):
    x = np.sort(np.asarray(x))
    return f"median {np.median(x):9.4f} ms   min {x[0]:9.4f}   max {x[-1]:9.4f}   (max - min) / median {100 * (x[-1] - x[0]) / np.median(x):5.1f} %"


def window_ms(fn, seconds):
    """Device time of one fn(): events around back-to-back calls that fill at least `seconds`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    k = max(3, int(np.ceil(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    while True:
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= seconds * 1e3:
            return ms / k, k
        k = int(np.ceil(k * 1.3 * seconds * 1e3 / ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.window < 0.5 or args.pairs < 3:
        ap.error("--window must be at least 0.5 s and --pairs at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_surface.py measures on the device: no GPU visible")
    import scipy
    from anoddpm_amd import _lib, metrics
    dev = torch.device("cuda:0")
    lines = [f"distance transform and boundary distances, csrc/surface.hip (ABI {_lib.ABI_VERSION}): {args.pairs} alternating repetitions, "
             f"windows of at least {args.window} s of back-to-back calls, every shape warmed first",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}; scipy {scipy.__version__}",
             "host leg: D2H copy + per map two scipy.ndimage.binary_erosion, two distance_transform_edt and numpy.percentile", ""]
    shapes = (("(a) 1 x 256^2", 1, 256, False), ("(b) 55 x 256^2, one shared mask", 55, 256, True), ("(c) 16 x 512^2", 16, 512, False))
    for label, S, side, shared in shapes:
        pred, ref = make(S, side, shared, dev)

        def transform():
            return metrics.distance_transform(pred)

        def surface():
            return metrics.surface_distance(pred, ref)

        legs = [("distance transform of the S maps (two launches)  ", transform), ("boundary distances of the S pairs (four launches)", surface)]
        for _, fn in legs:                                               # warm the shape: allocator, code object, caches
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name, _ in legs}
        launches = {}
        for _ in range(args.pairs):
            for name, fn in legs:
                ms, k = window_ms(fn, args.window)
                t[name].append(ms)
                launches[name] = k
        counts = metrics.surface_distance(pred, ref)["counts"].cpu().numpy().reshape(-1, 2)
        lines.append(f"{label}: S = {S}, {side} x {side}, {int((pred > 0).sum()) // S} foreground pixels per map, borders of {int(counts[:, 0].mean())} / "
                     f"{int(counts[:, 1].mean())} pixels (prediction / reference, mean)")
        for name, _ in legs:
            lines.append(f"  DEVICE time, {name}  {spread(t[name])}   [{launches[name]} per window]")

        def host_leg():
            pk, rk = pred.cpu().numpy(), ref.cpu().numpy()
            return np.array([host_surface(pk[s], rk if shared else rk[s]) for s in range(S)])

        def native_leg():
            o = metrics.surface_distance(pred, ref)
            return torch.stack([o["hd"], o["hd95"], o["assd"]], dim=-1).cpu().numpy()

        h, d = host_leg(), native_leg()
        worst = float(np.nanmax(np.abs(h - d) / np.maximum(np.abs(h), 1.0)))
        assert worst <= 1e-12 and np.array_equal(np.isnan(h), np.isnan(d)), (label, worst)
        th, tn = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_leg()
            th.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            native_leg()
            tn.append((time.perf_counter() - t0) * 1e3)
        lines += [f"  pair 0: HD {d[0, 0]:.4f}  HD95 {d[0, 1]:.4f}  ASSD {d[0, 2]:.4f}; largest relative |host - native| = {worst:.3g}",
                  f"  HOST wall time, host path   (copy + erosions + transforms + percentile)  {spread(th)}",
                  f"  HOST wall time, native path (launches + copy of [S, 3] results)         {spread(tn)}",
                  f"  ratio of medians host / native: {np.median(th) / np.median(tn):.0f}x", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
