"""A/B of the volume post-processing paths on one device, in one process: for (a) 1 x 4 x 256^2, (b) 1 x 64 x 256^2 and
(c) 4 x 155 x 240 x 240 (V volumes of D x H x W),
  host leg   the only path a user has without csrc/postproc3d.hip for device-resident squared-error volumes: copy them to the
             host, then per volume scipy.ndimage.median_filter(size=5) on the volume, the region of interest (one volume) eroded
             by binary_erosion(iterations=3) in 3-D and multiplied in, label (6 neighbours) + bincount on the volume cut at the
             threshold, components below 7 voxels dropped; then the filtered volumes and the predictions go back to the device
  native leg metrics.postprocess_volumes (one erosion launch, one median launch) + the small-components launches, plus the copy
             of the [V, 2] component counts
Both legs start from the same device tensors after a device synchronise and end with a synchronising copy; they alternate
inside every repetition.  Reported: median, min, max and quartiles of the wall time per leg, the HIP-event time of each native
step alone, and -- from the same run -- the per-voxel time of the 3-D k = 5 median against the per-pixel time of the plane-wise
k = 5 median (metrics.median_filter) on the same number of elements; the instruction count predicts a ratio of 125 / 25 = 5.
The two results are compared bit for bit before anything is timed.

    python tools/bench_postproc3d.py [--reps 20] [--warmup 2] [--host-reps 3] [--out profiles/postproc3d_ab.txt]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEDIAN, ERODE, MIN_SIZE, THRESHOLD = 5, 3, 7, 0.05
VALU_PEAK = 256 * 4 * 32 * 2.4e9                     # lane-instructions per second: 256 CUs x 4 SIMD-32 at 2.4 GHz
HBM_PEAK = 8.0e12


def make(V, D, H, W, dev):
    """Squared-error-like volumes with speckle and a blob per volume, and an ellipsoidal region of interest (one volume)."""
    g = torch.Generator(device="cpu").manual_seed(4321 + V + D)
    x = torch.rand(V, D, H, W, generator=g) * 0.3
    x = x * x
    x = torch.where(torch.rand(V, D, H, W, generator=g) < 0.01, torch.ones(()), x)
    cy, cx = H // 2, W // 2
    x[..., cy - H // 10:cy + H // 10, cx - W // 8:cx + W // 8] += 0.4
    k, i, j = torch.meshgrid(torch.arange(D, dtype=torch.float64), torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64),
                             indexing="ij")
    roi = ((((k - (D - 1) / 2) / (0.6 * D + 3)) ** 2 + ((i - cy) / (0.45 * H)) ** 2 + ((j - cx) / (0.4 * W)) ** 2) <= 1.0).float()
    return x.float().contiguous().to(dev), roi.to(dev)


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:10.3f} ms   min {s['min']:10.3f}   q25 {s['q25']:10.3f}   q75 {s['q75']:10.3f}   max {s['max']:10.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="repetitions of the native leg and of the event timings")
    ap.add_argument("--host-reps", type=int, default=3, help="of them, how many also run the host leg (scipy takes seconds on the large shapes)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20 or not 3 <= args.host_reps <= args.reps:
        ap.error("--reps must be at least 20 and --host-reps in 3 ... reps")
    if not torch.cuda.is_available():
        sys.exit("bench_postproc3d.py measures on the device: no GPU visible")
    import scipy
    from scipy import ndimage
    from anoddpm_amd import metrics
    dev = torch.device("cuda:0")
    pp = metrics.VolumePostProcess(median=MEDIAN, erode=ERODE, min_size=MIN_SIZE)
    lines = [f"volume post-processing (3-D median {MEDIAN}, {ERODE} 3-D erosions of the region of interest, 6-connected components below "
             f"{MIN_SIZE} voxels dropped at threshold {THRESHOLD}): host path (D2H + scipy + H2D) against the native path, same process, "
             f"legs alternating, {args.reps} native repetitions ({args.host_reps} of them with the host leg) after {args.warmup} warm-up",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}; scipy {scipy.__version__}",
             f"peaks used for the shares below: vector issue {VALU_PEAK / 1e12:.1f} T lane-instructions/s (256 CUs x 4 SIMD-32 x 2.4 GHz), "
             f"HBM {HBM_PEAK / 1e12:.1f} TB/s", ""]
    slower = []
    for label, V, D, H, W in (("(a) 1 x 4 x 256^2", 1, 4, 256, 256), ("(b) 1 x 64 x 256^2", 1, 64, 256, 256),
                              ("(c) 4 x 155 x 240 x 240", 4, 155, 240, 240)):
        vols, roi = make(V, D, H, W, dev)
        voxels = V * D * H * W
        planes = vols.reshape(V * D, 1, H, W)                            # the same elements as planes, for the plane-wise median

        def host_leg():
            x, r = vols.cpu().numpy(), roi.cpu().numpy()                 # the D2H copies a host pipeline needs
            r = ndimage.binary_erosion(r > 0, iterations=ERODE).astype(np.float32)
            f = np.empty_like(x)
            p = np.empty_like(x)
            for v in range(V):
                f[v] = ndimage.median_filter(x[v], size=MEDIAN) * r
                lab, found = ndimage.label(f[v] > np.float32(THRESHOLD))
                keep = np.bincount(lab.ravel(), minlength=found + 1) >= MIN_SIZE
                keep[0] = False
                p[v] = keep[lab]
            fd, pd = torch.from_numpy(f).to(dev), torch.from_numpy(p).to(dev)
            torch.cuda.synchronize()
            return f, p, fd, pd

        def native(sync=True):
            f = metrics.postprocess_volumes(vols, pp, roi=roi)
            p, counts = metrics._small_components3d(f, THRESHOLD, MIN_SIZE, 1)
            return f, p, (counts.cpu() if sync else counts)

        hf, hp, _, _ = host_leg()
        nf, npred, ncounts = native()
        assert hf.tobytes() == nf.cpu().numpy().tobytes() and hp.tobytes() == npred.cpu().numpy().tobytes(), label
        print(f"{label}: both legs give the same bits; timing", flush=True)
        for _ in range(args.warmup):
            native()
            metrics.median_filter(planes, MEDIAN)
        t_host, t_native = [], []
        ev = {k: [] for k in ("erode", "median", "components", "median_plain", "median2d")}
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        for rep in range(args.reps):
            if rep < args.host_reps:
                torch.cuda.synchronize()
                t = time.perf_counter()
                host_leg()
                t_host.append((time.perf_counter() - t) * 1e3)
            torch.cuda.synchronize()
            t = time.perf_counter()
            native()
            t_native.append((time.perf_counter() - t) * 1e3)
            # the steps alone, by HIP events (not part of the wall times above); the last two without a region of interest, so that
            # every element is selected in both
            torch.cuda.synchronize()
            e[0].record()
            r = metrics.erode_mask3d(roi, ERODE)
            e[1].record()
            f = metrics.median_filter3d(vols, MEDIAN, roi=r)
            e[2].record()
            metrics._small_components3d(f, THRESHOLD, MIN_SIZE, 1)
            e[3].record()
            metrics.median_filter3d(vols, MEDIAN)
            e[4].record()
            metrics.median_filter(planes, MEDIAN)
            e[5].record()
            torch.cuda.synchronize()
            for j, k in enumerate(ev):
                ev[k].append(e[j].elapsed_time(e[j + 1]))
        sh, sn = stats(t_host), stats(t_native)
        faster = sn["max"] < sh["min"]
        if not faster:
            slower.append(label)
        se = {k: stats(v) for k, v in ev.items()}
        inside = float(metrics.erode_mask3d(roi, ERODE).mean())
        t3, t2 = se["median_plain"]["median"] * 1e-3, se["median2d"]["median"] * 1e-3
        sel3, sel2 = voxels * 31 * 2 * MEDIAN ** 3, voxels * 31 * 2 * MEDIAN ** 2
        lines += [f"{label}: filtered volumes and predictions equal bit for bit; components found / kept in volume 0: {ncounts.reshape(-1, 2)[0].tolist()}",
                  f"  host   (D2H + scipy median, erosion, label + H2D)   {fmt(sh)}",
                  f"  native (erode + median + components + D2H counts)  {fmt(sn)}",
                  f"  ratio of medians host / native: {sh['median'] / sn['median']:.1f}x; slowest native repetition "
                  f"{'below' if faster else 'NOT below'} the fastest host repetition",
                  f"  erosion launch alone (HIP events, one volume)      {fmt(se['erode'])}",
                  f"  median launch alone ({inside:.0%} inside the region)      {fmt(se['median'])}",
                  f"  small-components launches alone (five)             {fmt(se['components'])}",
                  f"  3-D median, no region: every voxel selected        {fmt(se['median_plain'])}",
                  f"    {t3 / voxels * 1e12:.1f} ps per voxel; selection {sel3 / 1e9:.2f} G lane-instructions = {sel3 / t3 / 1e12:.1f} T/s, "
                  f"{sel3 / t3 / VALU_PEAK:.0%} of vector issue",
                  f"  plane-wise median of the same elements as planes   {fmt(se['median2d'])}",
                  f"    {t2 / voxels * 1e12:.1f} ps per pixel; selection {sel2 / 1e9:.2f} G lane-instructions = {sel2 / t2 / 1e12:.1f} T/s, "
                  f"{sel2 / t2 / VALU_PEAK:.0%} of vector issue",
                  f"  per-voxel time of the 3-D k = 5 median / per-pixel time of the 2-D k = 5 median: {t3 / t2:.2f} "
                  f"(the instruction count predicts {MEDIAN ** 3 / MEDIAN ** 2:.0f})", ""]
    if slower:
        lines.append("the native path is NOT faster than the host path at: " + ", ".join(slower))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
