"""A/B of the post-processing paths on one device, in one process: for (a) 1 x 1 x 256^2, (b) 55 x 1 x 256^2 with one shared region
of interest (the maps of one detection_B sweep) and (c) 16 x 3 x 512^2,
  host leg   what a user of the parent commit has for device-resident squared-error maps: copy them to the host, then per plane
             scipy.ndimage.median_filter(size=5), the region of interest eroded by binary_erosion(iterations=3) and multiplied in,
             label + bincount on the map cut at the threshold, components below 7 pixels dropped; then the filtered maps and
             the binary predictions go back to the device (where the ROC launch wants them)
  native leg metrics.postprocess_maps (one erosion launch, one median launch) + the small-components launches, plus the copy
             of the [S, 2] component counts
Both legs start from the same device tensors after a device synchronise and end with a synchronising copy; they alternate
inside every repetition.  Reported: median, min, max and quartiles of the wall time per leg, and the HIP-event time of each
native step alone with the work it does, counted from the shapes (vector instructions of the median's selection, bytes moved).
The two results are compared bit for bit before anything is timed.

    python tools/bench_postproc.py [--reps 20] [--warmup 3] [--out profiles/postproc_ab.txt]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MEDIAN, ERODE, MIN_SIZE, THRESHOLD = 5, 3, 7, 0.05
VALU_PEAK = 256 * 4 * 32 * 2.4e9                     # lane-instructions per second: 256 CUs x 4 SIMD-32 at 2.4 GHz
HBM_PEAK = 8.0e12


def make(S, C, side, dev):
    """Squared-error-like maps with speckle and a blob per plane, and an elliptic region of interest."""
    g = torch.Generator(device="cpu").manual_seed(1234 + S)
    x = torch.rand(S, C, side, side, generator=g) * 0.3
    x = x * x
    x = torch.where(torch.rand(S, C, side, side, generator=g) < 0.01, torch.ones(()), x)
    c = side // 2
    x[..., c - side // 10:c + side // 10, c - side // 8:c + side // 8] += 0.4
    i, j = torch.meshgrid(torch.arange(side, dtype=torch.float64), torch.arange(side, dtype=torch.float64), indexing="ij")
    roi = ((((i - c) / (0.45 * side)) ** 2 + ((j - c) / (0.4 * side)) ** 2) <= 1.0).float()
    return x.float().contiguous().to(dev), roi.to(dev)


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:10.3f} ms   min {s['min']:10.3f}   q25 {s['q25']:10.3f}   q75 {s['q75']:10.3f}   max {s['max']:10.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_postproc.py measures on the device: no GPU visible")
    import scipy
    from scipy import ndimage
    from anoddpm_amd import metrics
    dev = torch.device("cuda:0")
    pp = metrics.PostProcess(median=MEDIAN, erode=ERODE, min_size=MIN_SIZE)
    lines = [f"post-processing (median {MEDIAN}, {ERODE} erosions of the region of interest, components below {MIN_SIZE} pixels dropped at "
             f"threshold {THRESHOLD}): host path of the parent commit against the native path, same process, legs alternating, "
             f"{args.reps} repetitions after {args.warmup} warm-up",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}; scipy {scipy.__version__}",
             f"peaks used for the shares below: vector issue {VALU_PEAK / 1e12:.1f} T lane-instructions/s (256 CUs x 4 SIMD-32 x 2.4 GHz), "
             f"HBM {HBM_PEAK / 1e12:.1f} TB/s", ""]
    slower = []
    for label, S, C, side in (("(a) 1 x 1 x 256^2", 1, 1, 256), ("(b) 55 x 1 x 256^2, one shared region of interest", 55, 1, 256),
                              ("(c) 16 x 3 x 512^2", 16, 3, 512)):
        maps, roi = make(S, C, side, dev)
        planes = S * C
        pixels = planes * side * side

        def host_leg():
            x, r = maps.cpu().numpy(), roi.cpu().numpy()                 # the D2H copies a host pipeline needs
            r = ndimage.binary_erosion(r > 0, iterations=ERODE).astype(np.float32)
            f = np.empty_like(x)
            p = np.empty_like(x)
            for s in range(S):
                for c in range(C):
                    f[s, c] = ndimage.median_filter(x[s, c], size=MEDIAN) * r
                    lab, found = ndimage.label(f[s, c] > np.float32(THRESHOLD))
                    keep = np.bincount(lab.ravel(), minlength=found + 1) >= MIN_SIZE
                    keep[0] = False
                    p[s, c] = keep[lab]
            fd, pd = torch.from_numpy(f).to(dev), torch.from_numpy(p).to(dev)
            torch.cuda.synchronize()
            return f, p, fd, pd

        def native(sync=True):
            f = metrics.postprocess_maps(maps, pp, roi=roi)
            p, counts = metrics._small_components(f, THRESHOLD, MIN_SIZE, 1)
            return f, p, (counts.cpu() if sync else counts)

        hf, hp, _, _ = host_leg()
        nf, npred, ncounts = native()
        assert hf.tobytes() == nf.cpu().numpy().tobytes() and hp.tobytes() == npred.cpu().numpy().tobytes(), label
        for _ in range(args.warmup):
            host_leg()
            native()
        t_host, t_native = [], []
        ev = {k: [] for k in ("erode", "median", "components")}
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            host_leg()
            t_host.append((time.perf_counter() - t) * 1e3)
            torch.cuda.synchronize()
            t = time.perf_counter()
            native()
            t_native.append((time.perf_counter() - t) * 1e3)
            # the steps alone, by HIP events (not part of the wall times above)
            torch.cuda.synchronize()
            e[0].record()
            r = metrics.erode_mask(roi, ERODE)
            e[1].record()
            f = metrics.median_filter(maps, MEDIAN, roi=r)
            e[2].record()
            metrics._small_components(f, THRESHOLD, MIN_SIZE, 1)
            e[3].record()
            torch.cuda.synchronize()
            for j, k in enumerate(("erode", "median", "components")):
                ev[k].append(e[j].elapsed_time(e[j + 1]))
        sh, sn = stats(t_host), stats(t_native)
        faster = sn["max"] < sh["min"]
        if not faster:
            slower.append(label)
        se = {k: stats(v) for k, v in ev.items()}
        inside = float(roi.mean())
        sel = pixels * inside * 31 * 2 * MEDIAN * MEDIAN             # 31 rounds of k*k compare + add, pixels inside the region only
        t_med = se["median"]["median"] * 1e-3
        med_bytes = pixels * 8 + roi.numel() * 4
        cc_bytes = pixels * (4 + 8 + 8 + 4 + 8 + 4 + 12)             # clear r4 w8, link r>=8, flatten r4 w4, sizes r4 + atomics, filter r8 w4
        t_cc = se["components"]["median"] * 1e-3
        lines += [f"{label}: filtered maps and predictions equal bit for bit; components found / kept in plane 0: {ncounts.reshape(-1, 2)[0].tolist()}",
                  f"  host   (D2H + scipy median, erosion, label + H2D)   {fmt(sh)}",
                  f"  native (erode + median + components + D2H counts)  {fmt(sn)}",
                  f"  ratio of medians host / native: {sh['median'] / sn['median']:.1f}x; slowest native repetition "
                  f"{'below' if faster else 'NOT below'} the fastest host repetition",
                  f"  erosion launch alone (HIP events)                  {fmt(se['erode'])}",
                  f"  median launch alone                                {fmt(se['median'])}",
                  f"    selection: {sel / 1e9:.2f} G lane-instructions ({inside:.0%} of the pixels are inside the region) = "
                  f"{sel / t_med / 1e12:.1f} T/s, {sel / t_med / VALU_PEAK:.0%} of vector issue; "
                  f"{med_bytes / 1e6:.1f} MB moved = {med_bytes / t_med / 1e9:.0f} GB/s, {med_bytes / t_med / HBM_PEAK:.1%} of HBM",
                  f"  small-components launches alone (five)             {fmt(se['components'])}",
                  f"    at least {cc_bytes / 1e6:.1f} MB moved = {cc_bytes / t_cc / 1e9:.0f} GB/s, {cc_bytes / t_cc / HBM_PEAK:.1%} of HBM: bound by the "
                  f"dependent label reads of the link and flatten launches and by launch latency, not by bandwidth", ""]
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
