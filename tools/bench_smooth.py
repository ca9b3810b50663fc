"""A/B of the smoothing and image-score paths on one device, in one process: for (a) 1 x 1 x 256^2, (b) 55 x 1 x 256^2 (the maps
of one detection_B sweep) and (c) 16 x 3 x 512^2, at sigma 4 and the top 1 % of the pixels,
  host leg   what a user has without csrc/smooth.hip for device-resident anomaly maps: copy them to the host, per plane
             scipy.ndimage.gaussian_filter(sigma=4), per image numpy.max and the mean of numpy.partition's top k, then the
             smoothed maps go back to the device (where the ROC / PRO launches want them)
  native leg metrics.gaussian_filter (one launch) + metrics.image_scores (one launch), plus the copy of the [S] scores
Both legs start from the same device tensors after a device synchronise and end with a synchronising copy; they alternate
inside every repetition.  Reported: median, min, max and quartiles of the wall time per leg, and the HIP-event time of each
native launch alone with the work it does, counted from the shapes.  The smoothed maps are compared bit for bit and the scores
against the host's (max exactly, top-k mean within k * 2^-52) before anything is timed.  Without scipy the host leg is reported
as absent and the native leg is timed alone.

    python tools/bench_smooth.py [--reps 20] [--warmup 3] [--out profiles/smooth_ab.txt]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMA, TRUNCATE, TOP, TILE = 4.0, 4.0, 0.01, 32
FP64_PEAK = 78.6e12 / 2                              # fp64 vector instructions (lane-ops) per second: 78.6 TFLOP/s counts an FMA as two
HBM_PEAK = 8.0e12


def make(S, C, side, dev):
    """Squared-error-like maps: `random ** 4 * 3` with a brighter blob per plane."""
    g = torch.Generator(device="cpu").manual_seed(4321 + S)
    x = torch.rand(S, C, side, side, generator=g) ** 4 * 3
    c = side // 2
    x[..., c - side // 10:c + side // 10, c - side // 8:c + side // 8] += 0.4
    return x.float().contiguous().to(dev)


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
        sys.exit("bench_smooth.py measures on the device: no GPU visible")
    try:
        import scipy
        from scipy import ndimage
    except ImportError:
        scipy = ndimage = None
    from anoddpm_amd import metrics
    dev = torch.device("cuda:0")
    radius = int(TRUNCATE * SIGMA + 0.5)
    lines = [f"Gaussian filter (sigma {SIGMA:g}, truncate {TRUNCATE:g}: radius {radius}) and image scores (max, mean, mean of the top {TOP:.0%}): "
             f"host path against the native path, same process, legs alternating, {args.reps} repetitions after {args.warmup} warm-up",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}; scipy {scipy.__version__ if scipy else 'absent'}",
             f"peaks used for the shares below: fp64 vector issue {FP64_PEAK / 1e12:.1f} T lane-operations/s, HBM {HBM_PEAK / 1e12:.1f} TB/s", ""]
    if ndimage is None:
        lines += ["host leg: absent (scipy is not installed here); the native leg is timed alone", ""]
    slower = []
    for label, S, C, side in (("(a) 1 x 1 x 256^2", 1, 1, 256), ("(b) 55 x 1 x 256^2", 55, 1, 256), ("(c) 16 x 3 x 512^2", 16, 3, 512)):
        maps = make(S, C, side, dev)
        n = C * side * side
        k = max(1, int(TOP * n))

        def host_leg():
            x = maps.cpu().numpy()                                       # the D2H copy a host pipeline needs
            f = np.empty_like(x)
            for s in range(S):
                for c in range(C):
                    f[s, c] = ndimage.gaussian_filter(x[s, c], SIGMA, truncate=TRUNCATE)
            flat = f.reshape(S, n)
            mx = flat.max(axis=1)
            topk = np.partition(flat, n - k, axis=1)[:, n - k:].astype(np.float64).mean(axis=1)
            fd = torch.from_numpy(f).to(dev)
            torch.cuda.synchronize()
            return f, mx, topk, fd

        def native(sync=True):
            f = metrics.gaussian_filter(maps, SIGMA, TRUNCATE)
            o = metrics.image_scores(f, top=k, batched=True)
            return f, ((o["max"].cpu(), o["topk"].cpu()) if sync else o)

        nf, (nmax, ntopk) = native()
        if ndimage is not None:
            hf, hmax, htopk, _ = host_leg()
            assert hf.tobytes() == nf.cpu().numpy().tobytes(), label
            assert hmax.tobytes() == nmax.numpy().tobytes() and np.all(np.abs(htopk - ntopk.numpy()) <= k * 2.0 ** -52 * htopk), label
        for _ in range(args.warmup):
            if ndimage is not None:
                host_leg()
            native()
        t_host, t_native = [], []
        ev = {k_: [] for k_ in ("gauss", "scores")}
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for _ in range(args.reps):
            if ndimage is not None:
                torch.cuda.synchronize()
                t = time.perf_counter()
                host_leg()
                t_host.append((time.perf_counter() - t) * 1e3)
            torch.cuda.synchronize()
            t = time.perf_counter()
            native()
            t_native.append((time.perf_counter() - t) * 1e3)
            # the launches alone, by HIP events (not part of the wall times above)
            torch.cuda.synchronize()
            e[0].record()
            f = metrics.gaussian_filter(maps, SIGMA, TRUNCATE)
            e[1].record()
            metrics.image_scores(f, top=k, batched=True)
            e[2].record()
            torch.cuda.synchronize()
            for j, k_ in enumerate(("gauss", "scores")):
                ev[k_].append(e[j].elapsed_time(e[j + 1]))
        sn = stats(t_native)
        se = {k_: stats(v) for k_, v in ev.items()}
        tiles = S * C * (-(-side // TILE)) ** 2
        # per tile: axis 0 over TILE x (TILE + 2r) columns, axis 1 over TILE x TILE; (r + 1) multiplies and r pair sums + r accumulations each
        ops = tiles * (TILE * (TILE + 2 * radius) + TILE * TILE) * (3 * radius + 1)
        t_g = se["gauss"]["median"] * 1e-3
        g_bytes = S * n * 8
        t_s = se["scores"]["median"] * 1e-3
        s_bytes = S * n * 4 * 5                                          # five passes over an image: four select passes (the first with status / sum), the top sum
        lines.append(f"{label}: k = {k}" + ("; smoothed maps equal bit for bit, max equal, top-k mean within k * 2^-52" if ndimage is not None else ""))
        if ndimage is not None:
            sh = stats(t_host)
            faster = sn["max"] < sh["min"]
            if not faster:
                slower.append(label)
            lines += [f"  host   (D2H + scipy gaussian_filter + max / partition + H2D)  {fmt(sh)}"]
        lines += [f"  native (gauss + scores launches + D2H scores)                 {fmt(sn)}"]
        if ndimage is not None:
            lines += [f"  ratio of medians host / native: {sh['median'] / sn['median']:.1f}x; slowest native repetition "
                      f"{'below' if faster else 'NOT below'} the fastest host repetition"]
        lines += [f"  gauss launch alone (HIP events)                               {fmt(se['gauss'])}",
                  f"    {tiles} tiles, {ops / 1e9:.2f} G fp64 lane-operations = {ops / t_g / 1e12:.2f} T/s, {ops / t_g / FP64_PEAK:.0%} of fp64 vector issue; "
                  f"{g_bytes / 1e6:.1f} MB in and out = {g_bytes / t_g / 1e9:.0f} GB/s, {g_bytes / t_g / HBM_PEAK:.1%} of HBM",
                  f"  scores launch alone (one workgroup per image)                 {fmt(se['scores'])}",
                  f"    {s_bytes / 1e6:.1f} MB read in five passes = {s_bytes / t_s / 1e9:.0f} GB/s: {S} workgroup(s) on {S} of 256 CUs, bound by one "
                  f"workgroup's read rate and its LDS histogram atomics", ""]
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
