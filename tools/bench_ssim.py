"""A/B of the SSIM paths on one device, in one process: for (a) 1 x 1 x 256^2, (b) 55 x 1 x 256^2 (one detection_B sweep: one image
against 55 reconstructions) and (c) 16 x 3 x 512^2,
  host leg   what a user of the parent commit has for device-resident images: copy them to the host, then per pair the filter
             pipeline there (skimage.metrics.structural_similarity with data_range 2 when skimage can be imported, else the
             scipy.ndimage restatement of tests/ssim_cases.py, `ssim_expected`; the report says which)
  native leg metrics.ssim plus the copy of the [S] result
Both legs start from the same device tensors after a device synchronise and end with their synchronising copy; they alternate
inside every repetition.  Reported: median, min, max and quartiles of the wall time per leg, and the HIP-event time of the native
launches alone.  The two results are compared (1e-10, or 1e-6 against skimage's fp32 pipeline) before anything is timed.

    python tools/bench_ssim.py [--reps 20] [--warmup 3] [--out profiles/ssim_ab.txt]"""
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


def host_leg_factory():
    try:
        import skimage
        from skimage.metrics import structural_similarity

        def host_ssim(real, recon):
            return structural_similarity(real, recon, channel_axis=0, data_range=2.0)
        return host_ssim, f"skimage {skimage.__version__} structural_similarity(channel_axis=0, data_range=2.0) on the fp32 images", 1e-6
    except ImportError:
        import scipy
        import ssim_cases as sc

        def host_ssim(real, recon):
            return sc.ssim_expected(real, recon, 7)[0]
        return host_ssim, (f"scipy {scipy.__version__} ndimage.uniform_filter restatement of structural_similarity in fp64 "
                           "(tests/ssim_cases.py); skimage is not importable here"), 1e-10


def make(S, C, side, shared, dev):
    g = torch.Generator(device="cpu").manual_seed(4321 + S)
    real = torch.rand(1 if shared else S, C, side, side, generator=g) * 2 - 1
    recon = (real + (torch.rand(S, C, side, side, generator=g) - 0.5) * 0.4).clamp(-1, 1)
    return real.to(dev), recon.to(dev)


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
        sys.exit("bench_ssim.py measures on the device: no GPU visible")
    from anoddpm_amd import metrics
    dev = torch.device("cuda:0")
    host_ssim, host_kind, tol = host_leg_factory()
    lines = [f"SSIM: host path of the parent commit against metrics.ssim, same process, legs alternating, {args.reps} repetitions "
             f"after {args.warmup} warm-up",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}",
             f"host leg: {host_kind}", ""]
    slower = []
    for label, S, C, side, shared in (("(a) 1 x 1 x 256^2", 1, 1, 256, False), ("(b) 55 x 1 x 256^2, one shared real", 55, 1, 256, True),
                                      ("(c) 16 x 3 x 512^2", 16, 3, 512, False)):
        real, recon = make(S, C, side, shared, dev)

        def host_leg():
            x, y = real.cpu().numpy(), recon.cpu().numpy()              # the D2H copies a host SSIM needs
            return np.array([host_ssim(x[0 if shared else j], y[j]) for j in range(S)])

        def native_leg():
            return metrics.ssim(real[0] if shared else real, recon).cpu().numpy()

        h, d = host_leg(), native_leg()
        worst = float(np.max(np.abs(h - d)))
        assert worst <= tol, (label, worst)
        for _ in range(args.warmup):
            host_leg()
            native_leg()
        t_host, t_native, t_event = [], [], []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            host_leg()
            t_host.append((time.perf_counter() - t) * 1e3)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record()
            r = metrics.ssim(real[0] if shared else real, recon)
            e1.record()
            r.cpu()
            t_native.append((time.perf_counter() - t) * 1e3)
            t_event.append(e0.elapsed_time(e1))
        sh, sn, se = stats(t_host), stats(t_native), stats(t_event)
        faster = sn["max"] < sh["min"]
        if not faster:
            slower.append(label)
        lines += [f"{label}: largest |ssim_host - ssim_native| = {worst:.3g}",
                  f"  host   (copy + filters + mean)          {fmt(sh)}",
                  f"  native (ssim + copy of [S] fp64)        {fmt(sn)}",
                  f"  native launches alone (HIP events)      {fmt(se)}",
                  f"  ratio of medians host / native: {sh['median'] / sn['median']:.1f}x; slowest native repetition "
                  f"{'below' if faster else 'NOT below'} the fastest host repetition", ""]
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
