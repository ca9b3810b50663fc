"""A/B of Gaussian smoothing of whole volumes on one device, in one process: for (a) 1 x 4 x 256^2, (b) 1 x 64 x 256^2 and
(c) 4 x 155 x 240 x 240, at sigma 4 and at sigma (1, 4, 4) in (z, y, x) order, truncate 4,
  leg A   metrics.gaussian_filter3d on the device-resident volumes: its device time (HIP events around the call) and its wall
          time (call + device synchronise)
  leg B   what a user has without csrc/gauss3d.hip: copy the volumes to the host, scipy.ndimage.gaussian_filter per volume, copy
          the result back to the device (where the median, the cut and the distances want it)
Both legs start from the same device tensor after a device synchronise; they alternate inside every repetition.  Reported:
median, min, max and quartiles per leg, and the HIP-event time of each of the two launches alone -- the z launch as the call with
sigma (sz, 0, 0), the plane launch as the call with sigma (0, sy, sx): the same kernel on the same grid, reading the input instead
of the workspace -- with the fp64 work it does, counted from the shapes.  The results are compared bit for bit before anything is
timed.  Nothing here has a threshold.  Without scipy leg B is reported as absent and leg A is timed alone.

    python tools/bench_gauss3d.py [--reps 20] [--warmup 2] [--out profiles/gauss3d_ab.txt]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRUNCATE, TILE = 4.0, 32
FP64_PEAK = 78.6e12 / 2                              # fp64 vector instructions (lane-ops) per second: 78.6 TFLOP/s counts an FMA as two
HBM_PEAK = 8.0e12
SHAPES = (("(a) 1 x 4 x 256^2", (1, 4, 256, 256)), ("(b) 1 x 64 x 256^2", (1, 64, 256, 256)), ("(c) 4 x 155 x 240 x 240", (4, 155, 240, 240)))
SIGMAS = ((4.0, 4.0, 4.0), (1.0, 4.0, 4.0))


def make(shape, dev):
    """Squared-error-like volumes: `random ** 4 * 3` with a brighter block in every volume."""
    g = torch.Generator(device="cpu").manual_seed(4321 + shape[1])
    x = torch.rand(*shape, generator=g) ** 4 * 3
    d, h, w = shape[1:]
    x[:, d // 3:d // 3 + max(1, d // 4), h // 2 - h // 10:h // 2 + h // 10, w // 2 - w // 8:w // 2 + w // 8] += 0.4
    return x.float().contiguous().to(dev)


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:10.3f} ms   min {s['min']:10.3f}   q25 {s['q25']:10.3f}   q75 {s['q75']:10.3f}   max {s['max']:10.3f}"


def work(shape, radii):
    """fp64 lane-operations of the z launch and of the plane launch: r + 1 multiplies, r pair sums and r accumulations per output of
    a pass; the y pass of the plane launch also runs over the 2 rx halo columns of every 32-wide tile."""
    S, D, H, W = shape
    rz, ry, rx = radii
    n = S * D * H * W
    z = n * (3 * rz + 1) if rz else 0
    y = S * D * H * (-(-W // TILE)) * (TILE + 2 * rx) * (3 * ry + 1) if ry else 0
    x = n * (3 * rx + 1) if rx else 0
    return z, y + x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_gauss3d.py measures on the device: no GPU visible")
    try:
        import scipy
        from scipy import ndimage
    except ImportError:
        scipy = ndimage = None
    from anoddpm_amd import metrics
    dev = torch.device("cuda:0")
    lines = [f"Gaussian filter of whole volumes (truncate {TRUNCATE:g}): A the device call against B the host path, same process, legs alternating, "
             f"{args.reps} repetitions after {args.warmup} warm-up",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}; scipy {scipy.__version__ if scipy else 'absent'}",
             f"peaks used for the shares below: fp64 vector issue {FP64_PEAK / 1e12:.1f} T lane-operations/s, HBM {HBM_PEAK / 1e12:.1f} TB/s", ""]
    if ndimage is None:
        lines += ["leg B: absent (scipy is not importable here); leg A is timed alone", ""]
    printed = 0
    for label, shape in SHAPES:
        vols = make(shape, dev)
        n = vols.numel()
        for sigma in SIGMAS:
            radii = tuple(int(TRUNCATE * s + 0.5) for s in sigma)
            z_sigma, p_sigma = (sigma[0], 0.0, 0.0), (0.0, sigma[1], sigma[2])

            def host_leg():
                x = vols.cpu().numpy()                                   # the D2H copy a host pipeline needs
                f = np.stack([ndimage.gaussian_filter(v, sigma, truncate=TRUNCATE) for v in x])
                fd = torch.from_numpy(f).to(dev)
                torch.cuda.synchronize()
                return f, fd

            got = metrics.gaussian_filter3d(vols, sigma, TRUNCATE)
            if ndimage is not None:
                assert host_leg()[0].tobytes() == got.cpu().numpy().tobytes(), (label, sigma)
            for _ in range(args.warmup):
                if ndimage is not None:
                    host_leg()
                metrics.gaussian_filter3d(vols, sigma, TRUNCATE)
                metrics.gaussian_filter3d(vols, z_sigma, TRUNCATE)
                metrics.gaussian_filter3d(vols, p_sigma, TRUNCATE)
            t_host, t_wall = [], []
            ev = {k: [] for k in ("call", "z", "plane")}
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            for _ in range(args.reps):
                if ndimage is not None:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    host_leg()
                    t_host.append((time.perf_counter() - t) * 1e3)
                torch.cuda.synchronize()
                t = time.perf_counter()
                metrics.gaussian_filter3d(vols, sigma, TRUNCATE)
                torch.cuda.synchronize()
                t_wall.append((time.perf_counter() - t) * 1e3)
                for key, sg in (("call", sigma), ("z", z_sigma), ("plane", p_sigma)):      # by HIP events (not part of the wall times above)
                    torch.cuda.synchronize()
                    e[0].record()
                    metrics.gaussian_filter3d(vols, sg, TRUNCATE)
                    e[1].record()
                    torch.cuda.synchronize()
                    ev[key].append(e[0].elapsed_time(e[1]))
            sw = stats(t_wall)
            se = {k: stats(v) for k, v in ev.items()}
            ops_z, ops_p = work(shape, radii)
            lines.append(f"{label}, sigma {sigma}: radii {radii}" + ("; results equal bit for bit" if ndimage is not None else ""))
            if ndimage is not None:
                sh = stats(t_host)
                lines.append(f"  B host (D2H + scipy gaussian_filter + H2D), wall   {fmt(sh)}")
            lines += [f"  A device call, wall (call + synchronise)         {fmt(sw)}",
                      f"  A device call, device time (HIP events)          {fmt(se['call'])}"]
            if ndimage is not None:
                lines.append(f"  ratio of medians B / A wall: {sh['median'] / sw['median']:.1f}x")
            for key, name, ops in (("z", "z launch alone      ", ops_z), ("plane", "plane launch alone  ", ops_p)):
                t_l = se[key]["median"] * 1e-3
                lines += [f"  {name} (HIP events)                  {fmt(se[key])}",
                          f"    {ops / 1e9:.2f} G fp64 lane-operations = {ops / t_l / 1e12:.2f} T/s, {ops / t_l / FP64_PEAK:.0%} of fp64 vector issue; "
                          f"{n * 8 / 1e6:.1f} MB in and out = {n * 8 / t_l / 1e9:.0f} GB/s, {n * 8 / t_l / HBM_PEAK:.1%} of HBM"]
            lines.append("")
            print("\n".join(lines[printed:]), flush=True)               # as it goes: the largest shape takes a while on the host
            printed = len(lines)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
