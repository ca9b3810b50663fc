"""Cost of the per-region overlap score (anoddpm_component_areas of csrc/postproc.hip + anoddpm_pro_auc of csrc/pro.hip) on one
device, in one process: for (a) 1 x 256^2, (b) the 55 maps of a detection sweep with ONE shared mask and (c) one pooled segment of
2^22 elements (64 planes of 256^2),
  1. DEVICE time of the component-areas run + the PRO launch (what metrics.aupro issues), and of its two halves, from HIP events
     around a window of back-to-back launches that lasts at least --window seconds, divided by the launches in it; beside them
     the ROC-only launch of the same build on the same maps, for scale.  The legs alternate, the round is repeated --pairs times
     and the spread over the repetitions is reported
  2. native against host: HOST wall time of metrics.aupro with its [S] results copied to the host against what a user had to
     do without it: copy masks and maps to the host, then per map scipy.ndimage.label + numpy argsort / cumsum and the trapezoid
     up to the limit (the cumulative-sum form of the published evaluation code).  The two results are compared before anything
     is timed.

    python tools/bench_pro.py [--pairs 5] [--window 0.5] [--reps 10] [--out profiles/pro_ab.txt]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LIMIT = 0.3


def host_aupro(mask, score, limit=LIMIT):
    """One segment on the host: mask / score [m, H, W]."""
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(2, 2)
    area = np.zeros(mask.shape, np.int64)
    K = 0
    for p, plane in enumerate(mask):
        lab, k = ndimage.label(plane > 0, structure)
        size = np.bincount(lab.ravel())
        size[0] = 0
        area[p] = size[lab]
        K += k
    a, s = area.reshape(-1), score.reshape(-1)
    N = int((a == 0).sum())
    if K == 0 or N == 0:
        return float("nan")
    order = np.argsort(-s, kind="stable")
    a, s = a[order], s[order]
    fprs = np.cumsum(a == 0) / N
    pros = np.cumsum(np.where(a != 0, 1.0 / np.maximum(a, 1), 0.0)) / K
    keep = np.r_[s[1:] != s[:-1], True]
    fprs, pros = np.r_[0.0, fprs[keep]], np.r_[0.0, np.minimum(pros[keep], 1.0)]
    j = int(np.searchsorted(fprs, limit, side="right"))                  # points with fpr <= limit
    x, y = fprs[:j], pros[:j]
    val = float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) * 0.5))
    if j < fprs.size and x[-1] < limit:
        yl = y[-1] + (pros[j] - y[-1]) * (limit - x[-1]) / (fprs[j] - x[-1])
        val += (limit - x[-1]) * (yl + y[-1]) * 0.5
    return val / limit


def make(S, m, side, shared, dev):
    """Masks with a handful of rectangular lesions of very different sizes per plane; maps that respond to them."""
    rng = np.random.default_rng(4321 + S + m)
    planes = m if shared else S * m
    mask = np.zeros((planes, side, side), np.float32)
    for p in range(planes):
        for _ in range(int(rng.integers(1, 7))):
            h, w = rng.integers(1, 41, 2)
            y, x = rng.integers(0, side - h + 1), rng.integers(0, side - w + 1)
            mask[p, y:y + h, x:x + w] = 1
    mask = mask.reshape((m, side, side) if shared else (S, m, side, side))
    g = torch.Generator(device="cpu").manual_seed(1234 + S + m)
    base = torch.rand(S, m, side, side, generator=g)
    score = base * base * 0.9 + torch.from_numpy(mask).expand(S, m, side, side) * torch.rand(S, m, side, side, generator=g) * 0.35
    return torch.from_numpy(mask).to(dev), score.contiguous().to(dev)


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
        sys.exit("bench_pro.py measures on the device: no GPU visible")
    import scipy
    from anoddpm_amd import _lib, metrics
    dev = torch.device("cuda:0")
    lines = [f"per-region overlap score, csrc/postproc.hip + csrc/pro.hip (ABI {_lib.ABI_VERSION}), limit {LIMIT}, 8 neighbours: {args.pairs} "
             f"alternating repetitions, windows of at least {args.window} s of back-to-back launches, every shape warmed first",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}; scipy {scipy.__version__}",
             "host leg: D2H copy + scipy.ndimage.label per plane + numpy argsort / cumsum per map + trapezoid up to the limit", ""]
    shapes = (("(a) 1 x 256^2", 1, 1, True), ("(b) 55 x 256^2, one shared mask", 55, 1, True), ("(c) 1 x 2^22 (64 pooled planes of 256^2)", 1, 64, True))
    for label, S, m, shared in shapes:
        mask, score = make(S, m, 256, shared, dev)
        n = m * 256 * 256
        flat_mask = mask.reshape(-1)

        def areas_only():
            return metrics.component_areas(mask, connectivity=2)

        def both():
            return metrics._pro_launch(mask, score, LIMIT, 2, True, False)

        def roc_only():
            return metrics._roc_launch(flat_mask, score.reshape(S, -1), True, False)

        legs = [("component areas + PRO launch (metrics.aupro)", both), ("component areas alone (five small launches) ", areas_only),
                ("ROC-only launch of the same maps, for scale  ", roc_only)]
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
        regions = int(metrics.component_areas(mask, connectivity=2)[1].sum())
        lines.append(f"{label}: S = {S}, n = {n}, {regions} regions in the mask")
        for name, _ in legs:
            lines.append(f"  DEVICE time, {name}  {spread(t[name])}   [{launches[name]} per window]")
        med = {name: float(np.median(v)) for name, v in t.items()}
        lines.append(f"  PRO launch alone (difference of the medians): {med[legs[0][0]] - med[legs[1][0]]:.4f} ms = "
                     f"{(med[legs[0][0]] - med[legs[1][0]]) / med[legs[2][0]]:.2f} x the ROC-only launch")

        def host_leg():
            mk, sc = mask.cpu().numpy(), score.cpu().numpy()
            return np.array([host_aupro(mk, sc[j]) for j in range(S)])

        def native_leg():
            return metrics.aupro(mask, score, limit=LIMIT, batched=True).cpu().numpy()

        h, d = host_leg(), native_leg()
        worst = float(np.max(np.abs(h - d)))
        assert worst <= n * 2.0 ** -49, (label, worst)                   # each within n * 2^-50 of the exact value
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
        lines += [f"  AUPRO {d[0]:.6f} (segment 0); largest |host - native| = {worst:.3g}",
                  f"  HOST wall time, host path   (copy + label + argsort + cumsum)  {spread(th)}",
                  f"  HOST wall time, native path (launches + copy of [S] results)   {spread(tn)}",
                  f"  ratio of medians host / native: {np.median(th) / np.median(tn):.0f}x", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
