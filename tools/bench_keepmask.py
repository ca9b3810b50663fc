"""Measurements for the keep mask of a two-pass detection on one device, in one process, device time by HIP events after
warm-up:

  leg A  the fused launch (anoddpm_keep_mask through metrics.keep_mask: two asynchronous clears and one kernel)
  leg B  the composition the library offered before it, all on the device (tests/keepmask_cases.composition_torch): ATen
         `score > thr`; the complement padded by r with ones through `erode_mask(iterations=r)`, cropped and complemented again --
         the only way the existing erosion yields a correct dilation; ATen `where` for the stitch; the cast to bytes; `count_nonzero`

at 1 x 1 x 256^2, 55 x 1 x 256^2 (the settings of one detection_B sweep, one threshold each) and 16 x 3 x 512^2, r in {0, 2, 8}.  Each
leg is captured once as a HIP graph of `--inner` consecutive calls (so the device, not the Python launch path, sets the pace); a
repetition times one replay; the legs alternate inside every repetition.  Both legs are checked to give the same keep bytes,
stitched words and counts before they are timed.  One more line gives the host wall time of the path a user had before: the score
to the host, `scipy.ndimage.binary_dilation`, the mask back to the device.

What the mask does to detection quality is NOT measured here or anywhere: there is no trained checkpoint to measure it with.

    python tools/bench_keepmask.py [--reps 20] [--inner 50] [--warmup 3] [--out profiles/keepmask_ab.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
SHAPES = ((1, 1, 256), (55, 1, 256), (16, 3, 512))
RADII = (0, 2, 8)


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:8.2f} us   min {s['min']:8.2f}   q25 {s['q25']:8.2f}   q75 {s['q75']:8.2f}   max {s['max']:8.2f}"


def capture(leg, inner):
    leg()                                                                # first launch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            leg()
    return g


def time_graphs(graphs, args):
    times = {k: [] for k in graphs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(args.warmup + args.reps):
        for name, g in graphs.items():
            torch.cuda.synchronize()
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    return times


def make_inputs(S, C, N, dev):
    """Squared-error-like score planes (about 3 % of the pixels above their plane's threshold, in blobs), one threshold per plane."""
    g = torch.Generator().manual_seed(9900 + S)
    coarse = torch.rand((S, 1, N // 8, N // 8), generator=g)
    score = (torch.nn.functional.interpolate(coarse, size=(N, N), mode="bilinear") [:, 0] - 0.5 * torch.rand((S, N, N), generator=g)).square()
    thr = torch.quantile(score.reshape(S, -1), 0.97, dim=1)
    real = torch.rand((S, C, N, N), generator=g) * 2 - 1
    recon = torch.rand((S, C, N, N), generator=g) * 2 - 1
    return score.to(dev), thr.float().to(dev), real.to(dev), recon.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_keepmask.py measures on the device: no GPU visible")
    from anoddpm_amd import metrics
    from keepmask_cases import composition_torch
    dev = torch.device("cuda:0")
    lines = [f"keep mask of a two-pass detection: device time by HIP events, legs alternating, {args.reps} repetitions after {args.warmup} "
             f"warm-up; a leg is one replay of a captured graph of {args.inner} calls, times per call",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HBM peak used below {HBM_PEAK / 1e12:.1f} TB/s",
             "A: the fused launch (two clears + one kernel).  B: ATen compare, pad, erode_mask on the complement, crop, where, cast, "
             "count_nonzero.", ""]
    single = {}
    for S, C, N in SHAPES:
        score, thr, real, recon = make_inputs(S, C, N, dev)
        moved = (4 + 1 + 12 * C) * S * N * N                           # score, keep byte, real + recon + stitched per channel
        for r in RADII:
            def fused():
                return metrics.keep_mask(score, thr, r, real=real, recon=recon)

            def composed():
                return composition_torch(score, thr, r, real, recon)

            a, b = fused(), composed()
            same = torch.equal(a["keep"][:, 0], b[0]) and torch.equal(a["stitched"].view(torch.int32), b[1].view(torch.int32)) \
                and torch.equal(a["regen"], b[2])
            regen = float(a["regen"].sum()) / (S * N * N)
            if not same:
                lines.append(f"  {S} x {C} x {N}^2, r = {r}: results DIFFER -- not timed")
                continue
            graphs = {"B composed": capture(composed, args.inner), "A fused": capture(fused, args.inner)}
            st = {k: stats(v) for k, v in time_graphs(graphs, args).items()}
            lines.append(f"  {S} x {C} x {N}^2, r = {r}: results equal bit for bit; {regen:.1%} of the pixels regenerated")
            for k in ("B composed", "A fused"):
                extra = ""
                if k == "A fused":
                    bw = moved / (st[k]["median"] * 1e-6)
                    extra = f"   {moved / S / N / N:.0f} B/pixel = {bw / 1e9:6.0f} GB/s, {bw / HBM_PEAK:5.1%} of HBM"
                lines.append(f"    {k:10s} {fmt(st[k])}{extra}")
            ratio = st["A fused"]["median"] / st["B composed"]["median"]
            lines.append(f"    A / B, ratio of medians {ratio:.3f}; spread of leg B's own repetitions (max - min) "
                         f"{st['B composed']['max'] - st['B composed']['min']:.2f} us")
            if (S, C, N) == SHAPES[0]:
                single[r] = ratio
            del graphs
    lines.append("")
    if single:
        slower = [r for r, q in single.items() if q >= 1.0]
        lines.append("single 256^2 plane: the fused launch is " + ("NOT faster than leg B at r = " + ", ".join(map(str, slower)) if slower
                                                                  else "faster than leg B at every radius measured")
                     + "; the feature's case is staying on the device between two graph sweeps, not these microseconds")
    # the path a user had before: host wall time, one 256^2 plane, r = 2
    try:
        from scipy import ndimage as ndi
    except ImportError:
        lines.append("host path (D2H, scipy.ndimage.binary_dilation, H2D): not measured (no scipy)")
    else:
        score, thr, real, recon = make_inputs(1, 1, 256, dev)
        wall = []
        for rep in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seed = score[0].cpu().numpy() > float(thr.cpu()[0])
            keep = torch.from_numpy((~ndi.binary_dilation(seed, iterations=2)).astype(np.uint8)).to(dev)
            torch.cuda.synchronize()
            if rep >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e6)
        ok = torch.equal(keep, metrics.keep_mask(score, thr, 2)["keep"][0, 0])
        lines.append(f"host path, 1 x 1 x 256^2, r = 2 (score and threshold to the host, scipy.ndimage.binary_dilation, mask back; host wall "
                     f"time, two synchronisations; mask {'equal' if ok else 'DIFFERS'}):")
        lines.append(f"    {fmt(stats(wall))}")
    lines.append("detection quality (AUC, Dice) of the two-pass routine: not measured (no trained checkpoint)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
