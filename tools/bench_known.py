"""Measurements for known-region conditioning on one device, in one process, device time by HIP events after warm-up:

  (1) the fused conditioned launch (anoddpm_p_sample_update_known) against the composition it replaces, built from the entry
      points the library had before it: the update into a scratch plane, a fill of the known-region noise (in-kernel-noise form
      only: anoddpm_philox_fill, domain 3), anoddpm_q_sample of the input at the landing timestep, and an ATen `where` into x.
      Cases 16 x 1 x 256^2 and 1 x 1 x 256^2, ancestral and strided (stride 5, eta 0.5), tensor noise (both noises read from
      planes) and in-kernel noise (both generated).  Each leg is captured once as a HIP graph of `--inner` consecutive steps (so
      the device, not the Python launch path, sets the pace); a repetition times one replay; the legs alternate inside every
      repetition.  Both legs are checked to leave the same bits in x before they are timed.
  (2) one conditioned against one unconditioned chain step under graph replay, on the smallest UNet the sampler tests build
      (32^2, base 32, batch 2, deterministic weights), seeded, for noise="fixed" and "fresh": `--inner` replayed steps per
      repetition, legs alternating.

What conditioning does to detection quality is NOT measured here or anywhere: there is no trained checkpoint to measure it with.

    python tools/bench_known.py [--reps 20] [--inner 100] [--warmup 3] [--out profiles/known_ab.txt]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
T = 1000
# bytes per pixel: x_t, eps, x0 read and x_prev written (16), one keep byte, and in the tensor form the two noise planes
MOVED_FUSED = {"tensor noise": 16 + 1 + 8, "in-kernel noise": 16 + 1}
# the composition: update (x_t, eps[, noise] -> u), [fill -> kz], q_sample (x0, kz -> kn), where (keep, kn, u -> x)
MOVED_COMPOSED = {"tensor noise": 16 + 12 + 13, "in-kernel noise": 12 + 4 + 12 + 13}
LAUNCHES = {"tensor noise": 3, "in-kernel noise": 4}


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:8.2f} us   min {s['min']:8.2f}   q25 {s['q25']:8.2f}   q75 {s['q75']:8.2f}   max {s['max']:8.2f}"


def time_graphs(graphs, reset, args):
    """graphs: name -> captured graph of args.inner steps.  -> name -> list of device microseconds per step."""
    times = {k: [] for k in graphs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(args.warmup + args.reps):
        for name, g in graphs.items():
            reset()
            torch.cuda.synchronize()
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    return times


def capture(leg, inner):
    leg()                                                                # first launch outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            leg()
    return g


def launches(d, GD, dev, args, lines):
    from anoddpm_amd import philox
    from anoddpm_amd._lib import check, current_stream, lib, ptr
    tb = d._tables(dev)
    d.seed_gauss(1234)
    seed = d._gauss_seed_dev(dev)
    sampler = GD.StridedSampler(5, 0.5)
    lines.append("(1) fused conditioned launch against the composition of the earlier entry points, in place on x, t spread over "
                 f"60 ... {T - 1}, mask: half of the pixels kept")
    for B in (16, 1):
        g = torch.Generator().manual_seed(116 + B)
        shape = (B, 1, 256, 256)
        x_start = torch.randn(shape, generator=g).to(dev)
        x0 = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
        eps, noise, kz = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
        keep = (torch.rand(shape, generator=g) > 0.5).to(dev)
        keep8 = keep.to(torch.uint8)
        t = torch.linspace(T - 1, 60, B).long().to(dev)
        streams = philox.stream_ids(0, B).to(dev)
        pixels, n = x0.numel(), x0.numel() // B
        x, u, kn, kfill = x_start.clone(), torch.empty(shape, device=dev), torch.empty(shape, device=dev), torch.empty(shape, device=dev)

        def reset():
            x.copy_(x_start)

        for strided in (False, True):
            words = d._sampler_words(dev, sampler) if strided else None
            s = (t - (sampler.stride if strided else 1)).clamp(min=0)             # every t here lands at s >= 0
            for form in ("tensor noise", "in-kernel noise"):
                nz, st, kplane = (noise, None, kz) if form == "tensor noise" else (None, streams, None)

                def fused():
                    d._known_update(x, t, eps, nz, (x0, keep8, kplane), words, want_pred=False, out=x, gauss_streams=st)

                def composed():
                    if strided:
                        d._strided_update(x, t, eps, nz, None, want_pred=False, out=u, gauss_streams=st)
                    else:
                        d._reverse_update(x, t, eps, nz, want_pred=False, out=u, gauss_streams=st)
                    plane = kz
                    if form == "in-kernel noise":
                        check(lib().anoddpm_philox_fill(ptr(kfill), 1, B, n, ptr(seed), ptr(streams), 0, 3, ptr(s), 0, T,
                                                        current_stream()), "philox_fill")
                        plane = kfill
                    check(lib().anoddpm_q_sample(ptr(kn), ptr(x0), ptr(plane), ptr(s), ptr(tb.sqrt_alphas_cumprod),
                                                 ptr(tb.sqrt_one_minus_alphas_cumprod), B, n, T, current_stream()), "q_sample")
                    torch.where(keep, kn, u, out=x)

                reset()
                fused()
                got = x.clone()
                reset()
                composed()
                same = torch.equal(got, x)
                graphs = {"composed": capture(composed, args.inner), "fused": capture(fused, args.inner)}
                st_ = {k: stats(v) for k, v in time_graphs(graphs, reset, args).items()}
                lines.append(f"  {B} x 1 x 256^2, {'strided (5, 0.5)' if strided else 'ancestral'}, {form}: results "
                             f"{'equal bit for bit' if same else 'DIFFER'}")
                for k, moved, nl in (("composed", MOVED_COMPOSED[form], LAUNCHES[form]), ("fused", MOVED_FUSED[form], 1)):
                    bw = moved * pixels / (st_[k]["median"] * 1e-6)
                    lines.append(f"    {k:9s} {fmt(st_[k])}   {nl} launch{'es' if nl > 1 else ''}, {moved} B/pixel = {bw / 1e9:6.0f} GB/s, "
                                 f"{bw / HBM_PEAK:5.1%} of HBM")
                lines.append(f"    fused / composed, ratio of medians {st_['fused']['median'] / st_['composed']['median']:.3f}; spread of the "
                             f"composed leg's own repetitions (max - min) {st_['composed']['max'] - st_['composed']['min']:.2f} us")
    lines.append("")


def chain_step(GD, dev, args, lines):
    from UNet import UNetModel
    from bench import fill_weights
    torch.manual_seed(1234)
    m = UNetModel(img_size=32, base_channels=32, n_heads=2, attention_resolutions="16,8")
    fill_weights(m)
    m.to(dev).eval()
    d = GD.GaussianDiffusionModel([32, 32], GD.get_beta_schedule(T, "linear"), noise="gauss")
    d.seed_gauss(1234)
    g = torch.Generator().manual_seed(7)
    shape = (2, 1, 32, 32)
    x0 = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
    x_t, kz = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    keep = (torch.rand(shape, generator=g) > 0.5).to(dev)
    dist = args.inner + 3
    if dist > T:
        sys.exit(f"--inner must be at most {T - 3}")
    chains = {"unconditioned": GD.ReverseChain(d, m, x_t, dist, "gauss", use_graph=True),
              "known, fixed": GD.ReverseChain(d, m, x_t, dist, "gauss", use_graph=True, known=GD.KnownRegion(x0, keep, kz)),
              "known, fresh": GD.ReverseChain(d, m, x_t, dist, "gauss", use_graph=True, known=GD.KnownRegion(x0, keep, "fresh"))}
    times = {k: [] for k in chains}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(args.warmup + args.reps):
        for name, chain in chains.items():
            chain.reset(x_t, dist, stream_base=0)
            for _ in range(3):                                           # eager, capture, first replay (the first repetition)
                chain.step()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.inner):
                chain.step()
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    lines.append(f"(2) one chain step under graph replay, UNet 32^2 / base 32 / batch 2, seeded gaussian step noise, {args.inner} replayed "
                 "steps per repetition (event time includes the host's replay calls)")
    st = {k: stats(v) for k, v in times.items()}
    for k, s in st.items():
        lines.append(f"    {k:14s} {fmt(s)}")
    base = st["unconditioned"]
    for k in ("known, fixed", "known, fresh"):
        lines.append(f"    {k} - unconditioned, medians: {st[k]['median'] - base['median']:+.2f} us per step; the unconditioned leg's own "
                     f"repetitions spread over {base['max'] - base['min']:.2f} us")
    lines.append("  detection quality (AUC, Dice) under conditioning: not measured (no trained checkpoint)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_known.py measures on the device: no GPU visible")
    import GaussianDiffusion as GD
    dev = torch.device("cuda:0")
    d = GD.GaussianDiffusionModel([256, 256], GD.get_beta_schedule(T, "linear"), noise="gauss")
    lines = [f"known-region conditioning: device time by HIP events, legs alternating, {args.reps} repetitions after {args.warmup} warm-up; "
             f"launch legs are one replay of a captured graph of {args.inner} launches",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HBM peak used below {HBM_PEAK / 1e12:.1f} TB/s", ""]
    launches(d, GD, dev, args, lines)
    chain_step(GD, dev, args, lines)

    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
