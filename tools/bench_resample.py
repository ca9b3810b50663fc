"""Measurements for resampling jumps on one device, in one process, device time by HIP events after warm-up:

  (1) the fused resample launch (anoddpm_p_sample_update_resample) with EVERY sample jumping -- its costliest case -- against the
      composition it replaces, built from the entry points the library had before it: the conditioned launch
      (anoddpm_p_sample_update_known) into a scratch plane, a fill of the re-noise (in-kernel-noise form only: anoddpm_philox_fill,
      domain 4 at the landing level), anoddpm_q_sample with the (A, C) jump tables at the level the step lands on, and an ATen
      `where` on the jump flag into x; and against the conditioned launch alone, which is what a step costs without resampling.
      Cases 16 x 1 x 256^2 and 1 x 1 x 256^2, tensor noise (all three noises read from planes) and in-kernel noise (all three
      generated).  Each leg is captured once as a HIP graph of `--inner` consecutive launches; a repetition times one replay; the
      legs alternate inside every repetition.  The fused and the composed leg are checked to leave the same bits in x first.
  (2) one chain step under graph replay with and without resampling, on the smallest UNet the sampler tests build (32^2, base 32,
      batch 2, deterministic weights), seeded: unconditioned, conditioned, conditioned + Resampling(10, 2) for noise="fixed" and
      "fresh"; `--inner` replayed steps per repetition, legs alternating.  The resampled legs take their jumps on the way.

What resampling does to detection quality is NOT measured here or anywhere: there is no trained checkpoint to measure it with.

    python tools/bench_resample.py [--reps 20] [--inner 100] [--warmup 3] [--out profiles/resample_ab.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_known import HBM_PEAK, T, capture, fmt, stats, time_graphs  # noqa: E402

JUMP = 10
# bytes per pixel: x_t, eps, x0 read and x_prev written (16), one keep byte, and in the tensor form the three noise planes
MOVED = {"fused": {"tensor noise": 16 + 1 + 12, "in-kernel noise": 16 + 1},
         # known launch (-> u), [fill -> rz], q_sample (u, rz -> q), where (q, u -> x)
         "composed": {"tensor noise": 25 + 12 + 12, "in-kernel noise": 17 + 4 + 12 + 12},
         "known alone": {"tensor noise": 16 + 1 + 8, "in-kernel noise": 16 + 1}}
LAUNCHES = {"fused": {"tensor noise": 1, "in-kernel noise": 1}, "composed": {"tensor noise": 3, "in-kernel noise": 4},
            "known alone": {"tensor noise": 1, "in-kernel noise": 1}}


def jump_tables(d, dev):
    """fp32 A[s], C[s] of the jump from s to s + JUMP: fp64, each rounded once (1, 0 where s + JUMP leaves the schedule)."""
    acp = np.asarray(d.alphas_cumprod, dtype=np.float64)
    ratio = np.ones(T)
    ratio[:T - JUMP] = acp[JUMP:] / acp[:T - JUMP]
    return (torch.from_numpy(np.sqrt(ratio).astype(np.float32)).to(dev), torch.from_numpy(np.sqrt(1.0 - ratio).astype(np.float32)).to(dev))


def launches(d, GD, dev, args, lines):
    from anoddpm_amd import philox
    from anoddpm_amd._lib import PHILOX_RENOISE, check, current_stream, lib, ptr
    d.seed_gauss(1234)
    seed = d._gauss_seed_dev(dev)
    A, C = jump_tables(d, dev)
    lines.append(f"(1) fused resample launch, every sample jumping (jump {JUMP}), against the composition of the earlier entry points "
                 "and against the conditioned launch alone; in place on x, t spread over 981 ... 61, mask: half of the pixels kept")
    for B in (16, 1):
        g = torch.Generator().manual_seed(216 + B)
        shape = (B, 1, 256, 256)
        x_start = torch.randn(shape, generator=g).to(dev)
        x0 = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
        eps, noise, kz, rz = (torch.randn(shape, generator=g).to(dev) for _ in range(4))
        keep8 = (torch.rand(shape, generator=g) > 0.5).to(dev).to(torch.uint8)
        t = (torch.linspace(98, 6, B).round().long() * JUMP + 1).to(dev)          # every s = t - 1 is a jump point below top
        s, land = t - 1, t - 1 + JUMP
        i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)
        state = (torch.tensor([JUMP], dtype=torch.int32, device=dev), torch.tensor([2], dtype=torch.int32, device=dev),
                 i32(T - 1), i32(1), i32(0))
        flag = torch.ones((B, 1, 1, 1), dtype=torch.bool, device=dev)
        streams = philox.stream_ids(0, B).to(dev)
        pixels, n = x0.numel(), x0.numel() // B
        x, u, q, rfill = x_start.clone(), torch.empty(shape, device=dev), torch.empty(shape, device=dev), torch.empty(shape, device=dev)

        def reset():
            x.copy_(x_start)

        for form in ("tensor noise", "in-kernel noise"):
            nz, st, kplane, rplane = (noise, None, kz, rz) if form == "tensor noise" else (None, streams, None, None)

            def fused():
                d._known_update(x, t, eps, nz, (x0, keep8, kplane), None, want_pred=False, out=x, gauss_streams=st, resample=state + (rplane,))

            def known_alone():
                d._known_update(x, t, eps, nz, (x0, keep8, kplane), None, want_pred=False, out=x, gauss_streams=st)

            def composed():
                d._known_update(x, t, eps, nz, (x0, keep8, kplane), None, want_pred=False, out=u, gauss_streams=st)
                plane = rz
                if form == "in-kernel noise":
                    check(lib().anoddpm_philox_fill(ptr(rfill), 1, B, n, ptr(seed), ptr(streams), 0, PHILOX_RENOISE, ptr(land), 0, T,
                                                    current_stream()), "philox_fill")
                    plane = rfill
                check(lib().anoddpm_q_sample(ptr(q), ptr(u), ptr(plane), ptr(s), ptr(A), ptr(C), B, n, T, current_stream()), "q_sample")
                torch.where(flag, q, u, out=x)

            reset()
            fused()
            got = x.clone()
            reset()
            composed()
            same = torch.equal(got, x)
            graphs = {"composed": capture(composed, args.inner), "fused": capture(fused, args.inner),
                      "known alone": capture(known_alone, args.inner)}
            st_ = {k: stats(v) for k, v in time_graphs(graphs, reset, args).items()}
            lines.append(f"  {B} x 1 x 256^2, {form}: fused and composed results {'equal bit for bit' if same else 'DIFFER'}")
            for k in ("composed", "fused", "known alone"):
                moved, nl = MOVED[k][form], LAUNCHES[k][form]
                bw = moved * pixels / (st_[k]["median"] * 1e-6)
                lines.append(f"    {k:11s} {fmt(st_[k])}   {nl} launch{'es' if nl > 1 else ''}, {moved} B/pixel = {bw / 1e9:6.0f} GB/s, "
                             f"{bw / HBM_PEAK:5.1%} of HBM")
            lines.append(f"    fused / composed, ratio of medians {st_['fused']['median'] / st_['composed']['median']:.3f}; fused - known alone "
                         f"{st_['fused']['median'] - st_['known alone']['median']:+.2f} us; spread of the composed leg's own repetitions "
                         f"(max - min) {st_['composed']['max'] - st_['composed']['min']:.2f} us")
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
    dist = T
    if args.inner + 3 > T:
        sys.exit(f"--inner must be at most {T - 3}")
    res = GD.Resampling(JUMP, 2)
    fixed, fresh = GD.KnownRegion(x0, keep, kz), GD.KnownRegion(x0, keep, "fresh")
    chains = {"unconditioned": GD.ReverseChain(d, m, x_t, dist, "gauss", use_graph=True),
              "known, fixed": GD.ReverseChain(d, m, x_t, dist, "gauss", use_graph=True, known=fixed),
              "resample, fixed": GD.ReverseChain(d, m, x_t, dist, "gauss", use_graph=True, known=fixed, resampling=res),
              "known, fresh": GD.ReverseChain(d, m, x_t, dist, "gauss", use_graph=True, known=fresh),
              "resample, fresh": GD.ReverseChain(d, m, x_t, dist, "gauss", use_graph=True, known=fresh, resampling=res)}
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
    jumps = int(chains["resample, fixed"].rs_visit[0])
    lines.append(f"(2) one chain step under graph replay, UNet 32^2 / base 32 / batch 2, seeded gaussian step noise, {args.inner} replayed "
                 f"steps per repetition (event time includes the host's replay calls); Resampling({JUMP}, 2): {jumps} jumps taken in the "
                 "steps of one repetition")
    st = {k: stats(v) for k, v in times.items()}
    for k, s in st.items():
        lines.append(f"    {k:16s} {fmt(s)}")
    base = st["unconditioned"]
    for k, ref in (("resample, fixed", "known, fixed"), ("resample, fresh", "known, fresh")):
        lines.append(f"    {k} - {ref}, medians: {st[k]['median'] - st[ref]['median']:+.2f} us per step; - unconditioned: "
                     f"{st[k]['median'] - base['median']:+.2f} us; the unconditioned leg's own repetitions spread over "
                     f"{base['max'] - base['min']:.2f} us")
    lines.append("  detection quality (AUC, Dice) under resampling: not measured (no trained checkpoint)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_resample.py measures on the device: no GPU visible")
    import GaussianDiffusion as GD
    dev = torch.device("cuda:0")
    d = GD.GaussianDiffusionModel([256, 256], GD.get_beta_schedule(T, "linear"), noise="gauss")
    lines = [f"resampling jumps: device time by HIP events, legs alternating, {args.reps} repetitions after {args.warmup} warm-up; "
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
