"""A/B of the reverse update's gaussian step noise on one device, in one process, at 4 x 1 x 256^2 and 16 x 1 x 256^2:
  pair leg   torch.randn_like + anoddpm_p_sample_update with the noise tensor (two launches; 4 B/pixel written and 16 B/pixel
             moved by the update) -- what an unseeded chain step does after the UNet forward
  fused leg  anoddpm_p_sample_update_gauss (one launch, 12 B/pixel, the normals made in registers) -- a seeded chain step
Both update x in place, as ReverseChain does.  Each leg is captured once as a HIP graph of `--inner` consecutive steps (so that the
device, not the Python launch path, sets the pace, as in the product's graph-replayed chain step); a repetition times one replay
between two HIP events (device time per step = elapsed / inner); the legs alternate inside every repetition.  Before anything is timed the fused
launch is compared bit for bit with anoddpm_philox_fill + anoddpm_p_sample_update.

On a tree without the seeded path (the parent commit) only the pair leg runs: copy this file there for the parent's numbers.

    python tools/bench_gauss.py [--reps 20] [--inner 100] [--warmup 3] [--out profiles/gauss_fused_ab.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
T = 1000


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:8.2f} us   min {s['min']:8.2f}   q25 {s['q25']:8.2f}   q75 {s['q75']:8.2f}   max {s['max']:8.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_gauss.py measures on the device: no GPU visible")
    import GaussianDiffusion as GD
    dev = torch.device("cuda:0")
    d = GD.GaussianDiffusionModel([256, 256], GD.get_beta_schedule(T, "linear"), noise="gauss")
    has_fused = hasattr(d, "seed_gauss")
    lines = [f"gaussian step noise of the reverse update: torch.randn_like + p_sample_update against p_sample_update_gauss"
             f"{'' if has_fused else ' (this tree has no seeded path: pair leg only)'}; device time by HIP events over one replay of a captured graph of "
             f"{args.inner} steps, legs alternating, {args.reps} repetitions after {args.warmup} warm-up",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HBM peak used below {HBM_PEAK / 1e12:.1f} TB/s", ""]
    for B in (4, 16):
        g = torch.Generator().manual_seed(100 + B)
        x0 = (torch.rand(B, 1, 256, 256, generator=g) * 2 - 1).to(dev)
        eps = torch.randn(B, 1, 256, 256, generator=g).to(dev)
        t = torch.linspace(T - 1, 60, B).long().to(dev)
        pixels = x0.numel()
        x = x0.clone()

        def pair():
            d._reverse_update(x, t, eps, torch.randn_like(x), want_pred=False, out=x)

        legs = {"pair": pair}
        if has_fused:
            from anoddpm_amd import philox
            d.seed_gauss(1234)
            streams = philox.stream_ids(0, B).to(dev)
            noise = philox.normal(d._gauss_seed_dev(dev), x0.shape, stream=streams, step=t, domain=0, T=T)
            ref = d._reverse_update(x0, t, eps, noise, want_pred=False)[0]
            got = d._reverse_update(x0, t, eps, None, want_pred=False, gauss_streams=streams)[0]
            assert torch.equal(ref, got), "fused update differs from fill + update"
            legs["fused"] = lambda: d._reverse_update(x, t, eps, None, want_pred=False, out=x, gauss_streams=streams)
        times = {k: [] for k in legs}
        graphs = {}
        for name, leg in legs.items():
            leg()                                                        # first launch outside the capture
            torch.cuda.synchronize()
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(args.inner):
                    leg()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rep in range(args.warmup + args.reps):
            for name in legs:
                x.copy_(x0)
                torch.cuda.synchronize()
                e0.record()
                graphs[name].replay()
                e1.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.inner)
        lines.append(f"{B} x 1 x 256^2 ({pixels} pixels){': fused == fill + update bit for bit' if has_fused else ''}")
        st = {k: stats(v) for k, v in times.items()}
        moved = {"pair": 20, "fused": 12}
        for k, s in st.items():
            bw = moved[k] * pixels / (s["median"] * 1e-6)
            lines.append(f"  {k:5s} {fmt(s)}   {moved[k]} B/pixel = {bw / 1e9:6.0f} GB/s, {bw / HBM_PEAK:5.1%} of HBM")
        if has_fused:
            verdict = "no slower" if st["fused"]["median"] <= st["pair"]["median"] else "SLOWER"
            lines.append(f"  fused / pair, ratio of medians: {st['fused']['median'] / st['pair']['median']:.2f} ({verdict}); spread of the "
                         f"pair leg's own repetitions (max - min) {st['pair']['max'] - st['pair']['min']:.2f} us")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
