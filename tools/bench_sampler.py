"""Measurements for the strided sampler on one device, in one process, device time by HIP events after warm-up:

  (1) the strided update launch (anoddpm_strided_update) against the ancestral one (anoddpm_p_sample_update[_gauss]) of the same
      build at 16 x 1 x 256^2, for the tensor-noise, no-noise and seeded forms.  Each leg is captured once as a HIP graph of
      `--inner` consecutive in-place steps (so the device, not the Python launch path, sets the pace); a repetition times one
      replay; the legs alternate inside every repetition.
  (2) the ancestral launch of this build against the ancestral launch of another build of the library (`--parent-lib`, a
      libanoddpm_hip.so built from the parent commit), the same three forms, the same way.  Both libraries run every repetition,
      and the parent runs TWICE per repetition (legs parent, this, parent again): the difference between the two parent legs is the
      margin the comparison is read against.  Without --parent-lib this part is "not measured".
  (3) one detection_B sweep of one image at 256^2 / base 128 with deterministic weights (the workload of `bench.py --config det`:
      t_distance 50 ... 550 step 50 x 5 chains, octave-simplex forward noise, gaussian step noise, 16 chain slots) with
      sampler=None and with StridedSampler(5) and StridedSampler(10) (eta = 0): seconds per image, chain steps (= UNet evaluations
      of single images) and batched steps.  `--no-sweep` skips it.

What a stride does to detection quality is NOT measured here or anywhere: there is no trained checkpoint to measure it with.

    python tools/bench_sampler.py [--reps 20] [--inner 100] [--warmup 3] [--parent-lib PATH] [--sweep-reps 2] [--no-sweep]
                                  [--out profiles/sampler_ab.txt]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
T = 1000
FORMS = ("tensor noise", "no noise", "seeded")
MOVED = {"tensor noise": 16, "no noise": 12, "seeded": 12}       # B/pixel of the ancestral launch; the strided one reads the noise
                                                                 # tensor only where sigma != 0 (eta 0.5 below: it does)


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:8.2f} us   min {s['min']:8.2f}   q25 {s['q25']:8.2f}   q75 {s['q75']:8.2f}   max {s['max']:8.2f}"


def time_legs(legs, reset, args):
    """legs: name -> callable (one in-place step).  -> name -> list of device microseconds per step."""
    graphs = {}
    for name, leg in legs.items():
        leg()                                                            # first launch outside the capture
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(args.inner):
                leg()
    times = {k: [] for k in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(args.warmup + args.reps):
        for name in legs:
            reset()
            torch.cuda.synchronize()
            e0.record()
            graphs[name].replay()
            e1.record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    return times


def update_args(d, x, t, eps, noise):
    from anoddpm_amd._lib import PUpdateArgs
    tb = d._tables(x.device)
    a = PUpdateArgs()
    a.x_prev = a.x_t = x.data_ptr()
    a.eps, a.noise, a.t = eps.data_ptr(), noise.data_ptr() if noise is not None else None, t.data_ptr()
    a.c_recip, a.c_recipm1 = tb.sqrt_recip_alphas_cumprod.data_ptr(), tb.sqrt_recipm1_alphas_cumprod.data_ptr()
    a.c_coef1, a.c_coef2, a.c_sigma = tb.posterior_mean_coef1.data_ptr(), tb.posterior_mean_coef2.data_ptr(), tb.sigma.data_ptr()
    a.B, a.T, a.n = x.shape[0], d.num_timesteps, x.numel() // x.shape[0]
    return a


def launches(d, GD, dev, args, lines):
    from anoddpm_amd import philox
    from anoddpm_amd._lib import PUpdateArgs, check, current_stream, lib, ptr
    B = 16
    g = torch.Generator().manual_seed(116)
    x0 = (torch.rand(B, 1, 256, 256, generator=g) * 2 - 1).to(dev)
    eps = torch.randn(B, 1, 256, 256, generator=g).to(dev)
    noise = torch.randn(B, 1, 256, 256, generator=g).to(dev)
    t = torch.linspace(T - 1, 60, B).long().to(dev)
    pixels = x0.numel()
    x = x0.clone()
    d.seed_gauss(1234)
    streams = philox.stream_ids(0, B).to(dev)
    sampler = GD.StridedSampler(5, 0.5)
    d._sampler_words(dev, sampler)

    def reset():
        x.copy_(x0)

    def ancestral(form):
        nz, st = (noise if form == "tensor noise" else None), (streams if form == "seeded" else None)
        return lambda: d._reverse_update(x, t, eps, nz, want_pred=False, out=x, gauss_streams=st)

    def strided(form):
        nz, st = (noise if form == "tensor noise" else None), (streams if form == "seeded" else None)
        return lambda: d._strided_update(x, t, eps, nz, None, want_pred=False, out=x, gauss_streams=st)

    lines.append(f"(1) strided update launch against the ancestral launch of the same build, {B} x 1 x 256^2 ({pixels} pixels), in place, "
                 f"stride 5, eta 0.5, t spread over 60 ... {T - 1}")
    for form in FORMS:
        st = {k: stats(v) for k, v in time_legs({"ancestral": ancestral(form), "strided": strided(form)}, reset, args).items()}
        lines.append(f"  {form}")
        for k, s in st.items():
            bw = MOVED[form] * pixels / (s["median"] * 1e-6)
            lines.append(f"    {k:9s} {fmt(s)}   {MOVED[form]} B/pixel = {bw / 1e9:6.0f} GB/s, {bw / HBM_PEAK:5.1%} of HBM")
        lines.append(f"    strided / ancestral, ratio of medians {st['strided']['median'] / st['ancestral']['median']:.3f}; spread of the "
                     f"ancestral leg's own repetitions (max - min) {st['ancestral']['max'] - st['ancestral']['min']:.2f} us")
    lines.append("")

    lines.append("(2) ancestral launch of this build against the ancestral launch of the parent commit's build, same inputs")
    if not args.parent_lib:
        lines += ["  not measured (no --parent-lib given)", ""]
        return
    P = ctypes.CDLL(os.path.abspath(args.parent_lib))
    P.anoddpm_last_error.restype = ctypes.c_char_p
    P.anoddpm_p_sample_update.argtypes = [ctypes.POINTER(PUpdateArgs), ctypes.c_void_p]
    P.anoddpm_p_sample_update_gauss.argtypes = [ctypes.POINTER(PUpdateArgs), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    assert not hasattr(P, "anoddpm_strided_update"), "--parent-lib exports anoddpm_strided_update: that is not the parent commit's library"
    seed = d._gauss_seed_dev(dev)

    def of(L, form):
        a = update_args(d, x, t, eps, noise if form == "tensor noise" else None)
        if form == "seeded":
            return lambda: check(L.anoddpm_p_sample_update_gauss(ctypes.byref(a), ptr(seed), ptr(streams), 0, current_stream()), "gauss")
        return lambda: check(L.anoddpm_p_sample_update(ctypes.byref(a), current_stream()), "update")

    for form in FORMS:
        reset()
        of(P, form)()
        want = x.clone()
        reset()
        of(lib(), form)()
        same = torch.equal(want, x)
        st = {k: stats(v) for k, v in time_legs({"parent": of(P, form), "this": of(lib(), form), "parent again": of(P, form)},
                                                reset, args).items()}
        lines.append(f"  {form}: results {'equal bit for bit' if same else 'DIFFER'}")
        for k, s in st.items():
            lines.append(f"    {k:12s} {fmt(s)}")
        margin = abs(st["parent again"]["median"] - st["parent"]["median"])
        diff = st["this"]["median"] - min(st["parent"]["median"], st["parent again"]["median"])
        lines.append(f"    this - faster parent leg, medians: {diff:+.2f} us; the two parent legs differ by {margin:.2f} us, a parent leg's "
                     f"own repetitions spread over {st['parent']['max'] - st['parent']['min']:.2f} us")
    lines.append("")


def sweep(GD, dev, args, lines):
    from UNet import UNetModel
    from bench import fill_weights, mri_like
    os.environ["ANODDPM_DET_SLOTS"] = "16"
    torch.manual_seed(1234)
    np.random.seed(1234)
    model = UNetModel(256, 128, channel_mults="", n_heads=2, attention_resolutions="16,8")
    fill_weights(model)
    model.to(dev).eval()
    diff = GD.GaussianDiffusionModel([256, 256], GD.get_beta_schedule(T, "linear"), noise="simplex")
    x0 = mri_like(1, 256, dev, seed=1234)
    mask = (mri_like(1, 256, dev, seed=99) > 0.2).float()
    dargs = {"arg_num": "bench", "T": T, "img_size": [256, 256]}
    lines.append("(3) one detection_B sweep of one image, 256^2, base 128, deterministic weights, T = 1000: t_distance 50 ... 550 step 50 x 5 "
                 "chains (octave-simplex forward noise, gaussian step noise), 16 chain slots, wall time around a synchronised call; "
                 "each setting warmed by a 16-chain sweep of three batched steps (plan, graph capture) before it is timed")
    base = None
    for sampler, reps in ((None, 1), (GD.StridedSampler(5), args.sweep_reps), (GD.StridedSampler(10), args.sweep_reps)):
        diff.sampler = sampler
        # warm-up, three batched steps: eager (plan), capture, replay
        diff._run_chains(model, x0, [3 * (sampler.stride if sampler else 1)] * 16, torch.randn(16, 1, 256, 256, device=dev))
        torch.cuda.synchronize()
        secs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            diff.detection_B(model, x0, dargs, ("bench", "image"), mask, denoise_fn="octave", total_avg=5)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        sched = diff.last_chain_schedule
        finite = all(torch.isfinite(r["mse"]).all().item() for r in diff.last_detection)
        name = "sampler=None (ancestral)" if sampler is None else f"stride {sampler.stride}, eta 0"
        if sampler is None:
            base = (min(secs), sched["chain_steps"])
        rel = "" if sampler is None else (f"; time / ancestral {min(secs) / base[0]:.3f}, chain steps / ancestral "
                                          f"{sched['chain_steps'] / base[1]:.3f}")
        lines.append(f"  {name:26s} {', '.join(f'{s:7.3f}' for s in secs)} s per image ({reps} run{'s' if reps > 1 else ''}); "
                     f"{sched['chain_steps']} chain steps (UNet evaluations of one image) in {sched['steps']} batched steps of "
                     f"{sched['slots']}; {1e3 * min(secs) / sched['chain_steps']:.3f} ms per chain step; outputs finite: {finite}{rel}")
    lines.append("  detection quality (AUC, Dice) under a stride: not measured (no trained checkpoint)")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--sweep-reps", type=int, default=2)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sampler.py measures on the device: no GPU visible")
    import GaussianDiffusion as GD
    dev = torch.device("cuda:0")
    d = GD.GaussianDiffusionModel([256, 256], GD.get_beta_schedule(T, "linear"), noise="gauss")
    lines = [f"strided sampler: device time by HIP events over one replay of a captured graph of {args.inner} launches, legs alternating, "
             f"{args.reps} repetitions after {args.warmup} warm-up",
             f"box: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HBM peak used below {HBM_PEAK / 1e12:.1f} TB/s", ""]
    launches(d, GD, dev, args, lines)
    if not args.no_sweep:
        sweep(GD, dev, args, lines)

    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
