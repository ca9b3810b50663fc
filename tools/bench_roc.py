"""A/B of the ROC / AUC paths on one device, in one process: for (a) 1 x 256^2, (b) 55 x 256^2 (one detection_B sweep) and
(c) 1 x 2^22 elements,
  host leg   what the product did before the native kernel: copy masks and maps to the host, then per segment the stable sort,
             the curve with sklearn's drop rule and the trapezoid area (sklearn.metrics.roc_curve + auc when sklearn can be
             imported, else the same steps in numpy with np.argsort(kind="stable"); the report says which)
  native leg metrics.roc_auc plus the copy of the [S] result
Both legs start from the same device tensors after a device synchronise and end with their synchronising copy; they alternate
inside every repetition.  Reported: median, min, max and quartiles of the wall time per leg, and the HIP-event time of the native
launch alone.  The two results are compared (n * 2^-52) before anything is timed.

    python tools/bench_roc.py [--reps 20] [--warmup 3] [--out profiles/roc_auc_ab.txt]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_leg_factory():
    try:
        from sklearn.metrics import auc, roc_curve
        import sklearn

        def host_auc(mask, score):
            fpr, tpr, _ = roc_curve(mask, score)
            return auc(fpr, tpr)
        return host_auc, f"sklearn {sklearn.__version__} (roc_curve + auc)"
    except ImportError:
        def host_auc(mask, score):
            order = np.argsort(score, kind="stable")[::-1]
            y, t = score[order], (mask[order] == 1)
            idx = np.r_[np.where(np.diff(y))[0], y.size - 1]
            tps = np.cumsum(t, dtype=np.float64)[idx]
            fps = 1 + idx - tps
            if len(fps) > 2:
                keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
                fps, tps = fps[keep], tps[keep]
            fps, tps = np.r_[0, fps], np.r_[0, tps]
            fpr, tpr = fps / fps[-1], tps / tps[-1]
            return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2))
        return host_auc, "numpy restatement of roc_curve + auc (np.argsort(kind='stable')); sklearn is not importable here"


def make(S, n, dev):
    g = torch.Generator(device="cpu").manual_seed(1234 + S)
    mask = (torch.rand(S, n, generator=g) < 0.03).float()
    base = torch.rand(S, n, generator=g)
    score = base * base * 0.9 + mask * torch.rand(S, n, generator=g) * 0.35
    return mask.to(dev), score.to(dev)


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
        sys.exit("bench_roc.py measures on the device: no GPU visible")
    from anoddpm_amd import metrics
    dev = torch.device("cuda:0")
    host_auc, host_kind = host_leg_factory()
    lines = [f"ROC / AUC: host path of the parent commit against metrics.roc_auc, same process, legs alternating, {args.reps} repetitions "
             f"after {args.warmup} warm-up",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}",
             f"host leg: {host_kind}", ""]
    verdicts = []
    for label, S, n in (("(a) 1 x 256^2", 1, 65536), ("(b) 55 x 256^2", 55, 65536), ("(c) 1 x 2^22", 1, 1 << 22)):
        mask, score = make(S, n, dev)

        def host_leg():
            m, s = mask.cpu().numpy(), score.cpu().numpy()              # the D2H copies the parent's ROC_AUC makes
            return np.array([host_auc(m[j], s[j]) for j in range(S)])

        def native_leg():
            return metrics.roc_auc(mask, score, batched=True).cpu().numpy()

        h, d = host_leg(), native_leg()
        worst = float(np.max(np.abs(h - d)))
        assert worst <= n * 2.0 ** -52, (label, worst)
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
            r = metrics.roc_auc(mask, score, batched=True)
            e1.record()
            r.cpu()
            t_native.append((time.perf_counter() - t) * 1e3)
            t_event.append(e0.elapsed_time(e1))
        sh, sn, se = stats(t_host), stats(t_native), stats(t_event)
        faster = sn["max"] < sh["min"]
        verdicts.append((label, faster, sh["median"] / sn["median"]))
        lines += [f"{label}: S = {S}, n = {n}; largest |auc_host - auc_native| = {worst:.3g}",
                  f"  host   (copy + sort + curve + area)   {fmt(sh)}",
                  f"  native (roc_auc + copy of [S] fp64)   {fmt(sn)}",
                  f"  native launch alone (HIP events)      {fmt(se)}",
                  f"  ratio of medians host / native: {sh['median'] / sn['median']:.1f}x; slowest native repetition "
                  f"{'below' if faster else 'NOT below'} the fastest host repetition", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not all(f for lbl, f, _ in verdicts if not lbl.startswith("(c)")):
        sys.exit("the native path is not faster than the host path at (a) or (b)")


if __name__ == "__main__":
    main()
