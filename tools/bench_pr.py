"""A/B of the precision-recall outputs (average precision, best Dice) of csrc/roc.hip on one device, in one process: for
(a) 1 x 256^2, (b) 55 x 256^2 (one detection_B sweep) and (c) 1 x 2^22 elements,
  1. cost of the new outputs: the combined launch (AUC + AP + best Dice) against the ROC-only launch of the same build.  DEVICE
     time: HIP events around a window of back-to-back launches that lasts at least --window seconds, divided by the launches in
     it; the two forms alternate, the pair is repeated --pairs times, and the spread over the repetitions is reported
  2. the ROC-only figures of 1. are what a run of this file with --roc-only in a checkout of the parent commit is compared with
     (that mode touches nothing the parent lacks); profiles/pr_curve_ab.txt records both
  3. native against host: HOST wall time of metrics.average_precision + best_dice results copied to the host (one launch, one
     sort) against what the product needed before: copy masks and maps to the host, then per map sklearn's
     precision_recall_curve + average_precision_score and a numpy scan of the Dice 2 P R / (P + R) over the curve (the same steps in
     numpy when sklearn cannot be imported; the report says which).  The two results are compared before anything is timed.

    python tools/bench_pr.py [--pairs 5] [--window 0.5] [--reps 10] [--roc-only] [--out profiles/pr_curve_ab.txt]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_leg_factory():
    def best_f1(prec, rec):
        with np.errstate(divide="ignore", invalid="ignore"):
            f1 = 2.0 * prec * rec / (prec + rec)                         # Dice of a binary prediction = F1 = 2 P R / (P + R)
        return float(np.nanmax(f1))
    try:
        from sklearn.metrics import average_precision_score, precision_recall_curve
        import sklearn

        def host(mask, score):
            prec, rec, _ = precision_recall_curve(mask, score)
            return average_precision_score(mask, score), best_f1(prec[:-1], rec[:-1])
        return host, f"sklearn {sklearn.__version__} (precision_recall_curve + average_precision_score) + numpy best-Dice scan"
    except ImportError:
        def host(mask, score):
            order = np.argsort(score, kind="stable")[::-1]
            y, t = score[order], mask[order]
            idx = np.r_[np.where(np.diff(y))[0], y.size - 1]
            tps = np.cumsum(t, dtype=np.float64)[idx]
            prec, rec = tps / (1.0 + idx), tps / tps[-1]
            return float(np.sum(np.diff(np.r_[0.0, rec]) * prec)), best_f1(prec, rec)
        return host, "numpy restatement of precision_recall_curve + average_precision_score + best-Dice scan; sklearn is not importable here"


def make(S, n, dev):
    g = torch.Generator(device="cpu").manual_seed(1234 + S)
    mask = (torch.rand(S, n, generator=g) < 0.03).float()
    base = torch.rand(S, n, generator=g)
    score = base * base * 0.9 + mask * torch.rand(S, n, generator=g) * 0.35
    return mask.to(dev), score.to(dev)


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
    ap.add_argument("--roc-only", action="store_true", help="time only the ROC-only launch (works in a checkout of the parent commit)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.window < 0.5 or args.pairs < 3:
        ap.error("--window must be at least 0.5 s and --pairs at least 3")
    if not torch.cuda.is_available():
        sys.exit("bench_pr.py measures on the device: no GPU visible")
    from anoddpm_amd import _lib, metrics
    dev = torch.device("cuda:0")
    host, host_kind = host_leg_factory()
    lines = [f"precision-recall outputs of csrc/roc.hip (ABI {_lib.ABI_VERSION}): {args.pairs} alternating repetitions, windows of at "
             f"least {args.window} s of back-to-back launches, every shape warmed first",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}",
             f"host leg: {host_kind}", ""]
    for label, S, n in (("(a) 1 x 256^2", 1, 65536), ("(b) 55 x 256^2", 55, 65536), ("(c) 1 x 2^22", 1, 1 << 22)):
        mask, score = make(S, n, dev)

        def roc_only():
            return metrics._roc_launch(mask, score, True, False)

        def combined():
            return metrics._roc_launch(mask, score, True, False, pr=True)

        legs = [("ROC-only launch (AUC)              ", roc_only)] + ([] if args.roc_only else [("combined launch (AUC + AP + best Dice)", combined)])
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
        lines.append(f"{label}: S = {S}, n = {n}")
        for name, _ in legs:
            lines.append(f"  DEVICE time per launch, {name}  {spread(t[name])}   [{launches[name]} launches per window]")
        if not args.roc_only:
            a, b = np.median(t[legs[0][0]]), np.median(t[legs[1][0]])
            lines.append(f"  cost of the new outputs: combined / ROC-only = {b / a:.4f} ({1e3 * (b - a):+.1f} us per launch, medians)")

            def host_leg():
                m, s = mask.cpu().numpy(), score.cpu().numpy()
                return np.array([host(m[j], s[j]) for j in range(S)])

            def native_leg():
                o = metrics._roc_launch(mask, score, True, False, pr=True)
                return np.stack([o["ap"].cpu().numpy(), o["best_dice"].cpu().numpy()], axis=1)

            h, d = host_leg(), native_leg()
            worst_ap, worst_dice = float(np.max(np.abs(h[:, 0] - d[:, 0]))), float(np.max(np.abs(h[:, 1] - d[:, 1])))
            assert worst_ap <= n * 2.0 ** -52 and worst_dice <= 1e-12, (label, worst_ap, worst_dice)
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
            lines += [f"  largest |ap_host - ap_native| = {worst_ap:.3g}, |dice_host - dice_native| = {worst_dice:.3g}",
                      f"  HOST wall time, host path   (copy + sklearn + scan)       {spread(th)}",
                      f"  HOST wall time, native path (launch + copy of results)    {spread(tn)}",
                      f"  ratio of medians host / native: {np.median(th) / np.median(tn):.0f}x"]
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
