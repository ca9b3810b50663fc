"""A/B of the one-workgroup ROC launch (anoddpm_roc_auc) against the chip-wide one (anoddpm_roc_auc_wide) on ONE segment, in one
process, through the C ABI with preallocated outputs and workspaces, for n = 2^14, 2^16, ..., 2^22 and n = 5 767 168 (22 volumes
x 4 slices x 256^2: the pooled segment of the reference's iterateKnown_restricted run):
  workgroup leg   anoddpm_roc_auc of --parent-lib, a library built from the parent commit that holds anoddpm_roc_auc and
                  anoddpm_roc_workspace_bytes (without the option: of this build; the report says which)
  wide leg        anoddpm_roc_auc_wide of this build at the default tile
each ROC-only (auc, counts, status) and with average precision + best Dice.  The four legs alternate inside every repetition;
each starts after a device synchronise and ends with the synchronising copy of its [1] fp64 result.  Reported per leg: median,
min, max and quartiles of the wall time and of the HIP-event time of the launches alone.  Every output of the two paths is compared
bit for bit before anything is timed.  From those numbers: the smallest measured power of two from which, at every larger size,
the slowest wide repetition is below the fastest workgroup repetition (the proposed ROC_WIDE_MIN_N); and at 1 x 256^2 and
1 x 128^2 the public metrics.roc_auc with the dispatch at its default and switched off.

    python tools/bench_roc_wide.py [--reps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/roc_wide_ab.txt]"""
import argparse
import ctypes
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = tuple(1 << k for k in range(14, 23, 2)) + (22 * 4 * 256 * 256,)
MUST_WIN = (1 << 22, 22 * 4 * 256 * 256)


def make(n, dev):
    g = torch.Generator(device="cpu").manual_seed(4321)
    mask = (torch.rand(n, generator=g) < 0.03).float()
    base = torch.rand(n, generator=g)
    score = base * base * 0.9 + mask * torch.rand(n, generator=g) * 0.35
    return mask.to(dev), score.to(dev)


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:9.3f} ms   min {s['min']:9.3f}   q25 {s['q25']:9.3f}   q75 {s['q75']:9.3f}   max {s['max']:9.3f}"


class Leg:
    """One prepared launch: outputs, workspace and argument struct live as long as the object."""

    def __init__(self, _lib, entry, nbytes, mask, score, full, tile=None):
        dev, n = score.device, score.numel()
        self.entry, self.tile, self.stream = entry, tile, _lib.current_stream
        self.out = {"auc": torch.empty(1, dtype=torch.float64, device=dev), "counts": torch.empty((1, 4), dtype=torch.int64, device=dev),
                    "status": torch.empty(1, dtype=torch.int32, device=dev)}
        a = self.a = _lib.RocArgs()
        a.score, a.mask, a.n, a.S, a.score_stride, a.mask_stride = score.data_ptr(), mask.data_ptr(), n, 1, n, n
        a.auc, a.counts, a.status = (self.out[k].data_ptr() for k in ("auc", "counts", "status"))
        if full:
            self.out.update(ap=torch.empty(1, dtype=torch.float64, device=dev), best_dice=torch.empty(1, dtype=torch.float64, device=dev),
                            best_thr=torch.empty(1, dtype=torch.float32, device=dev), best_counts=torch.empty((1, 2), dtype=torch.int64, device=dev))
            a.ap, a.best_dice, a.best_thr, a.best_counts = (self.out[k].data_ptr() for k in ("ap", "best_dice", "best_thr", "best_counts"))
        self.ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), nbytes

    def launch(self):
        rc = self.entry(ctypes.byref(self.a), self.stream()) if self.tile is None else self.entry(ctypes.byref(self.a), self.tile, self.stream())
        if rc != 0:
            raise RuntimeError(f"launch failed: {rc}")
        return self.out["auc"]

    def results(self):
        return {k: v.cpu().numpy().tobytes() for k, v in self.out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_roc_wide.py measures on the device: no GPU visible")
    from anoddpm_amd import _lib, metrics
    L = _lib.lib()
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.anoddpm_roc_auc.argtypes, parent.anoddpm_roc_auc.restype = L.anoddpm_roc_auc.argtypes, ctypes.c_int
        parent.anoddpm_roc_workspace_bytes.argtypes, parent.anoddpm_roc_workspace_bytes.restype = L.anoddpm_roc_workspace_bytes.argtypes, ctypes.c_int64
        parent_kind = f"anoddpm_roc_auc of {args.parent_lib} (built from the parent commit)"
    else:
        parent, parent_kind = L, "anoddpm_roc_auc of THIS build (no --parent-lib given)"
    dev = torch.device("cuda:0")
    lines = [f"ROC of one segment: one workgroup against the whole chip, same process, legs alternating, {args.reps} repetitions after "
             f"{args.warmup} warm-up; wall = launch to the end of the synchronising copy of the result, event = HIP events around the launches",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}; torch {torch.__version__}; "
             f"ABI {_lib.ABI_VERSION}",
             f"workgroup leg: {parent_kind}", "wide leg: anoddpm_roc_auc_wide, tile 0 (the default)", ""]
    names = ("workgroup ROC ", "wide      ROC ", "workgroup full", "wide      full")
    wins = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for n in SIZES:
        mask, score = make(n, dev)
        legs = []
        for full in (False, True):
            legs.append(Leg(_lib, parent.anoddpm_roc_auc, parent.anoddpm_roc_workspace_bytes(1, n), mask, score, full))
            legs.append(Leg(_lib, L.anoddpm_roc_auc_wide, L.anoddpm_roc_wide_workspace_bytes(1, n, 0), mask, score, full, tile=0))
        for leg in legs:
            leg.launch()
        torch.cuda.synchronize()
        for a, b in ((0, 1), (2, 3)):
            assert legs[a].results() == legs[b].results(), f"n = {n}: the two paths differ"
        for _ in range(args.warmup):
            for leg in legs:
                leg.launch().cpu()
        wall, event = [[] for _ in legs], [[] for _ in legs]
        for _ in range(args.reps):
            for j, leg in enumerate(legs):
                torch.cuda.synchronize()
                t = time.perf_counter()
                e0.record()
                r = leg.launch()
                e1.record()
                r.cpu()
                wall[j].append((time.perf_counter() - t) * 1e3)
                event[j].append(e0.elapsed_time(e1))
        sw, se = [stats(x) for x in wall], [stats(x) for x in event]
        tiles = -(-n // 4096)
        lines.append(f"n = {n} ({tiles} tiles of 4096 keys); all outputs of both paths bit-identical")
        for j, name in enumerate(names):
            lines.append(f"  {name} wall  {fmt(sw[j])}")
            lines.append(f"  {name} event {fmt(se[j])}")
        ok = [sw[1]["max"] < sw[0]["min"], sw[3]["max"] < sw[2]["min"]]
        wins[n] = all(ok)
        lines += [f"  ratio of wall medians workgroup / wide: ROC {sw[0]['median'] / sw[1]['median']:.2f}x, full {sw[2]['median'] / sw[3]['median']:.2f}x; "
                  f"slowest wide repetition {'below' if ok[0] else 'NOT below'} the fastest workgroup repetition (ROC), "
                  f"{'below' if ok[1] else 'NOT below'} (full)", ""]
        del legs
    pow2 = [n for n in SIZES if n & (n - 1) == 0]
    threshold = None
    for n in reversed(pow2):
        if not all(wins[m] for m in SIZES if m >= n):
            break
        threshold = n
    lines += [f"proposed ROC_WIDE_MIN_N (smallest measured power of two from which the wide path wins at every larger size): "
              f"{threshold if threshold is not None else 'none: leave the dispatch off'}",
              f"ROC_WIDE_MIN_N of this build: {metrics.ROC_WIDE_MIN_N}", ""]
    # the common cases through the public function, dispatch at its default against dispatch off: 1 x 256^2, and 1 x 128^2 which is
    # below every threshold this tool can propose (both settings run the same launch there: what is left is the dispatch itself)
    default = metrics.ROC_WIDE_MIN_N
    for label, n in (("1 x 256^2", 1 << 16), ("1 x 128^2", 1 << 14)):
        mask, score = make(n, dev)
        t_pub = {"default": [], "off": []}
        for rep in range(args.warmup + args.reps):
            for which, value in (("default", default), ("off", 1 << 31)):
                metrics.ROC_WIDE_MIN_N = value
                torch.cuda.synchronize()
                t = time.perf_counter()
                metrics.roc_auc(mask, score, batched=False).cpu()
                if rep >= args.warmup:
                    t_pub[which].append((time.perf_counter() - t) * 1e3)
        metrics.ROC_WIDE_MIN_N = default
        path = metrics._roc_launch(mask, score, False, curve=False)["path"]
        lines += [f"{label} through metrics.roc_auc (wall, with the copy of the result); the default takes the {path} path:",
                  f"  dispatch at its default  {fmt(stats(t_pub['default']))}",
                  f"  dispatch switched off    {fmt(stats(t_pub['off']))}", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not all(wins[n] for n in MUST_WIN):
        sys.exit("the wide path is not faster than the one-workgroup path at 2^22 or at 5 767 168")


if __name__ == "__main__":
    main()
