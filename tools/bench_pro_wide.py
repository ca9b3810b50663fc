"""A/B of the one-workgroup AUPRO launch (anoddpm_pro_auc) against the chip-wide one (anoddpm_pro_auc_wide) on ONE pooled segment,
in one process, through the C ABI with preallocated outputs and workspaces, for n = 2^14, 2^16, ..., 2^22 and n = 5 767 168 (22
volumes x 4 slices x 256^2: the pooled segment of the reference's iterateKnown_restricted run), blob masks of a few regions per
plane, the areas from anoddpm_component_areas:
  workgroup leg   anoddpm_pro_auc of --parent-lib, a library built from the parent commit (ANODDPM_BUILD_TAG) (without the option:
                  of this build; the report says which)
  wide leg        anoddpm_pro_auc_wide of this build at the default tile
and, because the sort pass is now shared with csrc/roc_wide.hip, at n = 2^16 and 2^22
  parent leg      anoddpm_roc_auc_wide of --parent-lib
  this leg        anoddpm_roc_auc_wide of this build                (ROC only and with average precision + best Dice)
The legs alternate inside every repetition; each starts after a device synchronise and ends with the synchronising copy of its
[1] fp64 result.  Reported per leg: median, min, max and quartiles of the wall time and of the HIP-event time of the launches
alone.  Every output of two legs that are compared is checked bit for bit before anything is timed.  From those numbers: the
smallest measured power of two from which, at every larger size, the slowest wide repetition is below the fastest workgroup
repetition (the proposed PRO_WIDE_MIN_N); and whether the median of this build's roc_wide lies inside the parent's min .. max.

    python tools/bench_pro_wide.py [--reps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/pro_wide_ab.txt]"""
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
ROC_SIZES = (1 << 16, 1 << 22)


def make(n, dev):
    """n pixels as planes of 256 x 256 (128 x 128 for 2^14): three to six rectangular regions per plane, scores higher inside."""
    side = 256 if n >= 1 << 16 else 128
    planes = n // (side * side)
    assert planes * side * side == n
    rng = np.random.default_rng(8642)
    mask = np.zeros((planes, side, side), np.float32)
    for p in range(planes):
        for _ in range(int(rng.integers(3, 7))):
            h, w = rng.integers(1, side // 6, 2)
            y, x = rng.integers(0, side - h), rng.integers(0, side - w)
            mask[p, y:y + h, x:x + w] = 1
    score = (rng.random(mask.shape, dtype=np.float32) ** 2) * np.float32(0.9) + mask * rng.random(mask.shape, dtype=np.float32) * np.float32(0.35)
    return torch.from_numpy(mask).to(dev), torch.from_numpy(score.astype(np.float32)).to(dev)


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:9.3f} ms   min {s['min']:9.3f}   q25 {s['q25']:9.3f}   q75 {s['q75']:9.3f}   max {s['max']:9.3f}"


class ProLeg:
    """One prepared AUPRO launch: outputs, workspace and argument struct live as long as the object."""

    def __init__(self, _lib, entry, nbytes, score, areas, regions, tile=None):
        dev, n = score.device, score.numel()
        self.entry, self.tile, self.stream = entry, tile, _lib.current_stream
        self.out = {"aupro": torch.empty(1, dtype=torch.float64, device=dev), "counts": torch.empty((1, 4), dtype=torch.int64, device=dev),
                    "status": torch.empty(1, dtype=torch.int32, device=dev)}
        self.regions = regions.sum().reshape(1)                          # one plane of 1 x n: the kernels read the shape through n alone
        a = self.a = _lib.ProArgs()
        a.score, a.area, a.region_counts = score.data_ptr(), areas.data_ptr(), self.regions.data_ptr()
        a.aupro, a.counts, a.status = (self.out[k].data_ptr() for k in ("aupro", "counts", "status"))
        a.score_stride = a.area_stride = a.mask_stride = n
        a.limit, a.S, a.planes_per_segment, a.H, a.W = 0.3, 1, 1, 1, n
        self.ws = torch.empty(nbytes // 8 + 2, dtype=torch.float64, device=dev)
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), nbytes
        self.first = "aupro"

    def launch(self):
        rc = self.entry(ctypes.byref(self.a), self.stream()) if self.tile is None else self.entry(ctypes.byref(self.a), self.tile, self.stream())
        if rc != 0:
            raise RuntimeError(f"launch failed: {rc}")
        return self.out[self.first]

    def results(self):
        return {k: v.cpu().numpy().tobytes() for k, v in self.out.items()}


class RocLeg(ProLeg):
    """One prepared anoddpm_roc_auc_wide launch at the default tile."""

    def __init__(self, _lib, entry, nbytes, mask, score, full):
        dev, n = score.device, score.numel()
        self.entry, self.tile, self.stream = entry, 0, _lib.current_stream
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
        self.first = "auc"


def measure(legs, reps, warmup):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warmup):
        for leg in legs:
            leg.launch().cpu()
    wall, event = [[] for _ in legs], [[] for _ in legs]
    for _ in range(reps):
        for j, leg in enumerate(legs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record()
            r = leg.launch()
            e1.record()
            r.cpu()
            wall[j].append((time.perf_counter() - t) * 1e3)
            event[j].append(e0.elapsed_time(e1))
    return [stats(x) for x in wall], [stats(x) for x in event]


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
        sys.exit("bench_pro_wide.py measures on the device: no GPU visible")
    from anoddpm_amd import _lib, metrics
    L = _lib.lib()
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("anoddpm_pro_auc", "anoddpm_pro_workspace_bytes", "anoddpm_roc_auc_wide", "anoddpm_roc_wide_workspace_bytes"):
            getattr(parent, name).argtypes, getattr(parent, name).restype = getattr(L, name).argtypes, getattr(L, name).restype
        parent_kind = f"{args.parent_lib} (built from the parent commit)"
    else:
        parent, parent_kind = L, "THIS build (no --parent-lib given)"
    dev = torch.device("cuda:0")
    lines = [f"AUPRO of one pooled segment: one workgroup against the whole chip, same process, legs alternating, {args.reps} repetitions after "
             f"{args.warmup} warm-up; wall = launch to the end of the synchronising copy of the result, event = HIP events around the launches",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}; torch {torch.__version__}; "
             f"ABI {_lib.ABI_VERSION}",
             f"workgroup leg: anoddpm_pro_auc of {parent_kind}", "wide leg: anoddpm_pro_auc_wide, tile 0 (the default)", ""]
    wins = {}
    for n in SIZES:
        mask, score = make(n, dev)
        areas, regions = metrics.component_areas(mask, connectivity=2, batched=True)
        score = score.reshape(-1)
        legs = [ProLeg(_lib, parent.anoddpm_pro_auc, parent.anoddpm_pro_workspace_bytes(1, n), score, areas, regions),
                ProLeg(_lib, L.anoddpm_pro_auc_wide, L.anoddpm_pro_wide_workspace_bytes(1, n, 0), score, areas, regions, tile=0)]
        for leg in legs:
            leg.launch()
        torch.cuda.synchronize()
        assert legs[0].results() == legs[1].results(), f"n = {n}: the two paths differ"
        sw, se = measure(legs, args.reps, args.warmup)
        K, N, P, R = legs[1].out["counts"][0].tolist()
        lines.append(f"n = {n} ({-(-n // 4096)} tiles of 4096 elements; K {K} regions, P {P} pixels inside, {R} distinct scores, AUPRO "
                     f"{float(legs[1].out['aupro'][0]):.6f}); all outputs of both paths bit-identical")
        for j, name in enumerate(("workgroup", "wide     ")):
            lines.append(f"  {name} wall  {fmt(sw[j])}")
            lines.append(f"  {name} event {fmt(se[j])}")
        wins[n] = sw[1]["max"] < sw[0]["min"]
        lines += [f"  ratio of wall medians workgroup / wide: {sw[0]['median'] / sw[1]['median']:.2f}x; slowest wide repetition "
                  f"{'below' if wins[n] else 'NOT below'} the fastest workgroup repetition", ""]
        del legs
    pow2 = [n for n in SIZES if n & (n - 1) == 0]
    threshold = None
    for n in reversed(pow2):
        if not all(wins[m] for m in SIZES if m >= n):
            break
        threshold = n
    lines += [f"proposed PRO_WIDE_MIN_N (smallest measured power of two from which the wide path wins at every larger size): "
              f"{threshold if threshold is not None else 'none: leave the dispatch off'}",
              f"PRO_WIDE_MIN_N of this build: {metrics.PRO_WIDE_MIN_N}", ""]
    # the sort pass shared with roc_wide.hip: the parent's launch against this build's
    lines += [f"anoddpm_roc_auc_wide, tile 0: {parent_kind} against this build", ""]
    inside = True
    for n in ROC_SIZES:
        mask, score = make(n, dev)
        mask, score = mask.reshape(-1), score.reshape(-1)
        legs = []
        for full in (False, True):
            legs.append(RocLeg(_lib, parent.anoddpm_roc_auc_wide, parent.anoddpm_roc_wide_workspace_bytes(1, n, 0), mask, score, full))
            legs.append(RocLeg(_lib, L.anoddpm_roc_auc_wide, L.anoddpm_roc_wide_workspace_bytes(1, n, 0), mask, score, full))
        for leg in legs:
            leg.launch()
        torch.cuda.synchronize()
        for a, b in ((0, 1), (2, 3)):
            assert legs[a].results() == legs[b].results(), f"roc_wide, n = {n}: the two builds differ"
        sw, se = measure(legs, args.reps, args.warmup)
        lines.append(f"n = {n}; all outputs of both builds bit-identical")
        for j, name in enumerate(("parent ROC ", "this   ROC ", "parent full", "this   full")):
            lines.append(f"  {name} wall  {fmt(sw[j])}")
            lines.append(f"  {name} event {fmt(se[j])}")
        for a, b, what in ((0, 1, "ROC"), (2, 3, "full")):
            ok = sw[a]["min"] <= sw[b]["median"] <= sw[a]["max"] or sw[b]["median"] < sw[a]["min"]
            inside = inside and ok
            lines.append(f"  {what}: this build's wall median {sw[b]['median']:.3f} ms is {'inside or below' if ok else 'ABOVE'} the parent's "
                         f"min .. max {sw[a]['min']:.3f} .. {sw[a]['max']:.3f}")
        lines.append("")
        del legs
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not inside:
        sys.exit("roc_wide of this build is slower than the parent's")


if __name__ == "__main__":
    main()
