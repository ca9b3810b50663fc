"""Device time of the chip-wide select (anoddpm_select_wide) at Q = 1 and Q = 4 ranks on ONE segment, in one process, through the C
ABI with preallocated outputs and workspaces, for n = 65 536, 5 767 168 (22 volumes x 4 slices x 256^2: a pooled healthy set of
the size of the reference's iterateKnown_restricted run), 2^24 and 2^26, against every other way to an order statistic:
  one workgroup   anoddpm_map_scores, k = rank + 1                                       (n <= 2^24: above it the call is refused)
  sort route      anoddpm_roc_auc_wide on the same values with an all-zero mask: the only other chip-wide way
  host route      copy to the host + numpy.partition                                     (wall time only; --host-reps repetitions)
The device legs alternate inside every repetition; each starts after a device synchronise and ends with the synchronising copy
of one of its results.  Reported per leg: median, min, max and quartiles of the wall time and of the HIP-event time of the launches
alone.  Before anything is timed the selected value is compared with numpy.partition, and for n <= 2^24 every output of the Q = 1
select with what anoddpm_map_scores writes, bit for bit.
Then anoddpm_threshold_counts at T = 1 and T = 8 on the 55 maps of 256^2 of a sweep against T launches of anoddpm_anomaly_map
(one host threshold each; counts only).

    python tools/bench_select.py [--reps 20] [--warmup 3] [--host-reps 5] [--out profiles/select_ab.txt]"""
import argparse
import ctypes
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (1 << 16, 22 * 4 * 256 * 256, 1 << 24, 1 << 26)
SWEEP = (55, 256 * 256)


def make(n, dev):
    g = torch.Generator(device="cpu").manual_seed(4321)
    base = torch.rand(n, generator=g)
    return ((base * base) * (base * base) * 3.0).to(dev)         # like squared errors: many small values, a few large


def stats(x):
    x = np.sort(np.asarray(x))
    q = np.percentile(x, [25, 50, 75])
    return {"median": q[1], "min": x[0], "max": x[-1], "q25": q[0], "q75": q[2]}


def fmt(s):
    return f"median {s['median']:9.3f} ms   min {s['min']:9.3f}   q25 {s['q25']:9.3f}   q75 {s['q75']:9.3f}   max {s['max']:9.3f}"


class SelectLeg:
    def __init__(self, _lib, L, score, ranks):
        dev, n, Q = score.device, score.numel(), len(ranks)
        self.L, self.stream = L, _lib.current_stream
        self.table = torch.tensor(ranks, dtype=torch.int32, device=dev)
        self.host = (ctypes.c_uint32 * Q)(*ranks)
        nbytes = L.anoddpm_select_wide_workspace_bytes(n, Q, 0)
        self.ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        self.out = {"value": torch.empty((1, Q), dtype=torch.float32, device=dev), "above": torch.empty((1, Q), dtype=torch.int64, device=dev),
                    "equal": torch.empty((1, Q), dtype=torch.int64, device=dev), "topk": torch.empty((1, Q), dtype=torch.float64, device=dev),
                    "max": torch.empty(1, dtype=torch.float32, device=dev), "mean": torch.empty(1, dtype=torch.float64, device=dev),
                    "status": torch.empty(1, dtype=torch.int32, device=dev)}
        a = self.a = _lib.SelectArgs()
        a.src, a.ranks, a.ranks_host, a.workspace, a.workspace_bytes = score.data_ptr(), self.table.data_ptr(), ctypes.addressof(self.host), self.ws.data_ptr(), nbytes
        a.value, a.above, a.equal, a.topk_mean = (self.out[k].data_ptr() for k in ("value", "above", "equal", "topk"))
        a.max, a.mean, a.status = (self.out[k].data_ptr() for k in ("max", "mean", "status"))
        a.src_stride, a.n, a.S, a.Q = n, n, 1, Q

    def launch(self):
        if self.L.anoddpm_select_wide(ctypes.byref(self.a), 0, self.stream()) != 0:
            raise RuntimeError("select_wide failed: " + self.L.anoddpm_last_error().decode())
        return self.out["value"]


class WorkgroupLeg:
    def __init__(self, _lib, L, score, k):
        dev, n = score.device, score.numel()
        self.L, self.stream = L, _lib.current_stream
        self.out = {"max": torch.empty(1, dtype=torch.float32, device=dev), "mean": torch.empty(1, dtype=torch.float64, device=dev),
                    "topk": torch.empty(1, dtype=torch.float64, device=dev), "status": torch.empty(1, dtype=torch.int32, device=dev)}
        a = self.a = _lib.MapScoresArgs()
        a.src, a.max, a.mean, a.topk_mean, a.status = (score.data_ptr(),) + tuple(self.out[k_].data_ptr() for k_ in ("max", "mean", "topk", "status"))
        a.src_stride, a.n, a.k, a.S = n, n, k, 1

    def launch(self):
        if self.L.anoddpm_map_scores(ctypes.byref(self.a), self.stream()) != 0:
            raise RuntimeError("map_scores failed: " + self.L.anoddpm_last_error().decode())
        return self.out["topk"]


class SortLeg:
    def __init__(self, _lib, L, score, mask):
        dev, n = score.device, score.numel()
        self.L, self.stream = L, _lib.current_stream
        self.out = {"auc": torch.empty(1, dtype=torch.float64, device=dev), "counts": torch.empty((1, 4), dtype=torch.int64, device=dev),
                    "status": torch.empty(1, dtype=torch.int32, device=dev)}
        nbytes = L.anoddpm_roc_wide_workspace_bytes(1, n, 0)
        self.ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        a = self.a = _lib.RocArgs()
        a.score, a.mask, a.n, a.S, a.score_stride, a.mask_stride = score.data_ptr(), mask.data_ptr(), n, 1, n, n
        a.auc, a.counts, a.status = (self.out[k].data_ptr() for k in ("auc", "counts", "status"))
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), nbytes

    def launch(self):
        if self.L.anoddpm_roc_auc_wide(ctypes.byref(self.a), 0, self.stream()) != 0:
            raise RuntimeError("roc_auc_wide failed: " + self.L.anoddpm_last_error().decode())
        return self.out["counts"]


class CountsLeg:
    def __init__(self, _lib, L, score, mask, thr):
        dev, (S, n), T = score.device, score.shape, thr.numel()
        self.L, self.stream, self.thr = L, _lib.current_stream, thr
        self.counts = torch.empty((S, T, 2), dtype=torch.int64, device=dev)
        self.totals = torch.empty((S, 2), dtype=torch.int64, device=dev)
        self.status = torch.empty(S, dtype=torch.int32, device=dev)
        a = self.a = _lib.ThresholdCountsArgs()
        a.score, a.mask, a.thr, a.counts, a.totals, a.status = score.data_ptr(), mask.data_ptr(), thr.data_ptr(), self.counts.data_ptr(), self.totals.data_ptr(), self.status.data_ptr()
        a.n, a.score_stride, a.mask_stride, a.thr_stride, a.S, a.T = n, n, n, 0, S, T

    def launch(self):
        if self.L.anoddpm_threshold_counts(ctypes.byref(self.a), self.stream()) != 0:
            raise RuntimeError("threshold_counts failed: " + self.L.anoddpm_last_error().decode())
        return self.counts


class AnomalyLeg:
    """T launches of anoddpm_anomaly_map, one host threshold each, counts only: with real = 0 its squared error is recon * recon,
    the score the other leg reads."""

    def __init__(self, _lib, L, recon, mask, thresholds):
        dev, (B, n) = recon.device, recon.shape
        self.L, self.stream, self.thresholds = L, _lib.current_stream, thresholds
        self.recon, self.real = recon, torch.zeros_like(recon)
        self.counts = torch.zeros((len(thresholds), B, _lib.ANOMALY_NCOUNTS), dtype=torch.float64, device=dev)
        self.ws = torch.empty(_lib.ANOMALY_BLOCKS * B * _lib.ANOMALY_NCOUNTS, dtype=torch.float64, device=dev)
        self.args = []
        for j, t in enumerate(thresholds):
            a = _lib.AnomalyArgs()
            a.recon, a.real, a.mask, a.counts = self.recon.data_ptr(), self.real.data_ptr(), mask.data_ptr(), self.counts[j].data_ptr()
            a.workspace, a.workspace_doubles, a.n, a.recon_as, a.recon_bs, a.navg, a.B, a.threshold = self.ws.data_ptr(), self.ws.numel(), n, B * n, n, 1, B, float(t)
            self.args.append(a)

    def launch(self):
        for a in self.args:
            if self.L.anoddpm_anomaly_map(ctypes.byref(a), self.stream()) != 0:
                raise RuntimeError("anomaly_map failed: " + self.L.anoddpm_last_error().decode())
        return self.counts


def time_legs(legs, reps, warmup):
    """-> (wall stats, event stats) per leg; the legs alternate inside every repetition."""
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
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_select.py measures on the device: no GPU visible")
    from anoddpm_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    lines = [f"order statistics of one segment: the chip-wide select against one workgroup, the chip-wide sort and the host, same process, "
             f"device legs alternating, {args.reps} repetitions after {args.warmup} warm-up; wall = launch to the end of the synchronising "
             f"copy of a result, event = HIP events around the launches",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}; torch {torch.__version__}; "
             f"ABI {_lib.ABI_VERSION}",
             "select legs: anoddpm_select_wide, tile 0 (the default), 11 launches; rank n / 100 at Q = 1; ranks 0, n / 1000, n / 100, n / 20 at Q = 4", ""]
    for n in SIZES:
        score = make(n, dev)
        mask = torch.zeros(n, dtype=torch.float32, device=dev)
        r1, r4 = [n // 100], [0, n // 1000, n // 100, n // 20]
        legs, names = [SelectLeg(_lib, L, score, r1), SelectLeg(_lib, L, score, r4)], ["select Q = 1    ", "select Q = 4    "]
        if n <= _lib.MAP_SCORES_MAX_N:
            legs.append(WorkgroupLeg(_lib, L, score, r1[0] + 1))
            names.append("one workgroup   ")
        legs.append(SortLeg(_lib, L, score, mask))
        names.append("sort route      ")
        for leg in legs:
            leg.launch()
        torch.cuda.synchronize()
        host = score.cpu().numpy()
        want = np.partition(host, n - 1 - np.array(r4))[n - 1 - np.array(r4)]
        assert legs[1].out["value"].cpu().numpy()[0].tobytes() == want.tobytes(), f"n = {n}: the selected values differ from numpy.partition's"
        assert legs[0].out["value"].cpu().numpy()[0, 0] == want[2]
        checked = "values equal numpy.partition's"
        if n <= _lib.MAP_SCORES_MAX_N:
            for a, b in (("max", "max"), ("mean", "mean"), ("topk", "topk"), ("status", "status")):
                assert legs[0].out[a].cpu().numpy().tobytes() == legs[2].out[b].cpu().numpy().tobytes(), f"n = {n}: {a} differs from map_scores'"
            checked += "; max, mean, top-k mean and status of the Q = 1 select bit-identical to anoddpm_map_scores'"
        sw, se = time_legs(legs, args.reps, args.warmup)
        t_host = []
        for _ in range(max(1, args.host_reps)):
            torch.cuda.synchronize()
            t = time.perf_counter()
            h = score.cpu().numpy()
            np.partition(h, n - 1 - r1[0])[n - 1 - r1[0]]
            t_host.append((time.perf_counter() - t) * 1e3)
        tile = min(max(-(-(-(-n // 2048)) // 256) * 256, 1024), 16384)
        lines.append(f"n = {n} ({-(-n // tile)} tiles of {tile} values); {checked}")
        for j, name in enumerate(names):
            lines.append(f"  {name} wall  {fmt(sw[j])}")
            lines.append(f"  {name} event {fmt(se[j])}")
        lines.append(f"  host route       wall  {fmt(stats(t_host))}   ({len(t_host)} repetitions: copy to the host + numpy.partition, one rank)")
        by = dict(zip((nm.strip() for nm in names), se))
        ratio = [f"sort route / select Q = 1: {by['sort route']['median'] / by['select Q = 1']['median']:.2f}x"]
        if "one workgroup" in by:
            ratio.insert(0, f"one workgroup / select Q = 1: {by['one workgroup']['median'] / by['select Q = 1']['median']:.2f}x")
        lines += [f"  ratio of event medians: {', '.join(ratio)}; select Q = 4 / Q = 1: {by['select Q = 4']['median'] / by['select Q = 1']['median']:.2f}x; "
                  f"the Q = 1 select reads {5 * 4 * n / by['select Q = 1']['median'] / 1e6:.1f} GB/s (five passes over 4 n bytes)", ""]
        del legs, score, mask
    S, n = SWEEP
    g = torch.Generator(device="cpu").manual_seed(4322)
    base = torch.rand((S, n), generator=g)
    recon = (base * base * 1.7).to(dev)
    score = recon * recon                                        # fp32, rounded once: the bits anoddpm_anomaly_map thresholds
    mask = (torch.rand((S, n), generator=g) < 0.03).float().to(dev)
    lines.append(f"counts at thresholds, {S} maps of {n} values (a sweep): anoddpm_threshold_counts (a clear and ONE pass, thresholds read from "
                 f"device memory) against T launches of anoddpm_anomaly_map (one host threshold each, counts only)")
    for T in (1, 8):
        values = [0.5 / (j + 1) for j in range(T)]
        thr = torch.tensor(values, dtype=torch.float32, device=dev)
        legs = [CountsLeg(_lib, L, score, mask, thr), AnomalyLeg(_lib, L, recon, mask, thr.cpu().tolist())]
        for leg in legs:
            leg.launch()
        torch.cuda.synchronize()
        c, old = legs[0].counts.cpu().numpy(), legs[1].counts.cpu().numpy()
        assert (c[:, :, 0] == old[:, :, 3].T).all() and (c[:, :, 1] == old[:, :, 5].T).all(), "the counts of the two paths differ"
        sw, se = time_legs(legs, args.reps, args.warmup)
        lines.append(f"  T = {T}; tp and fp of both paths equal")
        for j, name in enumerate(("threshold_counts", f"{T} x anomaly_map ")):
            lines.append(f"    {name} wall  {fmt(sw[j])}")
            lines.append(f"    {name} event {fmt(se[j])}")
        lines.append(f"    ratio of event medians anomaly_map / threshold_counts: {se[1]['median'] / se[0]['median']:.2f}x")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
