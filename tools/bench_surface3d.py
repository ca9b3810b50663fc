"""Cost of the boundary distances of whole volumes (anoddpm_surface_distance3d of csrc/surface3d.hip) on one device, in one
process, against the only path there was before it.  For every shape the two legs are compared first and then run alternating:
  leg A  metrics.surface_distance3d with its [S, 3] results (HD, HD95, ASSD) copied to the host: wall time, and the HIP-event
         time of each of its seven launches (anoddpm_internal_surface3d_profile: events recorded between the launches of one call)
  leg B  copy the volumes to the host, then per pair two scipy.ndimage.binary_erosion, two distance_transform_edt and
         numpy.percentile; a few repetitions, it takes seconds
Per launch the bytes it must move are set against the time (an effective rate to hold against the HBM rate of the box); for the
y and x passes the mean walk length (steps a lane looks at a neighbour at distance k: the restatement of the walk in torch on the
device, checked against the library's squared distances); and the share of the call spent in scan + pack + statistics.

    python tools/bench_surface3d.py [--reps 3] [--calls 5] [--shapes a,b,c,d] [--out profiles/surface3d_ab.txt]"""
import argparse
import ctypes
import os
import platform
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAUNCHES = ("border", "z sweep", "y pass", "x pass", "scan", "pack", "stats")
FAR = 1 << 40


def host_surface(pred, ref):
    """One pair of volumes on the host, medpy's way: (hd, hd95, assd); NaN when a border is empty."""
    from scipy import ndimage
    p, r = pred > 0, ref > 0
    bp, br = p & ~ndimage.binary_erosion(p), r & ~ndimage.binary_erosion(r)
    if not bp.any() or not br.any():
        return float("nan"), float("nan"), float("nan")
    d_pr, d_rp = ndimage.distance_transform_edt(~br)[bp], ndimage.distance_transform_edt(~bp)[br]
    return max(d_pr.max(), d_rp.max()), np.percentile(np.hstack((d_pr, d_rp)), 95), (d_pr.mean() + d_rp.mean()) / 2


def make(S, D, H, W, kind, dev):
    """blob: a reference of a few blobs per volume and predictions that move and fray it; noise: half the voxels set at random,
    so that about half the voxels are border."""
    from scipy import ndimage
    rng = np.random.default_rng(977 + S + D + H)
    if kind == "noise":
        pred, ref = rng.random((S, D, H, W)) > 0.5, rng.random((S, D, H, W)) > 0.5
    else:
        sigma = (min(D, 16) / 4.0, H / 32.0, W / 32.0)
        ref = np.stack([ndimage.gaussian_filter(rng.random((D, H, W)), sigma) > 0.5 for _ in range(S)])
        pred = np.stack([np.roll(ref[s], (1, int(rng.integers(-4, 5)), int(rng.integers(-4, 5))), (0, 1, 2)) & (rng.random((D, H, W)) > 0.02)
                         for s in range(S)])
    return torch.from_numpy(pred.astype(np.float32)).to(dev), torch.from_numpy(ref.astype(np.float32)).to(dev)


def border_of(m):
    """The 6-neighbour border of bool volumes [S, D, H, W], on the device."""
    p = torch.nn.functional.pad(m, (1, 1, 1, 1, 1, 1))
    inner = p[:, :-2, 1:-1, 1:-1] & p[:, 2:, 1:-1, 1:-1] & p[:, 1:-1, :-2, 1:-1] & p[:, 1:-1, 2:, 1:-1] & p[:, 1:-1, 1:-1, :-2] & p[:, 1:-1, 1:-1, 2:]
    return m & ~inner


def sweep(zero):
    """g^2 along dim 1 of [S, D, H, W]: squared distance to the nearest True of `zero` in the own z column, FAR without one."""
    D = zero.shape[1]
    g = torch.full(zero.shape, FAR, dtype=torch.int64, device=zero.device)
    for order in (range(D), range(D - 1, -1, -1)):
        d = torch.full(zero.shape[:1] + zero.shape[2:], FAR, dtype=torch.int64, device=zero.device)
        for z in order:
            d = torch.where(zero[:, z], torch.zeros_like(d), torch.clamp(d + 1, max=FAR))
            g[:, z] = torch.minimum(g[:, z], d)
    return torch.where(g >= FAR, g, g * g)


def walk(v, axis, at=None):
    """The kernel's search along `axis` -> (result, steps): a step is one lane looking at distance k (k^2 < best, a neighbour in
    range on either side).  at: only these lanes walk (bool, v's shape)."""
    v = v.movedim(axis, -1)
    at = None if at is None else at.movedim(axis, -1)
    n = v.shape[-1]
    idx = torch.arange(n, device=v.device)
    best, steps = v.clone(), 0
    for k in range(1, n):
        active = (best > k * k) & ((idx >= k) | (idx + k < n))
        if at is not None:
            active &= at
        c = int(active.sum())
        if c == 0:
            break
        steps += c
        cand = torch.full_like(best, 4 * FAR)
        cand[..., k:] = v[..., :-k] + k * k
        cand[..., :-k] = torch.minimum(cand[..., :-k], v[..., k:] + k * k)
        best = torch.where(active, torch.minimum(best, cand), best)
    return best.movedim(-1, axis), steps


def walk_lengths(pred, ref):
    """(mean steps per voxel of the y pass over both sides' volumes, mean steps per own border voxel of the x pass, the x pass's
    squared distances at pred's border voxels for a check)."""
    bp, br = border_of(pred > 0), border_of(ref > 0)
    hp, sp = walk(sweep(bp), 2)
    hr, sr = walk(sweep(br), 2)
    d_pr, xp = walk(hr, 3, at=bp)
    _, xr = walk(hp, 3, at=br)
    return (sp + sr) / (2.0 * bp.numel()), (xp + xr) / max(1, int(bp.sum()) + int(br.sum())), d_pr[bp]


def bytes_moved(S, D, H, W, rows_hit, nb):
    """What each launch of one surface call must read + write (4-byte words unless said): fp32 inputs once (the neighbour loads
    hit cache), the z sweep reads twice and writes twice, the y pass reads and writes once, the x pass reads both sides' rows
    and writes the rows with an own border voxel, the pack reads those rows and writes the border voxels, the statistics read
    them once for the sums (each select pass reads them again: not counted)."""
    n = 2 * S * D * H * W
    return {"border": 8 * n, "z sweep": 16 * n, "y pass": 8 * n, "x pass": 8 * n + 4 * rows_hit * W, "scan": 24 * S * D * H,
            "pack": 4 * rows_hit * W + 4 * nb + 16 * S * D * H, "stats": 4 * nb}


def spread(x):
    x = np.sort(np.asarray(x))
    return f"median {np.median(x):10.3f} ms   min {x[0]:10.3f}   max {x[-1]:10.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="repetitions of the alternating legs")
    ap.add_argument("--calls", type=int, default=5, help="profiled device calls per shape")
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_surface3d.py measures on the device: no GPU visible")
    import scipy
    from anoddpm_amd import _lib, metrics
    L = _lib.lib()
    L.anoddpm_internal_surface3d_profile.argtypes = [ctypes.c_int32]
    L.anoddpm_internal_surface3d_times.argtypes = [ctypes.POINTER(ctypes.c_float)]
    dev = torch.device("cuda:0")
    lines = [f"boundary distances of whole volumes, csrc/surface3d.hip (ABI {_lib.ABI_VERSION}): {args.reps} alternating repetitions of the two legs, "
             f"{args.calls} profiled calls per shape, every shape warmed first",
             f"box: {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs visible; "
             f"torch {torch.__version__}; numpy {np.__version__}; scipy {scipy.__version__}",
             "leg A: metrics.surface_distance3d + copy of [S, 3] results; leg B: D2H copy + per pair two scipy.ndimage.binary_erosion, two "
             "distance_transform_edt and numpy.percentile", ""]
    shapes = {"a": ("(a) 1 x 4 x 256^2, blobs", 1, 4, 256, 256, "blob"), "b": ("(b) 1 x 64 x 256^2, blobs", 1, 64, 256, 256, "blob"),
              "c": ("(c) 4 x 155 x 240 x 240, blobs", 4, 155, 240, 240, "blob"), "d": ("(d) 1 x 64 x 256^2, noise: half the voxels are border", 1, 64, 256, 256, "noise")}
    for key in args.shapes.split(","):
        label, S, D, H, W, kind = shapes[key]
        pred, ref = make(S, D, H, W, kind, dev)

        def native_leg():
            o = metrics.surface_distance3d(pred, ref)
            return torch.stack([o["hd"], o["hd95"], o["assd"]], dim=-1).cpu().numpy(), o

        def host_leg():
            pk, rk = pred.cpu().numpy(), ref.cpu().numpy()
            return np.array([host_surface(pk[s], rk[s]) for s in range(S)])

        for _ in range(2):                                               # warm the shape: allocator, code object, caches
            d, o = native_leg()
        h = host_leg()
        counts = o["counts"].cpu().numpy().reshape(-1, 2)
        assert np.array_equal(np.isnan(h), np.isnan(d)) and np.array_equal(h[:, 0], d[:, 0]), (label, h, d)          # HD: the same bits
        worst = float(np.nanmax(np.abs(h - d) / np.maximum(np.abs(h), 1.0)))
        assert worst <= 1e-12, (label, worst)                            # HD95: numpy's lerp; ASSD: another order of the same sum
        tn, th = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            native_leg()
            tn.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_leg()
            th.append((time.perf_counter() - t0) * 1e3)
        assert L.anoddpm_internal_surface3d_profile(1) == 0
        per = []
        ms = (ctypes.c_float * 8)()
        for _ in range(args.calls):
            metrics.surface_distance3d(pred, ref)
            assert L.anoddpm_internal_surface3d_times(ms) == len(LAUNCHES)
            per.append([ms[i] for i in range(len(LAUNCHES))])
        assert L.anoddpm_internal_surface3d_profile(0) == 0
        per = np.median(np.array(per), axis=0)
        total = float(per.sum())
        bp, br = border_of(pred > 0), border_of(ref > 0)
        rows_hit = int(bp.any(dim=-1).sum()) + int(br.any(dim=-1).sum())
        nb = int(counts.sum())
        moved = bytes_moved(S, D, H, W, rows_hit, nb)
        wy, wx, d_pr = walk_lengths(pred, ref)
        sq = metrics.distance_transform3d((~br).float(), squared=True)   # the library's squared distances to ref's border
        assert torch.equal(sq[bp].long(), d_pr), label
        lines += [f"{label}: {S * D * H * W} voxels a side, borders of {int(counts[:, 0].sum())} / {int(counts[:, 1].sum())} voxels "
                  f"(prediction / reference), {rows_hit} of {2 * S * D * H} rows hold an own border voxel",
                  f"  pair 0: HD {d[0, 0]:.4f}  HD95 {d[0, 1]:.4f}  ASSD {d[0, 2]:.4f}; HD bit-equal in both legs, largest relative |B - A| = {worst:.3g}",
                  f"  leg A wall time  {spread(tn)}",
                  f"  leg B wall time  {spread(th)}",
                  f"  ratio of medians B / A: {np.median(th) / np.median(tn):.0f}x",
                  f"  HIP-event time per launch (median of {args.calls} calls; sum {total:.3f} ms):"]
        for name, t in zip(LAUNCHES, per):
            lines.append(f"    {name:8s} {t:9.4f} ms  {100 * t / total:5.1f} %   {moved[name] / 1e6:10.2f} MB to move -> {moved[name] / 1e6 / max(t, 1e-6):8.1f} GB/s")
        lines += [f"  mean walk length: y pass {wy:.2f} steps per voxel, x pass {wx:.2f} steps per own border voxel",
                  f"  scan + pack + statistics: {100 * float(per[4:].sum()) / total:.1f} % of the device time of the call", ""]
        del pred, ref, bp, br, d_pr, sq
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
