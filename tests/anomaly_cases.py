"""Shared by the anomaly-map element tests (tests/test_anomaly_reference.py on the CPU, tests/test_gpu_anomaly_elements.py on the
device): the seeded cases of anoddpm_anomaly_map (csrc/metrics.hip), its two statements and the per-element error model.  No
device needed here.

`restate(case)` is the kernel's own statement in numpy fp32, one rounding per operation (oracle.metrics_oracle.anomaly_maps over
the strided view the C ABI describes): the fp32 running sum of the chains in chain order, one division by navg, d = mean - real,
se = d d, img = 2 se - 1, thr = img > 0 ? 1 : -1, pred = se > threshold, and the twelve counts in fp64.  The device must give its
bits.  `reference(case)` is the same operation in fp64 of the fp32 inputs (mean = sum / navg, counts from the fp64 pred).

Error model, derived and not measured, u = 2^-24 (each line is the first-order rounding of one fp32 operation on top of the
propagated error of its operands):
    mean     E_m = navg u mean_k|recon_k|   (navg - 1 additions of at most u sum_k|recon_k| each, one division; 0 for navg 1)
    d        E_d = E_m + u (|m64| + |real|)
    sqerr    E_s = 2 |d64| E_d + E_d^2 + u se64
    mse_img  E_i = 2 E_s + u (2 se64 + 1)
Measured on the CPU (test_anomaly_reference.py prints them; `restate` against `reference` over every case below):
    worst |mean32 - mean64| / E_m = 0.759    worst |se32 - se64| / E_s = 0.925    worst |img32 - img64| / E_i = 0.559
so the forms hold with no constant added.  A `lattice` case (every operand a multiple of 2^-8, of 2^-4 with navg 16, in [-1, 1])
has every fp32 operation exact: its bound is 0, the reference is met with equality and no element is excluded.

Ambiguous elements: |se64 - threshold| <= E_s (pred, counts 0 and 2..8) or |2 se64 - 1| <= E_i (thr_img): the side of the
threshold is not decidable in fp32 there, and they are compared with `restate` only.  The builder caps their share at 1 % of a
case's elements (AMBIGUOUS_CAP); lattice cases have none by definition.  Share per family over the cases below:
    uniform 0 of 269 295    quiet 0 of 2 130    masks 0 of 3 028    nonfinite 0 of 3 771    ties 4 of 1 000    lattice 0 of 141 136
The four of `ties` are put there.  se = 0.5 (mse_img exactly 0, so thr_img -1) cannot be reached: 0.5 is not the square of a
dyadic rational, so it is not on the lattice, and no fp32 d has a rounded square of 0.5 either (`_half_root`).  `ties` holds the
two fp32 values of d nearest to it, one either side, in both signs; the lattice carries the ties at 0.25 and at 0 (`>` is strict:
pred 0) with one step either side.

Non-finite inputs: where the fp64 reference is NaN the output must be NaN, where it is infinite it must be that infinity; a NaN
compares false, so pred is 0 and thr_img -1 there; sum(sqerr) and max(real) keep a NaN like torch.sum and torch.max."""
import functools

import numpy as np

from oracle import metrics_oracle as mo

U = 2.0 ** -24
AMBIGUOUS_CAP = 0.01
BLOCKS = 64                                   # ANODDPM_ANOMALY_BLOCKS
NC = mo.NCOUNTS
MAPS = ("mean", "sqerr", "mse_img", "thr_img", "pred")
SENTINEL = np.float32(-77.0)                  # what the tests pre-fill outputs with; no map or count of any case takes this value
NS = (1, 63, 65, 255, 257, 1000, 16384, 16385, 32845)
NAVGS = (1, 2, 3, 5, 7, 16, 17, 18, 33)
MASK_VALUES = np.array([0.0, 1.0, 0.5, 2.0, -1.0, -0.0], dtype=np.float32)


def _half_root():
    """(d_below, d_above): the two fp32 neighbours of sqrt(0.5).  Their fp32 squares straddle 0.5 and neither is 0.5: d d steps by
    1.4 * 2^-24 there while only a window of 1.5 * 2^-25 rounds to 0.5, and no fp32 d falls into it."""
    lo = np.float32(np.sqrt(0.5))
    if np.float32(lo * lo) > np.float32(0.5):
        lo = np.nextafter(lo, np.float32(0))
    hi = np.nextafter(lo, np.float32(2))
    assert np.float32(lo * lo) < np.float32(0.5) < np.float32(hi * hi)
    return lo, hi


HALF_D = _half_root()


def _uniform(rs, B, n, navg):
    real = rs.uniform(-1.0, 1.0, (B, n))
    recon = np.clip(real[None] + 0.6 * rs.standard_normal((navg, B, n)), -1.0, 1.0)
    return real.astype(np.float32), recon.astype(np.float32)


def make_case(name, family, B, n, navg, threshold=0.5, mask="binary", seed=0):
    """One case: fp32 real [B][n], recon [navg][B][n] (the logical view; `layout` puts it into a flat buffer), mask [B][n] or None."""
    rs = np.random.RandomState(seed)
    real, recon = _uniform(rs, B, n, navg)
    exact = False
    if family == "quiet":
        assert B >= 2
        real[0] *= np.float32(2.0 ** -10)
        recon[:, 0] *= np.float32(2.0 ** -10)
        real[1] = -np.abs(real[1]) - np.float32(2.0 ** -6)             # all negative: max(real) starts from -inf
        recon[:, 1] = np.clip(real[1][None] + (0.6 * rs.standard_normal((navg, n))).astype(np.float32), -1, 1)
    elif family == "lattice":
        assert navg in (1, 2, 16)
        q = 16.0 if navg == 16 else 256.0
        real = (np.round(real * q) / q).astype(np.float32)
        recon = (np.round(recon * q) / q).astype(np.float32)
        step = np.float32(1.0 / q)
        # se exactly on a threshold with one step either side: d = 0.5 (se 0.25) and d = 0 (se 0), both signs of d
        ties = [(0.0, 0.5), (0.0, 0.5 + step), (0.0, 0.5 - step), (0.25, -0.25), (0.25, -0.25 - step), (0.25, -0.25 + step),
                (0.5, 0.5), (0.5, 0.5 + step), (-0.5, -0.5 - step), (-1.0, -1.0), (1.0, 1.0)]
        for j, (r, c) in enumerate(ties):
            if j < n:
                real[:, j] = r
                recon[:, :, j] = c
        exact = True
    elif family == "nonfinite":
        assert B == 3 and navg >= 2 and n >= 8
        recon[1, 1, n // 3] = np.nan
        recon[0, 1, n // 2] = np.inf
        real[2, n - 2] = np.nan
    elif family == "ties":
        assert navg == 1 and n >= 4
        real[:, :4] = 0.0
        for j, d in enumerate(HALF_D + HALF_D):
            recon[0, :, j] = d if j < 2 else -d
    else:
        assert family in ("uniform", "masks")
    if mask == "binary":
        m = (rs.uniform(0, 1, (B, n)) > 0.8).astype(np.float32)
    elif mask == "values":
        m = MASK_VALUES[rs.randint(0, MASK_VALUES.size, (B, n))]
        m[:, : min(n, MASK_VALUES.size)] = MASK_VALUES[: min(n, MASK_VALUES.size)]
    else:
        assert mask is None
        m = None
    return {"name": name, "family": family, "B": B, "n": n, "navg": navg, "threshold": float(threshold), "real": real,
            "recon": recon, "mask": m, "exact": exact}


def layout(case, padded=False):
    """The flat recon buffer of the C ABI: dense (recon_as = B n, recon_bs = n, what the wrapper hands in) or padded
    (recon_as = B n + 5, recon_bs = n + 3, seven more floats behind the last slice), every pad element NaN: a read of one shows.
    With B = 3 those two strides would lay the last image of a chain over the first float of the next chain (2 (n + 3) + n is
    B n + 6), so recon_as is B n + 8 there: two pad floats between the chains, as B = 2 has."""
    B, n, navg = case["B"], case["n"], case["navg"]
    if padded:
        rbs, extra = n + 3, 7
        ras = max(B * n + 5, (B - 1) * rbs + n + 2)
    else:
        ras, rbs, extra = B * n, n, 0
    buf = np.full((navg - 1) * ras + (B - 1) * rbs + n + extra, np.nan, dtype=np.float32)
    for k in range(navg):
        for b in range(B):
            o = k * ras + b * rbs
            buf[o:o + n] = case["recon"][k, b]
    return {"buf": buf, "recon_as": ras, "recon_bs": rbs}


def restate(case, padded=False):
    """(maps, counts [B][12] fp64): the kernel's own statement in numpy fp32 over the strided view of `layout`."""
    lay = layout(case, padded)
    rec = mo.strided_recon(lay["buf"], case["navg"], case["B"], case["n"], lay["recon_as"], lay["recon_bs"])
    with np.errstate(invalid="ignore", over="ignore"):
        return mo.anomaly_maps(case["real"], rec, case["mask"], threshold=np.float32(case["threshold"]))


def counts_of(pred, mask, se, real):
    """The twelve counts (include/anoddpm_hip.h) of a pred / mask / sqerr / real, each [B][n], in fp64."""
    B = pred.shape[0]
    mk = np.zeros(pred.shape) if mask is None else mask.astype(np.float64)
    p = pred.astype(np.float64)
    c = np.zeros((B, NC))
    with np.errstate(invalid="ignore"):
        c[:, 0], c[:, 1], c[:, 2] = p.sum(axis=1), mk.sum(axis=1), (p * mk).sum(axis=1)
        c[:, 3] = ((mk == 1) & (p == 1)).sum(axis=1)
        c[:, 4] = ((mk == 1) & (p == 0)).sum(axis=1)
        c[:, 5] = ((mk == 0) & (p == 1)).sum(axis=1)
        c[:, 6] = ((mk == 0) & (p == 0)).sum(axis=1)
        c[:, 7] = ((mk != 0) & (p != 0)).sum(axis=1)
        c[:, 8] = ((mk != 0) | (p != 0)).sum(axis=1)
        c[:, 9] = se.astype(np.float64).sum(axis=1)
        c[:, 10] = real.astype(np.float64).max(axis=1)                  # ndarray.max keeps a NaN, like torch.max
    return c


def reference(case):
    """fp64 of the fp32 inputs: the five maps, `counts` (from the fp64 pred), the bounds E_m, E_s, E_i [B][n] (0 for an exact case)
    and the ambiguous sets amb_pred, amb_thr."""
    f = np.float64
    real, recon, navg = case["real"].astype(f), case["recon"].astype(f), case["navg"]
    thr = f(np.float32(case["threshold"]))
    with np.errstate(invalid="ignore", over="ignore"):
        mean = recon.sum(axis=0) / navg
        d = mean - real
        se = d * d
        img = se * 2.0 - 1.0
        thr_img = np.where(img > 0, 1.0, -1.0)
        pred = (se > thr).astype(f)
        e_m = navg * U * np.abs(recon).mean(axis=0) if navg > 1 else np.zeros_like(mean)
        e_d = e_m + U * (np.abs(mean) + np.abs(real))
        e_s = 2.0 * np.abs(d) * e_d + e_d * e_d + U * se
        e_i = 2.0 * e_s + U * (2.0 * se + 1.0)
        if case["exact"]:
            e_m, e_s, e_i = np.zeros_like(e_m), np.zeros_like(e_s), np.zeros_like(e_i)
            amb_pred = amb_thr = np.zeros(se.shape, dtype=bool)
        else:
            amb_pred = np.isfinite(se) & (np.abs(se - thr) <= e_s)
            amb_thr = np.isfinite(se) & (np.abs(img) <= e_i)
    return {"mean": mean, "sqerr": se, "mse_img": img, "thr_img": thr_img, "pred": pred,
            "counts": counts_of(pred, case["mask"], se, case["real"]), "E_mean": e_m, "E_sqerr": e_s, "E_mse_img": e_i,
            "amb_pred": amb_pred, "amb_thr": amb_thr}


def ambiguous_share(ref):
    return float((ref["amb_pred"] | ref["amb_thr"]).sum()) / ref["pred"].size


def same_bits(a, b):
    """Element-wise: equal as uint32, all NaNs counting as equal."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _same64(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


def check(tag, case, maps, counts, ledger=None, show=True):
    """Failure lines (empty: passes) of the maps handed in (fp32 [B][n], any subset of MAPS) and the counts [B][12]:
    every map bit for bit `restate`; within the bound of `reference` (equal where that is not finite; thr_img and pred equal
    outside the ambiguous set); counts 0..8 and 10 exactly restate's and, with the ambiguous elements taken from restate, exactly
    the reference's; count 9 within 1e-12 relative of restate's and within sum(E_s) of the reference's.  Prints and records the
    worst err / bound per map."""
    rst, rc = restate_of(case)
    ref = reference_of(case)
    B, n = case["B"], case["n"]
    lines, shown = [], []
    for k in MAPS:
        if k not in maps:
            continue
        got = np.asarray(maps[k]).reshape(B, n)
        if got.dtype != np.float32:
            lines.append(f"{tag}: {k} is {got.dtype}")
            continue
        ok = same_bits(got, rst[k])
        if not ok.all():
            b, i = np.argwhere(~ok)[0]
            lines.append(f"{tag}: {k}[{b}][{i}] got {got[b, i]!r} restate {rst[k][b, i]!r} ({int((~ok).sum())} elements differ in bits)")
        want = ref[k]
        g64 = got.astype(np.float64)
        fin = np.isfinite(want)
        if not _same64(g64[~fin], want[~fin]).all():
            lines.append(f"{tag}: {k} differs from the reference where that is NaN or infinite")
        if k in ("thr_img", "pred"):
            clear = fin & ~ref["amb_thr" if k == "thr_img" else "amb_pred"]
            if not (g64[clear] == want[clear]).all():
                b, i = np.argwhere(clear & (g64 != want))[0]
                lines.append(f"{tag}: {k}[{b}][{i}] got {got[b, i]} reference {want[b, i]} at an unambiguous element")
            continue
        allow = ref["E_" + k]
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(fin, np.abs(g64 - want), 0.0)
            ratio = np.where(fin, np.where(allow > 0, err / allow, np.where(err == 0, 0.0, np.inf)), 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        worst = float(ratio.max()) if ratio.size else 0.0
        shown.append(f"{k} {worst:.3f}")
        if ledger is not None:
            ledger[k] = max(ledger.get(k, 0.0), worst)
        if worst > 1.0:
            b, i = np.unravel_index(np.argmax(ratio), ratio.shape)
            lines.append(f"{tag}: {k}[{b}][{i}] got {got[b, i]:.9g} reference {want[b, i]:.17g} err / bound {ratio[b, i]:.3f} "
                         f"({int((ratio > 1).sum())} elements)")
    if counts is not None:
        c = np.asarray(counts, dtype=np.float64).reshape(B, NC)
        exact_cols = list(range(9)) + [10]
        if not _same64(c[:, exact_cols], rc[:, exact_cols]).all():
            lines.append(f"{tag}: counts 0..8, 10 got {c[:, exact_cols].tolist()} restate {rc[:, exact_cols].tolist()}")
        with np.errstate(invalid="ignore"):
            near = _same64(c[:, 9], rc[:, 9]) | (np.abs(c[:, 9] - rc[:, 9]) <= 1e-12 * np.abs(rc[:, 9]))
        if not near.all():
            lines.append(f"{tag}: count 9 got {c[:, 9].tolist()} restate {rc[:, 9].tolist()}")
        # against fp64: the ambiguous elements' pred is restate's, every other is the reference's own
        pred = np.where(ref["amb_pred"], rst["pred"].astype(np.float64), ref["pred"])
        fc = counts_of(pred, case["mask"], ref["sqerr"], case["real"])
        if not _same64(c[:, exact_cols], fc[:, exact_cols]).all():
            lines.append(f"{tag}: counts 0..8, 10 got {c[:, exact_cols].tolist()} reference {fc[:, exact_cols].tolist()}")
        with np.errstate(invalid="ignore"):
            budget = np.where(np.isfinite(ref["sqerr"]), ref["E_sqerr"], 0.0).sum(axis=1) + 1e-12 * np.abs(fc[:, 9])
            near = _same64(c[:, 9], fc[:, 9]) | (np.abs(c[:, 9] - fc[:, 9]) <= budget)
        if not near.all():
            lines.append(f"{tag}: count 9 got {c[:, 9].tolist()} reference {fc[:, 9].tolist()} allowance {budget.tolist()}")
    if show:
        print(f"{tag:44s} " + "  ".join(shown))
    return lines


def _matrix():
    out = []
    for i, navg in enumerate(NAVGS):                                     # every navg with two sizes, every size twice
        for j, n in enumerate((NS[i], NS[(i + 4) % len(NS)])):
            B = 1 + (i + 2 * j) % 3
            out.append(make_case(f"uniform-navg{navg}-n{n}-B{B}", "uniform", B, n, navg, seed=300 + 2 * i + j))
    out.append(make_case("uniform-navg5-c3x7x5-B2", "uniform", 2, 3 * 7 * 5, 5, seed=330))
    out.append(make_case("quiet-navg5-n1000", "quiet", 2, 1000, 5, seed=340))
    out.append(make_case("quiet-navg1-n65", "quiet", 2, 65, 1, seed=341))
    sizes = (257, 1000, 16385)
    for i, navg in enumerate((1, 2, 16)):
        for j, thr in enumerate((0.5, 0.25, 0.0, -1.0)):
            out.append(make_case(f"lattice-navg{navg}-thr{thr:g}", "lattice", 2, sizes[(i + j) % 3], navg, threshold=thr,
                                 mask="binary" if j % 2 == 0 else "values", seed=350 + 4 * i + j))
    out.append(make_case("masks-values-navg3-n1000", "masks", 2, 1000, 3, mask="values", seed=370))
    out.append(make_case("masks-values-navg1-n257", "masks", 3, 257, 1, mask="values", seed=371))
    out.append(make_case("masks-none-navg2-n257", "masks", 1, 257, 2, mask=None, seed=372))
    out.append(make_case("nonfinite-navg3-n1000", "nonfinite", 3, 1000, 3, seed=380))
    out.append(make_case("nonfinite-navg17-n257", "nonfinite", 3, 257, 17, mask="values", seed=381))
    out.append(make_case("ties-half-n1000", "ties", 1, 1000, 1, seed=390))
    return out


@functools.lru_cache(maxsize=1)
def cases():
    out = _matrix()
    for c in out:
        ref = reference_of(c)
        share = ambiguous_share(ref)
        assert share <= AMBIGUOUS_CAP, (c["name"], share)
        assert not c["exact"] or share == 0.0
        for k in ("real", "recon", "mask"):
            if c[k] is not None:
                c[k].setflags(write=False)
    return out


_REFS, _RSTS = {}, {}


def reference_of(case):
    """`reference` of a case, computed once and not to be written to."""
    if case["name"] not in _REFS:
        _REFS[case["name"]] = reference(case)
    return _REFS[case["name"]]


def restate_of(case):
    """`restate` of a case over the dense layout, computed once and not to be written to."""
    if case["name"] not in _RSTS:
        _RSTS[case["name"]] = restate(case)
    return _RSTS[case["name"]]


def case_names():
    return [c["name"] for c in cases()]


def get(name):
    return next(c for c in cases() if c["name"] == name)


# ------------------------------------------------------------------ the ratios: evaluation.py:26-76 in fp64 torch
def edge_cases():
    """name -> (real_mask, pred) fp32 [B,1,8,8] {0,1} maps: the edges of the ratios."""
    rs = np.random.RandomState(400)
    rnd = lambda B: (rs.uniform(0, 1, (B, 1, 8, 8)) > 0.6).astype(np.float32)
    zero, one = np.zeros((1, 1, 8, 8), np.float32), np.ones((1, 1, 8, 8), np.float32)
    three_m, three_p = rnd(3), rnd(3)
    three_m[1], three_p[1] = 0.0, 0.0                                    # one empty image of three: dice is a mean of ratios
    return {"empty-mask": (zero, rnd(1)), "empty-both": (zero, zero), "full-mask": (one, rnd(1)), "full-both": (one, one),
            "empty-pred": (rnd(1), zero), "plain": (rnd(2), rnd(2)), "three-one-empty": (three_m, three_p)}


def ratio_formulas(real_mask, pred, smooth=0.000001):
    """The reference's tensor expressions (evaluation.py:34-36, 50-76) on fp64 torch tensors."""
    import torch
    m, p = torch.from_numpy(real_mask).double(), torch.from_numpy(pred).double()
    inter = torch.sum(p * m, dim=[1, 2, 3])
    union = torch.sum(p, dim=[1, 2, 3]) + torch.sum(m, dim=[1, 2, 3])
    tp, fp = ((m == 1) & (p == 1)).sum().double(), ((m == 1) & (p == 0)).sum().double()
    fn, tn = ((m == 0) & (p == 1)).sum().double(), ((m == 0) & (p == 0)).sum().double()
    land, lor = torch.logical_and(m, p).sum().double(), torch.logical_or(m, p).sum().double()
    return {"dice": float(torch.mean((2.0 * inter + smooth) / (union + smooth), dim=0)), "precision": float(tp / (tp + fp + 1e-6)),
            "recall": float(tp / (tp + fn + 1e-6)), "FPR": float(fp / (fp + tn + 1e-6)), "IoU": float(land / (lor + 1e-8))}


def psnr_formula(recon, real):
    """evaluation.py:40-44 on fp64 torch tensors of the fp32 inputs."""
    import torch
    recon, real = torch.from_numpy(recon).double(), torch.from_numpy(real).double()
    se = (real - recon).square()
    mse = torch.mean(se, dim=list(range(real.dim())))
    return float(20 * torch.log10(torch.max(real) / torch.sqrt(mse)))


def psnr_cases():
    """name -> (recon, real) fp32 [B,1,8,8]: a plain pair, an all-negative image (log10 of a negative: NaN) and one whose maximum
    is exactly 0 (log10(0): -inf)."""
    rs = np.random.RandomState(401)
    real = rs.uniform(-1, 1, (2, 1, 8, 8)).astype(np.float32)
    recon = np.clip(real + 0.3 * rs.standard_normal(real.shape), -1, 1).astype(np.float32)
    neg = -np.abs(real) - np.float32(0.125)
    zero_max = neg.copy()
    zero_max[1, 0, 3, 3] = 0.0
    return {"plain": (recon, real), "all-negative": (recon, neg), "zero-max": (recon, zero_max)}


def same_or_close(got, want, rel):
    """NaN and infinities must agree exactly, finite values within rel."""
    got, want = float(got), float(want)
    if np.isnan(want) or np.isinf(want):
        return (np.isnan(got) and np.isnan(want)) or got == want
    return abs(got - want) <= rel * abs(want)
