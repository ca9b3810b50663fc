"""Shared by the optimiser tests (tests/test_optim_reference.py on the CPU, tests/test_gpu_optim.py on the device): the fp64
statement of one fused AdamW + EMA step and of the clip norm, the seeded cases, the per-element error metric and its bars.
numpy only; no device needed here.

One step, in the kernel's order (csrc/optim.hip, the single-tensor path of torch.optim.AdamW + UNet.update_ema_params):
    g' = g s;  p' = p (1 - lr wd);  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2
    den = sqrt(v') / sqrt(1 - b2^t) + eps;  p'' = p' - lr / (1 - b1^t) m' / den;  e' = d e + (1 - d) p''
The hyper-parameters are the Python doubles the caller hands FusedAdamWEMA: a constant derived from their fp32 roundings
(1.0f - 0.999f is 1.29e-5 off 1 - b2) is an error of the code under test, not of the reference.

Metric, u = 2^-24, a = |b1 m| + |(1 - b1) g s|, A = lr / (1 - b1^t) a / den, every element compared:
    |m' - m_ref| <= T_m u a
    |v' - v_ref| <= T_v u v_ref
    |p'' - p_ref| <= ulp(p_ref) / 2 + 2 u |p| + T_p u A                     =: tol_p
    |e' - e_ref| <= T_e u (|d e| + |(1 - d) p_ref|) + (1 - d) tol_p
The first two terms of tol_p are the final rounding of p and the two roundings of the decay (its constant, its product); what
T_p measures is the update itself, which half of the parameters (exactly 0) show undiluted by their own ulp."""
import functools
import math

import numpy as np

U = 2.0 ** -24

# The optimiser's defaults (training.FusedAdamWEMA), weight decay aside.
HYPER = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, decay=0.9999)
STEPS = (1, 2, 3, 10, 1000, 100000)
WEIGHT_DECAYS = (0.0, 0.01)

# Worst figures of fp32 torch.optim.AdamW(foreach=False) + UNet.update_ema_params on the CPU against `adamw_ema_ref` through
# `ratios`, over `case(TORCH_N, seed, step)` for every step of STEPS, both weight decays and the scales of TORCH_SCALES (gradient
# times an fp32 clip factor, rounded to fp32 as clip_grad_norm_ does), each rounded up to the next half that leaves 0.05 of room.
# Obtained by running tests/test_optim_reference.py::test_torch_fp32_stays_within_its_recorded_baseline, which prints the raw
# figures and re-checks that torch still stays within these.  Measured (torch 2.x CPU, 262 144 elements per run): m 2.494,
# v 4.417, p 4.617, e 2.253.  (v: two roundings of b2 v + (1 - b2) g'^2 and twice the rounding of g' = g s.)
TORCH_T = {"m": 3.0, "v": 4.5, "p": 5.0, "e": 2.5}
TORCH_N = 1 << 18
TORCH_SCALES = (1.0, 0.37109375, 0.0123291015625)
# The kernel's bar: its operation order and FMA contraction differ legitimately from ATen's, one or two roundings each.
KERNEL_MARGIN = 4.0
KERNEL_T = {k: KERNEL_MARGIN * t for k, t in TORCH_T.items()}


@functools.lru_cache(maxsize=1)
def _draws(n, seed):
    """The step-independent part of `case` (the largest case is drawn once for all its steps)."""
    rs = np.random.RandomState(1000 + seed)
    g = rs.standard_normal(n) * 10.0 ** rs.uniform(-6.0, 0.0, n)
    p = 0.05 * rs.standard_normal(n)
    p[rs.uniform(size=n) < 0.5] = 0.0
    hist = np.abs(g) * np.exp(0.5 * rs.standard_normal(n))
    hm = hist * rs.uniform(0.1, 1.0, n) * np.where(rs.uniform(size=n) < 0.5, -1.0, 1.0)
    hv = hist * hist * rs.uniform(0.5, 2.0, n)
    fresh = rs.uniform(size=n) < 0.25
    hm[fresh], hv[fresh] = 0.0, 0.0
    ema = p + 0.01 * rs.standard_normal(n)
    return g.astype(np.float32), p.astype(np.float32), hm, hv, ema.astype(np.float32)


def case(n, seed=0, step=1, zero_grad=False, betas=HYPER["betas"]):
    """fp32 state of n elements on entry to step `step`: dict(p, m, v, ema, g).  g = N(0,1) 10^U(-6,0); p = 0.05 N(0,1) with half
    exactly 0; ema near p.  m (random sign) and v >= 0 are what step - 1 steps leave behind a gradient history of g's magnitude
    (a log-normal factor away from it): h (1 - b1^(step-1)) U(0.1, 1) and h^2 (1 - b2^(step-1)) U(0.5, 2), so both are zero on
    entry to step 1; on entry to any step a quarter of the elements has m = v = 0 (reached by the loss for the first time), which
    shows 1 - b2 undiluted by b2 v.  zero_grad: g = m = v = 0 (a parameter the loss does not reach)."""
    g, p, hm, hv, ema = _draws(n, seed)
    m = hm * (1.0 - betas[0] ** (step - 1))
    v = hv * (1.0 - betas[1] ** (step - 1))
    if zero_grad:
        g, m, v = np.zeros(n), np.zeros(n), np.zeros(n)
    return {k: np.ascontiguousarray(x, dtype=np.float32) for k, x in dict(p=p, m=m, v=v, ema=ema, g=g).items()}


def adamw_ema_ref(p, m, v, ema, g, scale, step, lr, betas, eps, wd, decay):
    """One step in float64 from the fp32 state handed in (upcast here).  ema may be None.  Returns dict(p, m, v, ema) plus the
    magnitudes of the metric: a, A, E = |d e| + |(1 - d) p_ref|, p0 = |p|."""
    p, m, v, g = (np.asarray(x, dtype=np.float64) for x in (p, m, v, g))
    b1, b2 = float(betas[0]), float(betas[1])
    gs = g * float(scale)
    p1 = p * (1.0 - float(lr) * float(wd))
    m1 = b1 * m + (1.0 - b1) * gs
    v1 = b2 * v + (1.0 - b2) * gs * gs
    bc1 = 1.0 - b1 ** int(step)
    bc2 = 1.0 - b2 ** int(step)
    den = np.sqrt(v1) / math.sqrt(bc2) + float(eps)
    p2 = p1 - (float(lr) / bc1) * (m1 / den)
    a = np.abs(b1 * m) + np.abs((1.0 - b1) * gs)
    out = {"p": p2, "m": m1, "v": v1, "ema": None, "a": a, "A": (float(lr) / bc1) * a / den, "p0": np.abs(p), "E": None}
    if ema is not None:
        e = np.asarray(ema, dtype=np.float64)
        d = float(decay)
        out["ema"] = d * e + (1.0 - d) * p2
        out["E"] = np.abs(d * e) + np.abs((1.0 - d) * p2)
    return out


def sumsq_ref(g, max_norm):
    """(sum of squares, norm, clip factor) in float64; fp32 squares are exact in fp64 and numpy's pairwise fp64 sum is good to
    ~1e-15 relative, nine digits below the fp32 results it judges.  The factor is 1 when max_norm <= 0."""
    g = np.asarray(g, dtype=np.float64)
    ss = float(np.sum(g * g))
    norm = math.sqrt(ss)
    clip = min(float(max_norm) / (norm + 1e-6), 1.0) if max_norm > 0 else 1.0
    return ss, norm, clip


def _worst(err, unit):
    """max err / unit over the elements; an element whose unit is 0 must be exact (inf otherwise); non-finite err -> inf."""
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / unit
    degenerate = ~(unit > 0)
    if degenerate.any():
        r[degenerate] = np.where(err[degenerate] == 0, 0.0, np.inf)
    worst = float(r.max())
    return worst if np.isfinite(worst) else math.inf


def tol_p(ref, t_p):
    """[n] float64: the bar on |p - p_ref| at T_p = t_p."""
    half_ulp = 0.5 * np.spacing(np.abs(ref["p"]).astype(np.float32)).astype(np.float64)
    return half_ulp + 2.0 * U * ref["p0"] + t_p * U * ref["A"]


def ratios(got, ref, decay=None, t_p=None):
    """Worst figure per quantity, in the units of the metric: {"m", "v", "p"[, "e"]}.  got: dict of fp32 arrays (p, m, v[, ema]).
    The e figure needs the T_p that its (1 - d) tol_p term grants (t_p) and is reported when got carries an ema."""
    g64 = {k: np.asarray(x, dtype=np.float64) for k, x in got.items() if x is not None}
    out = {"m": _worst(np.abs(g64["m"] - ref["m"]), U * ref["a"]),
           "v": _worst(np.abs(g64["v"] - ref["v"]), U * ref["v"])}
    base = tol_p(ref, 0.0)
    out["p"] = _worst(np.maximum(np.abs(g64["p"] - ref["p"]) - base, 0.0), U * ref["A"])
    if not np.isfinite(g64["p"]).all():
        out["p"] = math.inf
    if "ema" in g64 and ref["ema"] is not None:
        slack = (1.0 - float(decay)) * tol_p(ref, t_p)
        out["e"] = _worst(np.maximum(np.abs(g64["ema"] - ref["ema"]) - slack, 0.0), U * ref["E"])
        if not np.isfinite(g64["ema"]).all():
            out["e"] = math.inf
    return out


def beyond(tag, got, ref, bars, decay, ledger=None):
    """Prints the worst figures of a check beside their bars and returns the lines of those beyond them (empty: the check passes).
    ledger: {quantity: worst figure so far}, updated."""
    r = ratios(got, ref, decay=decay, t_p=bars["p"])
    print(f"{tag:56s} " + "  ".join(f"T_{k} {x:9.3f} / {bars[k]:g}" for k, x in r.items()))
    if ledger is not None:
        for k, x in r.items():
            ledger[k] = max(ledger.get(k, 0.0), x)
    return [f"{tag}: T_{k} = {x:.3f} > {bars[k]:g}" for k, x in r.items() if not x <= bars[k]]


def ulps32(got, ref):
    """|got - float32(ref)| in units of the fp32 spacing at float32(ref)."""
    r32 = np.float32(ref)
    return abs(float(np.float32(got)) - float(r32)) / float(np.spacing(np.abs(r32)))
