"""Shared by the loss element tests (tests/test_loss_reference.py on the CPU, tests/test_gpu_loss_elements.py on the device): the
seeded cases, the fp64 statement of calc_loss / p_loss / calc_vlb_xt (GaussianDiffusion.py:384-434) with its gradient with respect
to the model output, and the per-element error model.  No device needed here.

What the kernels (csrc/diffusion.hip: loss_fwd_kernel, loss_fold_kernel, loss_bwd_kernel, vlb_element, vlb_kernel) see is taken
as it is: the fp32 inputs x0, x_t, eps, noise, weights, g_*; the six fp32-rounded coefficient tables; the branch selectors
x0 < float32(-0.999), x0 > float32(0.999), t == 0 decided on those fp32 / integer inputs.  Everything after that is float64 here.
One deliberate exception: whether raw = recip x_t - recipm1 eps lies in [-1, 1] (torch.clamp passes the gradient there) is decided
on the fp64 raw, and the builder keeps |raw64| - 1 away from 0 by max(1e-4, 8 u (|recip x_t| + |recipm1 eps|)), u = 2^-24: the
second term is the rounding of the fp32 raw itself (at t = T - 1 of the cosine schedule recip is 2e4 and that term is 2e-2), so
that fp32 and fp64 agree on the side.  Only the `clamp_edge` case puts elements on purpose beyond the edge (by more than 5e-2).

d_eps[b][i] = c_b dmain / n + v_b dterm / (n ln 2),   c_b = g_per[b] + g_total w_b / B,   v_b = c_b + g_vlb[b]   (hybrid)

Error model (`bound`), per element, never normalised over a batch:
  main term and KL rows      |got - ref| <= K_KL u M.   M is the same closed form in fp64 with every addition and subtraction
                             replaced by the sum of the absolute values of its operands (the running forward-error magnitude):
                             |c_b| becomes |g_per| + |g_total w / B|, eps - noise becomes |eps| + |noise|, and
                             (c1 x0 + c2 x_t) - (c1 pred + c2 x_t) becomes |c1 x0| + 2 |c2 x_t| + |c1| (|recip x_t| + |recipm1 eps|).
  decoder NLL (t = 0)        K_NLL u (inv_std + |d64|) / delta64 * (|c_b| + |g_vlb|)-magnitude * coef1 recipm1 / (n ln 2), plus the
                             main-term part.  d64 = d(-log p)/d(mean), delta64 = what the selected logarithm is taken of
                             (cdf_plus, 1 - cdf_min or cdf_plus - cdf_min).  The chain factor uses the magnitude of v_b
                             (|g_per| + |g_total w / B| + |g_vlb|) where the issue's form has |v_b|: v_b is itself formed in fp32.
  ill-conditioned elements   t = 0, inside the clamp, delta64 < DELTA_MIN = 1e-3: not bounded.  fp32 cdf values differ from fp64 by
                             several 1e-8 there and the gradient divides by their difference; at the 1e-12 floor the reference's
                             own fp32 gradient is 0 where fp64's is not.  Such an element must be finite and
                             |g| <= |main part| + K_KL u M + magnitude(v_b) coef1 recipm1 inv_std C_SAT / (n ln 2).
  outside the clamp          the VLB gradient is 0: d_eps is the main-term part under its own bound, at every t.

Measured on the CPU (tests/test_loss_reference.py prints them; numpy fp32 restatement oracle.diffusion_oracle.loss_grad_analytic
against `reference`, over every case of `cases()`), and the constants fixed from them at twice the figure rounded up to one digit
(the factor 2 is for the few-ulp differences between the device's tanhf / expf / logf and numpy's, nothing else):
    K_KL   measured 2.869    -> 6
    K_NLL  measured 114.526  -> 300   (linear schedule alone: 66; its inv_std at t = 0 is the smaller one.  The worst elements are
                                       well-conditioned ones, delta64 = 0.6, near the zero of the gradient: what they show is the
                                       rounding of cen = x0 - mean under the second derivative, of the order inv_std^2)
    C_SAT  measured 8.232    -> 20    (max |vlb part of d32| / (chain inv_std) over the unbounded elements)
Share of the t = 0 elements that are inside the clamp with delta64 < DELTA_MIN, per eps family (the builder asserts <= 10 % per case, and the
KL rows have none by construction):
    trained 0 of 273 883 = 0 %    tiny 0 of 1 022 = 0 %    offset 0 of 724 = 0 %    untrained 982 of 17 373 = 5.65 % (worst case 10.0 %,
    n = 105; the upstream fixture loss_kat.npz, untrained too: 7.4 %)
Worst difference of the fp32 torch oracle (the expressions of loss_terms) from `reference` on the per-sample vlb and loss, per
eps family, rows without an element of delta64 < DELTA_MIN, relative to the value's magnitude companion (the value with |.| summed
as above: a KL row at large t is 0.5 (-1 + lv2 - lv1 + exp(lv1 - lv2)) + ... = 1e-6 out of terms of size 10, and relative to the
value itself the fp32 oracle is off by 25 % there); the device's bar is 4x that with a floor of 2e-6 (VALUE_BAR), the floor because
the kernels sum in fp64 and so must do at least as well as an oracle that sums in fp32:
    trained 8.95e-8    untrained 1.24e-7    tiny 9.06e-8    offset 1.43e-7      -> every bar is the floor, 2e-6
Rows that hold an element of delta64 < DELTA_MIN (t = 0, "untrained" family) are compared on the value against the fp32 oracle, not fp64: the
1e-12 floor and the granularity of an fp32 cdf difference near 0 are the reference's behaviour and fp64 does not reproduce them.
Their bar adds, per such element, log((delta64 (1 + SAT_R) + SAT_E) / max(delta64 (1 - SAT_R) - SAT_E, 1e-12)) / (n ln 2):
any fp32 evaluation of delta lies in that interval (SAT_E = 8 u: two cdf values of a few u each; SAT_R = 1e-3: the argument's
rounding, inv_std u |cen| ~ 2e-5, times the tail's logarithmic slope 2 c (1 + 3 k z^2) < 50), so two of them differ by no more."""
import functools
import math

import numpy as np

from oracle import diffusion_oracle as do

U = 2.0 ** -24
LN2 = math.log(2.0)
T = 1000
DELTA_MIN = 1e-3
FLOOR = 1e-12
SAT_E = 8.0 * U
SAT_R = 1e-3
UNBOUNDED_CAP = 0.10

K_KL = 6.0
K_NLL = 300.0
C_SAT = 20.0
VALUE_FLOOR = 2e-6
MEASURED_VALUE = {"trained": 9.0e-8, "untrained": 1.25e-7, "tiny": 9.1e-8, "offset": 1.44e-7}
VALUE_BAR = {k: max(4.0 * v, VALUE_FLOOR) for k, v in MEASURED_VALUE.items()}

KINDS = {"l1": 0, "l2": 1, "hybrid": 2}
FAMILIES = ("trained", "untrained", "tiny", "offset")
GCFGS = ("total", "per", "per+total", "vlb+per+total", "vlb")
CLASSES = ("main", "kl", "nll_lo", "nll_hi", "nll_mid")
T_ROWS = (0, 0, 1, 2, 50, 500, T - 2, T - 1, -1)                  # the last row is the twin of the row before it
T_BAD = (T, -T - 1)
TABLE_KEYS = {"c_recip": "sqrt_recip_alphas_cumprod", "c_recipm1": "sqrt_recipm1_alphas_cumprod",
              "c_coef1": "posterior_mean_coef1", "c_coef2": "posterior_mean_coef2",
              "c_post_logvar": "posterior_log_variance_clipped", "c_model_logvar": "model_log_variance"}


@functools.lru_cache(maxsize=None)
def schedule(name):
    """(fp64 tables of the oracle, the six fp32 tables the kernels are handed)."""
    tb = do.tables(do.beta_schedule(T, name))
    return tb, {k: np.ascontiguousarray(tb[v], dtype=np.float32) for k, v in TABLE_KEYS.items()}


def effective_t(t):
    """(table index, out of range) as the kernels form them: a negative t wraps once, what is still outside reads index 0."""
    t = np.asarray(t, dtype=np.int64)
    te = np.where(t < 0, t + T, t)
    bad = (te < 0) | (te >= T)
    return np.where(bad, 0, te), bad


def _rows(case, names=("c_recip", "c_recipm1", "c_coef1", "c_coef2", "c_post_logvar", "c_model_logvar")):
    te, _ = effective_t(case["t"])
    return [case["tables"][k][te].astype(np.float64)[:, None] for k in names]


def clamp_margin(case):
    """[B][n]: (| |raw64| - 1 |, the margin the builder keeps) of a hybrid case."""
    recip, recipm1 = _rows(case, ("c_recip", "c_recipm1"))
    xt, eps = case["xt"].astype(np.float64), case["eps"].astype(np.float64)
    raw = recip * xt - recipm1 * eps
    return np.abs(np.abs(raw) - 1.0), np.maximum(1e-4, 8.0 * U * (np.abs(recip * xt) + np.abs(recipm1 * eps)))


def _x0(rs, family, B, n):
    if family == "uniform":
        return np.round(rs.uniform(-1.0, 1.0, (B, n)), 1)
    if family in ("plus", "minus"):
        return np.full((B, n), 1.0 if family == "plus" else -1.0)
    assert family == "edges"
    e = np.float32(0.999)
    six = [e, np.nextafter(e, np.float32(1)), np.nextafter(e, np.float32(0))]
    six = np.array(six + [-v for v in six], dtype=np.float32)
    return np.tile(six, (B, -(-n // 6)))[:, :n].astype(np.float64)


def make_case(name, kind, sched="linear", family="trained", n=256, t=T_ROWS, weights=False, gcfg="total", x0_family="uniform",
              clamp_edge=False, clamp_boundary=False, zero_block=False, seed=0):
    """One case: a dict of fp32 [B][n] x0, xt, eps, noise, int64 t, fp32 weights / g_per / g_vlb [B] or None, g_total [1] or None,
    the fp32 tables, and its labels.  x_t = q_sample(x0, t, noise) in the fp32 order of the reference."""
    rs = np.random.RandomState(seed)
    t = np.asarray(t, dtype=np.int64)
    B = t.size
    tb, tables = schedule(sched)
    te, bad = effective_t(t)
    x0 = _x0(rs, x0_family, B, n).astype(np.float32)
    if clamp_edge:
        # x0 = +-1 where the prediction will be clamped to it (the decoder NLL stays well-conditioned there), within +-0.9 elsewhere
        third = np.broadcast_to(np.arange(n)[None, :] % 3, (B, n))
        x0 = np.where(third == 0, 1.0, np.where(third == 1, -1.0, np.clip(x0, -0.9, 0.9))).astype(np.float32)
    if clamp_boundary:
        sign = np.broadcast_to(np.where(np.arange(n)[None, :] % 4 == 0, 1.0, np.where(np.arange(n)[None, :] % 4 == 2, -1.0, 0.0)), (B, n))
        # on the t = 0 rows x0 is the value the prediction will be clamped to, so that the decoder NLL stays well-conditioned there
        x0 = np.where((sign != 0) & (t == 0)[:, None], sign, x0).astype(np.float32)
    noise = rs.standard_normal((B, n))
    draw = rs.standard_normal((B, n))
    if family == "trained":
        eps = noise + 0.3 * draw
    elif family == "untrained":
        eps = draw
    elif family == "tiny":
        eps = noise + 0.02 * draw
    else:
        assert family == "offset"
        noise = noise + 50.0
        eps = noise + 0.3 * draw
    noise, eps = noise.astype(np.float32), eps.astype(np.float32)
    a = tb["sqrt_alphas_cumprod"][te].astype(np.float32)[:, None]
    b = tb["sqrt_one_minus_alphas_cumprod"][te].astype(np.float32)[:, None]
    xt = (a * x0 + b * noise).astype(np.float32)
    case = {"name": name, "kind": KINDS[kind], "kind_name": kind, "sched": sched, "family": family, "x0_family": x0_family,
            "x0": x0, "xt": xt, "eps": eps, "noise": noise, "t": t, "tables": tables, "tb": tb,
            "weights": None, "g_per": None, "g_vlb": None, "g_total": None}
    if kind == "hybrid":
        recip, recipm1 = _rows(case, ("c_recip", "c_recipm1"))
        if clamp_edge:
            # a third beyond +1, a third beyond -1 (by 0.05 ... 0.5), a third inside near x0; eps solved from x_t
            far = 1.05 + rs.uniform(0.0, 0.45, (B, n))
            near = x0 + 0.003 * rs.standard_normal((B, n))
            target = np.where(third == 0, far, np.where(third == 1, -far, near))
            case["eps"] = eps = ((recip * xt.astype(np.float64) - target) / recipm1).astype(np.float32)
            case["third"] = third
        on_edge = np.zeros((B, n), dtype=bool)
        if clamp_boundary:
            # x_t moved (by a few ulp around (sign + recipm1 eps) / recip) until the fp32 raw is exactly +-1: torch.clamp passes the
            # gradient there.  x_t is free here (the C ABI takes it as an input), not q_sample's.
            r32, m32 = (case["tables"][k][te][:, None] for k in ("c_recip", "c_recipm1"))
            prod = (m32 * eps).astype(np.float32)
            guess = ((sign.astype(np.float32) + prod) / r32).astype(np.float32)
            for k in range(-8, 9):
                cand = (guess.view(np.int32) + np.int32(k)).view(np.float32)
                hit = (sign != 0) & ~on_edge & (((r32 * cand).astype(np.float32) - prod).astype(np.float32) == sign.astype(np.float32))
                xt[hit] = cand[hit]
                on_edge |= hit
            assert on_edge.sum() >= B * n // 8, name
            case["on_edge"] = on_edge
        for _ in range(16):
            dist, margin = clamp_margin(case)
            close = (dist < margin) & ~on_edge
            if not close.any():
                break
            step = np.maximum(4.0 * margin / recipm1, 4.0 * np.spacing(np.abs(eps)).astype(np.float64))
            eps[close] = (eps.astype(np.float64) + step)[close].astype(np.float32)
        dist, margin = clamp_margin(case)
        assert (dist >= margin)[~on_edge].all(), name
    if zero_block and n >= 4:
        eps[:, : n // 4] = noise[:, : n // 4]
    # the t = -1 row is the T - 1 row before it, datum for datum
    twins = [(i - 1, i) for i in range(1, B) if t[i] == -1 and t[i - 1] == T - 1]
    for arr in (x0, xt, eps, noise):
        for src, dst in twins:
            arr[dst] = arr[src]
    if weights:
        case["weights"] = rs.uniform(0.5, 1.5, B).astype(np.float32)
    if "per" in gcfg:
        case["g_per"] = rs.standard_normal(B).astype(np.float32)
    if "total" in gcfg:
        case["g_total"] = np.array([0.7], dtype=np.float32)
    if "vlb" in gcfg:
        assert kind == "hybrid"
        gv = 2.0 * rs.standard_normal(B)
        gv[::2] = -np.abs(gv[::2])
        gv[1::2] = np.abs(gv[1::2])
        case["g_vlb"] = gv.astype(np.float32)
    for k in ("weights", "g_per", "g_vlb"):
        if case[k] is not None:
            for src, dst in twins:
                case[k][dst] = case[k][src]
    case["twins"] = twins
    case["gcfg"] = gcfg
    return case


def with_gradients(case, g_per=None, g_vlb=None, g_total=None):
    """The same data under other upstream gradients."""
    out = dict(case)
    out.update(g_per=g_per, g_vlb=g_vlb, g_total=g_total, name=case["name"] + "/regraded")
    return out


def select_rows(case, rows):
    """The sub-batch of `rows` (its own B in the batch mean)."""
    out = dict(case)
    for k in ("x0", "xt", "eps", "noise", "t", "weights", "g_per", "g_vlb", "third", "on_edge"):
        if case.get(k) is not None:
            out[k] = case[k][rows]
    out["name"] = case["name"] + "/rows"
    out["twins"] = []
    return out


def valid_rows(case):
    """Rows whose t is in range (all of them where t is not read)."""
    if case["kind"] != 2:
        return np.arange(case["t"].size)
    return np.nonzero(~effective_t(case["t"])[1])[0]


def _cdf(z):
    return 0.5 * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))


def _dcdf(z):
    th = np.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3))
    return 0.5 * (1.0 - th * th) * (math.sqrt(2.0 / math.pi) * (1.0 + 3.0 * 0.044715 * z * z))


def reference(case):
    """fp64: dict(main, vlb, loss [B], total, d_eps [B][n]) and per element g_main (the main-term part of d_eps), delta64,
    inv_std [B][1], cls (index into CLASSES), inside (the clamp passes the gradient), M, nll_unit, sat_unit, unbounded, sat_log;
    bad [B].  Rows with an out-of-range t are NaN in vlb, loss, d_eps and make the total NaN (hybrid)."""
    f = np.float64
    x0, xt, eps, noise = (case[k].astype(f) for k in ("x0", "xt", "eps", "noise"))
    B, n = eps.shape
    kind = case["kind"]
    w = np.ones(B) if case["weights"] is None else case["weights"].astype(f)
    gp = np.zeros(B) if case["g_per"] is None else case["g_per"].astype(f)
    gt = 0.0 if case["g_total"] is None else float(case["g_total"][0])
    d = eps - noise
    if kind == 0:
        main_el, dmain, mmain = np.abs(d), np.sign(d), np.ones_like(d)
    else:
        main_el, dmain, mmain = d * d, 2.0 * d, 2.0 * (np.abs(eps) + np.abs(noise))
    main = main_el.sum(axis=1) / max(n, 1)
    cb = (gp + gt * w / max(B, 1))[:, None]
    cabs = (np.abs(gp) + np.abs(gt * w / max(B, 1)))[:, None]
    g_main = cb * dmain / max(n, 1)
    M = cabs * mmain / max(n, 1)
    out = {"main": main, "vlb": None, "loss": main, "g_main": g_main, "d_eps": g_main, "M": M, "M_main": M,
           "cls": np.zeros((B, n), dtype=np.int8), "inside": np.ones((B, n), dtype=bool), "bad": np.zeros(B, dtype=bool),
           "nll_unit": np.zeros((B, n)), "sat_unit": np.zeros((B, n)), "unbounded": np.zeros((B, n), dtype=bool),
           "delta64": np.full((B, n), np.inf), "sat_log": np.zeros((B, n))}
    if kind == 2:
        recip, recipm1, c1, c2, lv1, lv2 = _rows(case)
        _, bad = effective_t(case["t"])
        t0 = (case["t"] == 0)[:, None]
        gv = np.zeros(B) if case["g_vlb"] is None else case["g_vlb"].astype(f)
        raw = recip * xt - recipm1 * eps
        inside = (raw >= -1.0) & (raw <= 1.0)
        if "on_edge" in case:                                    # the fp32 raw is exactly +-1 there: inside, whatever raw64's last bits say
            assert (np.abs(np.abs(raw) - 1.0)[case["on_edge"]] < 4.0 * U * (np.abs(recip * xt) + np.abs(recipm1 * eps) + 1.0)[case["on_edge"]]).all()
            inside = inside | case["on_edge"]
        pred = np.clip(raw, -1.0, 1.0)
        dpred = np.where(inside, -recipm1, 0.0)
        mean = c1 * pred + c2 * xt
        dd = (c1 * x0 + c2 * xt) - mean
        e1, e2, inv_std = np.exp(lv1 - lv2), np.exp(-lv2), np.exp(-0.5 * lv2)
        kl = 0.5 * ((((-1.0 + lv2) - lv1) + e1) + dd * dd * e2)
        dmean_kl = -(dd * e2)
        cen = x0 - mean
        zp, zm = inv_std * (cen + 1.0 / 255.0), inv_std * (cen - 1.0 / 255.0)
        cp, cm = _cdf(zp), _cdf(zm)
        lo = case["x0"] < np.float32(-0.999)
        hi = ~lo & (case["x0"] > np.float32(0.999))
        delta = np.where(lo, cp, np.where(hi, 1.0 - cm, cp - cm))
        num = np.where(lo, _dcdf(zp), np.where(hi, -_dcdf(zm), _dcdf(zp) - _dcdf(zm)))
        with np.errstate(divide="ignore", invalid="ignore"):
            dcen = np.where(delta >= FLOOR, num * inv_std / delta, 0.0)
        nll = -np.log(np.maximum(delta, FLOOR))
        term = np.where(t0, nll, kl)
        dterm = np.where(t0, dcen, dmean_kl) * c1 * dpred
        vb = cb + gv[:, None]
        vabs = cabs + np.abs(gv)[:, None]
        g_vlb = vb * dterm / (n * LN2)
        vlb = term.sum(axis=1) / n / LN2
        md = np.abs(c1 * x0) + 2.0 * np.abs(c2 * xt) + np.abs(c1) * (np.abs(recip * xt) + np.abs(recipm1 * eps))
        chain = vabs * np.abs(c1 * recipm1) / (n * LN2)
        mpred = np.where(inside, np.abs(recip * xt) + np.abs(recipm1 * eps), 1.0)
        mcen = np.abs(x0) + np.abs(c1) * mpred + np.abs(c2 * xt)
        m_kl = np.where(inside & ~t0, md * e2 * chain, 0.0)
        nll_in = inside & t0
        with np.errstate(divide="ignore", invalid="ignore"):
            nll_unit = np.where(nll_in, (inv_std + np.abs(dcen)) / delta * chain, 0.0)
            sat_log = np.log((delta * (1.0 + SAT_R) + SAT_E) / np.maximum(delta * (1.0 - SAT_R) - SAT_E, FLOOR))
        unbounded = nll_in & (delta < DELTA_MIN)
        # magnitude companions of the values: what one rounding of every intermediate is worth in the term
        mdv = np.abs(c1 * x0) + 2.0 * np.abs(c2 * xt) + np.abs(c1) * mpred
        mag_kl = 0.5 * ((1.0 + np.abs(lv2) + np.abs(lv1) + e1) + (dd * dd + 2.0 * np.abs(dd) * mdv) * e2)
        dc = np.maximum(delta, FLOOR)
        with np.errstate(divide="ignore", invalid="ignore"):
            dlog = np.abs(num) * inv_std / dc
        mag_nll = np.abs(np.log(dc)) + np.where(delta < DELTA_MIN, 0.0, 4.0 / dc + dlog * (mcen + np.abs(cen) + 1.0 / 255.0))
        mv_vlb = np.where(t0, mag_nll, mag_kl).sum(axis=1) / n / LN2
        cls = np.where(t0, np.where(lo, 2, np.where(hi, 3, 4)), 1).astype(np.int8)
        vlb = np.where(bad, np.nan, vlb)
        nan_rows = np.where(bad, np.nan, 0.0)[:, None]
        out.update(vlb=vlb, loss=vlb + main, d_eps=g_main + g_vlb + nan_rows, M=M + m_kl, cls=cls, inside=inside, bad=bad,
                   nll_unit=np.where(unbounded, 0.0, nll_unit), sat_unit=np.where(nll_in, chain * inv_std, 0.0),
                   unbounded=unbounded, delta64=np.where(t0, delta, np.inf), inv_std=inv_std, dcen=dcen,
                   sat_log=np.where(t0 & (delta < DELTA_MIN), sat_log, 0.0), mv_vlb=mv_vlb, t0=np.broadcast_to(t0, (B, n)))
    out["total"] = float((out["loss"] * w).sum() / B) if B else float("nan")
    return out


def bound(case, ref, K=None):
    """[B][n] allowance on |d_eps - ref| (inf on the unbounded elements, whose own condition is `sat_limit`)."""
    K = K or {"kl": K_KL, "nll": K_NLL}
    allow = K["kl"] * U * ref["M"] + K["nll"] * U * ref["nll_unit"]
    return np.where(ref["unbounded"], np.inf, allow)


def sat_limit(case, ref, c_sat=None, K=None):
    """[B][n] limit on |d_eps| of an unbounded element."""
    K = K or {"kl": K_KL, "nll": K_NLL}
    return np.abs(ref["g_main"]) + K["kl"] * U * ref["M_main"] + ref["sat_unit"] * (C_SAT if c_sat is None else c_sat)


def unbounded_share(ref):
    """Share of the t = 0 elements that are unbounded (0 where there is none)."""
    pool = ref["cls"] >= 2
    return float(ref["unbounded"].sum()) / max(int(pool.sum()), 1)


def class_names(ref):
    """[B][n] of strings like 'nll_mid/in'."""
    names = np.array([f"{c}/{s}" for c in CLASSES for s in ("out", "in")])
    return names[ref["cls"].astype(np.int64) * 2 + ref["inside"]]


def element_failures(tag, got, case, ref, ledger=None, K=None, c_sat=None):
    """Per class and per sample: |got - ref| <= bound on the bounded elements, finite and within `sat_limit` on the unbounded ones.
    Prints the worst err / bound per class and returns the failure lines (empty: passes).  Rows with an out-of-range t are not
    judged here.  ledger: {class: worst ratio so far}, updated."""
    got = np.asarray(got, dtype=np.float64)
    allow = bound(case, ref, K)
    limit = sat_limit(case, ref, c_sat, K)
    names = class_names(ref)
    rows_ok = ~ref["bad"][:, None] & np.ones(got.shape, dtype=bool)
    err = np.abs(got - ref["d_eps"])
    lines, shown = [], []
    for cname in np.unique(names[rows_ok]) if rows_ok.any() else []:
        sel = rows_ok & (names == cname)
        bounded = sel & ~ref["unbounded"]
        if bounded.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bounded, np.where(allow > 0, err / allow, np.where(err == 0, 0.0, np.inf)), 0.0)
            ratio = np.where(np.isnan(ratio) | (bounded & ~np.isfinite(got)), np.inf, ratio)
            worst_b = ratio.max(axis=1)
            b, i = np.unravel_index(np.argmax(ratio), ratio.shape)
            shown.append(f"{cname} {ratio[b, i]:.3f}")
            if ledger is not None:
                ledger[cname] = max(ledger.get(cname, 0.0), float(ratio[b, i]))
            for bb in np.nonzero(worst_b > 1.0)[0]:
                ii = int(np.argmax(ratio[bb]))
                lines.append(f"{tag}: {cname} sample {bb} (t {case['t'][bb]}) element {ii}: got {got[bb, ii]:.9g} ref "
                             f"{ref['d_eps'][bb, ii]:.9g} err / bound {ratio[bb, ii]:.3f} ({int((ratio[bb] > 1).sum())} elements)")
        loose = sel & ref["unbounded"]
        if loose.any():
            over = loose & ~(np.isfinite(got) & (np.abs(got) <= limit))
            shown.append(f"{cname} unbounded {int(loose.sum())}")
            for bb in np.nonzero(over.any(axis=1))[0]:
                ii = int(np.argmax(over[bb]))
                lines.append(f"{tag}: {cname} unbounded sample {bb} element {ii}: got {got[bb, ii]:.9g} limit {limit[bb, ii]:.9g}")
    print(f"{tag:44s} " + "  ".join(shown))
    return lines


def value_targets(case, ref, oracle):
    """Per sample (target, allowance) of main, vlb, loss and of the total.  oracle: `oracle_values(case)` or None (then every
    target is fp64).  A row that holds an unbounded element takes the fp32 oracle's vlb as its target and the sum of its
    elements' `sat_log` on top of the relative bar."""
    bar = VALUE_BAR[case["family"]]
    B, n = case["eps"].shape
    out = {"main": (ref["main"], bar * np.abs(ref["main"]))}
    w = np.ones(B) if case["weights"] is None else case["weights"].astype(np.float64)
    if case["kind"] == 2:
        sat = ref["sat_log"].sum(axis=1) / (n * LN2)
        loose = sat > 0
        vlb_t = ref["vlb"].copy()
        if loose.any():
            assert oracle is not None
            vlb_t[loose] = oracle["vlb"][loose]
        vlb_a = bar * ref["mv_vlb"] + sat
        out["vlb"] = (vlb_t, vlb_a)
        out["loss"] = (vlb_t + ref["main"], vlb_a + bar * np.abs(ref["main"]))
    else:
        out["loss"] = out["main"]
    tgt, allow = out["loss"]
    out["total"] = (float((tgt * w).sum() / B), float((allow * w).sum() / B) + bar * abs(float((tgt * w).sum() / B)))
    return out


def oracle_values(case):
    """fp32 torch oracle (the expressions of oracle.diffusion_oracle.loss_terms over the case's own x_t) on the rows whose t is in range: dict(loss, vlb [B], NaN elsewhere)."""
    import torch
    rows = valid_rows(case)
    B = case["t"].size
    sub = select_rows(case, rows)
    tt = torch.from_numpy(sub["t"])
    tt = torch.where(tt < 0, tt + T, tt)
    x0, xt, eps, noise = (torch.from_numpy(sub[k]) for k in ("x0", "xt", "eps", "noise"))
    vlb = None
    if case["kind"] == 0:
        per = (eps - noise).abs().mean(dim=1)
    else:
        per = (eps - noise).square().mean(dim=1)
    if case["kind"] == 2:
        vlb = do.vlb_terms(case["tb"], x0, xt, tt, eps)[0]
        per = vlb + per
    out = {"loss": np.full(B, np.nan), "vlb": np.full(B, np.nan)}
    out["loss"][rows] = per.numpy().astype(np.float64)
    if vlb is not None:
        out["vlb"][rows] = vlb.numpy().astype(np.float64)
    return out


def _matrix():
    out, h = [], 0
    sizes = (1, 255, 256, 257, 3 * 7 * 5)
    i = 0
    for kind in ("l1", "l2", "hybrid"):
        for weights in (False, True):
            for gcfg in GCFGS if kind == "hybrid" else GCFGS[:3]:
                if kind == "hybrid":
                    sched, family = ("linear", "cosine")[h % 2], FAMILIES[(h // 2) % 4]
                    h += 1
                else:
                    sched, family = "linear", FAMILIES[i % 4]
                n = sizes[i % len(sizes)]
                out.append(make_case(f"{kind}-{'w' if weights else 'now'}-{gcfg}-{sched}-{family}-n{n}", kind, sched, family, n,
                                     weights=weights, gcfg=gcfg, zero_block=(kind == "l1"), seed=100 + i))
                i += 1
    return out


@functools.lru_cache(maxsize=1)
def cases():
    """The list: the kind x weights x upstream-gradient matrix over both schedules, the four eps families and the small sizes;
    the x0 families; out-of-range t; the clamp edges; the large shapes.  Every hybrid case holds the rows of T_ROWS unless named."""
    out = _matrix()
    for j, fam in enumerate(("plus", "minus", "edges")):
        for sched in ("linear", "cosine"):
            out.append(make_case(f"x0-{fam}-{sched}", "hybrid", sched, "trained", 257, weights=True, gcfg="per+total", x0_family=fam,
                                 seed=200 + j))
    out.append(make_case("x0-edges-untrained", "hybrid", "linear", "untrained", 258, t=(0, 0, 0, 1), gcfg="total", x0_family="edges",
                         seed=210))
    for j, sched in enumerate(("linear", "cosine")):
        out.append(make_case(f"badt-{sched}", "hybrid", sched, "trained", 257, t=T_ROWS + T_BAD, weights=True, gcfg="vlb+per+total",
                             seed=220 + j))
        out.append(make_case(f"clamp-edge-{sched}", "hybrid", sched, "trained", 258, gcfg="vlb+per+total", clamp_edge=True,
                             seed=230 + j))
    out.append(make_case("clamp-boundary", "hybrid", "linear", "trained", 256, t=(0, 1, 50, 500, T - 2), weights=True,
                         gcfg="vlb+per+total", clamp_boundary=True, seed=235))
    out.append(make_case("sweep-64x256+3", "hybrid", "linear", "untrained", 64 * 256 + 3, t=(0, 500, 1), weights=True, gcfg="total",
                         seed=240))
    out.append(make_case("stride-1024x256+257", "hybrid", "linear", "trained", 1024 * 256 + 257, t=(0,), gcfg="total", seed=241))
    out.append(make_case("stride-kl-1024x256+257", "hybrid", "cosine", "tiny", 1024 * 256 + 257, t=(500,), gcfg="vlb", seed=242))
    rs = np.random.RandomState(7)
    out.append(make_case("fold-B300", "hybrid", "linear", "trained", 64, t=rs.choice(T_ROWS, 300), weights=True, gcfg="per+total",
                         seed=243))
    out.append(make_case("fold-B300-l2", "l2", "linear", "offset", 64, t=np.zeros(300, dtype=np.int64), weights=True, gcfg="total",
                         seed=244))
    for c in out:
        if c["kind"] == 2:
            share = unbounded_share(reference_of(c["name"], c))
            assert share <= UNBOUNDED_CAP, (c["name"], share)
    return out


_REFS = {}


def reference_of(name, case=None):
    """`reference` of a case of `cases()`, computed once and not to be written to."""
    if name not in _REFS:
        if case is None:
            case = next(c for c in cases() if c["name"] == name)
        _REFS[name] = reference(case)
    return _REFS[name]


def case_names():
    return [c["name"] for c in cases()]


def get(name):
    return next(c for c in cases() if c["name"] == name)
