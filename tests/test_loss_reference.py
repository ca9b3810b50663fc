"""CPU: the fp64 loss reference and error model of tests/loss_cases.py.  Its gradient against float64 torch autograd of a plain
restatement written here; the upstream fixture (tests/golden/loss_kat.npz) and the numpy fp32 restatement of the reference
arithmetic (oracle.diffusion_oracle.loss_grad_analytic) within the model's bound, which is where K_KL, K_NLL and C_SAT come from;
the fp32 torch oracle's per-sample values, which is where VALUE_BAR comes from; the builder's caps.  Run with -s for the figures."""
import math
import os

import numpy as np
import pytest
import torch

import loss_cases as lc
from conftest import GOLDEN
from oracle import diffusion_oracle as do

G = np.load(os.path.join(GOLDEN, "loss_kat.npz"))
# without the case whose fp32 raw sits on the clamp's edge by construction: float64 autograd decides the side on other bits
NAMES = [c["name"] for c in lc.cases() if "on_edge" not in c]


def _round_up_one_digit(x):
    e = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / e - 1e-9) * e


def _autograd_objective(case, rows):
    """A plain statement of sum_b g_per[b] loss[b] + sum_b g_vlb[b] vlb[b] + g_total mean_b(w_b loss[b]) in float64 torch, of the
    rows whose t is in range (the batch mean keeps the whole batch's B).  Returns (objective, eps leaf)."""
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a[rows])).double()
    B = case["t"].size
    x0, xt, noise = t64(case["x0"]), t64(case["xt"]), t64(case["noise"])
    eps = t64(case["eps"]).requires_grad_(True)
    per = (eps - noise).abs().mean(dim=1) if case["kind"] == 0 else ((eps - noise) ** 2).mean(dim=1)
    vlb = None
    if case["kind"] == 2:
        t = torch.from_numpy(case["t"][rows])
        idx = torch.where(t < 0, t + lc.T, t)
        col = lambda k: torch.from_numpy(case["tables"][k]).double()[idx][:, None]
        pred = (col("c_recip") * xt - col("c_recipm1") * eps).clamp(-1, 1)
        mean = col("c_coef1") * pred + col("c_coef2") * xt
        true_mean = col("c_coef1") * x0 + col("c_coef2") * xt
        lv1, lv2 = col("c_post_logvar"), col("c_model_logvar")
        kl = 0.5 * (-1 + lv2 - lv1 + torch.exp(lv1 - lv2) + (true_mean - mean) ** 2 * torch.exp(-lv2))
        cdf = lambda z: 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * torch.pow(z, 3))))
        inv_std = torch.exp(-0.5 * lv2)
        cp, cm = cdf(inv_std * (x0 - mean + 1.0 / 255.0)), cdf(inv_std * (x0 - mean - 1.0 / 255.0))
        x32 = torch.from_numpy(case["x0"][rows])
        logp = torch.where(x32 < -0.999, torch.log(cp.clamp(min=1e-12)),
                           torch.where(x32 > 0.999, torch.log((1.0 - cm).clamp(min=1e-12)), torch.log((cp - cm).clamp(min=1e-12))))
        vlb = torch.where(t == 0, (-logp).mean(dim=1), kl.mean(dim=1)) / math.log(2.0)
        per = per + vlb
    obj = per.sum() * 0.0
    if case["g_per"] is not None:
        obj = obj + (t64(case["g_per"]) * per).sum()
    if case["g_vlb"] is not None:
        obj = obj + (t64(case["g_vlb"]) * vlb).sum()
    if case["g_total"] is not None:
        w = t64(case["weights"]) if case["weights"] is not None else 1.0
        obj = obj + float(case["g_total"][0]) * (per * w).sum() / B
    return obj, eps, per, vlb


@pytest.mark.parametrize("name", NAMES)
def test_reference_gradient_is_float64_autograd_of_a_plain_restatement(name):
    """1e-10 of the sample's own maximum; the clamp margin of every case allows it (nothing sits on the edge)."""
    lc.cases()
    case, ref = lc.get(name), lc.reference_of(name)
    rows = lc.valid_rows(case)
    obj, eps, per, vlb = _autograd_objective(case, rows)
    obj.backward()
    got, want = eps.grad.numpy(), ref["d_eps"][rows]
    assert np.isfinite(want).all()
    scale = np.abs(want).max(axis=1, keepdims=True)
    # The unbounded elements (delta64 < DELTA_MIN) are ill-conditioned in float64 as well: 1 - cdf_min and cdf_plus - cdf_min carry
    # an absolute 2^-53 or two, and the gradient divides by them.  They get the error model's own conditioning term in float64 units
    # on top (64 * 2^-53 where the fp32 bound has K_NLL * 2^-24); every other element is held to 1e-10 of the sample's maximum.
    sat = ref["sat_unit"][rows] * (1.0 + np.abs(ref.get("dcen", 0.0 * want)[rows]) / ref.get("inv_std", 1.0 + 0.0 * scale)[rows]) \
        / np.minimum(ref["delta64"][rows], 1.0)
    extra = np.where(ref["unbounded"][rows], 64.0 * 2.0 ** -53 * sat, 0.0)
    assert (np.abs(got - want) <= 1e-10 * scale + extra).all(), float((np.abs(got - want) / np.maximum(scale, 1e-300)).max())
    np.testing.assert_allclose(per.detach().numpy(), ref["loss"][rows], rtol=1e-8)       # log(delta) near 0: see above
    if vlb is not None:
        np.testing.assert_allclose(vlb.detach().numpy(), ref["vlb"][rows], rtol=1e-8, atol=1e-300)
    # rows with an out-of-range t: NaN, and they make the total NaN
    if ref["bad"].any():
        assert np.isnan(ref["d_eps"][ref["bad"]]).all() and np.isnan(ref["vlb"][ref["bad"]]).all() and math.isnan(ref["total"])


def test_builder_margins_twins_caps_and_shares():
    """x_t is the reference's fp32 q_sample; every clamp margin holds; the t = -1 row is its T - 1 twin; at most 10 % of a case's
    t = 0 elements are unbounded and none of the others; the clamp-edge thirds are where they were put."""
    shares = {}
    for case in lc.cases():
        ref = lc.reference_of(case["name"])
        rows = lc.valid_rows(case)
        if case["kind"] == 2:
            t = torch.from_numpy(case["t"][rows])
            t = torch.where(t < 0, t + lc.T, t)
            xt = do.q_sample(case["tb"], torch.from_numpy(case["x0"][rows]), t, torch.from_numpy(case["noise"][rows]))
            free = case.get("on_edge", np.zeros(case["xt"].shape, dtype=bool))
            assert np.array_equal(xt.numpy()[~free[rows]], case["xt"][rows][~free[rows]]), case["name"]
            dist, margin = lc.clamp_margin(case)
            assert (dist >= margin)[~free].all() and (margin >= 1e-4).all()
            if free.any():
                tab = case["tables"]
                raw32 = tab["c_recip"][case["t"]][:, None] * case["xt"] - tab["c_recipm1"][case["t"]][:, None] * case["eps"]
                assert raw32.dtype == np.float32 and (np.abs(raw32[free]) == 1).all() and (raw32[free] == 1).any() \
                    and (raw32[free] == -1).any()
                print(f"{case['name']}: {int(free.sum())} elements with an fp32 raw of exactly +-1")
            assert not ref["unbounded"][ref["cls"] < 2].any()
            share = lc.unbounded_share(ref)
            assert share <= lc.UNBOUNDED_CAP, (case["name"], share)
            pool = ref["cls"] >= 2
            if pool.any():
                s = shares.setdefault(case["family"], [0, 0, 0.0])
                s[0] += int(ref["unbounded"].sum())
                s[1] += int(pool.sum())
                s[2] = max(s[2], share)
            if "third" in case:
                assert (ref["inside"] == (case["third"] == 2)).all()
                assert (ref["d_eps"][~ref["inside"]] == ref["g_main"][~ref["inside"]]).all()
        for src, dst in case["twins"]:
            for k in ("x0", "xt", "eps", "noise"):
                assert np.array_equal(case[k][src], case[k][dst])
        if case["kind"] == 0:
            n = case["eps"].shape[1]
            if n >= 4:
                assert (ref["d_eps"][:, : n // 4] == 0).all()
    for fam, (k, n, worst) in sorted(shares.items()):
        print(f"unbounded share, {fam:9s}: {k} of {n} = {k / n:.4f}, worst case {worst:.4f}")
    assert shares["trained"][0] == 0 and shares["tiny"][0] == 0


def _fp32_restatement(case):
    """(rows, the data under g_total = 1 alone, its reference, loss_grad_analytic in fp32 on it)."""
    rows = lc.valid_rows(case)
    sub = lc.with_gradients(lc.select_rows(case, rows), g_total=np.array([1.0], dtype=np.float32))
    ref = lc.reference(sub)
    g32 = do.loss_grad_analytic(case["tb"], sub["x0"], sub["t"], sub["eps"], sub["noise"], sub["weights"], case["kind_name"],
                                dtype=np.float32)
    assert g32.dtype == np.float32
    return sub, ref, g32.astype(np.float64)


def test_constants_are_twice_what_the_fp32_restatement_needs():
    """The smallest K_KL, K_NLL and C_SAT that cover the numpy fp32 restatement of the reference arithmetic over every case; the
    fixed constants are those doubled and rounded up to one digit."""
    k_kl = k_nll = c_sat = 0.0
    runs = []
    cases = [c for c in lc.cases() if "on_edge" not in c]            # loss_grad_analytic forms x_t itself; that case's x_t is free
    for case in cases:
        sub, ref, g32 = _fp32_restatement(case)
        err = np.abs(g32 - ref["d_eps"])
        plain = (ref["nll_unit"] == 0) & ~ref["unbounded"]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(plain & (ref["M"] > 0), err / (lc.U * ref["M"]), 0.0)
        assert (err[plain & (ref["M"] == 0)] == 0).all()
        k_kl = max(k_kl, float(r.max()))
        runs.append((sub, ref, g32, err))
    for sub, ref, g32, err in runs:
        nll = ref["nll_unit"] > 0
        if nll.any():
            r = (err[nll] - k_kl * lc.U * ref["M"][nll]) / (lc.U * ref["nll_unit"][nll])
            k_nll = max(k_nll, float(r.max()))
        ub = ref["unbounded"]
        if ub.any():
            assert np.isfinite(g32[ub]).all()
            vlb_part = np.abs(g32 - ref["g_main"])[ub] / ref["sat_unit"][ub]
            c_sat = max(c_sat, float(vlb_part.max()))
    print(f"measured K_KL {k_kl:.3f}  K_NLL {k_nll:.3f}  C_SAT {c_sat:.3f}   fixed K_KL {lc.K_KL:g}  K_NLL {lc.K_NLL:g}  C_SAT {lc.C_SAT:g}")
    assert lc.K_KL == _round_up_one_digit(2.0 * k_kl)
    assert lc.K_NLL == _round_up_one_digit(2.0 * k_nll)
    assert lc.C_SAT == _round_up_one_digit(2.0 * c_sat)
    # and under the fixed constants the restatement passes the very check the device gets
    bad = []
    for case, (sub, ref, g32, err) in zip(cases, runs):
        bad += lc.element_failures(case["name"], g32, sub, ref)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ["l1", "l2", "hybrid"])
@pytest.mark.parametrize("lw", ["none", "prop-t"])
def test_upstream_fixture_gradient_lies_within_the_bound(kind, lw):
    """The reference implementation's own fp32 autograd (loss_kat.npz) under the model with the fixed constants."""
    tag = f"{kind}_{lw}"
    tb, tables = lc.schedule("linear")
    flat = lambda a: np.ascontiguousarray(a.reshape(a.shape[0], -1))
    case = {"name": tag, "kind": lc.KINDS[kind], "kind_name": kind, "sched": "linear", "family": "untrained", "tb": tb,
            "tables": tables, "x0": flat(G["x0"]), "xt": flat(G[f"{tag}_x_t"]), "eps": flat(G["eps"]), "noise": flat(G["noise"]),
            "t": G[f"{tag}_t"].astype(np.int64), "weights": None if lw == "none" else G[f"{tag}_weights"], "g_per": None,
            "g_vlb": None, "g_total": np.array([1.0], dtype=np.float32)}
    ref = lc.reference(case)
    bad = lc.element_failures(tag, flat(G[f"{tag}_d_eps"]), case, ref)
    assert not bad, "\n".join(bad)
    if kind == "hybrid":
        assert lc.unbounded_share(ref) <= lc.UNBOUNDED_CAP
        dist, margin = lc.clamp_margin(case)
        print(f"{tag}: unbounded share {lc.unbounded_share(ref):.4f}, elements inside the clamp margin {(dist < margin).sum()}")


def test_fp32_oracle_values_give_the_value_bars():
    """Per-sample main / vlb / loss of the fp32 torch oracle against the reference: the worst relative difference per eps family
    on rows without an unbounded element is what MEASURED_VALUE records (the device's bar is 4x that, floor 2e-6).  Rows with an
    unbounded element (t = 0, untrained eps) are not compared with fp64: the 1e-12 floor and the granularity of an fp32 cdf
    difference are the reference's behaviour, fp64 does not reproduce them, and the device is compared with this oracle there;
    here the oracle must lie within the bar those rows get around fp64's value widened by the same allowance."""
    worst = {}
    for case in lc.cases():
        ref = lc.reference_of(case["name"])
        rows = lc.valid_rows(case)
        orc = lc.oracle_values(case)
        B, n = case["eps"].shape
        loose = ref["sat_log"].sum(axis=1) > 0
        tight = np.zeros(B, dtype=bool)
        tight[rows] = True
        tight &= ~loose
        mv = ref["main"] + (ref["mv_vlb"] if case["kind"] == 2 else 0.0)
        figs = [np.abs(orc["loss"] - ref["loss"])[tight] / mv[tight]]
        if case["kind"] == 2:
            figs.append(np.abs(orc["vlb"] - ref["vlb"])[tight] / ref["mv_vlb"][tight])
            sat = ref["sat_log"].sum(axis=1) / (n * lc.LN2)
            assert (np.abs(orc["vlb"] - ref["vlb"])[loose] <= (lc.VALUE_BAR[case["family"]] * ref["mv_vlb"] + sat)[loose]).all()
            if loose.any():
                print(f"{case['name']}: rows with unbounded elements: oracle - fp64 {np.abs(orc['vlb'] - ref['vlb'])[loose].max():.3e} "
                      f"bits, allowance {sat[loose].max():.3e}")
        w = max(float(f.max()) for f in figs if f.size)
        worst[case["family"]] = max(worst.get(case["family"], 0.0), w)
    for fam in lc.FAMILIES:
        print(f"fp32 oracle values, {fam:9s}: worst relative difference {worst[fam]:.3e}  recorded {lc.MEASURED_VALUE[fam]:.3e}  "
              f"device bar {lc.VALUE_BAR[fam]:.3e}")
    for fam in lc.FAMILIES:
        assert worst[fam] <= lc.MEASURED_VALUE[fam] <= 1.5 * worst[fam] + 1e-9
        assert lc.VALUE_BAR[fam] == max(4.0 * lc.MEASURED_VALUE[fam], 2e-6)
