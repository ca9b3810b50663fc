"""CPU: the statement, restatement, bars and kernel model of tests/gn_bwd_cases.py, which tests/test_gpu_gn_bwd_elements.py holds
csrc/gn_backward.hip to.  The fp64 statement against fp64 autograd of [resample](silu(group_norm(cat(x)))); the fp32 restatement
against fp64 on every (case, regime) with 4 r32 <= CAP; the FLOOR constants against their measurement; the case list against the
guards it is there for; the numpy model of the three passes against the statement, and every planted defect seen by a named case."""
import pytest
import torch
import torch.nn.functional as F

import gn_bwd_cases as gc


def test_case_list_reaches_every_guard():
    g = {c.name: gc.Geo(c) for c in gc.CASES}
    c = gc.BY_NAME
    assert g["s01"].cpg == 1 and g["s01"].R == 32 and g["s01"].P < 4 * g["s01"].R and g["s01"].sp == 20 < g["s01"].R
    assert g["s02"].nbp == 64 and c["s02"].B == 65
    assert g["s03"].aslabs == 21 and g["s03"].P - 20 * g["s03"].asp == 40 and g["s03"].P % c["s03"].nslab != 0
    assert g["s04"].cpg == 3 and g["s04"].R * g["s04"].TQ == 240
    assert g["s05"].cpg == 5 and g["s05"].R == 6 and (g["s05"].Ha, g["s05"].Wa) == (6, 10) and c["s05"].a_mode == 2
    assert (g["s06"].Ha, g["s06"].Wa) == (12, 20) and c["s06"].a_mode == 1
    assert g["s07"].cpg == 12 and c["s07"].c0 % 12 != 0 and g["s07"].R == 2 and len(c["s07"].forms) == 8
    assert g["s08"].nbp == 21 and c["s08"].B == 22
    assert g["s09"].C4 == 256 and g["s09"].R == 1 and g["s09"].cpg == 32 and g["s09"].nbp == 8 and c["s09"].B % 8 == 1
    assert g["s10"].C4 == 272 and g["s10"].npass == 2 and c["s10"].c0 == 1024
    assert g["s11"].cpg == 64 and g["s11"].nbp == 4 and g["s11"].C4 == 512
    assert g["s12"].S == 4 and c["s12"].nslab == 8 * 4 + 5 and g["s12"].sp * 32 == g["s12"].P           # one trip, a tail, empty slabs
    assert g["s13"].S == 32 and c["s13"].nslab == 8 * 32
    assert c["s14"].act == 0 and c["s14"].forms == ((0, True),) and c["s15"].layout == "strided"
    assert c["s16a"].ready and c["s16b"].ready
    assert {(k.a_mode, k.act) for k in gc.CASES} == {(a, t) for a in (0, 1, 2) for t in (0, 1)}          # all six template instances
    assert all(k.Hs != k.Ws for k in gc.CASES if k.a_mode)
    assert len({k.name for k in gc.CASES}) == len(gc.CASES)
    for name in ("s01", "s02", "s03", "s04", "s08", "s13"):
        assert c[name].regimes == gc.REGIMES
    for defect, names in gc.SEEN_BY.items():
        assert defect in gc.DEFECTS and all(n in c for n in names)
    assert set(gc.SEEN_BY) == set(gc.DEFECTS)


@pytest.mark.parametrize("item", gc.ITEMS, ids=gc.item_id)
def test_restatement_against_fp64(item):
    """The fp32 restatement is the statement: its worst row is at rounding level, four times it fits under CAP (so no device bar is
    clamped below 4 r32), and it passes its own bar."""
    p = gc.prepared(*item)
    for form, outs in p["targets"].items():
        for name, t in outs.items():
            assert (t.S >= t.ref.abs() * (1 - 1e-12)).all(), (form, name)
            e = gc.row_error(t.y32, t.ref, t.S)
            assert torch.isfinite(e).all() and (e <= p["bar"][t.cls]).all(), (form, name, gc.worst_row(e))
    for cls, r32 in p["r32"].items():
        print(f"{gc.item_id(item)}: {cls} r32 {r32:.2e}, bar {p['bar'][cls]:.2e}")
        assert 4 * r32 <= gc.CAP, (cls, r32)
        assert gc.FLOOR[cls] <= p["bar"][cls] <= gc.CAP


def test_floors():
    """FLOOR[class] is 4 x the worst iid row figure of the restatement over all shapes, within a factor 1.5."""
    worst = {}
    for item in gc.ITEMS:
        if item[1] == "iid":
            for cls, r32 in gc.r32_of(*item)[0].items():
                worst[cls] = max(worst.get(cls, (-1.0, "")), (r32, item[0]))
    assert set(worst) == set(gc.FLOOR)
    for cls, (r32, where) in sorted(worst.items()):
        print(f"{cls}: worst iid r32 {r32:.3e} ({where}), 4 x = {4 * r32:.3e}, FLOOR {gc.FLOOR[cls]:.3e}, CAP {gc.CAP:.0e}")
    for cls, (r32, where) in worst.items():
        assert gc.FLOOR[cls] / 1.5 <= 4 * r32 <= 1.5 * gc.FLOOR[cls], (cls, r32, where)
        assert gc.FLOOR[cls] < gc.CAP


@pytest.mark.parametrize("item", [(c.name, r) for c in gc.CASES if not c.ready for r in c.regimes if r in ("iid", "off_centre", "saturated")],
                         ids=gc.item_id)
def test_statement_is_autograd(item):
    """The fp64 statement with the exact fp64 mean / rstd is fp64 autograd of [resample](silu(group_norm(cat(x)))) to 1e-11 of the
    largest S.  With the mean / rstd the launch is given -- rounded to fp32 -- xhat moves by at most e = 2^-24 (|mean| rstd + |xhat|),
    y by |gamma| e, silu'(y) by |gamma| e / 2 (|silu''| <= 1 / 2), so each term of dx, dgamma and dbeta moves by a few
    2^-24 (1 + |mean| rstd) (1 + |gamma|) of itself: the statement is held to 16 times that, of the largest S."""
    c = gc.BY_NAME[item[0]]
    geo, o = gc.Geo(c), gc.operands(c, item[1])
    B, C = c.B, geo.C
    x = o["x"].double().requires_grad_(True)
    gamma, beta = o["gamma"].double().requires_grad_(True), o["beta"].double().requires_grad_(True)
    a = F.group_norm(x.view(B, c.Hs, c.Ws, C).permute(0, 3, 1, 2), gc.GROUPS, gamma, beta, gc.EPS)
    if c.act:
        a = F.silu(a)
    if c.a_mode == 1:
        a = F.interpolate(a, scale_factor=2, mode="nearest")
    elif c.a_mode == 2:
        a = F.avg_pool2d(a, 2)
    (a.permute(0, 2, 3, 1).reshape(B, geo.Pa, C) * o["da"].double()).sum().backward()
    want = dict(dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
    exact = gc.statement(o, c, torch.float64, o["mean64"], o["rstd64"])
    given = gc.statement(o, c, torch.float64)
    S = gc.scales(o, c, given)
    loose = 16 * 2.0 ** -24 * (1 + (o["mean64"].abs() * o["rstd64"]).max().item()) * (1 + o["gamma"].abs().max().item())
    for k, w in want.items():
        top = S[k].max().item()
        e0, e1 = (exact[k] - w).abs().max().item() / top, (given[k] - w).abs().max().item() / top
        print(f"{gc.item_id(item)} {k}: exact moments {e0:.2e}, fp32 moments {e1:.2e} (allowed {loose:.2e})")
        assert e0 <= 1e-11 and e1 <= loose, (k, e0, e1)


@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_model_is_the_statement(name):
    """The numpy model of the three passes, without a defect, is the fp64 statement on every form."""
    p = gc.prepared(name, "iid")
    for form in p["c"].forms:
        for out, cls, fig, row, bar, beyond, rows, glob in gc.judge(p, form, gc.kernel_model(p, form)):
            assert fig <= 1e-11, (form, out, fig, row)


@pytest.mark.parametrize("defect", gc.DEFECTS)
def test_planted_defect_is_seen(defect):
    """Each defect, planted in the model, puts at least one row of every case named for it beyond the case's bar."""
    for name in gc.SEEN_BY[defect]:
        p = gc.prepared(name, "iid")
        worst = (0.0, None)
        for form in p["c"].forms:
            for out, cls, fig, row, bar, beyond, rows, glob in gc.judge(p, form, gc.kernel_model(p, form, defect)):
                worst = max(worst, (fig / bar, (form, out, fig, bar, beyond, rows)), key=lambda v: v[0])
        print(f"{defect} on {name}: worst figure / bar {worst[0]:.3g} at {worst[1]}")
        assert worst[0] > 1, (defect, name, worst)
