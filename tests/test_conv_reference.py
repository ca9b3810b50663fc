"""CPU: the references, restatements and bars of tests/conv_cases.py, which tests/test_gpu_conv_conditioning.py holds the
convolution kernels to.  The fp32 restatements of the three arithmetic classes against fp64 on every (case, regime); 4 r32 <= CAP on
every one; the FLOOR constants against their measurement; the per-plane figure on planted faults; the lattice bound."""
import pytest
import torch

import conv_cases as cc

ITEMS = sorted({(c, r) for c, r, _ in cc.cases()}, key=lambda cr: (cc.SHAPES.index(cr[0]), cc.REGIMES.index(cr[1])))
LATTICE = [c for c, r in ITEMS if r == "lattice"]


def _id(cr):
    return cc.case_id((cr[0], cr[1], 0))


def test_case_list_reaches_every_path_and_regime():
    items = cc.cases()
    assert {c.cfg for c, _, _ in items} == {-1, 0, 1, 2, 3, 4, 5, 6, 7}
    assert {v for c, _, v in items if c.cfg == 3} == {0, 3, 6, 7}
    for regime in cc.REGIMES:
        for cls in ("direct", "wino23", "wino43"):
            assert any(r == regime and cc.klass(c) == cls for c, r, _ in items), (regime, cls)
    # every lattice launch is plain, and the fused operand forms of the issue are among them
    lat = [c for c in LATTICE]
    assert any(c.a_mode == 1 for c in lat) and any(c.a_mode == 2 for c in lat) and any(c.cin[1] for c in lat)
    assert any(c.ksplit > 1 for c in lat) and any(c.res_up for c in lat)
    assert all(cc.operands(c, "lattice")["act"] == 0 for c in lat)
    assert len(set(cc.SHAPES)) == len(cc.SHAPES)


@pytest.mark.parametrize("item", ITEMS, ids=_id)
def test_restatement_against_fp64(item):
    """The restatement of the case's class is the fused layer: its worst plane is at rounding level, and four times it fits under
    the class's existing bar, so that no device bar is ever clamped below 4 r32."""
    case, regime = item
    p = cc.prepared(case, regime)
    cls = cc.klass(case)
    assert (p["S"] >= p["ref"].abs() * (1 - 1e-12)).all()                        # the figure's denominator bounds the result
    assert torch.isfinite(p["e32"]).all()
    fig, b, n = cc.worst_plane(p["e32"])
    print(f"{_id(item)}: r32 {fig:.2e} (image {b}, channel {n}); global {cc.global_error(p['y32'], p['ref']):.2e}; bar {p['bar']:.2e}")
    assert 4 * p["r32"] <= cc.CAP[cls], (fig, b, n)
    assert p["bar"] <= cc.CAP[cls] and p["bar"] >= cc.FLOOR[cls]
    if regime == "lattice":
        assert torch.equal(p["y32"].double(), p["ref"])                          # exact arithmetic: the restatement too


def test_floors():
    """FLOOR[class] is 4 x the worst iid plane figure of the class's restatement over all shapes, within the factor 1.5 by which that
    extreme value moves with the CPU's summation order (conv_cases.FLOOR)."""
    worst = {}
    for case, regime in ITEMS:
        if regime == "iid":
            cls = cc.klass(case)
            worst[cls] = max(worst.get(cls, 0.0), cc.prepared(case, regime)["r32"])
    for cls, r32 in worst.items():
        print(f"{cls}: worst iid r32 {r32:.3e}, 4 x = {4 * r32:.3e}, FLOOR {cc.FLOOR[cls]:.3e}, CAP {cc.CAP[cls]:.0e}")
        assert cc.FLOOR[cls] / 1.5 <= 4 * r32 <= 1.5 * cc.FLOOR[cls], (cls, r32)
        assert cc.FLOOR[cls] < cc.CAP[cls]


def _quiet_image_case(cfg, gn):
    return next(c for c in cc.SHAPES if c.cfg == cfg and c.gn == gn and c.temb and c.res and c.B >= 2)


def test_plane_error_sees_a_swapped_temb_row():
    """The fault of the issue: image 0's planes computed with image 1's temb row, under quiet_image, planted in the restatement's
    output.  Every plane of image 0 is far beyond its bar and no plane of image 1 moves.  (temb is of unit scale in every image, so
    this fault is loud enough for the global figure as well; the faults the global figure misses are the next test's.)"""
    for case in (_quiet_image_case(4, False), _quiet_image_case(3, True)):
        p = cc.prepared(case, "quiet_image")
        temb = p["o"]["temb"]
        bad = p["y32"].clone()
        bad[0] += (temb[1] - temb[0])[:, None, None]
        e = cc.plane_error(bad, p["ref"], p["S"])
        print(f"{case.cfg}: worst plane {e.max().item():.2e}, image 0 min {e[0].min().item():.2e}, bar {p['bar']:.2e}, "
              f"global {cc.global_error(bad, p['ref']):.2e}")
        moved = (temb[1] - temb[0]).abs() > 1e-3
        assert (e[0][moved] > 100 * p["bar"]).all()
        assert torch.equal(e[1:], p["e32"][1:])


def test_plane_error_sees_what_the_global_figure_misses():
    """Faults planted in the restatement's output that the figure of tests/test_gpu_ops.py passes at its bar and the plane figure
    does not: the contraction of the quiet image of a plain launch off by 1 %; the contraction under a loud residual off by 1 %; the
    contraction of the quiet output channels off by 1 %."""
    def both(p, bad, cls):
        return cc.global_error(bad, p["ref"]), cc.plane_error(bad, p["ref"], p["S"])

    plain = _quiet_image_case(4, False)                                          # streaming 1x1 with temb and residual
    p = cc.prepared(plain, "quiet_image")
    o = p["o"]
    conv0 = p["y32"][0] - o["bias"][:, None, None] - o["temb"][0][:, None, None] - o["res"][0]
    bad = p["y32"].clone()
    bad[0] += 0.01 * conv0
    g, e = both(p, bad, "direct")
    print(f"quiet_image, contraction 1 % off: global {g:.2e} (bar {cc.TOL:.0e}), image 0 planes {e[0].min().item():.2e} ... "
          f"{e[0].max().item():.2e} (bar {p['bar']:.2e})")
    assert g < cc.TOL and (e[0] > 4 * p["bar"]).all() and torch.equal(e[1:], p["e32"][1:])

    wino = _quiet_image_case(3, True)                                            # F(4x4,3x3) ResBlock conv over a concat
    p = cc.prepared(wino, "loud_residual")
    o = p["o"]
    conv = p["y32"] - o["bias"][None, :, None, None] - o["temb"][:, :, None, None] - o["res"]
    g, e = both(p, p["y32"] + 0.01 * conv, "wino43")
    print(f"loud_residual, contraction 1 % off: global {g:.2e} (bar 1e-4), worst plane {e.max().item():.2e}, least {e.min().item():.2e} "
          f"(bar {p['bar']:.2e})")
    assert g < cc.CAP["wino43"] and (e > 4 * p["bar"]).all()

    up = next(c for c in cc.SHAPES if c.cfg == 3 and c.a_mode == 1)                # F(4x4,3x3), nearest x2, no temb, no residue
    p = cc.prepared(up, "quiet_channels")
    quiet = torch.arange(up.N) % 4 == 1
    bad = p["y32"].clone()
    bad[:, quiet] += 0.01 * (p["y32"][:, quiet] - p["o"]["bias"][quiet][None, :, None, None])
    g, e = both(p, bad, "wino43")
    print(f"quiet_channels, their contraction 1 % off: global {g:.2e} (bar 1e-4), planes {e[:, quiet].min().item():.2e} ... "
          f"{e[:, quiet].max().item():.2e} (bar {p['bar']:.2e})")
    assert g < cc.CAP["wino43"] and (e[:, quiet] > 10 * p["bar"]).all() and torch.equal(e[:, ~quiet], p["e32"][:, ~quiet])


@pytest.mark.parametrize("case", LATTICE, ids=lambda c: cc.case_id((c, "lattice", 0)))
def test_lattice_bound(case):
    """Below 2^24 lattice steps at every intermediate and output of the absolute-value pipeline, fp32 arithmetic is exact in any
    order; the packed Winograd weights are exact; the statistics rows' sums are exact."""
    p = cc.prepared(case, "lattice")
    o, cls = p["o"], cc.klass(case)
    for name in ("x", "bias", "temb", "res", "scale", "shift"):
        if o[name] is not None:
            assert torch.equal(o[name], o[name].round()), name
    assert set(o["x"].unique().tolist()) <= {-1.0, 0.0, 1.0} and (o["x"] != 0).any()
    if case.gn:
        assert set(o["scale"].unique().tolist()) == {1.0, 2.0} and (o["shift"] != 0).any()
        assert not torch.equal(o["scale"][0], o["scale"][1])
    t = o["w"] * (8.0 / 9.0 if cls == "wino43" else 1.0)
    assert torch.equal(t, t.round()) and (t != 0).any()
    if cls != "direct":
        import hipops
        G = (hipops._WINO43_G if cls == "wino43" else hipops._WINO_G).double()
        exact = torch.einsum("ua,oiab,vb->uvio", G, o["w"].double(), G)
        U = cc.transformed_weights(o["w"], cls).double()
        steps = U / cc.LATTICE_STEP[cls]
        if cls == "wino23":                                                     # G holds 1 and 1/2: the fp64 pack is exact
            assert torch.equal(steps, steps.round()) and torch.equal(U, exact)
        else:                                                                   # exact but for the residue in entries whose value is 0
            on = steps.round() * cc.LATTICE_STEP[cls]
            assert torch.equal(U[on != 0], on[on != 0]) and (U[on == 0].abs() <= cc.residue_weights(o["w"])[on == 0]).all()
            assert steps.abs().max() < 2 ** 16                                  # small numerators: exact in fp32
    residue = cc.lattice_residue(case, o)
    assert residue < 2.0 ** -36 and (cls == "wino43" or residue == 0.0)          # half an ulp of one lattice step: 2^-34
    assert cc.lattice_mismatch(p["y32"], p["ref"], residue) is None
    off = p["y32"].clone()
    i = p["ref"].abs().argmax()
    off.view(-1)[i] = torch.nextafter(off.view(-1)[i], torch.tensor(float("inf")))          # one ulp is a mismatch
    assert cc.lattice_mismatch(off, p["ref"], residue) is not None
    bound = cc.lattice_bound(case, o)
    stats = cc.lattice_stats_bound(case, p["ref"])
    print(f"{cc.case_id((case, 'lattice', 0))}: pipeline 2^{torch.tensor(bound).log2().item():.1f} steps, statistics 2^{torch.tensor(stats).log2().item():.1f}; "
          f"max |ref| {p['ref'].abs().max().item():.1f}, non-zero outputs {(p['ref'] != 0).double().mean().item():.2f}")
    assert bound < 2 ** 24 and stats < 2 ** 24
    assert (p["ref"] != 0).double().mean() > 0.5                                 # not a test of zeros
