"""CPU pin of tests/attn_cases.py: the regimes deliver the logits they claim (standard deviation, a uniform P, row maxima beyond
the fp32 overflow point of exp), the packed layout is the one QKVAttentionLegacy reads, the fp32 restatement alone stays inside the
caps for every case of tests/test_gpu_attention.py (4 r32 <= 1.5e-4 forward, 2.5e-7 per row backward: the reference alone never
fails a case), and restatements with a planted defect fail the bars on the regimes that are there to catch them."""
import math

import pytest
import torch

import attn_cases as ac

FORWARD_CASES = ac.fused_cases() + [c for c in ac.launch3_cases() if c not in ac.fused_cases()]
FORWARD_SHAPES = tuple(dict.fromkeys(s for r, s in FORWARD_CASES if r != "mixed"))
SMALL = (1, 2, 48, 64)


def fails(P, out, regime, shape):
    """Whether a restated (P, out) misses a forward bar of the case, and whether it is finite."""
    c = ac.forward_case(regime, shape)
    bad = bool((ac.slab_error(P, c["P"]) >= c["bar_P"]).any() or (ac.slab_error(out, c["out"]) >= c["bar_out"]).any())
    return bad, bool(torch.isfinite(P).all() and torch.isfinite(out).all())


# ---------------------------------------------------------------------------------------------------- the regimes
@pytest.mark.parametrize("shape", FORWARD_SHAPES, ids=str)
def test_regimes_deliver_what_they_claim(shape):
    L = shape[2]
    for regime in ac.REGIMES:
        c = ac.forward_case(regime, shape)
        S = ac.logits(c["q"], c["k"])
        rowmax = S.amax(-1)
        pmax = c["P"].amax(-1)
        print(f"{str(shape):20s} {regime:10s} std {S.std().item():6.2f}  |S|max {S.abs().max().item():6.1f}  row max >= {rowmax.min().item():6.1f}  "
              f"median P_max {pmax.median().item():.3f}")
        if regime.startswith("sigma"):
            assert abs(S.std().item() / ac.LEVELS[regime] - 1) < 0.15, (regime, S.std().item())
        if regime == "uniform":
            assert ((c["P"] * L - 1).abs() <= 1e-7).all()
        if regime == "match8":
            assert 0.5 < pmax.median().item() < 0.99                                   # peaked, not one-hot
        if regime == "match100":
            assert (rowmax > ac.EXP_OVERFLOW).all(), rowmax.min().item()
            assert (c["P"].float().amax(-1) == 1.0).all()                               # one-hot to fp32 ...
            assert ((c["P"].float() != 0).sum(-1) > 1).any()                            # ... with a tail that is tiny, not 0
        if regime == "offset100":
            assert (rowmax > ac.EXP_OVERFLOW).double().mean().item() >= 0.9
            assert S.mean().item() > 90 and 0.15 < pmax.median().item() < 0.85           # a common offset, not a peak
    assert ac.LEVELS["sigma32"] == max(v for k, v in ac.LEVELS.items() if k.startswith("sigma"))
    assert (ac.forward_case("sigma32", shape)["P"].amax(-1) > 0.99).double().mean().item() > 0.5      # rows mostly one-hot


def test_mixed_has_six_different_regimes():
    assert len(set(ac.MIXED)) == 6 and set(ac.MIXED) <= set(ac.REGIMES)
    assert {"match100", "offset100", "uniform"} <= set(ac.MIXED)
    for shape in ac.MIXED_SHAPES:
        assert shape[:2] == (2, 3) and shape[2:] in {s[2:] for s in ac.FUSED_SHAPES}
        S = ac.logits(*ac.operand("mixed", *shape)[:2]).flatten(0, 1)
        assert (S[ac.MIXED.index("uniform")] == 0).all() and S[ac.MIXED.index("offset100")].min() > 60
        assert (S[ac.MIXED.index("match100")].amax(-1) > ac.EXP_OVERFLOW).all()


def test_the_cases_reach_the_paths_of_the_fused_kernel():
    tiles = {(s[2] // 16, s[3]) for s in ac.FUSED_SHAPES}
    assert {n for n, ch in tiles if ch < 512} >= {1, 3, 9, 17, 25, 64}          # double-buffered loop: second, third, fourth tile of wave 0
    assert {n for n, ch in tiles if ch == 512} >= {9, 17}                        # ch 512: one and two reloads
    assert any(s[0] > 1 and s[1] > 2 for s in ac.FUSED_SHAPES)                   # more than two heads and more than one image
    assert any(s[3] & (s[3] - 1) for s in ac.LAUNCH3_SHAPES)                     # a head width only the three-launch form takes
    assert all(s[2] % 16 == 0 and 16 <= s[2] <= 1024 for s in ac.FUSED_SHAPES)


def test_packed_layout_is_the_legacy_order():
    """pack_qkv against the expression of UNet.py:146-150 on the [B, 3 C, L] tensor the block's 1x1 convolution writes."""
    B, heads, L, ch = 2, 3, 16, 16
    q, k, v = ac.operand("sigma1", B, heads, L, ch)
    qkv = ac.pack_qkv(q, k, v).permute(0, 2, 1).double()                         # [B, 3 C, L]
    ql, kl, vl = qkv.reshape(B * heads, 3 * ch, L).split(ch, dim=1)
    s = 1 / math.sqrt(math.sqrt(ch))
    w = torch.softmax(torch.einsum("bct,bcs->bts", ql * s, kl * s), dim=-1)
    a = torch.einsum("bts,bcs->bct", w, vl).reshape(B, heads * ch, L)
    P, out = ac.forward_reference(q, k, v)
    assert torch.allclose(w.reshape(B, heads, L, L), P, rtol=0, atol=1e-14)
    assert torch.allclose(ac.unpack_out(a.permute(0, 2, 1), heads), out, rtol=0, atol=1e-13)


def test_forward_figure_is_per_slab():
    ref = torch.ones(1, 2, 4, 4, dtype=torch.float64)
    ref[0, 1] *= 1e-3                                                            # a quiet slab beside a loud one
    got = ref.clone()
    got[0, 1, 2, 3] += 1e-6
    e = ac.slab_error(got, ref)
    assert e[0, 0] == 0 and abs(e[0, 1].item() - 1e-3) < 1e-9
    got[0, 0, 0, 0] = float("nan")
    assert ac.slab_error(got, ref)[0, 0] == float("inf")


# ---------------------------------------------------------------------------------------------------- the caps
def test_restatement_stays_inside_the_forward_cap():
    worst = {}
    for regime, shape in FORWARD_CASES:
        c = ac.forward_case(regime, shape)
        for what in ("r32_P", "r32_out"):
            r = c[what].max().item()
            worst[regime] = max(worst.get(regime, 0.0), r)
            assert 4 * r <= ac.CAP, (regime, shape, what, r)
            assert (c["bar_" + what[4:]] <= ac.CAP).all() and (c["bar_" + what[4:]] >= ac.TOL).all()
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert ac.CAP == 1.5e-4 and ac.TOL == 2e-5


def test_restatement_stays_inside_the_backward_cap():
    worst = {}
    for regime, shape in ac.backward_cases():
        c = ac.backward_case(regime, shape)
        worst[regime] = max(worst.get(regime, 0.0), c["r32"].max().item())
        assert c["r32"].max().item() <= ac.BWD_R32_CAP, (regime, shape, c["r32"].max().item())
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert ac.BWD_BAR == 1e-6 and ac.BWD_R32_CAP == 2.5e-7
    # a P that is one-hot bit for bit has dS == 0 exactly, in fp32 as in fp64
    c = ac.backward_case("match100", ac.BWD_SHAPES[1])
    hot = ac.one_hot(c["P"])
    assert (hot.sum(-1) == 1).all() and ((hot == 0) | (hot == 1)).all() and torch.equal(hot.argmax(-1), c["P"].argmax(-1))
    assert not ac.backward_reference(hot, c["dP"]).any() and not ac.backward_fp32(hot, c["dP"]).any()


# ---------------------------------------------------------------------------------------------------- planted defects
def test_defect_no_max_subtraction():
    for regime in ("match100", "offset100"):
        for shape in (SMALL, (1, 1, 272, 128)):
            c = ac.forward_case(regime, shape)
            e = torch.exp((c["q"] @ c["k"].transpose(-1, -2)) / math.sqrt(shape[3]))
            P = e / e.sum(-1, keepdim=True)
            bad, finite = fails(P, P @ c["v"], regime, shape)
            assert bad and not finite, (regime, shape)


def test_defect_alpha_applied_once():
    for regime in ("sigma1", "sigma8", "sigma32"):
        for shape in ((2, 3, 16, 16), SMALL):
            c = ac.forward_case(regime, shape)
            P = torch.softmax((c["q"] @ c["k"].transpose(-1, -2)) * shape[3] ** -0.25, dim=-1)
            assert fails(P, P @ c["v"], regime, shape) == (True, True), (regime, shape)


def test_defect_neighbour_heads_v():
    for shape in ac.MIXED_SHAPES:
        c = ac.forward_case("mixed", shape)
        for slab in range(6):
            b, h = divmod(slab, 3)
            v = c["v"].clone()
            v[b, h] = c["v"][b, (h + 1) % 3]
            P, out = ac.forward_fp32(c["q"], c["k"], v)
            e = ac.slab_error(out, c["out"])
            assert e[b, h] >= c["bar_out"][b, h] and (e.flatten() < c["bar_out"].flatten()).sum() == 5, (shape, slab)
            assert (ac.slab_error(P, c["P"]) < c["bar_P"]).all()


def test_defect_swapped_key_columns():
    for shape in ((2, 3, 16, 16), SMALL, (1, 2, 1024, 64)):
        c = ac.forward_case("sigma1", shape)
        P, out = ac.forward_fp32(c["q"], c["k"], c["v"])
        assert fails(P, out, "sigma1", shape) == (False, True)
        j = shape[2] - 2
        P[..., [j, j + 1]] = P[..., [j + 1, j]]
        assert fails(P, out, "sigma1", shape) == (True, True), shape           # P alone gives it away
        assert fails(c["P"].float(), P @ c["v"], "sigma1", shape) == (True, True), shape      # and so does out


def test_defect_backward_dot_over_64_columns():
    for regime, shape in ac.backward_cases():
        c = ac.backward_case(regime, shape)
        P, dP = c["P"], c["dP"]
        got = P * (dP - (P[..., :64] * dP[..., :64]).sum(-1, keepdim=True))
        bad = bool((ac.row_error(got, c["dS"], P, dP) >= ac.BWD_BAR).any())
        assert bad == (shape[1] > 64), (regime, shape)


def test_defect_backward_another_rows_dot():
    for regime in ("uniform", "match8"):
        for shape in ac.BWD_SHAPES:
            c = ac.backward_case(regime, shape)
            P, dP = c["P"], c["dP"]
            got = P * (dP - (P * dP).sum(-1, keepdim=True).roll(1, dims=-2))
            assert (ac.row_error(got, c["dS"], P, dP) >= ac.BWD_BAR).any(), (regime, shape)
