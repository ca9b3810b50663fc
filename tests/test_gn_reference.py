"""CPU pin of tests/gn_cases.py: the operand recipe reaches its levels, fp32 F.group_norm stays at least 4x inside every bar (the
reference alone never fails a case), the fused statistics scheme -- fp32 rows of 256 addends, fp64 fold, var = Q / n - mean^2 --
stays inside every bar in both extreme summation orders (if a later change of row length breaks this, the design fails and not only
an implementation), and the conditioning number r = |mean| / sqrt(var + eps) that the workload's structured inputs reach in the
GroupNorms of the UNet stays inside the envelope the bars were chosen for."""
import pytest
import torch
import torch.nn.functional as F

import gn_cases as gc

B, C, H = 2, 128, 32


@pytest.fixture(scope="module")
def operands():
    out = {}
    for name in gc.CASES:
        x = gc.operand(name, B, C, H, H)
        gamma, beta = gc.affine(C)
        out[name] = (x, gamma, beta, gc.reference(x, gamma, beta))
    return out


@pytest.mark.parametrize("name", list(gc.CASES))
def test_cases_reach_their_level(name):
    kind, level, regime = gc.CASES[name]
    nominal = 0.0 if level == "const" else float(level)
    for (Bc, Cc, Hc) in ((2, 64, 32), (3, 128, 16), (2, 384, 8)):
        r = gc.achieved_r(gc.operand(name, Bc, Cc, Hc, Hc))
        assert (r >= nominal).all(), (name, r.min().item())
        if kind == "level":
            assert (r <= 1.1 * nominal + 0.5).all(), (name, r.max().item())            # and not far beyond it
            m, _ = gc.moments(gc.operand(name, Bc, Cc, Hc, Hc))
            assert level == 0 or ((m[:, 0::2] > 0).all() and (m[:, 1::2] < 0).all())       # signs alternate between groups
            assert level == 0 or ((m[1] / m[0]).abs() > 1.015).all()                        # every image has means of its own
        if kind == "const1":
            assert (r > 316).all()
        if kind == "group_const":
            assert (r[:, gc.CONST_GROUP] > 316).all()
        if kind == "blank_image":
            assert (r[0] > 316).all() and (r[1:] < 1.01).all()
    # the same case as the output of a convolution (3x3 and 1x1) and of the stem
    for ks in (3, 1):
        x, w, b, temb = gc.conv_operand(name, 2, 32, 64, 32, ks)
        y = F.conv2d(x.double(), w.double(), b.double(), padding=ks // 2) + temb.double()[:, :, None, None]
        assert (gc.achieved_r(y.float()) >= nominal).all(), (name, ks)
    x, w, b = gc.stem_operand(name, 2, 64, 32)
    assert (gc.achieved_r(F.conv2d(x.double(), w.double(), b.double(), padding=1).float()) >= nominal).all(), name


def test_bars_are_the_projects_own():
    assert gc.BARS == {0: 2e-5, 4: 2e-5, 16: 5e-5, 64: 1e-3, "const": 1e-3}
    b = gc.bars("group_const", 2)
    assert b[0, gc.CONST_GROUP] == 1e-3 and b[0, 0] == 2e-5
    b = gc.bars("blank_image", 3)
    assert (b[0] == 1e-3).all() and (b[1:] == 2e-5).all()


def test_error_is_per_image_and_per_group():
    ref = torch.ones(2, 64, 4, 4, dtype=torch.float64)
    ref[1] *= 100.0
    got = ref.clone()
    got[0, 5, 1, 1] += 0.5                                     # channel 5 = group 2 of image 0: not hidden by image 1's magnitude
    e = gc.error(got, ref)
    assert e.shape == (2, 32) and e[0, 2] == 0.5 and e.sum() == 0.5
    got[1, 0, 0, 0] = float("nan")
    assert gc.error(got, ref)[1, 0] == float("inf")


@pytest.mark.parametrize("name", list(gc.CASES))
def test_fp32_group_norm_stays_4x_inside_the_bar(name, operands):
    x, gamma, beta, ref = operands[name]
    got = F.group_norm(x, gc.GROUPS, gamma, beta, eps=gc.EPS)
    ratio = (gc.error(got, ref) / gc.bars(name, B)).max().item()
    print(f"{name}: fp32 F.group_norm at {ratio:.3f} of the bar")
    assert ratio < 0.25, (name, ratio)
    if name == "zeros":
        assert torch.equal(got, beta[None, :, None, None].expand_as(got))


@pytest.mark.parametrize("order", ["pairwise", "sequential"])
@pytest.mark.parametrize("name", list(gc.CASES))
def test_fused_statement_stays_inside_the_bar(name, order, operands):
    x, gamma, beta, ref = operands[name]
    y, mean, rstd = gc.fused_statement(x, gamma, beta, row_pixels=256, order=order)
    fails = []
    gc.failures(f"fused statement, 256-pixel rows, {order}", name, y, ref, fails)
    gc.failures(f"  its mean / rstd, {order}", name, gc.normalised(x, mean, rstd, gamma, beta), ref, fails)
    assert torch.isfinite(y).all() and not fails, fails
    if name == "zeros":
        assert torch.equal(y, beta[None, :, None, None].expand_as(y))


def test_fused_statement_counts_a_ragged_last_row():
    x = gc.operand("r4_unit", 2, 64, 20, 20)                  # 400 pixels: one full row of 256 and one of 144
    gamma, beta = gc.affine(64)
    for order in ("pairwise", "sequential"):
        y, _, _ = gc.fused_statement(x, gamma, beta, 256, order)
        assert (gc.error(y, gc.reference(x, gamma, beta)) < 2e-5).all()


def test_structured_inputs():
    x, t = gc.structured_batch(64)
    assert x.shape == (4, 1, 64, 64) and t.tolist() == [0, 100, 250, 999]
    assert (x[0] == -1).all() and x.abs().max() <= 4.0
    bg = (x[1] == -1).float().mean().item()
    assert 0.3 < bg < 0.8 and x[1].max() > 0.5, bg                    # a phantom that is mostly background
    assert (x[2] - x[1]).std() > 0.3 and (x[3].abs() <= 1).all()


ENVELOPE_MODELS = {
    "i64_b32_hc32": dict(img_size=64, base_channels=32, n_head_channels=32, attention_resolutions="16,8"),
    "i64_b128_h2": dict(img_size=64, base_channels=128, n_heads=2, attention_resolutions="16,8"),
}


@pytest.mark.parametrize("model", list(ENVELOPE_MODELS))
def test_envelope_of_the_workload(model, monkeypatch):
    """r of every GroupNorm of the UNet (fp64 statistics, t = 250, deterministic weights) for a blank slice, a phantom, the
    phantom noised as at t = 250 and a uniform image: the worst is what the r = 16 level stands for."""
    from oracle import unet_oracle as uo
    kw = ENVELOPE_MODELS[model]
    shapes = uo.param_shapes(kw["img_size"], kw["base_channels"], "", 2, kw["attention_resolutions"], 1)
    sd = uo.fill_deterministic(shapes)
    log = []
    real = uo._gn

    def gn(sd_, p, x):
        log.append((p, gc.achieved_r(x.reshape(x.shape[0], x.shape[1], -1, 1)).amax(1)))
        return real(sd_, p, x)
    monkeypatch.setattr(uo, "_gn", gn)
    x, _ = gc.structured_batch(64)
    uo.forward(sd, x, torch.full((4,), 250), **kw)
    assert len(log) == sum(1 for k in shapes if k.endswith((".in_layers.0.weight", ".out_layers.0.weight", ".norm.weight", "out.0.weight")))
    names = ["blank", "phantom", "phantom at t = 250", "uniform"]
    worst = {}
    for i, nm in enumerate(names):
        r, p = max((float(rr[i]), p) for p, rr in log)
        worst[nm] = r
        print(f"{model}: {nm:20s} worst r {r:6.2f} at {p}")
    assert max(worst.values()) <= 16.0, worst
    if model == "i64_b32_hc32":
        assert worst["blank"] > 8.0, worst                   # the case that motivates the r = 16 level must stay a real one
