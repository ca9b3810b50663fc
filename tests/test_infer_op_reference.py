"""CPU: the statements, restatements and bars of tests/infer_op_cases.py, which tests/test_gpu_infer_op_elements.py holds the small
inference kernels to.  Each fp64 statement against stock fp64 torch.nn.functional (F.linear, F.conv2d(padding=1),
conv2d(silu(x * scale + shift)), F.interpolate, F.avg_pool2d, slicing, torch.softmax, permute; posemb against forward_ledger.posemb);
the fp32 restatement against fp64 on every (case, regime), 4 r32 <= CAP on every one; the FLOOR constants against their measurement;
and the figure on five planted defects (the suite bites).

The planted defects, each put into a correct fp32 restatement, each failing the bar its case gets (printed: figure / bar, and the
figure of tests/test_gpu_ops.py -- max |err| / max |ref| over the whole tensor -- on the same defective tensor):
  border     one border pixel of the quiet image, in a quiet output channel, computed with the zero padding omitted (the edge
             replicated).  On that tensor the old figure is under TOL: the new one sees what the old one does not.  In an iid square
             case nothing is quiet, the wrong pixel is as large as its neighbours and the old figure is beyond TOL too: that second
             check does not hold and is not made.
  nan        one element left NaN.  The old figure turns NaN and `NaN < TOL` is false: it does not pass there either, on any case;
             the second check is not made.  What is new here is that every element is looked at with guards behind the buffer.
  swap       H and W swapped in the index of a non-square map.  On a square map the defect is the identity: the second check holds
             trivially, and no map of test_gpu_ops.py is anything but square.
  row16      row 16 of a B = 17 linear computed from row 15 (the first row of the second launch).  test_gpu_ops.py has no B > 16;
             on its shapes the defect changes nothing, and on an iid B = 17 case the old figure is beyond TOL: not made.
  strip      one strip's statistics counted in the neighbouring row.  The figure of test_stem_fused_groupnorm_sums is this one
             (relative to the sum of |.|) and sees it as well: not made."""
import pytest
import torch
import torch.nn.functional as F

import infer_op_cases as ic

ITEMS = [item for op in ic.OPS for item in ic.cases(op)]


def _items(op, regime=None):
    return [it for it in ic.cases(op) if regime is None or it[2] == regime]


def test_case_lists_reach_every_branch():
    B, K, N = ({s[i] for s in ic.LINEAR} for i in range(3))
    assert B == {1, 3, 4, 5, 8, 9, 16, 17, 33} and K == {4, 36, 64, 68, 200, 260} and N == {1, 3, 4, 5, 17, 33}
    assert {s[:2] for s in ic.LINEAR} >= {(b, k) for b in (16, 17, 33) for k in (36, 68, 200, 260)}
    assert {s[3:5] for s in ic.LINEAR} == {(0, 0), (0, 1), (1, 0), (1, 1)} and sum(1 for s in ic.LINEAR if not s[5]) >= 3
    assert 20 <= len(ic.LINEAR) <= 28
    assert {s[0] for s in ic.POSEMB} == {1, 5, 300} and {s[1] for s in ic.POSEMB} == {2, 6, 32, 130}
    assert {s[2] for s in ic.POSEMB} == {1.0, 0.25} and {s[3] for s in ic.POSEMB} == {0, 1, 7, 2 * 256 * 512 + 3}
    assert max(s[0] * s[1] // 2 for s in ic.POSEMB) > 256
    plain = {s[:5] for s in ic.STEM if s[5:] == (0, 0, 0)}
    assert plain == {(1, 1, 8, 1, 4), (3, 5, 24, 1, 32), (1, 8, 16, 2, 12), (3, 10, 16, 1, 96), (1, 64, 64, 1, 1024), (2, 7, 12, 1, 32),
                     (1, 9, 16, 3, 32), (2, 6, 8, 16, 12)}
    assert (1, 8, 16, 1, 32, 0, 1, 0) in ic.STEM and (1, 64, 64, 1, 1024, 0, 0, 1) in ic.STEM
    assert {s[:6] for s in ic.STEM if s[5]} == {(2, 16, 32, 1, 32, -1), (1, 10, 16, 2, 96, -1), (1, 16, 32, 1, 32, 1), (2, 16, 32, 2, 32, 1),
                                                (2, 32, 32, 1, 32, 1), (1, 20, 16, 1, 96, 1)}
    # workgroup trips of the statistics cases: per image H * W / 8 strips over rows x (256 / (Cout / 4)) strips per trip
    trips = {s[:5]: s[1] * s[2] // 8 // (ic.stem_rows(s) * (256 // (s[4] // 4))) for s in ic.STEM if s[5]}
    assert trips == {(2, 16, 32, 1, 32): 1, (1, 10, 16, 2, 96): 1, (1, 16, 32, 1, 32): 2, (2, 16, 32, 2, 32): 2, (2, 32, 32, 1, 32): 4,
                     (1, 20, 16, 1, 96): 4}
    assert {s[:5] for s in ic.HEAD if not s[5]} == {
        (1, 8, 8, 128, 1), (3, 8, 40, 64, 1), (1, 40, 8, 128, 1), (2, 32, 16, 128, 1), (1, 24, 72, 64, 3), (2, 16, 16, 128, 4), (1, 16, 24, 256, 1),
        (1, 8, 40, 256, 3), (3, 16, 16, 32, 2), (1, 24, 8, 160, 4), (2, 8, 16, 96, 1), (1, 16, 8, 48, 2), (3, 8, 8, 4, 1), (1, 8, 24, 80, 4)}
    assert {(s[:5], s[5]) for s in ic.HEAD if s[5]} == {((2, 32, 16, 128, 1), 1), ((2, 32, 16, 128, 1), 2), ((2, 32, 16, 128, 1), 3),
                                                         ((1, 24, 72, 64, 3), 1), ((1, 24, 72, 64, 3), 2)}
    assert set(ic.RESAMPLE) == {(m, 3, h, w, C) for m in (1, 2, 3, 4) for h, w in ((3, 5), (1, 7), (8, 2)) for C in (4, 12, 96)}
    assert set(ic.SOFTMAX) == {(r, L) for r in (1, 2, 5, 7, 64) for L in (1, 16, 63, 64, 65, 100, 256)}
    assert {s[:4] for s in ic.LAYOUT} == {(1, 1, 1, 1), (3, 7, 5, 5), (2, 300, 3, 8), (1, 64, 4, 128), (1, 699051, 3, 3)}
    assert 699051 * 3 == 8192 * 256 + 1
    for op in ic.OPS:
        assert len(set(ic.SHAPES[op])) == len(ic.SHAPES[op])
    regimes = {op: {r for _, _, r in ic.cases(op)} for op in ic.OPS}
    assert regimes["linear"] == {"iid", "quiet_row", "saturated"} and regimes["softmax"] == {"iid", "quiet_row", "peaked"}
    assert regimes["head"] == {"iid", "quiet_row", "saturated"} and regimes["stem"] == {"iid", "quiet_row"}
    assert {it[2] for it in ic.cases("resample") if it[1][0] == 2} == {"iid", "quiet_row", "saturated"}
    # every shape of the softmax sees every kind of peaked row, except where it has fewer than five rows
    for L in (1, 16, 63, 64, 65, 100, 256):
        assert {ic.peaked_kind((r, L), i) for r in (1, 2, 5, 7, 64) for i in range(r)} == set(ic.PEAKED)
    x = ic.prepared("softmax", (64, 100), "peaked")["o"]["x"]
    assert torch.isinf(x).any() and not torch.isinf(x).all(1).any() and x.max() > 9e3 and (x == 500).any()


@pytest.mark.parametrize("item", ITEMS, ids=ic.case_id)
def test_restatement_against_fp64(item):
    """The fp32 restatement is the statement: its worst row is at rounding level, four times it fits under the kernel's existing
    bar (so no device bar is clamped below 4 r32), and it passes its own bar; the bit-for-bit outputs are exact in fp64 too."""
    p = ic.prepared(*item)
    for name, out in p["outs"].items():
        assert (out.S >= out.ref.abs() * (1 - 1e-12)).all(), name                # the figure's denominator bounds the result
        if out.cls == "exact":
            # a copy is exact in either precision; the mean of four rounds three sums, each within 2^-24 of the sum of |.|
            assert out.y.dtype == torch.float32 and ((out.y.double() - out.ref).abs() <= 2.0 ** -22 * out.S).all(), name
            assert item[0] == "resample" and item[1][0] == 2 or torch.equal(out.y.double(), out.ref), name
            continue
        e = ic.row_error(out.y, out.ref, out.S)
        assert torch.isfinite(e).all() and (e <= p["bar"][out.cls]).all(), (name, ic.worst_row(e))
    for cls, r32 in p["r32"].items():
        print(f"{ic.case_id(item)}: {cls} r32 {r32:.2e}, bar {p['bar'][cls]:.2e}")
        assert 4 * r32 <= ic.CAP[cls], (cls, r32)
        assert ic.FLOOR[cls] <= p["bar"][cls] <= ic.CAP[cls]


def test_floors():
    """FLOOR[class] is 4 x the worst iid row figure of the class's restatement over all its shapes, within a factor 1.5."""
    worst, by_regime = {}, {}
    for item in ITEMS:
        for cls, r32 in ic.prepared(*item)["r32"].items():
            print(f"{ic.case_id(item)}: {cls} r32 {r32:.3e}")
            by_regime[cls, item[2]] = max(by_regime.get((cls, item[2]), (-1.0, "")), (r32, ic.case_id(item)))
            if item[2] == "iid":
                worst[cls] = max(worst.get(cls, (-1.0, "")), (r32, ic.case_id(item)))
    assert set(worst) == set(ic.FLOOR) == set(ic.CAP)
    for (cls, regime), (r32, where) in sorted(by_regime.items()):
        print(f"{cls} {regime}: worst r32 {r32:.3e} ({where})")
    for cls, (r32, where) in sorted(worst.items()):
        print(f"{cls}: worst iid r32 {r32:.3e} ({where}), 4 x = {4 * r32:.3e}, FLOOR {ic.FLOOR[cls]:.3e}, CAP {ic.CAP[cls]:.0e}")
    for cls, (r32, where) in worst.items():
        assert ic.FLOOR[cls] / 1.5 <= 4 * r32 <= 1.5 * ic.FLOOR[cls], (cls, r32, where)
        assert ic.FLOOR[cls] < ic.CAP[cls]


# ---------------------------------------------------------------------------------------------------- statements against stock torch
def _close(name, got, want, S):
    assert got.shape == want.shape, name
    assert (got - want).abs().max() <= 1e-12 * S.abs().max().clamp_min(1e-300), name


@pytest.mark.parametrize("item", _items("linear", "iid") + _items("linear", "saturated")[:6], ids=ic.case_id)
def test_linear_statement_is_f_linear(item):
    p = ic.prepared(*item)
    o, out = p["o"], p["outs"]["out"]
    x = o["x"].double()
    y = F.linear(F.silu(x) if o["act_in"] else x, o["w"].double(), None if o["bias"] is None else o["bias"].double())
    _close("out", out.ref, F.silu(y) if o["act_out"] else y, out.S)


@pytest.mark.parametrize("item", _items("posemb"), ids=ic.case_id)
def test_posemb_statement_is_the_ledgers(item):
    import forward_ledger
    p = ic.prepared(*item)
    o, out = p["o"], p["outs"]["out"]
    assert torch.equal(out.ref, forward_ledger.posemb(o["t"], o["freqs"], o["dim"], o["scale"]))
    assert o["freqs"].dtype == torch.float32 and o["freqs"][0] == 1 and out.ref.shape == (item[1][0], item[1][1])


@pytest.mark.parametrize("item", _items("stem", "iid") + _items("stem", "quiet_row")[:3], ids=ic.case_id)
def test_stem_statement_is_conv2d(item):
    p = ic.prepared(*item)
    o, outs = p["o"], p["outs"]
    y = F.conv2d(o["x"].double(), o["w"].double(), o["bias"].double(), padding=1)
    _close("out", outs["out"].ref, y.flatten(0, 1), outs["out"].S)
    if o["rows"]:
        B, Cout = y.shape[:2]
        y32 = outs["out"].y.double().view(y.shape)
        per = y32.flatten(2).shape[2] // o["rows"]
        for b in range(B):
            for r in range(o["rows"]):
                chunk = y32[b].flatten(1)[:, r * per:(r + 1) * per]              # NHWC: a contiguous pixel range of one image
                _close("sum", outs["sum"].ref[b * o["rows"] + r], chunk.sum(1), outs["sum"].S)
                _close("sq", outs["sq"].ref[b * o["rows"] + r], (chunk * chunk).sum(1), outs["sq"].S)


@pytest.mark.parametrize("item", _items("head", "iid") + _items("head", "saturated")[:4] + _items("head", "quiet_row")[:3], ids=ic.case_id)
def test_head_statement_is_conv2d_of_silu(item):
    p = ic.prepared(*item)
    o, out = p["o"], p["outs"]["out"]
    x = o["x"].double().permute(0, 3, 1, 2)
    a = F.silu(x * o["scale"].double()[:, :, None, None] + o["shift"].double()[:, :, None, None])
    _close("out", out.ref, F.conv2d(a, o["w"].double(), o["bias"].double(), padding=1).flatten(0, 1), out.S)


@pytest.mark.parametrize("item", _items("resample", "iid") + _items("resample", "saturated"), ids=ic.case_id)
def test_resample_statement_is_interpolate_pool_and_slices(item):
    p = ic.prepared(*item)
    o, outs = p["o"], p["outs"]
    mode = item[1][0]
    x = o["x"].double().permute(0, 3, 1, 2)
    if mode == 1:
        want = F.interpolate(x, scale_factor=2, mode="nearest")
    elif mode == 2:
        want = F.avg_pool2d(x, 2, 2)
        a = F.silu(x * o["scale"].double()[:, :, None, None] + o["shift"].double()[:, :, None, None])
        _close("act", outs["act"].ref, F.avg_pool2d(a, 2, 2).flatten(0, 1), outs["act"].S)
    elif mode == 3:
        want = x[:, :, ::2, ::2]
    else:
        want = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3], dtype=torch.float64)
        want[:, :, ::2, ::2] = x
        lin = x.clone().requires_grad_(True)                                       # the adjoint of the pick
        up = torch.randn(want.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        (lin[:, :, :, :] * up[:, :, ::2, ::2]).sum().backward()
        assert torch.equal(lin.grad, up[:, :, ::2, ::2])
    _close("out", outs["out"].ref, want.permute(0, 2, 3, 1), outs["out"].S)
    if mode == 2 and item[2] == "iid":                                             # the restated order is ATen's, bit for bit
        assert torch.equal(outs["out"].y, F.avg_pool2d(o["x"].permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))


@pytest.mark.parametrize("regime", ["iid", "quiet_row", "peaked"])
def test_softmax_statement_is_torch_softmax(regime):
    for item in _items("softmax", regime):
        p = ic.prepared(*item)
        out = p["outs"]["out"]
        _close(ic.case_id(item), out.ref, torch.softmax(p["o"]["x"].double(), -1), out.S)
        assert torch.isfinite(out.ref).all() and ((out.ref.sum(-1) - 1).abs() < 1e-12).all()


@pytest.mark.parametrize("item", _items("layout"), ids=ic.case_id)
def test_layout_statement_is_permute(item):
    B, P, C, in_ld, c0 = item[1]
    p = ic.prepared(*item)
    want = p["o"]["x"].double().narrow(2, c0, C).permute(0, 2, 1)
    assert p["outs"]["out"].ref.shape == (B, C, P) and torch.equal(p["outs"]["out"].ref, want)


def test_saturated_operands_reach_the_overflow():
    for item in _items("linear", "saturated"):
        o = ic.prepared(*item)["o"]
        assert o["x"][0, 0] == 0 and o["x"][0, 2] == -90 and o["x"][0, 3] == -100 and abs(o["x"][0, 1].item() - ic.SILU_GRAD_ZERO) < 1e-7
        if o["act_out"] and o["bias"] is not None and o["bias"].numel() > 6:
            assert o["bias"][5] == -100 and o["bias"][6] == 40
    h = ic.prepared("head", (1, 16, 24, 256, 1, 0), "saturated")["o"]
    assert (h["x"] * h["scale"][:, None, None] + h["shift"][:, None, None]).abs().max() > 25 and h["shift"].abs().max() == 4


# ---------------------------------------------------------------------------------------------------- the suite bites
def _report(what, item, cls, p, bad, out):
    e = ic.row_error(bad, out.ref, out.S)
    fig, row = ic.worst_row(e)
    old = ic.global_error(bad, out.ref)
    print(f"defect {what} in {ic.case_id(item)}: row {row} figure {fig:.3e} / bar {p['bar'][cls]:.3e} = {fig / p['bar'][cls]:.3g}; "
          f"the whole-tensor figure of test_gpu_ops.py on the same tensor {old:.3e} (TOL {ic.TOL:.0e})")
    return fig > p["bar"][cls], old


def _replicated(o, act=None):
    """The fp32 convolution of a case with the edge replicated instead of zero padding: [B, N, H, W]."""
    a = o["x"] if act is None else act
    w = o["w"]
    cols = F.unfold(F.pad(a, (1, 1, 1, 1), mode="replicate"), 3)
    return (torch.einsum("nk,bkp->bnp", w.reshape(w.shape[0], -1), cols) + o["bias"][None, :, None]).view(a.shape[0], -1, a.shape[2], a.shape[3])


@pytest.mark.parametrize("op", ["stem", "head"])
def test_defect_border_pixel_of_the_quiet_image_without_zero_padding(op):
    """Pixel (0, 0) of image 0, output channel 1 (both quiet) from a replicated edge: the row fails its bar and the border
    figure names it, while the whole-tensor figure on the same tensor stays under TOL."""
    hit = []
    for item in _items(op, "quiet_row"):
        B, H, W, _, Cout = item[1][:5]
        if B < 2 or Cout < 2 or (op == "stem" and (H < 2 or W < 2)):
            continue
        p = ic.prepared(*item)
        o, out = p["o"], p["outs"]["out"]
        act = None
        if op == "head":
            act = ic.silu(o["x"] * o["scale"][:, None, None] + o["shift"][:, None, None]).permute(0, 3, 1, 2)
        bad = out.y.clone().view(B, Cout, H, W)
        bad[0, 1, 0, 0] = _replicated(o, act)[0, 1, 0, 0]
        fails, old = _report("border", item, op, p, bad, out)
        eb = ic.border_error(bad, out.ref, out.S, ic.border_mask(H, W))
        assert eb[1] == ic.row_error(bad, out.ref, out.S)[1] and eb.argmax() == 1
        assert old < ic.TOL, "the old figure does not see it"
        hit.append(fails)
    assert len(hit) >= 2 and all(hit)


def test_defect_one_element_left_nan():
    hit = []
    for item in ITEMS:
        p = ic.prepared(*item)
        for name, out in p["outs"].items():
            if out.cls == "exact":
                continue
            bad = out.y.clone()
            bad.view(-1)[bad.numel() // 2] = float("nan")
            e = ic.row_error(bad, out.ref, out.S)
            hit.append(bool(torch.isinf(e).sum() == 1 and (e > p["bar"][out.cls]).sum() >= 1))
    item = ("head", (3, 8, 8, 4, 1, 0), "quiet_row")
    p = ic.prepared(*item)
    bad = p["outs"]["out"].y.clone()
    bad[0, 5] = float("nan")
    fails, old = _report("nan", item, "head", p, bad, p["outs"]["out"])
    assert fails and not old < ic.TOL                                              # NaN: the old comparison is false as well
    assert hit and all(hit)


def test_defect_h_and_w_swapped_in_the_index():
    """The output of a non-square map written with the pixel index y * H + x: every non-square case fails; on a square map the
    defect is the identity."""
    hit = []
    for op in ("stem", "head"):
        for item in _items(op):
            B, H, W = item[1][:3]
            p = ic.prepared(*item)
            out = p["outs"]["out"]
            y = out.y.view(-1, H, W)
            bad = torch.zeros_like(y).view(-1, H * W)
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            bad[:, (yy * H + xx).clamp_max(H * W - 1).reshape(-1)] = y.reshape(-1, H * W)
            if H == W:
                assert torch.equal(bad, y.reshape(-1, H * W))
                continue
            if H == 1:
                continue                                                          # y * H + x = x
            fails, _ = _report("swap", item, op, p, bad, out)
            hit.append(fails)
    assert len(hit) >= 20 and all(hit)


def test_defect_row_16_computed_from_row_15():
    hit = []
    for item in _items("linear"):
        if item[1][0] != 17:
            continue
        p = ic.prepared(*item)
        out = p["outs"]["out"]
        bad = out.y.clone()
        bad[16] = bad[15]
        fails, _ = _report("row16", item, "linear", p, bad, out)
        assert torch.equal(ic.row_error(bad, out.ref, out.S)[:16], ic.row_error(out.y, out.ref, out.S)[:16])
        hit.append(fails)
    assert len(hit) >= 8 and all(hit)


def test_defect_strip_counted_in_the_neighbouring_statistics_row():
    """The last strip (8 pixels) of a statistics row's range added to the next row instead."""
    hit = []
    for item in _items("stem"):
        B, H, W, Cin, Cout = item[1][:5]
        rows = ic.stem_rows(item[1])
        if B * rows < 2:
            continue
        p = ic.prepared(*item)
        y = p["outs"]["out"].y.view(B, Cout, H * W)
        per = H * W // rows
        strip = y[0, :, per - 8:per]
        for name, moved in (("sum", strip.sum(1)), ("sq", (strip * strip).sum(1))):
            out = p["outs"][name]
            bad = out.y.clone()
            bad[0] -= moved
            bad[1] += moved
            fails, _ = _report(f"strip ({name})", item, "stats", p, bad, out)
            hit.append(fails)
    assert len(hit) >= 6 and all(hit)
