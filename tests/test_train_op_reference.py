"""CPU: the statements, restatements, bars and dropout mask of tests/train_op_cases.py, which tests/test_gpu_train_op_elements.py holds
the small training kernels to.  Each fp64 statement against fp64 autograd of the expression it is the backward of; the fp32
restatement against fp64 on every (case, regime), 4 r32 <= CAP on every one; the FLOOR constants against their measurement; the
quality of the restated dropout mask; and the figure on six planted defects (the suite bites)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_op_cases as tc

ITEMS = [item for op in tc.OPS for item in tc.cases(op)]


def _items(op, regime=None):
    return [it for it in tc.cases(op) if regime is None or it[2] == regime]


def test_case_lists_reach_every_guard():
    B, K, N = ({s[i] for s in tc.LINEAR} for i in range(3))
    assert B == {1, 3, 4, 5, 8, 9, 16} and K == {4, 36, 64, 68, 200} and N == {1, 15, 16, 17, 33}
    assert {(b, k) for b, k, _, _ in tc.LINEAR} >= {(b, k) for b in (4, 5, 8, 9, 16) for k in (36, 68, 200)}
    assert {s[3] for s in tc.LINEAR} == {0, 1}
    assert {f[2] for f in tc.LINEAR_FORMS} == {True, False} and {f[3] for f in tc.LINEAR_FORMS} == {True, False}
    assert {(f[0], f[1]) for f in tc.LINEAR_FORMS} >= {(0, 0), (1, 1)}
    assert {s[0] for s in tc.BATCH} == {1, 3, 5} and {s[1:] for s in tc.BATCH} == {(5, 68), (16, 64)}
    assert len(set(tc.BATCH_N)) == 5 and max(tc.BATCH_N) > sorted(tc.BATCH_N)[-2]
    assert {r for r, _ in tc.SOFTMAX} == {1, 2, 5, 7, 64} and {L for _, L in tc.SOFTMAX} == {1, 16, 63, 64, 65, 100, 256}
    assert set(tc.TRANSPOSE) == {(Z, L) for Z in (1, 3) for L in (1, 31, 32, 33, 100)}
    assert {s[1] for s in tc.COLSUM} == {1, 7, 16, 17, 112, 113, 128, 129, 300, 512} and {s[2] for s in tc.COLSUM} == {1, 40, 64, 65, 130}
    assert not tc.colsum_unrolled(112).any() and tc.colsum_unrolled(113).sum() == 8 and tc.colsum_unrolled(512).all()
    assert {s[1:3] for s in tc.STEM} == {(1, 1), (1, 7), (5, 12), (32, 32), (25, 41), (33, 31)}
    assert {s[3] for s in tc.STEM} == {1, 2, 3, 16} and {s[4] for s in tc.STEM} == {4, 12, 32, 96, 256} and {s[0] for s in tc.STEM} >= {1, 3}
    assert {s[1] * s[2] for s in tc.STEM} >= {1023, 1024, 1025}
    assert {s[1:3] for s in tc.HEAD} == {(1, 1), (3, 5), (16, 32), (19, 27), (23, 22)}
    assert {s[3] for s in tc.HEAD} == {4, 32, 96, 256} and {s[4] for s in tc.HEAD} == {1, 2, 3, 4} and {s[0] for s in tc.HEAD} >= {1, 3}
    assert {s[1] * s[2] for s in tc.HEAD} >= {512, 513, 506}
    # the fold of the partial rows enters its unrolled loop from 8 * 15 + 1 rows on
    assert max(s[0] * -(-s[1] * s[2] // 1024) for s in tc.STEM) > 120 and max(s[0] * -(-s[1] * s[2] // 512) for s in tc.HEAD) > 120
    assert {(s[0], s[4]) for s in tc.RESAMPLE} == {(2, 4), (2, 12), (1, 4), (1, 12)} and all(s[2] != s[3] for s in tc.RESAMPLE)
    assert tc.DROPOUT_BIG[1] // 4 > 8192 * 256
    for op in tc.OPS:
        assert len(set(tc.SHAPES[op])) == len(tc.SHAPES[op])
    regimes = {op: {r for _, _, r in tc.cases(op)} for op in tc.OPS}
    assert regimes["linear"] == {"iid", "quiet_row", "saturated"} and regimes["softmax"] == {"iid", "quiet_row", "peaked"}
    assert regimes["head"] == {"iid", "quiet_row", "saturated"} and regimes["dropout0"] == {"iid", "saturated"}


@pytest.mark.parametrize("item", ITEMS, ids=tc.case_id)
def test_restatement_against_fp64(item):
    """The fp32 restatement is the statement: its worst row is at rounding level, four times it fits under the kernel's existing
    bar (so no device bar is clamped below 4 r32), and it passes its own bar."""
    p = tc.prepared(*item)
    for name, out in p["outs"].items():
        for acc in tc.forms(out):
            ref, S, y = tc.target(out, acc)
            assert (S >= ref.abs() * (1 - 1e-12)).all(), name                    # the figure's denominator bounds the result
            e = tc.row_error(y, ref, S)
            assert torch.isfinite(e).all() and (e <= p["bar"][out.cls]).all(), (name, acc, tc.worst_row(e))
    for cls, r32 in p["r32"].items():
        print(f"{tc.case_id(item)}: {cls} r32 {r32:.2e}, bar {p['bar'][cls]:.2e}")
        assert 4 * r32 <= tc.CAP[cls], (cls, r32)
        assert tc.FLOOR[cls] <= p["bar"][cls] <= tc.CAP[cls]


def test_floors():
    """FLOOR[class] is 4 x the worst iid row figure of the class's restatement over all its shapes, within a factor 1.5."""
    worst = {}
    for item in ITEMS:
        if item[2] == "iid":
            for cls, r32 in tc.prepared(*item)["r32"].items():
                worst[cls] = max(worst.get(cls, (-1.0, "")), (r32, tc.case_id(item)))
    assert set(worst) == set(tc.FLOOR) == set(tc.CAP)
    for cls, (r32, where) in sorted(worst.items()):
        print(f"{cls}: worst iid r32 {r32:.3e} ({where}), 4 x = {4 * r32:.3e}, FLOOR {tc.FLOOR[cls]:.3e}, CAP {tc.CAP[cls]:.0e}")
    for cls, (r32, where) in worst.items():
        assert tc.FLOOR[cls] / 1.5 <= 4 * r32 <= 1.5 * tc.FLOOR[cls], (cls, r32, where)
        assert tc.FLOOR[cls] < tc.CAP[cls]


# ---------------------------------------------------------------------------------------------------- statements against autograd
def _close(name, got, want, S):
    assert (got - want).abs().max() <= 1e-12 * S.abs().max().clamp_min(1e-300), name


def _leaf(t):
    return t.double().requires_grad_(True)


@pytest.mark.parametrize("item", _items("linear", "iid") + _items("linear_batch", "iid") + _items("linear_batch", "saturated"), ids=tc.case_id)
def test_linear_statement_is_autograd(item):
    p = tc.prepared(*item)
    o, outs = p["o"], p["outs"]
    x = _leaf(o["x"])
    a = F.silu(x) if o["act_in"] else x
    ws, bs, loss = [], [], 0
    for job in o["jobs"]:
        ws.append(_leaf(job["w"]))
        bs.append(_leaf(torch.zeros(job["w"].shape[0])))
        loss = loss + (F.linear(a, ws[-1], bs[-1]) * job["dy"].double()).sum()
    loss.backward()
    _close("dx", outs["dx"].ref0, x.grad, outs["dx"].S0)
    for j in range(len(ws)):
        _close("dw", outs[f"dw{j}"].ref0, ws[j].grad, outs[f"dw{j}"].S0)
        _close("db", outs[f"db{j}"].ref0, bs[j].grad, outs[f"db{j}"].S0)


def test_softmax_statement_is_autograd():
    gen = torch.Generator().manual_seed(11)
    for rows, L in ((5, 1), (7, 63), (3, 256)):
        z = (3 * torch.randn(rows, L, generator=gen, dtype=torch.float64)).requires_grad_(True)
        dp = torch.randn(rows, L, generator=gen, dtype=torch.float64)
        prob = torch.softmax(z, -1)
        prob.backward(dp)
        o = dict(p=prob.detach(), dp=dp)
        _close("dp", tc._fresh("softmax", o, torch.float64)["dp"][1], z.grad, tc._scale("softmax", o)["dp"])


@pytest.mark.parametrize("item", _items("colsum", "iid")[::7], ids=tc.case_id)
def test_colsum_statement_is_autograd(item):
    p = tc.prepared(*item)
    cs = p["o"]["colsum"].double()
    e, bias = _leaf(torch.zeros(cs.shape[0], cs.shape[2])), _leaf(torch.zeros(cs.shape[2]))
    ((torch.zeros_like(cs) + e[:, None] + bias) * cs).sum().backward()
    _close("dimg", p["outs"]["dimg"].ref0, e.grad, p["outs"]["dimg"].S0)
    _close("dbias", p["outs"]["dbias"].ref0, bias.grad, p["outs"]["dbias"].S0)


@pytest.mark.parametrize("item", _items("stem", "iid"), ids=tc.case_id)
def test_stem_statement_is_autograd(item):
    p = tc.prepared(*item)
    o, outs = p["o"], p["outs"]
    B, H, W, Cin, Cout = item[1]
    x, w, b = _leaf(o["x"]), _leaf(o["w"]), _leaf(torch.zeros(Cout))
    F.conv2d(x, w, b, padding=1).backward(o["dy"].double().view(B, H, W, Cout).permute(0, 3, 1, 2))
    for name, g in (("dx", x.grad), ("dw", w.grad), ("db", b.grad)):
        _close(name, outs[name].ref0, g, outs[name].S0)


@pytest.mark.parametrize("item", _items("head", "iid") + _items("head", "saturated")[:4], ids=tc.case_id)
def test_head_statement_is_autograd(item):
    p = tc.prepared(*item)
    o, outs = p["o"], p["outs"]
    B, H, W, C, Cout = item[1]
    act = F.silu(o["x"].double() * o["scale"].double()[:, None] + o["shift"].double()[:, None])
    a = act.view(B, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    w, b = _leaf(o["w"]), _leaf(torch.zeros(Cout))
    F.conv2d(a, w, b, padding=1).backward(o["dy"].double())
    _close("da", outs["da"].ref0, a.grad.permute(0, 2, 3, 1).reshape(B, H * W, C), outs["da"].S0)
    _close("dw", outs["dw"].ref0, w.grad, outs["dw"].S0)
    _close("db", outs["db"].ref0, b.grad, outs["db"].S0)


@pytest.mark.parametrize("item", _items("resample", "iid"), ids=tc.case_id)
def test_resample_statement_is_autograd(item):
    p = tc.prepared(*item)
    mode, B, h, w, C = item[1]
    g = p["o"]["g"].double().permute(0, 3, 1, 2)
    x = torch.zeros(B, C, h, w, dtype=torch.float64, requires_grad=True) if mode == 2 else \
        torch.zeros(B, C, 2 * h, 2 * w, dtype=torch.float64, requires_grad=True)
    (F.interpolate(x, scale_factor=2, mode="nearest") if mode == 2 else F.avg_pool2d(x, 2, 2)).backward(g)
    _close("out", p["outs"]["out"].ref0, x.grad.permute(0, 2, 3, 1), p["outs"]["out"].S0)


def test_silu_grad_zero():
    x = torch.tensor([tc.SILU_GRAD_ZERO], dtype=torch.float64, requires_grad=True)
    F.silu(x).backward()
    assert abs(x.grad.item()) < 1e-15 and abs(tc.SILU_GRAD_ZERO + 1.2785) < 1e-4
    sat = tc.prepared("linear", (16, 4, 16, 1), "saturated")["o"]["x"]
    assert sat[0, 0] == 0 and sat[0, 2] < -88 and sat[0, 3] < -88 and abs(sat[0, 1].item() - tc.SILU_GRAD_ZERO) < 1e-7
    wide = tc.prepared("linear", (9, 200, 17, 1), "saturated")["o"]["x"]
    assert wide[:, 4:].min() < -25 and wide[:, 4:].max() > 25
    h = tc.prepared("head", (3, 19, 27, 256, 4), "saturated")["o"]
    assert (h["x"] * h["scale"][:, None] + h["shift"][:, None]).abs().max() > 25 and h["scale"].max() > 8 and h["shift"].abs().max() == 4


# ---------------------------------------------------------------------------------------------------- the dropout specification
def test_dropout_restatement():
    """Scalar splitmix64 in Python integers against the numpy restatement; p = 0 keeps everything; the values."""
    M = (1 << 64) - 1
    for seed in tc.DROPOUT_SEEDS:
        keep = tc.dropout_keep(seed, 2, 24, 0.3)
        thresh = int(float(np.float32(0.3)) * 2 ** 32)
        for idx in range(48):
            z = (seed + idx * 0x9E3779B97F4A7C15) & M
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            z ^= z >> 31
            assert keep.reshape(-1)[idx] == ((z >> 32) >= thresh), (seed, idx)
        assert tc.dropout_keep(seed, 3, 64, 0.0).all()
    x = tc.dropout_input(2, 24, 0)
    v = tc.dropout_values(x, tc.dropout_keep(0, 2, 24, 0.5), 0.5)
    assert v.dtype == np.float32 and set(np.unique(v / x).tolist()) == {0.0, 2.0}
    assert np.array_equal(tc.dropout_values(x, tc.dropout_keep(5, 2, 24, 0.0), 0.0).view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("p", tc.DROPOUT_P)
def test_dropout_mask_quality(p):
    """A property of the specification (the device has to equal it exactly): over 2^20 elements the kept fraction is within five
    binomial standard deviations of 1 - p; the masks of two batch rows, and of two seeds, agree on a fraction within five of
    (1 - p)^2 + p^2."""
    n = 1 << 20
    p32 = float(np.float32(p))
    masks = {seed: tc.dropout_keep(seed, 2, n, p) for seed in tc.DROPOUT_SEEDS}
    for seed, m in masks.items():
        for b in range(2):
            frac = m[b].mean()
            print(f"p {p} seed {seed} row {b}: kept {frac:.6f}")
            assert abs(frac - (1 - p32)) <= 5 * math.sqrt(p32 * (1 - p32) / n), (seed, b, frac)
    q = (1 - p32) ** 2 + p32 ** 2
    sigma = math.sqrt(q * (1 - q) / n)
    pairs = [(masks[s][0], masks[s][1]) for s in tc.DROPOUT_SEEDS]
    pairs += [(masks[a][0], masks[b][0]) for a, b in ((0, 1), (0, 2 ** 63 + 5), (1, 2 ** 63 + 5))]
    for m0, m1 in pairs:
        agree = (m0 == m1).mean()
        print(f"p {p}: agree {agree:.6f} (expected {q:.6f}, sigma {sigma:.1e})")
        assert abs(agree - q) <= 5 * sigma


# ---------------------------------------------------------------------------------------------------- the suite bites
def _fails(cls, p, bad, ref, S):
    return bool((tc.row_error(bad, ref, S) > p["bar"][cls]).any())


def test_defect_dropped_ragged_k_chunk():
    """dx without the last, ragged 64-wide K chunk."""
    hit = []
    for item in _items("linear"):
        K = item[1][1]
        if K % 64:
            p = tc.prepared(*item)
            ref, S, y = tc.target(p["outs"]["dx"], False)
            bad = y.clone()
            bad[:, K // 64 * 64:] = 0
            hit.append(_fails("linear", p, bad, ref, S))
    assert hit and all(hit)


def test_defect_skipped_row_tail():
    """The softmax backward is in place: rows of the rows % 4 tail keep dp."""
    hit = []
    for item in _items("softmax"):
        rows = item[1][0]
        if rows % 4:
            p = tc.prepared(*item)
            ref, S, y = tc.target(p["outs"]["dp"], False)
            bad = y.clone()
            bad[rows // 4 * 4:] = p["o"]["dp"][rows // 4 * 4:]
            hit.append(_fails("softmax", p, bad, ref, S))
    assert hit and all(hit)


def test_defect_quiet_row_left_out_of_db():
    hit = []
    for item in _items("linear", "quiet_row") + _items("linear_batch", "quiet_row"):
        p = tc.prepared(*item)
        if p["o"]["x"].shape[0] >= 2:
            for acc in (False, True):
                ref, S, y = tc.target(p["outs"]["db0"], acc)
                bad = p["o"]["jobs"][0]["dy"][1:].sum(0) + (p["outs"]["db0"].old if acc else 0)
                hit.append(_fails("linear", p, bad, ref, S))
    assert hit and all(hit)


@pytest.mark.parametrize("op,name", [("stem", "dx"), ("head", "da")])
def test_defect_shifted_tap_at_a_border_pixel(op, name):
    """One border pixel of the last image computed from dy shifted by one column: its row fails, and the border figure names it."""
    hit = []
    for item in _items(op):
        B, H, W = item[1][:3]
        if W < 2:
            continue
        p = tc.prepared(*item)
        o = p["o"]
        ref, S, y = tc.target(p["outs"][name], False)
        d = o["dy"].transpose(1, 2).reshape(B, -1, H, W) if op == "stem" else o["dy"]
        shifted = tc._conv_t(torch.roll(d, 1, dims=3), o["w"])
        bad = y.clone()
        if op == "stem":
            bad[-1, :, 0, W - 1] = shifted[-1, :, 0, W - 1]
        else:
            bad[-1, W - 1, :] = shifted[-1, :, 0, W - 1]
        e = tc.row_error(bad, ref, S)
        eb = tc.border_error(bad, ref, S, tc.pixel_mask(op, item[1])[name])
        assert torch.equal(e[:-1], tc.row_error(y, ref, S)[:-1]) and eb[-1] == e[-1]
        hit.append(bool(e[-1] > p["bar"][p["outs"][name].cls]))
    assert hit and all(hit)


def test_defect_dropped_unrolled_column_sum():
    hit = []
    for item in _items("colsum"):
        ipb = item[1][1]
        tail = torch.from_numpy(~tc.colsum_unrolled(ipb))
        if not tail.all():
            p = tc.prepared(*item)
            ref, S, y = tc.target(p["outs"]["dimg"], False)
            bad = p["o"]["colsum"][:, tail].sum(1)
            hit.append(_fails("colsum", p, bad, ref, S))
    assert hit and all(hit)


def test_defect_dropout_index_off_by_one_in_a_quad():
    """Lane j of a quad hashed with the index of lane (j + 1) % 4: the mode 1 result is not the restatement's bits, and the mode 0
    values fail the figure."""
    for B, n, C in tc.DROPOUT_SHAPES:
        idx = tc.dropout_index(B, n)
        wrong = (idx & ~np.uint64(3)) | ((idx + np.uint64(1)) & np.uint64(3))
        for p in tc.DROPOUT_P[1:]:
            for seed in tc.DROPOUT_SEEDS:
                x = tc.dropout_input(B, n, seed)
                good = tc.dropout_values(x, tc.dropout_keep(seed, B, n, p), p)
                bad = tc.dropout_values(x, tc.dropout_keep(seed, B, n, p, idx=wrong), p)
                if n > 4:
                    assert not np.array_equal(good.view(np.uint32), bad.view(np.uint32)), (B, n, p, seed)
    hit = []
    for item in _items("dropout0"):
        B, n, C, p, seed = item[1]
        pr = tc.prepared(*item)
        ref, S, y = tc.target(pr["outs"]["out"], False)
        idx = tc.dropout_index(B, n)
        wrong = torch.from_numpy(tc.dropout_keep(seed, B, n, p, idx=(idx & ~np.uint64(3)) | ((idx + np.uint64(1)) & np.uint64(3))))
        full = tc._fresh("dropout0", dict(pr["o"], keep=torch.ones_like(wrong)), torch.float32)["out"][1]
        hit.append(_fails("dropout", pr, torch.where(wrong, full, torch.zeros_like(full)), ref, S))
    # p = 0 keeps everything and a map of one quad may lose or keep all four either way: every other case fails
    assert any(hit) and all(h for h, it in zip(hit, _items("dropout0")) if it[1][3] > 0 and it[1][1] > 4)
