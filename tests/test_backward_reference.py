"""CPU: the fp64 statements of tests/backward_ledger.py against fp64 autograd of stock torch ops (both sides fp64: 1e-10 of the
tensor's magnitude), and the pointer resolution / static checks of the ledger on hand-made structs over CPU tensors -- a planted
out-of-bounds stride, a second writer without its accumulate flag, a first writer that accumulates and an output that overlaps an
input must each be REPORTED."""
import ctypes
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import backward_ledger as bl
from anoddpm_amd import _lib

TOL = 1e-10


def close(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert float((got - ref).abs().max()) <= TOL * max(float(ref.abs().max()), 1e-300), float((got - ref).abs().max())


def rnd(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------- convolutions
@pytest.mark.parametrize("N,K", [(8, 12), (12, 8)])
def test_conv3x3_statements(N, K):
    B, H, W = 2, 5, 7
    a = rnd(B, K, H, W, seed=1).requires_grad_(True)
    w = rnd(N, K, 3, 3, seed=2).requires_grad_(True)
    dy = rnd(B, N, H, W, seed=3)
    F.conv2d(a, w, padding=1).backward(dy)
    d = dy.permute(0, 2, 3, 1)
    close(bl.conv3x3_input(d, w.detach()), a.grad.permute(0, 2, 3, 1))
    close(bl.conv3x3_weight(a.detach().permute(0, 2, 3, 1), d), w.grad)


def test_conv1x1_statement_over_a_column_range():
    B, P, N, K, k0, kc = 2, 9, 6, 20, 12, 8                  # the second source of a two-source skip convolution
    a = rnd(B, P, K, seed=1).requires_grad_(True)
    w = rnd(N, K, seed=2)
    dy = rnd(B, P, N, seed=3)
    (a @ w.T).backward(dy)
    close(bl.conv1x1_input(dy, w, k0, kc), a.grad[:, :, k0:k0 + kc])
    close(bl.conv1x1_input(dy, w), a.grad)


def test_head_and_stem_statements():
    B, H, W, C, Co = 2, 6, 5, 8, 2
    x = rnd(B, H, W, C, seed=1)
    sc, sh = rnd(B, C, seed=2), rnd(B, C, seed=3)
    a = F.silu(x * sc[:, None, None, :] + sh[:, None, None, :]).permute(0, 3, 1, 2).requires_grad_(True)
    w = rnd(Co, C, 3, 3, seed=4).requires_grad_(True)
    b = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    dy = rnd(B, Co, H, W, seed=5)
    F.conv2d(a, w, b, padding=1).backward(dy)
    da, dw, db = bl.head_backward(x, sc, sh, w.detach(), dy)
    close(da, a.grad.permute(0, 2, 3, 1))
    close(dw, w.grad)
    close(db, b.grad)
    xs = rnd(B, 1, H, W, seed=6).requires_grad_(True)
    ws = rnd(C, 1, 3, 3, seed=7).requires_grad_(True)
    bs = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    dys = rnd(B, H, W, C, seed=8)
    F.conv2d(xs, ws, bs, padding=1).backward(dys.permute(0, 3, 1, 2))
    dw, db, dx = bl.stem_backward(xs.detach(), ws.detach(), dys)
    close(dw, ws.grad)
    close(db, bs.grad)
    close(dx, xs.grad)


# ---------------------------------------------------------------------------------------------------- GroupNorm (+ SiLU, + resample)
def _gn_forward(x, gamma, beta, act, a_mode, Hs, Ws):
    """stock ops: GroupNorm(32) -> SiLU? -> nearest x2 / 2x2 average, on NCHW"""
    B, P, C = x.shape
    h = F.group_norm(x.reshape(B, Hs, Ws, C).permute(0, 3, 1, 2), 32, gamma, beta, eps=1e-5)
    if act:
        h = F.silu(h)
    if a_mode == 1:
        h = F.interpolate(h, scale_factor=2, mode="nearest")
    elif a_mode == 2:
        h = F.avg_pool2d(h, 2, 2)
    return h.permute(0, 2, 3, 1).reshape(B, -1, C)


def _stats(x, G=32):
    B, P, C = x.shape
    xg = x.reshape(B, P, G, C // G)
    mean = xg.mean(dim=(1, 3))
    var = xg.var(dim=(1, 3), unbiased=False)
    return mean, 1.0 / torch.sqrt(var + 1e-5)


@pytest.mark.parametrize("c0,c1", [(256, 128), (64, 0)])        # 256 + 128: 12 channels per group, groups straddle the sources
@pytest.mark.parametrize("a_mode", [0, 1, 2])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("with_dres", [False, True])
def test_gn_backward_statement(c0, c1, a_mode, act, with_dres):
    B, Hs, Ws, C = 2, 4, 6, c0 + c1
    x0, x1 = rnd(B, Hs * Ws, c0, seed=1) * 1.5 + 0.3, rnd(B, Hs * Ws, max(c1, 1), seed=2)
    x0.requires_grad_(True)
    x1.requires_grad_(True)
    x = torch.cat([x0, x1], dim=2) if c1 else x0
    gamma, beta = (1 + 0.3 * rnd(C, seed=3)).requires_grad_(True), (0.2 * rnd(C, seed=4)).requires_grad_(True)
    out = _gn_forward(x, gamma, beta, act, a_mode, Hs, Ws)
    da = rnd(*out.shape, seed=5)
    dres = rnd(B, Hs * Ws, C, seed=6) if with_dres else None
    out.backward(da)
    mean, rstd = _stats(x.detach())
    dx, dg, db = bl.gn_backward(x.detach(), da, gamma.detach(), beta.detach(), mean, rstd, act, a_mode, Hs, Ws, dres)
    ref = torch.cat([x0.grad, x1.grad], dim=2) if c1 else x0.grad
    close(dx, ref + dres if with_dres else ref)
    close(dg, gamma.grad)
    close(db, beta.grad)


def test_gn_tile_partials_statement():
    """Row (b, tile) = the per-image dbeta / dgamma of an upstream gradient that is zero outside that tile."""
    B, H, W, c0, c1 = 2, 32, 48, 64, 32
    C = c0 + c1
    x = rnd(B, H * W, C, seed=1) + 0.2
    gamma, beta = 1 + 0.3 * rnd(C, seed=2), 0.2 * rnd(C, seed=3)
    da = rnd(B, H * W, C, seed=4)
    mean, rstd = _stats(x)
    rows = bl.gn_tile_partials(x, da, gamma, beta, mean, rstd, H, W)
    assert rows.shape == (B, 6, C, 2)
    for b, tile in ((0, 0), (1, 4), (1, 5)):
        ty, tx = divmod(tile, W // 16)
        m = torch.zeros(B, H, W, 1, dtype=torch.float64)
        m[b, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = 1
        # y = gamma * xhat + beta with xhat held fixed: d/dbeta and d/dgamma of <silu(y), da * m>
        g, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        grp = torch.arange(C) // (C // 32)
        xhat = (x - mean[:, grp][:, None, :]) * rstd[:, grp][:, None, :]
        (F.silu(g * xhat + bt) * (da * m.reshape(B, H * W, 1))).sum().backward()
        close(rows[b, tile, :, 0], bt.grad)
        close(rows[b, tile, :, 1], g.grad)
    _, dg, db = bl.gn_backward(x, da, gamma, beta, mean, rstd, 1, 0, H, W)
    close(rows[..., 0].sum(dim=(0, 1)), db)
    close(rows[..., 1].sum(dim=(0, 1)), dg)


# ---------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("L", [16, 64])
def test_attention_backward_statement(heads, L):
    B, ch = 2, 8
    C = heads * ch
    qkv = rnd(B, L, 3 * C, seed=L + heads).requires_grad_(True)     # head h: q at channel 3 h ch, k at + ch, v at + 2 ch
    alpha = 1.0 / math.sqrt(ch)
    t = qkv.reshape(B, L, heads, 3, ch).permute(0, 2, 3, 1, 4)     # [B, heads, 3, L, ch]
    q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    S = alpha * q @ k.transpose(-1, -2)
    S.retain_grad()
    P = torch.softmax(S, dim=-1)
    att = P @ v                                                     # [B, heads, L, ch]
    datt = rnd(B, heads, L, ch, seed=7)
    att.backward(datt)
    dS, dV, dQ, dK = bl.attention_backward(q.detach(), k.detach(), v.detach(), P.detach(), datt, alpha)
    g = qkv.grad.reshape(B, L, heads, 3, ch).permute(0, 2, 3, 1, 4)
    close(dS, S.grad)
    close(dQ, g[:, :, 0])
    close(dK, g[:, :, 1])
    close(dV, g[:, :, 2])


# ---------------------------------------------------------------------------------------------------- linear, resample, dropout
@pytest.mark.parametrize("act_in", [0, 1])
def test_linear_backward_statements(act_in):
    B, K = 3, 10
    x = rnd(B, K, seed=1).requires_grad_(True)
    a = F.silu(x) if act_in else x
    ws = [rnd(n, K, seed=2 + n).requires_grad_(True) for n in (4, 12, 7)]          # jobs of different N
    bs = [torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True) for w in ws]
    dys = [rnd(B, w.shape[0], seed=20 + w.shape[0]) for w in ws]
    sum((F.linear(a, w, b) * dy).sum() for w, b, dy in zip(ws, bs, dys)).backward()
    outs, dx = bl.linear_backward_batch(x.detach(), [(w.detach(), dy) for w, dy in zip(ws, dys)], act_in)
    close(dx, x.grad)
    for (dw, db), w, b in zip(outs, ws, bs):
        close(dw, w.grad)
        close(db, b.grad)
    # the single form = a batch of one
    x1 = x.detach().clone().requires_grad_(True)
    (F.linear(F.silu(x1) if act_in else x1, ws[1].detach()) * dys[1]).sum().backward()
    dw, db, dx = bl.linear_backward(x1.detach(), ws[1].detach(), dys[1], act_in)
    close(dx, x1.grad)
    close(dw, ws[1].grad)
    close(db, bs[1].grad)


def test_resample_statements():
    B, H, W, C = 2, 4, 6, 5
    x = rnd(B, H, W, C, seed=1)
    nchw = lambda t: t.permute(0, 3, 1, 2)
    close(nchw(bl.resample(x, 1)), F.interpolate(nchw(x), scale_factor=2, mode="nearest"))
    close(nchw(bl.resample(x, 2, 4.0)), 4.0 * F.avg_pool2d(nchw(x), 2, 2))
    close(bl.resample(x, 3), x[:, ::2, ::2])
    close(bl.resample(x, 1, 0.0), bl.resample(x, 1, 1.0))                       # scale 0 is read as 1
    y3, y1 = rnd(B, H // 2, W // 2, C, seed=2), rnd(B, 2 * H, 2 * W, C, seed=3)
    # modes 3 / 4 are adjoints of each other; so are nearest-up and 4 x the average (the sum of the four children)
    assert abs(float((bl.resample(x, 3) * y3).sum() - (x * bl.resample(y3, 4)).sum())) <= TOL * float((x * bl.resample(y3, 4)).abs().sum())
    assert abs(float((bl.resample(x, 1) * y1).sum() - (x * bl.resample(y1, 2, 4.0)).sum())) <= TOL * float((x * bl.resample(y1, 2, 4.0)).abs().sum())
    z = bl.resample(y3, 4)
    assert z.shape == (B, H, W, C) and float(z[:, 1::2].abs().max()) == 0 and float(z[:, :, 1::2].abs().max()) == 0


def test_dropout_backward_statement():
    p = 0.3
    h = rnd(2, 12, 8, seed=1).requires_grad_(True)
    mask = (torch.rand(2, 12, 8, generator=torch.Generator().manual_seed(2)) > p).double()
    d = rnd(2, 12, 8, seed=3)
    (h * mask / (1 - p)).backward(d)
    close(bl.dropout_backward(d, mask, p), h.grad)


# ---------------------------------------------------------------------------------------------------- the metric
def test_block_figure_is_local():
    ref = rnd(3, 50, 192, seed=1)
    ref[:, :, :64] *= 1000                                       # a loud block must not hide a wrong quiet one
    got = ref.clone()
    got[1, 7, 130] += 1e-3 * float(ref[1, :, 128:].abs().max())
    fig, where, bar, ok = bl.block_figure(got, ref, bar=2e-5)
    assert where == (1, 128) and abs(fig - 1e-3) < 1e-9 and not ok and abs(bar - 2e-5) < 1e-12
    assert bl.block_figure(ref.clone(), ref, bar=2e-5)[3]
    got[0, 0, 0] = float("nan")
    assert bl.block_figure(got, ref, bar=2e-5)[0] == float("inf")
    # fan-in: the denominator is the largest contribution, not the (cancelled) sum
    a = rnd(1, 10, 64, seed=2)
    s = a + (-a + 1e-9)
    fig, _, bar, ok = bl.block_figure(s + 1e-6 * float(a.abs().max()), s, budget=2 * 2e-5 * bl.block_max(a), den=bl.block_max(a))
    assert ok and abs(fig - 1e-6) < 1e-9 and abs(bar - 4e-5) < 1e-12


# ---------------------------------------------------------------------------------------------------- pointers and static checks
def _plan(tensors, bops, params=None, packs=()):
    named = dict(params or {})
    grads = {k: torch.zeros_like(p) for k, p in named.items()}
    return SimpleNamespace(keep=list(tensors), named=named, gview=grads, pptr={k: p.data_ptr() for k, p in named.items()},
                           gptr={k: g.data_ptr() for k, g in grads.items()}, pack_ops=[(_lib.OP_PACK, st) for st in packs],
                           _drop_ops=[], bops=bops)


def _rs(inp, out, B, H, W, C, mode, scale=1.0, acc=0):
    st = _lib.ResampleArgs()
    st.inp, st.out = inp if isinstance(inp, int) else inp.data_ptr(), out if isinstance(out, int) else out.data_ptr()
    st.B, st.H, st.W, st.C, st.mode, st.scale, st.accumulate = B, H, W, C, mode, scale, acc
    return (_lib.OP_RESAMPLE, st)


def test_resolve_and_view():
    am = bl.AddressMap()
    big = torch.arange(2 * 12 * 6, dtype=torch.float32)
    part = torch.zeros(8, dtype=torch.float64)
    am.add(big, "big")
    am.add(part, "part")
    am.add(big[24:48], "inner")                                  # a view inside a larger tensor: the smallest holder wins
    t, off, name = am.resolve(big.data_ptr() + 4 * 5)
    assert t is big and off == 5 and name == "big"
    assert am.resolve(big.data_ptr() + 4 * 30)[2] == "inner" and am.resolve(big.data_ptr() + 4 * 30)[1] == 6
    inner = am.view(big.data_ptr() + 4 * 31, 1, 2, 3, 0, 4)       # read through a tensor that is itself a view at an offset
    assert inner.tolist() == [[[31, 32, 33], [35, 36, 37]]]
    assert am.resolve(part.data_ptr() + 8 * 3)[1] == 3           # offsets count elements of the tensor's own dtype
    # q / k / v style interior pointer: B 2, 12 rows of pitch 6, 2 columns from column 2
    v = am.view(big.data_ptr() + 4 * 2, 2, 12, 2, 72, 6)
    assert v.dtype == torch.float64 and v.shape == (2, 12, 2) and v[1, 3, 1] == 72 + 18 + 3
    with pytest.raises(bl.LedgerError, match="resolves to no tensor"):
        am.resolve(big.data_ptr() + 4 * big.numel() + 4096)
    with pytest.raises(bl.LedgerError, match="reaches element"):
        am.view(big.data_ptr() + 4 * 2, 2, 12, 2, 75, 6)          # a batch stride too long: the last row leaves the tensor
    with pytest.raises(bl.LedgerError, match="reaches element"):
        am.view(big.data_ptr() + 4 * 30, 1, 4, 6, 24, 6)          # stays inside `big` but leaves the tensor it resolves to
    with pytest.raises(bl.LedgerError, match="not aligned"):
        am.resolve(part.data_ptr() + 4)


def test_overlaps():
    am = bl.AddressMap()
    qkv = torch.zeros(2 * 16 * 48)
    am.add(qkv, "qkv")
    head = lambda off: am.region(qkv.data_ptr() + 4 * off, (2, 2, 16, 8), (16 * 48, 24, 48, 1))      # heads 2, ch 8: q, k, v interleaved
    q, k, v = head(0), head(8), head(16)
    assert not bl.overlaps(q, k) and not bl.overlaps(k, v) and not bl.overlaps(q, v) and bl.overlaps(q, q)
    assert bl.overlaps(q, head(4)) and bl.overlaps(k, am.region(qkv.data_ptr(), (2, 16, 48), (16 * 48, 48, 1)))
    a = am.region(qkv.data_ptr(), (100,), (1,))
    assert not bl.overlaps(a, am.region(qkv.data_ptr() + 400, (100,), (1,))) and bl.overlaps(a, am.region(qkv.data_ptr() + 396, (3, 5), (7, 1)))


def test_ledger_on_a_hand_made_plan_and_its_planted_violations():
    """Three launches on CPU tensors computed by hand: a nearest-up adjoint that overwrites g, a 1x1 data gradient that accumulates
    into it in place (res == out) through a pack job, a mode-4 scatter.  The ledger passes; each planted violation is reported."""
    B, H, W, C, N = 2, 4, 4, 8, 12
    gen = torch.Generator().manual_seed(5)
    up = torch.randn(B, 2 * H, 2 * W, C, generator=gen)
    dy = torch.randn(B, H * W, N, generator=gen)
    w = torch.randn(N, 20, 1, 1, generator=gen)
    g = torch.full((B, H * W, C), float("nan"))
    packed = torch.zeros(N * C)
    small = torch.randn(B, H // 2, W // 2, C, generator=gen)
    scat = torch.full((B, H, W, C), float("nan"))
    pk = _lib.PackArgs()
    pk.w, pk.out, pk.N, pk.K, pk.kind, pk.bwd, pk.k0, pk.kc = w.data_ptr(), packed.data_ptr(), N, 20, 2, 1, 12, C
    ig = _lib.IgemmArgs()
    ig.a0, ig.bmat, ig.res, ig.out = dy.data_ptr(), packed.data_ptr(), g.data_ptr(), g.data_ptr()
    ig.a0_bs, ig.a0_ld, ig.o_bs, ig.out_ld, ig.r_bs, ig.res_ld = H * W * N, N, H * W * C, C, H * W * C, C
    ig.c0, ig.N, ig.H, ig.W, ig.ks, ig.B, ig.heads, ig.ksplit, ig.alpha = N, C, H, W, 1, B, 1, 1, 1.0
    bops = [_rs(up, g, B, 2 * H, 2 * W, C, 2, 4.0, 0), (_lib.OP_IGEMM, ig), _rs(small, scat, B, H // 2, W // 2, C, 4)]
    # what the "device" computes, in fp32
    g.copy_((4.0 * up.reshape(B, H, 2, W, 2, C).mean(dim=(2, 4))).reshape(B, H * W, C))
    g.add_(dy @ w.reshape(N, 20)[:, 12:20])
    scat.zero_()
    scat[:, ::2, ::2] = small
    plan = _plan([up, dy, g, packed, small, scat], bops, params={"skip.weight": w}, packs=[pk])
    led = bl.Ledger(plan)
    assert len(led.launches) == 3 and not led.exempt and led.static_failures() == []
    assert [len(ws) for ws in led.regions().values()] == [2, 1]
    lines = []
    bad, figs = led.audit(log=lines.append)
    assert not bad and len(figs) == 2 and len(lines) == 2 and all(f[3] < 1e-6 for f in figs), lines
    # arithmetic: the 1x1 launch read the wrong column range of the weight
    pk.k0 = 8
    bad, _ = bl.Ledger(plan).audit(log=lines.append)
    assert len(bad) == 1 and bad[0][1] == [1] and bad[0][2] == "da", bad   # reported at the region's last writer
    pk.k0 = 12
    # 1. a second writer without its accumulate flag
    ig.res = None
    rep = bl.Ledger(plan).static_failures()
    assert len(rep) == 1 and "writer 2" in rep[0] and "overwrites" in rep[0], rep
    ig.res = g.data_ptr()
    # 2. a first writer that accumulates; the poison step's experiment switches this check off
    bops[0][1].accumulate = 1
    rep = bl.Ledger(plan).static_failures()
    assert len(rep) == 1 and "FIRST writer" in rep[0], rep
    assert bl.Ledger(plan).static_failures(first_writer=False) == []
    bops[0][1].accumulate = 0
    # 3. an output that overlaps an input: the scatter writes into the tensor it reads
    both = torch.zeros(B * H * W * C + 64)
    plan3 = _plan([both], [_rs(both.data_ptr() + 4 * 64, both.data_ptr(), B, H // 2, W // 2, C, 4)])
    rep = bl.Ledger(plan3).static_failures()
    assert len(rep) == 1 and "overlaps its input" in rep[0], rep
    # 4. res == out but other strides is not the declared in-place form
    ig.res_ld = C + 4
    with pytest.raises(bl.LedgerError, match="reaches element|different strides"):
        bl.Ledger(plan)
    ig.res_ld = C
    # 5. a region that leaves its buffer: one image too many
    bops[2][1].B = B + 1
    with pytest.raises(bl.LedgerError, match="reaches element"):
        bl.Ledger(plan)
    bops[2][1].B = B
    # 6. two written regions that share elements without being the same region
    plan6 = _plan([up, g], [_rs(up, g, B, 2 * H, 2 * W, C, 2), _rs(up, g.data_ptr() + 4 * C, B - 1, 2 * H, 2 * W, C, 2)])
    assert any("share elements" in r for r in bl.Ledger(plan6).static_failures())
    # 7. an op code without a statement
    plan7 = _plan([up, g], [(_lib.OP_SOFTMAX_BWD, _lib.SoftmaxBwdArgs())])
    with pytest.raises(bl.LedgerError, match="no fp64 statement"):
        bl.Ledger(plan7)
    assert ctypes.sizeof(_lib.LinearBwdArgs) % 8 == 0            # the device job table is read back as an array of these


def test_fused_groupnorm_rows_belong_to_their_groupnorm_backward():
    """A 3x3 data gradient whose epilogue writes the GroupNorm-backward rows (gnb_partial) and the GroupNorm backward that consumes
    them (partial_ready), on CPU tensors filled from the statements: the ledger passes; gnb_* fields that name another GroupNorm's
    statistics are reported at the data-gradient launch."""
    B, H, N, C, G = 2, 16, 32, 32, 32
    P = H * H
    gen = torch.Generator().manual_seed(8)
    w = 0.1 * torch.randn(N, C, 3, 3, generator=gen)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    dy, x = torch.randn(B, P, N, generator=gen), torch.randn(B, P, C, generator=gen)
    mean, rstd = (t.float() for t in _stats(x.double()))
    other_mean, other_rstd = mean + 0.5, rstd * 1.5
    da, gx, packed = torch.empty(B, P, C), torch.empty(B, P, C), torch.zeros(36 * N * C)
    part = torch.empty(B * 1 * C * 2, dtype=torch.float64)
    pk = _lib.PackArgs()
    pk.w, pk.out, pk.N, pk.K, pk.kind, pk.bwd = w.data_ptr(), packed.data_ptr(), N, C, 5, 1
    plan = _plan([dy, x, mean, rstd, other_mean, other_rstd, da, gx, packed, part], [],
                 params={"conv.weight": w, "gn.weight": gamma, "gn.bias": beta}, packs=[pk])
    ig = _lib.IgemmArgs()
    ig.a0, ig.bmat, ig.out = dy.data_ptr(), packed.data_ptr(), da.data_ptr()
    ig.a0_bs, ig.a0_ld, ig.o_bs, ig.out_ld = P * N, N, P * C, C
    ig.c0, ig.N, ig.H, ig.W, ig.ks, ig.B, ig.heads, ig.ksplit, ig.cfg, ig.alpha = N, C, H, H, 3, B, 1, 1, 3, 1.0
    ig.gnb_partial, ig.gnb_x0, ig.gnb_gamma, ig.gnb_beta = part.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    ig.gnb_mean, ig.gnb_rstd, ig.gnb_x0_bs, ig.gnb_c0, ig.gnb_x0_ld, ig.gnb_x1_ld, ig.gnb_groups = mean.data_ptr(), rstd.data_ptr(), P * C, C, C, 4, G
    ga = _lib.GnBwdArgs()
    ga.x0, ga.da, ga.gamma, ga.beta, ga.mean, ga.rstd = x.data_ptr(), da.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    ga.dx0, ga.dgamma, ga.dbeta, ga.partial = gx.data_ptr(), plan.gptr["gn.weight"], plan.gptr["gn.bias"], part.data_ptr()
    ga.x0_bs, ga.da_bs, ga.dx0_bs, ga.c0, ga.x0_ld, ga.x1_ld, ga.da_ld, ga.dx0_ld, ga.dx1_ld = P * C, P * C, P * C, C, C, 4, C, C, 4
    ga.Hs, ga.Ws, ga.B, ga.groups, ga.nslab, ga.act, ga.a_mode, ga.acc_dx, ga.partial_ready = H, H, B, G, 1, 1, 0, 0, 1
    plan.bops += [(_lib.OP_IGEMM, ig), (_lib.OP_GN_BWD, ga)]
    # the "device": the statements themselves, rounded to the buffers' types
    da.copy_(bl.conv3x3_input(dy.double().reshape(B, H, H, N), w.double()).reshape(B, P, C))
    args = (gamma.double(), beta.double(), mean.double(), rstd.double())
    part.copy_(bl.gn_tile_partials(x.double(), da.double(), *args, H, H).reshape(-1))
    dx, dg, db = bl.gn_backward(x.double(), da.double(), *args, 1, 0, H, H)
    gx.copy_(dx)
    plan.gview["gn.weight"].copy_(dg)
    plan.gview["gn.bias"].copy_(db)
    led = bl.Ledger(plan)
    assert [L.what.split()[0] for L in led.launches] == ["dgrad3", "gn_bwd"] and led.static_failures() == []
    lines = []
    bad, figs = led.audit(log=lines.append)
    assert not bad and {f[1] for f in figs} == {"da", "gnb_partial", "dx0", "dgamma", "dbeta"} and all(f[3] < 1e-6 for f in figs), lines
    # the rows of the wrong tile order would not pass: swap two images' rows
    part.copy_(part.reshape(B, -1).flip(0).reshape(-1))
    bad, _ = bl.Ledger(plan).audit(log=lines.append)
    assert [b[2] for b in bad] == ["gnb_partial"], bad
    # the other GroupNorm's statistics in the gnb_* fields
    ig.gnb_mean, ig.gnb_rstd = other_mean.data_ptr(), other_rstd.data_ptr()
    rep = bl.Ledger(plan).static_failures()
    assert len(rep) == 1 and "gnb_* fields" in rep[0] and "bops[0]" in rep[0], rep
    # rows nobody consumes
    ga.partial_ready = 0
    assert any("no GroupNorm backward consumes" in r for r in bl.Ledger(plan).static_failures())
