"""CPU: the fp64 statements of tests/forward_ledger.py against stock fp64 torch.nn.functional (and the fused-layer reference of
conv_cases.py), the pointer resolution on strided and offset regions, and the ledger on hand-made op lists over CPU tensors.  The
hand-made list (`Net`) is a small network in the plan's own struct vocabulary -- posemb, the timestep MLP and a BATCHED embedding
projection, a stem with statistics rows, finalize launches over rows and over an fp64 sum, F(4x4,3x3) launches with a GroupNorm
affine, a timestep embedding and a half-resolution residual, a split-K launch with the group-partitioned tail, a pool with its
activated twin, the head -- whose buffers are filled by stock fp64 torch ops rounded to fp32.  The clean list must pass every static
check and every figure; each list with ONE seeded defect must be reported."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
import forward_ledger as fl
from anoddpm_amd import _lib

TOL = 1e-10


def close(got, ref, tol=TOL):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert float((got - ref).abs().max()) <= tol * max(float(ref.abs().max()), 1e-300), float((got - ref).abs().max())


def rnd(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------- statements
CONV = [c for c in cc.SHAPES if c.kind == "igemm" and c.H <= 16] + [c for c in cc.SHAPES if c.res_up or (c.a_mode == 1 and c.cfg == 6)]


@pytest.mark.parametrize("case", CONV, ids=lambda c: cc.case_id((c, "iid", 0)))
@pytest.mark.parametrize("regime", ["iid", "lattice"])
def test_fused_conv_is_the_fused_layer_reference(case, regime):
    """iid: the GroupNorm of the operand is F.group_norm itself (what a fold is held to); lattice: the affine is given as rows."""
    o = cc.operands(case, regime)
    ref, _ = cc.reference(case, o, regime)
    c0 = case.cin[0]
    x = nhwc(o["x"].double())
    affine = None
    if case.gn:
        affine = ("affine", o["scale"].double(), o["shift"].double()) if regime == "lattice" else ("gn", o["gamma"].double(), o["beta"].double(), 32, 1e-5)
    got = fl.fused_conv([x[..., :c0], x[..., c0:]] if case.cin[1] else [x], o["w"].double(), affine=affine, act=o["act"], a_mode=case.a_mode,
                        bias=o["bias"].double(), temb=None if o["temb"] is None else o["temb"].double(),
                        res=None if o["res"] is None else nhwc(o["res"].double()), res_mode=int(case.res_up))
    close(got.permute(0, 3, 1, 2), ref)


def test_group_norm_linear_stem_head_statements():
    x = rnd(3, 64, 5, 7, seed=1) * 2 + 0.7
    g, b = 1 + 0.1 * rnd(64, seed=2), 0.1 * rnd(64, seed=3)
    close(fl.group_norm_nhwc(nhwc(x), g, b), nhwc(F.group_norm(x, 32, g, b, eps=1e-5)))
    close(fl.group_norm_nhwc(nhwc(x).reshape(3, 35, 64), g, b, 16, 1e-3), nhwc(F.group_norm(x, 16, g, b, eps=1e-3)).reshape(3, 35, 64))
    xi, w, bias = rnd(4, 20, seed=4), rnd(12, 20, seed=5), rnd(12, seed=6)
    for ai in (0, 1):
        for ao in (0, 1):
            ref = F.linear(F.silu(xi) if ai else xi, w, bias)
            close(fl.linear(xi, w, bias, ai, ao), F.silu(ref) if ao else ref)
    xs, ws, bs = rnd(2, 3, 6, 8, seed=7), rnd(8, 3, 3, 3, seed=8), rnd(8, seed=9)
    close(fl.stem(xs, ws, bs), nhwc(F.conv2d(xs, ws, bs, padding=1)))
    xh, sc, sh, wh, bh = rnd(2, 16, 6, 8, seed=10), rnd(2, 16, seed=11), rnd(2, 16, seed=12), rnd(3, 16, 3, 3, seed=13), rnd(3, seed=14)
    ref = F.conv2d(F.silu(xh * sc[:, :, None, None] + sh[:, :, None, None]), wh, bh, padding=1)
    close(fl.head(nhwc(xh), sc, sh, wh, bh), ref)
    y = rnd(2, 30, 8, seed=15)
    s, d = fl.chan_sums(y)
    close(s[..., 0], y.sum(1)), close(s[..., 1], (y * y).sum(1)), close(d[..., 0], y.abs().sum(1))
    close(fl.conv_nhwc(nhwc(xh), rnd(5, 16, 1, seed=16)), nhwc(F.conv2d(xh, rnd(5, 16, 1, seed=16)[..., None])))


def test_attention_and_posemb_statements():
    B, L, heads, ch = 2, 24, 2, 8
    C = heads * ch
    qkv = rnd(B, 3 * C, L, seed=21)                                       # UNet.py:137-153 on [B, 3 C, L]
    q, k, v = qkv.reshape(B * heads, 3 * ch, L).split(ch, dim=1)
    s = 1 / math.sqrt(math.sqrt(ch))
    wgt = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
    ref = torch.einsum("bts,bcs->bct", wgt, v).reshape(B, C, L)
    out, p = fl.attention(qkv.permute(0, 2, 1), heads, ch, 1 / math.sqrt(ch))
    close(out.permute(0, 2, 1), ref)
    close(p.reshape(B * heads, L, L), wgt)
    from anoddpm_amd.unet import _posemb_freqs
    t = torch.tensor([0, 1, 17, 500, 999])
    fr = _posemb_freqs(16)
    arg = torch.outer(t * 1, fr)                                          # test_posemb_matches_reference_expression
    assert float((fl.posemb(t, fr, 32) - torch.cat((arg.sin(), arg.cos()), -1).double()).abs().max()) < 1e-6


def test_producer_rows_per_kernel():
    def st(**kw):
        s = _lib.IgemmArgs()
        s.ksplit, s.B = 1, 2
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    assert fl.producer_rows(st(cfg=3, H=64, W=64, ks=3)) == 16 and fl.producer_rows(st(cfg=7, H=32, W=16, ks=3)) == 2
    assert fl.producer_rows(st(cfg=2, H=32, W=32, ks=3)) == 16 and fl.producer_rows(st(cfg=6, H=32, W=32, ks=3)) == 16
    assert fl.producer_rows(st(cfg=0, H=64, W=64, ks=3)) == 2 * 2 * 16 and fl.producer_rows(st(cfg=1, H=8, W=8, ks=3)) == 2
    assert fl.producer_rows(st(cfg=1, H=4, W=4, ks=3)) == 2 and fl.producer_rows(st(cfg=1, H=10, W=10, ks=1)) == 4
    assert fl.producer_rows(st(cfg=1, H=8, W=8, ks=3, ksplit=4, stats_rows=5)) == 5
    assert fl.producer_rows(st(cfg=5, H=8, W=8, ks=1, c0=64, N=64), smallmap_tile=lambda *a: 2 * 16 + 4) == 2


# ---------------------------------------------------------------------------------------------------- pointers
def test_span_map_on_strided_and_offset_regions():
    am = fl.SpanMap()
    big = torch.arange(4 * 6 * 10, dtype=torch.float32).reshape(4, 6, 10)
    am.add(big, "big")
    am.add(big[0], "row0")                                   # a kept view of the same storage: smaller, holds the first bytes only
    p0 = big.data_ptr()
    r = am.region(p0 + 4 * 3, (4, 6, 2), (60, 10, 1), "cols 3..4")          # a column range at an offset: past row0, inside big
    assert r.tensor is big and r.off == 3
    assert torch.equal(r.read(), big[:, :, 3:5].double())
    assert am.region(p0, (6, 10), (10, 1), "first").tensor.data_ptr() == p0 and am.region(p0, (6, 10), (10, 1), "first").name.endswith("row0")
    h = am.region(p0 + 4 * 5, (4, 2, 3, 5), (60, 30, 10, 1), "heads")       # [B][heads][rows][cols] at a column offset
    assert torch.equal(h.read(), big.reshape(4, 2, 3, 10)[..., 5:].double())
    with pytest.raises(fl.LedgerError, match="past the end"):
        am.region(p0 + 4 * 3, (4, 6, 8), (60, 10, 1), "one column too many")
    with pytest.raises(fl.LedgerError, match="no tensor"):
        am.region(p0 + 4 * big.numel(), (1,), (1,), "behind")
    with pytest.raises(fl.LedgerError, match="null"):
        am.region(None, (1,), (1,), "null")
    with pytest.raises(fl.LedgerError, match="aligned"):
        am.region(p0 + 2, (1,), (1,), "odd")
    d = torch.zeros(8, dtype=torch.float64)
    am.add(d, "doubles")
    assert am.region(d.data_ptr() + 16, (2, 3), (3, 1), "fp64").off == 2


# ---------------------------------------------------------------------------------------------------- a hand-made list
B, S, C, BASE, TED = 2, 16, 64, 32, 64


class Net:
    """See the module docstring.  Every buffer is computed by stock fp64 torch ops on the fp32 contents of its inputs and rounded
    to fp32, as a device launch would leave it."""

    def __init__(self, perturb=None):
        g = torch.Generator().manual_seed(3)
        self.perturb = perturb                                # a tensor's name: its producer stores a wrong block, everything after reads it
        self.keep, self.ops, self.packs, self.named = [], [], {}, {}

        def par(name, *shape, scale=1.0, shift=0.0):
            self.named[name] = (torch.randn(*shape, generator=g) * scale + shift).float()
            return self.named[name]
        for blk in ("blkA", "blkB"):
            par(f"{blk}.embed_layers.1.weight", C, TED, scale=TED ** -0.5), par(f"{blk}.embed_layers.1.bias", C, scale=0.1)
        par("time_embedding.1.weight", TED, BASE, scale=BASE ** -0.5), par("time_embedding.1.bias", TED, scale=0.1)
        par("stem.weight", C, 1, 3, 3, scale=0.3), par("stem.bias", C, scale=0.1)
        for n in ("blkB.in_layers.0", "blkB.out_layers.0", "out.0"):
            par(n + ".weight", C, scale=0.1, shift=1.0), par(n + ".bias", C, scale=0.1)
        par("blkB.in_layers.2.weight", C, C, 3, 3, scale=(9 * C) ** -0.5), par("blkB.in_layers.2.bias", C, scale=0.1)
        par("blkB.out_layers.3.weight", C, C, 3, 3, scale=(9 * C) ** -0.5), par("blkB.out_layers.3.bias", C, scale=0.1)
        par("proj.weight", 128, C, 1, scale=C ** -0.5), par("proj.bias", 128, scale=0.1)
        par("out.0b.weight", 128, scale=0.1, shift=1.0), par("out.0b.bias", 128, scale=0.1)
        par("out.2.weight", 1, 128, 3, 3, scale=(9 * 128) ** -0.5), par("out.2.bias", 1, scale=0.1)
        self.x = (torch.rand(B, 1, S, S, generator=g) * 2 - 1).float()
        self.t = torch.tensor([17, 640])
        self._build()

    # -- helpers
    def buf(self, *shape, dtype=torch.float32):
        t = torch.full(shape, float("nan"), dtype=dtype)
        self.keep.append(t)
        return t

    def copy(self, key):
        t = self.named[key].clone().reshape(-1)
        self.keep.append(t)
        self.packs[t.data_ptr()] = (key, fl.PACK["copy"], t.numel())
        return t.data_ptr()

    def pack(self, key, kind, taps):
        w = self.named[key]
        t = torch.zeros(taps * w.shape[0] * w.shape[1])      # the packed layout itself is the packer's business (kept by the poison step)
        self.keep.append(t)
        self.packs[t.data_ptr()] = (key, fl.PACK[kind], t.numel())
        return t.data_ptr()

    def add(self, code, st):
        self.ops.append((code, st))
        return st

    def d(self, key):
        return self.named[key].double()

    def conv(self, src, wkey, out, *, gn=None, temb=None, temb_ld=0, res=None, res_mode=0, cfg=3, ksplit=1, ks=3, kind="wino43", taps=36):
        st = _lib.IgemmArgs()
        N, K = self.named[wkey].shape[:2]
        P = S * S
        st.a0, st.c0, st.a0_ld, st.a0_bs = src.data_ptr(), K, K, P * K
        st.H, st.W, st.ks, st.N, st.B, st.heads, st.alpha, st.cfg, st.ksplit = S, S, ks, N, B, 1, 1.0, cfg, ksplit
        st.bmat, st.bias = self.pack(wkey, kind, taps), self.copy(wkey[:-7] + ".bias")
        st.out, st.out_ld, st.o_bs = out.data_ptr(), N, P * N
        if gn is not None:
            st.gn_scale, st.gn_shift, st.gn_ld, st.act = gn[0].data_ptr(), gn[1].data_ptr(), K, 1
        if temb is not None:
            st.temb, st.temb_ld = temb, temb_ld
        if res is not None:
            st.res, st.res_mode, st.res_ld, st.r_bs = res.data_ptr(), res_mode, N, (P // 4 if res_mode else P) * N
        return self.add(_lib.OP_IGEMM, st)

    def finalize(self, stats, rows, fmt, prefix, Cn, P):
        st = _lib.GnFinalizeArgs()
        st.stats0, st.rows0, st.fmt0, st.c0, st.c1, st.P, st.B, st.groups, st.eps = stats.data_ptr(), rows, fmt, Cn, 0, P, B, 32, 1e-5
        st.gamma, st.beta = self.copy(prefix + ".weight"), self.copy(prefix + ".bias")
        sc, sh = self.buf(B, Cn), self.buf(B, Cn)
        st.scale, st.shift = sc.data_ptr(), sh.data_ptr()
        self.add(_lib.OP_GN_FINALIZE, st)
        return st, sc, sh

    @staticmethod
    def affine(x, gamma, beta):
        """fp32 rows scale, shift of GroupNorm(32) over x [B, P, C] (fp64 fold of the sums, as the finalize kernel)"""
        sc, sh = cc._group_affine(x.double().permute(0, 2, 1), gamma, beta)
        return sc.float(), sh.float()

    @staticmethod
    def rows(y, rows):
        """[B, rows, C, 2]: fp32 partial sums of y [B, P, C] over `rows` contiguous pixel ranges"""
        yy = y.double().reshape(y.shape[0], rows, -1, y.shape[2])
        return torch.stack([yy.sum(2), (yy * yy).sum(2)], dim=-1).float()

    def layer(self, x, sc, sh, wkey, temb=None, res=None):
        """stock fp64: silu(x * scale + shift) -> conv2d -> + bias + temb + res; x [B, P, K] -> [B, P, N] fp32"""
        Bn, P, K = x.shape
        h = F.silu(x.double() * sc.double()[:, None, :] + sh.double()[:, None, :]).reshape(Bn, S, S, K).permute(0, 3, 1, 2)
        w = self.d(wkey)
        y = F.conv2d(h, w if w.dim() == 4 else w[..., None], self.d(wkey[:-7] + ".bias"), padding=w.shape[2] // 2 if w.dim() == 4 else 0)
        if temb is not None:
            y = y + temb.double()[:, :, None, None]
        if res is not None:
            y = y + res
        return nhwc(y).reshape(Bn, P, -1).float()

    # -- the list
    def _build(self):
        P = S * S
        from anoddpm_amd.unet import _posemb_freqs
        self.freqs = _posemb_freqs(BASE // 2).float()
        self.keep.append(self.freqs)
        pe = self.buf(B, BASE)
        st = self.posemb = _lib.PosembArgs()
        st.t, st.freqs, st.out, st.B, st.dim, st.scale = self.t.data_ptr(), self.freqs.data_ptr(), pe.data_ptr(), B, BASE, 1.0
        self.add(_lib.OP_POSEMB, st)
        arg = torch.outer(self.t.float(), self.freqs)
        pe.copy_(torch.cat([arg.double().sin(), arg.double().cos()], 1))
        # time MLP (one layer) and the batched projection of two blocks
        h1 = self.buf(B, TED)
        st = _lib.LinearArgs()
        st.inp, st.w, st.bias, st.out = pe.data_ptr(), self.copy("time_embedding.1.weight"), self.copy("time_embedding.1.bias"), h1.data_ptr()
        st.B, st.K, st.N, st.act_in, st.act_out = B, BASE, TED, 0, 1
        self.add(_lib.OP_LINEAR, st)
        h1.copy_(F.silu(F.linear(pe.double(), self.d("time_embedding.1.weight"), self.d("time_embedding.1.bias"))))
        w_all, b_all = torch.zeros(2 * C, TED), torch.zeros(2 * C)
        self.keep += [w_all, b_all]
        for j, blk in enumerate(("blkA", "blkB")):
            for dst, key in ((w_all[j * C:(j + 1) * C], f"{blk}.embed_layers.1.weight"), (b_all[j * C:(j + 1) * C], f"{blk}.embed_layers.1.bias")):
                dst.copy_(self.named[key])
                self.keep.append(dst)
                self.packs[dst.data_ptr()] = (key, fl.PACK["copy"], dst.numel())
        self.emb = emb = self.buf(B, 2 * C)
        st = _lib.LinearArgs()
        st.inp, st.w, st.bias, st.out = h1.data_ptr(), w_all.data_ptr(), b_all.data_ptr(), emb.data_ptr()
        st.B, st.K, st.N, st.act_in, st.act_out = B, TED, 2 * C, 1, 0
        self.add(_lib.OP_LINEAR, st)
        emb.copy_(F.linear(F.silu(h1.double()), w_all.double(), b_all.double()))
        # stem with two statistics rows
        self.h0 = h0 = self.buf(B, P, C)
        self.s0 = s0 = self.buf(B, 2, C, 2)
        st = self.stem = _lib.StemArgs()
        st.x, st.w, st.bias, st.out = self.x.data_ptr(), self.pack("stem.weight", "small", 9), self.copy("stem.bias"), h0.data_ptr()
        st.B, st.H, st.W, st.Cin, st.Cout, st.stats, st.stats_rows = B, S, S, 1, C, s0.data_ptr(), 2
        self.add(_lib.OP_STEM, st)
        h0.copy_(nhwc(F.conv2d(self.x.double(), self.d("stem.weight"), self.d("stem.bias"), padding=1)).reshape(B, P, C))
        s0.copy_(self.rows(h0, 2))
        # pool with its activated twin needs an affine of h0: finalize over the stem rows
        self.fin1, sc1, sh1 = self.finalize(s0, 2, 0, "blkB.in_layers.0", C, P)
        a, b_ = self.affine(h0, self.d("blkB.in_layers.0.weight"), self.d("blkB.in_layers.0.bias"))
        sc1.copy_(a), sh1.copy_(b_)
        self.half = half = self.buf(B, P // 4, C)
        half_act = self.buf(B, P // 4, C)
        st = _lib.ResampleArgs()
        st.inp, st.out, st.B, st.H, st.W, st.C, st.mode = h0.data_ptr(), half.data_ptr(), B, S, S, C, 2
        st.gn_scale, st.gn_shift, st.out_act = sc1.data_ptr(), sh1.data_ptr(), half_act.data_ptr()
        self.add(_lib.OP_RESAMPLE, st)
        x4 = h0.double().reshape(B, S, S, C).permute(0, 3, 1, 2)
        half.copy_(nhwc(F.avg_pool2d(x4, 2, 2)).reshape(B, P // 4, C))
        half_act.copy_(nhwc(F.avg_pool2d(F.silu(x4 * sc1.double()[:, :, None, None] + sh1.double()[:, :, None, None]), 2, 2)).reshape(B, P // 4, C))
        # ResBlock B: first convolution with ITS embedding columns (block 1 of 2), F(4x4) statistics: one row
        self.h1c = h1c = self.buf(B, P, C)
        self.s1 = s1 = self.buf(B, 1, C, 2)
        self.conv1 = self.conv(h0, "blkB.in_layers.2.weight", h1c, gn=(sc1, sh1), temb=emb.data_ptr() + 4 * C, temb_ld=2 * C)
        self.conv1.stats = s1.data_ptr()
        h1c.copy_(self.layer(h0, sc1, sh1, "blkB.in_layers.2.weight", temb=emb[:, C:]))
        s1.copy_(self.rows(h1c, 1))
        self.fin2, sc2, sh2 = self.finalize(s1, 1, 0, "blkB.out_layers.0", C, P)
        a, b_ = self.affine(h1c, self.d("blkB.out_layers.0.weight"), self.d("blkB.out_layers.0.bias"))
        sc2.copy_(a), sh2.copy_(b_)
        # second convolution: the half-resolution tensor as residual, repeated 2 x 2 on the read
        self.h2 = h2 = self.buf(B, P, C)
        self.conv2 = self.conv(h1c, "blkB.out_layers.3.weight", h2, gn=(sc2, sh2), res=half, res_mode=1)
        up = F.interpolate(half.double().reshape(B, S // 2, S // 2, C).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
        h2.copy_(self.layer(h1c, sc2, sh2, "blkB.out_layers.3.weight", res=up))
        # a plain 1x1 projection with split-K and the group-partitioned tail: fp64 sums
        self.h3 = h3 = self.buf(B, P, 128)
        self.cs = cs = self.buf(B, 128, 2, dtype=torch.float64)
        ws = self.buf(2 * B * P * 128)
        self.proj = st = self.conv(h2, "proj.weight", h3, cfg=1, ksplit=2, ks=1, kind="conv1", taps=1)
        st.ws, st.tail_csum, st.tail_groups, st.tail_eps = ws.data_ptr(), cs.data_ptr(), 32, 1e-5
        y = F.conv2d(h2.double().reshape(B, S, S, C).permute(0, 3, 1, 2), self.d("proj.weight")[..., None], self.d("proj.bias"))
        h3.copy_(nhwc(y).reshape(B, P, 128))
        if self.perturb == "h3":
            h3[1, :, 64:128] *= 1 + 1e-3                      # one 64-channel block of one image
        cs.copy_(torch.stack([h3.double().sum(1), (h3.double() ** 2).sum(1)], dim=-1))
        self.fin3, sc3, sh3 = self.finalize(cs, 1, 1, "out.0b", 128, P)
        a, b_ = self.affine(h3, self.d("out.0b.weight"), self.d("out.0b.bias"))
        sc3.copy_(a), sh3.copy_(b_)
        # head
        self.y = yb = self.buf(B, 1, S, S)
        st = _lib.HeadArgs()
        st.x, st.w, st.bias = h3.data_ptr(), self.pack("out.2.weight", "small", 9), self.copy("out.2.bias")
        st.gn_scale, st.gn_shift, st.out, st.B, st.H, st.W, st.C, st.Cout = sc3.data_ptr(), sh3.data_ptr(), yb.data_ptr(), B, S, S, 128, 1
        self.add(_lib.OP_HEAD, st)
        hh = F.silu(h3.double() * sc3.double()[:, None, :] + sh3.double()[:, None, :]).reshape(B, S, S, 128).permute(0, 3, 1, 2)
        yb.copy_(F.conv2d(hh, self.d("out.2.weight"), self.d("out.2.bias"), padding=1))

    def ledger(self):
        return fl.ForwardLedger(fl.PlanView(self.ops, self.keep, self.named, self.packs, self.x, self.t))


def report(net):
    led = net.ledger()
    static = led.static_failures()
    fails, figs = led.audit(log=lambda s: None) if not led.undescribed else ([], [])
    return led, static, fails, figs


def test_clean_list_passes():
    net = Net()
    led, static, fails, figs = report(net)
    assert not static and not fails, (static, fails)
    assert sum(len(L.idx) for L in led.launches) == len(net.ops) and len(figs) >= len(net.ops)
    assert max(f[3] for f in figs) < 1e-6                    # buffers rounded once to fp32
    assert {"res_mode 1", "pool_act double output", "batched embedding projection", "statistics: stem rows", "statistics: csum",
            "finalize fmt 1", "finalize fmt 0", "OP_HEAD", "shared split-K workspace"} <= led.routes


def _one_row_more(n):
    n.fin1.rows0 = 3                                         # the stem wrote two rows per image


def _fmt0_on_fp64(n):
    n.fin3.fmt0, n.fin3.rows0 = 0, 1


def _stats_of_another_tensor(n):
    """the first convolution's affine from the statistics of a DIFFERENT tensor of the same shape: a second stem-like tensor"""
    other, rows = n.buf(B, S * S, C), n.buf(B, 2, C, 2)
    st = _lib.ChanStatsArgs()
    st.a, st.stats, st.a_bs, st.C, st.a_ld, st.P, st.B, st.nslab = other.data_ptr(), rows.data_ptr(), S * S * C, C, C, S * S, B, 2
    cp = _lib.ResampleArgs()                                 # (a writer for `other`, so that only the wiring is wrong)
    cp.inp, cp.out, cp.B, cp.H, cp.W, cp.C, cp.mode = n.half.data_ptr(), other.data_ptr(), B, S // 2, S // 2, C, 1
    other.copy_(fl.resample(n.half.double().reshape(B, S // 2, S // 2, C), 1).reshape(B, S * S, C))
    rows.copy_(n.rows(other, 2))
    i = n.ops.index((_lib.OP_GN_FINALIZE, n.fin2))
    n.ops[i:i] = [(_lib.OP_RESAMPLE, cp), (_lib.OP_CHAN_STATS, st)]
    n.fin2.stats0, n.fin2.rows0 = rows.data_ptr(), 2


def _missing_temb(n):
    n.conv1.temb = None


def _temb_ld_of_one_block(n):
    n.conv1.temb_ld = C


def _res_mode0_on_half_resolution(n):
    n.conv2.res_mode = 0


def _reader_before_writer(n):
    i = n.ops.index((_lib.OP_IGEMM, n.conv2))
    n.ops[i], n.ops[i - 1] = n.ops[i - 1], n.ops[i]          # the convolution ahead of the finalize that writes its affine


def _perturbed_block(n):
    pass                                                     # Net(perturb="h3"): seeded while the list is built


def _perturbed_statistics(n):
    n.s1[0, 0, 5, 1] *= 1 + 1e-4


def _workspace_too_small(n):
    n.proj.ksplit = 3


def _embedding_columns_of_the_other_block(n):
    n.conv1.temb = n.emb.data_ptr()


def _output_over_an_input(n):
    n.conv2.out = n.h1c.data_ptr()


DEFECTS = [(_one_row_more, "static", "rows"), (_fmt0_on_fp64, "static", "format"), (_stats_of_another_tensor, "static", "normalises"),
           (_missing_temb, "static", "temb missing"), (_temb_ld_of_one_block, "static", "pitch"),
           (_res_mode0_on_half_resolution, "static", "past the end"), (_reader_before_writer, "static", "earlier finalize|does not come first|LATER"),
           (_perturbed_block, "figure", "igemm"), (_perturbed_statistics, "figure", "igemm"), (_workspace_too_small, "static", "past the end"),
           (_embedding_columns_of_the_other_block, "static", "column"), (_output_over_an_input, "static", "overlaps its input|write the same")]


@pytest.mark.parametrize("defect,where,match", DEFECTS, ids=[d[0].__name__.lstrip("_") for d in DEFECTS])
def test_seeded_defect_is_reported(defect, where, match):
    import re
    net = Net(perturb="h3" if defect is _perturbed_block else None)
    defect(net)
    led, static, fails, figs = report(net)
    if where == "static":
        assert any(re.search(match, s) for s in static), static
    else:
        assert not static, static
        assert len(fails) >= 1 and all(re.search(match, f[0]) for f in fails), fails
        if defect is _perturbed_block:
            # the perturbed output itself, and nothing upstream of it; its consumers read the perturbed buffer and stay clean
            assert [(f[0].split()[0], f[2], f[5]) for f in fails] == [("igemm", "out", (1, 64))], fails
            assert 2e-4 < fails[0][3] < 2e-3


def test_a_real_plan_built_over_host_buffers_passes_the_static_checks(monkeypatch):
    """The smallest plan of tests/test_gpu_forward_ledger.py, built from its structs alone (nothing is launched): every pointer
    resolves, every launch has a statement, no static check fails, and the routes it is listed for are there."""
    import test_gpu_forward_ledger as gpu
    routes = gpu._routes_from_structs("i32_b2", monkeypatch)
    assert {"fold: rows", "tail-attached GroupNorm", "batched embedding projection", "shared split-K workspace"} <= routes
