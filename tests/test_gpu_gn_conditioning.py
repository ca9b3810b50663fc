"""-m gpu: every fused GroupNorm statistics route on off-centre and near-constant activations (tests/gn_cases.py).

Every route builds var = Q / n - mean^2 from per-channel {sum, sum of squares} partials, most of them accumulated in fp32 before the
fp64 fold; an error d in Q becomes (1 + r^2) d in the variance, r = |mean| / sqrt(var + eps).  The rest of the suite feeds centred
operands (r < 1).  Here every case of gn_cases.CASES -- r in {0, 4, 16, 64} at std 1 and at std 1e-3, all zeros, constant 1.0, one
constant group, one blank image -- goes through every route, and x * scale + shift is compared with fp64 F.group_norm OF THE
TENSOR THE KERNEL ITSELF WROTE (the contraction's own error stays out of the figure), per image and per group.  Where a route
emits mean / rstd they are checked the same way and fed to anoddpm_gn_silu_backward, whose dx / dgamma / dbeta are compared with
fp64 autograd of silu(group_norm(x)) at the same bars.  A prologue fold has no scale / shift to read: its consumer (identity
weights) is compared with the same launch on the fp64 host affine of the same operand.

Bars (gn_cases.BARS, the project's own): 2e-5 up to r = 4, 5e-5 at r = 16 (the measured blank slice, 14.25), 1e-3 at r = 64 and
for exactly constant groups (r = 316); all zeros: scale * 0 + shift == beta bit for bit; every result finite.  Every figure is
printed before anything is asserted; a route asserts once, with every case beyond its bar listed.

Worst measured figure per route (MI355X), by bar:
not measured yet -- the module prints this table (route x bar) when it finishes.
"""

import pytest
import torch
import torch.nn.functional as F

import gn_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LEDGER = {}


@pytest.fixture(scope="module", autouse=True)
def ledger_report():
    yield
    tags = sorted({t for t, _ in LEDGER})
    print("\n" + f"{'route':66s}" + "".join(f"{c + ' (' + b + ')':>16s}" for c, b in zip(gc.COLUMNS, ("2e-5", "5e-5", "1e-3", "1e-3"))))
    for t in tags:
        print(f"{t:66s}" + "".join(f"{LEDGER[(t, c)]:16.1e}" if (t, c) in LEDGER else f"{'-':>16s}" for c in gc.COLUMNS))


def d(t):
    return t.to(DEV)


def split(x, c0):
    """NCHW cpu -> NHWC device sources [.., :c0], [.., c0:]."""
    import hipops
    xs = hipops.nhwc(d(x))
    return [xs] if c0 >= x.shape[1] else [xs[..., :c0].contiguous(), xs[..., c0:].contiguous()]


def check_affine(tag, name, srcs, gamma, beta, sc, sh, fails, mean=None, rstd=None, backward=False):
    """srcs: the NHWC device tensors the statistics are of (what the kernel read or wrote).  Returns nothing; figures are printed,
    failures appended."""
    import hipops
    xs = torch.cat(srcs, dim=3) if len(srcs) > 1 else srcs[0]
    x = hipops.nchw(xs).cpu()
    ref = gc.reference(x, gamma, beta)
    got = hipops.nchw(xs * sc[:, None, None, :] + sh[:, None, None, :]).cpu()
    gc.failures(tag, name, got, ref, fails, LEDGER)
    if gc.CASES[name][0] == "zeros" and not torch.equal(got, beta[None, :, None, None].expand_as(got)):
        fails.append(f"{tag} zeros: scale * 0 + shift is not beta bit for bit")
    if mean is None:
        return
    gc.failures(tag + " | mean, rstd", name, gc.normalised(x, mean.cpu(), rstd.cpu(), gamma, beta), ref, fails, LEDGER)
    if not backward:
        return
    B = x.shape[0]
    gen = torch.Generator().manual_seed(77)
    da = torch.randn(x.shape, generator=gen) * (1 + 0.15 * torch.arange(B, dtype=torch.float32))[:, None, None, None]
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    F.silu(F.group_norm(xd, gc.GROUPS, gd, bd, eps=gc.EPS)).backward(da.double())
    dx, dgamma, dbeta = hipops.gn_silu_backward(srcs, hipops.nhwc(d(da)).contiguous(), d(gamma), d(beta), mean, rstd, act=1)
    gc.failures(tag + " | backward dx", name, hipops.nchw(torch.cat(dx, dim=3)).cpu(), xd.grad, fails, LEDGER)
    summed = gc.bars(name, B).amax(0, keepdim=True)                      # dgamma / dbeta sum over the images
    gc.failures(tag + " | backward dgamma", name, dgamma.cpu()[None, :, None], gd.grad[None, :, None], fails, LEDGER, bar=summed)
    gc.failures(tag + " | backward dbeta", name, dbeta.cpu()[None, :, None], bd.grad[None, :, None], fails, LEDGER, bar=summed)


def conclude(fails):
    assert not fails, f"{len(fails)} beyond their bar:\n" + "\n".join(fails)


# ------------------------------------------------------------------------------------------- stand-alone fp64 (anoddpm_gn_stats)
@pytest.mark.parametrize("shape", [(2, 64, 0, 32), (2, 128, 0, 32), (2, 256, 128, 16), (3, 64, 0, 20)],
                         ids=["c64", "c128", "concat256+128", "ragged"])
def test_standalone_fp64(shape):
    """gn_partial_kernel (fp64 from the first add) -> gn_finalize_kernel: one and two sources (256 + 128: 12 channels per group,
    a group straddles the sources), nslab None / 1 / 3 (3: ragged slabs; 20 x 20 pixels: ragged everywhere)."""
    import hipops
    B, c0, c1, H = shape
    C = c0 + c1
    gamma, beta = gc.affine(C)
    fails = []
    for name in gc.CASES:
        srcs = split(gc.operand(name, B, C, H, H), c0)
        for nslab in (None, 1, 3):
            sc, sh = hipops.gn_affine(srcs, d(gamma), d(beta), nslab=nslab)
            check_affine(f"gn_stats fp64 C={c0}+{c1} {H}x{H} nslab={nslab}", name, srcs, gamma, beta, sc, sh, fails)
    conclude(fails)


# ------------------------------------------------------------------------------------------- fp32 channel rows (anoddpm_chan_stats)
def plan_nslab(P, C):
    return max(1, min(128, (P * (C // 4)) // 4096))                    # unet._Plan.chan_stats


@pytest.mark.parametrize("shape", [(2, 64, 32), (2, 128, 32), (3, 64, 20), (2, 128, 64)], ids=["c64", "c128", "ragged", "c128_64x64"])
def test_chan_stats_rows(shape):
    """chan_stats_kernel (an fp32 chain of P / nslab / R pixels per thread, R fp32 partials per channel) -> gn_finalize, with the
    plan's slab count and with 3 ragged slabs; mean / rstd out and through the backward."""
    import hipops
    B, C, H = shape
    gamma, beta = gc.affine(C)
    fails = []
    for name in gc.CASES:
        srcs = split(gc.operand(name, B, C, H, H), C)
        for nslab in (plan_nslab(H * H, C), 3):
            st = hipops.chan_stats(srcs[0], nslab)
            sc, sh, mean, rstd = hipops.gn_finalize([st], d(gamma), d(beta), H * H, want_mean_rstd=True)
            check_affine(f"chan_stats C={C} {H}x{H} nslab={nslab}", name, srcs, gamma, beta, sc, sh, fails, mean, rstd,
                         backward=(H == 32 and nslab != 3))
    conclude(fails)


def test_chan_stats_rows_as_second_source_of_a_concat():
    """Virtual concat (256, 128), 12 channels per group, a group straddles the sources: each source its own rows (other counts)."""
    import hipops
    B, c0, c1, H = 2, 256, 128, 16
    gamma, beta = gc.affine(c0 + c1)
    fails = []
    for name in gc.CASES:
        srcs = split(gc.operand(name, B, c0 + c1, H, H), c0)
        st = [hipops.chan_stats(srcs[0], plan_nslab(H * H, c0)), hipops.chan_stats(srcs[1], 3)]
        sc, sh, mean, rstd = hipops.gn_finalize(st, d(gamma), d(beta), H * H, want_mean_rstd=True)
        check_affine("chan_stats concat 256+128 16x16", name, srcs, gamma, beta, sc, sh, fails, mean, rstd, backward=True)
    conclude(fails)


# ------------------------------------------------------------------------------------------- stem rows
@pytest.mark.parametrize("shape", [(2, 64, 32), (2, 128, 64), (3, 32, 64)], ids=["c64_32x32", "c128_64x64", "c32_64x64"])
def test_stem_rows(shape):
    """anoddpm_conv_stem's own rows (fp32 over a workgroup's pixel range) -> gn_finalize.  Cout 32: 1 channel per group, the
    GroupNorm in which the blank slice reaches r = 14."""
    import hipops
    B, N, H = shape
    gamma, beta = gc.affine(N)
    fails = []
    for name in gc.CASES:
        x, w, b = gc.stem_operand(name, B, N, H)
        out, st = hipops.stem(d(x), d(w), d(b), with_stats=True)
        assert st is not None and st.shape[1] > 1
        sc, sh, mean, rstd = hipops.gn_finalize([st], d(gamma), d(beta), H * H, want_mean_rstd=True)
        check_affine(f"stem rows Cout={N} {H}x{H} rows={st.shape[1]}", name, [out], gamma, beta, sc, sh, fails, mean, rstd,
                     backward=(H == 32))
    conclude(fails)


# ------------------------------------------------------------------------------------------- contraction epilogue rows
EPILOGUE = [
    # id, cfg, f43 variant, B, Cin, N, H, ks
    ("igemm128_3x3", 0, 0, 2, 32, 128, 32, 3),
    ("igemm128_3x3_c64", 0, 0, 2, 32, 64, 32, 3),
    ("igemm128_1x1_ragged", 0, 0, 2, 32, 128, 24, 1),         # 576 pixels: 4.5 row tiles of 128
    ("igemm64_3x3", 1, 0, 2, 32, 64, 32, 3),
    ("igemm64_3x3_c128", 1, 0, 2, 32, 128, 32, 3),
    ("igemm64_1x1_ragged", 1, 0, 3, 32, 64, 20, 1),           # 400 pixels: 6.25 row tiles of 64
    ("f22", 2, 0, 2, 32, 128, 32, 3),
    ("f22_c64", 2, 0, 2, 32, 64, 32, 3),
    ("f43_auto", 3, 0, 2, 32, 128, 32, 3),
    ("f43_auto_c64", 3, 0, 2, 32, 64, 32, 3),
    ("f43_channel_sliced", 3, 3, 2, 32, 128, 32, 3),
    ("f43_wave_per_simd", 3, 6, 2, 32, 128, 32, 3),
    ("f43_wave_per_simd_tsplit", 3, 7, 2, 32, 128, 32, 3),
    ("f43_auto_64x64", 3, 0, 2, 32, 128, 64, 3),
    ("smallmap_3x3", 5, 0, 2, 32, 64, 16, 3),
    ("smallmap_1x1_c128", 5, 0, 2, 32, 128, 16, 1),
    ("wino23s_c128", 6, 0, 2, 64, 128, 32, 3),
    ("wino23s_c64", 6, 0, 4, 64, 64, 32, 3),
    ("bf16split3", 7, 0, 2, 32, 128, 32, 3),
]


def produce(name, cfg, variant, B, Cin, N, H, ks, ctot=None, seed=0, **kw):
    """One producer launch on the case's convolution operand -> (NHWC output on the device, whatever kw collects)."""
    import hipops
    from anoddpm_amd._lib import lib
    x, w, b, temb = gc.conv_operand(name, B, Cin, N, H, ks, seed=seed, ctot=ctot)
    lib().anoddpm_internal_variant(5, variant)
    try:
        return hipops.conv_igemm([hipops.nhwc(d(x))], d(w), d(b), Hout=H, ks=ks, temb=d(temb), cfg=cfg, **kw)
    finally:
        lib().anoddpm_internal_variant(5, 0)


@pytest.mark.parametrize("route", EPILOGUE, ids=[r[0] for r in EPILOGUE])
def test_epilogue_rows(route):
    """conv_igemm(..., stats_out=) -> gn_finalize for every contraction that writes rows: the 128- and 64-row implicit GEMM (3x3
    and 1x1 with a ragged last row tile), F(2x2,3x3), F(4x4,3x3) in all its workgroup forms, the small-map kernel, the no-split-K
    F(2x2,3x3) and the split-bf16 F(4x4,3x3)."""
    import hipops
    rid, cfg, variant, B, Cin, N, H, ks = route
    gamma, beta = gc.affine(N)
    fails = []
    for name in gc.CASES:
        st = []
        out = produce(name, cfg, variant, B, Cin, N, H, ks, stats_out=st)
        assert st[0].shape[1] > 1
        sc, sh, mean, rstd = hipops.gn_finalize(st, d(gamma), d(beta), H * H, want_mean_rstd=True)
        check_affine(f"epilogue rows {rid} N={N} {H}x{H} rows={st[0].shape[1]}", name, [out], gamma, beta, sc, sh, fails, mean, rstd,
                     backward=(rid in ("igemm64_3x3", "f43_auto", "smallmap_3x3")))
    conclude(fails)


# ------------------------------------------------------------------------------------------- split-K tails
@pytest.mark.parametrize("route", [(1, 64, 64, 16), (1, 64, 128, 32), (2, 64, 128, 32), (3, 64, 128, 32)],
                         ids=["igemm64_16x16", "igemm64_32x32", "f22", "f43"])
def test_splitk_rows(route):
    """ksplit 2 with stats_out: the slab tail sums the slices and writes 3 (ragged) rows per image."""
    import hipops
    cfg, Cin, N, H = route
    gamma, beta = gc.affine(N)
    fails = []
    for name in gc.CASES:
        st = []
        out = produce(name, cfg, 0, 2, Cin, N, H, 3, ksplit=2, stats_out=st)
        sc, sh, mean, rstd = hipops.gn_finalize(st, d(gamma), d(beta), H * H, want_mean_rstd=True)
        check_affine(f"split-K rows cfg={cfg} N={N} {H}x{H}", name, [out], gamma, beta, sc, sh, fails, mean, rstd)
    conclude(fails)


@pytest.mark.parametrize("route", [(2, 128, 128, 0, 16), (1, 128, 128, 0, 8), (2, 128, 256, 128, 16)],
                         ids=["f22_alone", "igemm64_alone", "f22_concat256+128"])
def test_splitk_gn_tail(route):
    """The group-partitioned split-K tail: fp64 per-channel sums (tail_csum), the consumer GroupNorm over [out] or over the
    virtual concat [out, other] (other_csum; 256 + 128: a group straddles), mean / rstd out and through the backward; and
    anoddpm_gn_finalize on the same fp64 sums (fmt 1), the launch a second consumer of the tensor takes."""
    import hipops
    cfg, Cin, N, c1, H = route
    B, C = 2, N + c1
    gamma, beta = gc.affine(C)
    fails = []
    for name in gc.CASES:
        other = other_csum = None
        if c1:
            other = hipops.nhwc(d(gc.operand(name, B, C, H, H, mean_scale=1.05)[:, N:])).contiguous()
            of = other.double().reshape(B, -1, c1)
            other_csum = torch.stack([of.sum(1), (of * of).sum(1)], dim=-1).contiguous()
        tail = dict(gamma=d(gamma), beta=d(beta), other_csum=other_csum, want_mean=True)
        out = produce(name, cfg, 0, B, Cin, N, H, 3, ctot=C, ksplit=2, gn_tail=tail)
        srcs = [out] + ([other] if c1 else [])
        tag = f"split-K gn_tail cfg={cfg} C={N}+{c1} {H}x{H}"
        check_affine(tag, name, srcs, gamma, beta, tail["scale"], tail["shift"], fails, tail["mean"], tail["rstd"], backward=True)
        st = [tail["csum"]] + ([other_csum] if c1 else [])
        sc, sh, mean, rstd = hipops.gn_finalize(st, d(gamma), d(beta), H * H, want_mean_rstd=True, fmts=(1, 1))
        check_affine(tag + " -> gn_finalize(fp64 sums)", name, srcs, gamma, beta, sc, sh, fails, mean, rstd)
    conclude(fails)


# ------------------------------------------------------------------------------------------- prologue folds
def host_affine(srcs, gamma, beta):
    """The exact affine of the operand: fp64 statistics on the host, rounded to fp32 once."""
    import hipops
    x = hipops.nchw(torch.cat(srcs, dim=3)).cpu()
    mean, var = gc.moments(x)
    cpg = x.shape[1] // gc.GROUPS
    sc = (1.0 / (var + gc.EPS).sqrt()).repeat_interleave(cpg, 1) * gamma.double()[None]
    sh = beta.double()[None] - mean.repeat_interleave(cpg, 1) * sc
    return d(sc.float()).contiguous(), d(sh.float()).contiguous()


def check_fold(tag, name, srcs, gamma, beta, fold, fails, *, cfg, ks, H, a_mode=0, variant=0):
    """Consumer with identity weights (output channel n = silu(GroupNorm(x))[n], through the kernel's own arithmetic) and the
    GroupNorm folded in its prologue, against the same launch with the host's fp64 affine: the difference is the statistic's."""
    import hipops
    from anoddpm_amd._lib import lib
    C = sum(s.shape[3] for s in srcs)
    w = torch.zeros(C, C, ks, ks)
    w[torch.arange(C), torch.arange(C), ks // 2, ks // 2] = 1.0
    lib().anoddpm_internal_variant(5, variant)
    try:
        got = hipops.conv_igemm(srcs, d(w), None, Hout=H, ks=ks, act=1, a_mode=a_mode, cfg=cfg, fold=fold)
        base = hipops.conv_igemm(srcs, d(w), None, Hout=H, ks=ks, act=1, a_mode=a_mode, cfg=cfg, gn=host_affine(srcs, gamma, beta))
    finally:
        lib().anoddpm_internal_variant(5, 0)
    x = hipops.nchw(torch.cat(srcs, dim=3)).cpu()
    gn = gc.reference(x, gamma, beta)
    if a_mode == 1:
        gn = F.interpolate(gn, scale_factor=2, mode="nearest")
    got_, base_ = hipops.nchw(got).cpu().double(), hipops.nchw(base).cpu().double()
    # the base launch is the kernel's own rendering of the fp64 expression (F(4x4,3x3): its 1e-4 bar; a constant group: scale and
    # shift are +-316 gamma rounded to fp32, the case's own bar)
    if not (gc.error(base_, F.silu(gn)) < gc.bars(name, x.shape[0]).clamp_min(1e-4)).all():
        fails.append(f"{tag} {name}: the launch on the host affine is not the reference")
    # the difference of the two launches relative to the GroupNorm output's own maximum: the metric of the affine routes
    # (SiLU has a slope of at most 1.1 and only shrinks the maximum)
    gc.failures(tag, name, gn + (got_ - base_), gn, fails, LEDGER)
    if gc.CASES[name][0] == "zeros" and not torch.equal(got, base):
        fails.append(f"{tag} zeros: folded affine is not (scale, beta) bit for bit")


FOLD43 = [
    # id, B, (c0, c1), H (of the consumer), a_mode
    ("c64", 2, (64, 0), 32, 0),                # 2 channels per group: a thread's four channels span two groups
    ("c128", 2, (128, 0), 32, 0),
    ("concat256+128", 2, (256, 128), 32, 0),   # 12 per group: a group straddles the two sources
    ("nearest_x2", 2, (128, 0), 32, 1),        # the statistics are those of the half-resolution source (P = 16 x 16)
]


@pytest.mark.parametrize("variant", [0, 3], ids=["auto", "channel-sliced"])
@pytest.mark.parametrize("route", FOLD43, ids=[r[0] for r in FOLD43])
def test_atomic_sums_and_prologue_fold(route, variant):
    """F(4x4,3x3) producers add fp32 workgroup sums to [B][N][2] fp64 with device-scope atomics (stats_csum); gn_finalize reads
    them (fmt 1) and the F(4x4,3x3) consumer finishes the GroupNorm in its prologue (fold_*, gn_fold.h)."""
    import hipops
    rid, B, (c0, c1), H, a_mode = route
    C, Hs = c0 + c1, (H // 2 if a_mode else H)
    gamma, beta = gc.affine(C)
    fails = []
    for name in gc.CASES:
        srcs, sums = [], []
        if c1:                                  # the second source: a plain tensor of the same GroupNorm, sums from a reduction
            other = hipops.nhwc(d(gc.operand(name, B, C, Hs, Hs, mean_scale=1.05)[:, c0:])).contiguous()
            of = other.double().reshape(B, -1, c1)
        cs = []
        srcs.append(produce(name, 3, variant, B, 32, c0, Hs, 3, ctot=C, csum_out=cs))
        sums.append(cs[0])
        if c1:
            srcs.append(other)
            sums.append(torch.stack([of.sum(1), (of * of).sum(1)], dim=-1).contiguous())
        tag = f"atomic sums f43 {rid} variant={variant}"
        sc, sh, mean, rstd = hipops.gn_finalize(sums, d(gamma), d(beta), Hs * Hs, want_mean_rstd=True, fmts=(1, 1))
        check_affine(tag + " -> gn_finalize", name, srcs, gamma, beta, sc, sh, fails, mean, rstd)
        fold = dict(stats=[(s_, 1) for s_ in sums], gamma=d(gamma), beta=d(beta))
        check_fold(tag + " -> prologue fold", name, srcs, gamma, beta, fold, fails, cfg=3, ks=3, H=H, a_mode=a_mode, variant=variant)
    conclude(fails)


def test_atomic_sums_of_both_sources_of_a_concat():
    """(256, 128) with BOTH sources written by F(4x4,3x3) producers that accumulate their sums atomically."""
    import hipops
    B, c0, c1, H = 2, 256, 128, 32
    C = c0 + c1
    gamma, beta = gc.affine(C)
    fails = []
    for name in ("r0_unit", "r16_unit", "r16_eps", "r64_unit", "zeros", "const1"):
        cs0, cs1 = [], []
        srcs = [produce(name, 3, 0, B, 32, c0, H, 3, ctot=C, csum_out=cs0)]
        # second producer: the LAST 128 channels of the same GroupNorm (conv_operand gives the first N of ctot: build all, keep the tail)
        x, w, b, temb = gc.conv_operand(name, B, 32, C, H, 3, seed=1)
        srcs.append(hipops.conv_igemm([hipops.nhwc(d(x))], d(w[c0:].contiguous()), d(b[c0:].contiguous()), Hout=H, ks=3,
                                      temb=d(temb[:, c0:].contiguous()), cfg=3, csum_out=cs1))
        fold = dict(stats=[(cs0[0], 1), (cs1[0], 1)], gamma=d(gamma), beta=d(beta))
        check_fold("atomic sums f43 both sources 256+128 -> prologue fold", name, srcs, gamma, beta, fold, fails, cfg=3, ks=3, H=H)
    conclude(fails)


ROWFOLD = [
    # id, consumer cfg, ks, B, C, H: rows written by the same kernel family's epilogue, folded in the consumer's prologue (fmt 0)
    ("smallmap_c64", 5, 1, 2, 64, 16),
    ("smallmap_c128_3x3", 5, 3, 2, 128, 16),
    ("wino23s_c128", 6, 3, 2, 128, 32),
]


@pytest.mark.parametrize("route", ROWFOLD, ids=[r[0] for r in ROWFOLD])
def test_rows_and_prologue_fold(route):
    """The route most launches of the small models take: epilogue rows of cfg 5 / 6 folded in the prologue of a cfg 5 / 6
    consumer, no gn_finalize launch."""
    rid, cfg, ks, B, C, H = route
    gamma, beta = gc.affine(C)
    fails = []
    for name in gc.CASES:
        st = []
        out = produce(name, cfg, 0, B, 64, C, H, 3, stats_out=st)
        fold = dict(stats=[(st[0], 0)], gamma=d(gamma), beta=d(beta))
        check_fold(f"rows -> prologue fold {rid}", name, [out], gamma, beta, fold, fails, cfg=cfg, ks=ks, H=H)
    conclude(fails)
