"""Shared by the convolution conditioning tests (tests/test_conv_reference.py on the CPU, tests/test_gpu_conv_conditioning.py on the
device): operands of the regimes a trained UNet produces, the fp64 reference of the fused layer, a per-plane error figure, fp32 CPU
restatements of the three arithmetic classes, and the bars.  No device needed here.

Why: every convolution case of tests/test_gpu_ops.py draws x, temb, res ~ N(0, 1), w ~ N(0, 1 / 9K), gamma = 1 +- 0.1, beta = +- 0.1 and
reports one figure, max |err| / max |ref| over the whole tensor.  A contraction error of 1 % under a residual 64 times louder, a wrong
row read by a quiet image, a wrong store in a quiet output channel, SiLU beyond |y| = 6, outlier input channels under F(4x4,3x3), or an
indexing error of 5e-5 inside the 1e-4 Winograd bars all pass that figure.

The fused layer (`reference`):  h = x * scale + shift  (GroupNorm(32, C) as an affine row per image, or an affine given directly, or
none) -> SiLU -> nearest x2 | 2x2 average -> ks x ks convolution, zero padding of h -> + bias + temb[b, n] + res (res_up: a
half-resolution residual repeated 2x2).  The device and the restatements read the affine rounded once to fp32, as they read every
operand; the fp64 reference of a GroupNorm launch is F.group_norm itself.

Operand regimes (`operands`): drawn in fp64 from a seeded generator, rounded once to fp32; the reference is fp64 of the fp32 values.
  iid               x, temb, res ~ N(0, 1); w ~ N(0, 1 / (ks^2 K)); bias = 0.1 n; gamma = 1 + 0.1 n; beta = 0.1 n
  loud_residual     res = 64 n, temb = 8 n: the convolution is about 1 / 64 of the output             (launches with a residual)
  quiet_image       image 0: x = 2^-10 (n + p_c), res = 2^-10 n, p_c = +-1.5 alternating over the channels (a pattern of its own that
                    no beta produces: its affine row differs from every other image's in scale AND shift)            (B >= 2)
  quiet_channels    output channels n % 4 == 1 and the last 16 (N > 16): w, bias scaled by 2^-10
  saturated         gamma = 8 on c % 16 == 3, 1 elsewhere; beta from {-4, 0, +4}: activations reach +-30      (GroupNorm + SiLU launches)
  outlier_channels  input channels c % 32 == 5 scaled by 64, and channel 2 of the second source of a virtual concat (launches without
                    GroupNorm: the data-gradient form, the Upsample convolutions, the skip 1x1)
  flat_edges        x = -1 + a_c [col >= cs] + b_c [row >= rs] + 0.01 n, a_c, b_c ~ N(0, 1); cs = 16 where the map is wider than 16 (a
                    16-pixel tile seam), else W / 2; rs = 5 H / 16 (never a seam); filters n % 2 == 0 have zero sum per input channel:
                    where the operand is flat their true output is only the noise                        (3x3 launches, H >= 16)
  lattice           see below                                                                         (anoddpm_igemm launches)
Levels: the x64 of outlier_channels, the gamma = 8 / beta = +-4 of saturated and the x64 / x8 of loud_residual are the first levels
tried; at them the restatements give (worst case of the class, 4 r32 against CAP)
  direct   loud_residual 2.2e-07   saturated 6.3e-07   outlier 9.7e-07    (CAP 2e-5)
  F(2x2)   loud_residual 2.2e-07   saturated 3.9e-07   outlier 1.2e-06    (CAP 1e-4)
  F(4x4)   loud_residual 2.5e-07   saturated 4.2e-06   outlier 2.0e-05    (CAP 1e-4)
so no level had to come down (test_conv_reference.py asserts 4 r32 <= CAP on every case).

Error figure (`plane_error`): one number per (image, output channel) plane,  max_p |got - ref| / max_p S,  S the fp64 running-sum
scale  |h| (*) |w| + |bias| + |temb| + |res|  of the plane (h: the activated, resampled operand the convolution reads).  S >= |ref|
pointwise, so within a plane the figure is never larger than max |err| / max |ref| of that plane: CAP, the old bar, is no loosening.

Restatements (`restate`): the published algorithms in fp32 on the CPU, accumulated over 16-channel chunks -- direct convolution;
Winograd F(2x2,3x3) on hipops._pack_wino weights; F(4x4,3x3) on hipops._pack_wino43 weights (Lavin & Gray, "Fast Algorithms for
Convolutional Neural Networks", 2016: Y = A^T [ sum_c (G g G^T) o (B^T d B) ] A with the matrices of its section 4).

Bars (`bar`): r32 = the worst plane of the restatement of the case's class, computed at run time; the device bar is
max(FLOOR[class], 4 r32), never above CAP[class] (2e-5 direct = TOL of test_gpu_ops.py, 1e-4 Winograd).  The factor 4 is
attn_cases.py's: another summation order plus the hardware exponential and reciprocal.  FLOOR = 4 x the worst iid r32 of the class
over all shapes of `cases()`, measured by test_conv_reference.py::test_floors (which holds the constants below to the measurement
within a factor 1.5: see FLOOR).

lattice: operands for which fp32 arithmetic is exact.  x sparse in {-1, 0, 1}; bias, temb, res small integers; the launch is plain (no
SiLU) and where the shape's layer has a GroupNorm the affine is given as integer rows scale in {1, 2}, shift = +-1 on one channel in 32 (c + 5 b = 1 mod 32), different
for every image; weights are sparse integers t (direct, F(2x2): G holds 1 and 1/2) or 9 t / 8 (F(4x4): G g G^T is then a multiple of
2^-9 with a small numerator, and the fp64 pack rounds it to fp32 exactly).  Every intermediate of every class then lies on a
dyadic lattice (LATTICE_STEP), and if the absolute-value pipeline  |A^T| ( sum_k |U| . |B^T| |d| |B| ) |A| + |bias| + |temb| + |res|
(direct: sum |h| |w| + ...) stays below 2^24 steps every order of fp32 operations -- FMA, MFMA, split-K -- gives the same, exact
result: `lattice_bound`, asserted by test_conv_reference.py.  The densities are chosen for that (LATTICE_DENSITY).  The sums and
sums of squares of the fused statistics rows are exact under the same reasoning (`lattice_stats_bound`).  One qualification, F(4x4)
only: an entry of G g G^T whose exact value is 0 keeps a residue of the fp64 pack (about 1e-18); it is absorbed wherever the exact
output is not 0 and bounded by `lattice_residue` (below 1e-12) where it is: `lattice_mismatch` is equality with that allowance."""
import collections
import functools
import math

import torch
import torch.nn.functional as F

TOL = 2e-5                                                      # TOL of test_gpu_ops.py
CAP = {"direct": TOL, "wino23": 1e-4, "wino43": 1e-4}           # the existing bar of each class
# 4 x the worst iid plane figure of the class's restatement over SHAPES.  test_conv_reference.py::test_floors measured
# 4 x 1.70e-07 (direct: the stem, K = 9), 4 x 7.45e-08 (F(2x2): cfg 6 nearest x2) and 4 x 1.53e-06 ... 1.75e-06 (F(4x4): K = 16, one
# chunk) and holds each constant within a factor 1.5 of its own measurement, either way.  The measurement is the largest of about a
# thousand plane figures, each the largest rounding error of a plane; the BLAS behind einsum and conv2d sums in an order that depends
# on the CPU's vector width and thread count, another order redraws every rounding error, and the largest of the redrawn errors
# moves by tens of per cent: two CPUs gave 1.53e-06 and 1.75e-06 for F(4x4) on the same operands, MKL_CBWR=COMPATIBLE 1.83e-06 (the
# other two classes agreed).
# A bar never depends on which side of its measurement the constant lies: it is max(FLOOR, 4 r32) with r32 measured at run time.
FLOOR = {"direct": 7.5e-7, "wino23": 3.3e-7, "wino43": 6.8e-6}

REGIMES = ("iid", "loud_residual", "quiet_image", "quiet_channels", "saturated", "outlier_channels", "flat_edges", "lattice")
QUIET = 2.0 ** -10
LATTICE_STEP = {"direct": 0.25, "wino23": 0.25, "wino43": 2.0 ** -9}       # direct: 1/4 for the 2x2 average of integers
# expected non-zero products per tap of an output: x and t are each non-zero with probability sqrt(LATTICE_DENSITY / K)
LATTICE_DENSITY = {"direct": 3.0, "wino23": 3.0, "wino43": 0.75}

Case = collections.namedtuple("Case", "kind cfg B cin N H ks a_mode gn act temb res ksplit res_up")


def _c(cfg, B, cin, N, H, ks=3, a_mode=0, gn=True, act=1, temb=False, res=False, ksplit=1, res_up=False, kind="igemm"):
    return Case(kind, cfg, B, cin, N, H, ks, a_mode, gn, act, temb, res, ksplit, res_up)


# the smallest shapes of tests/test_gpu_ops.py that reach each path, with B >= 2
SHAPES = (
    # cfg 0: 128 x 128 direct tiles
    _c(0, 2, (64, 0), 128, 32, temb=True, res=True),
    _c(0, 2, (64, 64), 128, 16, temb=True, res=True),                       # virtual concat
    _c(0, 2, (64, 32), 128, 16, ks=1, gn=False, act=0),                     # plain 1x1 skip over a concat
    # cfg 1: 64 x 64 direct tiles
    _c(1, 2, (96, 32), 96, 8, res=True, ksplit=4),                          # concat + split-K + N tail
    _c(1, 3, (64, 0), 32, 4, res=True, ksplit=2),                           # 4x4 level (partial tile)
    _c(1, 2, (64, 0), 64, 16, a_mode=2, temb=True, ksplit=2),               # fused 2x2 average
    # cfg 2: F(2x2,3x3)
    _c(2, 2, (32, 0), 64, 16, gn=False, act=0),                             # bare transform
    _c(2, 2, (96, 32), 96, 32, res=True),                                   # N tail
    _c(2, 2, (128, 64), 64, 16, res=True, ksplit=3),                        # split inside and across the sources
    _c(2, 2, (64, 0), 64, 32, a_mode=1, ksplit=2),                          # fused nearest x2
    # cfg 3: F(4x4,3x3), under every f43 variant that applies
    _c(3, 2, (16, 0), 128, 16, gn=False, act=0),                            # one K iteration
    _c(3, 2, (32, 32), 64, 32, res=True),                                   # N = 64
    _c(3, 2, (64, 64), 128, 32, temb=True, res=True),                       # virtual concat
    _c(3, 2, (64, 0), 128, 32, a_mode=1),                                   # fused nearest x2
    _c(3, 2, (128, 0), 128, 32, temb=True, res=True, ksplit=2),             # split-K + tail
    _c(3, 2, (64, 0), 128, 32, res=True, res_up=True),                      # half-resolution residual
    _c(3, 2, (128, 0), 128, 32, gn=False, act=0),                           # data-gradient form
    _c(3, 2, (64, 64), 128, 32, gn=False, act=0),                           # data-gradient form over a concat
    # cfg 4: streaming 1x1
    _c(4, 2, (128, 0), 128, 32, ks=1, gn=False, act=0, temb=True, res=True),
    _c(4, 2, (128, 0), 64, 32, ks=1, gn=False, act=0, res=True),
    # cfg 5: small maps
    _c(5, 2, (96, 32), 96, 8, temb=True, res=True),
    _c(5, 3, (64, 0), 32, 4, res=True),
    _c(5, 2, (32, 0), 64, 8),
    _c(5, 2, (128, 0), 384, 16, ks=1, act=0),                               # qkv: GroupNorm, no SiLU
    # cfg 6: F(2x2,3x3) without split-K
    _c(6, 12, (64, 32), 96, 16, res=True),
    _c(6, 4, (64, 0), 64, 32, a_mode=1),
    _c(6, 2, (128, 0), 128, 32, gn=False, act=0),
    # cfg 7: F(4x4,3x3) on split-bf16 products
    _c(7, 2, (32, 0), 128, 16, gn=False, act=0),
    _c(7, 2, (64, 64), 128, 32, temb=True, res=True),
    # head (GroupNorm + SiLU -> 3x3, N <= 4, NCHW output) and stem (NCHW input, plain 3x3)
    _c(-1, 2, (128, 0), 1, 32, kind="head"),
    _c(-1, 2, (128, 0), 4, 24, kind="head"),
    _c(-1, 2, (1, 0), 64, 32, gn=False, act=0, kind="stem"),
)


def klass(case):
    """The arithmetic class of a case: which restatement, FLOOR and CAP it takes."""
    return {2: "wino23", 6: "wino23", 3: "wino43", 7: "wino43"}.get(case.cfg, "direct")


def variants(case):
    """The f43 variants (anoddpm_internal_variant(5, v)) under which a case runs.  0: the launcher's choice.  3 (the channel-sliced
    kernel), 6 and 7 (one wave per SIMD) take the launch only where N % 128 == 0 and it is not split-K (split-K always runs the
    channel-sliced kernel); elsewhere they are the launcher's choice again and are not repeated."""
    if case.cfg != 3:
        return (0,)
    return (0, 3, 6, 7) if case.N % 128 == 0 and case.ksplit == 1 else (0,)


def applies(case, regime):
    """A regime applies to a shape only where the launch has the operand it perturbs."""
    if regime == "loud_residual":
        return case.res
    if regime == "quiet_image":
        return case.B >= 2
    if regime == "saturated":
        return case.gn and case.act == 1
    if regime == "outlier_channels":
        return not case.gn
    if regime == "flat_edges":
        return case.ks == 3 and case.H >= 16
    if regime == "lattice":
        return case.kind == "igemm"
    if regime == "quiet_channels":
        return case.N > 1
    return True


def cases():
    """[(case, regime, variant)] of the device test."""
    return [(c, r, v) for c in SHAPES for r in REGIMES if applies(c, r) for v in variants(c)]


def case_id(item):
    c, regime, v = item
    what = c.kind if c.kind != "igemm" else f"cfg{c.cfg}"
    mode = {0: "", 1: "-up", 2: "-avg"}[c.a_mode] + (f"-sk{c.ksplit}" if c.ksplit > 1 else "") + ("-resup" if c.res_up else "")
    mode += "" if c.gn or c.kind != "igemm" else "-plain"
    return f"{what}{'v%d' % v if c.cfg == 3 else ''}-{c.B}x{c.cin[0]}+{c.cin[1]}-{c.N}-{c.H}-k{c.ks}{mode}-{regime}"


# ---------------------------------------------------------------------------------------------------- operands
def _hin(case):
    return case.H if case.a_mode == 0 else (case.H // 2 if case.a_mode == 1 else case.H * 2)


def _group_affine(x, gamma, beta, groups=32, eps=1e-5):
    """fp64 rows scale, shift [B, C] of GroupNorm(groups, C): group_norm(x) == x * scale + shift."""
    B, C = x.shape[:2]
    xg = x.reshape(B, groups, -1)
    mean = xg.mean(-1)
    rstd = (xg.var(-1, unbiased=False) + eps).rsqrt()
    scale = gamma[None] * rstd.repeat_interleave(C // groups, 1)
    return scale, beta[None] - mean.repeat_interleave(C // groups, 1) * scale


def _lattice(case, o, rn, gen):
    B, C, N = case.B, sum(case.cin), case.N
    d = min(0.5, math.sqrt(LATTICE_DENSITY[klass(case)] / C))

    def sparse(shape, density):
        keep = torch.rand(shape, generator=gen, dtype=torch.float64) < density
        sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
        return keep * sign

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=gen).double()

    o["x"] = sparse(o["x"].shape, d)
    o["w"] = sparse(o["w"].shape, d) * (9.0 / 8.0 if klass(case) == "wino43" else 1.0)
    o["bias"], o["temb"], o["res"] = ints((N,), -2, 2), ints((B, N), -3, 3), ints(o["res"].shape, -4, 4)
    if case.gn:                                             # an integer affine, a different row for every image; sparse shift
        o["scale"] = ints((B, C), 1, 2)
        on = (torch.arange(C)[None, :] + 5 * torch.arange(B)[:, None]) % 32 == 1
        o["shift"] = on * (torch.randint(0, 2, (B, C), generator=gen).double() * 2 - 1)
    o["act"] = 0


def operands(case, regime):
    """dict of fp32 operands of a (case, regime): x [B, C, Hin, Hin], w [N, C, ks, ks], bias [N], temb [B, N] | None, res | None,
    scale, shift [B, C] | None (the affine the launch is given), act; and, where the affine is a GroupNorm, gamma and beta."""
    B, (c0, c1), N, H, ks = case.B, case.cin, case.N, case.H, case.ks
    C, Hin = c0 + c1, _hin(case)
    gen = torch.Generator().manual_seed(4000 + 97 * SHAPES.index(case) + REGIMES.index(regime))

    def rn(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)

    Hr = H // 2 if case.res_up else H
    o = dict(x=rn(B, C, Hin, Hin), w=rn(N, C, ks, ks) / math.sqrt(C * ks * ks), bias=0.1 * rn(N), temb=rn(B, N), res=rn(B, N, Hr, Hr),
             gamma=1 + 0.1 * rn(C), beta=0.1 * rn(C), scale=None, shift=None, act=case.act)
    if regime == "loud_residual":
        o["res"] *= 64
        o["temb"] *= 8
    elif regime == "quiet_image":
        pattern = 1.5 * (1 - 2 * (torch.arange(C) % 2)).double()
        o["x"][0] = QUIET * (o["x"][0] + pattern[:, None, None])
        o["res"][0] *= QUIET
    elif regime == "quiet_channels":
        quiet = torch.arange(N) % 4 == 1
        if N > 16:
            quiet[-16:] = True
        o["w"][quiet] *= QUIET
        o["bias"][quiet] *= QUIET
    elif regime == "saturated":
        o["gamma"] = torch.where(torch.arange(C) % 16 == 3, 8.0, 1.0).double()
        o["beta"] = 4.0 * (torch.randint(0, 3, (C,), generator=gen) - 1).double()
    elif regime == "outlier_channels":
        o["x"][:, torch.arange(C) % 32 == 5] *= 64
        if c1:
            o["x"][:, c0 + 2] *= 64
    elif regime == "flat_edges":
        cs, rs = (16 if Hin > 16 else Hin // 2), 5 * Hin // 16
        col = (torch.arange(Hin) >= cs).double()
        row = (torch.arange(Hin) >= rs).double()
        o["x"] = -1 + rn(1, C, 1, 1) * col[None, None, None, :] + rn(1, C, 1, 1) * row[None, None, :, None] + 0.01 * o["x"]
        o["w"][0::2] -= o["w"][0::2].mean(dim=(2, 3), keepdim=True)
    elif regime == "lattice":
        _lattice(case, o, rn, gen)
    o = {k: (v.float() if torch.is_tensor(v) else v) for k, v in o.items()}
    if case.gn and regime != "lattice":
        sc, sh = _group_affine(o["x"].double(), o["gamma"].double(), o["beta"].double())
        o["scale"], o["shift"] = sc.float(), sh.float()
    if not case.temb:
        o["temb"] = None
    if not case.res:
        o["res"] = None
    return o


# ---------------------------------------------------------------------------------------------------- the fused layer
def _activated(case, o, dtype, exact_groupnorm=False):
    """h: the activated, resampled operand the convolution reads."""
    h = o["x"].to(dtype)
    if exact_groupnorm:
        h = F.group_norm(h, 32, o["gamma"].to(dtype), o["beta"].to(dtype), eps=1e-5)
    elif o["scale"] is not None:
        h = h * o["scale"].to(dtype)[:, :, None, None] + o["shift"].to(dtype)[:, :, None, None]
    if o["act"]:
        h = F.silu(h)
    if case.a_mode == 1:
        h = F.interpolate(h, scale_factor=2, mode="nearest")
    elif case.a_mode == 2:
        h = F.avg_pool2d(h, 2, 2)
    return h


def _epilogue(case, o, y, dtype, absolute=False):
    f = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    y = y + f(o["bias"])[None, :, None, None]
    if o["temb"] is not None:
        y = y + f(o["temb"])[:, :, None, None]
    if o["res"] is not None:
        r = f(o["res"])
        y = y + (F.interpolate(r, scale_factor=2, mode="nearest") if case.res_up else r)
    return y


def reference(case, o, regime):
    """fp64 (ref, S) [B, N, H, H] of the fp32 operands: the fused layer and its running-sum scale."""
    h = _activated(case, o, torch.float64, exact_groupnorm=case.gn and regime != "lattice")
    w = o["w"].double()
    ref = _epilogue(case, o, F.conv2d(h, w, padding=case.ks // 2), torch.float64)
    S = _epilogue(case, o, F.conv2d(h.abs(), w.abs(), padding=case.ks // 2), torch.float64, absolute=True)
    return ref, S


def plane_error(got, ref, S):
    """[B, N] fp64: per (image, output channel) plane max_p |got - ref| / max_p S; inf where got is not finite."""
    e = (got.detach().double().cpu() - ref).abs().flatten(2)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf"))).amax(-1)
    return e / S.flatten(2).amax(-1).clamp_min(1e-300)


def global_error(got, ref):
    """The figure of tests/test_gpu_ops.py: max |got - ref| / max |ref| over the whole tensor."""
    return ((got.detach().double().cpu() - ref).abs().max() / ref.abs().max()).item()


def worst_plane(e):
    """(figure, image, channel) of the worst plane."""
    i = e.argmax().item()
    return e.flatten()[i].item(), i // e.shape[1], i % e.shape[1]


# ---------------------------------------------------------------------------------------------------- restatements
CHUNK = 16
# Lavin & Gray 2016, section 4.1 (F(2x2,3x3)) and 4.3 (F(4x4,3x3)): B^T and A^T; G is hipops._WINO_G / _WINO43_G
_BT = {"wino23": [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]],
       "wino43": [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                  [0, 4, 0, -5, 0, 1]]}
_AT = {"wino23": [[1, 1, 1, 0], [0, 1, -1, -1]],
       "wino43": [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]}


def transformed_weights(w, cls):
    """U [t, t, K, N] fp32 read back from the packed layout the kernels are given (hipops._pack_wino / _pack_wino43)."""
    import hipops
    N, K = w.shape[:2]
    packed = hipops._pack_wino43(w) if cls == "wino43" else hipops._pack_wino(w)          # [t * t][K / 4][N][4]
    t = 6 if cls == "wino43" else 4
    return packed.permute(0, 1, 3, 2).reshape(t, t, K, N)


def _winograd(h, U, cls, absolute=False):
    """Y [B, N, H, W] = A^T [ sum_c U o (B^T d B) ] A over m x m output tiles, in h's dtype, the channel sum accumulated over
    16-channel chunks.  absolute: the same pipeline on |.| of every matrix and operand (the lattice bound); also returns the
    largest |transformed operand| and |element-wise sum|."""
    BT = torch.tensor(_BT[cls], dtype=h.dtype)
    AT = torch.tensor(_AT[cls], dtype=h.dtype)
    if absolute:
        BT, AT, h, U = BT.abs(), AT.abs(), h.abs(), U.abs()
    t, m = BT.shape[0], AT.shape[0]
    B, K, H, W = h.shape
    assert H % m == 0 and W % m == 0
    d = F.pad(h, (1, 1, 1, 1)).unfold(2, t, m).unfold(3, t, m)                              # [B, K, H / m, W / m, t, t]
    V = BT @ d @ BT.T
    M = torch.zeros(B, U.shape[3], H // m, W // m, t, t, dtype=h.dtype)
    for c in range(0, K, CHUNK):
        M += torch.einsum("uvco,bcxyuv->boxyuv", U[:, :, c:c + CHUNK], V[:, c:c + CHUNK])
    Y = (AT @ M @ AT.T).permute(0, 1, 2, 4, 3, 5).reshape(B, U.shape[3], H, W)
    return (Y, V.max().item(), M.max().item()) if absolute else Y


def _direct(h, w, pad):
    y = None
    for c in range(0, h.shape[1], CHUNK):
        part = F.conv2d(h[:, c:c + CHUNK], w[:, c:c + CHUNK], padding=pad)
        y = part if y is None else y + part
    return y


def restate(case, o):
    """The fp32 CPU restatement of the case's arithmetic class: [B, N, H, H] fp32."""
    cls = klass(case)
    h = _activated(case, o, torch.float32)
    y = _direct(h, o["w"], case.ks // 2) if cls == "direct" else _winograd(h, transformed_weights(o["w"], cls), cls)
    return _epilogue(case, o, y, torch.float32)


def bar(cls, r32):
    return min(CAP[cls], max(FLOOR[cls], 4.0 * r32))


def lattice_bound(case, o):
    """The largest value the absolute-value pipeline of the case's class reaches at any intermediate or output, in lattice steps."""
    cls = klass(case)
    h = _activated(case, o, torch.float64)
    if cls == "direct":
        y, inner = F.conv2d(h.abs(), o["w"].double().abs(), padding=case.ks // 2), 0.0
    else:
        y, vmax, mmax = _winograd(h, transformed_weights(o["w"], cls).double(), cls, absolute=True)
        inner = max(vmax, mmax)
    y = _epilogue(case, o, y, torch.float64, absolute=True)
    return max(y.max().item(), inner) / LATTICE_STEP[cls]


U_RESIDUE = 4 * 2.0 ** -53      # of |G| |g| |G|^T: a few fp64 roundings of the terms of an entry of G g G^T


def lattice_residue(case, o):
    """F(4x4) only: G holds 1/6, 1/12, 1/24, which fp64 rounds, so G g G^T in fp64 is the lattice value plus a residue of a few
    2^-53 of the entry's terms.  Rounding to fp32 removes it from every non-zero entry and keeps it in an entry whose exact value is
    0.  Such a residue is absorbed by any non-zero lattice value it is added to (half an ulp of one lattice step is 2^-34); it can
    survive only into an output whose exact value is 0.  Returns the largest |output| it can leave there: the absolute-value
    pipeline with U_RESIDUE |G| |g| |G|^T in place of every weight whose exact value is 0 (the device packer of cfg 7 evaluates the
    same expression in fp64, so the bound serves it as well)."""
    if klass(case) != "wino43":
        return 0.0
    return _winograd(_activated(case, o, torch.float64), residue_weights(o["w"]), "wino43", absolute=True)[0].max().item()


def residue_weights(w):
    """[6, 6, K, N] fp64: the bound on what the fp64 pack leaves in each entry of U whose exact value is 0; 0 elsewhere."""
    import hipops
    U = transformed_weights(w, "wino43").double()
    exact = (U / LATTICE_STEP["wino43"]).round() * LATTICE_STEP["wino43"]
    G = hipops._WINO43_G.abs()
    terms = torch.einsum("ua,oiab,vb->uvio", G, w.double().abs(), G)
    return torch.where(exact == 0, U_RESIDUE * terms, torch.zeros_like(terms))


def lattice_mismatch(got, ref, residue):
    """None if got (fp32) is the exact result: bit-equal to ref wherever ref != 0, and within `residue` of 0 where ref == 0 (bit-equal
    there too when residue is 0).  Otherwise a description of the worst element."""
    got = got.detach().cpu().double()
    zero = ref == 0
    diff = (got - ref).abs()
    diff = torch.where(torch.isfinite(diff), diff, torch.full_like(diff, float("inf")))
    wrong = torch.where(zero, diff > residue, diff > 0)
    if not wrong.any():
        return None
    i = torch.where(wrong, diff, torch.zeros_like(diff)).argmax().item()
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), diff.shape))
    return f"{int(wrong.sum())} of {wrong.numel()} elements differ; worst at {idx}: got {got[idx].item()!r}, exact {ref[idx].item()!r}"


def lattice_stats_bound(case, ref):
    """Sums of the output and of its squares over a whole plane, in steps of the output's own lattice (integers; 1/4 after the 2x2
    average; 1/8 with the 9 t / 8 weights) and of its square: below 2^24 every partial sum of a statistics row is exact."""
    step = 0.125 if klass(case) == "wino43" else 0.25
    return max(ref.abs().flatten(2).sum(-1).max().item() / step, (ref * ref).flatten(2).sum(-1).max().item() / (step * step))


@functools.lru_cache(maxsize=None)
def prepared(case, regime):
    """Everything a check of a (case, regime) needs, computed once and shared, read-only, by the tests of a session:
    dict(o (operands), ref, S (fp64), e32 [B, N] (plane figures of the restatement), r32 (their worst), bar)."""
    o = operands(case, regime)
    ref, S = reference(case, o, regime)
    y32 = restate(case, o)
    e32 = plane_error(y32, ref, S)
    r32 = e32.max().item()
    return dict(o=o, ref=ref, S=S, y32=y32, e32=e32, r32=r32, bar=bar(klass(case), r32))
