"""Shared by the element tests of csrc/gn_backward.hip (anoddpm_gn_silu_backward: reduce, fold, apply) -- tests/test_gn_bwd_reference.py
on the CPU, tests/test_gpu_gn_bwd_elements.py on the device.  Seeded operands, the fp64 statement of every output, the fp32
restatement, a per-row error figure, the bars, and a numpy model of the three passes with the kernel's index arithmetic on which
defects are planted.  numpy and torch on the CPU only; the library is not imported.

Why: tests/test_gpu_ops.py::test_gn_silu_backward takes one figure max |err| / max |ref| over a whole tensor at seven square shapes
(C 64 / 128 / 384, B <= 2, nslab 4, acc_dx 0 / 3, no dres, dense operands).  A wrong value in a quiet image, in one group or in the
last pixels of a slab passes it, and none of its shapes reaches: idle threads (R = 256 / TQ with TQ R < 256), groups that are no
multiple of a channel quad, the second channel pass, the fold's image chunks and its unrolled loop, short / ragged / empty slabs,
the apply pass's tail, non-square maps under a_mode 1 / 2, acc_dx 1 / 2 alone, pixel strides wider than the channel count.

Statement (`statement`): the formulas of include/anoddpm_hip.h (anoddpm_gn_bwd_args) in plain torch on the fp32-rounded operands,
  xhat = (x - mean) rstd;  y = gamma xhat + beta;  dy = da silu'(y), silu'(y) = s (1 + y (1 - s)), s = sigmoid(y)  (act 0: dy = da)
  partial[b][slab][c] = {sum dy, sum dy xhat} over the slab's pixels, slab s = pixels [s sp, (s + 1) sp), sp = ceil(P / nslab)
  dbeta[c] += sum_{b, slab} partial[.][0];  dgamma[c] += sum partial[.][1]
  k0 = rstd gamma;  k1 = rstd mean_g(gamma dy);  k2 = rstd mean_g(gamma dy xhat)    (means over P cpg elements, from the slab sums)
  dx = k0 dy - k1 - xhat k2  (+ dres) (+ what is there, acc_dx)
Evaluated in fp64 it is the reference; in fp32 the restatement: products and the sigmoid in fp32, the per-channel sums in fp32
within a slab the way the kernel's threads walk it (row r of R = 256 / min(C / 4, 256) takes pixels p0 + r, p0 + r + R, ... in order;
the R rows are added in fp64), the folds in fp64, k0 .. k2 rounded to fp32, dx = (k0 dy - k1) - xhat k2, then + dres, then + old.
mean and rstd are inputs: fp64 from the fp32 x (biased variance, eps 1e-5), rounded to fp32.  da at the source pixel: a_mode 1 the
four children of a 2 Hs x 2 Ws map as (v00 + v01) + (v10 + v11), a_mode 2 a quarter of the parent of an Hs / 2 x Ws / 2 map.

Error figure: every element is compared; one number per row, max |got - ref| / max S within the row, S the fp64 sum of the absolute
values of the element's terms: dx |k0 dy| + |k1| + |xhat k2| + |dres| + |old|, row = (image, group); dgamma / dbeta sum |dy xhat| /
sum |dy| + |old|, row = the group's channels; partial the slab's sum |dy| / sum |dy xhat|, row = (image, slab, group) (an empty slab has
S = 0 and must hold exact zeros).

Regimes: drawn in fp64 from a seeded generator, rounded once to fp32.  x, da, dres, old ~ N(0, 1); gamma = 1 + 0.1 n, beta = 0.1 n.
  iid
  quiet_row   da of image 0 and of the channels c % 4 == 1 scaled by 2^-10 (and dres / old dx of image 0 with it, so that the
              quiet image's rows are not measured against a loud addend)
  saturated   gamma, beta from train_op_cases._saturated_affine (gamma x 8 on c % 16 == 3, beta from {-4, 0, +4}); beta = -100 on
              c % 32 == 5 where cpg >= 2 (__expf(-y) overflows; with cpg 1 a dgamma / dbeta row would be that one channel, S ~ 0)
  off_centre  x + 16 (r = 16 of gn_cases)
Bars: max(FLOOR[class], 4 r32), never above CAP = 2e-5 (BAR_GN, the bar of test_gn_silu_backward); r32 the worst row of the
restatement at run time; FLOOR = 4 x the worst iid r32 over all shapes (test_gn_bwd_reference.py::test_floors, within a factor 1.5).
The factor 4: another summation order plus the hardware exponential and reciprocal (attn_cases.py, train_op_cases.py)."""
import collections
import functools
import math

import numpy as np
import torch

from train_op_cases import GUARD, QUIET, _round, _saturated_affine, global_error, row_error, silu_grad, worst_row  # noqa: F401

GROUPS = 32
EPS = 1e-5
CAP = 2e-5                                                   # BAR_GN of tests/backward_ledger.py, the bar of test_gn_silu_backward
# 4 x the worst iid row figure of the restatement over all shapes (test_floors): dx 4 x 2.86e-07 (s08), dgamma / dbeta 4 x 1.02e-07
# (s11), partial 4 x 3.37e-07 (s12: two pixels per slab, rows of four channels)
FLOOR = {"dx": 1.14e-6, "sums": 4.1e-7, "partial": 1.35e-6}
REGIMES = ("iid", "quiet_row", "saturated", "off_centre")
ALL, TWO = REGIMES, REGIMES[:2]
PLAIN = ((0, False),)                                        # launch forms: (acc_dx, dres given)

Case = collections.namedtuple("Case", "name B c0 c1 Hs Ws a_mode act nslab forms regimes layout ready")


def _case(name, B, c0, c1, Hs, Ws, a_mode, act, nslab, forms=PLAIN, regimes=TWO, layout="dense", ready=False):
    return Case(name, B, c0, c1, Hs, Ws, a_mode, act, nslab, forms, regimes, layout, ready)


CASES = (
    _case("s01", 2, 32, 0, 6, 10, 0, 1, 3, regimes=ALL),     # cpg 1, R = 32; P = 60 < 4 R: the apply pass is all tail; slab of 20 < R
    _case("s02", 65, 32, 0, 2, 2, 0, 1, 1, regimes=ALL),     # nbp capped at 64, the second chunk holds one image
    _case("s03", 3, 64, 0, 40, 33, 0, 1, 7, regimes=ALL),    # 21 apply slabs of 64, the last of 40 pixels; reduce slabs 6 x 189 + 186
    _case("s04", 2, 96, 0, 5, 7, 0, 1, 2, regimes=ALL),      # cpg 3: quads straddle groups; R = 10 leaves 16 idle threads
    _case("s05", 2, 160, 0, 12, 20, 2, 1, 5),                # cpg 5, R = 6; da at 6 x 10
    _case("s06", 2, 64, 0, 6, 10, 1, 1, 2),                  # da at 12 x 20
    _case("s07", 3, 256, 128, 8, 12, 0, 1, 4, forms=tuple((a, d) for a in (0, 1, 2, 3) for d in (False, True))),   # cpg 12 straddles the sources
    _case("s08", 22, 256, 128, 2, 2, 0, 1, 1, regimes=ALL),  # nbp 21, two chunks (21 + 1)
    _case("s09", 9, 512, 512, 4, 6, 0, 1, 3),                # C4 = 256, R = 1, cpg 32, nbp 8, the last chunk holds one image
    _case("s10", 2, 1024, 64, 4, 6, 0, 1, 2),                # C4 = 272: the second pass has 16 quads, all x1
    _case("s11", 5, 1024, 1024, 2, 4, 0, 1, 1),              # cpg 64, the launcher's limit; nbp 4; two full passes
    _case("s12", 16, 128, 0, 8, 8, 0, 1, 37),                # S = 4: one unrolled fold trip (32 rows), then its tail; slabs beyond 32 empty
    _case("s13", 2, 128, 0, 64, 64, 0, 1, 256, regimes=ALL),  # the plan's slab count, S = 32: exactly one unrolled trip
    _case("s14", 1, 64, 0, 16, 16, 0, 0, 4, forms=((0, True),)),          # GroupNorm alone with dres: the attention block's form
    _case("s15", 2, 64, 32, 8, 8, 0, 1, 2, forms=((0, True),), layout="strided"),
    _case("s16a", 3, 64, 0, 40, 33, 0, 1, 5, ready=True),    # partial_ready: five rows written by the test, fold and apply only
    _case("s16b", 3, 256, 128, 8, 12, 0, 1, 5, ready=True),
    _case("s17", 2, 64, 0, 6, 10, 1, 0, 2),                  # s06 without SiLU
    _case("s18", 2, 160, 0, 12, 20, 2, 0, 5),                # s05 without SiLU: all six template instances launch
)
BY_NAME = {c.name: c for c in CASES}
ITEMS = [(c.name, r) for c in CASES for r in c.regimes]
# shape 15: both sources are channel slices of one [B][P][X_LD] tensor, both dx go into one [B][P][DX_LD], da and dres have rows of DA_LD
X_LD, DX_LD, DA_LD = 96, 104, 100


def item_id(item):
    return f"{item[0]}-{item[1]}"


def form_id(form):
    return f"acc_dx {form[0]}" + (" dres" if form[1] else "")


class Geo:
    """The sizes the kernels derive from the struct."""

    def __init__(self, c):
        self.C, self.P = c.c0 + c.c1, c.Hs * c.Ws
        self.cpg, self.C4 = self.C // GROUPS, self.C // 4
        self.TQ = min(self.C4, 256)
        self.R = 256 // self.TQ
        self.npass = -(-self.C4 // self.TQ)
        self.Ha, self.Wa = {0: (c.Hs, c.Ws), 1: (2 * c.Hs, 2 * c.Ws), 2: (c.Hs // 2, c.Ws // 2)}[c.a_mode]
        self.Pa = self.Ha * self.Wa
        self.sp = -(-self.P // c.nslab)                                  # reduce: pixels per slab
        nbp = min(256 // self.cpg, c.B, 64)                              # fold: images side by side, threads per image, slab lanes
        self.nbp, self.per = nbp, 256 // nbp
        self.S = self.per // self.cpg
        sp = (self.P * c.B + 2047) // 2048                               # apply: the launcher's slab
        m = self.R * 4
        self.asp = -(-sp // m) * m
        self.aslabs = -(-self.P // self.asp)


# ---------------------------------------------------------------------------------------------------- operands
def operands(c, regime):
    geo = Geo(c)
    gen = torch.Generator().manual_seed(9000 + 101 * CASES.index(c) + REGIMES.index(regime))

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float64)

    B, P, C = c.B, geo.P, geo.C
    x, da = rn(B, P, C), rn(B, geo.Pa, C)
    gamma, beta = 1 + 0.1 * rn(C), 0.1 * rn(C)
    dres, old_dx, old_dgamma, old_dbeta = rn(B, P, C), rn(B, P, C), rn(C), rn(C)
    if regime == "saturated":
        sc, sh = _saturated_affine(1, C, gen)
        gamma, beta = sc[0], sh[0]
        if geo.cpg >= 2:
            beta[torch.arange(C) % 32 == 5] = -100.0
    if regime == "off_centre":
        x = x + 16.0
    if regime == "quiet_row":
        da[0] *= QUIET
        dres[0] *= QUIET
        old_dx[0] *= QUIET
        da[:, :, torch.arange(C) % 4 == 1] *= QUIET
    o = _round(dict(x=x, da=da, gamma=gamma, beta=beta, dres=dres, old_dx=old_dx, old_dgamma=old_dgamma, old_dbeta=old_dbeta))
    o["mean64"], o["rstd64"] = moments(o["x"], geo.cpg)
    o["mean"], o["rstd"] = o["mean64"].float(), o["rstd64"].float()
    return o


def moments(x, cpg):
    """fp64 mean and rstd [B][GROUPS] of the fp32 x [B][P][C] (biased variance, eps 1e-5)."""
    B, P, C = x.shape
    v = x.double().view(B, P, GROUPS, cpg).permute(0, 2, 1, 3).reshape(B, GROUPS, -1)
    mean = v.mean(-1)
    var = ((v - mean[..., None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + EPS)


# ---------------------------------------------------------------------------------------------------- the statement
def _chan(v, cpg):
    """[B][GROUPS] -> [B][1][C]"""
    return v.repeat_interleave(cpg, 1)[:, None]


def da_at_source(da, c, dt):
    """The gradient at the SOURCE pixels [B][P][C]."""
    g, B, C = da.to(dt), c.B, c.c0 + c.c1
    if c.a_mode == 0:
        return g
    if c.a_mode == 1:
        g = g.view(B, 2 * c.Hs, 2 * c.Ws, C)
        return ((g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + (g[:, 1::2, 0::2] + g[:, 1::2, 1::2])).reshape(B, -1, C)
    g = g.view(B, c.Hs // 2, c.Ws // 2, C)
    return (g.repeat_interleave(2, 1).repeat_interleave(2, 2) * 0.25).reshape(B, -1, C)


def slab_sums(t, c):
    """t [B][P][C] -> float64 [B][nslab][C]: per slab and row r of R the pixels p0 + r, p0 + r + R, ... added in order in t's dtype,
    the R rows added in fp64."""
    geo = Geo(c)
    B, P, C = t.shape
    R, sp = geo.R, geo.sp
    T = max(1, -(-sp // R))
    s, r, j = torch.meshgrid(torch.arange(c.nslab), torch.arange(R), torch.arange(T), indexing="ij")
    off = r + j * R
    idx = s * sp + off
    idx = torch.where((off < sp) & (idx < P), idx, torch.full_like(idx, P))          # P: the zero row
    vals = torch.cat([t, torch.zeros(B, 1, C, dtype=t.dtype)], 1)[:, idx.reshape(-1)].view(B, c.nslab, R, T, C)
    acc = torch.zeros(B, c.nslab, R, C, dtype=t.dtype)
    for k in range(T):
        acc = acc + vals[:, :, :, k]
    return acc.double().sum(2)


def ready_rows(dy, dyxh, c):
    """The partial rows a partial_ready case is given: float64 [B][nslab][C][2], row s = the pixels p % nslab == s (any partition of the
    pixels is a valid producer; this one is not the reduce pass's)."""
    return torch.stack([torch.stack([dy[:, s::c.nslab].double().sum(1), dyxh[:, s::c.nslab].double().sum(1)], -1) for s in range(c.nslab)], 1)


def statement(o, c, dt, mean=None, rstd=None, partial=None):
    """dict of the launch's values without old / dres, in dtype dt (float64: the reference, float32: the restatement).
    mean, rstd: [B][GROUPS] (default: the fp32-rounded inputs); partial: the given rows of a partial_ready case."""
    geo = Geo(c)
    cpg, n = geo.cpg, float(geo.P * geo.cpg)
    f64 = dt == torch.float64
    mu = _chan((o["mean"] if mean is None else mean).to(dt), cpg)
    rs = _chan((o["rstd"] if rstd is None else rstd).to(dt), cpg)
    x, gamma, beta = o["x"].to(dt), o["gamma"].to(dt), o["beta"].to(dt)
    xhat = (x - mu) * rs
    g = da_at_source(o["da"], c, dt)
    if c.act:
        dy = g * silu_grad(xhat * gamma + beta)
    else:
        dy = g
    dyxh = dy * xhat
    if partial is None:
        partial = torch.stack([slab_sums(dy, c), slab_sums(dyxh, c)], -1)                     # float64 [B][nslab][C][2]
    chan = partial.sum(1)                                                                     # the folds: fp64
    gam64 = o["gamma"].double()
    grp = (chan * gam64[None, :, None]).view(c.B, GROUPS, cpg, 2).sum(2)                      # [B][GROUPS][2]
    r64 = (o["rstd"] if rstd is None else rstd).double()
    k0 = _chan(r64, cpg) * gam64
    k1, k2 = _chan(r64 * grp[..., 0] / n, cpg), _chan(r64 * grp[..., 1] / n, cpg)
    if not f64:
        k0, k1, k2 = k0.float(), k1.float(), k2.float()
    dx = (k0 * dy - k1) - xhat * k2
    return dict(dy=dy, xhat=xhat, dyxh=dyxh, partial=partial, dbeta=chan[..., 0].sum(0), dgamma=chan[..., 1].sum(0), dx=dx, k0=k0, k1=k1, k2=k2)


def scales(o, c, st):
    """S of every output without old / dres, fp64, from the fp64 statement `st`."""
    dy, dyxh = st["dy"].abs(), st["dyxh"].abs()
    return dict(dx=(st["k0"] * st["dy"]).abs() + st["k1"].abs() + (st["xhat"] * st["k2"]).abs(),
                partial=torch.stack([slab_sums(dy, c), slab_sums(dyxh, c)], -1), dbeta=dy.sum((0, 1)), dgamma=dyxh.sum((0, 1)))


# ---------------------------------------------------------------------------------------------------- rows
def rows_dx(t, cpg):
    B, P, C = t.shape
    return t.reshape(B, P, GROUPS, cpg).permute(0, 2, 1, 3).reshape(B * GROUPS, P * cpg)


def rows_chan(t, cpg):
    return t.reshape(GROUPS, cpg)


def rows_partial(t, cpg):
    B, ns, C, _ = t.shape
    return t.reshape(B, ns, GROUPS, cpg * 2).reshape(B * ns * GROUPS, cpg * 2)


def acc_mask(c, acc_dx):
    """bool [C]: the channels whose source gradient the launch adds to."""
    ch = torch.arange(c.c0 + c.c1)
    return torch.where(ch < c.c0, torch.tensor(bool(acc_dx & 1)), torch.tensor(bool(acc_dx & 2)))


def bar(cls, r32):
    return min(CAP, max(FLOOR[cls], 4.0 * r32))


Target = collections.namedtuple("Target", "cls ref S y32")      # rows x elements each


@functools.lru_cache(maxsize=2)
def prepared(name, regime):
    """Everything a check of a case needs, computed once: dict(c, geo, o, given (the rows of a partial_ready case or None),
    targets {form: {output: Target}}, r32 {class}, bar {class}).  Read-only."""
    c = BY_NAME[name]
    geo, o = Geo(c), operands(c, regime)
    cpg = geo.cpg
    given = None
    if c.ready:
        s0 = statement(o, c, torch.float64)
        given = ready_rows(s0["dy"], s0["dyxh"], c)
    s64, s32 = statement(o, c, torch.float64, partial=given), statement(o, c, torch.float32, partial=given)
    S = scales(o, c, s64)
    fixed = {}
    if not c.ready:
        fixed["partial"] = Target("partial", rows_partial(s64["partial"], cpg), rows_partial(S["partial"], cpg), rows_partial(s32["partial"], cpg))
    for k in ("dgamma", "dbeta"):
        old = o["old_" + k]
        fixed[k] = Target("sums", rows_chan(s64[k] + old.double(), cpg), rows_chan(S[k] + old.double().abs(), cpg),
                          rows_chan(s32[k].float() + old, cpg))                # the launch: (float) of the fp64 fold, added in fp32
    targets = {}
    for form in c.forms:
        acc_dx, with_dres = form
        m = acc_mask(c, acc_dx)
        ref, Sx, y = s64["dx"], S["dx"], s32["dx"]
        if with_dres:
            ref, Sx, y = ref + o["dres"].double(), Sx + o["dres"].double().abs(), y + o["dres"]
        if acc_dx:
            old = torch.where(m, o["old_dx"], torch.zeros(()))
            ref, Sx = ref + old.double(), Sx + old.double().abs()
            y = torch.where(m, y + o["old_dx"], y)
        targets[form] = dict(fixed, dx=Target("dx", rows_dx(ref, cpg), rows_dx(Sx, cpg), rows_dx(y, cpg)))
    r32 = {}
    for outs in targets.values():
        for t in outs.values():
            r32[t.cls] = max(r32.get(t.cls, 0.0), row_error(t.y32, t.ref, t.S).max().item())
    return dict(c=c, geo=geo, o=o, given=given, targets=targets, r32=r32, bar={k: bar(k, v) for k, v in r32.items()})


@functools.lru_cache(maxsize=None)
def r32_of(name, regime):
    p = prepared(name, regime)
    return dict(p["r32"]), dict(p["bar"])


def judge(p, form, got):
    """got: {dx [B][P][C], dgamma [C], dbeta [C], partial [B][nslab][C][2] (absent for partial_ready)} -> [(output, class, worst row
    figure, its row, bar, rows beyond the bar, rows, figure over the whole tensor)]."""
    cpg, out = p["geo"].cpg, []
    shape = {"dx": rows_dx, "dgamma": rows_chan, "dbeta": rows_chan, "partial": rows_partial}
    for name, t in p["targets"][form].items():
        g = shape[name](torch.as_tensor(got[name]).detach().cpu().double(), cpg)
        e = row_error(g, t.ref, t.S)
        fig, row = worst_row(e)
        b = p["bar"][t.cls]
        out.append((name, t.cls, fig, row, b, int((~(e <= b)).sum()), e.numel(), global_error(g, t.ref)))
    return out


# ---------------------------------------------------------------------------------------------------- a model of the three passes
DEFECTS = ("quad_group", "chunk_last_image", "children_row_stride", "slab_tail", "acc_bits", "second_pass", "mean_hs_hs", "fold_trip_twice")
# defect -> the cases that must see it
SEEN_BY = {"quad_group": ("s01", "s04", "s05"), "chunk_last_image": ("s02", "s08", "s09"), "children_row_stride": ("s06", "s17"),
           "slab_tail": ("s01", "s03"), "acc_bits": ("s07",), "second_pass": ("s10",), "mean_hs_hs": ("s01", "s03", "s05"),
           "fold_trip_twice": ("s12", "s13")}


def _walk(lo, hi, R, drop_tail):
    """bool [hi - lo]: the pixels of [lo, hi) the unrolled-by-4 loop and its tail take (thread row tr starts at lo + tr, step R)."""
    m = np.zeros(max(hi - lo, 0), dtype=bool)
    for tr in range(R):
        p = lo + tr
        while p + 3 * R < hi:
            m[[p - lo, p + R - lo, p + 2 * R - lo, p + 3 * R - lo]] = True
            p += 4 * R
        while p < hi and not drop_tail:
            m[p - lo] = True
            p += R
    return m


def kernel_model(p, form, defect=None):
    """numpy fp64: reduce, fold and apply with the kernel's index arithmetic (csrc/gn_backward.hip) on the buffers a test hands the
    launch (outputs NaN, accumulating targets prefilled); `defect` plants one of DEFECTS.  -> the `got` dict of `judge`."""
    assert defect is None or defect in DEFECTS
    c, geo, o = p["c"], p["geo"], p["o"]
    B, P, C, cpg, R = c.B, geo.P, geo.C, geo.cpg, geo.R
    acc_dx, with_dres = form
    f = {k: v.double().numpy() for k, v in o.items() if k not in ("mean64", "rstd64")}
    ch = np.arange(C)
    grp_of = ((ch - ch % 4) if defect == "quad_group" else ch) // cpg              # chan_params: the group per element
    mu, rs = f["mean"][:, grp_of][:, None], f["rstd"][:, grp_of][:, None]          # [B][1][C]
    sc = f["gamma"] * rs
    sh = f["beta"] - mu * sc
    pix = np.arange(P)
    sy, sx = pix // c.Ws, pix % c.Ws
    da = f["da"].reshape(B, -1)                                                    # [B][Pa * C], row length C
    if c.a_mode == 0:
        g = f["da"]
    elif c.a_mode == 1:
        Wd = c.Ws if defect == "children_row_stride" else c.Ws * 2
        base = ((2 * sy * Wd + 2 * sx) * C)[:, None] + ch[None]
        g = (da[:, base] + da[:, base + C]) + (da[:, base + Wd * C] + da[:, base + Wd * C + C])
    else:
        Wd = c.Ws >> 1
        g = da[:, (((sy >> 1) * Wd + (sx >> 1)) * C)[:, None] + ch[None]] * 0.25
    xhat = (f["x"] - mu) * rs
    if c.act:
        y = f["x"] * sc + sh
        with np.errstate(over="ignore"):
            s = 1.0 / (1.0 + np.exp(-y))
        dy = g * (s * (1.0 + y * (1.0 - s)))
    else:
        dy = g
    passes = 1 if defect == "second_pass" else geo.npass
    done = ch < passes * geo.TQ * 4                                                # channels a pass reaches
    # pass 1
    if c.ready:
        partial = p["given"].numpy().copy()
    else:
        partial = np.full((B, c.nslab, C, 2), np.nan)
        for s_ in range(c.nslab):
            p0 = s_ * geo.sp
            p1 = min(p0 + geo.sp, P)
            m = _walk(p0, p1, R, defect == "slab_tail" and c.a_mode == 0)          # a_mode != 0 has no unrolled loop
            sel = p0 + np.nonzero(m)[0]
            partial[:, s_, :, 0] = dy[:, sel].sum(1)
            partial[:, s_, :, 1] = (dy * xhat)[:, sel].sum(1)
        partial[:, :, ~done] = np.nan
    # pass 2: all groups at once (same cpg, nbp, S): chan[image slot][C][2]
    n = float((c.Hs * c.Hs if defect == "mean_hs_hs" else c.Hs * c.Ws) * cpg)
    dgam, dbet = np.zeros(C), np.zeros(C)
    coef = np.full((B, C, 3), np.nan)
    for b0 in range(0, B, geo.nbp):
        chan = np.zeros((geo.nbp, C, 2))
        for bl in range(geo.nbp):
            b = b0 + bl
            if b >= B:
                continue
            for sl in range(geo.S):                                                # the slab lanes, then added in lane order
                k, acc = sl, np.zeros((C, 2))
                while k + 7 * geo.S < c.nslab:
                    for j in range(8):
                        acc += partial[b, k + j * geo.S] * (2.0 if defect == "fold_trip_twice" else 1.0)
                    k += 8 * geo.S
                while k < c.nslab:
                    acc += partial[b, k]
                    k += geo.S
                chan[bl] += acc
            gs = (chan[bl] * f["gamma"][:, None]).reshape(GROUPS, cpg, 2).sum(1)   # [GROUPS][2]
            r = f["rstd"][b][ch // cpg]
            coef[b, :, 0] = r * f["gamma"]
            coef[b, :, 1] = r * gs[ch // cpg, 0] / n
            coef[b, :, 2] = r * gs[ch // cpg, 1] / n
        lim = min(B - b0, geo.nbp) - (1 if defect == "chunk_last_image" else 0)
        for i in range(lim):
            dbet += chan[i, :, 0]
            dgam += chan[i, :, 1]
    # pass 3
    first = ch < c.c0
    mine = np.where(first, 2, 1) if defect == "acc_bits" else np.where(first, 1, 2)
    acc = (acc_dx & mine) != 0
    dst = np.where(acc_mask(c, acc_dx).numpy()[None, None], f["old_dx"], np.nan)   # what the test put there
    covered = np.zeros(P, dtype=bool)
    for s_ in range(geo.aslabs):
        p0 = s_ * geo.asp
        p1 = min(p0 + geo.asp, P)
        covered[p0:p1] = _walk(p0, p1, R, defect == "slab_tail")
    dx = coef[:, None, :, 0] * dy - coef[:, None, :, 1] - xhat * coef[:, None, :, 2]
    if with_dres:
        dx = dx + f["dres"]
    dx = np.where(acc[None, None], dx + dst, dx)
    dx = np.where(covered[None, :, None] & done[None, None], dx, dst)
    got = dict(dx=torch.from_numpy(dx), dgamma=torch.from_numpy(f["old_dgamma"] + dgam), dbeta=torch.from_numpy(f["old_dbeta"] + dbet))
    if not c.ready:
        got["partial"] = torch.from_numpy(partial)
    return got


def refusals():
    """[(what, struct field overrides on case s07 / s05)]: each must come back as the bad-argument status with nothing launched."""
    return (("partial_ready with a_mode 1", "s06", dict(partial_ready=1)), ("partial_ready with act 0", "s14", dict(partial_ready=1)),
            ("cpg 128", "s11", dict(groups=16)), ("a_mode 2 with an odd Hs", "s05", dict(Hs=11)), ("c0 % 4 != 0", "s07", dict(c0=254, c1=130)),
            ("a stride that is no multiple of 4", "s07", dict(da_ld=386)), ("c1 > 0 with x1 NULL", "s07", dict(x1=None)))


assert math.isclose(QUIET, 2.0 ** -10)
