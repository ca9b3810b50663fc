"""Shared by the element tests of the small inference kernels (tests/test_infer_op_reference.py on the CPU,
tests/test_gpu_infer_op_elements.py on the device): the seven kernels of csrc/unet_kernels.hip that every reverse-diffusion step
launches -- posemb, linear_small, conv_stem, conv_head, resample2x, softmax_rows, nhwc_to_nchw.  Seeded operands, the fp64 statement
of every output, a per-row error figure, fp32 CPU restatements and the bars.  torch on the CPU only; the library is not imported.
The forward twin of tests/train_op_cases.py, whose pieces (silu, _saturated_affine, _quiet_channels, border_mask, QUIET, GUARD) it
uses.

Why: tests/test_gpu_ops.py draws every operand ~ N(0, 1), reports one figure max |err| / max |ref| over the whole tensor, uses square
maps at the shapes of the shipped models only, and the forward ledger runs the same kernels at plan shapes.  A wrong value in a quiet
image, a quiet output channel, one border pixel of a non-square map or an element the launch never writes passes both; three of the
five stem kernels, the head's LDS kernel, the odd chunk count of its tap kernel, the 16-row split of the linear and the grid-stride
loops of posemb and nhwc_to_nchw are not reached at all.

Statements (`_fresh`): plain torch on the fp32-rounded operands; evaluated in fp64 they are the reference, in fp32 the restatement.
test_infer_op_reference.py holds each to stock fp64 torch.nn.functional.  The posemb statement is forward_ledger.posemb: the argument
as the kernel forms it in fp32 (two fp32 products), then sin / cos in fp64 (the restatement: in fp32).

Error figure (`row_error`): every element is compared; one number per output row,  max |got - ref| / max S  within the row.  A row is
the batch row of the linear and of posemb, the (image, output channel) plane of the stem and the head, the softmax row, the (image,
channel) plane of out_act, the (image, pixel range) row of the stem statistics.  S is the fp64 sum of the absolute values of the terms
of the element: sum_k |w| |a(x)| + |bias| (behind act_out: |silu'(pre)| S_pre + |silu(pre)|), the mean of |silu| over the four pixels
of out_act, sum |o| / sum o^2 of the statistics, the probability itself for the softmax (a quotient of positive terms), 1 for posemb
(its figure is absolute).  S >= |ref|.

Operand regimes: drawn in fp64 from a seeded generator, rounded once to fp32.
  iid        everything N(0, 1), weights N(0, 1 / K) (K the fan-in), GroupNorm rows scale = 1 + 0.1 n, shift = 0.1 n
  quiet_row  with B >= 2 batch row / image 0 scaled by 2^-10 (head: rows 0 of gn_scale and gn_shift); output features / channels /
             softmax rows n % 4 == 1 scaled by 2^-10 (their weights and bias; the logits of the softmax row)
  saturated  where SiLU is applied.  linear: x uniform over [-30, 30] with x[:, 0] = 0, x[:, 1] = the zero of silu', x[:, 2] = -90,
             x[:, 3] = -100 (__expf(-x) overflows below -88); with act_out bias -100 on n % 8 == 5 and +40 on n % 8 == 6.  head and
             out_act: train_op_cases._saturated_affine
  peaked     softmax only, the kind of row r is PEAKED[(r + index of the shape) % 5]: sigma32 (32 randn), spike (one entry at 500),
             offset (every entry + 1e4), tie (all entries equal), masked (entries i % 3 == 1 at -inf; never a whole row)
These are the first levels tried; test_infer_op_reference.py asserts 4 r32 <= CAP on every case and regime and none had to come down.

Bars (`bar`): r32 = the worst row of the fp32 restatement of the case, computed at run time; the device bar is
max(FLOOR[class], 4 r32), never above CAP[class], the bar the same kernel has today (TOL = 2e-5 of tests/test_gpu_ops.py; 2e-6
absolute for posemb; 1e-5 for the stem statistics).  The factor 4 is attn_cases.py's and train_op_cases.py's: another summation order
plus the hardware exponential and reciprocal.  FLOOR = 4 x the worst iid r32 of the class over all its shapes, measured by
test_infer_op_reference.py::test_floors, which holds each constant within a factor 1.5 of its measurement.  Nothing comes from a
device's output.

Bit for bit against the fp32 restatement: resample modes 1, 3 and 4, mode 2's plain output (((v00 + v01) + v10) + v11) * 0.25f,
nhwc_to_nchw, the cleared range of posemb."""
import collections
import functools
import math

import torch
import torch.nn.functional as F

from train_op_cases import (GUARD, QUIET, SILU_GRAD_ZERO, _quiet_channels, _round, _saturated_affine, border_mask, global_error, silu,
                            silu_grad, worst_row)

__all__ = ["GUARD", "QUIET", "border_mask", "global_error", "worst_row"]

TOL = 2e-5                                                   # tests/test_gpu_ops.py
CAP = {"linear": TOL, "stem": TOL, "head": TOL, "act": TOL, "softmax": TOL, "posemb": 2e-6, "stats": 1e-5}
# 4 x the worst iid row figure of the class's restatement over all its shapes, measured by test_infer_op_reference.py::test_floors:
# 4 x 1.39e-07 (linear: 16 x 36 -> 33, act_in), 4 x 1.95e-07 (stem: 2 x 16 x 32, Cin 2, Cout 32), 4 x 1.50e-07 (head: 3 x 16 x 16,
# C 32, Cout 2), 4 x 1.97e-07 (act: 3 x 1 x 7, C 96), 4 x 1.64e-07 (softmax: 7 x 63), 4 x 3.52e-08 (posemb: 5 x 130, scale 0.25; half an
# ulp of a value in [0.5, 1)), 4 x 1.50e-07 (stats: 2 x 16 x 32, Cin 2, Cout 32, one row per image).  Each is the largest of some
# hundred row figures and moves with the summation order of the BLAS behind matmul; a bar never depends on which
# side of its measurement the constant lies: it is max(FLOOR, 4 r32) with r32 measured at run time.
FLOOR = {"linear": 5.6e-7, "stem": 7.8e-7, "head": 6.0e-7, "act": 7.9e-7, "softmax": 6.6e-7, "posemb": 1.4e-7, "stats": 6.0e-7}

REGIMES = ("iid", "quiet_row", "saturated", "peaked")
OPS = ("linear", "posemb", "stem", "head", "resample", "softmax", "layout")
PEAKED = ("sigma32", "spike", "offset", "tie", "masked")

# (B, K, N, act_in, act_out, bias given): every B of {1, 3, 4, 5, 8, 9, 16, 17, 33} (both sides of the template widths 4, 8, 16; a
# second launch of one row; a third), every K of {4, 36, 64, 68, 200, 260} (K / 4 = 1, 9, 16, 17, 50 lanes of 64, and 65: one lane takes
# a second quad), every N of {1, 3, 4, 5, 17, 33} (N % 4: the last block's idle waves), the four activation pairs, bias NULL four
# times, and every pair (B in 16, 17, 33) x (ragged K in 36, 68, 200, 260)
LINEAR = ((1, 4, 1, 0, 0, 1), (3, 64, 3, 1, 0, 1), (4, 36, 4, 0, 1, 1), (5, 68, 5, 1, 1, 1), (8, 200, 17, 1, 0, 0), (9, 260, 33, 0, 0, 1),
          (1, 260, 33, 1, 1, 1), (3, 4, 5, 1, 1, 0), (4, 64, 17, 0, 0, 1), (5, 200, 1, 0, 1, 1), (8, 64, 4, 1, 1, 1), (9, 36, 3, 1, 0, 1),
          (16, 36, 33, 1, 0, 1), (16, 68, 5, 0, 1, 1), (16, 200, 4, 1, 1, 0), (16, 260, 17, 1, 0, 1),
          (17, 36, 17, 1, 1, 1), (17, 68, 33, 1, 0, 0), (17, 200, 5, 0, 0, 1), (17, 260, 3, 1, 1, 1),
          (33, 36, 5, 1, 0, 1), (33, 68, 1, 1, 1, 1), (33, 200, 33, 0, 1, 0), (33, 260, 4, 1, 0, 1))
# (B, dim, scale, zero_doubles): B * dim / 2 = 1 ... 19500 (77 blocks); zero_doubles odd, and 2 * 256 * 512 + 3: one and a half
# doubles past a full pass of the capped grid of 512 blocks
POSEMB_T = (0, 1, 17, 500, 999)
POSEMB_BIG = 2 * 256 * 512 + 3
POSEMB = ((1, 2, 1.0, 0), (5, 6, 0.25, 1), (300, 32, 1.0, 7), (5, 130, 0.25, POSEMB_BIG), (300, 130, 1.0, 0), (1, 32, 0.25, 7),
          (300, 2, 0.25, 1), (1, 6, 1.0, POSEMB_BIG), (5, 32, 1.0, 0))
# (B, H, W, Cin, Cout, stats, offset, key9).  stats: 0 none, -1 the rows anoddpm_stem_stats_rows gives (`stem_stats_rows` restates
# them), n > 0 the caller's rows per image.  offset: the input pointer is moved by so many floats (1: no 16-byte alignment, the generic
# kernel).  key9: anoddpm_internal_variant(9, key9) around the launch (1: one trip per workgroup where the launcher would take two).
STEM = ((1, 1, 8, 1, 4, 0, 0, 0),           # W == 8: a strip with neither neighbour; H == 1: no row above or below
        (3, 5, 24, 1, 32, 0, 0, 0),         # 45 strips over workgroups of 32: a partial last workgroup
        (1, 8, 16, 2, 12, 0, 0, 0),         # Cout / 4 = 3: 85 strips per workgroup and an idle lane
        (3, 10, 16, 1, 96, 0, 0, 0),        # Cout / 4 = 24: 10 strips per workgroup and 16 idle lanes
        (1, 64, 64, 1, 1024, 0, 0, 0),      # 512 workgroup trips: the two-trip kernel by the launcher's own rule
        (2, 7, 12, 1, 32, 0, 0, 0),         # W % 8 != 0: the generic kernel
        (1, 9, 16, 3, 32, 0, 0, 0),         # Cin > 2
        (2, 6, 8, 16, 12, 0, 0, 0),
        (1, 8, 16, 1, 32, 0, 1, 0),         # an input that is not 16-byte aligned
        (2, 16, 32, 1, 32, -1, 0, 0), (1, 10, 16, 2, 96, -1, 0, 0),
        (1, 16, 32, 1, 32, 1, 0, 0),        # 2 trips: conv_stem_strip2_kernel with statistics
        (2, 16, 32, 2, 32, 1, 0, 0),        # 2 trips, two input channels: the LOOP form
        (2, 32, 32, 1, 32, 1, 0, 0),        # 4 trips
        (1, 20, 16, 1, 96, 1, 0, 0),        # 4 trips of 10 strips
        (1, 64, 64, 1, 1024, 0, 0, 1))      # the two-trip shape held to one trip
# (B, H, W, C, Cout, key4).  key4: anoddpm_internal_variant(4, key4) around the launch -- 0 the launcher's choice (16 x 28 matrix-pipe
# tiles at C = 64 / 128 with Cout = 1, 16 x 16 matrix-pipe tiles at C = 64 / 128 and at C = 256 with Cout = 1, the tap kernel at other
# C % 32 == 0 (its chunk count C / 32 is odd at 32, 96, 160), the LDS kernel elsewhere), 1 the LDS kernel, 2 the tap kernel, 3 the
# 16 x 16 matrix-pipe tiles
HEAD = ((1, 8, 8, 128, 1, 0), (3, 8, 40, 64, 1, 0), (1, 40, 8, 128, 1, 0),
        (2, 32, 16, 128, 1, 0),             # a second 26-row strip of 6 rows, a second 14-column tile of 2 columns
        (1, 24, 72, 64, 3, 0), (2, 16, 16, 128, 4, 0), (1, 16, 24, 256, 1, 0), (1, 8, 40, 256, 3, 0), (3, 16, 16, 32, 2, 0),
        (1, 24, 8, 160, 4, 0), (2, 8, 16, 96, 1, 0), (1, 16, 8, 48, 2, 0), (3, 8, 8, 4, 1, 0), (1, 8, 24, 80, 4, 0),
        (2, 32, 16, 128, 1, 1), (2, 32, 16, 128, 1, 2), (2, 32, 16, 128, 1, 3), (1, 24, 72, 64, 3, 1), (1, 24, 72, 64, 3, 2))
# (mode, B, h, w, C), h x w the low-resolution map: modes 1 and 4 read it and write 2h x 2w, modes 2 and 3 read 2h x 2w and write it.
# Mode 2 comes with out_act.  C = 4: the smallest the entry point accepts, 12: no power of two
RESAMPLE = tuple((m, 3, h, w, C) for m in (1, 3, 4, 2) for h, w in ((3, 5), (1, 7), (8, 2)) for C in (4, 12, 96))
SOFTMAX = tuple((r, L) for r in (1, 2, 5, 7, 64) for L in (1, 16, 63, 64, 65, 100, 256))
SOFTMAX_SPARE_ROWS = 3                                       # NaN rows behind `rows`, before the GUARD elements
# (B, P, C, in_ld, first channel): the last is one element past a full pass of the capped grid (8192 blocks of 256)
LAYOUT = ((1, 1, 1, 1, 0), (3, 7, 5, 5, 0), (2, 300, 3, 8, 0), (1, 64, 4, 128, 60), (1, 699051, 3, 3, 0))
SHAPES = {"linear": LINEAR, "posemb": POSEMB, "stem": STEM, "head": HEAD, "resample": RESAMPLE, "softmax": SOFTMAX, "layout": LAYOUT}

# cls: the class of FLOOR / CAP, or "exact" (bit for bit); ref, S: fp64, shaped [rows, ...]; y: the fp32 restatement
Out = collections.namedtuple("Out", "cls ref S y")


def applies(op, shape, regime):
    if regime == "iid":
        return True
    if regime == "quiet_row":
        if op in ("posemb", "layout"):
            return False
        if op == "resample":
            return shape[0] == 2
        # something must be quiet: a second image, or an output channel n % 4 == 1
        return op != "head" or shape[0] >= 2 or shape[4] >= 2
    if regime == "saturated":
        return op == "head" or (op == "resample" and shape[0] == 2) or (op == "linear" and (shape[3] or shape[4]))
    return op == "softmax"                                  # peaked


def cases(op):
    """[(op, shape, regime)] of an operator, in a fixed order."""
    return [(op, s, r) for s in SHAPES[op] for r in REGIMES if applies(op, s, r)]


def case_id(item):
    op, shape, regime = item
    return f"{op}-{'x'.join(str(v) for v in shape)}-{regime}"


def _generator(op, shape, regime):
    return torch.Generator().manual_seed(9000 + 100003 * OPS.index(op) + 101 * SHAPES[op].index(shape) + REGIMES.index(regime))


def stem_stats_rows(H, W, Cin, Cout):
    """anoddpm_stem_stats_rows restated for the selector 9 at 0 (the device test holds the library to it on the shapes it uses)."""
    if not 1 <= Cin <= 2 or W % 8 or Cout % 4 or Cout // 4 > 256:
        return 0
    ppb, per_image = 256 // (Cout // 4), H * W // 8
    if per_image % ppb:
        return 0
    trips, iters = per_image // ppb, 1
    if Cin == 1 and trips % 2 == 0 and trips // 2 >= 256:
        iters = 2
    while trips // iters > 1024:
        iters *= 2
    while iters > 1 and trips % iters:
        iters //= 2
    return trips // iters


def stem_rows(shape):
    """Statistics rows per image of a stem case (0: none)."""
    B, H, W, Cin, Cout, stats = shape[:6]
    return stem_stats_rows(H, W, Cin, Cout) if stats < 0 else stats


# ---------------------------------------------------------------------------------------------------- operands
def operands(op, shape, regime):
    """dict of the fp32 operands of a case (and the launch's scalars)."""
    gen = _generator(op, shape, regime)

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float64)

    quiet, sat = regime == "quiet_row", regime == "saturated"
    if op == "linear":
        B, K, N, act_in, act_out, has_bias = shape
        x, w, bias = rn(B, K), rn(N, K) / math.sqrt(K), rn(N)
        if sat:
            x = torch.rand(B, K, generator=gen, dtype=torch.float64) * 60 - 30
            x[:, 0], x[:, 1], x[:, 2], x[:, 3] = 0.0, SILU_GRAD_ZERO, -90.0, -100.0
            if act_out:
                n = torch.arange(N)
                bias[n % 8 == 5], bias[n % 8 == 6] = -100.0, 40.0
        if quiet:
            w[_quiet_channels(N)] *= QUIET
            bias[_quiet_channels(N)] *= QUIET
            if B >= 2:
                x[0] *= QUIET
        o = dict(x=x, w=w, bias=bias if has_bias else None, act_in=act_in, act_out=act_out)
    elif op == "posemb":
        B, dim, scale, zero_doubles = shape
        half = dim // 2
        freqs = torch.exp(-torch.arange(half, dtype=torch.float64) * (math.log(1e4) / half))
        o = dict(t=torch.tensor([POSEMB_T[b % len(POSEMB_T)] for b in range(B)], dtype=torch.int64), freqs=freqs, dim=dim, scale=scale,
                 zero_doubles=zero_doubles)
    elif op == "stem":
        B, H, W, Cin, Cout = shape[:5]
        x, w, bias = rn(B, Cin, H, W), rn(Cout, Cin, 3, 3) / math.sqrt(9 * Cin), rn(Cout)
        if quiet:
            w[_quiet_channels(Cout)] *= QUIET
            bias[_quiet_channels(Cout)] *= QUIET
            if B >= 2:
                x[0] *= QUIET
        o = dict(x=x, w=w, bias=bias, rows=stem_rows(shape))
    elif op == "head":
        B, H, W, C, Cout = shape[:5]
        x, w, bias = rn(B, H, W, C), rn(Cout, C, 3, 3) / math.sqrt(9 * C), rn(Cout)
        scale, shift = 1 + 0.1 * rn(B, C), 0.1 * rn(B, C)
        if sat:
            scale, shift = _saturated_affine(B, C, gen)
        if quiet:
            w[_quiet_channels(Cout)] *= QUIET
            bias[_quiet_channels(Cout)] *= QUIET
            if B >= 2:
                scale[0] *= QUIET
                shift[0] *= QUIET
        o = dict(x=x, w=w, bias=bias, scale=scale, shift=shift)
    elif op == "resample":
        mode, B, h, w, C = shape
        x = rn(B, h, w, C) if mode in (1, 4) else rn(B, 2 * h, 2 * w, C)
        scale, shift = 1 + 0.1 * rn(B, C), 0.1 * rn(B, C)
        if sat:
            scale, shift = _saturated_affine(B, C, gen)
        if quiet:
            x[..., _quiet_channels(C)] *= QUIET
            x[0] *= QUIET
        o = dict(x=x, scale=scale, shift=shift, mode=mode)
    elif op == "softmax":
        rows, L = shape
        x = rn(rows, L)
        if quiet:
            x[_quiet_channels(rows)] *= QUIET
            if rows >= 2:
                x[0] *= QUIET
        if regime == "peaked":
            for r in range(rows):
                kind = peaked_kind(shape, r)
                if kind == "sigma32":
                    x[r] *= 32
                elif kind == "spike":
                    x[r, (5 * r + 3) % L] = 500.0
                elif kind == "offset":
                    x[r] += 1e4
                elif kind == "tie":
                    x[r] = x[r, 0]
                elif L > 1:                                           # masked; never a whole row
                    x[r, torch.arange(L) % 3 == 1] = -math.inf
        o = dict(x=x)
    elif op == "layout":
        B, P, C, in_ld, c0 = shape
        o = dict(x=rn(B, P, in_ld), c0=c0, C=C)
    else:
        raise KeyError(op)
    return _round(o)


def peaked_kind(shape, r):
    return PEAKED[(r + SOFTMAX.index(shape)) % len(PEAKED)]


# ---------------------------------------------------------------------------------------------------- statements
def conv3(a, w, bias):
    """3x3, zero padding 1, as one product over the unfolded map: [B, C, H, W], [N, C, 3, 3], [N] -> [B, N, H, W]."""
    B, C, H, W = a.shape
    return (torch.einsum("nk,bkp->bnp", w.reshape(w.shape[0], -1), F.unfold(a, 3, padding=1)) + bias[None, :, None]).view(B, -1, H, W)


def pool4(v):
    """[B, 2h, 2w, C] -> [B, h, w, C]: the four pixels in the kernel's order."""
    return (((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + v[:, 1::2, 0::2]) + v[:, 1::2, 1::2]) * 0.25


def posemb_arg(o):
    """fp32 [B, half]: the argument as anoddpm_posemb forms it -- ((float) t * scale) * freqs, two fp32 products."""
    return (o["t"].to(torch.float32) * float(o["scale"]))[:, None] * o["freqs"].to(torch.float32)[None, :]


def range_sums(y, rows):
    """[B, Cout, H, W] -> ([B * rows, Cout] sums, the same of squares) over the `rows` contiguous pixel ranges of each image."""
    B, N = y.shape[:2]
    r = y.reshape(B, N, rows, -1)
    return r.sum(3).transpose(1, 2).reshape(B * rows, N).contiguous(), (r * r).sum(3).transpose(1, 2).reshape(B * rows, N).contiguous()


def _fresh(op, o, dt):
    """{name: (class, value shaped [rows, ...])} in dtype dt: fp64 is the reference, fp32 the restatement."""
    def c(t):
        return t.to(dt)

    if op == "linear":
        x, w = c(o["x"]), c(o["w"])
        pre = (silu(x) if o["act_in"] else x) @ w.t()
        if o["bias"] is not None:
            pre = pre + c(o["bias"])
        return {"out": ("linear", silu(pre) if o["act_out"] else pre)}
    if op == "posemb":
        arg = c(posemb_arg(o))
        return {"out": ("posemb", torch.cat([arg.sin(), arg.cos()], 1))}
    if op == "stem":
        y = conv3(c(o["x"]), c(o["w"]), c(o["bias"]))
        return {"out": ("stem", y.flatten(0, 1))}
    if op == "head":
        a = silu(c(o["x"]) * c(o["scale"])[:, None, None] + c(o["shift"])[:, None, None]).permute(0, 3, 1, 2)
        return {"out": ("head", conv3(a, c(o["w"]), c(o["bias"])).flatten(0, 1))}
    if op == "resample":
        x, mode = c(o["x"]), o["mode"]
        if mode == 1:
            return {"out": ("exact", x.repeat_interleave(2, 1).repeat_interleave(2, 2))}
        if mode == 3:
            return {"out": ("exact", x[:, 0::2, 0::2])}
        if mode == 4:
            B, h, w, C = x.shape
            out = torch.zeros(B, 2 * h, 2 * w, C, dtype=dt)
            out[:, 0::2, 0::2] = x
            return {"out": ("exact", out)}
        a = pool4(silu(x * c(o["scale"])[:, None, None] + c(o["shift"])[:, None, None]))
        return {"out": ("exact", pool4(x)), "act": ("act", a.permute(0, 3, 1, 2).flatten(0, 1))}
    if op == "softmax":
        x = c(o["x"])
        e = torch.exp(x - x.amax(-1, keepdim=True))
        return {"out": ("softmax", e / e.sum(-1, keepdim=True))}
    if op == "layout":
        return {"out": ("exact", c(o["x"])[:, :, o["c0"]:o["c0"] + o["C"]].transpose(1, 2).contiguous())}
    raise KeyError(op)


def _scale(op, o):
    """{name: S} fp64: the sum of the absolute values of the terms of each element."""
    def c(t):
        return t.double()

    if op == "linear":
        x, w = c(o["x"]), c(o["w"])
        a = silu(x) if o["act_in"] else x
        pre, S = a @ w.t(), a.abs() @ w.abs().t()
        if o["bias"] is not None:
            pre, S = pre + c(o["bias"]), S + c(o["bias"]).abs()
        return {"out": silu_grad(pre).abs() * S + silu(pre).abs() if o["act_out"] else S}
    if op == "posemb":
        return {"out": torch.ones(o["t"].numel(), o["dim"], dtype=torch.float64)}
    if op == "stem":
        return {"out": conv3(c(o["x"]).abs(), c(o["w"]).abs(), c(o["bias"]).abs()).flatten(0, 1)}
    if op == "head":
        a = silu(c(o["x"]) * c(o["scale"])[:, None, None] + c(o["shift"])[:, None, None]).abs().permute(0, 3, 1, 2)
        return {"out": conv3(a, c(o["w"]).abs(), c(o["bias"]).abs()).flatten(0, 1)}
    if op == "resample":
        ref = _fresh(op, o, torch.float64)
        S = {"out": ref["out"][1].abs()}
        if o["mode"] == 2:
            x = c(o["x"])
            S["out"] = pool4(x.abs())
            a = silu(x * c(o["scale"])[:, None, None] + c(o["shift"])[:, None, None]).abs()
            S["act"] = pool4(a).permute(0, 3, 1, 2).flatten(0, 1)
        return S
    if op in ("softmax", "layout"):
        return {"out": _fresh(op, o, torch.float64)["out"][1].abs()}
    raise KeyError(op)


def outputs(op, o):
    """{name: Out} of a case; a stem with statistics rows also states them over its own fp32 restatement (the device test states
    them over the buffer the launch wrote, with `stats_outputs`)."""
    ref, y32, S = _fresh(op, o, torch.float64), _fresh(op, o, torch.float32), _scale(op, o)
    outs = {k: Out(cls, r.contiguous(), S[k].contiguous(), y32[k][1].contiguous()) for k, (cls, r) in ref.items()}
    if op == "stem" and o["rows"]:
        B, (Cin, H, W) = o["x"].shape[0], o["x"].shape[1:]
        outs.update(stats_outputs(y32["out"][1].view(B, -1, H, W), o["rows"]))
    return outs


def stats_outputs(y, rows):
    """{"sum", "sq": Out} of the statistics rows of an fp32 output y [B, Cout, H, W]: fp64 sums of every row's own contiguous pixel
    range, S = the sums of |.|, restated as fp32 sums."""
    s64, q64 = range_sums(y.double(), rows)
    a64, _ = range_sums(y.double().abs(), rows)
    s32, q32 = range_sums(y.float(), rows)
    return {"sum": Out("stats", s64, a64, s32), "sq": Out("stats", q64, q64, q32)}


# ---------------------------------------------------------------------------------------------------- the figure and the bars
def row_error(got, ref, S):
    """[rows] fp64: per output row (dimension 0 of ref) max |got - ref| / max S; inf where an element is not what it should be and
    the difference is not finite (NaN, or an infinity the reference does not have)."""
    R = ref.shape[0]
    e = (got.detach().double().cpu().reshape(ref.shape) - ref).abs().reshape(R, -1)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf"))).amax(1)
    return e / S.reshape(R, -1).amax(1).clamp_min(1e-300)


def border_error(got, ref, S, mask):
    """row_error over the pixels of `mask` [H, W] alone (ref: [rows, H * W]), against the same max S of the whole row."""
    R = ref.shape[0]
    e = (got.detach().double().cpu().reshape(ref.shape) - ref).abs().reshape(R, -1)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    e = torch.where(mask.reshape(1, -1), e, torch.zeros_like(e)).amax(1)
    return e / S.reshape(R, -1).amax(1).clamp_min(1e-300)


def bar(cls, r32):
    return min(CAP[cls], max(FLOOR[cls], 4.0 * r32))


@functools.lru_cache(maxsize=None)
def prepared(op, shape, regime):
    """Everything a check of a case needs, computed once and shared, read-only, by the tests of a session:
    dict(o (operands), outs {name: Out}, r32 {class: worst row of the restatement over the outputs}, bar {class})."""
    o = operands(op, shape, regime)
    outs = outputs(op, o)
    r32 = {}
    for out in outs.values():
        if out.cls != "exact":
            r32[out.cls] = max(r32.get(out.cls, 0.0), row_error(out.y, out.ref, out.S).max().item())
    return dict(o=o, outs=outs, r32=r32, bar={cls: bar(cls, r) for cls, r in r32.items()})
