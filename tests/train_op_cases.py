"""Shared by the element tests of the small training kernels (tests/test_train_op_reference.py on the CPU,
tests/test_gpu_train_op_elements.py on the device): csrc/train_kernels.hip -- linear_small_backward and its batched form,
softmax_rows_backward, transpose_square, colsum_fold, conv_stem_backward, conv_head_backward -- the backward modes of resample2x and
the dropout kernel of csrc/unet_kernels.hip.  Seeded operands, the fp64 statement of every output, a per-row error figure, fp32 CPU
restatements, the bars, and the exact dropout mask.  numpy and torch on the CPU only; the library is not imported.

Why: tests/test_gpu_train_ops.py draws every operand ~ N(0, 1), reports one figure max |err| / max |ref| over the whole tensor, takes
fp32 autograd on the device as the reference of three kernels, and uses shapes that reach none of the kernels' guards (K % 64, rows % 4,
the unrolled column sum, N > 64, channel-quad counts that do not divide 256, non-square maps, the pixel-chunk boundaries, NULL
outputs).  A wrong value in a quiet batch row, a quiet output channel or one border pixel passes it, and so does an element the launch
never writes.

Statements (`_fresh`): plain torch on the fp32-rounded operands; evaluated in fp64 they are the reference, in fp32 the restatement.
test_train_op_reference.py holds each to fp64 autograd of the expression it is the backward of: F.linear(silu(x)), softmax,
F.conv2d(padding=1) (stem), conv2d(silu(x * scale + shift)) (head), nearest x2 and the 2x2 average, a plain column sum.

Error figure (`row_error`): every element is compared; one number per output row,  max |got - ref| / max S  within the row.  A row is
the batch row b of dx, da, dimg and the resampled map, the output channel / filter n of dw, db and dbias, the softmax row.  S is the
fp64 sum of the absolute values of the terms that make the element (sum_n |dy| |w| . |silu'(x)| for dx, ...) plus |old value| where
the launch accumulates.  S >= |ref|, so within a row the figure is never looser than max |err| / max |ref|.

Operand regimes: drawn in fp64 from a seeded generator, rounded once to fp32.
  iid        everything N(0, 1), weights N(0, 1 / K) (K the fan-in), GroupNorm rows scale = 1 + 0.1 n, shift = 0.1 n
  quiet_row  with B >= 2 batch row 0 of the activations and of dy scaled by 2^-10; output channels n % 4 == 1 of dy scaled by 2^-10
             (softmax: dp of row 0 and of rows r % 4 == 1; colsum_fold: image 0 and the columns n % 4 == 1)
  saturated  where SiLU or its derivative is applied.  linear: x uniform over [-30, 30] with x[:, 0] = 0, x[:, 1] = the zero of silu'
             (-1.2784645...), x[:, 2] = -90, x[:, 3] = -100 (__expf(-x) overflows below -88).  head, dropout mode 0: GroupNorm rows with
             scale 8 on c % 16 == 3 (1 elsewhere, times 1 + 0.1 n per image) and shift from {-4, 0, +4}
  peaked     softmax only: rows r % 3 == 0 one-hot (dp must come back exactly 0 off the hot entry), r % 3 == 1 a two-way tie,
             r % 3 == 2 one entry at 1 - 2^-20 and the rest sharing 2^-20
These are the first levels tried; test_train_op_reference.py asserts 4 r32 <= CAP on every case and regime and none had to come down.

Bars (`bar`): r32 = the worst row of the fp32 restatement of the case, computed at run time; the device bar is
max(FLOOR[class], 4 r32), never above CAP[class], the bar of the same kernel in tests/test_gpu_train_ops.py.  The factor 4 is
attn_cases.py's: another summation order plus the hardware exponential and reciprocal.  FLOOR = 4 x the worst iid r32 of the class over
all its shapes, measured by test_train_op_reference.py::test_floors, which holds each constant within a factor 1.5 of its measurement.
The restatements sum in fp32 through torch's matmul / sum; the column sum is the plain sequential loop.

Accumulating targets (acc_w, acc_x, accumulate; dw / db of the stem and the head and dbias of colsum_fold always add) are prefilled
with a seeded N(0, 1) tensor `old`; `target(out, acc)` gives the reference, S and restatement of either form.

Dropout (`dropout_keep`): the documented keep rule restated in numpy uint64: z = seed + idx * 0x9E3779B97F4A7C15 through the
splitmix64 finaliser, keep iff the high 32 bits >= floor(p * 2^32), idx = b * n + i; a kept value is x * (1 / (1 - p)) in fp32."""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

QUIET = 2.0 ** -10
GUARD = 64                                                   # NaN elements behind every output buffer; they come back untouched
# the bar of the same kernel in tests/test_gpu_train_ops.py (dropout mode 0: the issue's 2e-5)
CAP = {"linear": 1e-5, "softmax": 1e-5, "stem": 2e-5, "head": 2e-5, "head_dw": 5e-5, "resample": 1e-6, "colsum": 1e-6, "dropout": 2e-5}
# 4 x the worst iid row figure of the class's restatement over all its shapes, measured by test_train_op_reference.py::test_floors:
# 4 x 1.80e-07 (linear: B = 8, K = 68, N = 15), 4 x 8.97e-08 (softmax: 64 x 63), 4 x 2.04e-07 (stem: 61 x 25 x 41, Cin 1, Cout 4),
# 4 x 1.70e-07 (head da / db: 3 x 23 x 22, C 256, Cout 3), 4 x 1.19e-07 (head dW: one pixel, C 96), 4 x 6.80e-08 (resample: the sum of
# four), 4 x 1.30e-07 (colsum: 3 x 128 x 130, the sequential sum), 4 x 1.40e-07 (dropout mode 0: 2 x 2400, C 96).  Each is the largest
# of some thousand row figures and moves with the summation order of the BLAS behind matmul and conv2d (conv_cases.FLOOR); a bar never
# depends on which side of its measurement the constant lies: it is max(FLOOR, 4 r32) with r32 measured at run time.
FLOOR = {"linear": 7.2e-7, "softmax": 3.6e-7, "stem": 8.1e-7, "head": 6.8e-7, "head_dw": 4.8e-7, "resample": 2.7e-7, "colsum": 5.2e-7,
         "dropout": 5.6e-7}

REGIMES = ("iid", "quiet_row", "saturated", "peaked")
OPS = ("linear", "linear_batch", "softmax", "colsum", "stem", "head", "resample", "dropout0")

# (B, K, N, act_in): every B of {1, 3, 4, 5, 8, 9, 16} (both sides of the template widths 4, 8, 16), every K of {4, 36, 64, 68, 200}
# (a lone partial chunk, an exact chunk, a chunk plus four lanes, a ragged last chunk), every N of {1, 15, 16, 17, 33} (fewer output
# channels than the 16 waves, exactly 16, a tail), and every pair (B in 4, 5, 8, 9, 16) x (ragged K in 36, 68, 200)
LINEAR = ((1, 4, 1, 0), (3, 64, 16, 1), (1, 200, 33, 1), (3, 36, 15, 0),
          (4, 36, 17, 1), (4, 68, 33, 0), (4, 200, 15, 1),
          (5, 36, 16, 0), (5, 68, 17, 1), (5, 200, 1, 1),
          (8, 36, 33, 1), (8, 68, 15, 1), (8, 200, 16, 0),
          (9, 36, 1, 1), (9, 68, 16, 0), (9, 200, 17, 1),
          (16, 36, 15, 1), (16, 68, 33, 1), (16, 200, 17, 0), (16, 64, 33, 1), (16, 4, 16, 1))
# launch forms of linear_small_backward: (acc_w, acc_x, db given, dx given)
LINEAR_FORMS = ((1, 1, True, True), (0, 0, True, True), (0, 1, False, True), (1, 0, True, False))
# (njobs, B, K); job j has N = BATCH_N[j] (max_n exceeds most of them) and act_in is 1; job 1 (job 0 of a single job) has db = NULL
# in the forms that say so
BATCH = ((1, 5, 68), (3, 5, 68), (5, 5, 68), (1, 16, 64), (3, 16, 64), (5, 16, 64))
BATCH_N = (33, 4, 64, 17, 1)
# launch forms of the batch: (acc_w, acc_x, one job without db, dx and ws given)
BATCH_FORMS = ((1, 1, True, True), (0, 0, False, True), (1, 0, True, False))
SOFTMAX = tuple((r, L) for r in (1, 2, 5, 7, 64) for L in (1, 16, 63, 64, 65, 100, 256))
SOFTMAX_SPARE_ROWS = 3                                       # NaN rows behind `rows` (the row guard), before the GUARD elements
TRANSPOSE = tuple((Z, L) for Z in (1, 3) for L in (1, 31, 32, 33, 100))
# (B, ipb, N): ipb around the 8 x 16 unrolled loop (entered from 113 on) and the 16 item lanes; N around the 64 channels of a block
COLSUM = tuple((B, ipb, N) for B in (1, 3) for ipb in (1, 7, 16, 17, 112, 113, 128, 129, 300, 512) for N in (1, 40, 64, 65, 130))
# (B, H, W, Cin, Cout): pixel counts 1, 7, 60, 1024, 1025, 1023 (the 1024-pixel chunk); Cout / 4 = 1, 3, 8, 24, 64 (24 and 3 do not
# divide 256); every value once, each map with B = 1 and B = 3.  The last: 61 x 2 = 122 partial rows, the first size at which the fold
# of the partial rows (fold_rows8: eight row lanes, sixteen loads in flight while k + 120 < rows) enters its unrolled loop
STEM = ((1, 1, 1, 1, 4), (3, 1, 7, 2, 12), (1, 5, 12, 3, 32), (3, 32, 32, 1, 96), (1, 25, 41, 16, 256), (3, 33, 31, 3, 12),
        (1, 32, 32, 2, 256), (3, 25, 41, 1, 4), (1, 33, 31, 16, 96), (3, 5, 12, 16, 32), (1, 1, 7, 3, 96), (3, 1, 1, 2, 32), (61, 25, 41, 1, 4))
# (B, H, W, C, Cout): pixel counts 1, 15, 512, 513, 506 (the 512-pixel chunk); C / 4 = 1, 8, 24, 64; the last: 122 partial rows, as
# in STEM
HEAD = ((1, 1, 1, 4, 1), (3, 3, 5, 32, 2), (1, 16, 32, 96, 3), (3, 19, 27, 256, 4), (1, 23, 22, 32, 4), (3, 16, 32, 4, 1),
        (1, 19, 27, 96, 2), (3, 23, 22, 256, 3), (1, 3, 5, 256, 1), (3, 1, 1, 96, 4), (1, 16, 32, 256, 2), (3, 19, 27, 4, 3), (61, 19, 27, 4, 1))
# (mode, B, h, w, C), h x w the low-resolution map: mode 2 with scale 4 (the backward of nearest x2) reads [B, 2h, 2w, C] and writes
# [B, h, w, C]; mode 1 with scale 0.25 (the backward of the 2x2 average) reads [B, h, w, C] and writes [B, 2h, 2w, C].  C = 4 is the
# smallest the entry point accepts (C % 4 == 0), 12 is no power of two
RESAMPLE = tuple((m, 3, h, w, C) for m in (2, 1) for h, w in ((3, 5), (1, 7)) for C in (4, 12))
# dropout mode 1 (bit for bit): (B, n, C) x p x seed, and one map of n / 4 > 8192 * 256 quads (a second round of the grid-stride loop)
DROPOUT_SHAPES = ((1, 4, 4), (3, 4 * 257, 4), (2, 96 * 25, 96))
DROPOUT_P = (0.0, 0.1, 0.3, 0.5, 0.999)
DROPOUT_SEEDS = (0, 1, 2 ** 63 + 5)
DROPOUT_BIG = (1, 4 * (8192 * 256 + 3), 4)
# dropout mode 0 (values under the figure): (B, n, C, p, seed)
DROPOUT0 = tuple((B, n, C, p, seed) for (B, n, C), (p, seed) in zip(DROPOUT_SHAPES * 2, ((0.1, 0), (0.5, 1), (0.3, 2 ** 63 + 5),
                                                                                           (0.999, 1), (0.0, 0), (0.5, 2 ** 63 + 5))))
SHAPES = {"linear": LINEAR, "linear_batch": BATCH, "softmax": SOFTMAX, "colsum": COLSUM, "stem": STEM, "head": HEAD,
          "resample": RESAMPLE, "dropout0": DROPOUT0}

# cls: the class of FLOOR / CAP; ref0, S0: fp64, without the old value; old: fp32 prefill of an accumulating target or None;
# y0: the fp32 restatement, without the old value
Out = collections.namedtuple("Out", "cls ref0 S0 old y0")


def applies(op, shape, regime):
    if regime == "iid":
        return True
    if regime == "quiet_row":
        return op != "dropout0"
    if regime == "saturated":
        return op in ("linear_batch", "head", "dropout0") or (op == "linear" and shape[3] == 1)
    return op == "softmax"                                  # peaked


def cases(op):
    """[(op, shape, regime)] of an operator, in a fixed order."""
    return [(op, s, r) for s in SHAPES[op] for r in REGIMES if applies(op, s, r)]


def case_id(item):
    op, shape, regime = item
    return f"{op}-{'x'.join(str(v) for v in shape)}-{regime}"


# ---------------------------------------------------------------------------------------------------- pieces
def silu(x):
    return x * torch.sigmoid(x)


def silu_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def _silu_grad_zero():
    x = -1.2785
    for _ in range(8):                                      # Newton on f = 1 + x (1 - sigmoid(x)); f' = 1 - s - x s (1 - s)
        s = 1.0 / (1.0 + math.exp(-x))
        x -= (1 + x * (1 - s)) / (1 - s - x * s * (1 - s))
    return x


SILU_GRAD_ZERO = _silu_grad_zero()                           # -1.2784645427610737


def _generator(op, shape, regime):
    return torch.Generator().manual_seed(7000 + 100003 * OPS.index(op) + 101 * SHAPES[op].index(shape) + REGIMES.index(regime))


def _quiet_channels(n):
    return torch.arange(n) % 4 == 1


def _saturated_affine(B, C, gen):
    """GroupNorm rows [B, C] of the saturated regime: activations reach +-30."""
    scale = torch.where(torch.arange(C) % 16 == 3, 8.0, 1.0).double()[None] * (1 + 0.1 * torch.randn(B, C, generator=gen, dtype=torch.float64))
    shift = 4.0 * (torch.randint(0, 3, (B, C), generator=gen) - 1).double()
    return scale, shift


def _unfold3(t):
    """[B, C, H, W] -> [B, C * 9, H * W]: row c * 9 + tap holds the zero-padded map shifted by the tap."""
    return F.unfold(t, 3, padding=1)


def _conv_t(d, w):
    """The data gradient of conv2d(padding=1): [B, N, H, W], [N, C, 3, 3] -> [B, C, H, W]."""
    return F.conv2d(d, w.transpose(0, 1).flip(2, 3), padding=1)


def border_mask(H, W):
    m = torch.zeros(H, W, dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return m


# ---------------------------------------------------------------------------------------------------- operands
def operands(op, shape, regime):
    """dict of the fp32 operands of a case (and the launch's scalars)."""
    gen = _generator(op, shape, regime)

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float64)

    quiet = regime == "quiet_row"
    if op in ("linear", "linear_batch"):
        if op == "linear":
            B, K, N, act_in = shape
            Ns = (N,)
        else:
            (njobs, B, K), act_in = shape, 1
            Ns = BATCH_N[:njobs]
        x = rn(B, K)
        if regime == "saturated":
            x = torch.rand(B, K, generator=gen, dtype=torch.float64) * 60 - 30
            x[:, 0], x[:, 1], x[:, 2], x[:, 3] = 0.0, SILU_GRAD_ZERO, -90.0, -100.0
        if quiet and B >= 2:
            x[0] *= QUIET
        o = dict(x=x, old_dx=rn(B, K), act_in=act_in, jobs=[])
        for N in Ns:
            dy = rn(B, N)
            if quiet:
                dy[:, _quiet_channels(N)] *= QUIET
                if B >= 2:
                    dy[0] *= QUIET
            o["jobs"].append(dict(w=rn(N, K) / math.sqrt(K), dy=dy, old_dw=rn(N, K), old_db=rn(N)))
    elif op == "softmax":
        rows, L = shape
        p = torch.softmax(2 * rn(rows, L), -1)
        dp = rn(rows, L)
        if regime == "peaked":
            hot = torch.randint(0, L, (rows,), generator=gen)
            for r in range(rows):
                h, h2 = hot[r].item(), (hot[r].item() + 1 + L // 3) % L
                p[r] = 0.0
                if r % 3 == 0 or L == 1 or (r % 3 == 1 and h2 == h):
                    p[r, h] = 1.0
                elif r % 3 == 1:
                    p[r, h], p[r, h2] = 0.5, 0.5
                else:
                    p[r] = 2.0 ** -20 / (L - 1)
                    p[r, h] = 1 - 2.0 ** -20
        if quiet:
            dp[_quiet_channels(rows)] *= QUIET
            if rows >= 2:
                dp[0] *= QUIET
        o = dict(p=p, dp=dp)
    elif op == "colsum":
        B, ipb, N = shape
        cs = rn(B, ipb, N)
        if quiet:
            cs[:, :, _quiet_channels(N)] *= QUIET
            if B >= 2:
                cs[0] *= QUIET
        o = dict(colsum=cs, old_dbias=rn(N))
    elif op == "stem":
        B, H, W, Cin, Cout = shape
        x, dy = rn(B, Cin, H, W), rn(B, H * W, Cout)
        if quiet:
            dy[:, :, _quiet_channels(Cout)] *= QUIET
            if B >= 2:
                x[0] *= QUIET
                dy[0] *= QUIET
        o = dict(x=x, w=rn(Cout, Cin, 3, 3) / math.sqrt(9 * Cin), dy=dy, old_dw=rn(Cout, Cin, 3, 3), old_db=rn(Cout))
    elif op == "head":
        B, H, W, C, Cout = shape
        x, dy = rn(B, H * W, C), rn(B, Cout, H, W)
        scale, shift = 1 + 0.1 * rn(B, C), 0.1 * rn(B, C)
        if regime == "saturated":
            scale, shift = _saturated_affine(B, C, gen)
        if quiet:
            dy[:, _quiet_channels(Cout)] *= QUIET
            if B >= 2:
                x[0] *= QUIET
                dy[0] *= QUIET
        o = dict(x=x, scale=scale, shift=shift, w=rn(Cout, C, 3, 3) / math.sqrt(9 * C), dy=dy, old_dw=rn(Cout, C, 3, 3), old_db=rn(Cout))
    elif op == "resample":
        mode, B, h, w, C = shape
        g = rn(B, 2 * h, 2 * w, C) if mode == 2 else rn(B, h, w, C)
        if quiet:
            g[..., _quiet_channels(C)] *= QUIET
            g[0] *= QUIET
        o = dict(g=g, old=rn(B, h, w, C) if mode == 2 else rn(B, 2 * h, 2 * w, C), mode=mode, scale=4.0 if mode == 2 else 0.25)
    elif op == "dropout0":
        B, n, C, p, seed = shape
        scale, shift = 1 + 0.1 * rn(B, C), 0.1 * rn(B, C)
        if regime == "saturated":
            scale, shift = _saturated_affine(B, C, gen)
        o = dict(x=rn(B, n), scale=scale, shift=shift, p=p, seed=seed, keep=torch.from_numpy(dropout_keep(seed, B, n, p)))
    else:
        raise KeyError(op)
    return _round(o)


def _round(v):
    if torch.is_tensor(v):
        return v.float() if v.dtype == torch.float64 else v
    if isinstance(v, dict):
        return {k: _round(t) for k, t in v.items()}
    if isinstance(v, list):
        return [_round(t) for t in v]
    return v


# ---------------------------------------------------------------------------------------------------- statements
def _fresh(op, o, dt):
    """{name: (class, value without the old one, old or None)} in dtype dt: fp64 is the reference, fp32 the restatement."""
    def c(t):
        return t.to(dt)

    if op in ("linear", "linear_batch"):
        x = c(o["x"])
        a = silu(x) if o["act_in"] else x
        out, dx = {}, 0
        for j, job in enumerate(o["jobs"]):
            dy, w = c(job["dy"]), c(job["w"])
            out[f"dw{j}"] = ("linear", dy.t() @ a, job["old_dw"])
            out[f"db{j}"] = ("linear", dy.sum(0), job["old_db"])
            dx = dx + dy @ w                                              # the jobs in order
        out["dx"] = ("linear", dx * silu_grad(x) if o["act_in"] else dx, o["old_dx"])
        return out
    if op == "softmax":
        p, dp = c(o["p"]), c(o["dp"])
        return {"dp": ("softmax", p * (dp - (p * dp).sum(-1, keepdim=True)), None)}
    if op == "colsum":
        cs = c(o["colsum"])
        if dt == torch.float64:
            dimg = cs.sum(1)
            dbias = dimg.sum(0)
        else:                                                             # the plain loop: items in order, then the images in order
            dimg = torch.zeros_like(cs[:, 0])
            for i in range(cs.shape[1]):
                dimg = dimg + cs[:, i]
            dbias = torch.zeros_like(dimg[0])
            for b in range(cs.shape[0]):
                dbias = dbias + dimg[b]
        return {"dimg": ("colsum", dimg, None), "dbias": ("colsum", dbias, o["old_dbias"])}
    if op == "stem":
        x, w = c(o["x"]), c(o["w"])
        B, Cin, H, W = x.shape
        d = c(o["dy"]).transpose(1, 2)                                    # [B, Cout, P]
        dw = torch.einsum("bnp,bkp->nk", d, _unfold3(x)).view(w.shape)
        return {"dw": ("stem", dw, o["old_dw"]), "db": ("stem", d.sum(dim=(0, 2)), o["old_db"]),
                "dx": ("stem", _conv_t(d.reshape(B, -1, H, W), w), None)}
    if op == "head":
        w, dy = c(o["w"]), c(o["dy"])
        B, Cout, H, W = dy.shape
        a = silu(c(o["x"]) * c(o["scale"])[:, None] + c(o["shift"])[:, None])                 # [B, P, C]
        a = a.view(B, H, W, -1).permute(0, 3, 1, 2)
        dw = torch.einsum("bnp,bkp->nk", dy.flatten(2), _unfold3(a)).view(w.shape)
        da = _conv_t(dy, w).permute(0, 2, 3, 1).reshape(B, H * W, -1)
        return {"da": ("head", da, None), "dw": ("head_dw", dw, o["old_dw"]), "db": ("head", dy.sum(dim=(0, 2, 3)), o["old_db"])}
    if op == "resample":
        g = c(o["g"])
        if o["mode"] == 2:                                                # the four pixels in the kernel's order, * 0.25 * scale
            s = ((g[:, 0::2, 0::2] + g[:, 0::2, 1::2]) + g[:, 1::2, 0::2]) + g[:, 1::2, 1::2]
            return {"out": ("resample", s * 0.25 * o["scale"], o["old"])}
        return {"out": ("resample", g.repeat_interleave(2, 1).repeat_interleave(2, 2) * o["scale"], o["old"])}
    if op == "dropout0":
        B, C = o["scale"].shape
        x = c(o["x"]).view(B, -1, C)
        v = silu(x * c(o["scale"])[:, None] + c(o["shift"])[:, None]).view(B, -1)
        p32 = np.float32(o["p"])
        v = v / (1.0 - float(p32)) if dt == torch.float64 else v * float(np.float32(1) / (np.float32(1) - p32))
        return {"out": ("dropout", torch.where(o["keep"], v, torch.zeros_like(v)), None)}
    raise KeyError(op)


def _scale(op, o):
    """{name: S} fp64: the sum of the absolute values of the terms of each element, without the old value."""
    def c(t):
        return t.double()

    if op in ("linear", "linear_batch"):
        x = c(o["x"])
        a = (silu(x) if o["act_in"] else x).abs()
        S, dx = {}, 0
        for j, job in enumerate(o["jobs"]):
            dy = c(job["dy"]).abs()
            S[f"dw{j}"], S[f"db{j}"] = dy.t() @ a, dy.sum(0)
            dx = dx + dy @ c(job["w"]).abs()
        S["dx"] = dx * silu_grad(x).abs() if o["act_in"] else dx
        return S
    if op == "softmax":
        p, dp = c(o["p"]), c(o["dp"]).abs()
        return {"dp": p * dp + p * (p * dp).sum(-1, keepdim=True)}
    if op == "colsum":
        cs = c(o["colsum"]).abs()
        return {"dimg": cs.sum(1), "dbias": cs.sum(dim=(0, 1))}
    if op == "stem":
        x, w = c(o["x"]).abs(), c(o["w"]).abs()
        B, Cin, H, W = x.shape
        d = c(o["dy"]).abs().transpose(1, 2)
        return {"dw": torch.einsum("bnp,bkp->nk", d, _unfold3(x)).view(w.shape), "db": d.sum(dim=(0, 2)),
                "dx": _conv_t(d.reshape(B, -1, H, W), w)}
    if op == "head":
        w, dy = c(o["w"]).abs(), c(o["dy"]).abs()
        B, Cout, H, W = dy.shape
        a = silu(c(o["x"]) * c(o["scale"])[:, None] + c(o["shift"])[:, None]).abs().view(B, H, W, -1).permute(0, 3, 1, 2)
        return {"da": _conv_t(dy, w).permute(0, 2, 3, 1).reshape(B, H * W, -1),
                "dw": torch.einsum("bnp,bkp->nk", dy.flatten(2), _unfold3(a)).view(w.shape), "db": dy.sum(dim=(0, 2, 3))}
    if op == "resample":
        g = c(o["g"]).abs()
        if o["mode"] == 2:
            return {"out": (g[:, 0::2, 0::2] + g[:, 0::2, 1::2] + g[:, 1::2, 0::2] + g[:, 1::2, 1::2]) * 0.25 * o["scale"]}
        return {"out": g.repeat_interleave(2, 1).repeat_interleave(2, 2) * o["scale"]}
    if op == "dropout0":
        return {"out": _fresh(op, o, torch.float64)["out"][1].abs()}
    raise KeyError(op)


def outputs(op, o):
    """{name: Out} of a case."""
    ref, y32, S = _fresh(op, o, torch.float64), _fresh(op, o, torch.float32), _scale(op, o)
    return {k: Out(cls, r, S[k], old, y32[k][1]) for k, (cls, r, old) in ref.items()}


def target(out, acc):
    """(ref, S, restatement) of an output after a launch that adds to the old value (acc) or stores."""
    if acc:
        return out.ref0 + out.old.double(), out.S0 + out.old.double().abs(), out.y0 + out.old
    return out.ref0, out.S0, out.y0


def forms(out):
    """The forms a target is compared in by `prepared`: stored and / or added to."""
    return (False,) if out.old is None else (False, True)


# ---------------------------------------------------------------------------------------------------- the figure and the bars
def row_error(got, ref, S):
    """[rows] fp64: per output row (dimension 0 of ref) max |got - ref| / max S; inf where got is not finite."""
    R = ref.shape[0]
    e = (got.detach().double().cpu().reshape(ref.shape) - ref).abs().reshape(R, -1)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf"))).amax(1)
    return e / S.reshape(R, -1).amax(1).clamp_min(1e-300)


def border_error(got, ref, S, mask):
    """row_error over the elements of `mask` (broadcast to ref's shape) alone, against the same max S of the whole row."""
    R = ref.shape[0]
    e = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf")))
    e = torch.where(mask.expand(ref.shape), e, torch.zeros_like(e)).reshape(R, -1).amax(1)
    return e / S.reshape(R, -1).amax(1).clamp_min(1e-300)


def pixel_mask(op, shape):
    """{name: border mask broadcastable to the output} of the outputs that are maps of a padded convolution."""
    B, H, W = shape[:3]
    if op == "stem":
        return {"dx": border_mask(H, W)[None, None]}
    if op == "head":
        return {"da": border_mask(H, W).reshape(1, H * W, 1)}
    return {}


def global_error(got, ref):
    """The figure of tests/test_gpu_train_ops.py: max |got - ref| / max |ref| over the whole tensor."""
    return ((got.detach().double().cpu().reshape(ref.shape) - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def worst_row(e):
    i = e.argmax().item()
    return e[i].item(), i


def bar(cls, r32):
    return min(CAP[cls], max(FLOOR[cls], 4.0 * r32))


@functools.lru_cache(maxsize=None)
def prepared(op, shape, regime):
    """Everything a check of a case needs, computed once and shared, read-only, by the tests of a session:
    dict(o (operands), outs {name: Out}, r32 {class: worst row of the restatement over the outputs and forms}, bar {class})."""
    o = operands(op, shape, regime)
    outs = outputs(op, o)
    r32 = {}
    for out in outs.values():
        for acc in forms(out):
            ref, S, y = target(out, acc)
            r32[out.cls] = max(r32.get(out.cls, 0.0), row_error(y, ref, S).max().item())
    return dict(o=o, outs=outs, r32=r32, bar={cls: bar(cls, r) for cls, r in r32.items()})


# ---------------------------------------------------------------------------------------------------- dropout
def dropout_index(B, n):
    """uint64 [B * n]: idx = b * n + i."""
    return np.arange(B * n, dtype=np.uint64)


def dropout_keep(seed, B, n, p, idx=None):
    """bool [B, n]: the documented keep rule of anoddpm_dropout (include/anoddpm_hip.h, csrc/unet_kernels.hip dropout_keep)."""
    idx = dropout_index(B, n) if idx is None else idx
    with np.errstate(over="ignore"):
        z = np.full(1, seed, dtype=np.uint64) + idx * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    thresh = min(int(math.floor(float(np.float32(p)) * 4294967296.0)), 4294967295)
    return ((z >> np.uint64(32)) >= np.uint64(thresh)).reshape(B, n)


def dropout_values(x, keep, p):
    """fp32 [B, n]: mode 1 of anoddpm_dropout bit for bit: x * (1 / (1 - p)) in fp32 where kept, +0 elsewhere."""
    inv = np.float32(1) / (np.float32(1) - np.float32(p))
    return np.where(keep, x.astype(np.float32) * inv, np.float32(0)).astype(np.float32)


def dropout_input(B, n, seed):
    """fp32 [B, n] ~ N(0, 1), no zeros (a kept element is then never 0)."""
    x = np.random.default_rng(900 + seed % 1000).standard_normal((B, n)).astype(np.float32)
    x[x == 0] = 1.0
    return x


# ---------------------------------------------------------------------------------------------------- kernel geometry
def colsum_unrolled(ipb):
    """bool [ipb]: the items colsum_fold's 8 x 16 unrolled loop takes (lane il = i % 16 walks i = il, il + 16, ...; it takes eight
    items per round while i + 7 * 16 < ipb); the others are the tail loop's."""
    m = np.zeros(ipb, dtype=bool)
    for il in range(16):
        i = il
        while i + 7 * 16 < ipb:
            m[i:i + 8 * 16:16] = True
            i += 8 * 16
    return m
