"""Shared by the GroupNorm conditioning tests (tests/test_gn_reference.py on the CPU, tests/test_gpu_gn_conditioning.py on the
device): off-centre and near-constant operands, the fp64 reference, the per-image / per-group error metric, a CPU restatement of
the fused statistics scheme, the bars, and the structured inputs (blank slice, phantom) of the workload.  No device needed here.

Why: every fused GroupNorm route builds var = Q / n - mean^2 from per-channel {sum, sum of squares} partials that most producers
accumulate in fp32 before the fp64 fold.  An error d in Q becomes (1 + r^2) d in the variance, r = |mean| / sqrt(var + eps) of the
group; nn.GroupNorm's Welford / cascade moments degrade as r u only.  Centred operands (r < 1) cannot see that.

Operand recipe (`operand`, `conv_operand`): level r in LEVELS, regime "unit" (std 1) or "eps" (std 1e-3, the variance is of the
order of eps).  Group g of image b has |mean| = s (r (1.005 + 0.02 b) + 0.05 b + 0.01 (g % 4)), s = sqrt(std^2 + 1e-5), sign
(-1)^g: every group of every image has a mean of its own, never below the nominal level, and reading another image's row moves the
result by percent.  For a producer that is a convolution the mean sits in the bias (the per-image part in the per-image additive
row of the launch) and every output channel's weights have the norm `std`.

Error metric (`error`): per image and per group, max |err| over the maximum of that image's reference: a blank image cannot hide
behind a noisy one, nor a group behind another."""
import math

import torch
import torch.nn.functional as F

GROUPS, EPS = 32, 1e-5
LEVELS = (0, 4, 16, 64)
REGIMES = {"unit": 1.0, "eps": 1e-3}

# The project's own bars: TOL of test_gpu_ops.py up to r = 4; the whole-model bar of test_gpu_unet.py at r = 16 (the measured blank
# slice, 14.25, rounded up to the next level); the north-star bar at r = 64 (4x over the measured envelope) and for groups that are
# exactly constant at +-1.0 (r = 316).
BARS = {0: 2e-5, 4: 2e-5, 16: 5e-5, 64: 1e-3, "const": 1e-3}

# name -> (kind, level, regime)
CASES = {f"r{r}_{reg}": ("level", r, reg) for reg in REGIMES for r in LEVELS}
CASES.update({
    "zeros": ("zeros", 0, "unit"),                  # scale * 0 + shift == beta bit for bit
    "const1": ("const1", "const", "unit"),          # every group exactly 1.0
    "group_const": ("group_const", 0, "unit"),      # group 5 exactly 1.0, the others centred noise
    "blank_image": ("blank_image", 0, "unit"),      # image 0 exactly -1.0 (the MRI background); the others noise around -1 (r = 1)
})
CONST_GROUP = 5


def group_means(kind, level, regime, B, groups=GROUPS):
    """[B, groups] fp64: the mean the recipe gives group g of image b (level cases)."""
    std = REGIMES[regime]
    s = math.sqrt(std * std + EPS)
    b = torch.arange(B, dtype=torch.float64)[:, None]
    g = torch.arange(groups, dtype=torch.float64)[None, :]
    r = 0.0 if kind != "level" else float(level)
    mag = s * (r * (1.005 + 0.02 * b) + 0.05 * b + 0.01 * (g % 4))
    return mag * (1.0 - 2.0 * (g % 2))


def bars(name, B, groups=GROUPS):
    """[B, groups] fp64: the bar of every (image, group) of a case."""
    kind, level, _ = CASES[name]
    out = torch.full((B, groups), BARS[level], dtype=torch.float64)
    if kind == "group_const":
        out[:, CONST_GROUP] = BARS["const"]
    elif kind == "blank_image":
        out[0] = BARS["const"]
    return out


def operand(name, B, C, H, W, seed=0, mean_scale=1.0):
    """NCHW fp32 operand of a case.  Level cases: the noise of every (image, group) is standardised in fp64 (mean 0, biased std
    exactly `std`) before the group's mean is added, so that the achieved r is the nominal one up to the fp32 rounding of x.
    mean_scale: factor on the means (1.05 beside a `conv_operand` source of the same GroupNorm)."""
    kind, level, regime = CASES[name]
    gen = torch.Generator().manual_seed(1000 + seed)
    if kind == "zeros":
        return torch.zeros(B, C, H, W)
    if kind == "const1":
        return torch.ones(B, C, H, W)
    cpg = C // GROUPS
    z = torch.randn(B, GROUPS, cpg * H * W, generator=gen, dtype=torch.float64)
    z = (z - z.mean(-1, keepdim=True)) / z.var(-1, unbiased=False, keepdim=True).sqrt()
    if kind == "blank_image":
        x = z - 1.0
        x[0] = -1.0
    else:
        x = z * REGIMES[regime] + mean_scale * group_means(kind, level, regime, B)[:, :, None]
        if kind == "group_const":
            x[:, CONST_GROUP] = 1.0
    return x.reshape(B, C, H, W).float()


def conv_operand(name, B, Cin, N, H, ks, seed=0, ctot=None):
    """(x [B, Cin, H, H], w [N, Cin, ks, ks], bias [N], temb [B, N]) fp32 such that conv2d(x, w, bias) + temb[:, :, None, None] is
    an operand of the case: x is standard normal, ||w_n|| = std (so the output's interior std is `std`; zero padding only lowers
    it at the border, which raises r), the nominal mean times 1.05 (sampling error of the achieved std) in the bias and the
    per-image part of the mean in temb.  Degenerate cases: zero weights (the output is the bias, exactly, in every contraction:
    a Winograd transform of zero weights is zero), a zero image for the blank one.  ctot: the output is the FIRST N channels of
    a GroupNorm over ctot channels (virtual concat): the means follow that GroupNorm's groups."""
    kind, level, regime = CASES[name]
    gen = torch.Generator().manual_seed(2000 + seed)
    x = torch.randn(B, Cin, H, H, generator=gen)
    w = torch.randn(N, Cin, ks, ks, generator=gen, dtype=torch.float64)
    w = w / w.flatten(1).norm(dim=1)[:, None, None, None]
    cpg = (ctot or N) // GROUPS
    temb = torch.zeros(B, N)
    if kind == "zeros":
        return x, torch.zeros(N, Cin, ks, ks), torch.zeros(N), temb
    if kind == "const1":
        return x, torch.zeros(N, Cin, ks, ks), torch.ones(N), temb
    if kind == "blank_image":
        x[0] = 0.0
        return x, w.float(), torch.full((N,), -1.0), temb
    m = (1.05 * group_means(kind, level, regime, B)).repeat_interleave(cpg, dim=1)[:, :N]      # [B, N]
    bias = m[0].float()
    temb = (m - bias.double()[None]).float()
    w = (w * REGIMES[regime]).float()
    if kind == "group_const":
        w[CONST_GROUP * cpg:(CONST_GROUP + 1) * cpg] = 0.0           # (empty where the group lies beyond the first N channels)
        bias[CONST_GROUP * cpg:(CONST_GROUP + 1) * cpg] = 1.0
        temb[:, CONST_GROUP * cpg:(CONST_GROUP + 1) * cpg] = 0.0
    return x, w, bias, temb


def stem_operand(name, B, N, H, seed=0):
    """(x [B, 1, H, H], w [N, 1, 3, 3], bias [N]) for the stem, which has no per-image additive row: the images differ through the
    scale of the input instead (image b is randn (1 - 0.1 b): a smaller std, a larger r)."""
    x, w, bias, _ = conv_operand(name, B, 1, N, H, 3, seed)
    if CASES[name][0] != "blank_image":
        x = x * (1.0 - 0.1 * torch.arange(B, dtype=torch.float32))[:, None, None, None]
    return x, w, bias


def affine(C, seed=0):
    """gamma, beta [C] fp32 of the GroupNorm under test."""
    gen = torch.Generator().manual_seed(3000 + seed)
    return 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)


def moments(x, groups=GROUPS):
    """fp64 (mean, biased var) [B, groups] of an NCHW tensor."""
    g = x.detach().double().cpu().reshape(x.shape[0], groups, -1)
    return g.mean(-1), g.var(-1, unbiased=False)


def achieved_r(x, groups=GROUPS, eps=EPS):
    """[B, groups] fp64: |mean| / sqrt(var + eps) of the tensor handed in."""
    mean, var = moments(x, groups)
    return mean.abs() / (var + eps).sqrt()


# ---------------------------------------------------------------------------------------------------- reference and metric
def reference(x, gamma, beta, groups=GROUPS, eps=EPS):
    """fp64 F.group_norm of the NCHW tensor handed in.  For a fused route that tensor is the output the kernel itself wrote, so
    that the contraction's own error stays out of the statistic's figure."""
    return F.group_norm(x.detach().double().cpu(), groups, gamma.detach().double().cpu(), beta.detach().double().cpu(), eps=eps)


def normalised(x, mean, rstd, gamma, beta, groups=GROUPS):
    """fp64 (x - mean) rstd gamma + beta from given statistics [B, groups]: what a route's emitted mean / rstd stand for."""
    B, C = x.shape[:2]
    xd = x.detach().double().cpu().reshape(B, groups, -1)
    y = (xd - mean.detach().double().cpu()[:, :, None]) * rstd.detach().double().cpu()[:, :, None]
    return y.reshape(x.shape) * gamma.detach().double().cpu()[None, :, None, None] + beta.detach().double().cpu()[None, :, None, None]


def error(got, ref, groups=GROUPS):
    """[B, groups] fp64: per image and per group max |got - ref| over the maximum |ref| of that image; inf where got is not
    finite.  got, ref: [B, C, ...]."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    B = ref.shape[0]
    e = (got - ref).abs().reshape(B, groups, -1)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf"))).amax(-1)
    return e / ref.reshape(B, -1).abs().amax(-1).clamp_min(1e-300)[:, None]


COLUMNS = ("r<=4", "r16", "r64", "const")


def failures(tag, name, got, ref, out, ledger=None, bar=None):
    """Prints the worst figure of a check beside its bar and appends to `out` a line if an (image, group) is beyond it.
    ledger: {(tag, column): worst figure} with the columns r<=4 (bar 2e-5), r16 (5e-5), r64 (1e-3), const (1e-3).
    bar: [rows, groups] instead of the case's per-image bars (quantities summed over the images).
    Returns the worst figure and the worst figure-to-bar ratio."""
    e = error(got, ref)
    bar = bars(name, e.shape[0]) if bar is None else bar
    ratio = e / bar
    if ledger is not None:
        level = CASES[name][1]
        for col, mask in (("r<=4", bar == BARS[0]), ("r16", bar == BARS[16]), ("r64", (bar == BARS[64]) & (level == 64)),
                          ("const", (bar == BARS["const"]) & (level != 64))):
            if mask.any():
                ledger[(tag, col)] = max(ledger.get((tag, col), 0.0), e[mask].max().item())
    worst = ratio.argmax().item()
    b, g = divmod(worst, e.shape[1])
    print(f"{tag:64s} {name:12s} err {e.max().item():.2e}  worst/bar {ratio.max().item():.3f} (image {b}, group {g}, bar {bar[b, g].item():.0e})")
    if not (ratio < 1.0).all():
        out.append(f"{tag} {name}: {e[b, g].item():.3e} >= {bar[b, g].item():.0e} (image {b}, group {g})")
    return e.max().item(), ratio.max().item()


# ---------------------------------------------------------------------------------------------------- the fused scheme on the CPU
def _row_sum(v, order):
    """fp32 sum over the last axis in one of the two extreme orders: 'sequential' (one running sum) or 'pairwise' (a tree)."""
    if order == "sequential":
        acc = torch.zeros_like(v[..., 0])
        for i in range(v.shape[-1]):
            acc = acc + v[..., i]
        return acc
    assert order == "pairwise"
    while v.shape[-1] > 1:
        if v.shape[-1] % 2:
            v = torch.cat([v, torch.zeros_like(v[..., :1])], dim=-1)
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def fused_statement(x, gamma, beta, row_pixels=256, order="pairwise", groups=GROUPS, eps=EPS):
    """The fused routes' scheme restated: per channel fp32 {sum, sum of squares} over rows of `row_pixels` consecutive pixels
    (the last row may be shorter), an fp64 fold of rows and channels, mean = S / n, var = max(Q / n - mean^2, 0),
    rstd = (var + eps)^-1/2 in fp64, scale / shift rounded to fp32, y = x scale + shift in fp32.
    x: NCHW fp32.  Returns (y fp32, mean, rstd [B, groups] fp64)."""
    B, C = x.shape[:2]
    v = x.float().reshape(B, C, -1)
    P = v.shape[-1]
    S = torch.zeros(B, C, dtype=torch.float64)
    Q = torch.zeros(B, C, dtype=torch.float64)
    full = (P // row_pixels) * row_pixels
    parts = ([v[..., :full].reshape(B, C, -1, row_pixels)] if full else []) + ([v[..., full:].unsqueeze(2)] if full < P else [])
    for rows in parts:
        S += _row_sum(rows, order).double().sum(-1)
        Q += _row_sum(rows * rows, order).double().sum(-1)
    cpg = C // groups
    n = float(P * cpg)
    mean = S.reshape(B, groups, cpg).sum(-1) / n
    var = (Q.reshape(B, groups, cpg).sum(-1) / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / (var + eps).sqrt()
    sc = rstd.repeat_interleave(cpg, 1) * gamma.double()[None]
    sh = beta.double()[None] - mean.repeat_interleave(cpg, 1) * sc
    y = x.float() * sc.float()[:, :, None, None] + sh.float()[:, :, None, None]
    return y, mean, rstd


# ---------------------------------------------------------------------------------------------------- structured inputs
def phantom(img, seed=0):
    """[1, 1, img, img] fp32 in [-1, 1]: Gaussian blobs ("a head": one wide blob, a few narrow ones inside it) on the constant
    -1 background of a normalised MRI slice; about half of the pixels stay at the background value."""
    rs = torch.Generator().manual_seed(4000 + seed)
    yy, xx = torch.meshgrid(torch.arange(img, dtype=torch.float64), torch.arange(img, dtype=torch.float64), indexing="ij")
    c = (img - 1) / 2
    v = 1.2 * torch.exp(-(((yy - c) / (0.30 * img)) ** 2 + ((xx - c) / (0.24 * img)) ** 2) ** 2)
    for _ in range(5):
        cy, cx, s, a = (torch.rand(4, generator=rs, dtype=torch.float64) * torch.tensor([0.4, 0.4, 0.06, 0.8])
                        + torch.tensor([0.3, 0.3, 0.03, 0.2])).tolist()
        v = v + a * torch.exp(-((yy - cy * img) ** 2 + (xx - cx * img) ** 2) / (2 * (s * img) ** 2))
    x = (2 * v - 1).clamp(-1, 1)
    x[v < 0.02] = -1.0
    return x.float()[None, None]


def noised(x0, t, seed=0, T=1000):
    """sample_q of the linear schedule (betas 1e-4 ... 2e-2 over T steps) with seeded Gaussian noise, in fp64, rounded to fp32."""
    betas = torch.linspace(1e-4 * 1000 / T, 2e-2 * 1000 / T, T, dtype=torch.float64)
    acp = torch.cumprod(1 - betas, 0)[t]
    gen = torch.Generator().manual_seed(5000 + seed)
    return (acp.sqrt() * x0.double() + (1 - acp).sqrt() * torch.randn(x0.shape, generator=gen, dtype=torch.float64)).float()


STRUCTURED_T = (0, 100, 250, 999)


def structured_batch(img):
    """The batch of the structured-input fixture: [blank -1, phantom, phantom noised as at t = 250, uniform in [-1, 1]] with
    t = STRUCTURED_T."""
    gen = torch.Generator().manual_seed(6000)
    ph = phantom(img)
    x = torch.cat([torch.full((1, 1, img, img), -1.0), ph, noised(ph, 250), torch.rand(1, 1, img, img, generator=gen) * 2 - 1])
    return x, torch.tensor(STRUCTURED_T)
