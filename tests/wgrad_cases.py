"""Shared by the weight-gradient tests (tests/test_wgrad_reference.py on the CPU, tests/test_gpu_wgrad_plan.py on the device): the
seeded operand recipe, an fp64 statement of what anoddpm_conv3x3_wgrad / anoddpm_wgrad_pointwise compute, the per-block error
metric, and a restatement of how the Winograd-domain kernel (csrc/wgrad43.hip, algo 1) splits the output patches over its
workgroups.  No device needed here.

Operand recipe: every image of a batch has statistics of its own (activation (1 + 0.25 b) * randn + 0.1 b, dY scaled by
1 + 0.15 b, GroupNorm affines drawn per image), so that reading the wrong image anywhere changes a result by whole percent instead
of by sampling noise.

Error metric: per block of 64 output x 32 input channels (one workgroup set of wgrad43_kernel), max |err| / max |ref| within the
block; per-image sums against that image's own maximum.  A wrong block or a wrong image cannot hide behind a larger one."""
import torch
import torch.nn.functional as F

KB, NB = 32, 64                      # input / output channels of one workgroup set of wgrad43_kernel

# The walk cases of algo 1 (B, (c0, c1), N, H, W, a_mode) and what the grouping gives them, worked out by hand from
# PG = min(256 / ((K / 32) * (N / 64)), patches) and the walk pg, pg + PG, ... of workgroup pg (16 x 8-pixel output patches).
WALK_CASES = {
    "W1": (4, (128, 0), 128, 256, 256, 0),    # config-3 layer: 64 patches per workgroup over 4 images
    "W2": (3, (128, 0), 128, 48, 48, 0),      # ragged 1-2 patches; PG 32 > 18 patches per image: jumps 0 -> 2, leading zero rows
    "W3": (15, (32, 0), 64, 64, 64, 0),       # B at the affine-table limit; PG 256 strides over 8 images
    "W4": (2, (128, 0), 128, 128, 128, 1),    # nearest-x2 operand on an 8-patch walk
    "W5": (2, (48, 80), 64, 128, 128, 0),     # the block at k0 = 32 straddles the two sources (c0 % 32 = 16); 4 patches
    "W6": (4, (64, 0), 128, 40, 96, 0),       # non-square: 6 x 5 patches per image; ragged; skipped images
    "W7": (4, (512, 0), 512, 16, 16, 0),      # PG 2 = patches per image: every iteration changes image
}
WALK_CLAIMS = {
    #      PG, per image, patches, min / max per workgroup, change image, skip an image, start after image 0, change every step
    "W1": dict(PG=32, ppi=512, patches=2048, min=64, max=64, change=32, skip=0, late=0, every=0),
    "W2": dict(PG=32, ppi=18, patches=54, min=1, max=2, change=22, skip=14, late=14, every=22),
    "W3": dict(PG=256, ppi=32, patches=480, min=1, max=2, change=224, skip=224, late=224, every=224),
    "W4": dict(PG=32, ppi=128, patches=256, min=8, max=8, change=32, skip=0, late=0, every=0),
    "W5": dict(PG=64, ppi=128, patches=256, min=4, max=4, change=64, skip=0, late=0, every=0),
    "W6": dict(PG=64, ppi=30, patches=120, min=1, max=2, change=56, skip=56, late=34, every=56),
    "W7": dict(PG=2, ppi=2, patches=8, min=4, max=4, change=2, skip=0, late=0, every=2),
}


def source_size(H, W, a_mode):
    """Source map of a 3x3 layer with an H x W output: same size, half (nearest x2 on the load) or double (2x2 average)."""
    return {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[a_mode]


# ---------------------------------------------------------------------------------------------------- operand recipe
def image_rows(B, n, gen):
    """[B, n] fp32: image b is (1 + 0.25 b) * randn + 0.1 b."""
    s = torch.arange(B, dtype=torch.float32)[:, None]
    return torch.randn(B, n, generator=gen) * (1 + 0.25 * s) + 0.1 * s


def dy_rows(B, n, gen):
    """[B, n] fp32: image b is randn * (1 + 0.15 b)."""
    s = torch.arange(B, dtype=torch.float32)[:, None]
    return torch.randn(B, n, generator=gen) * (1 + 0.15 * s)


def affines(B, K, gen):
    """Per-image GroupNorm affines [B, K]: scale in [0.5, 1.5), shift randn -- drawn per image, so they differ between images."""
    return 0.5 + torch.rand(B, K, generator=gen), torch.randn(B, K, generator=gen)


def recipe(B, c0, c1, N, H, W, a_mode, seed):
    """NHWC sources [B, Hs, Ws, c], dY [B, H, W, N] and the affines [B, c0 + c1] of one 3x3 layer (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    Hs, Ws = source_size(H, W, a_mode)
    srcs = [image_rows(B, Hs * Ws * c, g).view(B, Hs, Ws, c) for c in (c0, c1) if c]
    dy = dy_rows(B, H * W * N, g).view(B, H, W, N)
    scale, shift = affines(B, c0 + c1, g)
    return srcs, dy, scale, shift


# ---------------------------------------------------------------------------------------------------- fp64 reference
def operand(srcs, a_mode=0, scale=None, shift=None, act=0):
    """fp64 NCHW operand the 3x3 kernels contract: virtual concat of the NHWC sources, per-image affine x * scale[b] + shift[b]
    (when given), SiLU (act), then nearest x2 (a_mode 1) or the 2x2 average (a_mode 2) of the activated map."""
    x = torch.cat([s.double() for s in srcs], dim=3).permute(0, 3, 1, 2)
    if scale is not None:
        x = x * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]
    if act:
        x = x * torch.sigmoid(x)
    if a_mode == 1:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    elif a_mode == 2:
        B, K, Hs, Ws = x.shape
        x = x.reshape(B, K, Hs // 2, 2, Ws // 2, 2).mean(dim=(3, 5))
    return x


def wgrad3(a, dy):
    """a: fp64 NCHW operand [B, K, H, W]; dy: NHWC [B, H, W, N].  Returns dW [N, K, 3, 3] = sum_b conv2d_weight(a_b, dY_b) (one
    image at a time) and the column sums dimg [B, N] = sum over the pixels of dY_b (their sum over b is the bias gradient)."""
    d = dy.double().permute(0, 3, 1, 2)
    N, K = d.shape[1], a.shape[1]
    dw = torch.zeros(N, K, 3, 3, dtype=torch.float64)
    for b in range(a.shape[0]):
        dw += torch.nn.grad.conv2d_weight(a[b:b + 1], (N, K, 3, 3), d[b:b + 1], padding=1)
    return dw, d.sum(dim=(2, 3))


def pointwise_operand(srcs, scale=None, shift=None, act=0):
    """fp64 [B, P, K] operand of the 1x1 kernel: concat of [B, P, c] sources, per-image affine, SiLU."""
    A = torch.cat([s.double() for s in srcs], dim=2)
    if scale is not None:
        A = A * scale.double()[:, None, :] + shift.double()[:, None, :]
    if act:
        A = A * torch.sigmoid(A)
    return A


def wgrad1(A, dy):
    """A: fp64 [B, P, K]; dy: [B, P, N].  dW [N, K] (the einsum of test_wgrad_pointwise) and dbias [N]."""
    d = dy.double()
    return torch.einsum("bpn,bpk->nk", d, A), d.sum(dim=(0, 1))


# ---------------------------------------------------------------------------------------------------- error metrics
def block_err(got, ref, base=None):
    """Worst block of 64 output x 32 input channels of max |got - (base + ref)| / max |ref|; got, ref, base: [N, K, ...].
    Returns (error, (n0, k0) of the worst block); inf when got holds a non-finite value."""
    got = got.detach().double().cpu()
    ref = ref.double()
    if not torch.isfinite(got).all():
        return float("inf"), None
    err = got - (ref if base is None else base.double().cpu() + ref)
    worst, where = 0.0, None
    N, K = ref.shape[0], ref.shape[1]
    for n0 in range(0, N, NB):
        for k0 in range(0, K, KB):
            r = ref[n0:n0 + NB, k0:k0 + KB].abs().max().item()
            e = err[n0:n0 + NB, k0:k0 + KB].abs().max().item() / max(r, 1e-300)
            if e > worst or where is None:
                worst, where = e, (n0, k0)
    return worst, where


def row_err(got, ref, base=None):
    """Worst row (image) of max |got - (base + ref)| / max |ref| within that row; got, ref: [B, N] or [N]."""
    got = got.detach().double().cpu().reshape(-1, ref.shape[-1])
    ref = ref.double().reshape(-1, ref.shape[-1])
    if not torch.isfinite(got).all():
        return float("inf")
    err = got - (ref if base is None else base.double().cpu().reshape(ref.shape) + ref)
    return max((err[b].abs().max() / ref[b].abs().max().clamp_min(1e-300)).item() for b in range(ref.shape[0]))


# ---------------------------------------------------------------------------------------------------- grouping of algo 1
def wgrad43_groups(K, N, B, H, W):
    """PG of the launcher (csrc/wgrad43.hip, wgrad43_groups): about one workgroup per CU over the (K / 32) x (N / 64) blocks,
    at most one per 16 x 8-pixel output patch."""
    blocks = (K // KB) * (N // NB)
    patches = B * (H // 8) * (W // 16)
    return min(max(256 // max(blocks, 1), 1), patches)


def walk(K, N, B, H, W):
    """What the workgroups of one block set walk: workgroup pg takes the patches pg, pg + PG, ... (image = patch // per image)."""
    PG = wgrad43_groups(K, N, B, H, W)
    ppi = (H // 8) * (W // 16)
    patches = B * ppi
    lists = [list(range(g, patches, PG)) for g in range(PG)]
    images = [[p // ppi for p in walk_] for walk_ in lists]
    sizes = [len(walk_) for walk_ in lists]
    steps = [list(zip(im, im[1:])) for im in images]
    return dict(PG=PG, ppi=ppi, patches=patches, lists=lists, images=images, min=min(sizes), max=max(sizes),
                change=sum(1 for im in images if im[0] != im[-1]),                          # reach another image
                skip=sum(1 for st in steps if any(b - a > 1 for a, b in st)),               # jump over an image (zero rows)
                late=sum(1 for im in images if im[0] > 0),                                  # leading zero rows
                every=sum(1 for st in steps if st and all(b != a for a, b in st)))          # a column-sum flush every patch
