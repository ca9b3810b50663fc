"""CPU checks of tests/wgrad_cases.py: the fp64 weight-gradient reference equals fp64 autograd of the same expression, the error
metric sees one bad block, the operand recipe makes an image mix-up visible, and the walk cases of tests/test_gpu_wgrad_plan.py
reach what they are there for according to the restatement of the launcher's grouping."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as wc

SHAPES = [(2, 32, 16, 8, 12), (3, 24, 8, 6, 10)]           # B, K, N, H, W (output map)


def _autograd3(srcs, dy, scale, shift, a_mode, act):
    """w.grad, bias.grad and the gradient of a per-image bias (the embedding term) of
    conv2d([resample](silu(cat(x) * scale + shift)), w) + b + emb[b], by fp64 autograd."""
    x = torch.cat([s.double() for s in srcs], dim=3).permute(0, 3, 1, 2)
    if scale is not None:
        x = x * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]
    if act:
        x = F.silu(x)
    if a_mode == 1:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    elif a_mode == 2:
        x = F.avg_pool2d(x, 2)
    B, N = dy.shape[0], dy.shape[3]
    K = x.shape[1]
    w = torch.randn(N, K, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.randn(N, dtype=torch.float64, requires_grad=True)
    emb = torch.randn(B, N, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, padding=1) + emb[:, :, None, None]
    y.backward(dy.double().permute(0, 3, 1, 2))
    return w.grad, b.grad, emb.grad


def _rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("a_mode", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_wgrad3_reference_is_autograd(shape, a_mode, concat):
    B, K, N, H, W = shape
    c0 = K // 3 if concat else K
    srcs, dy, scale, shift = wc.recipe(B, c0, K - c0, N, H, W, a_mode, seed=7)
    dw, dimg = wc.wgrad3(wc.operand(srcs, a_mode, scale, shift, act=1), dy)
    gw, gb, gemb = _autograd3(srcs, dy, scale, shift, a_mode, act=1)
    assert _rel(dw, gw) < 1e-12
    assert _rel(dimg, gemb) < 1e-12 and _rel(dimg.sum(dim=0), gb) < 1e-12


@pytest.mark.parametrize("a_mode", [0, 2])
def test_wgrad3_reference_plain_operand(a_mode):
    """No GroupNorm, no SiLU: the plain operand of the direct kernel (dropout output, Downsample / Upsample inputs)."""
    B, K, N, H, W = SHAPES[0]
    srcs, dy, _, _ = wc.recipe(B, K, 0, N, H, W, a_mode, seed=8)
    dw, dimg = wc.wgrad3(wc.operand(srcs, a_mode), dy)
    gw, gb, gemb = _autograd3(srcs, dy, None, None, a_mode, act=0)
    assert _rel(dw, gw) < 1e-12 and _rel(dimg, gemb) < 1e-12


@pytest.mark.parametrize("gn,act", [(True, 1), (True, 0), (False, 0)])
def test_wgrad1_reference_is_autograd(gn, act):
    B, P, c0, c1, N = 3, 40, 24, 8, 16
    g = torch.Generator().manual_seed(9)
    srcs = [wc.image_rows(B, P * c, g).view(B, P, c) for c in (c0, c1)]
    dy = wc.dy_rows(B, P * N, g).view(B, P, N)
    scale, shift = wc.affines(B, c0 + c1, g) if gn else (None, None)
    dw, db = wc.wgrad1(wc.pointwise_operand(srcs, scale, shift, act), dy)
    x = torch.cat([s.double() for s in srcs], dim=2)
    if gn:
        x = x * scale.double()[:, None, :] + shift.double()[:, None, :]
    if act:
        x = F.silu(x)
    w = torch.randn(N, c0 + c1, 1, 1, dtype=torch.float64, requires_grad=True)
    b = torch.randn(N, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.permute(0, 2, 1).reshape(B, c0 + c1, 5, 8), w, b)
    y.backward(dy.double().permute(0, 2, 1).reshape(B, N, 5, 8))
    assert _rel(dw, w.grad[:, :, 0, 0]) < 1e-12 and _rel(db, b.grad) < 1e-12


def test_block_err_sees_one_bad_block():
    """A block with a small gradient, wrong by 2e-4 of its own magnitude, fails a 1e-4 bar that the whole-tensor ratio (7e-7)
    would pass."""
    g = torch.Generator().manual_seed(10)
    ref = torch.randn(128, 96, 3, 3, generator=g, dtype=torch.float64)
    ref[64:128, 32:64] *= 1e-3
    base = torch.randn(128, 96, 3, 3, generator=g, dtype=torch.float64)
    got = base + ref
    assert wc.block_err(got, ref, base)[0] < 1e-12
    got[70, 40, 1, 1] += 2e-4 * ref[64:128, 32:64].abs().max()
    err, where = wc.block_err(got, ref, base)
    assert err > 1.9e-4 and where == (64, 32)
    assert ((got - base - ref).abs().max() / ref.abs().max()).item() < 1e-6
    got[0, 0, 0, 0] = float("nan")
    assert wc.block_err(got, ref, base)[0] == float("inf")


def test_recipe_makes_an_image_mixup_visible():
    """Reading image 1's affine row for image 0 changes the weight gradient by whole percent in every block."""
    B, c0, N, H, W = 2, 64, 128, 16, 16
    srcs, dy, scale, shift = wc.recipe(B, c0, 0, N, H, W, 0, seed=11)
    dw, dimg = wc.wgrad3(wc.operand(srcs, 0, scale, shift, act=1), dy)
    sc2, sh2 = scale.clone(), shift.clone()
    sc2[0], sh2[0] = scale[1], shift[1]
    dw2, _ = wc.wgrad3(wc.operand(srcs, 0, sc2, sh2, act=1), dy)
    for n0 in range(0, N, wc.NB):
        for k0 in range(0, c0, wc.KB):
            assert wc.block_err(dw2[n0:n0 + wc.NB, k0:k0 + wc.KB], dw[n0:n0 + wc.NB, k0:k0 + wc.KB])[0] > 1e-2
    # the per-image column sums of dY: image 1's against image 0's
    assert wc.row_err(dimg[[1, 1]], dimg) > 1e-2


@pytest.mark.parametrize("name", list(wc.WALK_CASES))
def test_walk_case_reaches_what_it_claims(name):
    B, (c0, c1), N, H, W, a_mode = wc.WALK_CASES[name]
    K = c0 + c1
    w = wc.walk(K, N, B, H, W)
    got = {k: w[k] for k in wc.WALK_CLAIMS[name]}
    assert got == wc.WALK_CLAIMS[name]
    assert w["max"] >= 2                                                   # the loop body runs more than once
    assert sorted(p for walk_ in w["lists"] for p in walk_) == list(range(w["patches"]))
    # shapes the Winograd-domain launcher accepts (csrc/wgrad43.hip, launch_wgrad43)
    assert H % 8 == 0 and W % 16 == 0 and K % 32 == 0 and N % 64 == 0 and (c1 == 0 or c0 % 16 == 0) and B <= 15
    assert a_mode in (0, 1)


def _walk_of(name):
    B, (c0, c1), N, H, W, _ = wc.WALK_CASES[name]
    return wc.walk(c0 + c1, N, B, H, W)


def test_walk_case_details():
    """What each case is for (tests/wgrad_cases.py: WALK_CASES) beyond the counts above."""
    assert sum(1 for im in _walk_of("W2")["images"] if im[0] == 0 and im[-1] == 2) == 14      # W2: jump from image 0 to 2
    w3 = _walk_of("W3")
    assert sum(1 for walk_ in w3["lists"] if len(walk_) == 2) == 224 and w3["PG"] == 8 * w3["ppi"]   # strides over 8 images
    _, (c0, c1), _, _, _, _ = wc.WALK_CASES["W5"]
    assert c0 % wc.KB == 16 and c1 > 0          # W5: the block at k0 = 32 reads channels 32..47 from a0 and 48..63 from a1
    _, _, _, H, W, _ = wc.WALK_CASES["W6"]
    assert (H // 8, W // 16) == (5, 6) and H != W                                              # tiles_y 5, tiles_x 6
    assert _walk_of("W7")["images"] == [[0, 1, 2, 3], [0, 1, 2, 3]]                          # a new image every patch
