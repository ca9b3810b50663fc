"""-m gpu: the small-map kernels at the shapes where moving a memory request can go wrong.

smallmap_kernel, wino23s_kernel and pointwise_stream_kernel read a virtual concat of two sources; here each source is a channel
slice of a WIDER buffer (random values around it), so that a0_ld != a1_ld != the channel counts and a request addressed with the
wrong source's pitch reads something else.  Every case runs twice -- contiguous sources through tests/hipops.py, then the same
prepared launch on the pitched slices -- and both results are compared with an fp64 CPU statement of the fused expression at the
tolerance tests/test_gpu_ops.py uses for the same kernel (2e-5 smallmap, 1e-4 F(2x2,3x3), 1e-5 streaming 1x1); the two results
must also be equal bit for bit (same sums in the same order).  gn_finalize2_kernel gets statistics rows built on the host from
off-centre operands (tests/gn_cases.py, r = 16) at every row count and channels-per-group its row loop distinguishes, against fp64
F.group_norm at gn_cases' bars."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import gn_cases as gc
from test_gpu_ops import TOL, dev, relerr, rnd

pytestmark = pytest.mark.gpu


def pitched(src, before, after, seed):
    """A [B, H, W, c] view with pixel pitch before + c + after inside a buffer of unrelated values."""
    B, H, W, c = src.shape
    wide = (rnd(B, H, W, before + c + after, seed=seed) * 3 + 1).to(src.device)
    wide[..., before:before + c] = src
    return wide[..., before:before + c]


def relaunch_pitched(srcs, out_like, pads):
    """Launches hipops' last prepared anoddpm_igemm call again, on pitched views of its sources and into a fresh output."""
    import hipops
    from anoddpm_amd._lib import check, current_stream, lib
    st = hipops.LAST_IGEMM
    views = [pitched(s, *pads[i], seed=900 + i) for i, s in enumerate(srcs)]
    for i, v in enumerate(views):
        assert v.stride(3) == 1 and v.stride(2) % 4 == 0 and v.data_ptr() % 16 == 0
        setattr(st, f"a{i}", v.data_ptr())
        setattr(st, f"a{i}_ld", v.stride(2))
        setattr(st, f"a{i}_bs", v.stride(0))
    assert len(views) == 1 or views[0].stride(2) != views[1].stride(2)
    out = torch.full_like(out_like, float("nan"))
    st.out = out.data_ptr()
    check(lib().anoddpm_igemm(ctypes.byref(st), current_stream()), "igemm")
    torch.cuda.synchronize()
    return out


def fused_reference(x, w, b, gamma, beta, gn, act, a_mode=0, temb=None, res=None):
    h = x.double()
    if gn:
        h = F.group_norm(h, 32, gamma.double(), beta.double(), eps=1e-5)
    if act:
        h = F.silu(h)
    if a_mode == 1:
        h = F.interpolate(h, scale_factor=2, mode="nearest")
    ref = F.conv2d(h, w.double(), b.double() if b is not None else None, padding=w.shape[2] // 2)
    if temb is not None:
        ref = ref + temb.double()[:, :, None, None]
    if res is not None:
        ref = ref + res.double()
    return ref.float()


def run_both(srcs, w, b, pads, **kw):
    import hipops
    got = hipops.conv_igemm(srcs, w.to(dev()), b.to(dev()) if b is not None else None, **kw)
    got_p = relaunch_pitched(srcs, got, pads)
    return got, got_p


SMALLMAP = [
    # B, (c0, c1), N, H, ks, gn, act, rows per image of the fold's statistics
    (2, (128, 384), 32, 8, 3, "given", 1, None),       # two 256-channel chunks, the split inside the first
    (2, (128, 384), 32, 8, 3, "fold", 1, (4, 4)),      # statistics rows as an 8x8 producer writes them
    (1, (256, 768), 32, 16, 1, "no", 0, None),         # 1x1: two 512-channel chunks, the first one straddles
    (1, (256, 768), 32, 16, 1, "fold", 0, (16, 8)),
    # 12 channels per group: group 21 lies in both sources; row counts that are no multiples of four; Kpad = 512 > K (zero fill)
    (2, (256, 128), 32, 8, 3, "fold", 1, (3, 5)),
    # the second source hands over one fp64 row (fmt 1), as a split-K tail's tail_csum; group 10 straddles
    (2, (128, 256), 32, 8, 3, "fold", 1, (3, "fp64")),
]


def fold_stats(src, rows):
    """(statistics tensor, fmt) of one NHWC source: `rows` fp32 rows from chan_stats, or the fp64 sums [B][c][2] of a split-K tail."""
    import hipops
    if rows != "fp64":
        return hipops.chan_stats(src, nslab=rows), 0
    of = src.double().reshape(src.shape[0], -1, src.shape[-1])
    return torch.stack([of.sum(1), (of * of).sum(1)], dim=-1).contiguous(), 1


@pytest.mark.parametrize("case", SMALLMAP, ids=[f"{c[4]}x{c[4]}_{c[3]}x{c[3]}_{c[1][0]}+{c[1][1]}_{c[5]}" for c in SMALLMAP])
def test_smallmap_pitched_concat(case):
    import hipops
    from anoddpm_amd._lib import lib
    B, (c0, c1), N, H, ks, gn_mode, act, rows = case
    C = c0 + c1
    assert lib().anoddpm_smallmap_tile(ks, H, H, C, c0, N, B) != 0
    x = rnd(B, C, H, H, seed=321) * 1.5 + 0.3
    w = rnd(N, C, ks, ks, seed=322, scale=1.0 / math.sqrt(C * ks * ks))
    b = rnd(N, seed=323, scale=0.1)
    gamma, beta = 1 + 0.1 * rnd(C, seed=324), 0.1 * rnd(C, seed=325)
    temb, res = rnd(B, N, seed=326), rnd(B, N, H, H, seed=327)
    ref = fused_reference(x, w, b, gamma, beta, gn_mode != "no", act, temb=temb, res=res)
    xs = hipops.nhwc(x.to(dev()))
    srcs = [xs[..., :c0].contiguous(), xs[..., c0:].contiguous()]
    gn = fold = None
    if gn_mode == "given":
        gn = hipops.gn_affine(srcs, gamma.to(dev()), beta.to(dev()))
    elif gn_mode == "fold":
        fold = dict(stats=[fold_stats(s_, r_) for s_, r_ in zip(srcs, rows)], gamma=gamma.to(dev()), beta=beta.to(dev()))
    got, got_p = run_both(srcs, w, b, [(8, 4), (4, 24)], Hout=H, ks=ks, gn=gn, act=act, fold=fold, temb=temb.to(dev()),
                          res=hipops.nhwc(res.to(dev())), cfg=5, stats_out=[])
    e, ep = relerr(hipops.nchw(got), ref), relerr(hipops.nchw(got_p), ref)
    print(f"smallmap {case}: contiguous {e:.2e}  pitched {ep:.2e}  (bar {TOL:.0e})")
    assert e < TOL and ep < TOL
    assert torch.equal(got, got_p)


WINO23S = [(ct, a_mode, c0, c1, rows) for (c0, c1, rows) in ((96, 160, (4, 16)), (256, 128, (3, 5))) for ct in (2, 4) for a_mode in (0, 1)]
WINO23S.append((2, 1, 96, 160, (4, "fp64")))         # fmt 1 on the second source, normalised at the half resolution


def wino23s_id(c):
    ct, a_mode, c0, c1, rows = c
    return f"ct{ct}_amode{a_mode}" + ("" if (c0, c1) == (96, 160) and rows == (4, 16) else f"_{c0}+{c1}_rows{rows[0]}+{rows[1]}")


@pytest.mark.parametrize("ct,a_mode,c0,c1,rows", WINO23S, ids=[wino23s_id(c) for c in WINO23S])
def test_wino23s_pitched_concat_fold(ct, a_mode, c0, c1, rows):
    """16x16 map, batch 1, K = 96 + 160 or 256 + 128 (12 channels per group: group 21 lies in both sources); the output widths are
    the smallest at which the launcher's tile rule picks the 32- (ct 2) and the 64-channel (ct 4) workgroup for four 8x8 blocks.
    Fold from `rows` statistics rows per source (fp32 rows, or "fp64": the one fp64 row a split-K tail hands over)."""
    import hipops
    from anoddpm_amd._lib import lib
    B, H = 1, 16
    N = 1024 if ct == 2 else 3200
    C = c0 + c1
    assert lib().anoddpm_wino23s_tile(H, H, C, c0, N, B, a_mode) == ct
    Hin = H // 2 if a_mode == 1 else H
    x = rnd(B, C, Hin, Hin, seed=421) * 1.5 + 0.3
    w = rnd(N, C, 3, 3, seed=422, scale=1.0 / math.sqrt(C * 9))
    b = rnd(N, seed=423, scale=0.1)
    gamma, beta = 1 + 0.1 * rnd(C, seed=424), 0.1 * rnd(C, seed=425)
    temb, res = rnd(B, N, seed=426), rnd(B, N, H, H, seed=427)
    ref = fused_reference(x, w, b, gamma, beta, True, 1, a_mode=a_mode, temb=temb, res=res)
    xs = hipops.nhwc(x.to(dev()))
    srcs = [xs[..., :c0].contiguous(), xs[..., c0:].contiguous()]
    fold = dict(stats=[fold_stats(s_, r_) for s_, r_ in zip(srcs, rows)], gamma=gamma.to(dev()), beta=beta.to(dev()))
    got, got_p = run_both(srcs, w, b, [(4, 12), (16, 0)], Hout=H, ks=3, act=1, a_mode=a_mode, fold=fold, temb=temb.to(dev()),
                          res=hipops.nhwc(res.to(dev())), cfg=6, stats_out=[])
    e, ep = relerr(hipops.nchw(got), ref), relerr(hipops.nchw(got_p), ref)
    print(f"wino23s ct {ct} a_mode {a_mode} {c0}+{c1} rows {rows}: contiguous {e:.2e}  pitched {ep:.2e}  (bar 1e-4)")
    assert e < 1e-4 and ep < 1e-4
    assert torch.equal(got, got_p)


POINTWISE = [(B, H, K, N, full) for (B, H) in ((1, 8), (2, 16)) for K in (128, 512) for N in (64, 128) for full in (False, True)]


@pytest.mark.parametrize("case", POINTWISE, ids=[f"b{c[0]}_{c[1]}x{c[1]}_k{c[2]}_n{c[3]}_{'bias_res' if c[4] else 'plain'}" for c in POINTWISE])
def test_pointwise_stream_pitched_concat(case):
    """8x8, batch 1: two 32-pixel tiles, so most waves leave after the weight fill's barrier.  First source 32 channels."""
    import hipops
    B, H, K, N, full = case
    c0, c1 = 32, K - 32
    x = rnd(B, K, H, H, seed=521)
    w = rnd(N, K, 1, 1, seed=522, scale=1.0 / math.sqrt(K))
    b = rnd(N, seed=523, scale=0.1) if full else None
    res = rnd(B, N, H, H, seed=527) if full else None
    ref = fused_reference(x, w, b, None, None, False, 0, res=res)
    xs = hipops.nhwc(x.to(dev()))
    srcs = [xs[..., :c0].contiguous(), xs[..., c0:].contiguous()]
    got, got_p = run_both(srcs, w, b, [(4, 28), (8, 0)], Hout=H, ks=1, res=hipops.nhwc(res.to(dev())) if full else None, cfg=4)
    e, ep = relerr(hipops.nchw(got), ref), relerr(hipops.nchw(got_p), ref)
    print(f"pointwise {case}: contiguous {e:.2e}  pitched {ep:.2e}  (bar 1e-5)")
    assert e < 1e-5 and ep < 1e-5
    assert torch.equal(got, got_p)


# ---- gn_finalize2_kernel ----------------------------------------------------------------------------------------------------
GN_H = 18               # 324 pixels: every row count below has at least one pixel per row
GN_NAME = "r16_unit"    # |mean| = 16 std: var = Q / n - mean^2 loses 2.5 digits, the fold has to be the fp64 one


def host_rows(xs, rows):
    """Statistics rows [B][rows][c][2] fp32 of an NHWC cpu tensor: per channel {sum, sum of squares} over `rows` consecutive,
    nearly equal pixel ranges, summed in fp64 and rounded once."""
    B, H, W, c = xs.shape
    v = xs.double().reshape(B, H * W, c)
    edges = [(H * W * r) // rows for r in range(rows + 1)]
    out = torch.empty(B, rows, c, 2, dtype=torch.float64)
    for r in range(rows):
        seg = v[:, edges[r]:edges[r + 1]]
        out[:, r, :, 0] = seg.sum(1)
        out[:, r, :, 1] = (seg * seg).sum(1)
    return out.float()


_GN_X = {}


def gn_operand(C):
    if C not in _GN_X:
        _GN_X[C] = gc.operand(GN_NAME, 2, C, GN_H, GN_H)
    return _GN_X[C]


def check_finalize(tag, x, c0, rows, want_mean_rstd=False):
    import hipops
    C = x.shape[1]
    gamma, beta = gc.affine(C)
    xs = x.permute(0, 2, 3, 1).contiguous()
    parts = [xs[..., :c0]] + ([xs[..., c0:]] if c0 < C else [])
    st = [host_rows(p, r).to(dev()) for p, r in zip(parts, rows)]
    got = hipops.gn_finalize(st, gamma.to(dev()), beta.to(dev()), GN_H * GN_H, want_mean_rstd=want_mean_rstd)
    sc, sh = got[0].cpu(), got[1].cpu()
    ref = gc.reference(x, gamma, beta)
    fails = []
    gc.failures(tag, GN_NAME, x * sc[:, :, None, None] + sh[:, :, None, None], ref, fails)
    if want_mean_rstd:
        gc.failures(tag + " | mean, rstd", GN_NAME, gc.normalised(x, got[2].cpu(), got[3].cpu(), gamma, beta), ref, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rows", [1, 16, 64, 256, 260])
@pytest.mark.parametrize("C", [128, 256, 1024])
def test_gn_finalize_rows_by_channels_per_group(C, rows):
    """cpg / 2 = 2, 4, 16 float4 per row; 260 rows take the second trip of a thread's row loop."""
    check_finalize(f"gn_finalize C={C} rows={rows}", gn_operand(C), C, (rows,), want_mean_rstd=(C == 256 and rows == 260))


def test_gn_finalize_two_sources():
    check_finalize("gn_finalize 256+256 rows 16/260", gn_operand(512), 256, (16, 260))


def test_gn_finalize_group_straddles_the_sources():
    """256 + 128 channels: 12 per group, group 21 lies in both sources."""
    check_finalize("gn_finalize 256+128 rows 64/5", gn_operand(384), 256, (64, 5), want_mean_rstd=True)
