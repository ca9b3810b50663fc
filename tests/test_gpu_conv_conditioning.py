"""-m gpu: the forward convolution kernels (anoddpm_igemm cfg 0-7, anoddpm_conv_head, anoddpm_conv_stem) on the operand regimes of
tests/conv_cases.py, one launch per item against fp64 of the fused layer.

Every item asserts that every (image, output channel) plane is within its bar: max_p |err| / max_p S <= max(FLOOR, 4 r32) <= CAP, S the
running-sum scale of the plane, r32 the worst plane of the fp32 CPU restatement of the item's arithmetic class (computed at run
time, tests/test_conv_reference.py holds 4 r32 <= CAP).  iid items also assert the figure of tests/test_gpu_ops.py at its bar there.
lattice items assert the exact result (conv_cases.lattice_mismatch), and exact sums and sums of squares in the statistics rows the
launch writes.  Every figure is printed before it is asserted; the module prints the worst figure per (kernel, regime) at its end.

cfg 7 on the lattice regime is held to the rounding bar (FLOOR, r32 being 0 there) and not to equality.  Its weights are exact (the
device packer evaluates G g G^T in fp64 as the host packer does), every operand and every transformed value has at most 16
significant bits, so the low bf16 piece of every split is 0 and none of the three dropped products exists; what is left is the
32-term sum inside v_mfma_f32_16x16x32_bf16, which is not a chain of fp32 additions.  Observed on the MI355X: 19 of 65 536 outputs of
(2, (32, 0), 128, 16) and 1 of 262 144 of (2, (64, 64), 128, 32) differ from the exact result, each by 2^-21 ... 2^-20 at outputs of magnitude
1 ... 4 (got 0.99999905 for 1.0): plane figure 6.1e-08 against the bar 6.8e-06; the statistics rows were still exact.  cfg 0-6 and
cfg 3 under every variant are bit-exact.

Measured on an MI355X: the table of DESIGN.md 5k (worst plane figure per kernel and regime, and its share of the bar).  The four
forms of cfg 3 (variants 0, 3, 6, 7) agree in every figure to the digits printed.  Wall time of the module on the device: 6.5 s for
the 308 items, the slowest 0.9 s (the first launch)."""
import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OLD_BAR = {0: cc.TOL, 1: cc.TOL, 5: cc.TOL, -1: cc.TOL, 4: 1e-5, 2: 1e-4, 3: 1e-4, 6: 1e-4, 7: 1e-4}     # tests/test_gpu_ops.py
LEDGER = {}
FAULT = []                  # the first launch that raised: nothing more is launched after it


@pytest.fixture(scope="module", autouse=True)
def ledger():
    yield
    for key in sorted(LEDGER):
        fig, ratio = LEDGER[key]
        print("worst", *key, f"{fig:.2e} ({ratio:.2f} of its bar)")


@pytest.fixture
def f43_variant(request):
    """The variant of the item (conv_cases.variants): see the fixture of the same name in tests/test_gpu_ops.py."""
    from anoddpm_amd._lib import lib
    v = request.node.callspec.params["item"][2]
    lib().anoddpm_internal_variant(5, v)
    yield v
    lib().anoddpm_internal_variant(5, 0)


def _launch(case, o, stats_out=None):
    """One launch -> [B, N, H, H] on the device."""
    assert not FAULT, f"not launched: an earlier launch raised ({FAULT[0]})"
    try:
        return _launch_once(case, o, stats_out)
    except BaseException as err:
        FAULT.append(repr(err))
        raise


def _launch_once(case, o, stats_out):
    import hipops
    x, w, b = o["x"].to(DEV), o["w"].to(DEV), o["bias"].to(DEV)
    if case.kind == "stem":
        return hipops.nchw(hipops.stem(x, w, b))
    gn = (o["scale"].to(DEV).contiguous(), o["shift"].to(DEV).contiguous()) if o["scale"] is not None else None
    xs = hipops.nhwc(x)
    if case.kind == "head":
        return hipops.head(xs, w, b, *gn)
    c0, c1 = case.cin
    srcs = [xs[..., :c0].contiguous()] + ([xs[..., c0:].contiguous()] if c1 else [])
    got = hipops.conv_igemm(srcs, w, b, Hout=case.H, ks=case.ks, gn=gn, act=o["act"], a_mode=case.a_mode,
                            temb=o["temb"].to(DEV) if o["temb"] is not None else None,
                            res=hipops.nhwc(o["res"].to(DEV)) if o["res"] is not None else None, res_up=case.res_up,
                            cfg=case.cfg, ksplit=case.ksplit, stats_out=stats_out)
    return hipops.nchw(got)


@pytest.mark.parametrize("item", cc.cases(), ids=cc.case_id)
def test_conv_regimes(item, f43_variant):
    case, regime, variant = item
    p = cc.prepared(case, regime)
    o, ref, cls = p["o"], p["ref"], cc.klass(case)
    tag = f"{case.kind} cfg {case.cfg} variant {variant} {cc.case_id(item)}"
    key = (case.kind if case.kind != "igemm" else f"cfg{case.cfg}" + (f"/v{variant}" if case.cfg == 3 else ""), regime)
    fails = []
    if regime == "lattice" and case.cfg != 7:
        st = [] if case.cfg != 4 else None                                      # the streaming 1x1 writes no statistics
        got = _launch(case, o, st).cpu()
        residue = cc.lattice_residue(case, o)
        diff = (got.double() - ref).abs().max().item()
        print(f"{tag}: max |got - exact| {diff:.3e} (allowed where exact == 0: {residue:.1e})")
        LEDGER[key] = max(LEDGER.get(key, (0.0, 0.0)), (diff, 0.0))
        bad = cc.lattice_mismatch(got, ref, residue)
        if bad:
            e = cc.plane_error(got, ref, p["S"])
            fig, b, n = cc.worst_plane(e)
            fails.append(f"{tag}: not the exact result: {bad}; worst plane (image {b}, channel {n}) {fig:.3e}")
        if st:
            s = st[0].double().cpu().sum(1)                                      # [B, N, 2]: rows are exact, so is their fp64 sum
            allow = residue * ref[0, 0].numel()
            for k, want in ((0, ref.sum(dim=(2, 3))), (1, (ref * ref).sum(dim=(2, 3)))):
                d = (s[..., k] - want).abs().max().item()
                print(f"{tag}: statistics rows {st[0].shape[1]}, max |{'sum sumsq'.split()[k]} - exact| {d:.3e}")
                if not d <= allow:
                    fails.append(f"{tag}: statistics rows: {'sum sumsq'.split()[k]} off by {d:.3e}")
    else:
        got = _launch(case, o).cpu()
        e = cc.plane_error(got, ref, p["S"])
        fig, b, n = cc.worst_plane(e)
        g = cc.global_error(got, ref)
        print(f"{tag}: worst plane (image {b}, channel {n}) {fig:.3e}, r32 {p['r32']:.3e}, bar {p['bar']:.3e} ({fig / p['bar']:.2f}); "
              f"global {g:.3e}")
        LEDGER[key] = max(LEDGER.get(key, (0.0, 0.0)), (fig, fig / p["bar"]), key=lambda t: t[1])
        if not (e <= p["bar"]).all():
            fails.append(f"{tag}: plane (image {b}, channel {n}) {fig:.3e} > bar {p['bar']:.3e} (r32 {p['r32']:.3e}); "
                         f"{int((e > p['bar']).sum())} of {e.numel()} planes beyond it")
        if regime == "iid" and not g < OLD_BAR[case.cfg]:
            fails.append(f"{tag}: global figure {g:.3e} >= {OLD_BAR[case.cfg]:.0e}")
    assert not fails, "\n".join(fails)
