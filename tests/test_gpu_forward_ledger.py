"""-m gpu: every launch of small INFERENCE plans against fp64 (tests/forward_ledger.py), after a poison step.

The inference plan (anoddpm_amd/unet.py, _Plan) takes routes the training plan never does -- GroupNorms finished inside their consumer
from statistics rows or fp64 sums (_GnFold), the statistics formats of stats_of and the row-count arithmetic of igemm(), a GroupNorm
attached to the producer's split-K tail, the pool with its activated twin, the half-resolution residual of the F(4x4,3x3) epilogue,
ANODDPM_CSUM / ANODDPM_ARITH -- so tests/test_gpu_backward_ledger.py never reaches them, the operator tests choose the wiring
themselves, and the end-to-end tests see one max-norm figure.

Per plan: (1) one forward builds the plan; (2) every floating-point tensor the plan keeps -- the shared split-K workspace and the
ANODDPM_CSUM arena included -- is filled with NaN, except the buffers `_kept` names and prints: the packed weight buffers (written
by the packing launch when a parameter changes, not by a forward) and the frequency table (uploaded when the plan is built);
(3) the same forward again must be finite and BIT-IDENTICAL to the first (ANODDPM_CSUM=1: within 1e-6, the bound of
test_config2_with_atomic_groupnorm_sums_matches_reference -- fp64 atomics reorder adds): a NaN means a launch read memory nobody
wrote in this forward; (4) the static checks of the ledger, then every launch from the second forward's buffers, fp64 on the
device; audited == len(plan.ops), no exempt class; (5) every figure is printed before it is asserted (-s), the worst per class
too, and all failures are collected into one assert.  FAULT: nothing is launched after a launch has raised.

Plans: the smallest shapes that reach each route (`_coverage` asserts from the structs that they do); PLANS says which.  Three
candidates of the issue did not reach a route they were listed for and were replaced or complemented, as read from the structs:
  * i32_b2 has no cfg 6 launch (its 3x3 layers on 16x16 / 32x32 maps have K < 64 or fit cfg 5): the row fold into a cfg 6 consumer is
    asserted on i64_b128_b4, which has twelve cfg 6 launches;
  * i64_b128_b1 has no cfg 3 launch at all (a batch of one fills 32 workgroups on its 64x64 maps): the deep-K split of cfg 3 needs
    a 128-channel grid of <= 64 workgroups with K >= 256 -- the 128x128 up-path layers (256 -> 128) of i128_b128_b1, which replaces
    it and also has the direct kernels with split-K and the materialised nearest-x2 residual;
  * no candidate runs cfg 0, or cfg 2 without split-K (the statistics rows of those two epilogues): the plan chooses them on the
    128x128 maps when the F(4x4,3x3) kernels (ANODDPM_NO_F43=1: cfg 2, 256 workgroups at a batch of two) or all Winograd kernels
    (ANODDPM_NO_WINOGRAD=1: cfg 0, 512 tiles at a batch of four) are switched off -- the plan's own switches, as ANODDPM_CSUM is;
    cfg is never forced.

Bars: the constants of forward_ledger.py, each named after the op test it comes from; none had to be derived.  First measurement (one
MI355X), worst figure of each class over the nine plans and its share of the bar:
    cfg 0 3x3 2.2e-6, cfg 1 3x3 2.7e-6 / 1x1 1.1e-6, cfg 4 1.3e-6, cfg 5 3x3 1.4e-6 / 1x1 6.1e-7 (of 2e-5: <= 13 %); cfg 2 7.4e-7, cfg 3
    1.2e-5, cfg 6 9.0e-7, cfg 7 1.3e-5 (of 1e-4: <= 13 %); fused attention 1.5e-6, chain softmax 1.5e-6, chain P v 3.1e-7, GroupNorm
    affine 2.2e-7, linear 2.4e-7, stem 2.3e-7, head 3.9e-7 (of 2e-5: <= 8 %); statistics rows 1.8e-7, fp64 sums 5.1e-8 (of 1e-5);
    posemb 4.8e-8 absolute (of 2e-6); resample 1.1e-7 (of 1e-6), its activated twin 1.4e-7 (of 2e-5), layout 0.
The poison step found no read-before-write: every second forward is finite and bit-identical (ANODDPM_CSUM=1: identical as well);
no static check failed.
Wall time per plan, references contracted in fp64 on the device (yardstick: 7.6 s, the slowest backward-ledger plan): i32_b2 1.8 s
(first plan of the process), i32_b2_gemm_attn 0.5 s, i64_b128_b4 2.8 s, i128_b128_b1 2.8 s, i64_b128_b4_csum 2.6 s, i128_b128_b4_bf16
2.9 s, i32_convrs_c3 2.3 s, i128_b128_b2_nof43 2.9 s, i128_b128_b4_direct 2.9 s.
"""
import gc
import time

import pytest
import torch

import forward_ledger as fl

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
I32 = dict(img_size=32, base_channels=32, n_heads=2, attention_resolutions="16,8")
I64 = dict(img_size=64, base_channels=128, n_heads=2, attention_resolutions="16,8")
I128 = dict(img_size=128, base_channels=128, n_heads=2, attention_resolutions="16,8")
PLANS = {
    # name: (constructor arguments, batch, environment, routes the plan is listed for)
    "i32_b2": (I32, 2, {}, {"cfg 5", "fold: rows", "attention: fused", "statistics: stem rows", "OP_HEAD", "statistics: cfg 1 rows"}),
    "i32_b2_gemm_attn": (I32, 2, {"ANODDPM_NO_FUSED_ATTENTION": "1"}, {"attention: three launches"}),
    "i64_b128_b4": (I64, 4, {}, {"cfg 3", "cfg 3 split-K", "statistics: csum", "tail-attached GroupNorm", "cfg 2 split-K", "cfg 4", "res_mode 1",
                                 "pool_act double output", "statistics: split-K rows", "shared split-K workspace", "cfg 6",
                                 "statistics: cfg 6 rows", "statistics: cfg 3 rows", "two-source finalize, mixed formats"}),
    "i128_b128_b1": (I128, 1, {}, {"cfg 3 split-K", "cfg 1 split-K", "res_mode 0", "resample mode 1"}),
    "i64_b128_b4_csum": (I64, 4, {"ANODDPM_CSUM": "1"}, {"statistics: asum", "fold: fp64 sums", "arena cleared by posemb"}),
    "i128_b128_b4_bf16": (I128, 4, {"ANODDPM_ARITH": "bf16split3"}, {"cfg 7", "statistics: cfg 7 rows"}),
    "i32_convrs_c3": (dict(img_size=32, base_channels=128, in_channels=3, biggan_updown=False, conv_resample=True), 2, {},
                      {"resample mode 3", "OP_LAYOUT", "statistics: chan_stats rows", "igemm head", "plain a_mode 1"}),
    "i128_b128_b2_nof43": (I128, 2, {"ANODDPM_NO_F43": "1"}, {"cfg 2", "statistics: cfg 2 rows"}),
    "i128_b128_b4_direct": (I128, 4, {"ANODDPM_NO_WINOGRAD": "1"}, {"cfg 0", "statistics: cfg 0 rows"}),
}
# taken over all plans together
EVERYWHERE = ({f"cfg {c}" for c in range(8)} | {"fold: rows", "fold: fp64 sums", "tail-attached GroupNorm", "res_mode 0", "res_mode 1",
              "attention: fused", "attention: three launches", "OP_HEAD", "OP_LAYOUT", "batched embedding projection",
              "pool_act double output", "shared split-K workspace", "arena cleared by posemb",
              "statistics: stem rows", "statistics: chan_stats rows", "statistics: split-K rows", "statistics: csum", "statistics: asum"} |
              {f"statistics: cfg {c} rows" for c in (0, 1, 2, 3, 5, 6, 7)})
FAULT = []                   # the first forward that raised: nothing more is launched after it
SEEN = {}                    # plan name -> routes


def _forward(model, x, t):
    assert not FAULT, f"not launched: an earlier forward raised ({FAULT[0]})"
    try:
        with torch.no_grad():
            y = model(x, t)
        torch.cuda.synchronize()
        return y
    except BaseException as err:
        FAULT.append(repr(err))
        raise


def _kept(plan, view):
    """Buffers the poison step leaves alone: [(tensor, name, reason)].  Everything else the plan keeps is rewritten by every forward."""
    spans = []
    for a, b in sorted((p, p + 4 * n) for p, (_, _, n) in view.packs.items()):
        if spans and a <= spans[-1][1]:
            spans[-1][1] = max(spans[-1][1], b)
        else:
            spans.append([a, b])
    kept = []
    for i, tt in enumerate(view.keep):
        lo, hi = tt.data_ptr(), tt.data_ptr() + tt.numel() * tt.element_size()
        if tt.data_ptr() == plan.posemb.freqs:
            kept.append((tt, f"keep[{i}] posemb.freqs", "the sinusoid frequencies: computed on the host and uploaded when the plan is built"))
        elif any(a <= lo and hi <= b for a, b in spans):
            kept.append((tt, f"keep[{i}] packed weights", "written by the packing launch when a parameter changes, read-only in a forward"))
    return kept


def _coverage(name, plan, led):
    """What a plan must contain for this test to mean what it says, asserted from the structs."""
    from anoddpm_amd import _lib
    want = PLANS[name][3]
    routes = set(led.routes)
    fin = [st for c, st in plan.ops if c == _lib.OP_GN_FINALIZE]
    if any(st.c1 and st.fmt0 != st.fmt1 for st in fin):
        routes.add("two-source finalize, mixed formats")
    if any(c == _lib.OP_IGEMM and st.b_mode == 0 and st.ks == 3 and st.N <= 4 for c, st in plan.ops):
        routes.add("igemm head")
    if any(c == _lib.OP_IGEMM and st.a_mode == 1 and not st.gn_scale and not st.fold_gamma for c, st in plan.ops):
        routes.add("plain a_mode 1")
    assert want <= routes, f"plan {name} misses {sorted(want - routes)}; it has {sorted(routes)}"
    ig = [st for c, st in plan.ops if c == _lib.OP_IGEMM]
    if name == "i128_b128_b1":
        assert any(st.cfg == 3 and st.ksplit > 1 and st.H == 128 for st in ig), "no deep-K split of cfg 3 on the 128x128 maps"
    if name == "i64_b128_b4":
        assert any(st.cfg == 6 and st.fold_gamma and not st.fold_fmt0 for st in ig), "no GroupNorm folded from rows into a cfg 6 consumer"
        assert any(st.cfg == 3 and st.ksplit == 1 and st.H == 64 for st in ig), "no cfg 3 launch on the 64x64 maps"
        assert any(st.cfg == 3 and st.ksplit > 1 and st.H == 32 and st.c0 + st.c1 >= 512 for st in ig), "no deep 32x32 cfg 3 split-K layer"
        assert any(st.cfg == 2 and st.ksplit > 1 and st.H == 16 and st.c0 + st.c1 > 256 for st in ig), "no cfg 2 split-K on 16x16 with K > 256"
    SEEN[name] = routes
    return routes


def _model(name, monkeypatch, dev):
    from UNet import UNetModel
    from oracle import unet_oracle as uo
    kw, B, env, _ = PLANS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    S, Cin = kw["img_size"], kw.get("in_channels", 1)
    torch.manual_seed(0)
    model = UNetModel(**kw)
    model.load_state_dict(uo.perturb(uo.fill_deterministic({k: tuple(v.shape) for k, v in model.state_dict().items()})))
    model.to(dev).eval()
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(B, Cin, S, S, generator=g) * 2 - 1).to(dev)
    t = ((torch.arange(B) * 61 + 17) % 1000).to(dev)         # a distinct timestep per image
    assert len(set(t.tolist())) == B
    return model, x, t


def _routes_from_structs(name, monkeypatch):
    """The routes of a plan this process has not run: the op list built over host buffers (nothing is launched) and walked by the
    ledger's descriptions and static checks."""
    from anoddpm_amd.unet import _Plan
    model, x, t = _model(name, monkeypatch, torch.device("cpu"))
    plan = _Plan(model, x.shape[0], x.shape[2], torch.device("cpu"))
    plan.stem.x, plan.posemb.t = x.data_ptr(), t.data_ptr()
    led = fl.ForwardLedger(fl.PlanView.of(plan, x, t))
    static = led.static_failures()
    assert not static and sum(len(L.idx) for L in led.launches) == len(plan.ops), static
    return _coverage(name, plan, led)


@pytest.mark.parametrize("name", list(PLANS))
def test_forward_ledger(name, monkeypatch):
    assert not FAULT, f"not run: an earlier plan raised ({FAULT[0]})"
    try:
        _ledger_of_plan(name, monkeypatch)
    except AssertionError:
        raise
    except BaseException as err:                             # a launch of the ledger's own arithmetic raised: the device is suspect
        FAULT.append(repr(err))
        raise


def _ledger_of_plan(name, monkeypatch):
    t0 = time.time()
    model, x, t = _model(name, monkeypatch, DEV)

    # 1. build the plan
    y1 = _forward(model, x, t)
    (plan,) = model._plans.values()
    assert plan.stem.x == x.data_ptr() and plan.posemb.t == t.data_ptr()
    view = fl.PlanView.of(plan, x, t)
    # 2. poison
    kept = _kept(plan, view)
    skip = {k[0].data_ptr() for k in kept}
    nw = sum(1 for k in kept if k[1].endswith("packed weights"))
    print(f"\nplan {name}: {len(plan.ops)} launches; poison step keeps {nw} packed weight buffers "
          f"({sum(k[0].numel() for k in kept if k[1].endswith('packed weights'))} floats) and "
          f"{[(n, tuple(tt.shape)) for tt, n, _ in kept if not n.endswith('packed weights')]}")
    assert len(kept) - nw == 1, "the frequency table is the one kept buffer that is no packed weight"
    npoison = 0
    for tt in view.keep:
        if tt.is_floating_point() and tt.data_ptr() not in skip:
            tt.fill_(float("nan"))
            npoison += 1
    if plan.csum_mode:
        assert not torch.isfinite(plan._csum_arena).any()
    # 3. the same forward again
    y2 = _forward(model, x, t)
    assert next(iter(model._plans.values())) is plan and len(model._plans) == 1
    bad = []
    if not torch.isfinite(y2).all():
        bad.append(("output", f"{int((~torch.isfinite(y2)).sum())} values not finite after the poison step: a launch read memory nobody wrote in this forward"))
    elif plan.csum_mode:
        d = float((y2 - y1).abs().max() / y1.abs().max())
        print(f"  second forward (fp64 atomics): max diff {d:.3e} of the output's magnitude (bar 1e-6)")
        if not d < 1e-6:
            bad.append(("output", f"differs by {d:.3e} after the poison step"))
    elif not torch.equal(y1, y2):
        bad.append(("output", f"not bit-identical: max diff {float((y1 - y2).abs().max()):.3e} of {float(y1.abs().max()):.3e}"))
    print(f"  poisoned {npoison} buffers; second forward: {len(bad)} findings")

    # 4. the ledger of the second forward's buffers
    led = fl.ForwardLedger(view, dev=DEV)
    static = led.static_failures()
    for s in static:
        print("  STATIC:", s)
    audited, nops = sum(len(L.idx) for L in led.launches), len(plan.ops)
    print(f"  launches {nops}: audited {audited}")
    routes = _coverage(name, plan, led)
    print(f"  routes: {sorted(routes)}")
    fails, figs = led.audit(log=print)
    worst = {}
    for L, oname, cls, fig, bar, ok in figs:
        if fig > worst.get(cls, (-1, 0))[0]:
            worst[cls] = (fig, bar)
    print("  worst per class: " + "; ".join(f"{k} {v[0]:.2e} ({100 * v[0] / v[1]:.1f} % of {v[1]:.0e})" for k, v in sorted(worst.items())))
    print(f"  plan {name}: wall time {time.time() - t0:.1f} s")
    del led, plan, model, view
    gc.collect()
    torch.cuda.empty_cache()
    assert audited == nops, f"{nops - audited} launches have no statement"
    assert not bad and not static and not fails, (bad, static, fails)


def test_routes_taken_over_all_plans(monkeypatch):
    """Every cfg 0-7, every statistics format, both fold kinds, a tail-attached GroupNorm, both res_mode values, both attention
    forms, OP_HEAD and the igemm head with OP_LAYOUT are reached by some plan of this module (a plan that did not run in this
    process is built from its structs alone)."""
    for name in PLANS:
        if name not in SEEN:
            with monkeypatch.context() as mp:
                _routes_from_structs(name, mp)
    have = set().union(*SEEN.values())
    assert EVERYWHERE | {"igemm head"} <= have, sorted((EVERYWHERE | {"igemm head"}) - have)
    print("  two-source finalize with mixed formats:", "present" if "two-source finalize, mixed formats" in have else "no candidate produces one")
