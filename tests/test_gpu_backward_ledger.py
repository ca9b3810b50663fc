"""-m gpu: every launch of a real training backward against fp64 (tests/backward_ledger.py), and the rule that a plan buffer is
written before it is read within a step.

Per plan: (1) one forward + backward builds the plan; (2) every floating-point tensor the plan keeps and the gradient arena are
filled with NaN, except the named buffers of KEPT below (uploaded once at build time, read-only afterwards), and every p.grad is
dropped; (3) a second forward + backward on the same inputs must give finite and BIT-IDENTICAL output, input gradient and
parameter gradients -- a NaN means a launch consumed memory nobody wrote this step; (4) the backward list is walked: the static
checks of the ledger (first writer overwrites, later writers accumulate, no output over an input outside the declared in-place
forms), then every written region against the fp64 sum of its writers' contributions, recomputed on the device in fp64 from the
buffers the launches read (their own pointers, strides and aliasing).  Every figure is printed before it is asserted (-s); all
failures are collected and asserted once.

Bars: the constants of backward_ledger.py, each named after the op test it comes from.  No bar had to be re-derived: on the
first measurement (one MI355X) the worst figure of every class is at least four times below its bar --
    3x3 Winograd (cfg 3 / 2 / 6) 2.3e-5 of 1e-4 (c3_b4); 3x3 direct / small-map 1.0e-6, 1x1 9.6e-7, attention GEMMs 1.0e-6 and
    the softmax-backward chain 1.6e-6 of 2e-5; GroupNorm backward dx 8.5e-7, dgamma 2.2e-7, dbeta 1.5e-7, gnb_partial rows 2.5e-7
    of 2e-5; linear 3.1e-7 of 1e-5; head / stem 2.1e-7 of 2e-5; resample 8.1e-8 of 1e-6; the in-place dropout composite 1.0e-6.
The poison step found no read-before-write: the only floating-point buffer a step does not rewrite is the frequency table.
Wall time per plan, reference contractions in fp64 on the device: c3_b4 7.6 s, c3_b1 3.8 s, i32_conv 1.8 s (first plan of the
process), i32_drop 0.5 s, m64_b15 0.6 s.
"""
import gc
import time

import pytest
import torch

import backward_ledger as bl

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
C3 = dict(img_size=256, base_channels=128, n_heads=2, attention_resolutions="16,8")
PLANS = {
    "c3_b4": (C3, 4),                                       # the benchmarked training step
    "c3_b1": (C3, 1),                                       # other kernel choices on the same layers
    "i32_conv": (dict(img_size=32, base_channels=32, n_heads=2, attention_resolutions="16,8", biggan_updown=False, conv_resample=True), 2),
    "i32_drop": (dict(img_size=32, base_channels=32, n_heads=2, attention_resolutions="16,8", dropout=0.3), 2),
    "m64_b15": (dict(img_size=64, base_channels=32, n_heads=1), 15),
}


def _kept(plan):
    """Buffers the poison step leaves alone: (tensor, name, reason).  Everything else the plan keeps is rewritten by every step."""
    am = bl.AddressMap()
    for i, t in enumerate(plan.keep):
        am.add(t if torch.is_tensor(t) else None, f"keep[{i}]")
    kept = [(am.resolve(plan.posemb.freqs)[0], "posemb.freqs",
             "the sinusoid frequencies of the timestep features: computed on the host and uploaded when the plan is built")]
    from anoddpm_amd import _lib
    for code, st in plan.fwd_list:
        if code == _lib.OP_PACK_BATCH:
            kept.append((am.resolve(st.jobs)[0], "pack_batch.jobs", "device job table of the batched weight packing, uploaded at build time"))
            kept.append((am.resolve(st.block0)[0], "pack_batch.block0", "prefix sums of the pack jobs' block counts, uploaded at build time"))
    for code, st in plan.bops:
        if code == _lib.OP_LINEAR_BWD_BATCH:
            kept.append((am.resolve(st.jobs)[0], "linear_bwd_batch.jobs", "device job table of the batched embedding-projection backward"))
    return kept


def _step(model, x, t, tgt, seed):
    torch.manual_seed(seed)                                  # the dropout masks of a forward are one draw from torch's generator
    for p in model.parameters():
        p.grad = None
    x.grad = None
    y = model(x, t)
    ((y - tgt) ** 2).mean().backward()
    torch.cuda.synchronize()
    return y.detach().clone(), x.grad.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _coverage(name, plan, led):
    """What a plan must contain for this test to mean what it says, asserted from the structs."""
    from anoddpm_amd import _lib
    bops = plan.bops
    ig = [st for c, st in bops if c == _lib.OP_IGEMM]
    d3 = [st for st in ig if st.ks == 3]
    gnb = [st for c, st in bops if c == _lib.OP_GN_BWD]
    chains = [L for L in led.launches if L.what.startswith("attention_bwd")]
    assert chains, "no attention backward"
    if name == "c3_b4":
        assert {st.H for st in d3 if st.cfg == 3 and st.gnb_partial} >= {256, 128, 64}, sorted({st.H for st in d3 if st.gnb_partial})
        two = {g.da for g in gnb if g.c1 > 0}
        assert any(st.N in (384, 256) and st.out in two for st in d3), "no 3x3 data gradient over a concatenated input"
        assert any(g.a_mode == 1 for g in gnb) and any(g.a_mode == 2 for g in gnb)
        assert any(g.acc_dx & 1 for g in gnb) and any(g.acc_dx & 2 for g in gnb) and any(g.dres for g in gnb)
        assert any(st.ks == 1 and st.b_mode == 0 and led.packs[st.bmat].k0 > 0 for st in ig), "no 1x1 data gradient into a second source"
        assert {int(L.what.split("L=")[1].split()[0]) for L in chains} >= {256, 64}
        assert max(len(ws) for ws in led.regions().values()) >= 3, "no fan-in region with three writers"
        # the two-source skip convolutions of the up path are first writers of both sources' gradients (no res); the single-source
        # ones of the down path (128 -> 256, 256 -> 512) run after the up path wrote their input's gradient: res == out
        skip = [st for st in ig if st.ks == 1 and st.b_mode == 0 and "skip_connection" in led.pname[led.packs[st.bmat].w]]
        two_src = [st for st in skip if led.packs[st.bmat].kc < led.packs[st.bmat].K]
        print(f"  skip-convolution data gradients: {len(skip)} ({len(two_src)} into one of two sources), "
              f"with res == out: {sum(1 for st in skip if st.res and st.res == st.out)}")
        one_src = [st for st in skip if st not in two_src]
        assert two_src and not any(st.res for st in two_src)
        assert one_src and all(st.res and st.res == st.out for st in one_src)
    elif name == "c3_b1":
        assert any(st.ksplit > 1 for st in ig), "no split-K launch in the backward list"
    elif name == "i32_conv":
        assert any(st.res and st.res == st.out for st in d3), "no 3x3 launch that accumulates into its output (into_gx)"
        assert {st.mode for c, st in bops if c == _lib.OP_RESAMPLE} >= {4}
    elif name == "i32_drop":
        assert any(len(L.idx) == 2 and "dropout" in L.what for L in led.launches), "no in-place dropout backward"


@pytest.mark.parametrize("name", list(PLANS))
def test_backward_ledger(name):
    from UNet import UNetModel
    from anoddpm_amd import _lib
    from oracle import unet_oracle as uo
    kw, B = PLANS[name]
    S = kw["img_size"]
    t0 = time.time()
    torch.manual_seed(0)
    model = UNetModel(**kw)
    model.load_state_dict(uo.perturb(uo.fill_deterministic({k: tuple(v.shape) for k, v in model.state_dict().items()})))
    model.to(DEV).train()
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(B, 1, S, S, generator=g) * 2 - 1).to(DEV).requires_grad_(True)
    tgt = torch.randn(B, 1, S, S, generator=g).to(DEV)
    t = ((torch.arange(B) * 61 + 17) % 1000).to(DEV)         # a distinct timestep per image
    assert len(set(t.tolist())) == B

    # 1. build the plan
    y1, dx1, g1 = _step(model, x, t, tgt, seed=5)
    (plan,) = model._tplans.values()
    # 2. poison
    kept = _kept(plan)
    skip = {k[0].data_ptr() for k in kept}
    print(f"\nplan {name}: poison step keeps {[(n, tuple(tt.shape), str(tt.dtype)) for tt, n, _ in kept]}")
    npoison = 0
    for tt in list(plan.keep) + [plan.arena]:
        if torch.is_tensor(tt) and tt.is_floating_point() and tt.data_ptr() not in skip:
            tt.fill_(float("nan"))
            npoison += 1
    # 3. the same step again
    y2, dx2, g2 = _step(model, x, t, tgt, seed=5)
    assert next(iter(model._tplans.values())) is plan and len(model._tplans) == 1
    bad = []
    for what, a, b in [("output", y1, y2), ("dx", dx1, dx2)] + [("grad " + k, g1[k], g2[k]) for k in g1]:
        if not torch.isfinite(b).all():
            bad.append((what, "not finite after the poison step: a launch read memory nobody wrote this step"))
        elif not torch.equal(a, b):
            bad.append((what, f"not bit-identical: max diff {float((a - b).abs().max()):.3e} of {float(a.abs().max()):.3e}"))
    print(f"  poisoned {npoison} buffers; second step: {len(g2) + 2} outputs compared, {len(bad)} differ or are not finite")

    # 4. the ledger of the second step's buffers
    led = bl.Ledger(plan, x=x, dev=DEV)
    audited = sum(len(L.idx) for L in led.launches)
    groups = led.regions()
    fan = sum(1 for ws in groups.values() if len(ws) > 1)
    print(f"  backward launches {len(plan.bops)}: audited {audited}, exempt (weight gradients) {len(led.exempt)}; "
          f"regions {len(groups)}, fan-in regions {fan}")
    assert audited + len(led.exempt) == len(plan.bops)
    assert all(plan.bops[i][0] in (_lib.OP_WGRAD3, _lib.OP_WGRAD1, _lib.OP_COLSUM_FOLD) for i in led.exempt)
    _coverage(name, plan, led)
    checked = {ws[0][1].region.tensor.data_ptr() for ws in groups.values()}
    missing = [tuple(gb.shape) for gb in plan._grads.values() if gb.data_ptr() not in checked]
    assert not missing, f"gradient buffers no region check covers: {missing}"
    static = led.static_failures()
    for s in static:
        print("  STATIC:", s)
    fails, figs = led.audit(log=print)
    worst = {}
    for L, oname, nw, fig, bar, ok in figs:
        cls = L.what.split()[0] + ("." + oname if oname in ("gnb_partial", "dgamma", "dbeta", "dS") else "") + \
            (" wino" if L.what.startswith("dgrad3") and bar > 5e-5 else "")
        if fig > worst.get(cls, (-1, 0))[0]:
            worst[cls] = (fig, bar)
    print(f"  worst per class: " + "; ".join(f"{k} {v[0]:.2e} (bar {v[1]:.1e})" for k, v in sorted(worst.items())))
    print(f"  plan {name}: wall time {time.time() - t0:.1f} s")
    del led, plan, model, groups
    gc.collect()
    torch.cuda.empty_cache()
    assert not bad and not static and not fails, (bad, static, fails)
