"""-m gpu: anoddpm_adamw_ema and anoddpm_sumsq (csrc/optim.hip) element by element against the fp64 reference of
tests/optim_cases.py, at the sizes that reach each path of their index arithmetic, and FusedAdamWEMA on odd-sized parameters.

Every step starts from fp32 state the test uploads, so a figure is one step's error, never a compounded one.  Every buffer is a
16-byte-aligned slice of a larger allocation with GUARD sentinel elements on each side; sentinels, the gradient and the unused
part of the sumsq workspace must come back unchanged.  The bars are optim_cases.KERNEL_T (4x fp32 torch's measured figures).

Worst figures on the MI355X over this file (bars m 12, v 18, p 20, e 10):
    constants formed in fp32 from `float` hyper-parameters (ABI <= 29):  m 5.54, v 219.4, p 170.6, e 2740.6   (21 of 37 tests fail)
    constants formed in double and rounded once (ABI 30):                m 2.38, v 4.01,  p 5.71,  e 1.28"""
import functools

import numpy as np
import pytest
import torch

import hipops
import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = -1234.5
EINVAL = -1

# anoddpm_adamw_ema: a workgroup owns `per` 16-byte quads (at least one unrolled trip of 512), 256 quads per pass.
#   1, 3: tail only; 4, 5: one quad (+ tail); 1023, 1024: remainder loop only; 2048: exactly one unrolled trip; 2052: a second
#   workgroup that owns one quad; 4095: unrolled + remainder in one workgroup, thread 255 diverges, 3-element tail
SMALL = (0, 1, 3, 4, 5, 1023, 1024, 2048, 2052, 4095)
# per = 1024 (two unrolled trips per workgroup), 2049 workgroups, a ragged last one, tail of 1
LARGE = 8391409
# anoddpm_sumsq: one workgroup per 256 elements up to a cap of 2048, four quads in flight per thread.
#   257: two workgroups; 524 288: exactly the cap; 524 289 / 525 315: past it; LARGE: the 4-deep loop plus one remainder quad
SUMSQ_SIZES = (0, 1, 3, 4, 255, 256, 257, 1023, 524288, 524289, 525315, LARGE)
SUMSQ_BLOCKS = 2048
SCALES = ("none", "clipped", "unclipped", "zero")

LEDGER = {}


class Guarded:
    """n elements, 16-byte aligned, inside an allocation with GUARD sentinels on each side.  `ptr` is the address of element 0
    (also for n == 0, where a tensor view has no address)."""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + n]
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()
        assert self.ptr % 16 == 0

    def load(self, arr):
        self.buf.fill_(SENTINEL)
        if self.n:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))

    def numpy(self):
        return self.view.cpu().numpy().copy()

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all() and (self.buf[GUARD + self.n:] == SENTINEL).all())


class Norm:
    """out[3] and the 2048-double workspace of anoddpm_sumsq, guarded."""

    def __init__(self):
        self.out = Guarded(3)
        self.ws = Guarded(SUMSQ_BLOCKS, torch.float64)

    def run(self, g, max_norm):
        """-> fp32[3]; checks that nothing but out[0..2] and the partials of the launched workgroups was written."""
        self.out.load(np.full(3, SENTINEL, np.float32))
        self.ws.load(np.full(SUMSQ_BLOCKS, SENTINEL))
        hipops.sumsq(g.ptr, g.n, self.out.ptr, self.ws.ptr, max_norm)
        used = min(max(-(-g.n // 256), 1), SUMSQ_BLOCKS)
        assert self.out.intact() and self.ws.intact() and g.intact()
        assert (self.ws.view[used:] == SENTINEL).all(), "sumsq wrote workspace entries beyond its workgroups"
        return self.out.numpy()


class Rig:
    """The five guarded state buffers of one size."""

    def __init__(self, n):
        self.n = n
        self.bufs = {k: Guarded(n) for k in ("p", "m", "v", "ema", "g")}
        self.norm = Norm()

    def step(self, st, *, step, wd, ema=True, grad_scale=None):
        """One launch from the fp32 state `st` -> dict of fp32 outputs (ema: None when the launch got a NULL ema)."""
        for k, b in self.bufs.items():
            b.load(st[k])
        b = self.bufs
        hipops.adamw_ema(b["p"].ptr, b["m"].ptr, b["v"].ptr, b["g"].ptr, b["ema"].ptr if ema else None, grad_scale,
                         n=self.n, step=step, wd=wd, **oc.HYPER)
        assert all(x.intact() for x in b.values()), "a sentinel beside a state buffer changed"
        got = {k: b[k].numpy() for k in ("p", "m", "v", "ema")}
        assert np.array_equal(b["g"].numpy(), st["g"]), "the gradient buffer changed"
        if not ema:
            assert np.array_equal(got["ema"], st["ema"]), "a launch with a NULL ema wrote the ema buffer"
            got["ema"] = None
        return got

    def scale(self, st, kind):
        """(grad_scale argument, the factor the reference multiplies by) of a scale kind; the clip factor comes from
        anoddpm_sumsq on the case's own gradient and is checked against the fp64 one."""
        if kind == "none":
            return None, 1.0
        self.bufs["g"].load(st["g"])
        _, norm, _ = oc.sumsq_ref(st["g"], 1.0)
        max_norm = {"clipped": 0.5 * norm, "unclipped": 2.0 * norm, "zero": 1.0}[kind]
        if self.n == 0:
            max_norm = 1.0
        out = self.norm.run(self.bufs["g"], max_norm)
        clip = oc.sumsq_ref(st["g"], np.float32(max_norm))[2]
        assert oc.ulps32(out[2], clip) <= 4, (kind, out, clip)
        if kind == "clipped" and self.n:
            assert out[2] < 1.0
        else:
            assert out[2] == 1.0
        return self.norm.out.ptr + 8, float(out[2])


@functools.lru_cache(maxsize=None)
def rig(n):
    return Rig(n)


def check_config(r, tag, *, step, wd, kind, both_ema=True, seed=0):
    """One (step, weight decay, scale kind) at the rig's size: metric on every element, and p, m, v bit-identical between a launch
    with an ema and one without.  Returns the failure lines."""
    st = oc.case(r.n, seed=seed, step=step, zero_grad=(kind == "zero"))
    scale_ptr, s = r.scale(st, kind)
    got = r.step(st, step=step, wd=wd, ema=True, grad_scale=scale_ptr)
    ref = oc.adamw_ema_ref(st["p"], st["m"], st["v"], st["ema"], st["g"], s, step, wd=wd, **oc.HYPER)
    bad = oc.beyond(tag, got, ref, oc.KERNEL_T, oc.HYPER["decay"], LEDGER) if r.n else []
    if kind == "zero" and r.n:
        assert not got["m"].any() and not got["v"].any()
        assert all(np.isfinite(got[k]).all() for k in got)
        # weight decay only: the decay's constant and its product round once each
        assert (np.abs(got["p"].astype(np.float64) - ref["p"]) <= oc.tol_p(ref, 0.0)).all()
        if wd == 0.0:
            assert np.array_equal(got["p"], st["p"])
    if both_ema:
        bare = r.step(st, step=step, wd=wd, ema=False, grad_scale=scale_ptr)
        for k in ("p", "m", "v"):
            assert np.array_equal(bare[k].view(np.uint32), got[k].view(np.uint32)), f"{tag}: {k} differs without an ema"
    return bad


@pytest.mark.parametrize("n", SMALL)
def test_adamw_ema_every_element_small_sizes(n):
    """The full product step x weight decay x scale kind x {ema, NULL} at each small size."""
    r = rig(n)
    bad = []
    for step in oc.STEPS:
        for wd in oc.WEIGHT_DECAYS:
            for kind in SCALES:
                bad += check_config(r, f"n {n} step {step} wd {wd} {kind}", step=step, wd=wd, kind=kind, seed=n)
    assert not bad, "\n".join(bad)


# the large size once per axis: every step; then NULL ema, each scale kind and weight decay away from the first line
LARGE_CONFIGS = [dict(step=s, wd=0.0, kind="none") for s in oc.STEPS] + [
    dict(step=3, wd=0.0, kind="clipped"), dict(step=3, wd=0.0, kind="unclipped"), dict(step=3, wd=0.0, kind="zero"),
    dict(step=10, wd=0.01, kind="clipped")]


@pytest.mark.parametrize("cfg", LARGE_CONFIGS, ids=lambda c: f"step{c['step']}-wd{c['wd']}-{c['kind']}")
def test_adamw_ema_every_element_large_size(cfg):
    bad = check_config(rig(LARGE), f"n {LARGE} step {cfg['step']} wd {cfg['wd']} {cfg['kind']}", both_ema=False, **cfg)
    assert not bad, "\n".join(bad)


def test_adamw_ema_large_size_without_ema_and_twice():
    """At the large size: p, m, v bit-identical with and without an ema, and two launches from one state bit-identical."""
    r = rig(LARGE)
    st = oc.case(LARGE, step=2)
    a = r.step(st, step=2, wd=0.01, ema=True)
    b = r.step(st, step=2, wd=0.01, ema=True)
    c = r.step(st, step=2, wd=0.01, ema=False)
    for k in ("p", "m", "v", "ema"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    for k in ("p", "m", "v"):
        assert np.array_equal(a[k].view(np.uint32), c[k].view(np.uint32)), k
    ref = oc.adamw_ema_ref(st["p"], st["m"], st["v"], st["ema"], st["g"], 1.0, 2, wd=0.01, **oc.HYPER)
    bad = oc.beyond(f"n {LARGE} step 2 wd 0.01 none", a, ref, oc.KERNEL_T, oc.HYPER["decay"], LEDGER)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n", (5, 4095))
def test_adamw_ema_twice_from_one_state_is_bit_identical(n):
    r = rig(n)
    st = oc.case(n, seed=7, step=10)
    scale_ptr, _ = r.scale(st, "clipped")
    a = r.step(st, step=10, wd=0.01, grad_scale=scale_ptr)
    b = r.step(st, step=10, wd=0.01, grad_scale=scale_ptr)
    for k in ("p", "m", "v", "ema"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_against_fp64(n):
    """out[0] within 1 ulp of the rounded fp64 sum, norm and clip factor within 4 ulp (two or three correctly rounded fp32
    operations after an essentially exact sum), exactly 1 for max_norm <= 0, two runs bit-identical."""
    g = oc.case(n, seed=11)["g"]
    buf = Guarded(n)
    buf.load(g)
    nr = Norm()
    ss, norm, _ = oc.sumsq_ref(g, 1.0)
    for max_norm in ((0.5 * norm, 2.0 * norm, 1.0, 0.0, -1.0) if n else (1.0, 0.0, -1.0)):
        ref = oc.sumsq_ref(g, np.float32(max_norm))
        out = nr.run(buf, max_norm)
        again = nr.run(buf, max_norm)
        print(f"sumsq n {n} max_norm {max_norm:.6g}: out {out}  ulps {[oc.ulps32(out[i], ref[i]) if ref[i] else 0.0 for i in range(3)]}")
        assert np.array_equal(out.view(np.uint32), again.view(np.uint32))
        assert np.array_equal(buf.numpy(), g)
        if n == 0:
            assert out[0] == 0.0 and out[1] == 0.0
        else:
            assert oc.ulps32(out[0], ref[0]) <= 1 and oc.ulps32(out[1], ref[1]) <= 4
        assert oc.ulps32(out[2], ref[2]) <= 4
        raw = max_norm / (norm + 1e-6) if max_norm > 0.0 else np.inf
        assert abs(raw - 1.0) > 1e-5            # the cases stay clear of the clamp's edge
        assert (out[2] == 1.0) if raw > 1.0 else (out[2] < 1.0)
    # an all-zero gradient: the factor is exactly 1, not max_norm / 1e-6
    if n:
        buf.load(np.zeros(n, np.float32))
        assert list(nr.run(buf, 1.0)) == [0.0, 0.0, 1.0]


def test_argument_checks_refuse_before_any_launch():
    """Misaligned buffers, step 0 and a NULL p are errors, and the buffers are as they were."""
    from anoddpm_amd import _lib
    n = 2052
    r = rig(n)
    st = oc.case(n, seed=5, step=3)
    for k, b in r.bufs.items():
        b.load(st[k])
    ptrs = {k: b.ptr for k, b in r.bufs.items()}

    def call(step=3, **over):
        a = dict(ptrs, **over)
        return hipops.adamw_ema(a["p"], a["m"], a["v"], a["g"], a["ema"], None, n=n - 4, step=step, wd=0.01, raw=True, **oc.HYPER)

    for k in ("p", "m", "v", "g", "ema"):
        assert call(**{k: ptrs[k] + 4}) == EINVAL, k
        assert b"16-byte" in _lib.lib().anoddpm_last_error()
    assert call(step=0) == EINVAL
    assert call(step=-1) == EINVAL
    assert call(p=None) == EINVAL
    nr = Norm()
    assert hipops.sumsq(ptrs["g"] + 4, n - 4, nr.out.ptr, nr.ws.ptr, 1.0, raw=True) == EINVAL
    assert hipops.sumsq(None, n, nr.out.ptr, nr.ws.ptr, 1.0, raw=True) == EINVAL
    assert hipops.sumsq(ptrs["g"], n, None, nr.ws.ptr, 1.0, raw=True) == EINVAL
    torch.cuda.synchronize()
    for k, b in r.bufs.items():
        assert np.array_equal(b.numpy(), st[k]) and b.intact(), k
    assert (nr.out.buf == SENTINEL).all() and (nr.ws.buf == SENTINEL).all()


class OddNet(torch.nn.Module):
    """Odd-sized parameters: 37x64, 64, 64x5, 5 and a lone element; the flat layout pads each to a multiple of 4."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(37, 64)
        self.b = torch.nn.Linear(64, 5)
        self.s = torch.nn.Parameter(torch.full((1,), 0.3))


def test_fused_adamw_ema_ten_steps_full_tensors():
    """FusedAdamWEMA over 10 steps with weight decay and clipping; each step's gradient is written into flat_grad (no backward)
    and the fp64 reference steps from the optimiser's own fp32 state with the same gradient.  Full tensors under the metric, the
    padding between parameters exactly 0 everywhere, state_dict()'s exp_avg_sq under T_v."""
    import copy
    from anoddpm_amd.training import FlatBuffers, FusedAdamWEMA
    torch.manual_seed(0)
    net = OddNet().to(DEV)
    ema = copy.deepcopy(net)
    with torch.no_grad():
        for q in ema.parameters():
            q.add_(0.01 * torch.randn_like(q))
    flat, flat_ema = FlatBuffers(net), FlatBuffers(ema)
    hp = dict(oc.HYPER, wd=0.01)
    opt = FusedAdamWEMA(flat, flat_ema, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["wd"],
                        ema_decay=hp["decay"], max_norm=1.0)
    n = flat.numel
    real = np.zeros(n, dtype=bool)
    for q, o in zip(flat.params, flat.offsets):
        real[o:o + q.numel()] = True
    assert n == 2368 + 64 + 320 + 8 + 4 and real.sum() == 2368 + 64 + 320 + 5 + 1
    rs = np.random.RandomState(21)
    bad = []
    for step in range(1, 11):
        # odd steps are clipped (norm > 1), even ones are not
        g = (rs.standard_normal(n) * 10.0 ** rs.uniform(-6.0, 0.0, n) * (1.0 if step % 2 else 1e-2) * real).astype(np.float32)
        flat.flat_grad.copy_(torch.from_numpy(g))
        before = {"p": flat.flat_param.cpu().numpy(), "m": opt.m.cpu().numpy(), "v": opt.v.cpu().numpy(),
                  "ema": flat_ema.flat_param.cpu().numpy()}
        norm = opt.step()
        torch.cuda.synchronize()
        out = opt.norm_out.cpu().numpy()
        ss, norm_ref, clip = oc.sumsq_ref(g, 1.0)
        assert (clip < 1.0) == bool(step % 2)
        assert oc.ulps32(out[0], ss) <= 1 and oc.ulps32(out[1], norm_ref) <= 4 and oc.ulps32(out[2], clip) <= 4
        assert norm.item() == out[1]
        got = {"p": flat.flat_param.cpu().numpy(), "m": opt.m.cpu().numpy(), "v": opt.v.cpu().numpy(),
               "ema": flat_ema.flat_param.cpu().numpy()}
        ref = oc.adamw_ema_ref(before["p"], before["m"], before["v"], before["ema"], g, float(out[2]), step, **hp)
        bad += oc.beyond(f"FusedAdamWEMA step {step}", got, ref, oc.KERNEL_T, hp["decay"], LEDGER)
        assert np.array_equal(flat.flat_grad.cpu().numpy(), g)
        for k, x in got.items():
            assert not x[~real].any(), f"step {step}: padding of {k} is not 0"
        sd = opt.state_dict()["state"]
        assert len(sd) == len(flat.params)
        for i, (q, o) in enumerate(zip(flat.params, flat.offsets)):
            vs = sd[i]["exp_avg_sq"].cpu().numpy().reshape(-1).astype(np.float64)
            vr = ref["v"][o:o + q.numel()]
            assert sd[i]["exp_avg_sq"].shape == q.shape and float(sd[i]["step"]) == step
            assert (np.abs(vs - vr) <= oc.KERNEL_T["v"] * oc.U * vr).all(), f"step {step}: exp_avg_sq of parameter {i}"
            assert np.array_equal(sd[i]["exp_avg"].cpu().numpy().reshape(-1), got["m"][o:o + q.numel()])
    assert not bad, "\n".join(bad)
