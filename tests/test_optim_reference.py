"""The fp64 reference of the optimiser tests (tests/optim_cases.py) against torch, and the fp32 baseline its bars come from.
CPU only."""
import copy

import numpy as np
import torch

import optim_cases as oc


class _Net(torch.nn.Module):
    """Odd-sized parameters, one of them a lone element."""

    def __init__(self, dtype):
        super().__init__()
        self.a = torch.nn.Linear(37, 64).to(dtype)
        self.b = torch.nn.Linear(64, 5).to(dtype)
        self.s = torch.nn.Parameter(torch.full((1,), 0.3, dtype=dtype))


def test_reference_matches_float64_torch_over_ten_chained_steps():
    """adamw_ema_ref + sumsq_ref chained over 10 steps == float64 torch.optim.AdamW + clip_grad_norm_ + update_ema_params to
    1e-12 relative: parameters, both moments, the EMA and the norm."""
    from UNet import update_ema_params
    torch.manual_seed(0)
    hp = dict(oc.HYPER, wd=0.01)
    net = _Net(torch.float64)
    ema = copy.deepcopy(net)
    with torch.no_grad():
        for q in ema.parameters():
            q.add_(0.01 * torch.randn_like(q))
    opt = torch.optim.AdamW(net.parameters(), lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["wd"], foreach=False)
    params = list(net.parameters())
    state = {"p": np.concatenate([q.detach().numpy().ravel() for q in params]),
             "ema": np.concatenate([q.detach().numpy().ravel() for q in ema.parameters()])}
    state["m"], state["v"] = np.zeros_like(state["p"]), np.zeros_like(state["p"])
    rs = np.random.RandomState(5)
    for step in range(1, 11):
        # odd steps are clipped (norm > 1), even ones are not
        g = rs.standard_normal(state["p"].size) * 10.0 ** rs.uniform(-6.0, 0.0, state["p"].size) * (1.0 if step % 2 else 1e-2)
        o = 0
        for q in params:
            q.grad = torch.from_numpy(g[o:o + q.numel()].reshape(q.shape).copy())
            o += q.numel()
        norm = torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        update_ema_params(ema, net, hp["decay"])
        ss, norm_ref, clip = oc.sumsq_ref(g, 1.0)
        assert (clip < 1.0) == bool(step % 2)
        assert abs(norm.item() - norm_ref) <= 1e-12 * norm_ref
        ref = oc.adamw_ema_ref(state["p"], state["m"], state["v"], state["ema"], g, clip, step, **hp)
        state = {k: ref[k] for k in ("p", "m", "v", "ema")}
    got = {"p": np.concatenate([q.detach().numpy().ravel() for q in params]),
           "ema": np.concatenate([q.detach().numpy().ravel() for q in ema.parameters()]),
           "m": np.concatenate([opt.state[q]["exp_avg"].numpy().ravel() for q in params]),
           "v": np.concatenate([opt.state[q]["exp_avg_sq"].numpy().ravel() for q in params])}
    for k, x in got.items():
        scale = np.maximum(np.abs(state[k]), np.abs(state[k]).max() * 1e-3)
        assert (np.abs(x - state[k]) <= 1e-12 * scale).all(), k


def _torch_fp32_step(st, scale, step, lr, betas, eps, wd, decay):
    """One fp32 step of torch.optim.AdamW(foreach=False) + update_ema_params on the CPU from the state `st`, entered at step
    count `step` - 1; the gradient is g * scale rounded to fp32 (clip_grad_norm_'s g.mul_(coef))."""
    from UNet import update_ema_params
    holder, ema = torch.nn.Module(), torch.nn.Module()
    holder.w = torch.nn.Parameter(torch.from_numpy(st["p"].copy()))
    ema.w = torch.nn.Parameter(torch.from_numpy(st["ema"].copy()))
    opt = torch.optim.AdamW([holder.w], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    opt.state[holder.w] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(st["m"].copy()),
                           "exp_avg_sq": torch.from_numpy(st["v"].copy())}
    holder.w.grad = torch.from_numpy(st["g"].copy()).mul_(torch.tensor(scale, dtype=torch.float32))
    opt.step()
    assert float(opt.state[holder.w]["step"]) == step
    update_ema_params(ema, holder, decay)
    return {"p": holder.w.detach().numpy(), "ema": ema.w.detach().numpy(),
            "m": opt.state[holder.w]["exp_avg"].numpy(), "v": opt.state[holder.w]["exp_avg_sq"].numpy()}


def test_torch_fp32_stays_within_its_recorded_baseline():
    """Measures the bars: fp32 torch on the CPU against the fp64 reference through the metric, every step of STEPS, both weight
    decays, three clip factors.  optim_cases.TORCH_T records the worst figures (rounded up); the device kernel
    is held to KERNEL_MARGIN times them."""
    ledger, bad = {}, []
    for i, step in enumerate(oc.STEPS):
        for wd in oc.WEIGHT_DECAYS:
            scale = oc.TORCH_SCALES[(i + (wd > 0)) % len(oc.TORCH_SCALES)]
            st = oc.case(oc.TORCH_N, seed=i, step=step)
            hp = dict(oc.HYPER, wd=wd)
            got = _torch_fp32_step(st, scale, step, **hp)
            ref = oc.adamw_ema_ref(st["p"], st["m"], st["v"], st["ema"], st["g"], scale, step, **hp)
            assert ref["v"].min() > 1e-30 and (np.abs(st["g"]) > 1e-15).all()       # the generator stays clear of fp32 denormals
            bad += oc.beyond(f"torch fp32 step {step} wd {wd} scale {scale}", got, ref, oc.TORCH_T, hp["decay"], ledger)
    # a parameter the loss does not reach: weight decay only, nothing non-finite
    st = oc.case(4099, seed=99, step=3, zero_grad=True)
    hp = dict(oc.HYPER, wd=0.01)
    got = _torch_fp32_step(st, 1.0, 3, **hp)
    ref = oc.adamw_ema_ref(st["p"], st["m"], st["v"], st["ema"], st["g"], 1.0, 3, **hp)
    assert not got["m"].any() and not got["v"].any()
    bad += oc.beyond("torch fp32 zero gradient", got, ref, oc.TORCH_T, hp["decay"], ledger)
    print("worst torch fp32 figures:", {k: round(x, 3) for k, x in ledger.items()})
    assert not bad, "\n".join(bad)
    # the record is the measurement, not a loose ceiling
    for k, x in ledger.items():
        assert oc.TORCH_T[k] - x < 1.0, (k, x, oc.TORCH_T[k])


def test_metric_sees_the_fp32_derived_constants():
    """The metric has teeth: the same fp64 step with 1 - b2 and 1 - b2^t formed in fp32 from fp32 betas (what a host that
    carries `float` hyper-parameters computes) is far beyond the kernel's bars in v and p."""
    st = oc.case(1 << 14, seed=3, step=2)
    hp = dict(oc.HYPER, wd=0.0)
    ref = oc.adamw_ema_ref(st["p"], st["m"], st["v"], st["ema"], st["g"], 1.0, 2, **hp)
    f = np.float32
    b1, b2 = f(hp["betas"][0]), f(hp["betas"][1])
    omb1, omb2 = float(f(1) - b1), float(f(1) - b2)
    bc1, bc2 = float(f(1) - b1 * b1), float(f(1) - b2 * b2)
    g, m, v, p, e = (st[k].astype(np.float64) for k in ("g", "m", "v", "p", "ema"))
    m1 = float(b1) * m + omb1 * g
    v1 = float(b2) * v + omb2 * g * g
    p1 = p - (hp["lr"] / bc1) * (m1 / (np.sqrt(v1) / np.sqrt(bc2) + hp["eps"]))
    got = {"p": p1.astype(f), "m": m1.astype(f), "v": v1.astype(f), "ema": (hp["decay"] * e + (1 - hp["decay"]) * p1).astype(f)}
    r = oc.ratios(got, ref, decay=hp["decay"], t_p=oc.KERNEL_T["p"])
    print(r)
    assert r["v"] > 10 * oc.KERNEL_T["v"] and r["p"] > 5 * oc.KERNEL_T["p"]
    assert r["m"] <= oc.KERNEL_T["m"]


def test_sumsq_ref_and_case_generator():
    g = np.array([3.0, -4.0, 12.0], dtype=np.float32)
    assert oc.sumsq_ref(g, 1.0) == (169.0, 13.0, 1.0 / (13.0 + 1e-6))
    assert oc.sumsq_ref(g, 100.0)[2] == 1.0 and oc.sumsq_ref(g, 0.0)[2] == 1.0 and oc.sumsq_ref(g, -1.0)[2] == 1.0
    assert oc.sumsq_ref(np.zeros(0, np.float32), 1.0) == (0.0, 0.0, 1.0)
    a, b = oc.case(1001, seed=4, step=10), oc.case(1001, seed=4, step=10)
    assert all(a[k].dtype == np.float32 and (a[k] == b[k]).all() for k in a)
    assert 0.4 < (a["p"] == 0).mean() < 0.6 and (a["v"] >= 0).all() and (a["m"] < 0).any() and (a["m"] > 0).any()
    assert 0.15 < (a["v"] == 0).mean() < 0.35 and ((a["v"] == 0) == (a["m"] == 0)).all()
    first = oc.case(1001, seed=4, step=1)
    assert not first["m"].any() and not first["v"].any() and (first["g"] == a["g"]).all()
    z = oc.case(7, zero_grad=True)
    assert not z["g"].any() and not z["m"].any() and not z["v"].any() and z["p"].any()
    assert oc.ulps32(np.float32(1.0) + np.float32(2.0 ** -23), 1.0) == 1.0


def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    """step < 1, a NULL state pointer and a buffer off 16-byte alignment are errors of anoddpm_adamw_ema / anoddpm_sumsq that are
    found before any launch (the addresses are never dereferenced), and n == 0 is a no-op; the struct carries doubles."""
    import ctypes
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert all(dict(_lib.AdamwArgs._fields_)[k] is ctypes.c_double for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "ema_decay"))

    def call(n=64, step=1, **over):
        a = _lib.AdamwArgs()
        a.p, a.m, a.v, a.ema, a.g = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
        a.n, a.step = n, step
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.ema_decay = 1e-4, 0.9, 0.999, 1e-8, 0.01, 0.9999
        for k, x in over.items():
            setattr(a, k, x)
        return L.anoddpm_adamw_ema(ctypes.byref(a), None)

    assert call(n=0) == 0
    for k in ("p", "m", "v", "g", "ema"):
        assert call(**{k: 0x60004}) == -1 and b"16-byte" in L.anoddpm_last_error(), k
    for k in ("p", "m", "v", "g"):
        assert call(**{k: None}) == -1, k
    assert call(step=0) == -1 and call(step=-3) == -1 and call(n=-1) == -1
    assert L.anoddpm_adamw_ema(None, None) == -1
    assert L.anoddpm_sumsq(0x10004, 64, 0x20000, 0x30000, 1.0, None) == -1 and b"16-byte" in L.anoddpm_last_error()
    assert L.anoddpm_sumsq(None, 64, 0x20000, 0x30000, 1.0, None) == -1
    assert L.anoddpm_sumsq(0x10000, 64, None, 0x30000, 1.0, None) == -1
    assert L.anoddpm_sumsq(0x10000, 64, 0x20000, None, 1.0, None) == -1
    assert L.anoddpm_sumsq(0x10000, -1, 0x20000, 0x30000, 1.0, None) == -1
