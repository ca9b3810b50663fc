"""-m gpu: anoddpm_p_sample_update_resample through the C ABI, every output element bit for bit (a NaN equal to a NaN) against a
composition of existing entry points, joined by torch.where:
    anoddpm_philox_fill, kind 1, per sample in domains 8 v (step ti), 8 v + 3 (step s), 8 v + 4 (step land)    -> generated noises
    anoddpm_p_sample_update_known on planes                                                                  -> x_s, pred_x0, mean
    anoddpm_q_sample with host-built fp32 tables A[s], C[s] (fp64 numpy.sqrt, rounded once) at t = s           -> the re-noised image
    torch.where on the jump flag (resample_cases.jumps)                                                        -> x_prev
The composition is the reference: the same expressions built with the same flags, so there is no tolerance.  A poisoned sample
(out-of-range t, a jump or reps word < 1) is all NaN.  anoddpm_chain_advance_resample is driven alone, word for word against the
pure-Python state machine."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import known_cases as kc
import resample_cases as rc
from test_gpu_known_elements import DEV, NAN, diffusion, offset_copy, same
from test_resample_reference import refused_argument_sets

pytestmark = pytest.mark.gpu


def _lib():
    from anoddpm_amd import _lib
    return _lib


_TABLES = {}


def jump_tables(T, J):
    if (T, J) not in _TABLES:
        A, C = rc.jump_tables(diffusion(T)[0].alphas_cumprod, J)
        _TABLES[T, J] = (torch.from_numpy(A).to(DEV), torch.from_numpy(C).to(DEV))
    return _TABLES[T, J]


def i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


class Case:
    """Device operands of one launch.  row: (t, top, rep, visit) per sample; form: resample_cases.FORMS; full = (x0, keep, known
    noise, re-noise) planes per sample (stride n) or one for all (stride 0); words = (jump, reps)."""

    def __init__(self, n, T, J, row, form, mask="random", full=(True,) * 4, offset=0, streams=True, seed=0, reps=2):
        self.B, self.n, self.T, self.J, self.R, self.row, self.form, self.full = len(row), n, T, J, reps, row, form, full
        B = self.B
        self.seeded, self.kz_plane, self.rz_plane = rc.FORMS[form]
        x_t, eps, z, x0, kz, rz = (torch.from_numpy(a) for a in rc.inputs(B, n, seed))
        keep = torch.from_numpy(kc.keep_plane(mask, B, n, seed))
        x0, keep, kz, rz = (p if f else p[:1] for p, f in zip((x0, keep, kz, rz), full))
        fo, ko = (1 if offset == 1 else 0), (1 if offset == 2 else 0)
        self.x_t, self.eps, self.z, self.x0, self.kz, self.rz = (offset_copy(a, fo) for a in (x_t, eps, z, x0, kz, rz))
        self.keep = offset_copy(keep, ko)
        self.fo = fo
        self.t = torch.tensor([r[0] for r in row], dtype=torch.int64, device=DEV)
        self.top, self.rep, self.visit = (i32(r[i] for r in row) for i in (1, 2, 3))
        self.jump_w, self.reps_w = i32([J]), i32([reps])
        self.seed = torch.tensor([kc.SEED], dtype=torch.int64, device=DEV)
        self.stream_ids = [5, -1, 0, 9][:B] if streams else [(2 ** 32 - 2 + b) & 0xFFFFFFFF for b in range(B)]
        self.streams = i32(self.stream_ids) if streams else None
        self.stream0 = 0 if streams else 2 ** 32 - 2

    def out(self):
        return offset_copy(torch.full((self.B, self.n), NAN), self.fo)

    def update_args(self, x_t, x_prev, pred, mean, noise):
        L = _lib()
        _, tb, _ = diffusion(self.T)
        a = L.PUpdateArgs()
        a.x_prev, a.pred_x0, a.mean_out = L.ptr(x_prev), L.ptr(pred), L.ptr(mean)
        a.x_t, a.eps, a.t, a.noise = L.ptr(x_t), L.ptr(self.eps), L.ptr(self.t), L.ptr(noise)
        a.c_recip, a.c_recipm1 = L.ptr(tb.sqrt_recip_alphas_cumprod), L.ptr(tb.sqrt_recipm1_alphas_cumprod)
        a.c_coef1, a.c_coef2, a.c_sigma = L.ptr(tb.posterior_mean_coef1), L.ptr(tb.posterior_mean_coef2), L.ptr(tb.sigma)
        a.n, a.B, a.T = self.n, self.B, self.T
        return a

    def known_args(self, kz, full):
        L = _lib()
        _, tb, _ = diffusion(self.T)
        k = L.KnownArgs()
        k.x0, k.keep, k.noise = L.ptr(self.x0), L.ptr(self.keep), L.ptr(kz)
        k.ca, k.cb = L.ptr(tb.sqrt_alphas_cumprod), L.ptr(tb.sqrt_one_minus_alphas_cumprod)
        k.x0_stride, k.keep_stride, k.noise_stride = (self.n if f else 0 for f in full)
        return k

    def resample_args(self):
        L = _lib()
        r = L.ResamplingArgs()
        r.jump, r.reps, r.top, r.rep, r.visit = (L.ptr(w) for w in (self.jump_w, self.reps_w, self.top, self.rep, self.visit))
        r.noise = L.ptr(self.rz) if self.rz_plane else None
        r.noise_stride = self.n if self.rz_plane and self.full[3] else 0
        r.alphas_cumprod = L.ptr(diffusion(self.T)[2])
        return r

    def key(self):
        L = _lib()
        return (L.ptr(self.seed), L.ptr(self.streams), self.stream0) if self.seeded else (None, None, 0)

    def fused(self, alias=False, outs=True):
        L = _lib()
        x_t = offset_copy(self.x_t, self.fo) if alias else self.x_t
        x_prev = x_t if alias else self.out()
        pred, mean = (self.out(), self.out()) if outs else (None, None)
        a = self.update_args(x_t, x_prev, pred, mean, None if self.seeded else self.z)
        k = self.known_args(self.kz if self.kz_plane else None, self.full[:3])
        r = self.resample_args()
        L.check(L.lib().anoddpm_p_sample_update_resample(ctypes.byref(a), ctypes.byref(k), ctypes.byref(r), *self.key(),
                                                         L.current_stream()), "resample")
        return x_prev, pred, mean

    def state(self):
        """Per sample (normalised ti, s, poisoned, jumps, land), from the predicate alone."""
        out = []
        for t, top, rep, _ in self.row:
            ti, ok = kc.normalise(t, self.T)
            poisoned = not ok or self.J < 1 or self.R < 1
            s = -1 if poisoned else ti - 1
            jump = not poisoned and rc.jumps(s, self.J, self.R, top, rep)
            out.append((ti, s, poisoned, jump, s + self.J if jump else s))
        return out

    def filled(self, kind, steps):
        """The generated noise of every sample in domain kind + 8 visit at steps[b]: one anoddpm_philox_fill per sample."""
        L = _lib()
        out = torch.empty((self.B, self.n), dtype=torch.float32, device=DEV)
        for b, (_, _, _, visit) in enumerate(self.row):
            L.check(L.lib().anoddpm_philox_fill(L.ptr(out[b]), 1, 1, self.n, L.ptr(self.seed), None, self.stream_ids[b] & 0xFFFFFFFF,
                                                (kind + 8 * visit) & 0xFFFFFFFF, None, max(steps[b], 0), 0, L.current_stream()), "fill")
        return out

    def composition(self):
        L = _lib()
        lib = L.lib()
        st = self.state()
        z = self.filled(rc.STEP, [v[0] for v in st]) if self.seeded else self.z
        kz = self.kz.expand(self.B, self.n).contiguous() if self.kz_plane else self.filled(rc.KNOWN, [v[1] for v in st])
        rz = self.rz.expand(self.B, self.n).contiguous() if self.rz_plane else self.filled(rc.RENOISE, [v[4] for v in st])
        x_s, pred, mean = self.out(), self.out(), self.out()
        a = self.update_args(self.x_t, x_s, pred, mean, z)
        k = self.known_args(kz, self.full[:2] + (True,))
        L.check(lib.anoddpm_p_sample_update_known(ctypes.byref(a), ctypes.byref(k), None, None, None, None, None, 0,
                                                  L.current_stream()), "known")
        A, C = jump_tables(self.T, max(self.J, 1))
        s_dev = torch.tensor([max(v[1], 0) for v in st], dtype=torch.int64, device=DEV)
        x_in = x_s.contiguous()
        q = torch.empty_like(x_in)
        L.check(lib.anoddpm_q_sample(L.ptr(q), L.ptr(x_in), L.ptr(rz), L.ptr(s_dev), L.ptr(A), L.ptr(C), self.B, self.n, self.T,
                                     L.current_stream()), "q_sample")
        jump = torch.tensor([v[3] for v in st], device=DEV)[:, None]
        poisoned = torch.tensor([v[2] for v in st], device=DEV)[:, None]
        want = torch.where(jump, q, x_in)
        return torch.where(poisoned, torch.full_like(want, NAN), want), pred, mean


@pytest.mark.parametrize("n", rc.NS)
def test_every_element_equals_the_composition(n):
    """Schedule x state row x noise form in full, with mask kind x stride words x pointer offsets x aliasing x optional outputs
    cycled over them; every value of each of those is seen at every n.  Outputs NaN-poisoned before the call."""
    aux = rc.aux_cases()
    start = rc.NS.index(n) * 48
    seen = [set() for _ in range(5)]
    count = jumped = 0
    for i, ((T, J), form) in enumerate(itertools.product(rc.SCHEDULES, rc.FORMS)):
        for j, row in enumerate(rc.rows(T, J)):
            mask, full, offset, alias, outs = what = aux[(start + count) % len(aux)]
            c = Case(n, T, J, row, form, mask, full, offset, streams=bool((i + j) % 2), seed=count % 3)
            assert [v[3] for v in c.state()] == rc.expected_flags(row, T, J)
            want = c.composition()
            got = c.fused(alias, outs)
            assert same(got[0], want[0]), (T, J, row, form, what)
            if outs:
                assert same(got[1], want[1]) and same(got[2], want[2]), (T, J, row, form, what)
            else:
                assert got[1] is None and got[2] is None
            for b, v in enumerate(c.state()):
                assert bool(torch.isnan(got[0][b]).all()) == v[2] and (v[2] or bool(torch.isfinite(got[0][b]).all()))
                jumped += v[3]
            for s, v in zip(seen, what):
                s.add(v)
            count += 1
    assert count == 48 and jumped >= 48
    assert seen[0] == set(kc.MASKS) and seen[1] >= {(True,) * 4, (False,) * 4} and seen[2] == {0, 1, 2}
    assert seen[3] == {False, True} == seen[4]
    for w in range(4):
        assert {f[w] for f in seen[1]} == {True, False}                        # every stride word both ways


def test_second_trip_of_the_grid_stride_loop():
    """n one quad past 4096 workgroups x 256 quads, a jumping sample: the last quad is reached on a thread's second trip."""
    n, T, J = rc.N_SECOND_TRIP, kc.T_BIG, 10
    for form in ("fresh", "tensor"):
        c = Case(n, T, J, [(501, 510, 1, 2)], form)
        want = c.composition()
        got = c.fused(False, True)
        assert c.state()[0][3] and all(same(g, w) for g, w in zip(got, want)), form
        assert torch.isfinite(got[0][:, -4:]).all() and not same(got[0][:, -4:], c.x_t[:, -4:])


def test_without_a_jump_at_visit_zero_the_bits_are_the_known_launch():
    L = _lib()
    n, T, J = 1028, kc.T_BIG, 10
    row = [(501, 999, 0, 0), (506, 999, 1, 0), (0, 999, 1, 0)]
    for form in ("tensor", "gauss", "fresh"):
        c = Case(n, T, J, row, form)
        assert not any(v[3] for v in c.state())
        got = c.fused()
        x_s, pred, mean = c.out(), c.out(), c.out()
        a = c.update_args(c.x_t, x_s, pred, mean, None if c.seeded else c.z)
        k = c.known_args(c.kz if c.kz_plane else None, c.full[:3])
        L.check(L.lib().anoddpm_p_sample_update_known(ctypes.byref(a), ctypes.byref(k), None, None, None, *c.key(), L.current_stream()), "known")
        assert all(same(g, w) for g, w in zip(got, (x_s, pred, mean))), form


def test_visit_changes_every_generated_noise():
    """The same launch at visit 0 and 2 shares no element: the repeated pass over a segment draws its own randomness."""
    n, T, J = 1028, kc.T_BIG, 10
    a = Case(n, T, J, [(501, 510, 1, 0), (506, 999, 1, 0)], "fresh", "checker").fused()[0]
    b = Case(n, T, J, [(501, 510, 1, 2), (506, 999, 1, 2)], "fresh", "checker").fused()[0]
    assert float((a == b).float().mean()) < 0.01


def test_poison_words_and_out_of_range_timesteps():
    T, J = kc.T_SMALL, 2
    row = rc.rows(T, J)[0]
    for J_, R_ in ((0, 2), (2, 0), (-3, 2), (2, -1)):
        c = Case(1028, T, J_, row, "gauss", "ones", reps=R_)
        assert same(c.fused()[0], c.composition()[0]) and torch.isnan(c.fused()[0]).all()
    c = Case(1028, T, J, rc.rows(T, J)[3], "gauss", "ones")
    got = c.fused()[0]
    assert torch.isnan(got[0]).all() and torch.isnan(got[2]).all() and torch.isfinite(got[1]).all()
    c = Case(5, T, J, [(5, T + 3, 1, 0), (7, T + 3, 1, 0)], "tensor")             # a `top` beyond the schedule: s + J == T is poisoned
    got = c.fused()[0]
    assert torch.isfinite(got[0]).all() and torch.isnan(got[1]).all()


@pytest.mark.parametrize("n", [5, 1028])
def test_nan_isolation(n):
    """The conditioning stays a select under the jump's arithmetic: without a jump, NaN in x_t under the kept pixels (a NaN in eps alone is absorbed by the clamp of pred_x0), and in x0 /
    the known noise under the others, changes nothing; with a jump, a NaN reaches exactly the pixels it belongs to."""
    T, J = kc.T_BIG, 10
    for form in ("tensor", "gauss"):
        c = Case(n, T, J, [(501, 510, 1, 0), (501, 999, 0, 2), (506, 999, 1, 0)], form)
        assert [v[3] for v in c.state()] == [True, False, False]
        clean = c.fused()[0]
        kept = c.keep != 0
        assert kept.any() and (~kept).any() and torch.isfinite(clean).all()
        x_t, x0, kz = c.x_t.clone(), c.x0.clone(), c.kz.clone()
        c.x_t[kept] = NAN
        got = c.fused()[0]
        assert torch.isfinite(got).all() and same(got, clean)
        c.x_t.copy_(x_t)
        c.x0[~kept] = NAN
        c.kz[~kept] = NAN
        assert same(c.fused()[0], clean)
        c.x0.copy_(x0)
        c.kz.copy_(kz)
        c.x_t[~kept] = NAN                                                     # outside the mask the NaN stays where it is
        got = c.fused()[0]
        assert torch.isnan(got[~kept]).all() and same(got[kept], clean[kept])
        c.x_t.copy_(x_t)
        c.rz[0, 0] = NAN                                                       # the re-noise reaches the jumping sample only
        got = c.fused()[0]
        assert torch.isnan(got[0, 0]) and same(got[0, 1:], clean[0, 1:]) and same(got[1:], clean[1:])


def test_refused_arguments_launch_nothing():
    """Every refused argument set returns EINVAL with a text and leaves the NaN-poisoned outputs as they were."""
    L = _lib()
    lib = L.lib()
    n = 1028
    c = Case(n, kc.T_SMALL, 2, rc.rows(kc.T_SMALL, 2)[0][:2], "tensor")
    outs = [c.out() for _ in range(3)]

    def structs():
        return c.update_args(c.x_t, *outs, c.z), c.known_args(c.kz, c.full[:3]), c.resample_args()

    def call(a, k, r, seed):
        rc_ = lib.anoddpm_p_sample_update_resample(a, k, r, L.ptr(c.seed) if seed else None, None, 0, L.current_stream())
        torch.cuda.synchronize()
        assert rc_ == L.EINVAL and b"p_sample_update_resample" in lib.anoddpm_last_error()
        assert all(torch.isnan(o).all() for o in outs)
    a, k, r = structs()
    call(None, ctypes.byref(k), ctypes.byref(r), False)
    call(ctypes.byref(a), None, ctypes.byref(r), False)
    call(ctypes.byref(a), ctypes.byref(k), None, False)
    for what, mutate in refused_argument_sets(n):
        a, k, r = structs()
        call(ctypes.byref(a), ctypes.byref(k), ctypes.byref(r), mutate(a, k, r))
    a, k, r = structs()
    L.check(lib.anoddpm_p_sample_update_resample(ctypes.byref(a), ctypes.byref(k), ctypes.byref(r), None, None, 0, L.current_stream()), "resample")
    assert all(torch.isfinite(o).all() for o in outs)


# ------------------------------------------------------------------ the advance launch, alone

def run_advance(tops, J, R, steps, start_t=None):
    """Drive anoddpm_chain_advance_resample `steps` times -> the (t, rep, visit) words after every launch [steps + 1, B, 3]."""
    L = _lib()
    B = len(tops)
    t = torch.tensor([max(v, 0) for v in tops] if start_t is None else start_t, dtype=torch.int64, device=DEV)
    top, rep, visit = i32(tops), i32([R - 1] * B), i32([0] * B)
    jump_w, reps_w, step = i32([J]), i32([R]), i32([0])
    rows = [torch.stack([t.clone(), rep.clone().long(), visit.clone().long()], dim=1)]
    for _ in range(steps):
        L.check(L.lib().anoddpm_chain_advance_resample(L.ptr(t), B, L.ptr(step), L.ptr(jump_w), L.ptr(reps_w), L.ptr(top), L.ptr(rep),
                                                       L.ptr(visit), L.current_stream()), "advance")
        rows.append(torch.stack([t.clone(), rep.clone().long(), visit.clone().long()], dim=1))
    assert int(step) == steps
    assert torch.equal(top, i32(tops)) and int(jump_w) == J and int(reps_w) == R              # read, never written
    return torch.stack(rows).cpu().numpy()


@pytest.mark.parametrize("L_", [1, 5, 13])
def test_advance_follows_the_state_machine(L_):
    for J, R in itertools.product((1, 2, 5), (1, 3)):
        sched = rc.simulate(L_, J, R)
        got = run_advance([L_ - 1], J, R, len(sched) + 2)                      # two launches past the end: t stays floored at 0
        assert np.array_equal(got, rc.state_trace([L_ - 1], J, R, len(sched) + 2)), (L_, J, R)
        assert [int(v) for v in got[:len(sched), 0, 0]] == [ti for ti, _, _ in sched]
        assert [int(v) for v in got[:len(sched), 0, 2]] == [v for _, _, v in sched]
        assert [int(v) for v in got[1:len(sched), 0, 0]] == [land for _, land, _ in sched[:-1]]
        assert (got[len(sched):, 0, 0] == 0).all()


def test_advance_of_a_batch_of_different_tops():
    tops, J, R = [12, 4, 0, 7], 2, 3
    steps = max(len(rc.simulate(top + 1, J, R)) for top in tops)
    got = run_advance(tops, J, R, steps)
    assert np.array_equal(got, rc.state_trace(tops, J, R, steps))
    for b, top in enumerate(tops):
        sched = rc.simulate(top + 1, J, R)
        assert [int(v) for v in got[:len(sched), b, 0]] == [ti for ti, _, _ in sched]
    idle = run_advance([-1, 12], J, R, 9, start_t=[8, 12])                       # an idle slot counts down and never jumps
    assert [int(v) for v in idle[:, 0, 0]] == [8, 7, 6, 5, 4, 3, 2, 1, 0, 0] and (idle[:, 0, 2] == 0).all()
    for J_, R_ in ((0, 2), (2, 0)):                                             # poison words: only the count-down rule
        got = run_advance([6], J_, R_, 8)
        assert [int(v) for v in got[:, 0, 0]] == [6, 5, 4, 3, 2, 1, 0, 0, 0] and (got[:, 0, 2] == 0).all()
