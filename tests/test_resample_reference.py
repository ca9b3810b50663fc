"""CPU: the resampling schedule (Resampling) against the pure-Python simulation of the device state machine, the ABI of
the two entry points, the host refusals, and planted defects in the restatement the GPU tests compare against."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import known_cases as kc
import resample_cases as rc
from test_known_reference import fp32_tables, oracle_tables

F = np.float32
GRID = [(L, J, R) for L in rc.LENGTHS for J in rc.JUMPS for R in rc.REPS]


def _GD():
    import GaussianDiffusion as GD
    return GD


def test_timesteps_equal_the_state_machine():
    GD = _GD()
    for L, J, R in GRID:
        assert GD.Resampling(J, R).timesteps(L) == rc.simulate(L, J, R), (L, J, R)


def test_length_formula():
    GD = _GD()
    for L, J, R in GRID:
        r = GD.Resampling(J, R)
        want = L + ((L - 1) // J) * (R - 1) * J if L >= 1 else 0
        assert r.steps(L) == want == len(r.timesteps(L)) == len(rc.simulate(L, J, R)), (L, J, R)


def test_worked_example():
    r = _GD().Resampling(2, 2)
    assert [ti for ti, _, _ in r.timesteps(5)] == [4, 3, 4, 3, 2, 1, 2, 1, 0] and r.steps(5) == 9
    assert [land for _, land, _ in r.timesteps(5)] == [3, 4, 3, 2, 1, 2, 1, 0, -1]
    assert [v for _, _, v in r.timesteps(5)] == [0, 0, 1, 1, 1, 1, 2, 2, 2]


def test_one_repetition_is_the_plain_chain():
    GD = _GD()
    for L in rc.LENGTHS:
        for J in rc.JUMPS:
            assert GD.Resampling(J, 1).timesteps(L) == [(ti, ti - 1, 0) for ti in range(L - 1, -1, -1)]


def test_schedule_properties():
    """Every (ti, visit) pair is unique -- the domain offset relies on it --, no landing exceeds top, the last landing is -1, and
    every landing but a jump's is ti - 1."""
    GD = _GD()
    for L, J, R in GRID:
        sched = GD.Resampling(J, R).timesteps(L)
        assert len({(ti, v) for ti, _, v in sched}) == len(sched), (L, J, R)
        assert all(land <= L - 1 and ti <= L - 1 for ti, land, _ in sched)
        assert all(land == ti - 1 or (land == ti - 1 + J and (ti - 1) % J == 0) for ti, land, _ in sched)
        if L:
            assert sched[-1][1] == -1 and all(land >= 0 for _, land, _ in sched[:-1])
            assert all(a[1] == b[0] for a, b in zip(sched, sched[1:]))              # a chain: each step starts where the last landed


def test_resampling_is_a_value():
    GD = _GD()
    r = GD.Resampling(3, 2)
    assert r == GD.Resampling(3, 2) and hash(r) == hash(GD.Resampling(3, 2)) and r != GD.Resampling(2, 3) and r != (3, 2)
    assert pickle.loads(pickle.dumps(r)) == r and repr(r) == "Resampling(jump=3, reps=2)"
    with pytest.raises(AttributeError):
        r.jump = 4
    with pytest.raises(AttributeError):
        del r.reps
    for bad in ((0, 1), (1, 0), (-1, 2), (2.0, 2), (2, "2"), (True, 2), (2, None), (2 ** 31, 1)):
        with pytest.raises(ValueError, match="Resampling"):
            GD.Resampling(*bad)
    assert GD.Resampling.parse("10,3") == GD.Resampling(10, 3) == GD.Resampling.parse(" 10 , 3 ")
    for text in ("", "10", "10,3,1", "a,3", "10,0", "2.5,2", "0,2"):
        with pytest.raises(ValueError, match="ANODDPM_RESAMPLE"):
            GD.Resampling.parse(text)


def test_environment_sets_the_attribute(monkeypatch):
    GD = _GD()
    betas = GD.get_beta_schedule(100, "linear")
    assert GD.GaussianDiffusionModel([8, 8], betas).resampling is None and GD.GaussianDiffusionModel.detection_keep is None
    monkeypatch.setenv("ANODDPM_RESAMPLE", "5,2")
    assert GD.GaussianDiffusionModel([8, 8], betas).resampling == GD.Resampling(5, 2)
    monkeypatch.setenv("ANODDPM_RESAMPLE", "5")
    with pytest.raises(ValueError, match="ANODDPM_RESAMPLE"):
        GD.GaussianDiffusionModel([8, 8], betas)


def _owner(seed=None, noise="gauss"):
    GD = _GD()
    d = GD.GaussianDiffusionModel([8, 12], GD.get_beta_schedule(100, "linear"), noise=noise)
    if seed is not None:
        d.seed_gauss(seed)
    return GD, d


def test_host_refusals():
    GD, plain = _owner()
    _, simplex = _owner(noise="simplex")
    x, keep = torch.zeros(1, 1, 8, 12), torch.ones(1, 1, 8, 12)
    known, R = GD.KnownRegion(x, keep), GD.Resampling(2, 2)
    ok = GD.ReverseChain._check_resample_request
    assert ok(plain, "gauss", None, known, R) is R and ok(plain, "gauss", None, None, None) is None
    assert ok(plain, "gauss", GD.StridedSampler(2), known, None) is None
    with pytest.raises(ValueError, match="strided sampler is refused"):
        ok(plain, "gauss", GD.StridedSampler(2), known, R)
    with pytest.raises(ValueError, match="without `known`"):
        ok(plain, "gauss", None, None, R)
    for fn in ("noise_fn", "simplex"):
        with pytest.raises(ValueError, match="simplex"):
            ok(simplex, fn, None, known, R)
    with pytest.raises(TypeError):
        ok(plain, "gauss", None, known, (2, 2))
    with pytest.raises(ValueError, match="requires `keep`"):
        plain.forward_backward(None, x, t_distance=3, resampling=R)
    plain.resampling = R
    with pytest.raises(ValueError, match="detection_keep"):
        plain._detection_conditioning(x)
    plain.resampling = None
    assert plain._detection_conditioning(x) == {}
    plain.detection_keep = torch.ones(8, 12)
    with pytest.raises(ValueError, match="detection_keep"):
        plain._detection_conditioning(x)
    plain.detection_keep = torch.ones(1, 8, 12)
    cond = plain._detection_conditioning(x)
    assert cond["known"].mode == "fixed" and cond["known"].keep.shape == (1, 1, 8, 12) and cond["resampling"] is None


def test_reuse_key_carries_the_resample_tag():
    GD, plain = _owner()
    _, seeded = _owner(5)
    x, keep = torch.zeros(1, 1, 8, 12), torch.ones(1, 1, 8, 12)
    fixed, fresh = GD.KnownRegion(x, keep), GD.KnownRegion(x, keep, "fresh")
    key = GD.ReverseChain._reuse_key_of
    assert key(plain, "gauss", None, fixed) == ("gauss", ("known", "fixed"))                                  # as it was
    assert key(plain, "gauss", None, fixed, GD.Resampling(2, 2)) == ("gauss", ("known", "fixed"), "resample")
    assert key(seeded, "gauss", None, fresh, GD.Resampling(2, 2)) == key(seeded, "gauss", None, fresh, GD.Resampling(7, 1)) \
        == ("gauss", "seeded", ("known", "fresh"), "resample")                                               # (jump, reps) are device words
    assert key(seeded, "gauss", None, fixed, GD.Resampling(2, 2), True) == ("gauss", "seeded", ("known", "fixed"), "resample", "shared")
    assert key(plain, lambda x, t: x, None, fixed, GD.Resampling(2, 2)) is None


def test_shim_exports_the_names():
    import inspect
    GD = _GD()
    from anoddpm_amd import diffusion
    assert GD.Resampling is diffusion.Resampling and "Resampling" in diffusion.__all__
    for fn in (GD.ReverseChain.__init__, GD.ReverseChain.reset, GD.GaussianDiffusionModel.reverse_chain,
               GD.GaussianDiffusionModel.forward_backward, GD.GaussianDiffusionModel._run_chains):
        assert inspect.signature(fn).parameters["resampling"].default is None
    assert inspect.signature(GD.GaussianDiffusionModel._run_chains).parameters["known"].default is None


# ------------------------------------------------------------------ ABI

def test_abi_of_the_resample_entry_points():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 39 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    assert {"anoddpm_p_sample_update_resample", "anoddpm_chain_advance_resample"} <= set(_lib.SYMBOLS)
    assert [n for n, _ in _lib.ResamplingArgs._fields_] == ["jump", "reps", "top", "rep", "visit", "noise", "alphas_cumprod", "noise_stride"]
    assert L.anoddpm_struct_size(b"anoddpm_resampling_args") == ctypes.sizeof(_lib.ResamplingArgs) == 64
    assert _lib.PHILOX_RENOISE == 4 == rc.RENOISE and _lib.PHILOX_KNOWN == rc.KNOWN and _lib.PHILOX_REVERSE == rc.STEP
    assert "4 re-noise of a resampling jump" in open(_lib.HEADER).read()


def refused_argument_sets(n):
    """(what, mutate(a, k, r) -> use a seed?) of every argument set the entry point refuses; a, k, r are valid for the all-planes
    form (no seed) when handed in."""
    def setter(obj, seed=False, **kw):
        def f(a, k, r):
            for name, v in kw.items():
                setattr({"a": a, "k": k, "r": r}[obj], name, v)
            return seed
        return f
    sets = [("null " + f, setter("r", **{f: None})) for f in ("jump", "reps", "top", "rep", "visit", "alphas_cumprod")]
    sets += [("null " + f, setter("k", **{f: None})) for f in ("x0", "keep", "ca", "cb")]
    sets += [("null " + f, setter("a", **{f: None})) for f in ("x_prev", "x_t", "eps", "t", "c_recip", "c_coef1", "c_sigma")]
    sets += [("x0 stride", setter("k", x0_stride=n + 4)), ("keep stride", setter("k", keep_stride=1)),
             ("known noise stride", setter("k", noise_stride=-n)), ("re-noise stride", setter("r", noise_stride=n - 1)),
             ("no known noise and no seed", setter("k", noise=None)), ("no re-noise and no seed", setter("r", noise=None)),
             ("a step-noise tensor together with a seed", setter("a", seed=True)),
             ("bad sizes", setter("a", T=0)), ("B > 65535", setter("a", B=65536))]
    return sets


def test_refused_arguments_without_a_device():
    """Every refusal happens on the host, before anything is launched: EINVAL and a text, with pointers that are never read."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    n, fake = 8, 0x1000

    def valid():
        a, k, r = _lib.PUpdateArgs(), _lib.KnownArgs(), _lib.ResamplingArgs()
        for f in ("x_prev", "x_t", "eps", "noise", "t", "c_recip", "c_recipm1", "c_coef1", "c_coef2", "c_sigma"):
            setattr(a, f, fake)
        a.n, a.B, a.T = n, 2, 8
        k.x0 = k.keep = k.noise = k.ca = k.cb = fake
        k.x0_stride, k.keep_stride, k.noise_stride = n, 0, n
        for f in ("jump", "reps", "top", "rep", "visit", "noise", "alphas_cumprod"):
            setattr(r, f, fake)
        r.noise_stride = 0
        return a, k, r

    def refused(a, k, r, seed):
        assert L.anoddpm_p_sample_update_resample(a, k, r, fake if seed else None, None, 0, None) == _lib.EINVAL
        assert b"p_sample_update_resample" in L.anoddpm_last_error()
    a, k, r = valid()
    refused(None, ctypes.byref(k), ctypes.byref(r), False)
    refused(ctypes.byref(a), None, ctypes.byref(r), False)
    refused(ctypes.byref(a), ctypes.byref(k), None, False)
    sets = refused_argument_sets(n)
    assert len(sets) >= 25
    for what, mutate in sets:
        a, k, r = valid()
        refused(ctypes.byref(a), ctypes.byref(k), ctypes.byref(r), mutate(a, k, r))
    for bad in range(6):
        args = [fake, 2, fake, fake, fake, fake, fake, fake]
        args[0 if bad == 0 else bad + 2] = None
        assert L.anoddpm_chain_advance_resample(*args, None) == _lib.EINVAL and b"chain_advance_resample" in L.anoddpm_last_error()
    assert L.anoddpm_chain_advance_resample(fake, 1025, None, fake, fake, fake, fake, fake, None) == _lib.EINVAL


# ------------------------------------------------------------------ planted defects

def _launch(defect, visit, form):
    """One restated launch at T = 8, J = 2 of a jumping sample (and a non-jumping neighbour) -> x_prev [2, n]."""
    T, J, n = kc.T_SMALL, 2, 37
    tb = fp32_tables(oracle_tables(T))
    x_t, eps, z, x0, kz, rz = rc.inputs(2, n)
    keep = kc.keep_plane("checker", 2, n)
    noise = rc.plane_noise(z, kz, rz) if form == "tensor" else rc.philox_noise([5, 6])
    return rc.resample_step(x_t, eps, x0, keep, (5, 4), tb, T, J, 2, (6, 6), (1, 1), (visit, visit), noise, defect)


@pytest.mark.parametrize("defect", rc.DEFECTS)
def test_planted_defect_is_caught(defect):
    """Each defect changes what the GPU tests compare: the launch's bits (same_bits) or the state trace."""
    GD = _GD()
    if defect in ("rep_never_reset", "jump_above_top"):
        bad = [(L, J, R) for L, J, R in GRID if rc.simulate(L, J, R, defect) != GD.Resampling(J, R).timesteps(L)]
        assert ((5, 2, 2) if defect == "rep_never_reset" else (4, 2, 2)) in bad
        if defect == "jump_above_top":
            assert any(land > 3 for _, land, _ in rc.simulate(4, 2, 2, defect))
        return
    form, visit = ("fresh", 2) if defect == "visit_not_in_domain" else ("tensor", 0)
    good, bad = _launch(None, visit, form), _launch(defect, visit, form)
    assert good[3] == bad[3] == [True, False]
    assert not rc.same_bits(good[0][0], bad[0][0]).all()                       # the jumping sample
    if defect == "visit_not_in_domain":
        assert not rc.same_bits(good[0][1], bad[0][1]).all()                   # the step and known noise of every sample
        assert rc.same_bits(_launch(None, 0, form)[0], _launch(defect, 0, form)[0]).all()      # invisible at visit 0
    else:
        assert rc.same_bits(good[0][1], bad[0][1]).all()


def test_restatement_without_a_jump_is_the_conditioned_step():
    """visit 0, no jump: the bits of known_cases.known_step; a jump re-noises the kept pixels too."""
    T, J, n = kc.T_SMALL, 2, 37
    tb = fp32_tables(oracle_tables(T))
    x_t, eps, z, x0, kz, rz = rc.inputs(3, n)
    keep = kc.keep_plane("random", 3, n)
    row = (5, 4, 0)
    got = rc.resample_step(x_t, eps, x0, keep, row, tb, T, J, 2, (7, 7, 7), (0, 1, 1), (0, 0, 0), rc.plane_noise(z, kz, rz))
    want = kc.known_step(x_t, eps, z, x0, keep, kz, row, tb, T)
    assert got[3] == [False, False, False] and all(rc.same_bits(g, w).all() for g, w in zip(got[:3], want))
    jumped = rc.resample_step(x_t, eps, x0, keep, row, tb, T, J, 2, (7, 7, 7), (1, 1, 1), (0, 0, 0), rc.plane_noise(z, kz, rz))
    assert jumped[3] == [True, False, False]
    A, C = rc.coefficients(tb["acp"], 4, 6)
    assert rc.same_bits(jumped[0][0], A * want[0][0] + C * rz[0]).all() and rc.same_bits(jumped[0][1:], want[0][1:]).all()
    assert abs(float(A) ** 2 + float(C) ** 2 - 1.0) < 1e-6
    for J_, R_ in ((0, 2), (2, 0)):                                            # poison words
        out = rc.resample_step(x_t, eps, x0, keep, row, tb, T, J_, R_, (7, 7, 7), (1, 1, 1), (0, 0, 0), rc.plane_noise(z, kz, rz))
        assert np.isnan(out[0]).all() and out[3] == [False] * 3


def test_rows_cover_what_they_claim():
    for T, J in rc.SCHEDULES:
        rows = rc.rows(T, J)
        flags = [rc.expected_flags(row, T, J) for row in rows]
        assert flags[0] == [True, False, False] and flags[3] == [False, True, False]
        assert flags[1][0] and not flags[1][1] and flags[2][1] and not flags[2][0]
        assert {v for row in rows for _, _, _, v in row} == {0, 2} and {r for row in rows for _, _, r, _ in row} == {0, 1}
        assert any(top == -1 for row in rows for _, top, _, _ in row)
