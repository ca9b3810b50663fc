"""CPU: known-region conditioning -- the numpy restatement of tests/known_cases.py against the oracle's q-sample and
reverse update joined by numpy.where, planted defects against the comparison the GPU tests use, the C ABI of the new entry point and
the host logic (KnownRegion, the reuse-key tag, the shim export)."""
import ctypes

import numpy as np
import pytest
import torch

import known_cases as kc
import philox_cases as pc
import sampler_cases as sc
from oracle import diffusion_oracle as do

F = np.float32


def oracle_tables(T):
    return do.tables(do.beta_schedule(T, "cosine" if T == kc.T_SMALL else "linear"))


def fp32_tables(tbo):
    """The device tables: the fp64 tables rounded to fp32, sigma by the reference's fp32 torch expression."""
    names = {"recip": "sqrt_recip_alphas_cumprod", "recipm1": "sqrt_recipm1_alphas_cumprod", "coef1": "posterior_mean_coef1",
             "coef2": "posterior_mean_coef2", "ca": "sqrt_alphas_cumprod", "cb": "sqrt_one_minus_alphas_cumprod"}
    tb = {k: np.asarray(tbo[v], dtype=np.float64).astype(F) for k, v in names.items()}
    tb["sigma"] = torch.exp(0.5 * torch.from_numpy(tbo["model_log_variance"]).float()).numpy()
    tb["acp"] = np.asarray(tbo["alphas_cumprod"], dtype=np.float64)
    return tb


def in_range_rows(B, T):
    return [row for row in kc.t_rows(B, T) if all(kc.normalise(t, T)[1] for t in row)]


@pytest.mark.parametrize("T", [kc.T_SMALL, kc.T_BIG])
def test_restatement_equals_the_oracle_composition(T):
    """known_step == numpy.where(keep, oracle q_sample at s (x0 itself for s < 0), oracle p_sample_update), bit for bit, and its
    pred_x0 is the oracle's.  The oracle indexes its tables like the reference and cannot state an out-of-range t: those rows are
    checked to be NaN."""
    tbo = oracle_tables(T)
    tb = fp32_tables(tbo)
    checked = 0
    for B in kc.BATCHES:
        for n in kc.NS[:4] + (37,):
            x_t, eps, z, x0, kz = kc.inputs(B, n)
            for row in in_range_rows(B, T):
                for mask in kc.MASKS:
                    keep = kc.keep_plane(mask, B, n)
                    got, pred, _ = kc.known_step(x_t, eps, z, x0, keep, kz, row, tb, T)
                    t = torch.tensor(row)
                    u, want_pred = do.p_sample_update(tbo, torch.from_numpy(x_t), t, torch.from_numpy(eps), torch.from_numpy(z))
                    s = torch.tensor([kc.landing(v, T)[0] for v in row])
                    kn = do.q_sample(tbo, torch.from_numpy(x0), s.clamp(min=0), torch.from_numpy(kz)).numpy()
                    kn = np.where((s < 0).numpy()[:, None], x0, kn)
                    want = np.where(keep != 0, kn, u.numpy())
                    assert kc.same_bits(got, want).all(), (B, n, row, mask)
                    assert kc.same_bits(pred, want_pred.numpy()).all()
                    checked += 1
    assert checked >= 100
    x_t, eps, z, x0, kz = kc.inputs(3, 5)
    for sampler in (None, (3, 1.0), (0, 1.0)):
        row = (-T - 1, T, 1)
        got = kc.known_step(x_t, eps, z, x0, kc.keep_plane("checker", 3, 5), kz, row, tb, T, sampler)[0]
        assert np.isnan(got[:2]).all() and np.isnan(got[2]).all() == (sampler == (0, 1.0))


def test_strided_restatement_is_within_the_fp64_bound():
    """The fp32 strided `u` of known_cases.update against the fp64 restatement of sampler_cases, inside its derived bound."""
    T = sc.T
    acp = sc.alphas_cumprod()
    recip, recipm1 = sc.recip_tables(acp, F)
    tb = {"recip": recip, "recipm1": recipm1, "acp": acp}
    x_t, eps, z, _, _ = kc.inputs(1, 301)
    for t in (0, 4, 57, T - 1):
        for stride, eta in ((1, 1.0), (5, 0.5), (T + 3, 1.0), (3, 0.0)):
            r = sc.step(x_t[0], eps[0], z[0], t, stride, eta, acp, recip, recipm1)
            got, pred, mean = kc.update(x_t[0], eps[0], z[0], t, tb, T, (stride, eta))
            assert (np.abs(got.astype(np.float64) - r["x_prev"]) <= sc.error_bound(r)).all(), (t, stride, eta)
            assert (np.abs(mean.astype(np.float64) - r["mean"]) <= sc.error_bound(r)).all()


# ------------------------------------------------------------------ planted defects


def _defect(kind, x_t, eps, z, x0, keep, kz, row, tb, T):
    """known_step with one planted defect."""
    B, n = x_t.shape
    out = np.empty((B, n), dtype=F)
    for b in range(B):
        u = kc.update(x_t[b], eps[b], z[b], row[b], tb, T)[0]
        s, _ = kc.landing(row[b], T)
        k = keep[0 if kind == "keep_stride" else b]
        if kind == "s_is_t":
            s += 1
        if s < 0 and kind != "x0_inexact":
            kn = x0[b]
        else:
            kn = tb["ca"][max(s, 0)] * x0[b] + tb["cb"][max(s, 0)] * kz[b]
        if kind == "blend":
            m = (k != 0).astype(F)
            with np.errstate(invalid="ignore"):
                out[b] = m * kn + (F(1.0) - m) * u
        else:
            out[b] = np.where(k != 0, kn, u)
    return out


@pytest.mark.parametrize("kind", ["blend", "s_is_t", "x0_inexact", "keep_stride"])
def test_planted_defect_is_caught(kind):
    T = kc.T_SMALL
    tb = fp32_tables(oracle_tables(T))
    B, n = 3, 37
    x_t, eps, z, x0, kz = kc.inputs(B, n)
    keep = kc.keep_plane("random", B, n)
    row = (0, 1, T - 1)
    if kind == "blend":
        eps = eps.copy()
        eps[keep != 0] = np.nan                                   # NaN in `u` under the kept pixels: a select never sees it
    want = kc.known_step(x_t, eps, z, x0, keep, kz, row, tb, T)[0]
    assert np.isfinite(want[keep != 0]).all()
    assert kc.same_bits(_defect(None, x_t, eps, z, x0, keep, kz, row, tb, T), want).all()          # the harness itself is sound
    bad = _defect(kind, x_t, eps, z, x0, keep, kz, row, tb, T)
    miss = ~kc.same_bits(bad, want)
    assert miss.any()
    if kind == "x0_inexact":
        assert miss[0].any() and not miss[1:].any()               # only the sample that lands below t = 0
    if kind == "s_is_t":
        assert miss[1].any() and miss[2].any()


def test_planted_domain_reuse_is_caught():
    """Known-region noise drawn from domain 0 -- the step noise's own counter block at step s -- instead of domain 3."""
    T = kc.T_SMALL
    tb = fp32_tables(oracle_tables(T))
    B, n = 3, 37
    x_t, eps, z, x0, _ = kc.inputs(B, n)
    keep = kc.keep_plane("checker", B, n)
    row = (2, 1, T - 1)

    def fill(domain):
        return np.stack([pc.normals(kc.SEED, 5 + b, kc.landing(row[b], T)[0], domain, n)[0].astype(F) for b in range(B)])
    want = kc.known_step(x_t, eps, z, x0, keep, fill(3), row, tb, T)[0]
    bad = kc.known_step(x_t, eps, z, x0, keep, fill(0), row, tb, T)[0]
    miss = ~kc.same_bits(bad, want)
    assert miss[keep != 0].all() and not miss[keep == 0].any()


# ------------------------------------------------------------------ ABI


def test_abi_of_the_known_entry_point():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION >= 38 and L.anoddpm_abi_version() == _lib.ABI_VERSION
    assert L.anoddpm_struct_size(b"anoddpm_known_args") == ctypes.sizeof(_lib.KnownArgs) == 8 * 8
    assert [n for n, _ in _lib.KnownArgs._fields_] == ["x0", "keep", "noise", "ca", "cb", "x0_stride", "keep_stride", "noise_stride"]
    assert [t for _, t in _lib.KnownArgs._fields_] == [ctypes.c_void_p] * 5 + [ctypes.c_int64] * 3
    _, params = _lib._PROTOS["anoddpm_p_sample_update_known"]                  # from the header
    assert [p[0] for p in params] == ["a", "k", "alphas_cumprod", "stride", "eta", "seed", "streams", "stream0", "stream"]
    assert L.anoddpm_p_sample_update_known.argtypes == [ctypes.POINTER(_lib.PUpdateArgs), ctypes.POINTER(_lib.KnownArgs)] + \
        [ctypes.c_void_p] * 5 + [ctypes.c_uint32, ctypes.c_void_p]
    assert _lib.PHILOX_KNOWN == 3 and "3 known-region noise" in open(_lib.HEADER).read()


def refused_argument_sets(a, k, n):
    """(what, mutate(a, k) -> the five optional pointers (alphas_cumprod, stride, eta, seed) as a dict) of every argument set the
    entry point refuses; `a` and `k` are valid for the ancestral tensor form when handed in."""
    fake = 0x1000

    def setter(obj, **kw):
        def f(a, k):
            for name, v in kw.items():
                setattr(a if obj == "a" else k, name, v)
            return {}
        return f
    return [
        ("null x0", setter("k", x0=None)), ("null keep", setter("k", keep=None)), ("null ca", setter("k", ca=None)),
        ("null cb", setter("k", cb=None)),
        ("x0 stride", setter("k", x0_stride=n + 4)), ("keep stride", setter("k", keep_stride=1)),
        ("noise stride", setter("k", noise_stride=-n)),
        ("partial strided block: no eta", lambda a, k: {"alphas_cumprod": fake, "stride": fake}),
        ("partial strided block: only eta", lambda a, k: {"eta": fake}),
        ("no known noise and no seed", setter("k", noise=None)),
        ("a noise tensor together with a seed", lambda a, k: {"seed": fake}),
    ]


def test_refused_arguments_without_a_device():
    """Every refusal happens on the host, before anything is launched: EINVAL and a last_error text, with pointers that are never
    read (the GPU test repeats this with real buffers and checks that they stay untouched)."""
    from anoddpm_amd import _lib
    L = _lib.lib()
    n = 8

    def valid():
        a, k = _lib.PUpdateArgs(), _lib.KnownArgs()
        for f in ("x_prev", "x_t", "eps", "noise", "t", "c_recip", "c_recipm1", "c_coef1", "c_coef2", "c_sigma"):
            setattr(a, f, 0x1000)
        a.n, a.B, a.T = n, 2, 8
        k.x0 = k.keep = k.noise = k.ca = k.cb = 0x1000
        k.x0_stride, k.keep_stride, k.noise_stride = n, 0, n
        return a, k
    a, k = valid()
    assert L.anoddpm_p_sample_update_known(ctypes.byref(a), None, None, None, None, None, None, 0, None) == _lib.EINVAL
    assert b"p_sample_update_known" in L.anoddpm_last_error()
    assert L.anoddpm_p_sample_update_known(None, ctypes.byref(k), None, None, None, None, None, 0, None) == _lib.EINVAL
    for what, mutate in refused_argument_sets(a, k, n):
        a, k = valid()
        opt = mutate(a, k)
        rc = L.anoddpm_p_sample_update_known(ctypes.byref(a), ctypes.byref(k), opt.get("alphas_cumprod"), opt.get("stride"),
                                             opt.get("eta"), opt.get("seed"), None, 0, None)
        assert rc == _lib.EINVAL and b"p_sample_update_known" in L.anoddpm_last_error(), what


# ------------------------------------------------------------------ host logic


def _owner(seed=None, noise="gauss"):
    import GaussianDiffusion as GD
    d = GD.GaussianDiffusionModel([8, 12], GD.get_beta_schedule(100, "linear"), noise=noise)
    if seed is not None:
        d.seed_gauss(seed)
    return GD, d


def test_known_region_validation():
    GD, d = _owner()
    x = torch.linspace(-1, 1, 2 * 2 * 8 * 12).reshape(2, 2, 8, 12).double()
    keep = torch.zeros(1, 1, 8, 12)
    keep[..., 3:, :5] = -2.5
    k = GD.KnownRegion(x, keep)
    assert k.mode == "fixed" and k.x_0.dtype == torch.float32 and k.x_0.is_contiguous()
    assert k.keep.dtype == torch.uint8 and k.keep.shape == (1, 2, 8, 12) and k.keep.is_contiguous()       # broadcast over channels
    assert torch.equal(k.keep[0, 0], (keep[0, 0] != 0).to(torch.uint8)) and torch.equal(k.keep[0, 0], k.keep[0, 1])
    assert GD.KnownRegion(x, keep.bool(), "fresh").mode == "fresh"
    z = torch.zeros(2, 2, 8, 12, dtype=torch.float64)
    assert GD.KnownRegion(x, keep, z).mode == "fixed" and GD.KnownRegion(x, keep, z).noise.dtype == torch.float32
    with pytest.raises(AttributeError):
        k.noise = "fresh"
    for bad_x, bad_keep, bad_noise in ((x[0], keep, "fixed"), (x.long(), keep, "fixed"), (x, keep[0], "fixed"),
                                       (x, torch.zeros(1, 1, 8, 11), "fixed"), (x, torch.zeros(1, 3, 8, 12), "fixed"),
                                       (x, keep, "sometimes"), (x, keep, None), (x, keep, torch.zeros(2, 1, 8, 12))):
        with pytest.raises(ValueError, match="KnownRegion"):
            GD.KnownRegion(bad_x, bad_keep, bad_noise)
    k.check_batch((2, 2, 8, 12))
    GD.KnownRegion(x[:1], keep, z[:1]).check_batch((5, 2, 8, 12))
    for shape in ((3, 2, 8, 12), (2, 1, 8, 12), (2, 2, 8, 13)):
        with pytest.raises(ValueError, match="does not fit"):
            k.check_batch(shape)
    with pytest.raises(TypeError):
        GD.ReverseChain._known_mode_of(d, "gauss", "fixed")


def test_fresh_noise_needs_a_seeded_gaussian_owner():
    GD, plain = _owner()
    _, seeded = _owner(5)
    _, simplex = _owner(5, noise="simplex")
    x, keep = torch.zeros(1, 1, 8, 12), torch.ones(1, 1, 8, 12)
    fresh, fixed = GD.KnownRegion(x, keep, "fresh"), GD.KnownRegion(x, keep)
    mode = GD.ReverseChain._known_mode_of
    assert mode(seeded, "gauss", fresh) == "fresh" and mode(seeded, "noise_fn", fresh) == "fresh"
    assert mode(plain, "gauss", fixed) == mode(simplex, "noise_fn", fixed) == "fixed" and mode(plain, "gauss", None) is None
    with pytest.raises(ValueError, match="not seeded"):
        mode(plain, "gauss", fresh)
    with pytest.raises(ValueError, match="simplex"):
        mode(simplex, "noise_fn", fresh)
    with pytest.raises(ValueError, match="simplex"):
        mode(simplex, "simplex", fresh)
    with pytest.raises(ValueError, match="not seeded"):
        mode(seeded, lambda x, t: torch.zeros_like(x), fresh)


def test_reuse_key_carries_the_known_tag():
    GD, plain = _owner()
    _, seeded = _owner(5)
    x, keep = torch.zeros(1, 1, 8, 12), torch.ones(1, 1, 8, 12)
    fresh, fixed, tensor = GD.KnownRegion(x, keep, "fresh"), GD.KnownRegion(x, keep), GD.KnownRegion(x, keep, torch.zeros_like(x))
    key = GD.ReverseChain._reuse_key_of
    S = GD.StridedSampler(3)
    assert key(plain, "gauss") == ("gauss",) and key(plain, "gauss", S) == ("gauss", "strided")              # as they were
    assert key(plain, "gauss", None, fixed) == ("gauss", ("known", "fixed")) == key(plain, "gauss", None, tensor)
    assert key(seeded, "gauss", S, fresh) == ("gauss", "seeded", "strided", ("known", "fresh"))
    assert key(seeded, "gauss", S, fixed) == ("gauss", "seeded", "strided", ("known", "fixed"))
    assert key(plain, lambda x, t: x, None, fixed) is None                                                    # never kept
    keys = {key(seeded, "gauss", s, k) for s in (None, S) for k in (None, fixed, fresh)}
    assert len(keys) == 6


def test_shim_exports_the_names():
    import GaussianDiffusion as GD
    from anoddpm_amd import diffusion
    assert GD.KnownRegion is diffusion.KnownRegion and "KnownRegion" in diffusion.__all__
    assert hasattr(GD.GaussianDiffusionModel, "sample_p_known")
    import inspect
    assert "known" in inspect.signature(GD.ReverseChain.__init__).parameters
    assert "known" in inspect.signature(GD.ReverseChain.reset).parameters
    assert "known" in inspect.signature(GD.GaussianDiffusionModel.reverse_chain).parameters
    fb = inspect.signature(GD.GaussianDiffusionModel.forward_backward).parameters
    assert fb["keep"].default is None and fb["known_noise"].default == "fixed"
