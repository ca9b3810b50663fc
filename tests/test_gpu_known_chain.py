"""-m gpu: known-region conditioning in the chain plumbing -- eager chains against a host loop of the one-step form and
that against the composition of sample_p / sample_q / torch.where, the all-zero and all-one masks, graph replay and a kept graph
following a new image, mask and noise, the chain cache's keys, and forward_backward(keep=)."""
import pytest
import torch

from test_gpu_detection import DEV, tiny

pytestmark = pytest.mark.gpu

T = 100
SHAPES = [(1, 1, 8, 12), (3, 2, 8, 12)]


def _owner(seed=None, channels=1):
    import GaussianDiffusion as GD
    d = GD.GaussianDiffusionModel([8, 12], GD.get_beta_schedule(T, "linear"), img_channels=channels, noise="gauss")
    if seed is not None:
        d.seed_gauss(seed)
    return GD, d


def _model(x, t):
    return 0.1 * x


def _planes(shape, seed=0, mask_batch=None):
    g = torch.Generator().manual_seed(100 + seed)
    B, C, H, W = shape
    x0 = torch.rand(shape, generator=g) * 2 - 1
    keep = torch.rand((mask_batch or B, 1, H, W), generator=g) > 0.5
    kz = torch.randn(shape, generator=g)
    x_t = torch.randn(shape, generator=g)
    return tuple(a.to(DEV) for a in (x0, keep, kz, x_t))


def _step_noise(shape, seed=0):
    """A denoise_fn (a plain callable: the chain runs eagerly) whose draw depends on t only."""
    def fn(x, t):
        g = torch.Generator().manual_seed(1000 * seed + int(t[0]))
        return torch.randn(shape, generator=g).to(DEV)
    return fn


def _run(chain):
    while chain.remaining:
        chain.step()
    return chain.x


def _tb(B, t):
    return torch.full((B,), t, device=DEV, dtype=torch.int64)


def _visited(GD, dist, S):
    return S.timesteps(dist) if S is not None else list(range(dist - 1, -1, -1))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("stride", [None, 3])
def test_eager_chain_equals_host_loop_equals_composition(shape, stride):
    GD, d = _owner(channels=shape[1])
    S = GD.StridedSampler(stride, 1.0) if stride else None
    dist = 7 if stride else 3
    x0, keep, kz, x_t = _planes(shape)
    fn = _step_noise(shape)
    K = GD.KnownRegion(x0, keep, kz)
    chain = d.reverse_chain(_model, x_t, dist, fn, sampler=S, known=K)
    assert not chain.use_graph and chain.remaining == 3 and chain.reuse_key is None and chain.known_mode == "fixed"
    got = _run(chain).clone()
    loop, comp = x_t, x_t
    B = shape[0]
    kept = K.keep != 0
    assert kept.shape == shape and kept.any() and (~kept).any()
    for t in _visited(GD, dist, S):
        with torch.no_grad():
            out = d.sample_p_known(_model, loop, _tb(B, t), K, fn, sampler=S)
            loop = out["sample"]
            ref = d.sample_p_strided(_model, comp, _tb(B, t), S, fn) if S else d.sample_p(_model, comp, _tb(B, t), fn)
        s = t - (stride or 1)
        kn = d.sample_q(x0, _tb(B, s), kz) if s >= 0 else x0
        assert torch.equal(out["pred_x_0"], ref["pred_x_0"])              # the unconditioned one at every pixel
        comp = torch.where(kept, kn, ref["sample"])
        assert torch.equal(loop, comp), t
    assert torch.equal(got, loop) and torch.equal(got[kept], x0[kept]) and not torch.equal(got, x0)


@pytest.mark.parametrize("stride", [None, 3])
def test_fresh_noise_on_a_seeded_owner_equals_the_streams_values(stride):
    """noise="fresh": step noise (domain 0, step t) and known noise (domain 3, step s) both made in the launch from the chain's
    streams; an unseeded owner handed the same streams' values as tensors gives the same bits."""
    from anoddpm_amd import philox
    shape = SHAPES[1]
    GD, d = _owner(9, channels=2)
    _, plain = _owner(channels=2)
    S = GD.StridedSampler(stride, 1.0) if stride else None
    dist = 7 if stride else 3
    x0, keep, _, x_t = _planes(shape, 1)
    d._take_streams(4)                                                       # the chain draws from streams 4, 5, 6
    chain = d.reverse_chain(_model, x_t, dist, "gauss", sampler=S, known=GD.KnownRegion(x0, keep, "fresh"))
    assert chain.known_mode == "fresh" and chain.k_noise is None and chain.streams.tolist() == [4, 5, 6] and not chain.use_graph
    got = _run(chain).clone()
    x = x_t
    for t in _visited(GD, dist, S):
        s = t - (stride or 1)
        z = philox.normal(9, shape, stream=4, step=t, domain=0, device=DEV)
        kz = philox.normal(9, shape, stream=4, step=max(s, 0), domain=3, device=DEV)
        with torch.no_grad():
            x = plain.sample_p_known(_model, x, _tb(3, t), GD.KnownRegion(x0, keep, kz), lambda xx, tt: z, sampler=S)["sample"]
    assert torch.equal(got, x)
    # the one-step form on the seeded owner draws B fresh stream ids per call, as sample_p does
    before = d.gauss_next_stream
    with torch.no_grad():
        one = d.sample_p_known(_model, x_t, _tb(3, 5), GD.KnownRegion(x0, keep, "fresh"), "gauss", sampler=S)["sample"]
    assert d.gauss_next_stream == before + 3
    s = 5 - (stride or 1)
    z = philox.normal(9, shape, stream=before, step=5, domain=0, device=DEV)
    kz = philox.normal(9, shape, stream=before, step=s, domain=3, device=DEV)
    with torch.no_grad():
        want = plain.sample_p_known(_model, x_t, _tb(3, 5), GD.KnownRegion(x0, keep, kz), lambda xx, tt: z, sampler=S)["sample"]
    assert torch.equal(one, want)
    with pytest.raises(ValueError, match="not seeded"):
        plain.reverse_chain(_model, x_t, dist, "gauss", known=GD.KnownRegion(x0, keep, "fresh"))
    with pytest.raises(ValueError, match="single step"):
        plain.sample_p_known(_model, x_t, _tb(3, 5), GD.KnownRegion(x0, keep), "gauss")


@pytest.mark.parametrize("noise", ["fresh", "tensor"])
def test_all_zero_mask_is_the_unconditioned_chain(noise):
    GD, d = _owner(9, channels=2)
    shape = SHAPES[1]
    x0, keep, kz, x_t = _planes(shape, 2)
    for S in (None, GD.StridedSampler(3, 1.0)):
        K = GD.KnownRegion(x0, torch.zeros_like(keep), "fresh" if noise == "fresh" else kz)
        got = _run(GD.ReverseChain(d, _model, x_t, 7, "gauss", stream_base=11, sampler=S, known=K)).clone()
        want = _run(GD.ReverseChain(d, _model, x_t, 7, "gauss", stream_base=11, sampler=S))
        assert torch.equal(got, want) and torch.isfinite(got).all()


@pytest.mark.parametrize("dist, stride", [(1, None), (4, None), (4, 3), (7, 3)])
def test_all_one_mask_lands_on_x0(dist, stride):
    GD, d = _owner(9, channels=2)
    shape = SHAPES[1]
    x0, keep, kz, x_t = _planes(shape, 3)
    S = GD.StridedSampler(stride, 1.0) if stride else None
    for noise in ("fresh", kz):
        chain = d.reverse_chain(_model, x_t, dist, "gauss", sampler=S, known=GD.KnownRegion(x0, torch.ones_like(keep), noise))
        first = chain.step().clone()
        t = dist - 1 - (stride or 1)
        if t >= 0 and torch.is_tensor(noise):
            assert torch.equal(first, d.sample_q(x0, _tb(3, t), kz))
        assert torch.equal(_run(chain), x0)


def test_fixed_noise_of_a_directly_built_chain_is_one_noise_fn_draw():
    GD, d = _owner()
    shape = SHAPES[0]
    x0, keep, kz, x_t = _planes(shape, 4)
    calls = []

    def noise_fn(x, t):
        calls.append((x.clone(), t.clone()))
        return kz
    d.noise_fn = noise_fn
    fn = _step_noise(shape)
    got = _run(d.reverse_chain(_model, x_t, 3, fn, known=GD.KnownRegion(x0, keep, "fixed"))).clone()
    assert len(calls) == 1 and torch.equal(calls[0][0], x0) and calls[0][1].tolist() == [2]
    assert torch.equal(got, _run(d.reverse_chain(_model, x_t, 3, fn, known=GD.KnownRegion(x0, keep, kz))))


# ------------------------------------------------------------------ graph replay


def _tiny_planes(seed):
    g = torch.Generator().manual_seed(seed)
    shape = (2, 1, 32, 32)
    x0 = (torch.rand(shape, generator=g) * 2 - 1).to(DEV)
    keep = (torch.rand(shape, generator=g) > 0.4).to(DEV)
    kz = torch.randn(shape, generator=g).to(DEV)
    x_t = torch.randn(shape, generator=g).to(DEV)
    return x0, keep, kz, x_t


@pytest.mark.parametrize("noise", ["fixed", "fresh"])
def test_graph_replay_equals_eager_and_a_kept_graph_follows_reset(noise):
    """4 steps on the smallest UNet the sampler tests build, seeded, a mixed mask: use_graph=True == use_graph=False; then reset()
    with another image, mask and noise: the same graph object, the bits of a fresh eager chain."""
    GD, m, d = tiny()
    d.seed_gauss(5)
    x0, keep, kz, x_t = _tiny_planes(1)
    K = GD.KnownRegion(x0, keep, kz if noise == "fixed" else "fresh")
    chain = GD.ReverseChain(d, m, x_t, 4, "gauss", use_graph=True, stream_base=20, known=K)
    assert chain.use_graph and chain.reuse_key == ("gauss", "seeded", ("known", noise))
    got = _run(chain).clone()
    graph = chain.graph
    assert graph is not None and chain._graph_state == 2 and chain.step_idx.item() == 4
    eager = GD.ReverseChain(d, m, x_t, 4, "gauss", use_graph=False, stream_base=20, known=K)
    want = _run(eager)
    assert eager.graph is None and torch.equal(got, want) and torch.isfinite(got).all()
    kept = keep.expand_as(got)
    assert torch.equal(got[kept], x0[kept]) and not torch.equal(got[~kept], x0[~kept])
    x0b, keepb, kzb, x_tb = _tiny_planes(2)
    Kb = GD.KnownRegion(x0b, keepb, kzb if noise == "fixed" else "fresh")
    assert chain.reset(x_tb, 6, stream_base=30, known=Kb) is chain
    again = _run(chain).clone()
    assert chain.graph is graph                                           # no recapture
    fresh = _run(GD.ReverseChain(d, m, x_tb, 6, "gauss", use_graph=False, stream_base=30, known=Kb))
    assert torch.equal(again, fresh) and not torch.equal(again, got)
    # a reset without `known` keeps the planes; another mode, or a chain built without one, is refused
    assert torch.equal(_run(chain.reset(x_tb, 6, stream_base=30)), fresh)
    other = GD.KnownRegion(x0, keep, "fresh" if noise == "fixed" else kz)
    with pytest.raises(ValueError, match="known-region noise"):
        chain.reset(x_t, 4, known=other)
    plain = GD.ReverseChain(d, m, x_t, 4, "gauss", use_graph=False)
    with pytest.raises(ValueError, match="unconditioned chain"):
        plain.reset(x_t, 4, known=K)
    with pytest.raises(ValueError, match="does not fit"):
        chain.reset(x_tb, 6, known=GD.KnownRegion(x0b[:, :, :16], keepb[:, :, :16], "fresh" if noise == "fresh" else kzb[:, :, :16]))


def test_chain_cache_keeps_conditioned_and_unconditioned_graphs_apart():
    GD, m, d = tiny()
    d.seed_gauss(5)
    x0, keep, kz, x_t = _tiny_planes(3)
    K = GD.KnownRegion(x0, keep, kz)
    with torch.no_grad():
        d.seed_gauss(5)
        plain = d._reverse_chain(m, x_t, 4, "gauss", None)
        d.seed_gauss(5)
        cond = d._reverse_chain(m, x_t, 4, "gauss", None, None, K)
        assert sorted(k[3] for k in d._chains) == [("gauss", "seeded"), ("gauss", "seeded", ("known", "fixed"))]
        chains = dict((k[3], c) for k, c in d._chains.items())
        graphs = {k: c.graph for k, c in chains.items()}
        assert all(g is not None for g in graphs.values())
        d.seed_gauss(5)
        assert torch.equal(d._reverse_chain(m, x_t, 4, "gauss", None), plain)
        d.seed_gauss(5)
        assert torch.equal(d._reverse_chain(m, x_t, 4, "gauss", None, None, K), cond)
        d.seed_gauss(5)
        fresh = d._reverse_chain(m, x_t, 4, "gauss", None, None, GD.KnownRegion(x0, keep, "fresh"))
    assert len(d._chains) == 3 and all(chains[k].graph is graphs[k] for k in graphs)
    kept = keep.expand_as(cond)
    assert not torch.equal(plain, cond) and torch.equal(cond[kept], x0[kept]) and torch.equal(fresh[kept], x0[kept])
    assert not torch.equal(plain[kept], x0[kept])
    d.release_chains()


# ------------------------------------------------------------------ forward_backward


@pytest.mark.parametrize("stride", [None, 3])
def test_forward_backward_with_keep(stride):
    """keep=mask in the three forms of see_whole_sequence: kept pixels of the final image are x exactly, and every intermediate
    frame's kept pixels are sample_q(x, s, forward noise) bit for bit -- the forward noise being the draw x was noised with
    ("half", None) or, in the "whole" form that noises gradually, the one more draw made for the known region.  "half" ends on the
    bits of the None form.  "whole" starts its reverse half from a different x_t (gradual noising), so it is compared on the kept
    pixels, which do not depend on it."""
    GD, d = _owner()
    shape = SHAPES[1]
    x, keep, _, _ = _planes(shape, 5, mask_batch=1)
    S = GD.StridedSampler(stride, 1.0) if stride else None
    dist = 7
    kept = keep.expand(shape).cpu()
    draws = []

    def noise_fn(xx, t):
        g = torch.Generator().manual_seed(50 + len(draws))
        draws.append(torch.randn(shape, generator=g).to(DEV))
        return draws[-1]
    d.noise_fn = noise_fn
    results = {}
    for form in (None, "half", "whole"):
        del draws[:]
        torch.manual_seed(21)                                             # the "gauss" step noise of an unseeded owner
        out = d.forward_backward(_model, x, see_whole_sequence=form, t_distance=dist, denoise_fn="gauss", sampler=S, keep=keep)
        assert len(draws) == (dist + 1 if form == "whole" else 1)
        results[form] = (out, draws[-1])
    final, fwd = results[None]
    assert torch.is_tensor(final) and torch.equal(final.cpu()[kept], x.cpu()[kept]) and not torch.equal(final, x)
    steps = _visited(GD, dist, S)
    for form in ("half", "whole"):
        seq, noise = results[form]
        frames = seq[-len(steps):]
        assert len(seq) == (2 if form == "half" else 1 + dist) + len(steps)
        for t, frame in zip(steps, frames):
            s = t - (stride or 1)
            want = d.sample_q(x, _tb(shape[0], s), noise).cpu() if s >= 0 else x.cpu()
            assert torch.equal(frame[kept], want[kept]), (form, t)
        assert torch.equal(seq[-1][kept], final.cpu()[kept])
    assert torch.equal(results["half"][0][-1], final.cpu()) and torch.equal(results["half"][1], fwd)
    # unconditioned calls are what they were, and "fresh" asks for a seeded owner
    torch.manual_seed(21)
    del draws[:]
    plain = d.forward_backward(_model, x, see_whole_sequence=None, t_distance=dist, denoise_fn="gauss", sampler=S)
    assert len(draws) == 1 and not torch.equal(plain.cpu()[kept], x.cpu()[kept])
    with pytest.raises(ValueError, match="not seeded"):
        d.forward_backward(_model, x, see_whole_sequence=None, t_distance=dist, denoise_fn="gauss", keep=keep, known_noise="fresh")
    d.seed_gauss(3)
    d.noise_fn = d._default_noise_fn
    out = d.forward_backward(_model, x, see_whole_sequence=None, t_distance=dist, denoise_fn="gauss", sampler=S, keep=keep,
                             known_noise="fresh")
    assert torch.equal(out.cpu()[kept], x.cpu()[kept]) and torch.isfinite(out).all()
