"""-m gpu: the seeded Gaussian stream on the device -- the fill kernel against the numpy restatement, the fused update /
q-sample kernels against fill + the unfused kernels, and what seeding buys the detection sweeps: results that do not depend on the
slot count, that repeat, and that follow a re-written seed through a kept graph."""
import functools

import numpy as np
import pytest
import torch

import philox_cases as pc
from test_gpu_detection import DEV, tiny

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1025, 37 * 41]          # single partial quad, tail quads, around the 256 * 4 block stride
T = 100
# Per-element bound of the fp32 normals against the fp64 restatement, |d| <= 2 * E * 2^-23 * r with r = sqrt(-2 ln u) of the pair.
# E in ulp: the HIP math-function accuracy table gives 1 ulp each for logf, sqrtf and sincospif; the logarithm's error is halved by
# the square root (0.5), sqrtf adds 1, sincospif 1 (of a value <= 1, scaled by r), the product r * cos one rounding (0.5): 3.  That
# table records maxima observed over tested ranges, not proofs: one further ulp of allowance gives E = 4.  The leading 2 turns ulp
# (between 2^-24 and 2^-23 of the value) into a bound relative to the value.  At the largest radius the stream can produce,
# sqrt(-2 ln 2^-24) = 5.77, this is 5.5e-6 < 1e-5.
E_ULP = 4.0


@functools.lru_cache(maxsize=None)
def ref_bits(seed, stream, step, domain):
    return pc.bits(seed, stream, step, domain, max(SIZES))


@functools.lru_cache(maxsize=None)
def ref_normals(seed, stream, step, domain):
    return pc.normals(seed, stream, step, domain, max(SIZES))


@pytest.mark.parametrize("n", SIZES)
def test_fill_words_equal_restatement_bit_for_bit(n):
    from anoddpm_amd import philox
    for seed in pc.SEEDS:
        for domain in pc.DOMAINS:
            got = philox.bits(seed, (3, n), stream=list(pc.STREAMS), step=list(pc.STEPS), domain=domain, device=DEV)
            got = got.cpu().numpy().view(np.uint32)
            for b in range(3):
                assert np.array_equal(got[b], ref_bits(seed, pc.STREAMS[b], pc.STEPS[b], domain)[:n]), (hex(seed), domain, b)
    # stream0 + b when no per-sample ids are given (wrapping mod 2^32), one step for all
    got = philox.bits(1234, (3, n), stream=2 ** 32 - 1, step=249, domain=1, device=DEV).cpu().numpy().view(np.uint32)
    for b, stream in enumerate((2 ** 32 - 1, 0, 1)):
        assert np.array_equal(got[b], pc.bits(1234, stream, 249, 1, n))


@pytest.mark.parametrize("n", SIZES)
def test_fill_normals_against_fp64_restatement(n):
    from anoddpm_amd import philox
    worst = 0.0
    for seed in pc.SEEDS:
        for domain in pc.DOMAINS:
            got = philox.normal(seed, (3, n), stream=list(pc.STREAMS), step=list(pc.STEPS), domain=domain, device=DEV)
            got = got.cpu().numpy().astype(np.float64)
            for b in range(3):
                z, r = ref_normals(seed, pc.STREAMS[b], pc.STEPS[b], domain)
                bound = 2.0 * E_ULP * 2.0 ** -23 * r[:n]
                err = np.abs(got[b] - z[:n])
                worst = max(worst, float((err / (2.0 ** -23 * r[:n])).max()))
                assert bound.max() <= 1e-5
                assert (err <= bound).all(), (hex(seed), domain, b, float((err / bound).max()))
    print("n = %d: largest |error| = %.3f x 2^-23 r (bound %.0f)" % (n, worst, 2 * E_ULP))


def _seeded():
    import GaussianDiffusion as GD
    d = GD.GaussianDiffusionModel([32, 32], GD.get_beta_schedule(T, "linear"), noise="gauss")
    d.seed_gauss(0x0123456789ABCDEF)
    return d


@pytest.mark.parametrize("shape", [(3, 5), (3, 37, 41), (3, 1, 64, 64)])
@pytest.mark.parametrize("t", [(0, 1, T - 1), (T - 1, -1, 0)])
def test_fused_reverse_update_equals_fill_then_update(shape, t):
    from anoddpm_amd import philox
    d = _seeded()
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(shape, generator=g) * 2 - 1).to(DEV)
    eps = torch.randn(shape, generator=g).to(DEV)
    tt = torch.tensor(t, device=DEV)
    streams = philox.stream_ids(2 ** 32 - 2, 3).to(DEV)                   # wraps: 2^32 - 2, 2^32 - 1, 0
    noise = philox.normal(d._gauss_seed_dev(x.device), shape, stream=streams, step=tt, domain=0, T=T)
    want = [(tt[b].item() % T, (2 ** 32 - 2 + b) % 2 ** 32) for b in range(3)]
    for b, (step, stream) in enumerate(want):                             # the fill's own keying, so the comparison means something
        z = pc.normals(d.gauss_seed, stream, step, 0, 5)[0]
        assert np.abs(noise[b].reshape(-1)[:5].cpu().numpy() - z).max() < 1e-5
    for want_pred, want_mean in ((True, True), (False, False)):
        ref = d._reverse_update(x, tt, eps, noise, want_pred=want_pred, want_mean=want_mean)
        got = d._reverse_update(x, tt, eps, None, want_pred=want_pred, want_mean=want_mean, gauss_streams=streams)
        for r, o in zip(ref, got):
            assert (r is None) == (o is None) and (r is None or torch.equal(r, o))
        assert (got[1] is not None) == want_pred and (got[2] is not None) == want_mean
    xi = x.clone()
    d._reverse_update(xi, tt, eps, None, want_pred=False, out=xi, gauss_streams=streams)        # in place: x_prev aliases x_t
    assert torch.equal(xi, ref[0])


@pytest.mark.parametrize("shape", [(3, 5), (3, 37, 41), (3, 1, 64, 64)])
def test_fused_q_sample_equals_fill_then_q_sample(shape):
    from anoddpm_amd import philox
    d = _seeded()
    g = torch.Generator().manual_seed(4)
    x = (torch.rand(shape, generator=g) * 2 - 1).to(DEV)
    tt = torch.tensor((0, -1, 57), device=DEV)
    noise = philox.normal(d._gauss_seed_dev(x.device), shape, stream=11, step=tt, domain=1, T=T)
    ref = d.sample_q(x, tt, noise)
    out, nz = d._q_sample_gauss(x, tt, 11, want_noise=True)
    assert torch.equal(out, ref) and torch.equal(nz, noise)
    out, nz = d._q_sample_gauss(x, tt, 11)
    assert torch.equal(out, ref) and nz is None
    assert d.gauss_next_stream == 0                                       # explicit streams do not move the allocator


def test_seeded_draws_outside_a_chain_take_fresh_streams():
    from anoddpm_amd import philox
    d = _seeded()
    x = torch.zeros(2, 1, 32, 32, device=DEV)
    t = torch.tensor([5, 9], device=DEV)
    a = d.noise_fn(x, t)                                                  # forward / training noise: domain 1, streams 0, 1
    b = d._denoise_noise(x, t, "gauss")                                   # step noise: domain 0, streams 2, 3
    c = d._denoise_noise(x, t, "random")
    assert d.gauss_next_stream == 6
    assert torch.equal(a, philox.normal(d.gauss_seed, x.shape, stream=0, step=[5, 9], domain=1, device=DEV))
    assert torch.equal(b, philox.normal(d.gauss_seed, x.shape, stream=2, step=[5, 9], domain=0, device=DEV))
    assert torch.equal(c, philox.normal(d.gauss_seed, x.shape, stream=4, step=[5, 9], domain=0, device=DEV))
    sp = d.sample_p(lambda xx, tt: xx, x + 0.1, t, denoise_fn="gauss")["sample"]
    nz = philox.normal(d.gauss_seed, x.shape, stream=6, step=[5, 9], domain=0, device=DEV)
    assert torch.equal(sp, d._reverse_update(x + 0.1, t, x + 0.1, nz)[0])


DISTS = [9, 9, 6, 6, 3, 3, 1, 0, 12]


def _sweep(seed, slots, d=None, m=None):
    """One `_run_chains` sweep of DISTS after seed_gauss(seed) (None: keep seed and allocator), on a fresh tiny model and
    diffusion instance unless one is handed in."""
    if d is None:
        _, m, d = tiny()
    if seed is not None:
        d.seed_gauss(seed)
    torch.manual_seed(3)
    x_0 = torch.rand(1, 1, 32, 32, device=DEV) * 2 - 1
    return d, m, x_0, d._run_chains(m, x_0, DISTS, None, slots=slots)


def test_seeded_sweep_does_not_depend_on_the_slot_count():
    from anoddpm_amd import philox
    d, m, x_0, one = _sweep(5, 1)
    assert d.gauss_next_stream == len(DISTS) and d.last_chain_schedule["slots"] == 1
    _, _, _, four = _sweep(5, 4, d, m)
    assert d.gauss_next_stream == len(DISTS) and d.last_chain_schedule["slots"] == 4
    _, _, _, auto = _sweep(5, None, d, m)
    assert d.last_chain_schedule["slots"] not in (1, 4)
    for other in (four, auto):
        assert torch.allclose(one, other, atol=1e-4, rtol=0), float((one - other).abs().max())
        assert torch.equal(one[7], other[7])                              # the chain without reverse steps
    # every chain against a serial sample_q / sample_p loop on an UNSEEDED instance that is handed the stream's values
    _, _, serial = tiny()
    shape = (1, 1, 32, 32)
    for c, dist in enumerate(DISTS):
        fwd = philox.normal(5, shape, stream=c, step=dist, domain=1, device=DEV)
        x = serial.sample_q(x_0, torch.full((1,), dist, device=DEV, dtype=torch.int64), fwd)
        for t in range(dist - 1, -1, -1):
            tb = torch.full((1,), t, device=DEV, dtype=torch.int64)
            with torch.no_grad():
                x = serial.sample_p(m, x, tb, denoise_fn=lambda xx, tt, t=t: philox.normal(5, shape, stream=c, step=t, domain=0, device=DEV))["sample"]
        for got in (one, four, auto):
            if dist == 0:
                assert torch.equal(got[c:c + 1], x)
            assert torch.allclose(got[c:c + 1], x, atol=1e-4, rtol=0), (c, float((got[c:c + 1] - x).abs().max()))


def test_seeded_sweep_repeats_and_follows_a_new_seed_through_the_kept_graph():
    d, m, _, a = _sweep(5, 4)
    _, _, _, b = _sweep(5, 4)
    _, _, _, c = _sweep(6, 4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    chain = next(iter(d._chains.values()))
    assert len(d._chains) == 1 and chain.use_graph and chain.graph is not None and chain.streams is not None
    again = _sweep(None, 4, d, m)[3]                                      # allocator advanced: other streams
    assert d.gauss_next_stream == 2 * len(DISTS) and not torch.equal(again, a)
    reseeded = _sweep(6, 4, d, m)[3]                                      # same chain object, same captured graph
    assert next(iter(d._chains.values())) is chain and torch.equal(reseeded, c)


def test_seeded_detection_leaves_torchs_generator_alone():
    GD, m, d = tiny()
    torch.manual_seed(1)
    x_0 = torch.rand(1, 1, 32, 32, device=DEV) * 2 - 1
    mask = (torch.rand(1, 1, 32, 32, device=DEV) > 0.7).float()
    args = {"arg_num": 9, "T": 100, "img_size": [32, 32]}
    before = torch.cuda.get_rng_state(DEV)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert not torch.equal(before, torch.cuda.get_rng_state(DEV))         # unseeded: torch.randn_like draws
    plain = d.last_detection
    d.seed_gauss(5)
    before = torch.cuda.get_rng_state(DEV)
    assert d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2) == [None]
    assert torch.equal(before, torch.cuda.get_rng_state(DEV))
    assert d.gauss_next_stream == 2
    seeded_chains = [ch for ch in d._chains.values() if ch.streams is not None]
    assert len(seeded_chains) == 1 and seeded_chains[0].noise is None and seeded_chains[0].use_graph
    assert len(d.last_detection) == len(plain)
    for rec, ref in zip(d.last_detection, plain):
        assert rec.keys() == ref.keys()
        for k in rec:
            if torch.is_tensor(ref[k]):
                assert rec[k].shape == ref[k].shape and rec[k].dtype == ref[k].dtype, k
        assert torch.isfinite(rec["output"]).all() and not torch.equal(rec["output"], ref["output"])
    first = d.last_detection[0]["output"].clone()
    d.seed_gauss(5)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert torch.equal(d.last_detection[0]["output"], first)


def test_seeded_forward_backward_eager_equals_graph(monkeypatch):
    outs = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("ANODDPM_NO_GRAPH", no_graph)
        GD, m, d = tiny()
        d.seed_gauss(5)
        torch.manual_seed(11)
        x = torch.rand(2, 1, 32, 32, device=DEV) * 2 - 1
        outs.append(d.forward_backward(m, x, see_whole_sequence=None, t_distance=6, denoise_fn="gauss"))
        assert d.gauss_next_stream == 4                                   # 2 forward-noise streams + 2 chain streams
        assert bool(d.__dict__.get("_chains")) == (no_graph == "0")
    assert torch.equal(outs[0], outs[1])
