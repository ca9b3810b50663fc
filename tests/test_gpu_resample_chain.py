"""-m gpu: resampling jumps in the chain plumbing, on the small UNet the known-chain test uses (32^2, base 32): the
device-driven timestep trace, graph replay against eager, a kept graph following reset(), Resampling(j, 1) against the plain
conditioned chain, an unseeded owner, the chain cache's keys, the slot-batched sweep against chains run alone, and the detection
routines' two opt-in attributes."""
import pytest
import torch

from test_gpu_detection import DEV, tiny

pytestmark = pytest.mark.gpu

_TINY = []


def shared():
    """One model for the file; a fresh diffusion owner per test (they carry the seeds, the chain cache and the attributes)."""
    if not _TINY:
        _TINY.append(tiny())
    GD, m, _ = _TINY[0]
    return GD, m, GD.GaussianDiffusionModel([32, 32], GD.get_beta_schedule(100, "linear"), noise="gauss")


def planes(seed, B=2):
    g = torch.Generator().manual_seed(seed)
    shape = (B, 1, 32, 32)
    x0 = (torch.rand(shape, generator=g) * 2 - 1).to(DEV)
    keep = (torch.rand(shape, generator=g) > 0.4).to(DEV)
    kz = torch.randn(shape, generator=g).to(DEV)
    x_t = torch.randn(shape, generator=g).to(DEV)
    return x0, keep, kz, x_t


def run(chain):
    while chain.remaining:
        chain.step()
    return chain.x


@pytest.mark.parametrize("L,J,R", [(5, 2, 2), (5, 7, 3), (6, 1, 2)])
def test_device_timestep_trace_is_the_schedule(L, J, R):
    """t, visit and rep are read back before every step of an eager chain: the device decides every jump."""
    GD, m, d = shared()
    d.seed_gauss(5)
    x0, keep, kz, x_t = planes(1)
    res = GD.Resampling(J, R)
    chain = GD.ReverseChain(d, m, x_t, L, "gauss", use_graph=False, stream_base=20, known=GD.KnownRegion(x0, keep, kz), resampling=res)
    sched = res.timesteps(L)
    assert chain.remaining == len(sched) == res.steps(L) and chain.rs_top.tolist() == [L - 1] * 2
    assert (chain.rs_jump.item(), chain.rs_reps.item()) == (J, R)
    trace = []
    while chain.remaining:
        trace.append((chain.t.tolist(), chain.rs_visit.tolist()))
        chain.step()
    assert [(t[0], v[0]) for t, v in trace] == [(ti, v) for ti, _, v in sched] and all(t[0] == t[1] and v[0] == v[1] for t, v in trace)
    assert chain.t.tolist() == [0, 0] and chain.step_idx.item() == len(sched)
    if J > L - 1:
        assert [ti for ti, _, _ in sched] == list(range(L - 1, -1, -1)) and chain.rs_visit.tolist() == [0, 0]
    kept = keep.expand_as(chain.x)
    assert torch.equal(chain.x[kept], x0[kept]) and torch.isfinite(chain.x).all()


@pytest.mark.parametrize("noise", ["fixed", "fresh"])
def test_graph_replay_equals_eager_and_a_kept_graph_follows_reset(noise):
    GD, m, d = shared()
    d.seed_gauss(5)
    x0, keep, kz, x_t = planes(1)
    K = GD.KnownRegion(x0, keep, kz if noise == "fixed" else "fresh")
    res = GD.Resampling(2, 2)
    chain = GD.ReverseChain(d, m, x_t, 5, "gauss", use_graph=True, stream_base=20, known=K, resampling=res)
    assert chain.use_graph and chain.reuse_key == ("gauss", "seeded", ("known", noise), "resample")
    got = run(chain).clone()
    graph = chain.graph
    assert graph is not None and chain._graph_state == 2 and chain.step_idx.item() == 9
    eager = GD.ReverseChain(d, m, x_t, 5, "gauss", use_graph=False, stream_base=20, known=K, resampling=res)
    want = run(eager)
    assert eager.graph is None and torch.equal(got, want) and torch.isfinite(got).all()
    kept = keep.expand_as(got)
    assert torch.equal(got[kept], x0[kept]) and not torch.equal(got[~kept], x0[~kept])
    plain = run(GD.ReverseChain(d, m, x_t, 5, "gauss", use_graph=False, stream_base=20, known=K))
    assert not torch.equal(plain[~kept], got[~kept])                       # the jumps change the generated region
    # another image, mask, noise and (jump, reps): the same graph object, the bits of a fresh eager chain
    x0b, keepb, kzb, x_tb = planes(2)
    Kb = GD.KnownRegion(x0b, keepb, kzb if noise == "fixed" else "fresh")
    resb = GD.Resampling(3, 3)
    assert chain.reset(x_tb, 7, stream_base=30, known=Kb, resampling=resb) is chain and chain.remaining == resb.steps(7) == 19
    again = run(chain).clone()
    assert chain.graph is graph
    fresh = run(GD.ReverseChain(d, m, x_tb, 7, "gauss", use_graph=False, stream_base=30, known=Kb, resampling=resb))
    assert torch.equal(again, fresh) and not torch.equal(again, got)
    assert torch.equal(run(chain.reset(x_tb, 7, stream_base=30)), fresh)     # None keeps planes and schedule
    with pytest.raises(ValueError, match="without resampling"):
        GD.ReverseChain(d, m, x_t, 4, "gauss", use_graph=False, known=K).reset(x_t, 4, resampling=res)
    with pytest.raises(ValueError, match="strided sampler is refused"):
        GD.ReverseChain(d, m, x_t, 4, "gauss", use_graph=False, known=K, resampling=res, sampler=GD.StridedSampler(2))
    with pytest.raises(ValueError, match="without `known`"):
        d.reverse_chain(m, x_t, 4, resampling=res)


def test_one_repetition_gives_the_bits_of_the_plain_conditioned_chain():
    GD, m, d = shared()
    d.seed_gauss(7)
    x0, keep, kz, x_t = planes(3)
    for noise in (kz, "fresh"):
        K = GD.KnownRegion(x0, keep, noise)
        plain = run(GD.ReverseChain(d, m, x_t, 6, "gauss", use_graph=False, stream_base=11, known=K)).clone()
        for J in (1, 2, 9):
            chain = GD.ReverseChain(d, m, x_t, 6, "gauss", use_graph=False, stream_base=11, known=K, resampling=GD.Resampling(J, 1))
            assert chain.remaining == 6 and chain.rs_top is not None             # the new launches
            assert torch.equal(run(chain), plain), (J, noise if isinstance(noise, str) else "tensor")


def test_unseeded_owner_runs_on_three_planes_per_step(monkeypatch):
    """No seed: step noise, fixed known noise and a re-noise plane drawn per step; under the all-ones mask the chain returns the
    input image, and the re-noise draw is the one more torch.randn_like per step."""
    GD, m, d = shared()
    x0, _, kz, x_t = planes(4)
    K = GD.KnownRegion(x0, torch.ones(1, 1, 32, 32), kz)
    res = GD.Resampling(2, 2)
    calls = []
    real = torch.randn_like
    monkeypatch.setattr(torch, "randn_like", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    chain = GD.ReverseChain(d, m, x_t, 5, "gauss", use_graph=False, known=K, resampling=res)
    assert chain.streams is None and chain.k_noise is not None and chain.remaining == 9
    got = run(chain)
    assert len(calls) == 2 * 9 and torch.equal(got, x0)
    monkeypatch.undo()
    mixed = GD.KnownRegion(x0, planes(4)[1], kz)
    kept = mixed.keep != 0
    for use_graph in (False, True):                                           # torch's generator is registered with the capture
        chain = GD.ReverseChain(d, m, x_t, 5, "gauss", use_graph=use_graph, known=mixed, resampling=res)
        got = run(chain)
        assert chain.step_idx.item() == 9 and torch.isfinite(got).all() and torch.equal(got[kept], x0[kept])
        assert not torch.equal(got[~kept], x0[~kept])


def test_chain_cache_keeps_resampled_and_plain_conditioned_graphs_apart():
    GD, m, d = shared()
    x0, keep, kz, x_t = planes(3)
    K = GD.KnownRegion(x0, keep, kz)
    res = GD.Resampling(2, 2)
    with torch.no_grad():
        d.seed_gauss(5)
        cond = d._reverse_chain(m, x_t, 5, "gauss", None, None, K)
        d.seed_gauss(5)
        jumped = d._reverse_chain(m, x_t, 5, "gauss", None, None, K, res)
        assert sorted(k[3] for k in d._chains) == [("gauss", "seeded", ("known", "fixed")), ("gauss", "seeded", ("known", "fixed"), "resample")]
        graphs = {k[3]: c.graph for k, c in d._chains.items()}
        assert all(g is not None for g in graphs.values())
        d.seed_gauss(5)
        assert torch.equal(d._reverse_chain(m, x_t, 5, "gauss", None, None, K), cond)
        d.seed_gauss(5)
        assert torch.equal(d._reverse_chain(m, x_t, 5, "gauss", None, None, K, GD.Resampling(2, 2)), jumped)
        seq = [x_t.cpu()]
        d.seed_gauss(5)
        d._reverse_chain(m, x_t, 5, "gauss", seq, None, K, GD.Resampling(4, 3))      # the kept graph, other words
    assert len(seq) == 1 + GD.Resampling(4, 3).steps(5) and len(d._chains) == 2
    assert all(c.graph is graphs[k[3]] for k, c in d._chains.items()) and not torch.equal(cond, jumped)
    d.release_chains()


# ------------------------------------------------------------------ the slot-batched sweep

LENS = [0, 1, 3, 4, 6]


def test_sweep_equals_chains_run_alone():
    """Lengths {0, 1, 3, 4, 6} on 2 slots (the longest chain takes 10 evaluations; refills happen mid-run): every chain equals
    the same chain run alone through ReverseChain on its stream id, at the bar of test_mixed_length_chains_on_slots_equal_serial_chains
    (the kernels' batch-dependent choice; these chains are no longer than that test's)."""
    GD, m, d = shared()
    res = GD.Resampling(2, 2)
    x0, keep, _, _ = planes(6, B=1)
    K = GD.KnownRegion(x0, keep, "fixed")
    for seed in (5, 6):                                                     # the second sweep replays the kept slot chain's graph
        d.seed_gauss(seed)
        d._take_streams(3)
        base = d.gauss_next_stream
        out = d._run_chains(m, x0, LENS, None, slots=2, known=K, resampling=res)
        sched = d.last_chain_schedule
        assert sched["slots"] == 2 and sched["chain_steps"] == sum(res.steps(l) for l in LENS) == 22 and max(map(res.steps, LENS)) == 10
        assert sched["steps"] >= 11 and out.shape == (5, 1, 32, 32) and torch.isfinite(out).all()
        assert d.gauss_next_stream == base + len(LENS)
        t_all = torch.tensor(LENS, device=DEV)
        x_start, fwd = d._q_sample_gauss(x0.repeat(len(LENS), 1, 1, 1), t_all, base, want_noise=True)
        kept = keep[0]
        for c, L in enumerate(LENS):
            if L == 0:
                assert torch.equal(out[c], x_start[c])
                continue
            alone = run(GD.ReverseChain(d, m, x_start[c:c + 1], L, "gauss", use_graph=False, stream_base=base + c,
                                        known=GD.KnownRegion(x0, keep, fwd[c:c + 1]), resampling=res))
            assert torch.allclose(out[c:c + 1], alone, atol=1e-4, rtol=0), (c, float((out[c:c + 1] - alone).abs().max()))
            assert torch.equal(out[c][kept], x0[0][kept])
    slot_keys = [k[3] for k, ch in d._chains.items() if getattr(ch, "slot_chain", False)]
    assert slot_keys == [("gauss", "seeded", ("known", "fixed"), "resample", "shared")]
    with pytest.raises(ValueError, match="strided sampler is refused"):
        d._run_chains(m, x0, LENS, None, slots=2, known=K, resampling=res, sampler=GD.StridedSampler(2))
    with pytest.raises(ValueError, match="without `known`"):
        d._run_chains(m, x0, LENS, None, slots=2, resampling=res)
    with pytest.raises(ValueError, match="noise tensor is refused"):
        d._run_chains(m, x0, LENS, None, slots=2, known=GD.KnownRegion(x0, keep, torch.zeros_like(x0)))
    d.release_chains()


@pytest.mark.parametrize("stride", [None, 3])
def test_conditioned_sweep_with_nothing_kept_is_the_unconditioned_sweep(stride):
    GD, m, d = shared()
    S = GD.StridedSampler(stride, 1.0) if stride else None
    x0, _, _, _ = planes(7, B=1)
    fwd = torch.randn(len(LENS), 1, 32, 32, device=DEV)
    d.seed_gauss(9)
    plain = d._run_chains(m, x0, LENS, fwd, slots=2, sampler=S)
    steps = d.last_chain_schedule["chain_steps"]
    d.seed_gauss(9)
    K = GD.KnownRegion(x0, torch.zeros(1, 1, 32, 32), "fixed")
    cond = d._run_chains(m, x0, LENS, fwd, slots=2, sampler=S, known=K)
    assert d.last_chain_schedule["chain_steps"] == steps
    assert torch.allclose(cond, plain, atol=1e-4, rtol=0) and torch.isfinite(cond).all()
    d.seed_gauss(9)
    ones = d._run_chains(m, x0, LENS, fwd, slots=2, sampler=S, known=GD.KnownRegion(x0, torch.ones(1, 1, 32, 32), "fixed"))
    assert all(torch.equal(ones[c], x0[0]) for c, L in enumerate(LENS) if L > 0)       # everything kept: the image itself
    d.release_chains()


def test_detection_B_with_keep_and_resampling(tmp_path, monkeypatch):
    """Records keep their keys and order; with both attributes unset again the images are those of a run made before either was
    ever set."""
    GD, m, d = shared()
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(1)
    x_0 = torch.rand(1, 1, 32, 32, device=DEV) * 2 - 1
    mask = (torch.rand(1, 1, 32, 32, device=DEV) > 0.7).float()
    args = {"arg_num": 9, "T": 100, "img_size": [32, 32]}
    d.seed_gauss(4)
    assert d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2) == [None]
    before = d.last_detection
    keys, images = [list(r) for r in before], [r["output"].clone() for r in before]
    assert d.last_chain_schedule["chain_steps"] == 100
    keep = torch.zeros(1, 32, 32, device=DEV)
    keep[:, :, :16] = 1
    d.detection_keep, d.resampling = keep, GD.Resampling(25, 2)
    d.seed_gauss(4)
    assert d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2) == [None]
    assert d.last_chain_schedule["chain_steps"] == 2 * GD.Resampling(25, 2).steps(50) == 150
    recs = d.last_detection
    assert [list(r) for r in recs] == keys and [r["t_distance"] for r in recs] == [50]
    out = recs[0]["output"]
    assert out.shape == (2, 1, 32, 32) and torch.isfinite(out).all()
    assert torch.equal(out[:, :, :, :16], x_0[:, :, :, :16].expand(2, -1, -1, -1)) and not torch.equal(out, images[0])
    d.resampling = None                                                      # conditioned, no jumps: the known launch
    d.seed_gauss(4)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert d.last_chain_schedule["chain_steps"] == 100
    assert torch.equal(d.last_detection[0]["output"][:, :, :, :16], x_0[:, :, :, :16].expand(2, -1, -1, -1))
    d.detection_keep = None
    d.seed_gauss(4)
    d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    assert [list(r) for r in d.last_detection] == keys
    assert all(torch.equal(r["output"], img) for r, img in zip(d.last_detection, images))
    d.resampling = GD.Resampling(25, 2)
    with pytest.raises(ValueError, match="detection_keep"):
        d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2)
    d.release_chains()
