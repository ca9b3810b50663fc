"""-m gpu: the strided sampler on the device -- the fused strided update against the fp64 restatement
(tests/sampler_cases.py), its three noise sources against each other and against the ancestral launch's pred_x0, and the chain /
detection plumbing: graph replay against serial one-step loops, a kept graph following a re-written stride and eta, slot-batched
sweeps, and the ancestral path left exactly as it was."""
import functools

import numpy as np
import pytest
import torch

import sampler_cases as sc
from test_gpu_detection import DEV, tiny

pytestmark = pytest.mark.gpu

T = sc.T


def _model(seed=None):
    import GaussianDiffusion as GD
    d = GD.GaussianDiffusionModel([32, 32], GD.get_beta_schedule(T, "linear"), noise="gauss")
    if seed is not None:
        d.seed_gauss(seed)
    return GD, d


@functools.lru_cache(maxsize=None)
def _reference(shape, row, stride, eta):
    return sc.reference(shape, row, stride, eta)


def _inputs(shape, row):
    x, eps, z = (torch.from_numpy(a).to(DEV) for a in sc.inputs(shape, row))
    return x, eps, z, torch.tensor(sc.T_ROWS[row], device=DEV)


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_strided_update_against_fp64_restatement(shape):
    """Every element of x_prev, mean and pred_x0 of every in-range sample against the restatement, no element excluded, for all
    t rows x strides x etas.  Bound (derivation: sampler_cases.error_bound): with u = 2^-23,
        u [(c_x0 + 2 c_dir / c_recipm1) (|p| + |q|) + 2.5 (|c_x0 x0| + |c_dir e'| + |sigma z|)]
    -- two roundings reach p - q and one more rounds it, the clamp is 1-Lipschitz, e' costs at most two such errors over
    c_recipm1 (c_dir / c_recipm1 <= 1), and the fp32 coefficients, the three products and the two sums round once each.  The
    out-of-range sample is all NaN."""
    GD, d = _model()
    worst = 0.0
    for row in range(len(sc.T_ROWS)):
        x, eps, z, t = _inputs(shape, row)
        for stride in sc.STRIDES:
            for eta in sc.ETAS:
                got, pred, mean = d._strided_update(x, t, eps, z, GD.StridedSampler(stride, eta), want_pred=True, want_mean=True)
                got, pred, mean = (a.cpu().numpy().astype(np.float64) for a in (got, pred, mean))
                for b, r in enumerate(_reference(shape, row, stride, eta)):
                    if r is None:
                        assert np.isnan(got[b]).all() and np.isnan(mean[b]).all(), (row, b, stride, eta)
                        continue
                    bound = sc.error_bound(r)
                    for name, g, want in (("x_prev", got[b], r["x_prev"]), ("mean", mean[b], r["mean"])):
                        err = np.abs(g - want)
                        ratio = float((err / bound).max())
                        worst = max(worst, ratio)
                        assert (err <= bound).all(), (name, row, b, stride, eta, ratio)
                    assert (np.abs(pred[b] - r["x0"]) <= 2.0 ** -23 * (np.abs(r["p"]) + np.abs(r["q"]))).all()
                    if r["sigma"] == 0.0:
                        assert np.array_equal(got[b], mean[b])           # no noise term at all
    print(f"shape {shape}: worst |error| / bound = {worst:.3f}")


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_pred_x0_is_the_ancestral_launchs_bit_for_bit(shape):
    GD, d = _model()
    for row in range(len(sc.T_ROWS)):
        x, eps, z, t = _inputs(shape, row)
        want = d._reverse_update(x, t, eps, z, want_pred=True)[1]
        got = d._strided_update(x, t, eps, z, GD.StridedSampler(5, 0.5), want_pred=True)[1]
        keep = [b for b in range(3) if sc.BAD.get(row) != b]
        assert torch.equal(got[keep], want[keep]), row


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_out_of_range_sample_is_nan_and_leaves_its_neighbours_alone(shape):
    GD, d = _model()
    (row, bad), = sc.BAD.items()
    x, eps, z, t = _inputs(shape, row)
    S = GD.StridedSampler(5, 0.5)
    got = d._strided_update(x, t, eps, z, S, want_pred=False)[0]
    assert torch.isnan(got[bad]).all()
    t_ok = t.clone()
    t_ok[bad] = 11
    ref = d._strided_update(x, t_ok, eps, z, S, want_pred=False)[0]
    keep = [b for b in range(3) if b != bad]
    assert torch.equal(got[keep], ref[keep]) and torch.isfinite(ref).all()
    # below -T is out of range too; a stride < 1 in the device word (the host never writes one) poisons every sample
    t_low = t_ok.clone()
    t_low[0] = -T - 1
    low = d._strided_update(x, t_low, eps, z, S, want_pred=False)[0]
    assert torch.isnan(low[0]).all() and torch.equal(low[1:], ref[1:])
    words = d._sampler_words(x.device, S)
    words.stride.zero_()
    words.held = None
    assert torch.isnan(d._strided_update(x, t_ok, eps, z, None, want_pred=False)[0]).all()


@pytest.mark.parametrize("shape", sc.SHAPES)
@pytest.mark.parametrize("row", [0, 1])
def test_seeded_form_equals_fill_then_tensor_form(shape, row):
    """The in-kernel Philox form (domain 0, step = normalised t: the ancestral keying) is philox.normal + the tensor form bit for
    bit, with and without pred_x0 / mean_out, and in place."""
    from anoddpm_amd import philox
    GD, d = _model(0x0123456789ABCDEF)
    x, eps, _, t = _inputs(shape, row)
    streams = philox.stream_ids(2 ** 32 - 2, 3).to(DEV)                   # wraps: 2^32 - 2, 2^32 - 1, 0
    noise = philox.normal(d._gauss_seed_dev(x.device), shape, stream=streams, step=t, domain=0, T=T)
    for stride, eta in ((5, 0.5), (1, 1.0), (T + 3, 1.0)):
        S = GD.StridedSampler(stride, eta)
        for want_pred, want_mean in ((True, True), (False, False)):
            ref = d._strided_update(x, t, eps, noise, S, want_pred=want_pred, want_mean=want_mean)
            got = d._strided_update(x, t, eps, None, S, want_pred=want_pred, want_mean=want_mean, gauss_streams=streams)
            for r, o in zip(ref, got):
                assert (r is None) == (o is None) and (r is None or torch.equal(r, o))
            assert (got[1] is not None) == want_pred and (got[2] is not None) == want_mean
        xi = x.clone()
        d._strided_update(xi, t, eps, None, S, want_pred=False, out=xi, gauss_streams=streams)     # in place: x_prev aliases x_t
        assert torch.equal(xi, ref[0])
    assert not torch.equal(d._strided_update(x, t, eps, noise, GD.StridedSampler(5, 0.5))[0],
                           d._strided_update(x, t, eps, None, GD.StridedSampler(5, 0.5))[0])        # the noise does enter


@pytest.mark.parametrize("shape", sc.SHAPES)
def test_eta_zero_reads_no_noise(shape):
    """sigma == 0: a NaN-filled noise tensor, no noise and the seeded form give the same bits."""
    from anoddpm_amd import philox
    GD, d = _model(77)
    streams = philox.stream_ids(5, 3).to(DEV)
    for row in (0, 1):
        x, eps, _, t = _inputs(shape, row)
        for stride in sc.STRIDES:
            S = GD.StridedSampler(stride, 0.0)
            none = d._strided_update(x, t, eps, None, S, want_mean=True)
            nans = d._strided_update(x, t, eps, torch.full_like(x, float("nan")), S, want_mean=True)
            seeded = d._strided_update(x, t, eps, None, S, want_mean=True, gauss_streams=streams)
            for a, b, c in zip(none, nans, seeded):
                assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
    # with eta > 0 the steps that pass t = 0 (sigma == 0) read no noise either; the others do
    x, eps, _, t = _inputs(shape, 0)                                      # t = 0, 4, 5
    out = d._strided_update(x, t, eps, torch.full_like(x, float("nan")), GD.StridedSampler(5, 1.0), want_pred=False)[0]
    assert torch.isfinite(out[:2]).all() and torch.isnan(out[2]).all()


def test_chain_advance_strided_floors_at_zero_and_counts():
    from anoddpm_amd._lib import check, current_stream, lib, ptr
    t = torch.tensor([22, 5, 4, 0, 99, 1], device=DEV, dtype=torch.int64)
    step = torch.tensor([3], device=DEV, dtype=torch.int32)
    for stride, want in ((5, [17, 0, 0, 0, 94, 0]), (1, [16, 0, 0, 0, 93, 0]), (T + 3, [0] * 6)):
        k = torch.tensor([stride], device=DEV, dtype=torch.int32)
        check(lib().anoddpm_chain_advance_strided(ptr(t), t.numel(), ptr(step), ptr(k), current_stream()), "chain_advance_strided")
        assert t.tolist() == want
    assert step.item() == 6
    check(lib().anoddpm_chain_advance_strided(ptr(t), t.numel(), None, ptr(k), current_stream()), "chain_advance_strided")
    assert lib().anoddpm_chain_advance_strided(ptr(t), t.numel(), ptr(step), None, current_stream()) == -1


# ------------------------------------------------------------------ chains


def _serial(m, d, x, t_distance, S, noise_of=None):
    """The chain as a loop of the public one-step form, at the batch size of x."""
    for t in S.timesteps(t_distance):
        tb = torch.full((x.shape[0],), t, device=DEV, dtype=torch.int64)
        fn = "gauss" if noise_of is None else (lambda xx, tt, t=t: noise_of(t))
        with torch.no_grad():
            x = d.sample_p_strided(m, x, tb, S, denoise_fn=fn)["sample"]
    return x


def test_graph_replaying_chain_equals_serial_steps():
    from anoddpm_amd import philox
    GD, m, d = tiny()
    torch.manual_seed(11)
    x = torch.rand(2, 1, 32, 32, device=DEV) * 2 - 1
    S = GD.StridedSampler(5)
    chain = d.reverse_chain(m, x, 23, "gauss", sampler=S)
    assert chain.use_graph and chain.remaining == 5 and chain.reuse_key == ("gauss", "strided")
    while chain.remaining:
        chain.step()
    assert chain.graph is not None and chain.t.tolist() == [0, 0] and chain.step_idx.item() == 5
    want = _serial(m, d, x, 23, S)
    assert torch.isfinite(want).all() and not torch.equal(want, x) and torch.equal(chain.x, want)
    # eta = 0.5 on a seeded instance: the chain draws in the kernel from streams 0, 1; the serial loop on an unseeded instance is
    # handed the same stream's values as a tensor
    d.seed_gauss(5)
    S = GD.StridedSampler(5, 0.5)
    chain = d.reverse_chain(m, x, 23, "gauss", sampler=S)
    assert chain.streams is not None and chain.noise is None and chain.reuse_key == ("gauss", "seeded", "strided")
    while chain.remaining:
        chain.step()
    _, plain = _model()
    want = _serial(m, plain, x, 23, S, lambda t: philox.normal(5, x.shape, stream=0, step=t, domain=0, device=DEV))
    assert torch.equal(chain.x, want)
    assert not torch.equal(want, _serial(m, plain, x, 23, GD.StridedSampler(5)))
    # the instance attribute is used when no keyword is given, the keyword first
    d.sampler = GD.StridedSampler(7)
    assert d.reverse_chain(m, x, 23, "gauss").remaining == 4 and d.reverse_chain(m, x, 23, "gauss", sampler=S).remaining == 5


def test_kept_chain_follows_a_new_stride_and_eta(monkeypatch):
    """One strided graph serves every stride and eta: the kept chain is restarted with k = 3 and with eta = 1 -- the same
    ReverseChain, the same graph object -- and equals fresh eager chains."""
    GD, m, d = tiny()
    d.seed_gauss(5)
    torch.manual_seed(12)
    xs = [torch.rand(2, 1, 32, 32, device=DEV) * 2 - 1 for _ in range(3)]
    runs = [(xs[0], 23, GD.StridedSampler(5, 0.5)), (xs[1], 17, GD.StridedSampler(3, 0.0)), (xs[2], 23, GD.StridedSampler(5, 1.0)),
            (xs[0], 9, GD.StridedSampler(3, 1.0))]
    outs, chain, graph = [], None, None
    for x, dist, S in runs:
        with torch.no_grad():
            outs.append(d._reverse_chain(m, x, dist, "gauss", None, S))
        kept = list(d._chains.values())
        assert len(kept) == 1 and kept[0].use_graph and kept[0].graph is not None and kept[0].sampler == S
        if chain is None:
            chain, graph = kept[0], kept[0].graph
        assert kept[0] is chain and chain.graph is graph
    assert d.gauss_next_stream == 2 * len(runs)
    monkeypatch.setenv("ANODDPM_NO_GRAPH", "1")
    for i, (x, dist, S) in enumerate(runs):
        _, fresh = _model(5)
        fresh.gauss_next_stream = 2 * i                                   # the streams the kept chain drew at its i-th restart
        with torch.no_grad():
            want = fresh._reverse_chain(m, x, dist, "gauss", None, S)
        assert not fresh.__dict__.get("_chains") and torch.equal(outs[i], want), i
    assert not torch.equal(outs[0], outs[2])


RUN_DISTS = [9, 9, 6, 3, 1, 0, 12]


def test_run_chains_on_slots_equal_serial_chains():
    from anoddpm_amd import philox
    from anoddpm_amd.diffusion import plan_chain_slots
    GD, m, d = tiny()
    S = GD.StridedSampler(4, 0.5)
    torch.manual_seed(3)
    x_0 = torch.rand(1, 1, 32, 32, device=DEV) * 2 - 1
    outs = {}
    for slots in (1, 4):
        d.seed_gauss(5)
        outs[slots] = d._run_chains(m, x_0, RUN_DISTS, None, slots=slots, sampler=S)
        sched = d.last_chain_schedule
        steps = [-(-l // 4) for l in RUN_DISTS]                            # 3, 3, 2, 1, 1, 0, 3
        assert sched["slots"] == slots and sched["chain_steps"] == sum(steps) == 13
        assert sched["steps"] == plan_chain_slots([k for k in steps if k], slots)[0] and torch.isfinite(outs[slots]).all()
    assert sched["steps"] == 4                                            # 4 slots, longest first: 3, 3, 3, 2 + 1, then 3 + 1
    assert torch.allclose(outs[1], outs[4], atol=1e-4, rtol=0) and torch.equal(outs[1][5], outs[4][5])
    _, serial = _model()
    shape = (1, 1, 32, 32)
    for c, dist in enumerate(RUN_DISTS):
        fwd = philox.normal(5, shape, stream=c, step=dist, domain=1, device=DEV)
        x = serial.sample_q(x_0, torch.full((1,), dist, device=DEV, dtype=torch.int64), fwd)
        x = _serial(m, serial, x, dist, S, lambda t, c=c: philox.normal(5, shape, stream=c, step=t, domain=0, device=DEV))
        for got in outs.values():
            if dist == 0:
                assert torch.equal(got[c:c + 1], x)
            assert torch.allclose(got[c:c + 1], x, atol=1e-4, rtol=0), (c, float((got[c:c + 1] - x).abs().max()))
    # the instance attribute does the same as the keyword, and equal slot counts repeat bit for bit
    d.sampler = S
    d.seed_gauss(5)
    assert torch.equal(d._run_chains(m, x_0, RUN_DISTS, None, slots=4), outs[4])


def test_ancestral_path_is_untouched_by_a_strided_run():
    GD, m, d = tiny()
    torch.manual_seed(13)
    x = torch.rand(2, 1, 32, 32, device=DEV) * 2 - 1
    d.seed_gauss(5)
    S = GD.StridedSampler(5, 0.5)
    seq = d.forward_backward(m, x, see_whole_sequence="half", t_distance=23, denoise_fn="gauss", sampler=S)
    assert len(seq) == 2 + 5 and all(torch.isfinite(s).all() for s in seq)
    strided = d.forward_backward(m, x, see_whole_sequence=None, t_distance=23, denoise_fn="gauss", sampler=S)
    assert strided.shape == x.shape and torch.isfinite(strided).all()
    d.seed_gauss(5)
    got = d.forward_backward(m, x, see_whole_sequence=None, t_distance=6, denoise_fn="gauss")
    assert sorted(k[3] for k in d._chains) == [("gauss", "seeded"), ("gauss", "seeded", "strided")]
    assert all(ch.use_graph and ch.graph is not None for ch in d._chains.values())
    _, fresh = _model(5)
    want = fresh.forward_backward(m, x, see_whole_sequence=None, t_distance=6, denoise_fn="gauss")
    assert torch.equal(got, want) and "_sampler_dev" not in fresh.__dict__
    # and a strided run after the ancestral one replays ITS graph, not the ancestral one
    d.seed_gauss(5)
    again = d.forward_backward(m, x, see_whole_sequence=None, t_distance=23, denoise_fn="gauss", sampler=S)
    d.seed_gauss(5)
    d.forward_backward(m, x, see_whole_sequence="half", t_distance=23, denoise_fn="gauss", sampler=S)
    d.sampler = S
    d.seed_gauss(5)
    assert torch.equal(d.forward_backward(m, x, see_whole_sequence=None, t_distance=23, denoise_fn="gauss"), again)
    assert len(d._chains) == 2


def test_detection_B_opts_in_through_the_environment(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    GD, m, plain = tiny()
    monkeypatch.setenv("ANODDPM_SAMPLER", "5,0")
    _, _, d = tiny()
    assert plain.sampler is None and d.sampler == GD.StridedSampler(5, 0.0)
    torch.manual_seed(1)
    x_0 = torch.rand(1, 1, 32, 32, device=DEV) * 2 - 1
    mask = (torch.rand(1, 1, 32, 32, device=DEV) > 0.7).float()
    args = {"arg_num": 9, "T": 100, "img_size": [32, 32]}
    assert plain.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2) == [None]
    assert plain.last_chain_schedule["chain_steps"] == 100
    assert d.detection_B(m, x_0, args, ("vol", "slice"), mask, denoise_fn="gauss", total_avg=2) == [None]
    assert d.last_chain_schedule["chain_steps"] == 20 and d.last_chain_schedule["steps"] == 10 and d.last_chain_schedule["slots"] == 2
    assert len(d.last_detection) == len(plain.last_detection) == 1
    rec, ref = d.last_detection[0], plain.last_detection[0]
    assert rec.keys() == ref.keys() and rec["t_distance"] == 50
    for k in rec:
        if torch.is_tensor(ref[k]):
            assert rec[k].shape == ref[k].shape and rec[k].dtype == ref[k].dtype, k
    assert torch.isfinite(rec["output"]).all() and torch.isfinite(rec["auc"]) and rec["ssim"] is not None
    assert not list(tmp_path.iterdir())
