"""CPU: the two statements and the error model of tests/anomaly_cases.py.  The numpy fp32 restatement of anoddpm_anomaly_map
(oracle.metrics_oracle.anomaly_maps over the C ABI's strided view) against the fp64 reference within the derived bounds, against
the upstream fixture bit for bit, and against CPU ATen's torch.mean(dim=0) where that keeps the sequential order; six mutated
restatements that the check the device gets must catch; the builder's cap; the oracle's ratios against the reference's formulas
(evaluation.py:26-76) in fp64 torch.  Run with -s for the figures."""
import os

import numpy as np
import pytest
import torch

import anomaly_cases as ac
from conftest import GOLDEN
from oracle import metrics_oracle as mo

G = np.load(os.path.join(GOLDEN, "metrics_kat.npz"))
NAMES = ac.case_names()
LEDGER = {}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_lies_within_the_bounds_of_the_reference(name):
    case = ac.get(name)
    maps, counts = ac.restate_of(case)
    bad = ac.check(name, case, maps, counts, LEDGER)
    assert not bad, "\n".join(bad)
    pm, pc = ac.restate(case, padded=True)                                # the pad is NaN: a read of it would show
    for k in ac.MAPS:
        assert ac.same_bits(pm[k], maps[k]).all(), k
    assert pc.tobytes() == counts.tobytes()


@pytest.mark.parametrize("fixture", ["one", "batch"])
def test_restatement_is_the_upstream_fixture_bit_for_bit(fixture):
    real, recon, mask = G[f"{fixture}_real"], G[f"{fixture}_recon"], G[f"{fixture}_mask"]
    B = real.shape[0]
    n = real.size // B
    navg = recon.size // real.size
    case = {"name": "fixture-" + fixture, "family": "uniform", "B": B, "n": n, "navg": navg, "threshold": 0.5, "exact": False,
            "real": real.reshape(B, n), "recon": recon.reshape(navg, B, n), "mask": mask.reshape(B, n)}
    for padded in (False, True):
        maps, counts = ac.restate(case, padded)
        for k in ac.MAPS:
            assert np.array_equal(maps[k].view(np.uint32), G[f"{fixture}_{k}"].reshape(B, n).view(np.uint32)), k
    bad = ac.check("fixture-" + fixture, case, maps, counts)
    assert not bad, "\n".join(bad)


def _aten(real, recon):
    """The reference's tensor expressions (GaussianDiffusion.py:517-520, detection.py:229-232) on CPU fp32 torch."""
    mean = torch.mean(torch.from_numpy(recon), dim=0)
    se = (mean - torch.from_numpy(real)).square()
    img = se * 2 - 1
    return {"mean": mean.numpy(), "sqerr": se.numpy(), "mse_img": img.numpy(), "thr_img": ((img > 0).float() * 2 - 1).numpy(),
            "pred": (se > 0.5).float().numpy()}


def _slices(navg, shape, seed):
    rs = np.random.RandomState(seed)
    real = rs.uniform(-1, 1, shape).astype(np.float32)
    recon = np.clip(real[None] + 0.6 * rs.standard_normal((navg,) + shape), -1, 1).astype(np.float32)
    return real, recon


@pytest.mark.parametrize("shape", [(1, 1, 32, 32), (3, 1, 8, 8)])
def test_restatement_is_cpu_aten_where_aten_keeps_the_sequential_order(shape):
    """navg <= 16 and a slice that is a multiple of 64 floats: bit for bit torch.mean(dim=0) and the expressions after it."""
    for navg in range(1, 17):
        real, recon = _slices(navg, shape, 500 + navg)
        maps, _ = mo.anomaly_maps(real, recon)
        want = _aten(real, recon)
        for k in ac.MAPS:
            assert np.array_equal(maps[k].view(np.uint32), want[k].view(np.uint32)), (navg, k)


def test_first_navg_at_which_cpu_aten_leaves_the_sequential_order():
    """Print only (csrc/metrics.hip cites it); asserted: ATen's mean and the restatement both lie within E_m of fp64 either way."""
    for shape in ((1, 1, 32, 32), (2, 3, 7, 5), (1, 1, 1, 1)):
        first = None
        for navg in range(1, 41):
            real, recon = _slices(navg, shape, 600 + navg)
            seq = mo.anomaly_maps(real, recon)[0]["mean"]
            aten = torch.mean(torch.from_numpy(recon), dim=0).numpy()
            m64 = recon.astype(np.float64).sum(axis=0) / navg
            e_m = navg * ac.U * np.abs(recon.astype(np.float64)).mean(axis=0) if navg > 1 else 0.0
            assert (np.abs(seq - m64) <= e_m).all() and (np.abs(aten - m64) <= e_m).all(), (shape, navg)
            if first is None and not np.array_equal(seq.view(np.uint32), aten.view(np.uint32)):
                first = navg
        print(f"slice {shape} ({int(np.prod(shape))} floats): CPU ATen (torch {torch.__version__}, {torch.get_num_threads()} threads) "
              f"first differs from the sequential sum at navg {first}")


MUTATIONS = ("reciprocal", "ge", "tail", "dense_as", "mask0", "max0")


def _statement(case, padded=False, mutate=None):
    """The kernel's statement written out here, with one defect switched in by `mutate`."""
    f = np.float32
    lay = ac.layout(case, padded)
    B, n, navg = case["B"], case["n"], case["navg"]
    ras = B * n if mutate == "dense_as" else lay["recon_as"]
    rec = mo.strided_recon(lay["buf"], navg, B, n, ras, lay["recon_bs"])
    real = case["real"]
    with np.errstate(invalid="ignore", over="ignore"):
        s = rec[0].copy()
        for k in range(1, navg):
            s = (s + rec[k]).astype(f)
        if navg > 1:
            s = (s * f(1.0 / navg)).astype(f) if mutate == "reciprocal" else (s / f(navg)).astype(f)
        d = (s - real).astype(f)
        se = (d * d).astype(f)
        img = (se * f(2) - f(1)).astype(f)
        thr = np.where(img > 0, f(1), f(-1)).astype(f)
        t = f(case["threshold"])
        pred = ((se >= t) if mutate == "ge" else (se > t)).astype(f)
    maps = {"mean": s, "sqerr": se, "mse_img": img, "thr_img": thr, "pred": pred}
    mask = case["mask"]
    if mutate == "mask0" and mask is not None:
        mask = np.broadcast_to(mask[:1], mask.shape)
    keep = n - n % 256 if mutate == "tail" else n
    if keep == 0:
        counts = np.zeros((B, ac.NC))
        counts[:, 10] = -np.inf
    else:
        counts = ac.counts_of(pred[:, :keep], None if mask is None else mask[:, :keep], se[:, :keep], real[:, :keep])
    if mutate == "max0":
        counts[:, 10] = np.maximum(counts[:, 10], 0.0)
    for k in maps:
        maps[k] = maps[k].copy()
        maps[k][:, keep:] = ac.SENTINEL
    return maps, counts


def test_the_statement_written_here_is_the_restatement():
    for name in NAMES:
        case = ac.get(name)
        for padded in (False, True):
            maps, counts = _statement(case, padded)
            want, wc = ac.restate_of(case)
            for k in ac.MAPS:
                assert ac.same_bits(maps[k], want[k]).all(), (name, k)
            assert ac._same64(counts[:, :9], wc[:, :9]).all() and ac._same64(counts[:, 10], wc[:, 10]).all(), name


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_a_mutated_restatement_fails_a_case(mutate):
    """Each defect is caught by the very check the device gets, on at least one case; which cases catch it is printed."""
    caught = []
    for name in NAMES:
        case = ac.get(name)
        if mutate == "reciprocal" and case["navg"] not in (3, 5, 7):
            continue
        maps, counts = _statement(case, padded=(mutate == "dense_as"), mutate=mutate)
        if ac.check(f"{mutate} {name}", case, maps, counts, show=False):
            caught.append(name)
    print(f"{mutate}: caught on {len(caught)} cases: {caught[:6]}")
    assert caught


def test_builder_cap_and_ambiguous_shares():
    shares = {}
    for case in ac.cases():
        ref = ac.reference_of(case)
        share = ac.ambiguous_share(ref)
        assert share <= ac.AMBIGUOUS_CAP, (case["name"], share)
        if case["exact"]:
            assert share == 0.0
            maps, _ = ac.restate_of(case)
            for k in ac.MAPS:                                          # every fp32 operation exact: equality with fp64
                assert (maps[k].astype(np.float64) == ref[k]).all(), (case["name"], k)
        s = shares.setdefault(case["family"], [0, 0])
        s[0] += int((ref["amb_pred"] | ref["amb_thr"]).sum())
        s[1] += ref["pred"].size
    for fam, (k, n) in sorted(shares.items()):
        print(f"ambiguous share, {fam:9s}: {k} of {n} = {k / n:.6f}")
    # the ties the cases put there
    tie = ac.get("ties-half-n1000")
    maps, _ = ac.restate_of(tie)
    half = np.float32(0.5)                                             # se = 0.5 itself is not reachable: the nearest either side
    assert (maps["sqerr"][0, [0, 2]] == np.nextafter(half, np.float32(0))).all() and (maps["sqerr"][0, [1, 3]] == np.nextafter(half, np.float32(1))).all()
    assert (maps["thr_img"][0, :4] == [-1, 1, -1, 1]).all() and (maps["pred"][0, :4] == [0, 1, 0, 1]).all()
    for navg in (1, 2, 16):
        lat = ac.get(f"lattice-navg{navg}-thr0.25")
        maps, _ = ac.restate_of(lat)
        assert (maps["sqerr"][:, 0] == 0.25).all() and (maps["pred"][:, 0] == 0).all()          # `>` is strict
        assert (maps["pred"][:, 1] == 1).all() and (maps["pred"][:, 2] == 0).all()
        zero = ac.get(f"lattice-navg{navg}-thr0")
        maps, _ = ac.restate_of(zero)
        assert (maps["sqerr"][:, 6] == 0).all() and (maps["pred"][:, 6] == 0).all() and (maps["pred"][:, 7] == 1).all()
        every = ac.restate_of(ac.get(f"lattice-navg{navg}-thr-1"))[0]
        assert (every["pred"] == 1).all()
    quiet = ac.get("quiet-navg5-n1000")
    _, c = ac.restate_of(quiet)
    assert (c[0, [0, 2, 3, 5, 7]] == 0).all() and 0 < c[0, 10] < 2.0 ** -10 and c[1, 10] < 0
    nonf = ac.get("nonfinite-navg3-n1000")
    maps, c = ac.restate_of(nonf)
    i = nonf["n"] // 3
    assert np.isnan(maps["mean"][1, i]) and np.isnan(maps["sqerr"][1, i]) and np.isnan(maps["mse_img"][1, i]) and np.isnan(c[1, 9])
    assert maps["pred"][1, i] == 0 and maps["thr_img"][1, i] == -1 and np.isnan(c[2, 10]) and np.isfinite(c[0]).all()


def test_mask_counts_follow_the_header():
    """Counts 3..6 count only mask values equal to 1 or 0, 7 and 8 any non-zero value, 1 and 2 are weighted sums."""
    case = ac.get("masks-values-navg3-n1000")
    maps, c = ac.restate_of(case)
    m, p = case["mask"].astype(np.float64), maps["pred"].astype(np.float64)
    for b in range(case["B"]):
        assert c[b, 1] == m[b].sum() and c[b, 2] == (m[b] * p[b]).sum()
        assert c[b, 3] + c[b, 4] == (m[b] == 1).sum() and c[b, 5] + c[b, 6] == (m[b] == 0).sum()      # -0.0 == 0
        assert c[b, 3:7].sum() < case["n"]                              # 0.5, 2 and -1 are in none of the four cells
        assert c[b, 7] == ((m[b] != 0) & (p[b] == 1)).sum() and c[b, 8] == ((m[b] != 0) | (p[b] == 1)).sum()


@pytest.mark.parametrize("edge", sorted(ac.edge_cases()))
def test_oracle_ratios_are_the_reference_formulas(edge):
    mask, pred = ac.edge_cases()[edge]
    _, c = mo.anomaly_maps(np.zeros_like(pred), pred[None], mask)         # (pred - 0)^2 > 0.5 is pred itself
    got, want = mo.ratios(c), ac.ratio_formulas(mask, pred)
    print(edge, {k: f"{want[k]:.9g}" for k in want})
    for k in want:
        assert ac.same_or_close(got[k], want[k], 1e-12), (k, got[k], want[k])


@pytest.mark.parametrize("name", sorted(ac.psnr_cases()))
def test_oracle_psnr_is_the_reference_formula(name):
    recon, real = ac.psnr_cases()[name]
    with np.errstate(invalid="ignore", divide="ignore"):
        _, c = mo.anomaly_maps(real, recon[None])
        got = mo.psnr(c, real.size)
    want = ac.psnr_formula(recon, real)
    print(name, got, want)
    assert ac.same_or_close(got, want, 1e-6), (got, want)                # sqerr is formed in fp32 by the pass, in fp64 by the formula
    assert {"all-negative": np.isnan(want), "zero-max": want == -np.inf, "plain": np.isfinite(want)}[name]


def test_zz_worst_figures_of_this_file():
    for k in sorted(LEDGER):
        print(f"restatement: worst err / bound  {k:8s} {LEDGER[k]:.3f}")
    assert all(v <= 1.0 for v in LEDGER.values())
