"""-m gpu: anoddpm_anomaly_map straight through the C ABI, element by element and count by count, against the two statements and
the error model of tests/anomaly_cases.py (derived bounds; nothing here is fitted to what the device gives), then through
metrics.anomaly_maps and the evaluation.py-shaped functions on top of it.

Every output buffer, the counts and the workspace are filled with a sentinel before a launch and carry guard elements behind
their end: an element that is not written, or one that is written and should not be, shows.

Worst err / bound on the MI355X over this file (must be <= 1):    mean 0.759    sqerr 0.925    mse_img 0.559
the CPU restatement's own figures, as they must be: every map of every case, layout and NULL pattern came back with the
restatement's bits.  This file and tests/test_gpu_metrics.py together: 93 tests in 3.2 s.
What the three findings behind this file turned out to be on the device:
  1. the mean: the device's bits are the sequential fp32 sum and one division at every navg and size of the cases (1 ... 33 chains,
     1 ... 32 845 elements, both layouts); CPU ATen keeps that order only up to navg 16 on whole vector lanes, so the identity with
     torch.mean is a property of the two upstream fixtures and the contract is the statement plus E_m.
  2. NaN in `real`: fmax dropped it (read from the code; the earlier kernel was not run against this file); the running maximum
     and its three folds now keep it and counts[b][10] is NaN, like torch.max.
  3. dice_coeff(mse=X): for a real-valued X the earlier code thresholded sqrt(X) and returned another number than the reference
     (read from the code); it now forms the reference's three sums in fp64 for every X, asserted below for a binary and a
     real-valued X."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import anomaly_cases as ac
from anoddpm_amd import _lib
from anoddpm_amd._lib import AnomalyArgs, current_stream, lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
GUARD = 64
NAMES = ac.case_names()
BATCHED = [c["name"] for c in ac.cases() if c["B"] > 1]
LEDGER = {}
SENT = float(ac.SENTINEL)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)   # the cases are read-only


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def row_of(case, b):
    """Image b of a case as a case of its own."""
    out = dict(case)
    out.update(name=f"{case['name']}/row{b}", B=1, real=case["real"][b:b + 1], recon=case["recon"][:, b:b + 1],
               mask=None if case["mask"] is None else case["mask"][b:b + 1])
    return out


class Launch:
    """The device copy of a case in one layout, sentinel-filled outputs with guards, and the argument struct over them.
    `outputs`: the maps whose pointer is handed in; the others are NULL."""

    def __init__(self, case, padded=False, outputs=ac.MAPS):
        self.case, self.outputs = case, tuple(outputs)
        self.B, self.n = case["B"], case["n"]
        self.lay = ac.layout(case, padded)
        self.recon, self.real, self.mask = dev(self.lay["buf"]), dev(case["real"]), dev(case["mask"])
        self.maps = {k: torch.empty(self.B * self.n + GUARD, dtype=torch.float32, device=DEV) for k in ac.MAPS}
        self.counts = torch.empty((self.B, ac.NC), dtype=torch.float64, device=DEV)
        self.need = ac.BLOCKS * self.B * ac.NC
        self.ws = torch.empty(self.need + GUARD, dtype=torch.float64, device=DEV)
        self.fill()

    def fill(self):
        for t in list(self.maps.values()) + [self.counts, self.ws]:
            t.fill_(SENT)

    def args(self):
        a = AnomalyArgs()
        a.recon, a.real, a.mask = ptr(self.recon), ptr(self.real), ptr(self.mask)
        for k in ac.MAPS:
            setattr(a, k, ptr(self.maps[k] if k in self.outputs else None))
        a.counts, a.workspace, a.workspace_doubles = ptr(self.counts), ptr(self.ws), self.need
        a.n, a.recon_as, a.recon_bs = self.n, self.lay["recon_as"], self.lay["recon_bs"]
        a.navg, a.B, a.threshold = self.case["navg"], self.B, self.case["threshold"]
        return a

    def call(self, a=None):
        a = self.args() if a is None else a
        return lib().anoddpm_anomaly_map(ctypes.byref(a), current_stream())

    def run(self):
        _lib.check(self.call(), "anomaly_map")
        torch.cuda.synchronize()
        return self.read()

    def read(self):
        """(the maps that were asked for as [B][n] numpy, counts [B][12]) after the guards and the NULL outputs were looked at."""
        size = self.B * self.n
        for k, t in self.maps.items():
            host = t.cpu().numpy()
            assert (host[size:] == ac.SENTINEL).all(), f"{k}: written behind its end"
            if k not in self.outputs:
                assert (host == ac.SENTINEL).all(), f"{k}: written though its pointer was NULL"
        ws = self.ws.cpu().numpy()
        assert (ws[self.need:] == SENT).all(), "workspace written beyond 64 B 12 doubles"
        counts = self.counts.cpu().numpy()
        assert (counts[:, 11] == SENT).all(), "the reserved column 11 was written"
        return {k: self.maps[k].cpu().numpy()[:size].reshape(self.B, self.n) for k in self.outputs}, counts

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in list(self.maps.values()) + [self.counts, self.ws])


def bits_equal(a, b):
    return all(ac.same_bits(a[k], b[k]).all() for k in a)


def counts_equal(a, b):
    return ac._same64(a[:, :11], b[:, :11]).all()


@pytest.mark.parametrize("name", NAMES)
def test_every_element_and_every_count_through_the_c_abi(name):
    case = ac.get(name)
    maps, counts = Launch(case).run()
    bad = ac.check(name, case, maps, counts, LEDGER)
    assert not bad, "\n".join(bad)
    for k in ac.MAPS:                                                    # no written element still holds the sentinel
        assert not (maps[k] == ac.SENTINEL).any(), k
    # the padded layout (every pad element NaN): the same bits
    pmaps, pcounts = Launch(case, padded=True).run()
    assert bits_equal(maps, pmaps) and counts_equal(counts, pcounts), "padded layout"
    # NULL outputs: none, then each output alone -- what is written is the same bits, nothing else is written (Launch.read)
    for outputs in [()] + [(k,) for k in ac.MAPS]:
        smaps, scounts = Launch(case, outputs=outputs).run()
        assert bits_equal(smaps, {k: maps[k] for k in outputs}) and counts_equal(counts, scounts), outputs


@pytest.mark.parametrize("name", BATCHED)
def test_a_row_of_a_batch_is_the_image_launched_alone(name):
    case = ac.get(name)
    maps, counts = Launch(case).run()
    for b in range(case["B"]):
        rmaps, rcounts = Launch(row_of(case, b)).run()
        for k in ac.MAPS:
            assert ac.same_bits(maps[k][b], rmaps[k][0]).all(), (b, k)
        assert counts_equal(counts[b:b + 1], rcounts), b


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("nonfinite")])
def test_nonfinite_inputs_stay_in_their_image_and_show_in_its_counts(name):
    case = ac.get(name)
    n = case["n"]
    maps, counts = Launch(case).run()
    clean = row_of(case, 0)
    cmaps, ccounts = Launch(clean).run()
    assert all(ac.same_bits(maps[k][0], cmaps[k][0]).all() for k in ac.MAPS) and counts_equal(counts[:1], ccounts)
    assert np.isfinite(counts[0, :11]).all() and all(np.isfinite(maps[k][0]).all() for k in ac.MAPS)
    i = n // 3                                                           # the NaN in recon of image 1
    assert np.isnan(maps["mean"][1, i]) and np.isnan(maps["sqerr"][1, i]) and np.isnan(maps["mse_img"][1, i])
    assert maps["pred"][1, i] == 0 and maps["thr_img"][1, i] == -1 and np.isnan(counts[1, 9])
    j = n // 2                                                           # the +inf in recon of image 1
    assert maps["mean"][1, j] == np.inf and maps["sqerr"][1, j] == np.inf and maps["pred"][1, j] == 1 and maps["thr_img"][1, j] == 1
    assert np.isfinite(counts[1, :9]).all() and np.isfinite(counts[1, 10])
    assert np.isnan(counts[2, 10]), "max(real) of an image with a NaN in real must be NaN, like torch.max"
    assert np.isnan(maps["sqerr"][2, n - 2]) and np.isnan(counts[2, 9]) and np.isnan(maps["mean"][2]).sum() == 0


def test_two_launches_and_a_graph_replay_give_identical_bits():
    case = ac.get("uniform-navg5-n16385-B3")
    run = Launch(case, padded=True)
    first = run.run()
    run.fill()
    second = run.run()
    assert bits_equal(first[0], second[0]) and counts_equal(first[1], second[1])
    run.fill()
    a = run.args()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()                                                        # no collection of older graphs inside the capture
    try:
        with torch.cuda.graph(g):
            rc = run.call(a)
    finally:
        if was_enabled:
            gc.enable()
    assert rc == 0
    g.replay()
    torch.cuda.synchronize()
    third = run.read()                                                  # column 11, the workspace's tail and the guards as well
    assert bits_equal(first[0], third[0]) and counts_equal(first[1], third[1])
    bad = ac.check(case["name"] + " (replay)", case, third[0], third[1], LEDGER)
    assert not bad, "\n".join(bad)


def test_refusals_come_without_a_launch_and_empty_batches_write_nothing():
    case = ac.get("uniform-navg3-n65-B3")

    def refused(change):
        run = Launch(case)
        a = run.args()
        change(a, run)
        assert run.call(a) == EINVAL and lib().anoddpm_last_error()
        assert run.untouched()

    refused(lambda a, run: setattr(a, "navg", 0))
    refused(lambda a, run: setattr(a, "B", 65536))
    refused(lambda a, run: setattr(a, "workspace_doubles", run.need - 1))
    for field in ("recon", "real", "counts", "workspace"):
        refused(lambda a, run, field=field: setattr(a, field, None))
    for field in ("B", "n"):
        run = Launch(case)
        a = run.args()
        setattr(a, field, 0)
        assert run.call(a) == 0 and run.untouched()


def _wrapper_case():
    case = ac.get("uniform-navg5-c3x7x5-B2")
    return case, ac.restate_of(case)


def test_wrapper_takes_the_three_recon_forms_and_three_channels():
    from anoddpm_amd import metrics
    case, (want, wc) = _wrapper_case()
    B, navg, shape = case["B"], case["navg"], (3, 7, 5)
    real, recon = dev(case["real"]).reshape(B, *shape), dev(case["recon"]).reshape(navg, B, *shape)
    mask = dev(case["mask"]).reshape(B, *shape)
    maps, counts = metrics.anomaly_maps(real, recon, mask)              # [navg,B,C,H,W]
    assert set(maps) == set(ac.MAPS) and all(maps[k].shape == real.shape for k in maps)
    got = {k: maps[k].cpu().numpy().reshape(B, -1) for k in maps}
    bad = ac.check("wrapper [navg,B,C,H,W]", case, got, counts.cpu().numpy(), LEDGER)
    assert not bad, "\n".join(bad)
    assert (counts[:, 11] == 0).all()                                   # the wrapper hands out zeroed counts
    # a bool mask, and a non-contiguous real: the same bits
    wide = torch.zeros(B, 3, 7, 9, device=DEV)
    wide[..., 2:7] = real
    m2, c2 = metrics.anomaly_maps(wide[..., 2:7], recon, mask.bool())
    assert not wide[..., 2:7].is_contiguous() and all(torch.equal(m2[k], maps[k]) for k in maps) and torch.equal(c2, counts)
    # [B,C,H,W]: one reconstruction per image
    one = dict(case, name=case["name"] + "/navg1", navg=1, recon=case["recon"][:1])
    m1, c1 = metrics.anomaly_maps(real, recon[0], mask)
    bad = ac.check("wrapper [B,C,H,W]", one, {k: m1[k].cpu().numpy().reshape(B, -1) for k in m1}, c1.cpu().numpy(), LEDGER)
    assert not bad, "\n".join(bad)
    # [navg,C,H,W] with B = 1: the chains of one image
    row = row_of(case, 1)
    mr, cr = metrics.anomaly_maps(real[1:2], recon[:, 1], mask[1:2])
    bad = ac.check("wrapper [navg,C,H,W]", row, {k: mr[k].cpu().numpy().reshape(1, -1) for k in mr}, cr.cpu().numpy(), LEDGER)
    assert not bad, "\n".join(bad)
    assert all(ac.same_bits(mr[k].cpu().numpy().reshape(-1), want[k][1]).all() for k in mr)
    # want=(): counts alone
    m0, c0 = metrics.anomaly_maps(real, recon, mask, want=())
    assert m0 == {} and torch.equal(c0, counts)
    # mismatches
    with pytest.raises(ValueError):
        metrics.anomaly_maps(real, recon[:, :, :, :6], mask)
    with pytest.raises(ValueError):
        metrics.anomaly_maps(real, recon[:, :1], mask)
    with pytest.raises(ValueError):
        metrics.anomaly_maps(real, recon, mask[:1])


@pytest.mark.parametrize("edge", sorted(ac.edge_cases()))
def test_ratios_are_the_reference_formulas_on_the_edges(edge):
    """dice_coeff (also with mse=), precision, recall, FPR and IoU against evaluation.py:26-76 in fp64 torch, rel 1e-6."""
    from anoddpm_amd import metrics
    mask, pred = ac.edge_cases()[edge]
    want = ac.ratio_formulas(mask, pred)
    m, p = dev(mask), dev(pred)
    zeros = torch.zeros_like(p)
    got = {"dice": metrics.dice_coeff(zeros, p, m).item(), "dice(mse=)": metrics.dice_coeff(zeros, zeros, m, mse=p).item(),
           "precision": metrics.precision(m, p).item(), "recall": metrics.recall(m, p).item(), "FPR": metrics.FPR(m, p).item(),
           "IoU": metrics.IoU(m, p)}
    print(edge, {k: f"{v:.9g}" for k, v in got.items()})
    for k, v in got.items():
        assert ac.same_or_close(v, want["dice" if k.startswith("dice") else k], 1e-6), (k, v, want)


def test_dice_coeff_uses_a_given_mse_as_it_is():
    """evaluation.py:31-36: a given `mse` is not thresholded.  X = the real-valued squared error of a case (values anywhere in
    [0, 4]) and a mask with values other than 0 and 1: sum(X mask) and sum(X) + sum(mask) per image in fp64, rel 1e-6."""
    from anoddpm_amd import metrics
    case = ac.get("masks-values-navg3-n1000")
    ref = ac.reference_of(case)
    B = case["B"]
    x = ac.restate_of(case)[0]["sqerr"].reshape(B, 1, 25, 40)
    mask = case["mask"].reshape(B, 1, 25, 40)
    x64, m64 = torch.tensor(x, dtype=torch.float64), torch.tensor(mask, dtype=torch.float64)
    inter = torch.sum(x64 * m64, dim=[1, 2, 3])
    union = torch.sum(x64, dim=[1, 2, 3]) + torch.sum(m64, dim=[1, 2, 3])
    want = float(torch.mean((2.0 * inter + 0.000001) / (union + 0.000001), dim=0))
    got = metrics.dice_coeff(None, None, dev(mask), mse=dev(x)).item()
    c = ref["counts"]                                                   # X run through the threshold pass, as the earlier code did
    thresholded = float(np.mean((2.0 * c[:, 2] + 0.000001) / (c[:, 0] + c[:, 1] + 0.000001)))
    print(f"dice_coeff(mse=real-valued): got {got:.9g} reference {want:.9g} (thresholding X first would give about {thresholded:.6g})")
    assert abs(got - want) <= 1e-6 * abs(want)
    assert abs(thresholded - want) > 1e-3 * abs(want)                    # the case can tell the two readings apart
    with pytest.raises(ValueError):
        metrics.dice_coeff(None, None, dev(mask[:1]), mse=dev(x))


@pytest.mark.parametrize("name", sorted(ac.psnr_cases()))
def test_psnr_is_the_reference_formula(name):
    """rel 1e-5 as tests/test_gpu_metrics.py has it; NaN for an all-negative image and -inf for a maximum of 0, as the formula gives."""
    from anoddpm_amd import metrics
    recon, real = ac.psnr_cases()[name]
    want = ac.psnr_formula(recon, real)
    got = metrics.PSNR(dev(recon), dev(real))
    print(name, float(got), want)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and ac.same_or_close(got, want, 1e-5), (got, want)


def test_zz_worst_figures_of_this_file():
    """Prints the ledger (run the file with -s); every figure is <= 1 or an assertion above has failed."""
    for k in sorted(LEDGER):
        print(f"device: worst err / bound  {k:8s} {LEDGER[k]:.3f}")
    assert LEDGER and all(v <= 1.0 for v in LEDGER.values())
