"""-m gpu: anoddpm_loss_forward / anoddpm_loss_backward / anoddpm_vlb_terms straight through the C ABI, element by element and sample
by sample against the fp64 reference and the error model of tests/loss_cases.py (whose constants come from a CPU measurement of the
reference arithmetic, tests/test_loss_reference.py, never from the kernels).

Every output buffer and the workspace are filled with NaN before a launch: an element the kernels do not write shows.  d_eps is
judged per class ({main, kl, nll_lo, nll_hi, nll_mid} x {inside, outside the clamp}) and per sample, never against a batch-wide
scale; per_sample, vlb and total against VALUE_BAR.  anoddpm_vlb_terms states the element mathematics a second time: its out[0]
must meet the same bar and agree with loss_forward's vlb to 4 ulp, and its pred_x0 is the fp32 expression bit for bit (observed:
bit for bit; csrc/diffusion.hip is built with -ffp-contract=off).

Worst err / bound per class on the MI355X over this file (must be <= 1; none comes near it):
    main/in 0.418    kl/in 0.401    kl/out 0.502    nll_lo/in 0.223    nll_lo/out 0.339    nll_hi/in 0.239    nll_hi/out 0.344
    nll_mid/in 0.383    nll_mid/out 0.280        values: loss 0.032    vlb 0.015    total 0.017    vlb_terms against loss_forward: 0 ulp
Before the clamp of the predicted x0 kept a NaN (fminf / fmaxf return their other operand: read from the code, the earlier
kernel was not run against this file), a row with an out-of-range t came back with a finite vlb, a finite per-sample loss and d_eps equal to the main-term part, where vlb_kernel's comment promises NaN;
a NaN in the model output was hidden from vlb_terms' out[0] and out[1] in the same way (torch.clamp keeps it)."""
import ctypes

import numpy as np
import pytest
import torch

import loss_cases as lc
from anoddpm_amd import _lib
from anoddpm_amd._lib import LossArgs, VlbArgs, current_stream, lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
BLOCKS = 64                                                      # LOSS_BLOCKS = VLB_BLOCKS of csrc/diffusion.hip
NAMES = lc.case_names()
HYBRID = [c["name"] for c in lc.cases() if c["kind"] == 2]
LEDGER = {}
_TABLES = {}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def tables(sched):
    if sched not in _TABLES:
        _TABLES[sched] = {k: dev(v) for k, v in lc.schedule(sched)[1].items()}
    return _TABLES[sched]


def ulps32(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)


class Launch:
    """The device copy of a case and the argument struct over it.  `kind` overrides the case's (an l2 launch over a hybrid case's
    data gives the main-term part alone); kind < 2 hands x0, xt, t and the tables as NULL."""

    def __init__(self, case, kind=None):
        self.case = case
        self.kind = case["kind"] if kind is None else kind
        B, n = case["eps"].shape
        self.B, self.n = B, n
        self.t = {k: dev(case[k]) for k in ("eps", "noise", "x0", "xt", "t", "weights", "g_per", "g_total")}
        self.t["g_vlb"] = dev(case["g_vlb"]) if self.kind == 2 else None
        self.tab = tables(case["sched"])
        self.per, self.vlb, self.total = nans(B), nans(B), nans(1)
        self.ws = nans(B * BLOCKS * 2, dtype=torch.float64)
        self.d_eps = nans(B, n)

    def args(self):
        a, t = LossArgs(), self.t
        a.eps, a.noise, a.weights = ptr(t["eps"]), ptr(t["noise"]), ptr(t["weights"])
        if self.kind == 2:
            a.x0, a.xt, a.t = ptr(t["x0"]), ptr(t["xt"]), ptr(t["t"])
            for k, v in self.tab.items():
                setattr(a, k, ptr(v))
        a.per_sample, a.vlb, a.total = ptr(self.per), ptr(self.vlb), ptr(self.total)
        a.workspace, a.workspace_doubles = ptr(self.ws), self.ws.numel()
        a.g_per, a.g_vlb, a.g_total, a.d_eps = ptr(t["g_per"]), ptr(t["g_vlb"]), ptr(t["g_total"]), ptr(self.d_eps)
        a.n, a.B, a.T, a.kind = self.n, self.B, lc.T, self.kind
        return a

    def forward(self):
        a = self.args()
        _lib.check(lib().anoddpm_loss_forward(ctypes.byref(a), current_stream()), "loss_forward")
        return self.per.cpu().numpy(), self.vlb.cpu().numpy(), float(self.total.cpu()[0])

    def backward(self):
        a = self.args()
        _lib.check(lib().anoddpm_loss_backward(ctypes.byref(a), current_stream()), "loss_backward")
        return self.d_eps.cpu().numpy()


def value_failures(tag, case, ref, per=None, vlb=None, total=None):
    """Those of per_sample, vlb and total that are handed in, against `value_targets`; rows with an out-of-range t must be NaN and
    make the total NaN."""
    loose = case["kind"] == 2 and (ref["sat_log"].sum(axis=1) > 0).any()
    tg = lc.value_targets(case, ref, lc.oracle_values(case) if loose else None)
    ok = ~ref["bad"]
    lines = []
    for key, got in (("loss", per), ("vlb", vlb)):
        if got is None or (key == "vlb" and case["kind"] != 2):
            continue
        want, allow = tg[key]
        err = np.abs(got.astype(np.float64) - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(ok, err / allow, 0.0)
        ratio = np.where(ok & ~np.isfinite(got), np.inf, ratio)
        print(f"{tag:44s} {key}: worst err / bar {ratio.max():.3f}")
        LEDGER["value " + key] = max(LEDGER.get("value " + key, 0.0), float(ratio.max()))
        lines += [f"{tag}: {key}[{b}] (t {case['t'][b]}) got {got[b]:.9g} want {want[b]:.9g} err / bar {ratio[b]:.3f}"
                  for b in np.nonzero(ratio > 1.0)[0]]
        if not np.isnan(got[~ok]).all():
            lines.append(f"{tag}: {key} of a row with an out-of-range t is not NaN: {got[~ok]}")
    if total is None:
        return lines
    if ok.all():
        want, allow = tg["total"]
        r = abs(total - want) / allow if np.isfinite(total) else np.inf
        print(f"{tag:44s} total: err / bar {r:.3f}")
        LEDGER["value total"] = max(LEDGER.get("value total", 0.0), float(r))
        if not r <= 1.0:
            lines.append(f"{tag}: total got {total:.9g} want {want:.9g} err / bar {r:.3f}")
    elif not np.isnan(total):
        lines.append(f"{tag}: the total of a batch with an out-of-range t is {total}, not NaN")
    return lines


@pytest.mark.parametrize("name", NAMES)
def test_every_element_and_every_sample_against_fp64(name):
    case, ref = lc.get(name), lc.reference_of(name)
    run = Launch(case)
    per, vlb, total = run.forward()
    got = run.backward()
    ok_rows = torch.from_numpy(~ref["bad"]).to(DEV)              # (a row with an out-of-range t writes its NaN there)
    assert not torch.isnan(run.ws.view(run.B, BLOCKS, 2)[ok_rows]).any(), "the forward folds workspace entries it did not write"
    bad = lc.element_failures(name, got, case, ref, LEDGER)
    bad += value_failures(name, case, ref, per, vlb, total)
    if case["kind"] != 2:
        assert np.isnan(vlb).all(), "kind < 2 wrote vlb"
    # exactness
    for src, dst in case["twins"]:                               # t = -1 is t = T - 1
        assert np.array_equal(got[src].view(np.uint32), got[dst].view(np.uint32)), "d_eps of the t = -1 row"
        assert per[src].tobytes() == per[dst].tobytes() and vlb[src].tobytes() == vlb[dst].tobytes()
    if ref["bad"].any():                                         # out-of-range t: NaN rows, the others judged above
        assert np.isnan(got[ref["bad"]]).all(), "d_eps of a row with an out-of-range t is not NaN"
        assert np.isfinite(got[~ref["bad"]]).all()
    else:
        assert np.isfinite(got).all()
    if case["kind"] == 0:
        zero = case["eps"] == case["noise"]
        assert zero[:, : run.n // 4].all() and (got[zero] == 0).all()
    if case["kind"] == 2:
        # outside the clamp d_eps is the main-term part, to the bit: what an l2 launch over the same data and upstream gradients gives
        main = Launch(case, kind=1).backward()
        out = ~ref["inside"] & ~ref["bad"][:, None]
        assert (got[out] == main[out]).all(), "a clamped-out element carries a vlb contribution"
        if "third" in case:
            assert out.sum() >= 2 * (out.size // 3) - 2 * run.B
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", HYBRID)
def test_vlb_terms_and_loss_forward_state_the_same_mathematics(name):
    case, ref = lc.get(name), lc.reference_of(name)
    run = Launch(case)
    per, vlb, total = run.forward()
    B, n = run.B, run.n
    a, t = VlbArgs(), run.t
    a.x0, a.xt, a.eps, a.noise, a.t = ptr(t["x0"]), ptr(t["xt"]), ptr(t["eps"]), ptr(t["noise"]), ptr(t["t"])
    for k, v in run.tab.items():
        setattr(a, k, ptr(v))
    pred, out, ws = nans(B, n), nans(3, B), nans(B * BLOCKS * 3, dtype=torch.float64)
    a.pred_x0, a.out, a.workspace, a.workspace_doubles = ptr(pred), ptr(out), ptr(ws), ws.numel()
    a.n, a.B, a.T = n, B, lc.T
    _lib.check(lib().anoddpm_vlb_terms(ctypes.byref(a), current_stream()), "vlb_terms")
    out, pred = out.cpu().numpy(), pred.cpu().numpy()
    ok = ~ref["bad"]
    assert not torch.isnan(ws.view(B, BLOCKS, 3)[torch.from_numpy(ok).to(DEV)]).any()
    bad = value_failures(name + " (vlb_terms)", case, ref, vlb=out[0]) + value_failures(name, case, ref, vlb=vlb)
    u = ulps32(out[0][ok], vlb[ok])
    print(f"{name:44s} vlb_terms against loss_forward: {u.max() if u.size else 0:.1f} ulp")
    assert (u <= 4).all(), (out[0], vlb)
    assert np.isnan(out[0][~ok]).all() and np.isnan(out[1][~ok]).all() and np.isnan(pred[~ok]).all()
    # pred_x0: the fp32 expression of the reference, one rounding per operation
    tab = case["tables"]
    te, _ = lc.effective_t(case["t"])
    raw = tab["c_recip"][te][:, None] * case["xt"] - tab["c_recipm1"][te][:, None] * case["eps"]
    want = np.clip(raw, np.float32(-1), np.float32(1))
    assert raw.dtype == np.float32 and np.array_equal(pred[ok].view(np.uint32), want[ok].view(np.uint32))
    assert not bad, "\n".join(bad)


def test_null_upstream_gradients_and_weights_follow_the_formula():
    """All eight null-or-set combinations of g_per, g_vlb, g_total, with and without weights, on one hybrid case: each is what
    c_b = g_per[b] + g_total w_b / B, v_b = c_b + g_vlb[b] gives in fp64 (all NULL: exactly 0)."""
    base = lc.get("badt-linear")
    base = lc.select_rows(base, lc.valid_rows(base))
    bad = []
    for w in (None, base["weights"]):
        for mask in range(8):
            case = lc.with_gradients(base, g_per=base["g_per"] if mask & 1 else None, g_vlb=base["g_vlb"] if mask & 2 else None,
                                     g_total=base["g_total"] if mask & 4 else None)
            case["weights"] = w
            ref = lc.reference(case)
            got = Launch(case).backward()
            assert np.isfinite(got).all()
            if mask == 0:
                assert (got == 0).all()
            bad += lc.element_failures(f"gradients {mask:03b} weights {'set' if w is not None else 'null'}", got, case, ref, LEDGER)
    assert not bad, "\n".join(bad)


def test_empty_batches_and_argument_checks():
    """B = 0 and n = 0 return OK and write nothing; kind < 2 with NULL x0 / xt / t / tables is accepted (every l1 / l2 case above
    runs that way); hybrid with a NULL table, x0 or t is refused with a message before any launch."""
    case = lc.get("hybrid-now-total-linear-trained-n256")
    for B, n in ((0, 256), (9, 0)):
        run = Launch(case)
        run.B, run.n = B, n
        a = run.args()
        assert lib().anoddpm_loss_forward(ctypes.byref(a), current_stream()) == 0
        assert lib().anoddpm_loss_backward(ctypes.byref(a), current_stream()) == 0
        torch.cuda.synchronize()
        for buf in (run.per, run.vlb, run.total, run.ws, run.d_eps):
            assert torch.isnan(buf).all()
    for field in ("c_coef2", "c_model_logvar", "x0", "t"):
        run = Launch(case)
        a = run.args()
        setattr(a, field, None)
        for fn in (lib().anoddpm_loss_forward, lib().anoddpm_loss_backward):
            assert fn(ctypes.byref(a), current_stream()) == EINVAL
            assert lib().anoddpm_last_error()
        torch.cuda.synchronize()
        for buf in (run.per, run.vlb, run.total, run.ws, run.d_eps):
            assert torch.isnan(buf).all()
    assert b"null table" in lib().anoddpm_last_error() or b"needs x0" in lib().anoddpm_last_error()


def test_zz_worst_figures_of_this_file():
    """Prints the ledger (run the file with -s); every figure is <= 1 or an assertion above has failed."""
    for k in sorted(LEDGER):
        print(f"worst err / bound  {k:16s} {LEDGER[k]:.3f}")
    assert all(v <= 1.0 for v in LEDGER.values())
