"""-m gpu: the attention core and its softmax backward on peaked and offset logits (tests/attn_cases.py), through the C ABI:
anoddpm_attention (csrc/attention.hip), the three-launch form (anoddpm_igemm b_mode 1 -> anoddpm_softmax_rows -> anoddpm_igemm
b_mode 2) and anoddpm_softmax_rows_backward, each against fp64 of the same expression.

Forward: per (image, head) slab max |err| / max |ref| of P and of out, bar max(2e-5, 4 r32) <= 1.5e-4 with r32 the figure of the
fp32 CPU restatement of that slab; rows of P sum to 1 within 1e-5; out does not depend on whether P is requested.  The shapes are
the smallest that reach each path of attention_kernel: key-tile counts 1, 3, 9, 17, 25 and 64 in the double-buffered score loop
(9: only wave 0 owns a second tile; 17: a third, jt + 2 * AT_WAVES < nkt; 25: a fourth), head width 512 at L = 144 and 272 (the
single-buffered loop with one and two reloads, if (jt != wave) load_k), three heads in two images.
Backward: per row max |err| / (max P * max |dP|), bar 1e-6; a P that is one-hot bit for bit gives dS == 0 exactly; nothing is
written behind the last row; P is left alone.

Every (shape, regime) asserts; every figure is printed before it is asserted; a test collects its failures and asserts once.

Measured on an MI355X: the worst figure of a regime over its shapes, and the worst figure-to-bar ratio (the bars are 2e-5 except
sigma32: 2e-5 ... 4.9e-5, offset100: 2e-5 ... 9.0e-5, mixed: the bar of each slab's own regime, 2.7e-5 ... 4.2e-5 for its offset100 slab; backward bar 1e-6):
    regime      fused P          fused out        three-launch P   three-launch out   backward
    sigma1      1.6e-06 (0.08)   1.4e-06 (0.07)   2.0e-06 (0.10)   1.3e-06 (0.07)     1.2e-07
    sigma8      4.6e-06 (0.23)   4.6e-06 (0.23)   5.1e-06 (0.25)   4.2e-06 (0.21)     1.4e-07
    sigma32     1.9e-05 (0.66)   1.8e-05 (0.64)   2.0e-05 (0.71)   1.9e-05 (0.69)     1.2e-07
    uniform     3.0e-08 (0.00)   9.6e-07 (0.05)   3.0e-08 (0.00)   7.2e-07 (0.04)     1.1e-07
    match8      1.0e-06 (0.05)   1.8e-06 (0.09)   7.4e-07 (0.04)   1.3e-06 (0.06)     1.5e-07
    match100    4.4e-16 (0.00)   4.3e-16 (0.00)   3.2e-29 (0.00)   0       (0.00)     1.1e-10, one-hot P: 0 exactly
    offset100   1.8e-05 (0.53)   2.1e-05 (0.47)   1.9e-05 (0.56)   2.3e-05 (0.48)     1.2e-07
    mixed       1.0e-05 (0.27)   1.3e-05 (0.30)   -                -                  8.8e-08
    ragged backward (7 rows of 50, P = softmax(8 randn)): 1.6e-08.  cfg 0 and cfg 1 of the three-launch form agree to the digits shown.
Before the ch = 512 score tile summed into four accumulators (csrc/attention.hip, NACC) offset100 stood at 3.7e-05 (0.97) for
P and 3.6e-05 (0.84) for out at (1, 1, 144, 512), and at 2.9e-05 (0.92 / 0.94) at (1, 1, 272, 512); now 1.2e-05 (0.30) and 7.8e-06 (0.25).
Wall time of the module on the device: 3.2 s for the 18 tests, the slowest 0.35 s."""
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEDGER = {}


@pytest.fixture(scope="module", autouse=True)
def ledger():
    yield
    for key in sorted(LEDGER):
        print("worst", *key, f"{LEDGER[key]:.2e}")


def _check_forward(tag, regime, shape, P, out, fails):
    """P [B * heads, L, L], out [B, L, C] from the device."""
    B, heads, L, ch = shape
    P = P.cpu().reshape(B, heads, L, L)
    ac.forward_failures(tag, regime, shape, P, ac.unpack_out(out.cpu(), heads), fails, LEDGER)
    rowsum = (P.double().sum(-1) - 1).abs().max().item()
    print(f"{tag:12s} {str(shape):20s} {regime:10s} |rowsum(P) - 1| {rowsum:.2e}")
    if not rowsum <= 1e-5:
        fails.append(f"{tag} {shape} {regime}: rows of P sum to 1 within {rowsum:.3e} > 1e-5")


@pytest.mark.parametrize("shape", ac.FUSED_SHAPES + tuple(s for s in ac.MIXED_SHAPES if s not in ac.FUSED_SHAPES), ids=str)
def test_fused_attention_regimes(shape):
    import hipops
    heads = shape[1]
    fails = []
    for regime in [r for r, s in ac.fused_cases() if s == shape]:
        d = ac.forward_case(regime, shape)["qkv"].to(DEV)
        out, P = hipops.attention_fused(d, heads, want_probs=True)
        _check_forward("fused", regime, shape, P, out, fails)
        out2, none = hipops.attention_fused(d, heads)
        if none is not None or not torch.equal(out, out2):
            fails.append(f"fused {shape} {regime}: out depends on whether P is requested")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("shape", ac.LAUNCH3_SHAPES, ids=str)
def test_three_launch_attention_regimes(shape):
    import hipops
    heads, L = shape[1], shape[2]
    fails = []
    for regime, _ in [c for c in ac.launch3_cases() if c[1] == shape]:
        d = ac.forward_case(regime, shape)["qkv"].to(DEV)
        for cfg in ((1, 0) if L >= 128 else (1,)):
            out, P = hipops.attention(d, heads, cfg=cfg)
            _check_forward(f"launch3/cfg{cfg}", regime, shape, P, out, fails)
    assert not fails, "\n".join(fails)


def _check_backward(tag, regime, P, dP, dS, fails, exact_zero=False):
    import hipops
    p = P.to(DEV).contiguous()
    got, guard = hipops.softmax_rows_backward(p, dP.to(DEV))
    e = ac.row_error(got, dS, P, dP)
    worst = e.argmax().item()
    print(f"{tag:28s} {regime:10s} err {e.max().item():.2e} (row {worst}) vs bar {ac.BWD_BAR:.0e}")
    LEDGER[("backward", regime)] = max(LEDGER.get(("backward", regime), 0.0), e.max().item())
    if not (e < ac.BWD_BAR).all():
        fails.append(f"{tag} {regime}: {e.max().item():.3e} >= {ac.BWD_BAR:.0e} (row {worst})")
    if exact_zero and got.cpu().any():
        fails.append(f"{tag} {regime}: dS of a one-hot P is not exactly 0 (max {got.abs().max().item():.3e})")
    if not torch.isnan(guard).all():
        fails.append(f"{tag} {regime}: wrote behind the last row")
    if not torch.equal(p.cpu(), P):
        fails.append(f"{tag} {regime}: P was modified")


@pytest.mark.parametrize("shape", ac.BWD_SHAPES, ids=str)
def test_softmax_backward_regimes(shape):
    fails = []
    for regime in [r for r, s in ac.backward_cases() if s == shape]:
        c = ac.backward_case(regime, shape)
        _check_backward(f"backward {shape}", regime, c["P"], c["dP"], c["dS"], fails)
        if regime == "match100":
            hot = ac.one_hot(c["P"])
            _check_backward(f"backward {shape} one-hot", regime, hot, c["dP"], ac.backward_reference(hot, c["dP"]), fails, exact_zero=True)
    assert not fails, "\n".join(fails)


def test_softmax_backward_ragged():
    """The generic call: 7 rows (a partial block of 4) of 50 columns (no multiple of the wave)."""
    gen = torch.Generator().manual_seed(9000)
    P = torch.softmax(8 * torch.randn(7, 50, generator=gen, dtype=torch.float64), dim=-1).float()
    dP = torch.randn(7, 50, generator=gen, dtype=torch.float64).float()
    fails = []
    _check_backward("backward ragged (7, 50)", "8*randn", P, dP, ac.backward_reference(P, dP), fails)
    assert not fails, "\n".join(fails)
