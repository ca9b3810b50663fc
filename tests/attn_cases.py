"""Shared by the attention conditioning tests (tests/test_attn_reference.py on the CPU, tests/test_gpu_attention.py on the device):
operands whose logits are peaked or ride on a large common offset, the fp64 references of the attention core and of the softmax
backward, the per-slab and per-row error figures, an fp32 CPU restatement of both, and the bars.  No device needed here.

Why: QKVAttentionLegacy (UNet.py:137-153) is  P = softmax(alpha q k^T),  out = P v,  alpha = ch^-1/2.  With standard-normal operands
the logits have a standard deviation of 1-2, no row of P comes near one-hot, and neither the max subtraction, nor exp far from 0,
nor 1 / sum on a sum of 1, nor the cancellation in  dS = P o (dP - sum_j P dP)  on a peaked P is exercised.  A trained model has
logits of several tens.

Operand recipe (`operand`): fp32 q, k, v [B, heads, L, ch], drawn in fp64 from a seeded generator; v is standard normal.
  sigma1 / sigma8 / sigma32   q, k = sqrt(sigma) n: logits of standard deviation sigma (today's operands ... rows mostly one-hot)
  uniform                     q = 0: P = 1 / L everywhere
  match8 / match100           unit vectors u_i;  q_i = sqrt(m) ch^1/4 u_i + 0.3 n,  k_pi(i) = sqrt(m) ch^1/4 u_i + 0.3 n'  with a random
                              permutation pi per slab: every query has one key at a logit of about m
  offset100                   q, k = n + sqrt(100) ch^1/4 d, d one unit vector per slab: every logit sits near 100, P is not peaked
  mixed                       B * heads = 6 slabs, each of a different regime (MIXED)
In match100 and offset100 the row maxima lie beyond 88.73 = log(FLT_MAX): an exponential without the max subtraction overflows.

Forward figure (`slab_error`): per (image, head) slab  max |got - ref| / max |ref|,  separately for P [L, L] and out [L, ch]: a quiet
slab cannot hide behind a loud one.  Forward bar of a slab: max(TOL, 4 r32), r32 the same figure of the fp32 CPU restatement
(`forward_fp32`) of that slab, computed at run time: the inherent fp32 error of P grows like eps |S|max, so one fixed bar cannot
serve logits of 1 and of 100; the factor 4 allows for another summation order and for the hardware exponential.  No bar may
exceed CAP: test_attn_reference.py asserts 4 r32 <= CAP for every case of the device test, and `forward_bars` clamps to it.  The
widest sigma regime is 32 and not 48 for that reason: at sigma = 48 the restatement reached 3.8e-5 at (1, 1, 400, 256), 4 r32 = 1.51e-4;
at sigma = 32 its worst slab over all shapes is 1.9e-5 (offset100: 2.3e-5).

Backward figure (`row_error`): per row  max_j |err_ij| / (max_j P_ij * max_j |dP_ij|),  the natural rounding scale of the row:
every term of the row's dot product and every factor of the result is bounded by that product.  Dividing by max |dS| instead is
ill-conditioned where the gradient vanishes (a one-hot row has dS = 0): the fp32 restatement itself then shows errors of
1e-3 ... 1.  Backward bar: BWD_BAR = 1e-6, four times the worst row of the fp32 restatement (`backward_fp32`), which
test_attn_reference.py holds at or below BWD_R32_CAP = 2.5e-7.  That cap is about four half-ulp roundings stacked the same way and
the worst of some 30 000 rows sits close to it: of six draws tried, four stayed below (worst 1.5e-7 ... 2.3e-7) and two had a single
row at 2.6e-7.  BWD_SEED pins one of the four; the device bar does not depend on it.

match100: every row of the fp32 P has a maximum of exactly 1.0, but the other entries are tiny (1e-10 ... 1e-40) and not 0, so dS is
tiny and not 0.  `one_hot` rounds such a P to the bit-for-bit one-hot matrix, for which dS is exactly 0 whatever dP is."""
import functools
import math

import torch

TOL = 2e-5                  # TOL of test_gpu_ops.py
CAP = 1.5e-4                # no forward bar may exceed this
BWD_BAR = 1e-6
BWD_R32_CAP = 2.5e-7
BWD_SEED = 1
EXP_OVERFLOW = 88.73        # log(FLT_MAX) rounded up: expf overflows beyond it

LEVELS = {"sigma1": 1.0, "sigma8": 8.0, "sigma32": 32.0, "uniform": 0.0, "match8": 8.0, "match100": 100.0, "offset100": 100.0}
REGIMES = tuple(LEVELS)
MIXED = ("sigma1", "match100", "offset100", "sigma32", "uniform", "match8")         # slab b * heads + h of the `mixed` case

# (B, heads, L, ch) of the fused kernel: the smallest shapes that reach each path of csrc/attention.hip (key tiles = L / 16, eight
# waves; wave w owns key tiles w, w + 8, ...)
FUSED_SHAPES = (
    (2, 3, 16, 16),         # one key tile; CHQ = 1: only wave 0 works in P v
    (1, 2, 48, 64),         # 3 tiles: the odd tail of the P v pairing
    (1, 2, 144, 32),        # 9 tiles: only wave 0 owns a second tile
    (1, 1, 272, 128),       # 17 tiles: wave 0 owns a third tile (jt + 2 * AT_WAVES < nkt)
    (1, 1, 400, 256),       # 25 tiles: a fourth tile; two channel tiles per wave
    (1, 1, 144, 512),       # the non-double-buffered loop WITH its reload (if (jt != wave) load_k)
    (1, 1, 272, 512),       # the non-double-buffered loop with two reloads
    (1, 2, 1024, 64),       # the largest resident score block
)
MIXED_SHAPES = ((2, 3, 16, 16), (2, 3, 144, 32))
LAUNCH3_SHAPES = ((1, 2, 48, 64), (1, 2, 144, 96), (1, 1, 400, 256))               # head width 96 can take only this route
BWD_SHAPES = ((6, 16, 16), (2, 48, 64), (2, 144, 512), (1, 272, 32), (2, 1024, 64))    # (Z, L, ch)


def fused_cases():
    """[(regime, shape)] of the fused kernel's test."""
    return [(r, s) for s in FUSED_SHAPES for r in REGIMES] + [("mixed", s) for s in MIXED_SHAPES]


def launch3_cases():
    return [(r, s) for s in LAUNCH3_SHAPES for r in REGIMES]


def backward_cases():
    return [(r, s) for s in BWD_SHAPES for r in REGIMES + (("mixed",) if s[0] == len(MIXED) else ())]


# ---------------------------------------------------------------------------------------------------- operands
def _slab(regime, L, ch, gen):
    """fp64 q, k, v [L, ch] of one (image, head)."""
    def rn(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)

    level = LEVELS[regime]
    v = rn(L, ch)
    if regime.startswith("sigma"):
        return math.sqrt(level) * rn(L, ch), math.sqrt(level) * rn(L, ch), v
    if regime == "uniform":
        return torch.zeros(L, ch, dtype=torch.float64), rn(L, ch), v
    if regime.startswith("match"):
        u = rn(L, ch)
        u = math.sqrt(level) * ch ** 0.25 * u / u.norm(dim=1, keepdim=True)
        q = u + 0.3 * rn(L, ch)
        k = torch.empty(L, ch, dtype=torch.float64)
        k[torch.randperm(L, generator=gen)] = u + 0.3 * rn(L, ch)
        return q, k, v
    assert regime.startswith("offset"), regime
    d = rn(ch)
    d = math.sqrt(level) * ch ** 0.25 * d / d.norm()
    return rn(L, ch) + d, rn(L, ch) + d, v


def slab_regimes(regime, B, heads):
    """The regime of every (image, head) slab, image-major."""
    if regime == "mixed":
        assert B * heads == len(MIXED), "the mixed case has six slabs"
        return MIXED
    return (regime,) * (B * heads)


def operand(regime, B, heads, L, ch, seed=0):
    """fp32 q, k, v [B, heads, L, ch] of a regime."""
    gen = torch.Generator().manual_seed(7000 + 100 * seed + (REGIMES + ("mixed",)).index(regime))
    slabs = [_slab(r, L, ch, gen) for r in slab_regimes(regime, B, heads)]
    return tuple(torch.stack([s[i] for s in slabs]).reshape(B, heads, L, ch).float() for i in range(3))


def pack_qkv(q, k, v):
    """[B, heads, L, ch] x 3 -> [B, L, 3 C], the legacy layout both device routes read: per head a contiguous q|k|v block of 3 ch."""
    B, heads, L, ch = q.shape
    return torch.cat([q, k, v], dim=-1).permute(0, 2, 1, 3).reshape(B, L, heads * 3 * ch).contiguous()


def unpack_out(out, heads):
    """[B, L, C] -> [B, heads, L, ch]."""
    B, L, C = out.shape
    return out.reshape(B, L, heads, C // heads).permute(0, 2, 1, 3)


def logits(q, k):
    """fp64 S = alpha q k^T [B, heads, L, L] of fp32 operands."""
    return (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(q.shape[-1])


# ---------------------------------------------------------------------------------------------------- forward
def forward_reference(q, k, v):
    """fp64 (P [B, heads, L, L], out [B, heads, L, ch]) from the fp32 operands."""
    P = torch.softmax(logits(q, k), dim=-1)
    return P, P @ v.double()


def forward_fp32(q, k, v):
    """The plain fp32 CPU restatement: (q k^T) alpha, torch.softmax, P v, all in fp32."""
    S = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(q.shape[-1]))
    P = torch.softmax(S, dim=-1)
    return P, P @ v


def slab_error(got, ref):
    """[B, heads] fp64: per slab max |got - ref| / max |ref|; inf where got is not finite.  got, ref: [B, heads, rows, cols]."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    e = (got - ref).abs().flatten(2)
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf"))).amax(-1)
    return e / ref.abs().flatten(2).amax(-1).clamp_min(1e-300)


def forward_bars(r32):
    """The bar of every slab from the restatement's figure of that slab."""
    return (4.0 * r32).clamp(TOL, CAP)


@functools.lru_cache(maxsize=None)
def forward_case(regime, shape):
    """Everything a forward check needs, computed once per (regime, shape) and shared, read-only, by the tests of a session:
    dict(q, k, v, qkv (packed), P, out (fp64 reference), r32_P, r32_out, bar_P, bar_out [B, heads])."""
    q, k, v = operand(regime, *shape)
    P, out = forward_reference(q, k, v)
    P32, out32 = forward_fp32(q, k, v)
    r32_P, r32_out = slab_error(P32, P), slab_error(out32, out)
    return dict(q=q, k=k, v=v, qkv=pack_qkv(q, k, v), P=P, out=out, r32_P=r32_P, r32_out=r32_out,
                bar_P=forward_bars(r32_P), bar_out=forward_bars(r32_out))


def forward_failures(tag, regime, shape, got_P, got_out, out, ledger=None):
    """Prints the figures of a forward check beside their bars and appends to `out` a line per quantity with a slab beyond its bar.
    got_P, got_out: [B, heads, L, L], [B, heads, L, ch].  ledger: {(tag, regime of the slab, quantity): worst figure}."""
    c = forward_case(regime, shape)
    names = slab_regimes(regime, shape[0], shape[1])
    for what, got, ref, bar in (("P", got_P, c["P"], c["bar_P"]), ("out", got_out, c["out"], c["bar_out"])):
        e = slab_error(got, ref)
        ratio = e / bar
        worst = ratio.argmax().item()
        b, h = divmod(worst, e.shape[1])
        print(f"{tag:12s} {str(shape):20s} {regime:10s} {what:3s} err {e.max().item():.2e}  worst/bar {ratio.max().item():.3f} "
              f"(slab {b},{h}: {e[b, h].item():.2e} vs bar {bar[b, h].item():.2e})")
        if ledger is not None:
            for i, name in enumerate(names):
                key = (tag, name, what)
                ledger[key] = max(ledger.get(key, 0.0), e.flatten()[i].item())
        if not (ratio < 1.0).all():
            out.append(f"{tag} {shape} {regime} {what}: {e[b, h].item():.3e} >= {bar[b, h].item():.3e} (image {b}, head {h})")


# ---------------------------------------------------------------------------------------------------- softmax backward
def backward_operand(regime, Z, L, ch, seed=BWD_SEED):
    """fp32 (P, dP) [Z, L, L]: P the fp32 rounding of the fp64 softmax (what the training plan keeps), dP the fp32 rounding of
    datt v^T with datt standard normal."""
    q, k, v = operand(regime, 1, Z, L, ch, seed)
    gen = torch.Generator().manual_seed(8000 + seed)
    datt = torch.randn(Z, L, ch, generator=gen, dtype=torch.float64).float()
    P = torch.softmax(logits(q, k)[0], dim=-1).float()
    dP = (datt.double() @ v[0].double().transpose(-1, -2)).float()
    return P, dP


def backward_reference(P, dP):
    """fp64 dS = P o (dP - rowsum(P o dP)) of the fp32 operands."""
    P, dP = P.double(), dP.double()
    return P * (dP - (P * dP).sum(-1, keepdim=True))


def backward_fp32(P, dP):
    dot = (P * dP).sum(-1, keepdim=True)
    return P * (dP - dot)


def row_error(got, ref, P, dP):
    """[..., rows] fp64: per row max_j |got - ref| / (max_j P * max_j |dP|); inf where got is not finite."""
    e = (got.detach().double().cpu() - ref).abs()
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf"))).amax(-1)
    return e / (P.double().amax(-1) * dP.double().abs().amax(-1)).clamp_min(1e-300)


def one_hot(P):
    """fp32 P rounded to one-hot bit for bit: 1.0 at every row's maximum, 0.0 elsewhere."""
    return torch.zeros_like(P).scatter_(-1, P.argmax(-1, keepdim=True), 1.0)


@functools.lru_cache(maxsize=None)
def backward_case(regime, shape):
    """dict(P, dP (fp32), dS (fp64 reference), r32 [Z, L]), computed once per (regime, shape)."""
    P, dP = backward_operand(regime, *shape)
    dS = backward_reference(P, dP)
    return dict(P=P, dP=dP, dS=dS, r32=row_error(backward_fp32(P, dP), dS, P, dP))
