"""The forward ledger: every launch of an inference plan's op list (_Plan.ops) recomputed in fp64 from the buffers it actually read,
and the plan's wiring checked from the structs alone.  Shared by tests/test_forward_reference.py (CPU: the fp64 statements against
stock fp64 torch.nn.functional, hand-made struct lists with one seeded defect each) and tests/test_gpu_forward_ledger.py (device:
real plans after a poison step).  No device and no project kernel is needed here.  Region, AddressMap, overlaps, block_figure,
tensor_figure, silu and resample are those of backward_ledger.py; the fused-layer `reference` of conv_cases.py (NCHW, F.conv2d) is
what test_forward_reference.py holds `fused_conv` to -- the ledger itself states the convolution as shifted matrix products on NHWC
regions, the form backward_ledger.py uses, because the references of a real plan are contracted in fp64 on the device.

  1. pointers    every pointer of every struct resolves, with its own strides / pitches / offsets, into ONE tensor the plan keeps
                 (or the caller's x / t, or a parameter); unresolved or out of bounds = failure
  2. statements  what each forward op code computes (include/anoddpm_hip.h), in fp64, from the fp32 buffers the launch read
  3. wiring      from the structs, before any arithmetic: a statistics pointer a finalize / fold / tail reads is the statistics
                 buffer of exactly the tensor it normalises, with the row count and format that tensor's producer wrote, and the
                 producer comes first; every buffer has one writer, which comes before its first reader (the caller's input, the
                 packed weights and the frequency table excepted); no output overlaps an input of its launch (the in-place softmax
                 is inside its launch group: scores, softmax and P v are audited as one) or another launch's output (the shared
                 split-K workspace is scratch of each launch that addresses it, and nobody's operand); a split-K launch's
                 ksplit * Z * P * N floats fit its workspace; a ResBlock's first convolution reads ITS columns of the batched
                 embedding projection with that launch's pitch
  4. figures     block_figure per image and block of 64 channels.  Statistics (rows summed over the row axis in fp64, fp64
                 csum / asum accumulators) against the fp64 per-channel sum and sum of squares of the producer's OUTPUT BUFFER,
                 relative to the sum of |.|; a scale / shift pair by x * scale + shift on the actual source buffers against fp64
                 group_norm of those buffers

Bars: the constants of backward_ledger.py and of the operator tests they are named after; none is new."""
import math

import torch

from anoddpm_amd import _lib
from backward_ledger import (BAR_CONV1, BAR_CONV3, BAR_GN, BAR_HEAD, BAR_RESAMPLE, BAR_SOFTMAX, BAR_WINO, AddressMap, LedgerError, Region,
                             attn_gemm, block_figure, block_max, overlaps, resample, silu, tensor_figure)

BAR_LINEAR = 2e-5        # TOL of test_gpu_ops.py::test_linear_small
BAR_STEM = BAR_HEAD      # test_stem, test_head_conv: TOL
BAR_ATTN = BAR_CONV1     # test_fused_attention, test_attention_legacy_order: TOL
BAR_STATS = 1e-5         # test_stem_fused_groupnorm_sums: relative to the sum of |.|
BAR_POSEMB = 2e-6        # test_posemb_matches_reference_expression: absolute
BAR_ACT = 2e-5           # test_resample_pooled_activated_operand: TOL (the plain outputs of a resample: BAR_RESAMPLE)
BAR_COPY = BAR_RESAMPLE  # OP_LAYOUT moves data as the resample modes do

PACK = {"conv3": 0, "wino": 1, "conv1": 2, "small": 3, "copy": 4, "wino43": 5, "wino43b": 6}       # unet.PACK_KINDS + the bf16 planes

__all__ = ["ForwardLedger", "PlanView", "Region", "AddressMap", "overlaps", "block_figure", "tensor_figure", "silu", "resample"]


# ============================================================================================================ 1. pointers
class SpanMap(AddressMap):
    """AddressMap whose regions resolve into the smallest kept tensor that holds the WHOLE region: a plan keeps views of its own
    buffers (the rows of the concatenated embedding weights), so the smallest tensor around the first byte need not be the one."""

    def region(self, ptr, shape, strides, what=""):
        if not ptr:
            raise LedgerError(f"null pointer where a buffer is expected ({what})")
        shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        if any(s < 1 for s in shape) or any(s < 0 for s in strides):
            raise LedgerError(f"{what}: bad shape {shape} / strides {strides}")
        last = sum((n - 1) * s for n, s in zip(shape, strides))
        best, holds = None, False
        for lo, hi, t, name in self.ents:
            if lo <= ptr < hi:
                holds = True
                if ptr + (last + 1) * t.element_size() <= hi and (best is None or hi - lo < best[1] - best[0]):
                    best = (lo, hi, t, name)
        if best is None:
            raise LedgerError(f"{what}: pointer {ptr:#x} " + (f"reaches element {last} past the end of every tensor that holds it" if holds
                                                               else "resolves to no tensor of the plan"))
        lo, _, t, name = best
        if (ptr - lo) % t.element_size():
            raise LedgerError(f"{what}: pointer {ptr:#x} is not aligned to the elements of {name}")
        return Region(ptr, t, (ptr - lo) // t.element_size(), shape, strides, f"{what}:{name}" if what else name)


class PlanView:
    """What the ledger reads of a plan: ops [(code, struct)], keep (tensors), named {parameter name: tensor}, packs
    {pointer: (parameter name, PACK kind, floats)}, x, t."""

    def __init__(self, ops, keep, named, packs, x=None, t=None):
        self.ops, self.keep, self.named, self.packs, self.x, self.t = ops, keep, named, packs, x, t

    @classmethod
    def of(cls, plan, x, t):
        """A real _Plan after a run with the caller's (contiguous fp32) x and (int64) t."""
        named = {k: p.detach() for k, p in plan.model.named_parameters()}
        packs = {}
        for key, st in plan._pack_jobs:
            n = named[key].numel() if st.kind == PACK["copy"] else {0: 9, 1: 16, 2: 1, 3: 9, 5: 36}[st.kind] * st.N * st.K
            packs[st.out] = (key, st.kind, n)
        for key, dst, N, K in plan._bf16_jobs:
            packs[dst.data_ptr()] = (key, PACK["wino43b"], dst.numel())
        return cls(plan.ops, [k for k in plan.keep if torch.is_tensor(k)], named, packs, x, t)


# ============================================================================================================ 2. fp64 statements
def posemb(t, freqs, dim, scale=1.0):
    """UNet.py:50-57 as anoddpm_posemb states it: the argument is ONE fp32 product (as torch.outer forms it); sin / cos in fp64."""
    arg = ((t.to(torch.float32) * float(scale))[:, None] * freqs.to(torch.float32)[None, :]).double()
    return torch.cat([arg.sin(), arg.cos()], dim=1)[:, :dim]


def linear(x, w, bias, act_in, act_out):
    y = (silu(x) if act_in else x) @ w.T
    if bias is not None:
        y = y + bias
    return silu(y) if act_out else y


def conv_nhwc(h, w):
    """h NHWC [B, H, W, K], w OIHW [N, K, ks, ks] (or [N, K] / [N, K, 1]) -> [B, H, W, N]; stride 1, zero padding ks // 2."""
    if w.dim() < 4 or w.shape[2] == 1:
        return h @ w.reshape(w.shape[0], w.shape[1]).T
    B, H, W, K = h.shape
    p = torch.nn.functional.pad(h, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(B, H, W, w.shape[0], dtype=h.dtype, device=h.device)
    for ky in range(3):
        for kx in range(3):
            out += p[:, ky:ky + H, kx:kx + W, :] @ w[:, :, ky, kx].T
    return out


def group_norm_nhwc(x, gamma, beta, groups=32, eps=1e-5):
    """nn.GroupNorm(groups, C) of x [B, ..., C] (channels last): biased variance over a group's channels and all pixels."""
    B, C = x.shape[0], x.shape[-1]
    xg = x.reshape(B, -1, groups, C // groups)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    return ((xg - mean) / torch.sqrt(var + eps)).reshape(x.shape) * gamma + beta


def fused_conv(xs, w, *, affine=None, act=0, a_mode=0, bias=None, temb=None, res=None, res_mode=0, alpha=1.0):
    """anoddpm_igemm with packed weights (b_mode 0): xs = the one or two NHWC sources [B, Hin, Win, c], concatenated along channels;
    affine None | ("affine", scale [B, K], shift [B, K]) | ("gn", gamma, beta, groups, eps) -> SiLU -> nearest x2 (a_mode 1) | 2 x 2
    average (a_mode 2) -> convolution -> * alpha + bias + temb[b] + res (res_mode 1: a half-resolution residual repeated 2 x 2)."""
    h = torch.cat(list(xs), dim=-1)
    if affine is not None and affine[0] == "gn":
        h = group_norm_nhwc(h, affine[1], affine[2], affine[3], affine[4])
    elif affine is not None:
        h = h * affine[1][:, None, None, :] + affine[2][:, None, None, :]
    if act:
        h = silu(h)
    if a_mode:
        h = resample(h, a_mode)
    y = conv_nhwc(h, w) * alpha
    if bias is not None:
        y = y + bias
    if temb is not None:
        y = y + temb[:, None, None, :]
    if res is not None:
        y = y + (resample(res, 1) if res_mode == 1 else res)
    return y


def attention(qkv, heads, ch, scale):
    """QKVAttentionLegacy (UNet.py:137-153): qkv [B, L, 3 * heads * ch], head h holds q at channel 3 h ch, k at + ch, v at + 2 ch.
    Returns (out [B, L, heads * ch], probs [B, heads, L, L])."""
    B, L, _ = qkv.shape
    q, k, v = qkv.reshape(B, L, heads, 3, ch).permute(3, 0, 2, 1, 4)
    p = torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1)
    return (p @ v).permute(0, 2, 1, 3).reshape(B, L, heads * ch), p


def stem(x, w, bias):
    """x NCHW [B, Ci, H, W], w OIHW -> NHWC [B, H, W, Co]"""
    return conv_nhwc(x.permute(0, 2, 3, 1), w) + bias


def head(x, scale, shift, w, bias):
    """x NHWC [B, H, W, C] -> silu(x * scale + shift) -> 3x3 -> NCHW [B, Co, H, W]"""
    y = fused_conv([x], w, affine=("affine", scale, shift), act=1, bias=bias)
    return y.permute(0, 3, 1, 2)


def chan_sums(y):
    """y [B, P, C] -> (sums [B, C, 2] = {sum, sum of squares} over the pixels, their scale [B, C, 2] = {sum |y|, sum y^2})"""
    q = (y * y).sum(dim=1)
    return torch.stack([y.sum(dim=1), q], dim=-1), torch.stack([y.abs().sum(dim=1), q], dim=-1)


def producer_rows(st, smallmap_tile=None):
    """Statistics rows per image the kernel behind an anoddpm_igemm launch WRITES (csrc: the row index of each epilogue), from the
    launch's own fields -- stated apart from the arithmetic of unet.py's igemm(), which sizes the buffer and tells the consumer."""
    P = st.H * st.W
    if st.ksplit > 1:
        return st.stats_rows                                           # splitk_reduce_stats_kernel: grid.x = stats_rows
    if st.cfg in (3, 7):
        return (st.H // 16) * (st.W // 16)                             # one per workgroup of 16 x 16 pixels
    if st.cfg == 2:
        return P // 64                                                 # wino_kernel: (8 WMW) x 16 pixel patches x 2 WMW wave rows
    if st.cfg == 6:
        return (st.H // 8) * (st.W // 8)
    if st.cfg == 5:
        fn = smallmap_tile or _lib.lib().anoddpm_smallmap_tile
        return P // (16 * (fn(st.ks, st.H, st.W, st.c0 + st.c1, st.c0, st.N, st.B) >> 4))
    bm = 128 if st.cfg == 0 else 64                                    # igemm_kernel: two wave rows per pixel tile
    if st.ks == 1:
        return 2 * -(-P // bm)
    tw = min(st.W, 32)
    return 2 * (st.W // tw) * -(-st.H // (bm // tw))


# ============================================================================================================ 3. ledger
class Out:
    def __init__(self, name, region, bar, cls):
        self.name, self.region, self.bar, self.cls = name, region, bar, cls


class Launch:
    def __init__(self, idx, what, cfg=""):
        self.idx, self.what, self.cfg = idx, what, cfg
        self.inputs, self.outs, self.scratch = [], [], []
        self.compute = None          # dev -> {out name: (got [Z, rows, width], ref, den [Z, blocks] | None)}
        self.st = None


def _z3(t):
    return t.reshape(-1, t.shape[-2], t.shape[-1]) if t.dim() >= 3 else t.reshape(t.shape[0], 1, -1)


def _stat3(t):
    """[B, C, 2] -> [2 B, 1, C]: the sums and the sums of squares are judged separately"""
    return t.permute(2, 0, 1).reshape(-1, 1, t.shape[1])


class ForwardLedger:
    def __init__(self, view, dev="cpu", smallmap_tile=None):
        self.view, self.dev, self.smallmap_tile = view, torch.device(dev), smallmap_tile
        am = self.amap = SpanMap()
        for i, t in enumerate(view.keep):
            am.add(t, f"keep[{i}]")
        for k, p in view.named.items():
            am.add(p, k)
        am.add(view.x, "x")
        am.add(view.t, "t")
        self.external = [(p.data_ptr(), p.data_ptr() + p.numel() * p.element_size()) for p in list(view.named.values()) + [view.x, view.t] if p is not None]
        self.external += [(ptr, ptr + 4 * n) for ptr, (_, _, n) in view.packs.items()]
        self.launches, self.static, self.undescribed = [], [], []
        self.stats_of = {}           # statistics pointer -> dict(tensor=Region, fmt, rows, C, idx)
        self.affine = {}             # scale pointer -> dict(shift, srcs=[Region], idx, C)
        self.linears = []            # (launch index, struct, out region, [(row offset, key)])
        self.copy_checks = []        # (region, [(offset, parameter name)]): a packed "copy" buffer equals its parameters
        self.zeroed = None           # (first byte, one past the last) the plan's first op clears
        self.routes = set()
        self._describe_all()

    # ------------------------------------------------------------------ helpers
    def reg(self, ptr, shape, strides, what):
        return self.amap.region(ptr, shape, strides, what)

    def copy_of(self, ptr, n, what, shape=None):
        """`n` floats at ptr that are packed copies of parameters (bias, gamma, beta, linear weights): (region, [(offset, name)])."""
        r = self.reg(ptr, shape or (n,), (shape[1], 1) if shape else (1,), what)
        jobs = sorted(((p - ptr) // 4, key, cnt) for p, (key, kind, cnt) in self.view.packs.items() if kind == PACK["copy"] and ptr <= p < ptr + 4 * n)
        at = 0
        for off, key, cnt in jobs:
            if off != at or cnt != self.view.named[key].numel():
                break
            at += cnt
        if at != n:
            raise LedgerError(f"{what}: {n} floats at {ptr:#x} are not tiled by packed copies of parameters")
        self.copy_checks.append((r, [(off, key) for off, key, _ in jobs]))
        return r, [(off, key) for off, key, _ in jobs]

    def param_pair(self, wptr, bptr, C, what):
        """gamma / beta (or any .weight / .bias pair) of ONE module"""
        g, gk = self.copy_of(wptr, C, what + ".gamma")
        b, bk = self.copy_of(bptr, C, what + ".beta")
        if len(gk) != 1 or len(bk) != 1 or not gk[0][1].endswith(".weight") or bk[0][1] != gk[0][1][:-7] + ".bias":
            raise LedgerError(f"{what}: affine parameters {gk} / {bk} are not the weight and bias of one GroupNorm")
        return g, b, gk[0][1][:-7]

    def weight(self, bmat, want, N, K, ks, what):
        ent = self.view.packs.get(bmat)
        if ent is None:
            raise LedgerError(f"{what}: bmat {bmat:#x} is the output of no pack job")
        key, kind, n = ent
        w = self.view.named[key]
        ok = w.shape[0] == N and w.shape[1] == K and ((w.dim() == 4 and w.shape[2] == ks) or (w.dim() == 3 and ks == 1))
        if kind != want or not ok:
            raise LedgerError(f"{what}: packed weight {key} {tuple(w.shape)} in layout {kind} does not fit N={N} K={K} ks={ks} (layout {want})")
        return self.reg(w.data_ptr(), tuple(w.shape), tuple(w.stride()), what + ".w=" + key), self.reg(bmat, (n,), (1,), what + ".bmat"), key

    def bias_of(self, ptr, N, wkey, what):
        if not ptr:
            return None
        r, keys = self.copy_of(ptr, N, what + ".bias")
        if len(keys) != 1 or keys[0][1] != wkey[:-7] + ".bias":
            raise LedgerError(f"{what}: bias {keys} is not the bias of {wkey}")
        return r

    def new_stats(self, ptr, tensor, fmt, rows, idx, what):
        C = tensor.shape[-1]
        B = tensor.shape[0]
        r = self.reg(ptr, (B, C, 2) if fmt else (B, rows, C, 2), (C * 2, 2, 1) if fmt else (rows * C * 2, C * 2, 2, 1), what)
        if (r.tensor.dtype == torch.float64) != bool(fmt):
            raise LedgerError(f"{what}: {r} holds {r.tensor.dtype} for statistics format {fmt}")
        if not fmt and r.numel != r.tensor.numel():
            raise LedgerError(f"{what}: the producer writes {rows} rows per image, the buffer {r} has room for {r.tensor.numel() // (B * C * 2)}")
        self.stats_of[ptr] = dict(tensor=tensor, fmt=fmt, rows=rows, C=C, idx=idx, region=r)
        return r

    def stats_source(self, ptr, rows, fmt, src, idx, what):
        """The statistics a finalize / fold / tail reads at `ptr` are those of tensor `src` (None: whatever tensor they describe)."""
        ent = self.stats_of.get(ptr)
        if ent is None:
            raise LedgerError(f"{what}: statistics pointer {ptr:#x} is the statistics buffer of no tensor written so far")
        if src is not None and ent["tensor"].key != src.key:
            raise LedgerError(f"{what}: reads the statistics of {ent['tensor']}, but normalises {src}")
        if ent["fmt"] != fmt:
            raise LedgerError(f"{what}: format {fmt} for statistics their producer wrote in format {ent['fmt']}")
        if not fmt and ent["rows"] != rows:
            raise LedgerError(f"{what}: reads {rows} statistics rows, the producer (ops[{ent['idx']}]) wrote {ent['rows']}")
        if ent["idx"] >= idx:
            raise LedgerError(f"{what}: the statistics' producer ops[{ent['idx']}] does not come first")
        return ent

    def affine_use(self, scale, shift, srcs, K, idx, what):
        ent = self.affine.get(scale)
        if ent is None:
            raise LedgerError(f"{what}: gn_scale {scale:#x} is written by no earlier finalize / tail")
        if ent["shift"] != shift or ent["C"] != K or ent["idx"] >= idx:
            raise LedgerError(f"{what}: gn_scale / gn_shift are not the pair of ops[{ent['idx']}] over {ent['C']} channels")
        if [r.key for r in ent["srcs"]] != [r.key for r in srcs]:
            raise LedgerError(f"{what}: its affine (ops[{ent['idx']}]) normalises {ent['srcs']}, the launch reads {srcs}")
        return (self.reg(scale, (srcs[0].shape[0], K), (K, 1), what + ".gn_scale"), self.reg(shift, (srcs[0].shape[0], K), (K, 1), what + ".gn_shift"))

    # ------------------------------------------------------------------ descriptions
    def _describe_all(self):
        ops, i = self.view.ops, 0
        table = {_lib.OP_POSEMB: self._posemb, _lib.OP_LINEAR: self._linear, _lib.OP_STEM: self._stem, _lib.OP_CHAN_STATS: self._chan_stats,
                 _lib.OP_GN_FINALIZE: self._finalize, _lib.OP_RESAMPLE: self._resample, _lib.OP_ATTENTION: self._attention,
                 _lib.OP_HEAD: self._head, _lib.OP_LAYOUT: self._layout}
        while i < len(ops):
            code, st = ops[i]
            n = 1
            try:
                if code == _lib.OP_IGEMM and st.b_mode in (1, 2):
                    n = 3
                    L = self._attention_chain(i)
                elif code == _lib.OP_IGEMM:
                    L = self._conv(i, st)
                elif code in table:
                    L = table[code](i, st)
                else:
                    raise LedgerError(f"ops[{i}]: op code {code} has no fp64 statement in the forward ledger")
                L.st = st
                self.launches.append(L)
            except LedgerError as e:
                self.static.append(f"ops[{i}]: {e}")
                self.undescribed.append(i)
                n = 1
            i += n

    def _posemb(self, i, st):
        what = f"ops[{i}] POSEMB"
        L = Launch([i], f"posemb B={st.B} dim={st.dim}")
        t = self.reg(st.t, (st.B,), (1,), what + ".t")
        fr = self.reg(st.freqs, (st.dim // 2,), (1,), what + ".freqs")
        out = self.reg(st.out, (st.B, st.dim), (st.dim, 1), what + ".out")
        if t.tensor.dtype != torch.int64:
            raise LedgerError(f"{what}: timesteps are int64")
        self.external.append(fr.span())
        L.inputs += [t, fr]
        L.outs.append(Out("out", out, BAR_POSEMB, "posemb"))
        if st.zero_doubles:
            z = self.reg(st.zero, (st.zero_doubles,), (1,), what + ".zero")
            if z.tensor.dtype != torch.float64 or i != 0:
                raise LedgerError(f"{what}: the accumulator arena is fp64 and is cleared by the plan's FIRST op")
            self.zeroed = z.span()
            self.routes.add("arena cleared by posemb")
        dim, scale = st.dim, st.scale

        def compute(dev):
            ref = posemb(t.raw().to(dev), fr.raw().to(dev), dim, scale)
            return {"out": (_z3(out.read(dev)), _z3(ref), torch.ones(st.B, -(-dim // 64), dtype=torch.float64, device=dev))}
        L.compute = compute
        return L

    def _linear(self, i, st):
        what = f"ops[{i}] LINEAR"
        B, K, N = st.B, st.K, st.N
        L = Launch([i], f"linear B={B} K={K} N={N} act_in={st.act_in} act_out={st.act_out}")
        x = self.reg(st.inp, (B, K), (K, 1), what + ".in")
        w, wkeys = self.copy_of(st.w, N * K, what + ".w", shape=(N, K))
        b, bkeys = self.copy_of(st.bias, N, what + ".bias") if st.bias else (None, [])
        for (wo, wk), (bo, bk) in zip(wkeys, bkeys):
            if wo != bo * K or not wk.endswith(".weight") or bk != wk[:-7] + ".bias":
                raise LedgerError(f"{what}: weight rows {wkeys} and bias entries {bkeys} are not those of the same modules in the same order")
        if b is not None and len(wkeys) != len(bkeys):
            raise LedgerError(f"{what}: {len(wkeys)} weights, {len(bkeys)} biases")
        out = self.reg(st.out, (B, N), (N, 1), what + ".out")
        L.inputs += [x, w] + ([b] if b is not None else [])
        L.outs.append(Out("out", out, BAR_LINEAR, "linear"))
        self.linears.append((i, st, out, [(o // K, k) for o, k in wkeys]))
        if len(wkeys) > 1:
            self.routes.add("batched embedding projection")
        ai, ao = st.act_in, st.act_out
        L.compute = lambda dev: {"out": (_z3(out.read(dev)), _z3(linear(x.read(dev), w.read(dev), b.read(dev) if b is not None else None, ai, ao)), None)}
        return L

    def _stat_out(self, L, name, ptr, tensor, fmt, rows, idx, what):
        r = self.new_stats(ptr, tensor, fmt, rows, idx, what)
        L.outs.append(Out(name, r, BAR_STATS, "statistics " + ("fp64" if fmt else "rows")))
        return r

    @staticmethod
    def _stat_figure(r, fmt, y, dev):
        """(got, ref, den) of a statistics region against the tensor values y [B, P, C] (fp64)"""
        got = r.read(dev)
        ref, scale = chan_sums(y)
        return _stat3(got if fmt else got.sum(dim=1)), _stat3(ref), block_max(_stat3(scale))

    def _stem(self, i, st):
        what = f"ops[{i}] STEM"
        B, H, W, Ci, Co = st.B, st.H, st.W, st.Cin, st.Cout
        L = Launch([i], f"stem B={B} {H}x{W} Cin={Ci} Cout={Co}" + (f" stats_rows={st.stats_rows}" if st.stats else ""))
        x = self.reg(st.x, (B, Ci, H * W), (Ci * H * W, H * W, 1), what + ".x")
        w, pk, wkey = self.weight(st.w, PACK["small"], Co, Ci, 3, what)
        b = self.bias_of(st.bias, Co, wkey, what)
        out = self.reg(st.out, (B, H * W, Co), (H * W * Co, Co, 1), what + ".out")
        L.inputs += [x, w, pk] + ([b] if b is not None else [])
        L.outs.append(Out("out", out, BAR_STEM, "stem"))
        srow = self._stat_out(L, "stats", st.stats, out, 0, st.stats_rows, i, what + ".stats") if st.stats else None
        if srow is not None:
            self.routes.add("statistics: stem rows")

        def compute(dev):
            ref = stem(x.read(dev).reshape(B, Ci, H, W), w.read(dev), b.read(dev) if b is not None else 0.0).reshape(B, H * W, Co)
            r = {"out": (out.read(dev), ref, None)}
            if srow is not None:
                r["stats"] = self._stat_figure(srow, 0, out.read(dev), dev)
            return r
        L.compute = compute
        return L

    def _chan_stats(self, i, st):
        what = f"ops[{i}] CHAN_STATS"
        B, C, P = st.B, st.C, st.P
        L = Launch([i], f"chan_stats B={B} P={P} C={C} nslab={st.nslab}")
        a = self.reg(st.a, (B, P, C), (st.a_bs, st.a_ld, 1), what + ".a")
        L.inputs.append(a)
        srow = self._stat_out(L, "stats", st.stats, a, 0, st.nslab, i, what + ".stats")
        self.routes.add("statistics: chan_stats rows")
        L.compute = lambda dev: {"stats": self._stat_figure(srow, 0, a.read(dev), dev)}
        return L

    def _affine_out(self, L, scale, shift, srcs, gamma, beta, groups, eps, idx, what):
        """scale / shift [B, C] written by a finalize or a tail over the tensors `srcs`: judged as x * scale + shift against fp64
        group_norm(x) of the source buffers."""
        B, C = srcs[0].shape[0], sum(r.shape[-1] for r in srcs)
        sc, sh = self.reg(scale, (B, C), (C, 1), what + ".scale"), self.reg(shift, (B, C), (C, 1), what + ".shift")
        if C % groups:
            raise LedgerError(f"{what}: {C} channels in {groups} groups")
        L.outs += [Out("scale", sc, BAR_GN, "groupnorm affine"), Out("shift", sh, BAR_GN, "groupnorm affine")]
        self.affine[scale] = dict(shift=shift, srcs=list(srcs), idx=idx, C=C)

        def figures(dev):
            x = torch.cat([r.read(dev) for r in srcs], dim=-1)
            ref = group_norm_nhwc(x, gamma.read(dev), beta.read(dev), groups, eps)
            got = x * sc.read(dev)[:, None, :] + sh.read(dev)[:, None, :]
            # one figure for the pair (a scale alone has no reference): reported under both names
            return {"scale": (got, ref, None), "shift": (got, ref, None)}
        return figures

    def _finalize(self, i, st):
        what = f"ops[{i}] GN_FINALIZE"
        B, c0, c1 = st.B, st.c0, st.c1
        L = Launch([i], f"gn_finalize B={B} C={c0}+{c1} P={st.P} rows={st.rows0}/{st.rows1} fmt={st.fmt0}/{st.fmt1}")
        ents = [self.stats_source(st.stats0, st.rows0, st.fmt0, None, i, what + ".stats0")]
        if c1:
            ents.append(self.stats_source(st.stats1, st.rows1, st.fmt1, None, i, what + ".stats1"))
        for e, c in zip(ents, (c0, c1)):
            if e["C"] != c or e["tensor"].shape[0] != B or e["tensor"].shape[1] != st.P:
                raise LedgerError(f"{what}: c / B / P = {c} / {B} / {st.P} over the statistics of {e['tensor']}")
            L.inputs.append(e["region"])
        srcs = [e["tensor"] for e in ents]
        gamma, beta, _ = self.param_pair(st.gamma, st.beta, c0 + c1, what)
        L.inputs += [gamma, beta]                              # (the tensors are read by the ledger's statement, not by the launch)
        if st.mean_out or st.rstd_out:
            raise LedgerError(f"{what}: mean / rstd outputs are a training form")
        L.compute = self._affine_out(L, st.scale, st.shift, srcs, gamma, beta, st.groups, st.eps, i, what)
        self.routes.add(f"finalize fmt {st.fmt0}" + (f"+{st.fmt1}" if c1 else ""))
        return L

    def _resample(self, i, st):
        what = f"ops[{i}] RESAMPLE"
        B, H, W, C, mode = st.B, st.H, st.W, st.C, st.mode
        if mode not in (1, 2, 3) or st.accumulate:
            raise LedgerError(f"{what}: mode {mode} / accumulate {st.accumulate} is a backward form")
        Ho, Wo = (2 * H, 2 * W) if mode == 1 else (H // 2, W // 2)
        L = Launch([i], f"resample mode={mode} B={B} {H}x{W}x{C}" + (" +out_act" if st.out_act else ""))
        inp = self.reg(st.inp, (B, H * W, C), (H * W * C, C, 1), what + ".in")
        out = self.reg(st.out, (B, Ho * Wo, C), (Ho * Wo * C, C, 1), what + ".out")
        L.inputs.append(inp)
        L.outs.append(Out("out", out, BAR_RESAMPLE, "resample"))
        act = aff = None
        if st.out_act or st.gn_scale:
            if mode != 2 or not (st.out_act and st.gn_scale and st.gn_shift):
                raise LedgerError(f"{what}: the activated second output is a mode-2 form with scale, shift and out_act")
            aff = self.affine_use(st.gn_scale, st.gn_shift, [inp], C, i, what)
            act = self.reg(st.out_act, (B, Ho * Wo, C), (Ho * Wo * C, C, 1), what + ".out_act")
            L.inputs += list(aff)
            L.outs.append(Out("out_act", act, BAR_ACT, "resample out_act"))
            self.routes.add("pool_act double output")
        self.routes.add(f"resample mode {mode}")
        scale = st.scale

        def compute(dev):
            x = inp.read(dev).reshape(B, H, W, C)
            r = {"out": (out.read(dev), resample(x, mode, scale).reshape(B, Ho * Wo, C), None)}
            if act is not None:
                h = silu(x * aff[0].read(dev)[:, None, None, :] + aff[1].read(dev)[:, None, None, :])
                r["out_act"] = (act.read(dev), resample(h, 2, scale).reshape(B, Ho * Wo, C), None)
            return r
        L.compute = compute
        return L

    def _attention(self, i, st):
        what = f"ops[{i}] ATTENTION"
        B, Lq, heads, ch = st.B, st.L, st.heads, st.ch
        C = heads * ch
        L = Launch([i], f"attention B={B} heads={heads} L={Lq} ch={ch}")
        qkv = self.reg(st.qkv, (B, Lq, 3 * C), (Lq * 3 * C, 3 * C, 1), what + ".qkv")
        out = self.reg(st.out, (B, Lq, C), (Lq * C, C, 1), what + ".out")
        L.inputs.append(qkv)
        L.outs.append(Out("out", out, BAR_ATTN, "attention"))
        if st.probs:
            raise LedgerError(f"{what}: the probability output is a training form")
        if abs(st.scale - 1.0 / math.sqrt(ch)) > 1e-6 / math.sqrt(ch):
            raise LedgerError(f"{what}: scale {st.scale} is not ch^-1/2")
        self.routes.add("attention: fused")
        scale = float(st.scale)
        L.compute = lambda dev: {"out": (out.read(dev), attention(qkv.read(dev), heads, ch, scale)[0], None)}
        return L

    def _attention_chain(self, i):
        """ops[i .. i + 2]: S = alpha q k^T; S <- softmax(S) in place; att = S v.  One launch group: the scores are gone when the
        ledger reads the buffers.  The probabilities against softmax(alpha q k^T) of qkv; att against the ACTUAL probabilities."""
        ops = self.view.ops
        what = f"ops[{i}..{i + 2}] attention chain"
        if i + 3 > len(ops) or [c for c, _ in ops[i:i + 3]] != [_lib.OP_IGEMM, _lib.OP_SOFTMAX, _lib.OP_IGEMM]:
            raise LedgerError(f"{what}: an activation-operand IGEMM outside the IGEMM / SOFTMAX / IGEMM chain has no statement")
        g1, sm, g2 = [s for _, s in ops[i:i + 3]]
        B, heads, Lq, ch = g1.B, g1.heads, g1.W, g1.c0
        for g in (g1, g2):
            if (g.ks != 1 or g.H != 1 or g.W != Lq or g.B != B or g.heads != heads or g.gn_scale or g.fold_gamma or g.act or g.bias or g.temb
                    or g.res or g.c1 or g.a_mode or g.stats or g.tail_csum or g.stats_csum):
                raise LedgerError(f"{what}: unexpected GEMM form")

        def A(g, tag):
            return self.reg(g.a0, (B, heads, Lq, g.c0), (g.a0_bs, g.a0_hs, g.a0_ld, 1), f"{what}.{tag}.a")

        def Bm(g, tag):
            rows, cols = (g.N, g.c0) if g.b_mode == 1 else (g.c0, g.N)
            return self.reg(g.bmat, (B, heads, rows, cols), (g.b_bs, g.b_hs, g.ldb, 1), f"{what}.{tag}.b")

        def O(g, tag):
            return self.reg(g.out, (B, heads, Lq, g.N), (g.o_bs, g.o_hs, g.out_ld, 1), f"{what}.{tag}.out")
        q, k, S, P2, v, att = A(g1, "scores"), Bm(g1, "scores"), O(g1, "scores"), A(g2, "att"), Bm(g2, "att"), O(g2, "att")
        ok = (g1.b_mode == 1 and g2.b_mode == 2 and g1.N == Lq and g2.c0 == Lq and g2.N == ch and S.key == P2.key and sm.x == g1.out
              and sm.rows == B * heads * Lq and sm.L == Lq and S.numel == B * heads * Lq * Lq and g2.alpha == 1.0
              and abs(g1.alpha - 1.0 / math.sqrt(ch)) <= 1e-6 / math.sqrt(ch))
        if not ok:
            raise LedgerError(f"{what}: the three launches are not chained through one score buffer as the statement assumes")
        L = Launch([i, i + 1, i + 2], f"attention_chain B={B} heads={heads} L={Lq} ch={ch}", f"cfg={g1.cfg}/{g2.cfg} ksplit={g1.ksplit}/{g2.ksplit}")
        L.inputs += [q, k, v]
        L.outs += [Out("probs", S, BAR_SOFTMAX, "attention chain softmax"), Out("att", att, BAR_ATTN, "attention chain")]
        for g in (g1, g2):
            self._workspace(L, g, what)
        self.routes.add("attention: three launches")
        alpha = float(g1.alpha)

        def compute(dev):
            p = S.read(dev)
            ref = torch.softmax(attn_gemm(q.read(dev), k.read(dev), 1, alpha), dim=-1)
            return {"probs": (_z3(p), _z3(ref), None), "att": (_z3(att.read(dev)), _z3(attn_gemm(p, v.read(dev), 2)), None)}
        L.compute = compute
        return L

    def _workspace(self, L, st, what):
        if st.ksplit > 1:
            n = st.ksplit * st.B * st.heads * st.H * st.W * st.N
            L.scratch.append(self.reg(st.ws, (n,), (1,), what + ".ws"))
            self.routes.add("shared split-K workspace")

    def _conv(self, i, st):
        B, H, W, ks, N, c0, c1, cfg, am = st.B, st.H, st.W, st.ks, st.N, st.c0, st.c1, st.cfg, st.a_mode
        K, P = c0 + c1, st.H * st.W
        what = f"ops[{i}] IGEMM cfg {cfg}"
        if st.heads != 1 or st.alpha != 1.0 or st.gnb_partial or st.o_hs or st.a0_hs:
            raise LedgerError(f"{what}: a packed-weight launch has one head, alpha 1 and no backward fields")
        Hin, Win = {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[am]
        srcs = [self.reg(st.a0, (B, Hin * Win, c0), (st.a0_bs, st.a0_ld, 1), what + ".a0")]
        if c1:
            srcs.append(self.reg(st.a1, (B, Hin * Win, c1), (st.a1_bs, st.a1_ld, 1), what + ".a1"))
        want = {2: "wino", 6: "wino", 3: "wino43", 7: "wino43b"}.get(cfg, "conv3" if ks == 3 else "conv1")
        w, pk, wkey = self.weight(st.bmat, PACK[want], N, K, ks, what)
        wino = cfg in (2, 3, 6, 7)
        cls = f"igemm cfg {cfg} {ks}x{ks}"
        L = Launch([i], f"igemm B={B} {H}x{W} K={c0}+{c1}->N={N} ks={ks} a_mode={am} act={st.act}", f"cfg={cfg} ksplit={st.ksplit}")
        L.inputs += srcs + [w, pk]
        self.routes.add(f"cfg {cfg}")
        # -- operand
        affine = None
        if st.fold_gamma:
            gamma, beta, _ = self.param_pair(st.fold_gamma, st.fold_beta, K, what + ".fold")
            folds = [(st.fold_stats0, st.fold_rows0, st.fold_fmt0)] + ([(st.fold_stats1, st.fold_rows1, st.fold_fmt1)] if c1 else [])
            for k_, ((p_, r_, f_), src) in enumerate(zip(folds, srcs)):
                L.inputs.append(self.stats_source(p_, r_, f_, src, i, f"{what}.fold_stats{k_}")["region"])
            if not (cfg in (5, 6) or (cfg == 3 and st.ksplit == 1 and all(f[2] == 1 for f in folds))):
                raise LedgerError(f"{what}: a folded GroupNorm needs a cfg 5 / 6 consumer, or a cfg 3 one over fp64 sums")
            L.inputs += [gamma, beta]
            affine = ("gn", gamma, beta, st.fold_groups, st.fold_eps)
            L.what += " fold" + "".join(str(f[2]) for f in folds)
            self.routes.add("fold: fp64 sums" if folds[0][2] else "fold: rows")
        elif st.gn_scale:
            if st.gn_ld != K:
                raise LedgerError(f"{what}: gn_ld {st.gn_ld} over {K} channels")
            sc, sh = self.affine_use(st.gn_scale, st.gn_shift, srcs, K, i, what)
            L.inputs += [sc, sh]
            affine = ("affine", sc, sh)
            L.what += " gn"
        # -- epilogue
        bias = self.bias_of(st.bias, N, wkey, what)
        temb = None
        if st.temb:
            temb = self.reg(st.temb, (B, N), (st.temb_ld, 1), what + ".temb")
            L.inputs.append(temb)
        self._temb_wiring(st, wkey, what)
        res = None
        if st.res:
            if st.res_mode not in (0, 1) or (st.res_mode == 1 and (cfg != 3 or st.ksplit != 1)):
                raise LedgerError(f"{what}: res_mode {st.res_mode}")
            res = self.reg(st.res, (B, P // 4 if st.res_mode else P, N), (st.r_bs, st.res_ld, 1), what + ".res")
            L.inputs.append(res)
            self.routes.add(f"res_mode {st.res_mode}")
        if bias is not None:
            L.inputs.append(bias)
        out = self.reg(st.out, (B, P, N), (st.o_bs, st.out_ld, 1), what + ".out")
        L.outs.append(Out("out", out, BAR_WINO if wino else (BAR_CONV3 if ks == 3 else BAR_CONV1), cls))
        self._workspace(L, st, what)
        if st.ksplit > 1:
            self.routes.add(f"cfg {cfg} split-K")
        # -- statistics
        stat = []                                             # (out name, region, fmt)
        if st.stats:
            if st.tail_csum or st.stats_csum:
                raise LedgerError(f"{what}: statistics rows together with fp64 sums")
            rows = producer_rows(st, self.smallmap_tile)
            stat.append(("stats", self._stat_out(L, "stats", st.stats, out, 0, rows, i, what + ".stats"), 0))
            self.routes.add("statistics: split-K rows" if st.ksplit > 1 else f"statistics: cfg {cfg} rows")
        elif st.stats_rows:
            raise LedgerError(f"{what}: stats_rows without statistics")
        if st.stats_csum:
            if cfg != 3 or st.ksplit != 1:
                raise LedgerError(f"{what}: stats_csum is a cfg 3 feature without split-K")
            r = self._stat_out(L, "stats_csum", st.stats_csum, out, 1, 1, i, what + ".stats_csum")
            if self.zeroed is None or not (self.zeroed[0] <= r.span()[0] and r.span()[1] <= self.zeroed[1]):
                raise LedgerError(f"{what}: the atomic accumulator {r} lies outside what the plan's first op clears")
            stat.append(("stats_csum", r, 1))
            self.routes.add("statistics: asum")
        tail = None
        if st.tail_csum:
            if st.ksplit < 2:
                raise LedgerError(f"{what}: the GroupNorm tail needs split-K")
            stat.append(("tail_csum", self._stat_out(L, "tail_csum", st.tail_csum, out, 1, 1, i, what + ".tail_csum"), 1))
            self.routes.add("statistics: csum")
            if st.tail_gamma:
                C = N + st.tail_c1
                tsrcs = [out]
                if st.tail_c1:
                    e = self.stats_source(st.tail_other, 1, 1, None, i, what + ".tail_other")
                    if e["C"] != st.tail_c1 or e["tensor"].shape[:2] != out.shape[:2]:
                        raise LedgerError(f"{what}: tail_c1 {st.tail_c1} over the sums of {e['tensor']}")
                    tsrcs.append(e["tensor"])
                    L.inputs.append(e["region"])
                elif st.tail_other:
                    raise LedgerError(f"{what}: tail_other without tail_c1")
                g_, b_, _ = self.param_pair(st.tail_gamma, st.tail_beta, C, what + ".tail")
                L.inputs += [g_, b_]
                if st.tail_mean or st.tail_rstd:
                    raise LedgerError(f"{what}: tail mean / rstd outputs are a training form")
                tail = self._affine_out(L, st.tail_scale, st.tail_shift, tsrcs, g_, b_, st.tail_groups, st.tail_eps, i, what + ".tail")
                self.routes.add("tail-attached GroupNorm")
        elif st.tail_gamma or st.tail_scale:
            raise LedgerError(f"{what}: tail affine without tail_csum")
        act, rm = st.act, st.res_mode

        def compute(dev):
            aff = None if affine is None else (affine[0], affine[1].read(dev), affine[2].read(dev)) + tuple(affine[3:])
            ref = fused_conv([s.read(dev).reshape(B, Hin, Win, -1) for s in srcs], w.read(dev), affine=aff, act=act, a_mode=am,
                             bias=bias.read(dev) if bias is not None else None, temb=temb.read(dev) if temb is not None else None,
                             res=res.read(dev).reshape(B, H // 2 if rm else H, W // 2 if rm else W, N) if res is not None else None, res_mode=rm)
            y = out.read(dev)
            r = {"out": (y, ref.reshape(B, P, N), None)}
            for name, reg_, fmt in stat:
                r[name] = self._stat_figure(reg_, fmt, y, dev)
            if tail is not None:
                r.update(tail(dev))
            return r
        L.compute = compute
        return L

    def _temb_wiring(self, st, wkey, what):
        """The first convolution of a ResBlock (`<block>.in_layers.2`) adds the block's embedding projection: its columns of the
        batched LINEAR launch (the rows `<block>.embed_layers.1.weight` occupies in the concatenated weights), with that launch's
        row pitch.  No other launch adds one."""
        first = wkey.endswith(".in_layers.2.weight")
        if not first:
            if st.temb:
                raise LedgerError(f"{what}: {wkey} adds a timestep embedding")
            return
        if not st.temb:
            raise LedgerError(f"{what}: {wkey} is the first convolution of a ResBlock and adds no timestep embedding (temb missing)")
        ekey = wkey[:-len("in_layers.2.weight")] + "embed_layers.1.weight"
        for idx, lin, out, rows in self.linears:
            off = dict((k, o) for o, k in rows).get(ekey)
            if off is not None:
                if st.temb != lin.out + 4 * off or st.temb_ld != lin.N:
                    raise LedgerError(f"{what}: temb = out + {(st.temb - lin.out) // 4} with pitch {st.temb_ld}; {ekey} is at column {off} of "
                                      f"ops[{idx}], whose rows are {lin.N} floats apart")
                if off + st.N > lin.N or self.view.named[ekey].shape[0] != st.N:
                    raise LedgerError(f"{what}: {st.N} embedding columns at {off} of {lin.N}")
                return
        raise LedgerError(f"{what}: no earlier LINEAR launch projects {ekey}")

    def _head(self, i, st):
        what = f"ops[{i}] HEAD"
        B, H, W, C, Co = st.B, st.H, st.W, st.C, st.Cout
        L = Launch([i], f"head B={B} {H}x{W} C={C} Cout={Co}")
        x = self.reg(st.x, (B, H * W, C), (H * W * C, C, 1), what + ".x")
        w, pk, wkey = self.weight(st.w, PACK["small"], Co, C, 3, what)
        b = self.bias_of(st.bias, Co, wkey, what)
        sc, sh = self.affine_use(st.gn_scale, st.gn_shift, [x], C, i, what)
        out = self.reg(st.out, (B, Co, H * W), (Co * H * W, H * W, 1), what + ".out")
        L.inputs += [x, w, pk, sc, sh] + ([b] if b is not None else [])
        L.outs.append(Out("out", out, BAR_HEAD, "head"))
        self.routes.add("OP_HEAD")

        def compute(dev):
            ref = head(x.read(dev).reshape(B, H, W, C), sc.read(dev), sh.read(dev), w.read(dev), b.read(dev) if b is not None else None)
            return {"out": (out.read(dev).transpose(1, 2), ref.reshape(B, Co, H * W).transpose(1, 2), None)}
        L.compute = compute
        return L

    def _layout(self, i, st):
        what = f"ops[{i}] LAYOUT"
        B, P, C = st.B, st.P, st.C
        L = Launch([i], f"layout B={B} P={P} C={C}")
        inp = self.reg(st.inp, (B, P, C), (P * st.in_ld, st.in_ld, 1), what + ".in")
        out = self.reg(st.out, (B, C, P), (C * P, P, 1), what + ".out")
        L.inputs.append(inp)
        L.outs.append(Out("out", out, BAR_COPY, "layout"))
        self.routes.add("OP_LAYOUT")
        L.compute = lambda dev: {"out": (out.read(dev).transpose(1, 2), inp.read(dev), None)}
        return L

    # ------------------------------------------------------------------ static checks
    def static_failures(self):
        """Violations visible in the structs alone: what the descriptions raised (pointers, statistics producers, embedding columns,
        weights), then writer order and aliasing over all launches."""
        bad = list(self.static)
        written = []                                          # (region, launch) in list order

        ext = []                                              # adjacent packed copies (the concatenated embedding weights) merge
        for a, b in sorted(self.external):
            if ext and a <= ext[-1][1]:
                ext[-1][1] = max(ext[-1][1], b)
            else:
                ext.append([a, b])

        def is_external(r):
            lo, hi = r.span()
            return any(a <= lo and hi <= b for a, b in ext)
        for L in self.launches:
            for r in L.inputs:
                if is_external(r):
                    continue
                lo, hi = r.span()
                if not any(w.span()[0] <= lo and hi <= w.span()[1] for w, _ in written):
                    late = [M for M in self.launches if M.idx[0] > L.idx[0] and any(o.region.span()[0] <= lo and hi <= o.region.span()[1] for o in M.outs)]
                    bad.append(f"{L.what} (ops{L.idx}): reads {r}, which " +
                               (f"ops{late[0].idx} ({late[0].what}) writes LATER" if late else "no launch of the list writes"))
            for o in L.outs:
                for r in L.inputs:
                    if overlaps(o.region, r):
                        bad.append(f"{L.what} (ops{L.idx}): output {o.region} overlaps its input {r}")
                for r in L.scratch:
                    if any(overlaps(r, q) for q in L.inputs) or overlaps(r, o.region):
                        bad.append(f"{L.what} (ops{L.idx}): the split-K workspace {r} overlaps an operand of its own launch")
                if is_external(o.region):
                    bad.append(f"{L.what} (ops{L.idx}): writes {o.region}, a parameter / packed weight / caller's tensor")
                written.append((o.region, L))
        order = sorted(range(len(written)), key=lambda j: written[j][0].span())
        for a in range(len(order)):
            ra, La = written[order[a]]
            for b in range(a + 1, len(order)):
                rb, Lb = written[order[b]]
                if rb.span()[0] >= ra.span()[1]:
                    break
                if overlaps(ra, rb):
                    bad.append(f"{ra} (ops{La.idx}) and {rb} (ops{Lb.idx}): two launches write the same elements")
        for L in self.launches:                               # the shared workspace is scratch: nobody else's operand or output
            for r in L.scratch:
                lo, hi = r.span()
                for w, M in written:
                    if w.span()[0] < hi and lo < w.span()[1]:
                        bad.append(f"{L.what} (ops{L.idx}): the split-K workspace {r} overlaps {w}, written by ops{M.idx}")
        return bad

    # ------------------------------------------------------------------ arithmetic
    def audit(self, log=print):
        """Every output of every launch against its fp64 statement.  Returns (failures, figures): figures = [(launch, out name, class,
        figure, bar, ok)]."""
        bad, figs = [], []
        for r, jobs in self.copy_checks:
            flat = r.raw().reshape(-1)
            for off, key in jobs:
                p = self.view.named[key].detach().reshape(-1)
                if not torch.equal(flat[off:off + p.numel()].cpu(), p.cpu()):
                    bad.append((f"packed copy of {key} in {r}", None, "copy", float("nan"), 0.0, None))
        for L in self.launches:
            res = L.compute(self.dev)
            for o in L.outs:
                got, ref, den = res[o.name]
                got, ref = _z3(got), _z3(ref)
                if got.shape != ref.shape:
                    raise LedgerError(f"{L.what}: statement of {o.name} has shape {tuple(ref.shape)}, the region {tuple(got.shape)}")
                fig, where, bar, ok = block_figure(got, ref, den=den, bar=o.bar)
                log(f"  ops{L.idx} {L.what} [{L.cfg}] {o.name} {list(o.region.shape)}: worst (image, channel)={where} figure {fig:.3e} "
                    f"bar {o.bar:.3g}{'' if ok else '   <-- FAIL'}")
                figs.append((L, o.name, o.cls, fig, o.bar, ok))
                if not ok:
                    bad.append((L.what, L.idx, o.name, fig, o.bar, where))
            del res
        return bad, figs
