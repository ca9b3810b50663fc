"""Training-time execution of `UNetModel`: forward AND backward as two flat op lists over static NHWC buffers, run by
the native executor (`anoddpm_run_ops`) -- the reference's `loss.backward()` (diffusion_training.py:102) through
UNet.py:390-406 without a single ATen / MIOpen / rocBLAS compute kernel.

Design (MI355X-first, mirrors the inference plan of unet.py):
  * every activation of the forward keeps its buffer (the backward needs it anyway); every activation has a gradient
    buffer of the same shape; 288 GB of HBM makes recycling pointless and keeps all pointers static;
  * the forward op list starts with the device-side weight packing (3x3 direct / Winograd-domain, pointwise, small
    convs; forward and data-gradient layouts) of the CURRENT parameters, so an optimizer step needs no notification;
  * GroupNorm-apply + SiLU + resample + concat stay fused into the operand loads in both directions: forward convs,
    weight gradients (`anoddpm_conv3x3_wgrad`, `anoddpm_wgrad_pointwise`), and the GroupNorm backward
    (`anoddpm_gn_silu_backward`) read the raw block inputs; the data gradient of a conv is the forward kernel on the
    flipped / transposed weights;
  * QKVAttention backward = five MFMA GEMMs (anoddpm_igemm with activation B operands) around a softmax-backward and two
    square transposes;
  * gradient fan-in (skip connections, residuals, the shared time embedding) is resolved at BUILD time: the first writer
    of a gradient buffer overwrites, later writers accumulate -- no zero-fill and no add kernels;
  * parameter gradients are accumulated straight into `param.grad` storage (the flat gradient buffer of
    training.FlatBuffers when present), so neither autograd nor the optimizer copies them.

`UNetModel.forward` under autograd wraps the two lists in one autograd Function (`TrainPlanFunction`); everything else
of the reference loop body (p_loss, the loss expression) stays the reference's torch code on [B,1,S,S] tensors.
"""
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import (ColsumFoldArgs, DropoutArgs, GnBwdArgs, HeadBwdArgs, LinearBwdArgs, LinearBwdBatchArgs, Op, PackArgs, SoftmaxBwdArgs,
                   StemBwdArgs, TransposeArgs, Wgrad1Args, WgradArgs, check, lib)
from .unet import _Plan, _Srcs, _op_array, _pack_table, pack_floats, pack_kind

__all__ = ["TrainPlan", "TrainPlanFunction", "eligible"]


def eligible(model, B, S):
    """Shapes the native training plan covers: everything the reference's args files use and every constructor option
    (dropout, the Downsample / Upsample topology); what is left out are extreme sizes (batch > 16 per GPU, base_channels > 256,
    more than four image channels), which raise."""
    cfin, nout = model._final_cin, model.in_channels
    head_ok = nout <= 4 and S % 8 == 0 and (100 * (cfin + 16) + 9 * cfin * nout) * 4 <= 64 * 1024 and cfin <= 256
    return head_ok and 1 <= B <= 16 and model.model_channels % 4 == 0 and model.model_channels <= 256


class TrainPlan(_Plan):
    honours_arith = False        # fp32 only: the split-bf16 side configuration has no backward
    honours_csum = False         # statistics rows + finalize launches everywhere: the backward needs mean / rstd as tensors

    def __init__(self, model, B, S, device, want_dx=False, p_drop=0.0):
        self.want_dx = want_dx
        self.p_drop = float(p_drop)  # nn.Dropout of ResBlock.out_layers (UNet.py:192), training mode only
        self._drop_ops = []          # (forward struct, backward struct, layer index): the seeds are patched per forward
        self.bops = []               # backward op list
        self.pack_ops = []           # weight packing, runs ahead of the forward
        self._packs = {}
        self._bw = []                # closures emitting the backward of each forward stage (run in reverse)
        self._grads = {}             # data_ptr of an activation -> its gradient buffer
        self.gwritten = set()
        self._touched = set()
        self.bwd_marks = []          # (backward op count after a stage, parameter names whose gradient that stage wrote)
        self._ws_patch = []          # (struct, field, floats) sharing one training workspace
        self._tws_need = 0
        super().__init__(model, B, S, device)
        self.fwd_list = self._batched_packs() + self.ops
        self.fwd_array = _op_array(self.fwd_list)
        self.bwd_array = _op_array(self.bops)

    def _batched_packs(self):
        """The ~270 per-weight pack launches of a forward as ONE launch (anoddpm_pack_batch: device-resident job table, a block finds
        its job by bisection); ANODDPM_PACK_BATCH=0 keeps one launch per weight."""
        if os.environ.get("ANODDPM_PACK_BATCH", "1") == "0" or not self.pack_ops:
            return list(self.pack_ops)
        pb, raw, b0 = _pack_table([st for _, st in self.pack_ops], self.device)
        self.keep += [raw, b0, pb]
        return [(_lib.OP_PACK_BATCH, pb)]

    # ------------------------------------------------------------------ parameters
    def _bind_params(self):
        """Destinations of the parameter gradients: the parameter's existing `.grad` storage (e.g. the views of
        training.FlatBuffers) or a slice of a plan-owned arena."""
        self.named = dict(self.model.named_parameters())
        need = sum((p.numel() + 3) // 4 * 4 for p in self.named.values() if p.grad is None)
        self.arena = torch.zeros(max(need, 4), device=self.device)
        self.pptr, self.gptr, self.gview = {}, {}, {}
        off = 0
        for k, p in self.named.items():
            if p.device != self.device or p.dtype != torch.float32 or not p.is_contiguous():
                raise _lib.AnoddpmError(f"parameter {k}: the training plan needs contiguous fp32 parameters on {self.device}")
            self.pptr[k] = p.data_ptr()
            if p.grad is not None:
                if p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    raise _lib.AnoddpmError(f"parameter {k}: .grad must be contiguous fp32")
                self.gptr[k] = p.grad.data_ptr()
                self.gview[k] = None
            else:
                v = self.arena[off:off + p.numel()].view(p.shape)
                off += (p.numel() + 3) // 4 * 4
                self.gptr[k] = v.data_ptr()
                self.gview[k] = v

    def params_match(self):
        """True while every parameter (and its gradient destination, if it has one) still lives where the op lists point."""
        for k, p in self.named.items():
            if p.data_ptr() != self.pptr[k]:
                return False
            if p.grad is not None and p.grad.data_ptr() != self.gptr[k]:
                return False
            if p.grad is None and self.gview[k] is None:
                return False
        return True

    def W(self, key):
        return self.pptr[key]

    def dW(self, key):
        self._touched.add(key)                # backward stage that (last) writes this parameter's gradient: see bwd_marks
        return self.gptr[key]

    def pack(self, key, kind, bwd=0, k0=0, kc=0):
        """Packed copy of a weight in the layout `kind` names (unet.PACK_KINDS, or "conv"), refreshed by an OP_PACK at the head of
        every forward; bwd=1: the data-gradient twin (flipped / transposed; pointwise: input channels k0 .. k0 + kc)."""
        w = self.named[key]
        kind = pack_kind(kind, w.shape)
        ck = (key, kind, bwd, k0, kc)
        hit = self._packs.get(ck)
        if hit is not None:
            return hit
        N, K = w.shape[0], w.shape[1]
        out = self.buf(pack_floats(kind, N, K, bwd, kc))
        st = PackArgs()
        st.w, st.out, st.N, st.K, st.kind, st.bwd, st.k0, st.kc = self.W(key), out.data_ptr(), N, K, kind, bwd, k0, kc
        self.keep.append(st)
        self.pack_ops.append((_lib.OP_PACK, st))
        self._packs[ck] = out
        return out

    weight = pack                # unet._Plan.weight: the layouts the forward asks for are packed copies refreshed every forward
    param = W                    # unet._Plan.param: biases and affine parameters are read in place

    # ------------------------------------------------------------------ gradient buffers
    def G(self, t):
        g = self._grads.get(t.data_ptr())
        if g is None:
            g = self._grads[t.data_ptr()] = self.buf(*t.shape)
        return g

    def gacc(self, t):
        """0 for the first writer of t's gradient in backward order (overwrite), 1 afterwards (accumulate)."""
        k = t.data_ptr()
        if k in self.gwritten:
            return 1
        self.gwritten.add(k)
        return 0

    def badd(self, code, st):
        self.keep.append(st)
        self.bops.append((code, st))
        return st

    def tws(self, st, field, floats):
        """The op's workspace is a slice of one shared training workspace (ops run in stream order)."""
        self._tws_need = max(self._tws_need, int(floats))
        self._ws_patch.append((st, field))

    # ------------------------------------------------------------------ emitters
    def linear_bwd(self, x, wkey, bkey, dy, K, N, act_in, dx):
        st = LinearBwdArgs()
        st.x, st.w, st.dy = x.data_ptr(), self.W(wkey), dy.data_ptr()
        st.dw, st.db = self.dW(wkey), self.dW(bkey)
        st.dx = dx.data_ptr() if dx is not None else None
        st.B, st.K, st.N, st.act_in, st.acc_w = self.B, K, N, act_in, 1
        st.acc_x = self.gacc(dx) if dx is not None else 0
        self.badd(_lib.OP_LINEAR_BWD, st)

    def linear_bwd_batch(self, x, jobs, K, dx):
        """Backward of several linear layers that share the input x (anoddpm_linear_small_backward_batch)."""
        if not jobs:
            return
        arr = (LinearBwdArgs * len(jobs))()
        for i, (wkey, bkey, dy, N) in enumerate(jobs):
            arr[i].w, arr[i].dy, arr[i].dw, arr[i].db, arr[i].N = self.W(wkey), dy.data_ptr(), self.dW(wkey), self.dW(bkey), N
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        ws = self.buf(len(jobs) * self.B * K)
        st = LinearBwdBatchArgs()
        st.jobs, st.x, st.dx, st.ws = raw.data_ptr(), x.data_ptr(), dx.data_ptr(), ws.data_ptr()
        st.njobs, st.max_n = len(jobs), max(j[3] for j in jobs)
        st.B, st.K, st.act_in, st.acc_w, st.acc_x = self.B, K, 1, 1, self.gacc(dx)
        self.keep.append(raw)
        self.badd(_lib.OP_LINEAR_BWD_BATCH, st)

    def in_backward(self):
        """Context: igemm / resample ops emitted inside go to the backward list."""
        plan = self

        class _Ctx:
            def __enter__(self):
                self.saved = plan.ops
                plan.ops = plan.bops

            def __exit__(self, *a):
                plan.ops = self.saved
        return _Ctx()

    def wgrad3(self, srcs, Hs, H, gn, a_mode, dy, N, wkey, bkey, d_emb=None):
        """3x3 weight gradient (+ the column sums of dy: bias gradient and, optionally, the per-image embedding gradient)."""
        B = self.B
        a = _Srcs(srcs)
        K, c0, c1 = a.K, a.c0, a.c1
        W = H
        tiles = -(-K // 64) * -(-N // 64)
        TW = next(t for t in (32, 16, 8, 4, 2) if W % t == 0)
        per_band = tiles * B * (W // TW)
        nband = max(1, min(H, round(512 / per_band)))
        band = -(-H // nband)
        nband = -(-H // band)
        ipb = (W // TW) * nband
        nitems = B * ipb
        # Winograd-domain weight gradient (csrc/wgrad43.hip: the adjoint of the F(4x4,3x3) forward kernel, 4x fewer MFMAs) on the
        # maps where the forward uses that kernel; ANODDPM_NO_WGRAD43=1 keeps the direct nine-tap kernel everywhere
        # (a plain operand -- dropout output, Downsample / Upsample inputs -- takes the direct kernel: gn is None)
        algo = int(gn is not None and a_mode in (0, 1) and H % 8 == 0 and W % 16 == 0 and K % 32 == 0 and N % 64 == 0 and (c1 == 0 or c0 % 16 == 0)
                   and B <= 15 and H * W >= int(os.environ.get("ANODDPM_WGRAD43_MIN_PIXELS", 16 * 16))   # round 6: the 16x16 maps too (40.55 -> 40.32 ms per config-3 step, profiles/r6_knob_sweep_c3.txt; 32x32 was the limit before)
                   and os.environ.get("ANODDPM_NO_WGRAD43", "0") != "1")
        wa = WgradArgs()
        wa.a0, wa.a1, wa.c0, wa.c1, wa.a0_ld, wa.a1_ld = a.p0, a.p1, c0, c1, a.ld0, a.ld1
        wa.gn_scale, wa.gn_shift = (gn[0].data_ptr(), gn[1].data_ptr()) if gn is not None else (None, None)
        wa.dy, wa.dw = dy.data_ptr(), self.dW(wkey)
        wa.algo = algo
        if algo:
            wa.ws_floats = lib().anoddpm_wgrad43_groups(K, N, B, H, W) * 9 * K * N
            ipb = lib().anoddpm_wgrad43_colsum_items(K, N, B, H, W)   # column-sum rows per image: one per workgroup set and tile row
        else:
            wa.ws_floats = nitems * 9 * K * N
        self.tws(wa, "ws", wa.ws_floats)
        (wa.a0_bs, wa.a1_bs), wa.dy_bs, wa.dy_ld = a.strides(Hs * Hs), H * W * N, N
        wa.H, wa.W, wa.N, wa.B = H, W, N, B
        wa.a_mode, wa.act, wa.gn_ld, wa.band, wa.accumulate = a_mode, (1 if gn is not None else 0), K, band, 1
        colsum = self.buf(B, ipb, N)
        wa.colsum = colsum.data_ptr()
        if d_emb is None:
            d_emb = self.buf(B, N)                               # per-image sums: scratch when only the bias gradient is wanted
        wa.dimg = wa.dbias = None
        if algo:
            # the fold launch of the Winograd-domain kernel also folds the column sums (round 6: 64 colsum_fold launches less per step)
            wa.dimg, wa.dbias = d_emb.data_ptr(), self.dW(bkey)
            self.badd(_lib.OP_WGRAD3, wa)
            return
        self.badd(_lib.OP_WGRAD3, wa)
        cf = ColsumFoldArgs()
        cf.colsum, cf.dimg, cf.dbias = colsum.data_ptr(), d_emb.data_ptr(), self.dW(bkey)
        cf.B, cf.ipb, cf.N = B, ipb, N
        self.badd(_lib.OP_COLSUM_FOLD, cf)

    def wgrad1(self, srcs, P, gn, act, dy, dy_ld, N, wkey, bkey):
        B = self.B
        a = _Srcs(srcs)
        K = a.K
        tiles = -(-K // 128) * -(-N // 128)
        want_items = max(1, 512 // tiles)
        span = max(32, (B * P // want_items + 31) // 32 * 32)
        span = min(span, (P + 31) // 32 * 32)
        nitems = B * -(-P // span)
        st = Wgrad1Args()
        st.a0, st.a1, st.c0, st.c1, st.a0_ld, st.a1_ld = a.p0, a.p1, a.c0, a.c1, a.ld0, a.ld1
        st.gn_scale = gn[0].data_ptr() if gn else None
        st.gn_shift = gn[1].data_ptr() if gn else None
        st.dy, st.dw, st.dbias = dy if isinstance(dy, int) else dy.data_ptr(), self.dW(wkey), self.dW(bkey)
        st.ws_floats = nitems * (K * N + N)
        self.tws(st, "ws", st.ws_floats)
        (st.a0_bs, st.a1_bs), st.dy_bs, st.dy_ld = a.strides(P), P * dy_ld, dy_ld
        st.P, st.N, st.B, st.act, st.gn_ld, st.span, st.accumulate = P, N, B, act, K, span, 1
        self.badd(_lib.OP_WGRAD1, st)

    def gn_bwd(self, srcs, Hs, da, da_P, gnp, prefix, act, a_mode, dres=None, fused=None):
        """Backward of the fused GroupNorm(+SiLU)(+resample) operand load into the gradients of its sources.
        fused = (partial buffer, rows per image) when the data-gradient launch that produced `da` already wrote the
        reduction pass's partial sums (dgrad3(..., gnb=...)): fold + elementwise launches only."""
        B = self.B
        x = _Srcs(srcs)
        C, c0, c1 = x.K, x.c0, x.c1
        P = Hs * Hs
        nslab = max(1, min(int(os.environ.get("ANODDPM_GNBWD_SLABS", 256)), P // 16))     # >= 4 workgroups per CU on the large maps
        if fused is not None:
            assert a_mode == 0 and act == 1
            nslab = fused[1]
        ga = GnBwdArgs()
        ga.x0, ga.x1, ga.c0, ga.c1, ga.x0_ld, ga.x1_ld = x.p0, x.p1, c0, c1, x.ld0, x.ld1
        ga.da = da.data_ptr()
        ga.gamma, ga.beta = self.W(prefix + ".weight"), self.W(prefix + ".bias")
        ga.mean, ga.rstd = gnp[2].data_ptr(), gnp[3].data_ptr()
        g0 = self.G(srcs[0][0])
        ga.dx0 = g0.data_ptr()
        acc = self.gacc(srcs[0][0])
        if c1:
            g1 = self.G(srcs[1][0])
            ga.dx1 = g1.data_ptr()
            acc |= self.gacc(srcs[1][0]) << 1
        ga.dgamma, ga.dbeta = self.dW(prefix + ".weight"), self.dW(prefix + ".bias")
        part = fused[0] if fused is not None else self.buf(B * nslab * C * 2, dtype=torch.float64)
        coef = self.buf(B * C * 4)
        ga.partial, ga.coef = part.data_ptr(), coef.data_ptr()
        ga.partial_ready = 1 if fused is not None else 0
        (ga.x0_bs, ga.x1_bs), (ga.dx0_bs, ga.dx1_bs), ga.da_bs = x.strides(P), x.strides(P), da_P * C
        ga.da_ld, ga.dx0_ld, ga.dx1_ld = C, x.ld0, x.ld1           # (the gradients have their sources' layout)
        ga.Hs, ga.Ws, ga.B, ga.groups, ga.nslab = Hs, Hs, B, 32, nslab
        ga.act, ga.a_mode, ga.acc_dx = act, a_mode, acc
        if dres is not None:
            ga.dres, ga.dres_bs, ga.dres_ld = dres.data_ptr(), P * C, C
        else:
            ga.dres, ga.dres_bs, ga.dres_ld = None, 0, 0
        self.badd(_lib.OP_GN_BWD, ga)

    # ------------------------------------------------------------------ network
    # The forward is unet._Plan's, inherited.  What differs enters through the overrides below (`weight` / `param` above, `gn`,
    # `time_path` / `emb_of`, `pool_act`, `dropout`, `keep_probs`); every block method calls the inherited forward and registers
    # the backward of that block from the record it returns.
    keep_probs = True            # the softmax output of every attention block is kept for the backward

    def _build(self):
        self._bind_params()
        self.walk()
        # --- backward list: the stages in reverse
        for fn in reversed(self._bw):
            self._touched = set()
            fn()
            self.bwd_marks.append((len(self.bops), sorted(self._touched)))
        # split-K workspace of the shared igemm emitter (forward and backward launches) + the training workspace
        self.share_workspace(self.ops + self.bops)
        if self._tws_need:
            tws = self.buf(self._tws_need)
            for st, field in self._ws_patch:
                setattr(st, field, tws.data_ptr())

    def gn(self, srcs, P, prefix, consumer=None):
        """GroupNorm statistics -> (scale, shift, mean, rstd), always as tensors (the backward reads mean / rstd) and never folded
        into the `consumer`; parameters are read in place."""
        self.gn_sums(srcs, P)
        gamma, beta = self.W(prefix + ".weight"), self.W(prefix + ".bias")
        return self.gn_tail_job(srcs, gamma, beta, want_mean=True) or self.gn_finalize(srcs, P, gamma, beta, want_mean=True)

    def pool_act(self):
        # ANODDPM_NO_POOL_ACT is an A/B switch of the inference plan only: honouring it here would move the first convolution of every
        # down block from the Winograd kernels to the pool-fused direct one (the backward re-applies the pooling on the raw input either way)
        return True

    def time_path(self):
        """Timestep path (UNet.py:271-276): pre-activations are kept, SiLU rides on the next layer's input (the backward needs z1)."""
        m = self.model
        base, ted = m.model_channels, m._ted
        pe = self.posemb_features()
        z1 = self.linear(pe, self.W("time_embedding.1.weight"), self.W("time_embedding.1.bias"), base, ted, 0)
        temb = self.temb = self.linear(z1, self.W("time_embedding.3.weight"), self.W("time_embedding.3.bias"), ted, ted, 1)
        g_temb, g_z1 = self.G(temb), self.G(z1)

        # Forward: every ResBlock's embedding projection in ONE launch (round 6: 22 launches of ~8 us at config 3) when the projections'
        # weights and biases are consecutive in memory in one order -- training.FlatBuffers stores them that way; a model with
        # separately allocated parameters keeps one launch per block.  linear_small computes one output feature per wave, so the
        # values are the per-block launches' bit for bit.
        self._emb_all, self._emb_off, self._emb_tot = None, {}, 0
        ekeys = [k[:-len(".weight")] for k in self.named if k.endswith(".embed_layers.1.weight")]
        if len(ekeys) > 1 and os.environ.get("ANODDPM_BATCH_EMB_FWD", "1") != "0":
            wp, bp, ok = self.W(ekeys[0] + ".weight"), self.W(ekeys[0] + ".bias"), True
            for k in ekeys:
                w = self.named[k + ".weight"]
                ok = ok and self.W(k + ".weight") == wp and self.W(k + ".bias") == bp and w.shape[1] == ted
                self._emb_off[k[:-len(".embed_layers.1")]] = self._emb_tot
                wp += 4 * w.numel()
                bp += 4 * w.shape[0]
                self._emb_tot += w.shape[0]
            if ok:
                self._emb_all = self.linear(temb, self.W(ekeys[0] + ".weight"), self.W(ekeys[0] + ".bias"), ted, self._emb_tot, 1)

        self._emb_jobs = []          # (weight key, bias key, d_emb buffer, cout) of every ResBlock's embedding projection
        # One batched launch for all of them at the END of the backward.  With a data-parallel reducer attached that is still
        # right: training.FlatBuffers stores the embedding projections (and the timestep MLP) at the bottom of the flat buffer,
        # so they share the last gradient bucket(s) and no other bucket's all-reduce waits for them.
        self._batch_emb = os.environ.get("ANODDPM_BATCH_EMB_BWD", "1") != "0"

        def time_bwd():
            self.linear_bwd_batch(temb, self._emb_jobs, ted, g_temb)        # all embedding projections at once
            self.linear_bwd(z1, "time_embedding.3.weight", "time_embedding.3.bias", g_temb, ted, ted, 1, g_z1)
            self.linear_bwd(pe, "time_embedding.1.weight", "time_embedding.1.bias", g_z1, base, ted, 0, None)
        self._bw.append(time_bwd)

    def emb_of(self, prefix, cout):
        """(pointer, row pitch) of a block's embedding projection: a column range of the batched launch, or its own launch."""
        if self._emb_all is not None:
            return super().emb_of(prefix, cout)
        ted = self.model._ted
        return self.linear(self.temb, self.W(prefix + ".embed_layers.1.weight"), self.W(prefix + ".embed_layers.1.bias"), ted, cout, 1).data_ptr(), cout

    def dropout(self, h1, g2, P, C):
        """Dropout between the activation and the second convolution of a ResBlock: the dropped activation is materialised once
        (one elementwise launch) and the convolution, its weight gradient and its data gradient see a plain operand."""
        a2 = self.buf(self.B, P, C)
        dr = DropoutArgs()
        dr.x, dr.out, dr.gn_scale, dr.gn_shift = h1.data_ptr(), a2.data_ptr(), g2[0].data_ptr(), g2[1].data_ptr()
        dr.n, dr.B, dr.C, dr.mode, dr.p, dr.seed = P * C, self.B, C, 0, self.p_drop, 0
        self.add(_lib.OP_DROPOUT, dr)
        self._drop_ops.append([dr, None, len(self._drop_ops)])       # forward order; the block's backward fills in the backward twin
        return a2

    def dgrad3(self, dy, Hout, Kc, N, wkey, gnb=None):
        """da [B][Hout^2][Kc] = conv3x3(dy, flipped / transposed weights): the forward kernels on the packed twin.
        gnb = (sources, gn tuple, GroupNorm prefix) of the operand a = SiLU(GroupNorm(x)) this gradient belongs to: where the
        launch runs on the channel-sliced F(4x4,3x3) kernel its epilogue also writes the partial sums of the GroupNorm
        backward's reduction pass (round 6: one pass over x and da less per layer); returns (da, fused) for gn_bwd."""
        B = self.B
        da = self.buf(B, Hout * Hout, Kc)
        st = self.igemm(srcs=[(dy, N)], H=Hout, W=Hout, ks=3, N=Kc, **self.conv_weights(wkey, bwd=1), out=da)
        st.gnb_partial = None
        if gnb is None:
            return da
        fused = None
        xs, gnp, gprefix = gnb
        x = _Srcs(xs)
        xc0 = x.c0
        if (os.environ.get("ANODDPM_NO_GNB_FUSE", "0") != "1" and st.cfg == 3 and st.ksplit == 1 and xc0 % 16 == 0
                and x.K == Kc and lib().anoddpm_f43_channel_sliced(Hout, Hout, Kc, B) == 1):
            rows = (Hout // 16) * (Hout // 16)
            part = self.buf(B * rows * Kc * 2, dtype=torch.float64)
            st.gnb_partial = part.data_ptr()
            st.gnb_x0, st.gnb_x1, st.gnb_c0, st.gnb_x0_ld, st.gnb_x1_ld, st.gnb_groups = x.p0, x.p1, xc0, x.ld0, x.ld1, 32
            st.gnb_gamma, st.gnb_beta = self.W(gprefix + ".weight"), self.W(gprefix + ".bias")
            st.gnb_mean, st.gnb_rstd = gnp[2].data_ptr(), gnp[3].data_ptr()
            st.gnb_x0_bs, st.gnb_x1_bs = x.strides(Hout * Hout)
            fused = (part, rows)
        return da, fused

    def stem_block(self, prefix, cin, cout):
        r = super().stem_block(prefix, cin, cout)
        B, S = self.B, self.S

        def stem_bwd():
            sb = StemBwdArgs()
            self.stem_bwd_args = sb
            sb.x, sb.w, sb.dy = None, self.W(prefix + ".weight"), self.G(r.out).data_ptr()
            sb.dw, sb.db = self.dW(prefix + ".weight"), self.dW(prefix + ".bias")
            self.dx = self.buf(B, cin, S, S) if self.want_dx else None
            sb.dx = self.dx.data_ptr() if self.want_dx else None
            nblk = B * -(-(S * S) // 1024)
            sb.ws_floats = nblk * (cin * 9 + 1) * cout
            self.tws(sb, "ws", sb.ws_floats)
            sb.B, sb.H, sb.W, sb.Cin, sb.Cout = B, S, S, cin, cout
            self.badd(_lib.OP_STEM_BWD, sb)
        self._bw.append(stem_bwd)
        return r

    def res_block(self, prefix, srcs, Hin, cout, resample):
        r = super().res_block(prefix, srcs, Hin, cout, resample)
        B, ted, temb = self.B, self.model._ted, self.temb
        cin, Hout, am, g1, g2, h1, h2, a2 = r.cin, r.H, r.a_mode, r.g1, r.g2, r.h1, r.out, r.a2
        Pin, Pout = Hin * Hin, Hout * Hout
        drop_entry = self._drop_ops[-1] if a2 is not None else None

        def bwd():
            gh2 = self.G(h2)
            with self.in_backward():
                # 1. skip path
                if r.skip == "conv":
                    self.wgrad1(srcs, Pin, None, 0, gh2, cout, cout, prefix + ".skip_connection.weight",
                                prefix + ".skip_connection.bias")
                    k0 = 0
                    for (src, c) in [(s[0], s[1]) for s in srcs]:
                        gs = self.G(src)
                        acc = self.gacc(src)
                        self.igemm(srcs=[(gh2, cout)], H=Hout, W=Hout, ks=1, N=c, kind="conv1",
                                   bmat=self.pack(prefix + ".skip_connection.weight", "conv", bwd=1, k0=k0, kc=c),
                                   res=(gs if acc else None), out=gs)
                        k0 += c
                elif r.skip == "resample":
                    src = srcs[0][0]
                    # forward nearest-up -> backward sums the four children (avg pool * 4); forward avg pool -> nearest-up / 4
                    mode, scale = (2, 4.0) if resample == "up" else (1, 0.25)
                    self.resample(gh2, Hout, cout, mode, self.G(src), scale, self.gacc(src))
                # 2-4. out_layers: weight gradient, data gradient, GroupNorm + SiLU backward into g(h1)
                if a2 is not None:
                    self.wgrad3([(a2, cout)], Hout, Hout, None, 0, gh2, cout, prefix + ".out_layers.3.weight", prefix + ".out_layers.3.bias")
                    da2, fused2 = self.dgrad3(gh2, Hout, cout, cout, prefix + ".out_layers.3.weight"), None
                    db = DropoutArgs()                           # d(activation) = mask / (1 - p) * d(dropped), in place
                    db.x, db.out, db.n, db.B, db.C, db.mode, db.p, db.seed = da2.data_ptr(), da2.data_ptr(), Pout * cout, B, cout, 1, self.p_drop, 0
                    self.add(_lib.OP_DROPOUT, db)
                    drop_entry[1] = db
                else:
                    self.wgrad3([(h1, cout)], Hout, Hout, g2, 0, gh2, cout, prefix + ".out_layers.3.weight", prefix + ".out_layers.3.bias")
                    da2, fused2 = self.dgrad3(gh2, Hout, cout, cout, prefix + ".out_layers.3.weight",
                                              gnb=([(h1, cout)], g2, prefix + ".out_layers.0"))
                self.gn_bwd([(h1, cout)], Hout, da2, Pout, g2, prefix + ".out_layers.0", 1, 0, fused=fused2)
                gh1 = self.G(h1)
                # 5. in_layers weight gradient; its dy column sums are the conv bias and the embedding gradients
                d_emb = self.buf(B, cout)
                self.wgrad3(srcs, Hin, Hout, g1, am, gh1, cout, prefix + ".in_layers.2.weight", prefix + ".in_layers.2.bias", d_emb=d_emb)
                if self._batch_emb:
                    self._emb_jobs.append((prefix + ".embed_layers.1.weight", prefix + ".embed_layers.1.bias", d_emb, cout))
                else:
                    self.linear_bwd(temb, prefix + ".embed_layers.1.weight", prefix + ".embed_layers.1.bias", d_emb, ted, cout, 1, self.G(temb))
                # 6-7. data gradient and the fused operand load's backward into the block inputs
                if am == 0:
                    da1, fused1 = self.dgrad3(gh1, Hout, cin, cout, prefix + ".in_layers.2.weight", gnb=(srcs, g1, prefix + ".in_layers.0"))
                else:                                            # a resampling sits between the activation and the convolution
                    da1, fused1 = self.dgrad3(gh1, Hout, cin, cout, prefix + ".in_layers.2.weight"), None
                self.gn_bwd(srcs, Hin, da1, Pout, g1, prefix + ".in_layers.0", 1, am,
                            dres=(gh2 if r.skip == "identity" else None), fused=fused1)
        self._bw.append(bwd)
        return r

    def attn_block(self, prefix, x, Hc, C):
        r = super().attn_block(prefix, x, Hc, C)
        B, L, heads, ch, g, att, Pm, y = self.B, r.L, r.heads, r.ch, r.g, r.att, r.probs, r.out
        Z = B * heads
        alpha = 1.0 / math.sqrt(ch)
        qp = r.qkv.data_ptr()

        def bwd():
            gy = self.G(y)
            with self.in_backward():
                # proj_out: dW, d(att)
                self.wgrad1([(att, C)], L, None, 0, gy, C, C, prefix + ".proj_out.weight", prefix + ".proj_out.bias")
                datt = self.buf(B, L, C)
                self.igemm(srcs=[(gy, C)], H=Hc, W=Hc, ks=1, N=C, kind="qkvproj",
                           bmat=self.pack(prefix + ".proj_out.weight", "conv", bwd=1, k0=0, kc=C), out=datt)
                dqkv = self.buf(B, L, 3 * C)
                dq = dqkv.data_ptr()
                dP = self.buf(Z, L, L)
                T1 = self.buf(Z, L, L)
                # dP = d(att)_h v_h^T
                self.igemm(srcs=[(datt.data_ptr(), ch, C)], H=1, W=L, ks=1, N=L, b_mode=1, ldb=3 * C, heads=heads,
                           bmat=qp + 4 * 2 * ch, kind="attn", a_strides=(L * C, ch), b_strides=(L * 3 * C, 3 * ch),
                           out=dP, out_ld=L, o_strides=(heads * L * L, L * L))
                # dV_h = P^T d(att)_h
                tr = TransposeArgs()
                tr.inp, tr.out, tr.Z, tr.L = Pm.data_ptr(), T1.data_ptr(), Z, L
                self.add(_lib.OP_TRANSPOSE, tr)
                self.igemm(srcs=[(T1.data_ptr(), L, L)], H=1, W=L, ks=1, N=ch, b_mode=2, ldb=C, heads=heads,
                           bmat=datt.data_ptr(), kind="attn", a_strides=(heads * L * L, L * L), b_strides=(L * C, ch),
                           out=dq + 4 * 2 * ch, out_ld=3 * C, o_strides=(L * 3 * C, 3 * ch))
                # dS = P o (dP - rowsum(dP o P)), in place
                sb = SoftmaxBwdArgs()
                sb.p, sb.dp, sb.rows, sb.L = Pm.data_ptr(), dP.data_ptr(), Z * L, L
                self.add(_lib.OP_SOFTMAX_BWD, sb)
                # dQ_h = alpha dS k_h ; dK_h = alpha dS^T q_h
                self.igemm(srcs=[(dP.data_ptr(), L, L)], H=1, W=L, ks=1, N=ch, b_mode=2, ldb=3 * C, heads=heads,
                           bmat=qp + 4 * ch, alpha=alpha, kind="attn", a_strides=(heads * L * L, L * L),
                           b_strides=(L * 3 * C, 3 * ch), out=dq, out_ld=3 * C, o_strides=(L * 3 * C, 3 * ch))
                tr2 = TransposeArgs()
                tr2.inp, tr2.out, tr2.Z, tr2.L = dP.data_ptr(), T1.data_ptr(), Z, L
                self.add(_lib.OP_TRANSPOSE, tr2)
                self.igemm(srcs=[(T1.data_ptr(), L, L)], H=1, W=L, ks=1, N=ch, b_mode=2, ldb=3 * C, heads=heads,
                           bmat=qp, alpha=alpha, kind="attn", a_strides=(heads * L * L, L * L),
                           b_strides=(L * 3 * C, 3 * ch), out=dq + 4 * ch, out_ld=3 * C, o_strides=(L * 3 * C, 3 * ch))
                # to_qkv: dW (input = GroupNorm(x), no SiLU), d(normed x), GroupNorm backward + the residual
                self.wgrad1([(x, C)], L, g, 0, dqkv, 3 * C, 3 * C, prefix + ".to_qkv.weight", prefix + ".to_qkv.bias")
                da = self.buf(B, L, C)
                self.igemm(srcs=[(dqkv, 3 * C)], H=Hc, W=Hc, ks=1, N=C, kind="qkvproj",
                           bmat=self.pack(prefix + ".to_qkv.weight", "conv", bwd=1, k0=0, kc=C), out=da)
                self.gn_bwd([(x, C)], Hc, da, L, g, prefix + ".norm", 0, 0, dres=gy)
        self._bw.append(bwd)
        return r

    def resample_layer(self, prefix, kind, x, Hc, C, conv):
        """Downsample / Upsample of the biggan_updown=False topology (UNet.py:60-92).  Backward: the weight gradient on the plain
        operand, the data gradient as the forward kernel on the flipped weights, and the adjoint of the resampling around it."""
        r = super().resample_layer(prefix, kind, x, Hc, C, conv)
        B, out, Ho, wk = self.B, r.out, r.H, r.wkey
        bk = wk[:-len("weight")] + "bias" if conv else None

        def bwd():
            with self.in_backward():
                if not conv:
                    # avg pool -> nearest-up / 4; nearest x2 -> the sum of the four children
                    mode, scale = (1, 0.25) if kind == "downsample" else (2, 4.0)
                    self.resample(self.G(out), Ho, C, mode, self.G(x), scale, self.gacc(x))
                elif kind == "downsample":
                    gfull = self.buf(B, Hc * Hc, C)
                    self.resample(self.G(out), Ho, C, 4, gfull)     # gradient on the stride-1 grid: zeros off the even pixels
                    self.wgrad3([(x, C)], Hc, Hc, None, 0, gfull, C, wk, bk)
                    # dx (+)= conv3x3(dy, flipped weights), straight into the gradient buffer of x
                    gx = self.G(x)
                    acc = self.gacc(x)
                    self.igemm(srcs=[(gfull, C)], H=Hc, W=Hc, ks=3, N=C, **self.conv_weights(wk, bwd=1),
                               res=(gx if acc else None), out=gx)
                else:
                    self.wgrad3([(x, C)], Hc, Ho, None, 1, self.G(out), C, wk, bk)
                    dup = self.dgrad3(self.G(out), Ho, C, C, wk)    # gradient of the upsampled operand, at the output resolution
                    self.resample(dup, Ho, C, 2, self.G(x), 4.0, self.gacc(x))   # nearest x2 -> the sum of the four children
        self._bw.append(bwd)
        return r

    def head_block(self, hfin, cfin):
        r = super().head_block(hfin, cfin)
        B, S, gh, nout = self.B, self.S, r.g, r.nout
        self.dy = self.buf(B, nout, S, S)

        def head_bwd():
            hb = HeadBwdArgs()
            da = self.buf(B, S * S, cfin)
            hb.x, hb.gn_scale, hb.gn_shift = hfin.data_ptr(), gh[0].data_ptr(), gh[1].data_ptr()
            hb.w, hb.dy, hb.da = self.W("out.2.weight"), self.dy.data_ptr(), da.data_ptr()
            hb.dw, hb.db = self.dW("out.2.weight"), self.dW("out.2.bias")
            nblk = B * -(-(S * S) // 512)
            hb.ws_floats = nblk * 10 * nout * cfin
            self.tws(hb, "ws", hb.ws_floats)
            hb.B, hb.H, hb.W, hb.C, hb.Cout = B, S, S, cfin, nout
            self.badd(_lib.OP_HEAD_BWD, hb)
            self.gn_bwd([(hfin, cfin)], S, da, S * S, gh, "out.0", 1, 0)
        self._bw.append(head_bwd)
        return r

    # ------------------------------------------------------------------ execution
    def run_forward(self, x, t):
        """x: contiguous fp32 [B,C,S,S] on self.device (kept alive by the caller until the backward); t: int64 [B]."""
        self.stem.x = x.data_ptr()
        self.posemb.t = t.data_ptr()
        if self._drop_ops:
            # a fresh mask per forward and per layer: the seed is one draw from torch's CPU generator (so torch.manual_seed
            # between steps matters, as it does for nn.Dropout, and the stream advances per forward) mixed with the
            # data-parallel rank (replicas seeded alike must not drop the same units) and the layer index; the forward launch
            # and the backward launch of a layer get the same value
            draw = int(torch.randint(0, 2 ** 62, (1,)).item())
            rank = 0
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                rank = torch.distributed.get_rank()
            base = (draw * 0x9E3779B97F4A7C15 + (rank + 1) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
            for fwd, bwd, idx in self._drop_ops:
                fwd.seed = (base + idx * 0x2545F4914F6CDD1D) & 0xFFFFFFFFFFFFFFFF
                if bwd is not None:
                    bwd.seed = fwd.seed
        check(lib().anoddpm_run_ops(self.fwd_array, len(self.fwd_list), _lib.current_stream()), "UNet training forward")
        return self.y

    def run_backward(self, x, dy):
        """Accumulates every parameter gradient into its destination; returns d(x) when the plan was built with want_dx."""
        fresh = [k for k, p in self.named.items() if p.grad is None]
        if fresh:
            if len(fresh) == len(self.named):
                self.arena.zero_()
            else:
                for k in fresh:
                    self.gview[k].zero_()
        self.dy.copy_(dy.reshape(self.dy.shape))
        self.stem_bwd_args.x = x.data_ptr()
        from .training import reducer_of
        red = reducer_of(self.model)
        if red is not None and any(self.named[k].requires_grad for k in fresh):
            # (frozen parameters never get a .grad and are not in the flat buffers: they do not count)
            # every rank must cut its backward at the same places (the collectives are issued in bucket order): with a reducer
            # attached the gradients are bound to the flat views before the forward (UNetModel._forward_autograd), so a
            # missing .grad here means they were dropped between forward and backward
            raise _lib.AnoddpmError("UNetModel training plan: .grad of some parameters was set to None between forward and backward "
                                    "while a GradAllReducer is attached")
        if red is not None:
            # data parallel: the op list is cut where a gradient bucket becomes final, and the bucket's all-reduce is enqueued
            # right there -- RCCL's stream picks it up behind the ops already launched and runs beside the rest of the backward
            lo = 0
            for hi, buckets in self.reduce_schedule(red):
                if hi > lo:
                    check(lib().anoddpm_run_ops(self._bwd_slice(lo), hi - lo, _lib.current_stream()),
                          "UNet training backward")
                for b in buckets:
                    red.launch_bucket(b, ops_done=hi)
                lo = hi
            if lo < len(self.bops):
                check(lib().anoddpm_run_ops(self._bwd_slice(lo), len(self.bops) - lo,
                                            _lib.current_stream()), "UNet training backward")
        else:
            check(lib().anoddpm_run_ops(self.bwd_array, len(self.bops), _lib.current_stream()), "UNet training backward")
        for k in fresh:
            if self.named[k].requires_grad:                  # frozen parameters: their gradient stays plan-owned scratch
                self.named[k].grad = self.gview[k]
        return self.dx

    def _bwd_slice(self, lo):
        return ctypes.cast(ctypes.addressof(self.bwd_array) + lo * ctypes.sizeof(Op), ctypes.POINTER(Op))

    def reduce_schedule(self, red):
        """[(backward op count, [bucket ids])]: after that many ops every gradient of those buckets of `red`
        (training.GradAllReducer) is final.  A parameter's gradient is final after the LAST backward stage that wrote it
        (bwd_marks); parameters no stage writes (unused) are final from the start."""
        key = (red.bounds, tuple(red.flat.names))      # not id(red): CPython reuses ids, a stale schedule would reduce too early
        hit = getattr(self, "_sched", None)
        if hit is not None and hit[0] == key:
            return hit[1]
        final = {}
        for end, keys in self.bwd_marks:
            for k in keys:
                final[k] = end
        names = red.flat.names
        at = {}
        for b, (_, _, members) in enumerate(red.buckets):
            end = max([final.get(names[i], 0) for i in members] + [0])
            at.setdefault(end, []).append(b)
        sched = sorted(at.items())
        self._sched = (key, sched)
        return sched


class TrainPlanFunction(torch.autograd.Function):
    """y = UNet(x, t) on the training plan.  `anchor` is any tensor that requires grad (a parameter): it makes autograd
    call backward() even when x needs no gradient; parameter gradients are accumulated in place by the kernels, so
    backward() returns no gradient for it."""

    @staticmethod
    def forward(ctx, x, t, anchor, plan):
        xin = x.detach()
        if xin.dtype != torch.float32 or not xin.is_contiguous():
            xin = xin.float().contiguous()
        if xin.data_ptr() % 16:
            xin = xin.clone()                        # a view at an odd storage offset: the stem kernel reads 16-byte rows
        tt = t.detach()
        if tt.dtype != torch.int64 or tt.device != x.device or not tt.is_contiguous():
            tt = tt.to(device=x.device, dtype=torch.int64).contiguous()
        y = plan.run_forward(xin, tt)
        plan.fwd_epoch = getattr(plan, "fwd_epoch", 0) + 1
        ctx.plan, ctx.xin, ctx.epoch, ctx.x_dtype = plan, xin, plan.fwd_epoch, x.dtype
        return y.clone().to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        plan = ctx.plan
        if ctx.epoch != plan.fwd_epoch:
            raise _lib.AnoddpmError("UNetModel training plan: backward() of a forward whose activations were overwritten by a "
                                    "later forward of the same (batch, size); run one forward/backward pair at a time")
        if not plan.params_match():
            raise _lib.AnoddpmError("UNetModel training plan: parameters or their .grad tensors moved between forward and backward")
        dx = plan.run_backward(ctx.xin, dy.detach().float().contiguous())
        return (dx.clone().to(ctx.x_dtype) if (ctx.needs_input_grad[0] and dx is not None) else None), None, None, None
