"""The backward ledger: every launch of a training plan's backward list (TrainPlan.bops) recomputed in fp64 from the buffers it
actually read.  Shared by tests/test_backward_reference.py (CPU: the fp64 statements against fp64 autograd, the static checks on
hand-made structs) and tests/test_gpu_backward_ledger.py (device: real plans).  No device and no project kernel is needed here:
the structs are the ctypes mirrors of include/anoddpm_hip.h, the pointers in them are resolved against the tensors the plan keeps
alive (CPU tensors work as well as device tensors), and every statement is plain torch in fp64 on `dev`.

  1. AddressMap        pointer -> (tensor, element offset); strided regions, bounds asserted
  2. fp64 statements   what each backward op code computes (anoddpm_hip.h; UNet.py through the reference's expressions)
  3. Ledger            launches grouped by the region they write: expected content = sum of the writers' contributions in list
                       order; first writer overwrites, later ones accumulate (checked from the structs before any arithmetic);
                       an output region overlaps no input region unless the launch is one of the declared in-place forms
  4. block_figure      per image and per block of 64 channels, max |got - ref| / max |ref| within the (image, block)

A plan buffer must be written before it is read within a step: the ledger reads the buffers AFTER a step and relies on the plan
never reusing an activation or gradient buffer (one torch.empty per _Plan.buf call)."""
import ctypes

import torch

from anoddpm_amd import _lib

CB = 64                                  # channels per block of the error metric

# Bars, by the launch's own fields; each from the op test of the same kernel (tests/test_gpu_ops.py, tests/test_gpu_train_ops.py)
BAR_WINO = 1e-4                          # 3x3, cfg 3 / 2 / 6: test_winograd_f43_conv, test_winograd_conv, test_wino23s_conv
BAR_CONV3 = 2e-5                         # 3x3 direct / small-map: TOL of test_gpu_ops.py
BAR_CONV1 = 2e-5                         # 1x1 (cfg 0 / 1 / 4 / 5) and the attention GEMMs: TOL (test_streaming_pointwise_conv: 1e-5)
BAR_GN = 2e-5                            # OP_GN_BWD dx / dgamma / dbeta and the gnb_partial rows: test_gn_silu_backward,
#                                          test_f43_data_gradient_writes_the_gn_backward_partials
BAR_SOFTMAX = 2e-5                       # softmax backward chain: test_softmax_backward_and_transpose, 1e-5 per op, two ops
# the four bars below are the caps of tests/train_op_cases.py, whose element tests (tests/test_gpu_train_op_elements.py) hold the same
# kernels per output row to max(FLOOR, 4 r32) under them, and run colsum_fold (exempt here) at the shapes of its unrolled loop
BAR_LINEAR = 1e-5                        # test_linear_small_backward
BAR_HEAD = 2e-5                          # test_conv_head_backward, test_conv_stem_backward
BAR_HEAD_DW = 5e-5                       # test_conv_head_backward (dW)
BAR_RESAMPLE = 1e-6                      # test_resample_backward_modes_and_colsum_fold

EXEMPT = (_lib.OP_WGRAD3, _lib.OP_WGRAD1, _lib.OP_COLSUM_FOLD)        # tests/test_gpu_wgrad_plan.py replays these


class LedgerError(AssertionError):
    pass


# ============================================================================================================ 1. pointers
class Region:
    """Elements a launch addresses: tensor.reshape(-1)[off + sum_i idx_i * strides_i], idx < shape."""

    def __init__(self, ptr, tensor, off, shape, strides, name=""):
        self.ptr, self.tensor, self.off, self.name = int(ptr), tensor, int(off), name
        self.shape, self.strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        self.isz = tensor.element_size()

    @property
    def key(self):
        return (self.ptr, self.shape, self.strides)

    @property
    def last(self):
        return sum((n - 1) * s for n, s in zip(self.shape, self.strides))

    @property
    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def span(self):
        return self.ptr, self.ptr + (self.last + 1) * self.isz

    def raw(self):
        """The addressed elements in their own dtype, on the tensor's device."""
        flat = self.tensor.detach().reshape(-1)              # (as_strided counts its offset from the start of the STORAGE)
        return torch.as_strided(flat, self.shape, self.strides, flat.storage_offset() + self.off)

    def read(self, dev="cpu"):
        return self.raw().to(device=dev, dtype=torch.float64)

    def __repr__(self):
        return f"{self.name or 'region'}@{self.ptr:#x}{list(self.shape)}/{list(self.strides)}"


class AddressMap:
    def __init__(self):
        self.ents = []                   # (first byte, one past the last byte, tensor, name)
        self._hit = {}

    def add(self, t, name):
        if t is None or not torch.is_tensor(t) or t.numel() == 0:
            return
        if not t.is_contiguous():
            raise LedgerError(f"{name}: plan tensors are contiguous")
        self.ents.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), t, name))
        self._hit.clear()

    def resolve(self, ptr):
        """(tensor, element offset, name) of the smallest registered tensor that holds `ptr` (interior pointers are normal)."""
        if not ptr:
            raise LedgerError("null pointer where a buffer is expected")
        if ptr in self._hit:
            return self._hit[ptr]
        best = None
        for lo, hi, t, name in self.ents:
            if lo <= ptr < hi and (best is None or hi - lo < best[1] - best[0]):
                best = (lo, hi, t, name)
        if best is None:
            raise LedgerError(f"pointer {ptr:#x} resolves to no tensor of the plan")
        lo, _, t, name = best
        if (ptr - lo) % t.element_size():
            raise LedgerError(f"pointer {ptr:#x} is not aligned to the elements of {name}")
        self._hit[ptr] = (t, (ptr - lo) // t.element_size(), name)
        return self._hit[ptr]

    def region(self, ptr, shape, strides, what=""):
        t, off, name = self.resolve(ptr)
        r = Region(ptr, t, off, shape, strides, f"{what}:{name}" if what else name)
        if any(s < 1 for s in r.shape) or any(s < 0 for s in r.strides):
            raise LedgerError(f"{r}: bad shape / strides")
        if off + r.last + 1 > t.numel():
            raise LedgerError(f"{r}: reaches element {off + r.last} of a tensor of {t.numel()} ({what})")
        return r

    def view(self, ptr, B, rows, width, batch_stride, ld, dev="cpu"):
        """The [B, rows, width] region a launch addresses (row pitch ld, batch stride batch_stride), as an fp64 tensor; asserts that
        it lies inside the tensor `ptr` resolves to."""
        return self.region(ptr, (B, rows, width), (batch_stride, ld, 1)).read(dev)


def _offsets(r, cap=1 << 22):
    if r.numel > cap:
        return None
    idx = torch.zeros(1, dtype=torch.int64)
    for n, s in zip(r.shape, r.strides):
        idx = (idx[:, None] + torch.arange(n, dtype=torch.int64)[None, :] * s).reshape(-1)
    return idx * r.isz + r.ptr


def overlaps(a, b):
    """True when the two regions share an element.  Exact for regions of up to 4M elements and for regions with one row pitch whose
    columns stay inside a row (the q / k / v column ranges of a qkv buffer); conservative (True) otherwise."""
    (alo, ahi), (blo, bhi) = a.span(), b.span()
    if ahi <= blo or bhi <= alo:
        return False
    if a.key == b.key:
        return True

    def rows_cols(r):
        """(row pitch, in-row element offsets) when every other stride is a multiple of the row pitch, else None"""
        if len(r.shape) < 2 or r.strides[-1] != 1:
            return None
        ld = r.strides[-2]
        cols = torch.arange(r.shape[-1], dtype=torch.int64)
        for n, s in zip(r.shape[:-2], r.strides[:-2]):
            if n > 1 and s % ld:
                if s >= ld:
                    return None
                cols = (cols[None, :] + torch.arange(n, dtype=torch.int64)[:, None] * s).reshape(-1)
        return (ld, cols) if int(cols.max()) < ld else None
    ra, rb = rows_cols(a), rows_cols(b)
    if ra is not None and rb is not None and ra[0] == rb[0] and a.isz == b.isz and (b.ptr - a.ptr) % a.isz == 0:
        ld = ra[0]
        m = ((b.ptr - a.ptr) // a.isz) % ld
        cb = rb[1] + m
        if int(cb.max()) < ld:
            return bool(torch.isin(ra[1], cb).any())
    oa, ob = _offsets(a), _offsets(b)
    if oa is None or ob is None:
        return True
    return bool(torch.isin(oa, ob).any())


# ============================================================================================================ 2. fp64 statements
def silu(y):
    return y * torch.sigmoid(y)


def dsilu(y):
    s = torch.sigmoid(y)
    return s * (1 + y * (1 - s))


def conv3x3_input(dy, w):
    """Data gradient of a 3x3 / stride 1 / pad 1 convolution: dy NHWC [B, H, W, N], w OIHW [N, K, 3, 3] -> da NHWC [B, H, W, K],
    da[y, x, k] = sum_{ky, kx, n} dy[y - ky + 1, x - kx + 1, n] * w[n, k, ky, kx], as nine shifted matrix products."""
    B, H, W, N = dy.shape
    p = torch.nn.functional.pad(dy, (0, 0, 1, 1, 1, 1))
    da = torch.zeros(B, H, W, w.shape[1], dtype=dy.dtype, device=dy.device)
    for ky in range(3):
        for kx in range(3):
            da += p[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W, :] @ w[:, :, ky, kx]
    return da


def conv3x3_weight(a, dy):
    """a NHWC [B, H, W, K], dy NHWC [B, H, W, N] -> dw OIHW [N, K, 3, 3] = sum_{b, y, x} dy[y, x, n] * a[y + ky - 1, x + kx - 1, k]."""
    B, H, W, K = a.shape
    p = torch.nn.functional.pad(a, (0, 0, 1, 1, 1, 1))
    dw = torch.zeros(dy.shape[3], K, 3, 3, dtype=a.dtype, device=a.device)
    d = dy.reshape(-1, dy.shape[3])
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = d.T @ p[:, ky:ky + H, kx:kx + W, :].reshape(-1, K)
    return dw


def conv1x1_input(dy, w, k0=0, kc=None):
    """dy [B, P, N], w [N, K] -> dy @ w[:, k0:k0 + kc] per pixel."""
    kc = w.shape[1] - k0 if kc is None else kc
    return dy @ w[:, k0:k0 + kc]


def resample(x, mode, scale=1.0):
    """anoddpm_resample2x on NHWC [B, H, W, C]: 1 nearest x2, 2 the 2x2 average, 3 the even pixels, 4 the adjoint of 3."""
    B, H, W, C = x.shape
    if mode == 1:
        out = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    elif mode == 2:
        out = x.reshape(B, H // 2, 2, W // 2, 2, C).mean(dim=(2, 4))
    elif mode == 3:
        out = x[:, ::2, ::2, :]
    elif mode == 4:
        out = torch.zeros(B, 2 * H, 2 * W, C, dtype=x.dtype, device=x.device)
        out[:, ::2, ::2, :] = x
    else:
        raise LedgerError(f"resample mode {mode}")
    return out * (scale if scale else 1.0)


def _groups(t, G):
    """[B, ..., C] -> per-channel view helpers: index of the group of channel c"""
    C = t.shape[-1]
    return torch.arange(C, device=t.device) // (C // G)


def gn_dy(x, da_src, gamma, beta, mean, rstd, act):
    """xhat and dy = da * silu'(gamma * xhat + beta) of anoddpm_gn_bwd_args: x, da_src [B, P, C]; mean, rstd [B, G]."""
    g = _groups(x, mean.shape[1])
    xhat = (x - mean[:, g][:, None, :]) * rstd[:, g][:, None, :]
    dy = da_src * dsilu(gamma * xhat + beta) if act else da_src
    return xhat, dy


def gn_backward(x, da, gamma, beta, mean, rstd, act, a_mode, Hs, Ws, dres=None):
    """anoddpm_hip.h:728-760.  x [B, Hs * Ws, C] (the concatenated sources), da [B, Pa, C] the gradient of the tensor the
    convolution read: Pa = Hs * Ws (a_mode 0), 4 Hs Ws (1: the four children are summed), Hs Ws / 4 (2: a quarter of the parent).
    Returns dx [B, Hs * Ws, C] (+ dres), dgamma [C], dbeta [C]."""
    B, P, C = x.shape
    G = mean.shape[1]
    if a_mode == 1:
        da = da.reshape(B, Hs, 2, Ws, 2, C).sum(dim=(2, 4)).reshape(B, P, C)
    elif a_mode == 2:
        da = (0.25 * da).reshape(B, Hs // 2, 1, Ws // 2, 1, C).expand(B, Hs // 2, 2, Ws // 2, 2, C).reshape(B, P, C)
    xhat, dy = gn_dy(x, da, gamma, beta, mean, rstd, act)
    dgamma, dbeta = (dy * xhat).sum(dim=(0, 1)), dy.sum(dim=(0, 1))
    gd = gamma * dy
    cg = C // G
    m1 = gd.reshape(B, P, G, cg).mean(dim=(1, 3))                              # [B, G]
    m2 = (gd * xhat).reshape(B, P, G, cg).mean(dim=(1, 3))
    g = _groups(x, G)
    dx = rstd[:, g][:, None, :] * (gd - m1[:, g][:, None, :] - xhat * m2[:, g][:, None, :])
    if dres is not None:
        dx = dx + dres
    return dx, dgamma, dbeta


def gn_tile_partials(x, da, gamma, beta, mean, rstd, H, W):
    """anoddpm_hip.h:252-262: gnb_partial[b][tile][c] = {sum dy, sum dy * xhat} over the 16 x 16 pixels of the tile (tiles row-major),
    dy = da * silu'(gamma * xhat + beta).  x, da [B, H * W, C] -> [B, (H / 16) * (W / 16), C, 2]."""
    B, P, C = x.shape
    xhat, dy = gn_dy(x, da, gamma, beta, mean, rstd, 1)

    def tiles(t):
        return t.reshape(B, H // 16, 16, W // 16, 16, C).sum(dim=(2, 4)).reshape(B, -1, C)
    return torch.stack([tiles(dy), tiles(dy * xhat)], dim=-1)


def attn_gemm(A, Bm, b_mode, alpha=1.0):
    """The activation-operand forms of anoddpm_igemm per (image, head): A [..., P, K]; b_mode 1: Bm rows [N][K] -> alpha A Bm^T;
    b_mode 2: Bm rows [K][N] -> alpha A Bm."""
    return alpha * (A @ (Bm.transpose(-1, -2) if b_mode == 1 else Bm))


def softmax_backward(p, dp):
    """ds = p o (dp - rowsum(dp o p))"""
    return p * (dp - (dp * p).sum(dim=-1, keepdim=True))


def attention_backward(q, k, v, p, datt, alpha):
    """QKVAttention backward per (image, head) as the plan chains it: q, k, v, datt [..., L, ch], p = softmax(alpha q k^T) [..., L, L].
    Returns dS, dV, dQ, dK."""
    dP = attn_gemm(datt, v, 1)                               # dP = dAtt v^T
    dS = softmax_backward(p, dP)
    dV = attn_gemm(p.transpose(-1, -2), datt, 2)             # dV = P^T dAtt
    dQ = attn_gemm(dS, k, 2, alpha)                          # dQ = alpha dS k
    dK = attn_gemm(dS.transpose(-1, -2), q, 2, alpha)        # dK = alpha dS^T q
    return dS, dV, dQ, dK


def linear_backward(x, w, dy, act_in):
    """y = act_in(x) W^T + b: dw [N, K], db [N], dx [B, K]."""
    a = silu(x) if act_in else x
    dx = dy @ w
    if act_in:
        dx = dx * dsilu(x)
    return dy.T @ a, dy.sum(dim=0), dx


def linear_backward_batch(x, jobs, act_in):
    """Several linear layers on one input: jobs = [(w [N_j, K], dy [B, N_j])] -> [(dw_j, db_j)], dx = act_in'(x) * sum_j dy_j w_j."""
    outs, dx = [], torch.zeros_like(x)
    a = silu(x) if act_in else x
    for w, dy in jobs:
        outs.append((dy.T @ a, dy.sum(dim=0)))
        dx = dx + dy @ w
    return outs, (dx * dsilu(x) if act_in else dx)


def head_backward(x, scale, shift, w, dy):
    """x NHWC [B, H, W, C], scale / shift [B, C], w OIHW [Co, C, 3, 3], dy NCHW [B, Co, H, W] -> da NHWC, dw, db."""
    a = silu(x * scale[:, None, None, :] + shift[:, None, None, :])
    d = dy.permute(0, 2, 3, 1)
    return conv3x3_input(d, w), conv3x3_weight(a, d), dy.sum(dim=(0, 2, 3))


def stem_backward(x, w, dy):
    """x NCHW [B, Ci, H, W], w OIHW [Co, Ci, 3, 3], dy NHWC [B, H, W, Co] -> dw, db, dx NCHW."""
    return conv3x3_weight(x.permute(0, 2, 3, 1), dy), dy.sum(dim=(0, 1, 2)), conv3x3_input(dy, w).permute(0, 3, 1, 2)


def dropout_backward(d, mask, p):
    return d * mask / (1.0 - p)


# ============================================================================================================ 4. metric
def block_figure(got, ref, budget=None, den=None, bar=None):
    """got, ref [Z, rows, width] fp64.  Per z and per block of CB channels: err = max |got - ref|, den = max |ref| (or the given
    [Z, blocks] denominators of a fan-in region), budget = bar * den (or the given one).  Returns (figure = err / den at the worst
    (z, block) relative to its budget, (z, first channel of the block), the bar there = budget / den, ok)."""
    Z, _, width = ref.shape
    nb = -(-width // CB)
    if not torch.isfinite(got).all():
        return float("inf"), None, (float("nan") if bar is None else bar), False
    err = torch.stack([(got - ref)[:, :, j * CB:(j + 1) * CB].abs().amax(dim=(1, 2)) for j in range(nb)], dim=1)
    if den is None:
        den = torch.stack([ref[:, :, j * CB:(j + 1) * CB].abs().amax(dim=(1, 2)) for j in range(nb)], dim=1)
    if budget is None:
        budget = bar * den
    ok = bool(((err < budget) | ((den == 0) & (err == 0))).all())
    ratio = torch.where(budget > 0, err / budget.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(ratio.reshape(-1).argmax())
    z, j = divmod(i, nb)
    d = float(den[z, j])
    return (float(err[z, j]) / d if d > 0 else (0.0 if float(err[z, j]) == 0 else float("inf"))), (z, j * CB), \
        (float(budget[z, j]) / d if d > 0 else 0.0), ok


def block_max(t):
    """[Z, rows, width] -> [Z, blocks] of max |t|"""
    nb = -(-t.shape[2] // CB)
    return torch.stack([t[:, :, j * CB:(j + 1) * CB].abs().amax(dim=(1, 2)) for j in range(nb)], dim=1)


def tensor_figure(got, ref, bar):
    """Parameter-shaped outputs: max |got - ref| / max |ref| over the tensor."""
    if not torch.isfinite(got).all():
        return float("inf"), None, bar, False
    den = float(ref.abs().max())
    err = float((got - ref).abs().max())
    fig = err / den if den > 0 else (0.0 if err == 0 else float("inf"))
    return fig, None, bar, fig < bar or (den == 0 and err == 0)


# ============================================================================================================ 3. ledger
class Out:
    """One written region of a launch.  kind "data": an activation gradient (first writer overwrites, later ones accumulate);
    "param": a parameter gradient, accumulated into a destination that is zero at the start of the backward."""

    def __init__(self, name, region, acc, bar, kind="data", z3=None):
        self.name, self.region, self.acc, self.bar, self.kind = name, region, bool(acc), bar, kind
        # [images (x heads), rows, channels]; a [B, K] output has one row per image
        self.z3 = z3 or (lambda t: t.reshape(-1, t.shape[-2], t.shape[-1]) if t.dim() >= 3 else t.reshape(t.shape[0], 1, -1))


class Launch:
    def __init__(self, idx, what, cfg=""):
        self.idx, self.what, self.cfg = idx, what, cfg      # idx: positions in bops
        self.inputs, self.outs, self.inplace = [], [], []   # inplace: keys of input regions an output may coincide with
        self.compute = None                                 # dev -> {out name: fp64 contribution}
        self.st = None                                      # the argument struct (single-op launches)


class Ledger:
    def __init__(self, plan, x=None, dev="cpu"):
        """plan: a TrainPlan after a step (or an object with its keep / named / pptr / gptr / gview / pack_ops / _drop_ops / bops)."""
        self.plan, self.dev = plan, torch.device(dev)
        am = self.amap = AddressMap()
        for i, t in enumerate(plan.keep):
            am.add(t if torch.is_tensor(t) else None, f"keep[{i}]")
        for k, p in plan.named.items():
            am.add(p.detach(), k)
            g = plan.gview.get(k)
            g = p.grad if g is None else g
            am.add(g, "grad:" + k)
        for n in ("arena", "dy", "dx", "y"):
            am.add(getattr(plan, n, None), n)
        am.add(x.detach() if x is not None else None, "x")
        self.pname = {ptr: k for k, ptr in plan.pptr.items()}
        self.packs = {st.out: st for _, st in plan.pack_ops}
        self.drop_fwd = {ctypes.addressof(b): f for f, b, _ in getattr(plan, "_drop_ops", []) if b is not None}
        self.launches, self.exempt = [], []
        self._describe_all()

    # ------------------------------------------------------------------ helpers
    def reg(self, ptr, shape, strides, what):
        return self.amap.region(ptr, shape, strides, what)

    def param(self, ptr, what):
        """The PARAMETER at ptr (not a packed copy), as a region over the whole tensor."""
        k = self.pname.get(ptr)
        if k is None:
            raise LedgerError(f"{what}: {ptr:#x} is not the start of a parameter")
        p = self.plan.named[k]
        return self.reg(ptr, tuple(p.shape), tuple(p.stride()), f"{what}={k}")

    def pgrad(self, ptr, shape, what):
        st, n = [], 1
        for s in reversed(shape):
            st.insert(0, n)
            n *= s
        r = self.reg(ptr, shape, st, what)
        if not r.name.split(":", 1)[1].startswith(("grad:", "arena")):
            raise LedgerError(f"{r}: a parameter gradient lands outside the gradient destinations")
        return r

    def weight_of_pack(self, bmat, what):
        pk = self.packs.get(bmat)
        if pk is None:
            raise LedgerError(f"{what}: bmat {bmat:#x} is the output of no pack job")
        return pk, self.param(pk.w, what + ".w")

    # ------------------------------------------------------------------ descriptions
    def _describe_all(self):
        bops, i = self.plan.bops, 0
        while i < len(bops):
            code, st = bops[i]
            if code in EXEMPT:
                self.exempt.append(i)
                i += 1
                continue
            n = 1
            if code == _lib.OP_IGEMM and st.b_mode in (1, 2):
                L, n = self._attention_chain(i), 7
            elif code == _lib.OP_IGEMM and st.ks == 3:
                drop = i + 1 < len(bops) and bops[i + 1][0] == _lib.OP_DROPOUT and bops[i + 1][1].x == st.out
                L, n = self._dgrad3(i, st, bops[i + 1][1] if drop else None), (2 if drop else 1)
            elif code == _lib.OP_IGEMM and st.ks == 1:
                L = self._dgrad1(i, st)
            elif code == _lib.OP_GN_BWD:
                L = self._gn_bwd(i, st)
            elif code == _lib.OP_RESAMPLE:
                L = self._resample(i, st)
            elif code == _lib.OP_LINEAR_BWD:
                L = self._linear(i, st)
            elif code == _lib.OP_LINEAR_BWD_BATCH:
                L = self._linear_batch(i, st)
            elif code == _lib.OP_HEAD_BWD:
                L = self._head(i, st)
            elif code == _lib.OP_STEM_BWD:
                L = self._stem(i, st)
            else:
                raise LedgerError(f"bops[{i}]: op code {code} has no fp64 statement in the ledger")
            L.st = st
            self.launches.append(L)
            i += n

    def _plain_operand(self, st, what):
        if st.gn_scale or st.fold_gamma or st.act or st.a_mode or st.c1 or st.a1 or st.bias or st.temb or st.heads != 1 or st.b_mode or st.res_mode \
                or st.alpha != 1.0:
            raise LedgerError(f"{what}: a data-gradient launch has a plain single-source operand and no bias / embedding")

    def _res(self, L, st, out, what):
        """`res` of a data-gradient launch: the output itself (accumulate in place, identical strides) or another input."""
        if not st.res:
            return None, False
        r = self.reg(st.res, out.shape, (st.r_bs, st.res_ld, 1), what + ".res")
        L.inputs.append(r)
        if st.res == st.out:
            if r.key != out.key:
                raise LedgerError(f"{what}: res == out with different strides")
            L.inplace.append(r.key)
            return None, True
        return r, False

    def _dgrad3(self, i, st, drop):
        what = f"bops[{i}] IGEMM 3x3 dgrad"
        self._plain_operand(st, what)
        B, H, W, N, Kc = st.B, st.H, st.W, st.c0, st.N
        wino = st.cfg in (2, 3, 6)
        L = Launch([i] + ([i + 1] if drop else []), f"dgrad3{'+dropout' if drop else ''} B={B} {H}x{W} N={N}->K={Kc}" +
                   (" gnb" if st.gnb_partial else "") + (" res=out" if st.res and st.res == st.out else ""), f"cfg={st.cfg} ksplit={st.ksplit}")
        dy = self.reg(st.a0, (B, H * W, N), (st.a0_bs, st.a0_ld, 1), what + ".a0")
        out = self.reg(st.out, (B, H * W, Kc), (st.o_bs, st.out_ld, 1), what + ".out")
        pk, w = self.weight_of_pack(st.bmat, what)
        if not (pk.bwd == 1 and pk.kind == {3: 5, 2: 1, 6: 1}.get(st.cfg, 0) and (pk.N, pk.K) == (N, Kc) and w.shape == (N, Kc, 3, 3)):
            raise LedgerError(f"{what}: packed twin kind={pk.kind} bwd={pk.bwd} N={pk.N} K={pk.K} does not fit cfg {st.cfg}, {N}->{Kc}")
        L.inputs += [dy, w, self.reg(st.bmat, (pk.N * pk.K * {0: 9, 1: 16, 5: 36}[pk.kind],), (1,), what + ".bmat")]
        res, acc = self._res(L, st, out, what)
        bar = BAR_WINO if wino else BAR_CONV3
        L.outs.append(Out("da", out, acc, bar))
        mask = None
        if drop is not None:
            fwd = self.drop_fwd.get(ctypes.addressof(drop))
            if fwd is None or drop.mode != 1 or drop.out != drop.x or drop.n != H * W * Kc or drop.B != B or acc:
                raise LedgerError(f"{what}: in-place dropout backward without its forward twin / with other sizes")
            mask = self.reg(fwd.out, (B, H * W, Kc), (H * W * Kc, Kc, 1), what + ".dropped")
            L.inputs.append(mask)
            p_drop = drop.p
        gnb = None
        if st.gnb_partial:
            c0, c1 = st.gnb_c0, Kc - st.gnb_c0
            if H % 16 or W % 16:
                raise LedgerError(f"{what}: gnb_partial on a map that is not a multiple of 16")
            T = (H // 16) * (W // 16)
            xs = [self.reg(st.gnb_x0, (B, H * W, c0), (st.gnb_x0_bs, st.gnb_x0_ld, 1), what + ".gnb_x0")]
            if c1:
                xs.append(self.reg(st.gnb_x1, (B, H * W, c1), (st.gnb_x1_bs, st.gnb_x1_ld, 1), what + ".gnb_x1"))
            G = st.gnb_groups
            gnb = (xs, self.reg(st.gnb_gamma, (Kc,), (1,), what + ".gnb_gamma"), self.reg(st.gnb_beta, (Kc,), (1,), what + ".gnb_beta"),
                   self.reg(st.gnb_mean, (B, G), (G, 1), what + ".gnb_mean"), self.reg(st.gnb_rstd, (B, G), (G, 1), what + ".gnb_rstd"))
            L.inputs += xs + list(gnb[1:])
            part = self.reg(st.gnb_partial, (B, T, Kc, 2), (T * Kc * 2, Kc * 2, 2, 1), what + ".gnb_partial")
            # the two sums are judged separately: [B, T, C, 2] -> [2 B, T, C]
            L.outs.append(Out("gnb_partial", part, False, BAR_GN, z3=lambda t: t.permute(3, 0, 1, 2).reshape(-1, t.shape[1], t.shape[2])))

        def compute(dev):
            da = conv3x3_input(dy.read(dev).reshape(B, H, W, N), w.read(dev)).reshape(B, H * W, Kc)
            if res is not None:
                da = da + res.read(dev)
            if mask is not None:
                da = dropout_backward(da, (mask.read(dev) != 0).double(), p_drop)
            r = {"da": da}
            if gnb is not None:
                # the epilogue holds the da it stores: the sums are stated on the stored values, so that this row judges the reduction
                x = torch.cat([t.read(dev) for t in gnb[0]], dim=2)
                r["gnb_partial"] = gn_tile_partials(x, out.read(dev), gnb[1].read(dev), gnb[2].read(dev), gnb[3].read(dev), gnb[4].read(dev), H, W)
            return r
        L.compute = compute
        return L

    def _dgrad1(self, i, st):
        what = f"bops[{i}] IGEMM 1x1 dgrad"
        self._plain_operand(st, what)
        B, P, N, Kc = st.B, st.H * st.W, st.c0, st.N
        L = Launch([i], f"dgrad1 B={B} P={P} N={N}->K={Kc}" + (" res=out" if st.res and st.res == st.out else ""), f"cfg={st.cfg} ksplit={st.ksplit}")
        dy = self.reg(st.a0, (B, P, N), (st.a0_bs, st.a0_ld, 1), what + ".a0")
        out = self.reg(st.out, (B, P, Kc), (st.o_bs, st.out_ld, 1), what + ".out")
        pk, w = self.weight_of_pack(st.bmat, what)
        if not (pk.bwd == 1 and pk.kind == 2 and pk.N == N and pk.kc == Kc and w.shape[0] == N and pk.k0 + pk.kc <= pk.K):
            raise LedgerError(f"{what}: packed twin kind={pk.kind} bwd={pk.bwd} N={pk.N} k0={pk.k0} kc={pk.kc} does not fit {N}->{Kc}")
        L.what += f" k0={pk.k0}"
        L.inputs += [dy, w, self.reg(st.bmat, (N * Kc,), (1,), what + ".bmat")]
        res, acc = self._res(L, st, out, what)
        L.outs.append(Out("da", out, acc, BAR_CONV1))
        k0 = pk.k0

        def compute(dev):
            da = conv1x1_input(dy.read(dev), w.read(dev).reshape(N, -1), k0, Kc)
            return {"da": da if res is None else da + res.read(dev)}
        L.compute = compute
        return L

    def _gn_bwd(self, i, st):
        what = f"bops[{i}] GN_BWD"
        B, c0, c1, Hs, Ws, G, am = st.B, st.c0, st.c1, st.Hs, st.Ws, st.groups, st.a_mode
        C, P = c0 + c1, st.Hs * st.Ws
        Pa = {0: P, 1: 4 * P, 2: P // 4}[am]
        L = Launch([i], f"gn_bwd B={B} {Hs}x{Ws} C={c0}+{c1} act={st.act} a_mode={am} acc_dx={st.acc_dx}" + (" dres" if st.dres else "") +
                   (" partial_ready" if st.partial_ready else ""), f"nslab={st.nslab}")
        xs = [self.reg(st.x0, (B, P, c0), (st.x0_bs, st.x0_ld, 1), what + ".x0")]
        dxs = [self.reg(st.dx0, (B, P, c0), (st.dx0_bs, st.dx0_ld, 1), what + ".dx0")]
        if c1:
            xs.append(self.reg(st.x1, (B, P, c1), (st.x1_bs, st.x1_ld, 1), what + ".x1"))
            dxs.append(self.reg(st.dx1, (B, P, c1), (st.dx1_bs, st.dx1_ld, 1), what + ".dx1"))
        da = self.reg(st.da, (B, Pa, C), (st.da_bs, st.da_ld, 1), what + ".da")
        gamma, beta = self.param(st.gamma, what + ".gamma"), self.param(st.beta, what + ".beta")
        mean, rstd = self.reg(st.mean, (B, G), (G, 1), what + ".mean"), self.reg(st.rstd, (B, G), (G, 1), what + ".rstd")
        dres = self.reg(st.dres, (B, P, C), (st.dres_bs, st.dres_ld, 1), what + ".dres") if st.dres else None
        L.inputs += xs + [da, gamma, beta, mean, rstd] + ([dres] if dres is not None else [])
        if st.partial_ready:                                 # the reduction rows are an input the kernel did not make itself
            L.inputs.append(self.reg(st.partial, (B, st.nslab, C, 2), (st.nslab * C * 2, C * 2, 2, 1), what + ".partial"))
        L.outs.append(Out("dx0", dxs[0], st.acc_dx & 1, BAR_GN))
        if c1:
            L.outs.append(Out("dx1", dxs[1], st.acc_dx & 2, BAR_GN))
        L.outs.append(Out("dgamma", self.pgrad(st.dgamma, (C,), what + ".dgamma"), True, BAR_GN, "param"))
        L.outs.append(Out("dbeta", self.pgrad(st.dbeta, (C,), what + ".dbeta"), True, BAR_GN, "param"))
        act = st.act

        def compute(dev):
            x = torch.cat([t.read(dev) for t in xs], dim=2)
            dx, dg, db = gn_backward(x, da.read(dev), gamma.read(dev), beta.read(dev), mean.read(dev), rstd.read(dev), act, am, Hs, Ws,
                                     dres.read(dev) if dres is not None else None)
            r = {"dx0": dx[:, :, :c0], "dgamma": dg, "dbeta": db}
            if c1:
                r["dx1"] = dx[:, :, c0:]
            return r
        L.compute = compute
        return L

    def _resample(self, i, st):
        what = f"bops[{i}] RESAMPLE"
        B, H, W, C, mode = st.B, st.H, st.W, st.C, st.mode
        if st.gn_scale or st.out_act:
            raise LedgerError(f"{what}: the activated second output is a forward form")
        Ho, Wo = {1: (2 * H, 2 * W), 2: (H // 2, W // 2), 3: (H // 2, W // 2), 4: (2 * H, 2 * W)}[mode]
        L = Launch([i], f"resample mode={mode} scale={st.scale:g} B={B} {H}x{W}x{C} acc={st.accumulate}")
        inp = self.reg(st.inp, (B, H * W, C), (H * W * C, C, 1), what + ".in")
        out = self.reg(st.out, (B, Ho * Wo, C), (Ho * Wo * C, C, 1), what + ".out")
        L.inputs.append(inp)
        L.outs.append(Out("out", out, st.accumulate, BAR_RESAMPLE))
        scale = st.scale
        L.compute = lambda dev: {"out": resample(inp.read(dev).reshape(B, H, W, C), mode, scale).reshape(B, Ho * Wo, C)}
        return L

    def _linear_outs(self, L, st, B, K, what, tag=""):
        N = st.N
        dw, db = self.pgrad(st.dw, (N, K), what + ".dw"), self.pgrad(st.db, (N,), what + ".db")
        L.outs.append(Out("dw" + tag, dw, True, BAR_LINEAR, "param"))
        L.outs.append(Out("db" + tag, db, True, BAR_LINEAR, "param"))
        w = self.param(st.w, what + ".w")
        if w.shape != (N, K):
            raise LedgerError(f"{what}: weight {w} is not [{N}, {K}]")
        dy = self.reg(st.dy, (B, N), (N, 1), what + ".dy")
        L.inputs += [w, dy]
        return w, dy

    def _linear(self, i, st):
        what = f"bops[{i}] LINEAR_BWD"
        B, K = st.B, st.K
        if not st.acc_w:
            raise LedgerError(f"{what}: parameter gradients are accumulated (acc_w)")
        L = Launch([i], f"linear_bwd B={B} K={K} N={st.N} act_in={st.act_in} acc_x={st.acc_x}")
        x = self.reg(st.x, (B, K), (K, 1), what + ".x")
        L.inputs.append(x)
        w, dy = self._linear_outs(L, st, B, K, what)
        if st.dx:
            L.outs.append(Out("dx", self.reg(st.dx, (B, K), (K, 1), what + ".dx"), st.acc_x, BAR_LINEAR))
        act = st.act_in

        def compute(dev):
            dw, db, dx = linear_backward(x.read(dev), w.read(dev), dy.read(dev), act)
            return {"dw": dw, "db": db, "dx": dx}
        L.compute = compute
        return L

    def _linear_batch(self, i, st):
        what = f"bops[{i}] LINEAR_BWD_BATCH"
        B, K, nj = st.B, st.K, st.njobs
        if not st.acc_w:
            raise LedgerError(f"{what}: parameter gradients are accumulated (acc_w)")
        size = ctypes.sizeof(_lib.LinearBwdArgs)
        table = self.reg(st.jobs, (nj * size,), (1,), what + ".jobs")
        jobs = (_lib.LinearBwdArgs * nj).from_buffer_copy(bytes(table.raw().cpu().numpy().tobytes()))   # the DEVICE job table
        L = Launch([i], f"linear_bwd_batch B={B} K={K} jobs={nj} N={sorted({j.N for j in jobs})} acc_x={st.acc_x}")
        x = self.reg(st.x, (B, K), (K, 1), what + ".x")
        L.inputs += [x, table]
        if max(j.N for j in jobs) != st.max_n:
            raise LedgerError(f"{what}: max_n {st.max_n} is not the largest N of the job table")
        ops = [self._linear_outs(L, j, B, K, f"{what}.job{n}", tag=str(n)) for n, j in enumerate(jobs)]
        if st.dx:
            L.outs.append(Out("dx", self.reg(st.dx, (B, K), (K, 1), what + ".dx"), st.acc_x, BAR_LINEAR))
        act = st.act_in

        def compute(dev):
            outs, dx = linear_backward_batch(x.read(dev), [(w.read(dev), dy.read(dev)) for w, dy in ops], act)
            r = {"dx": dx}
            for n, (dw, db) in enumerate(outs):
                r[f"dw{n}"], r[f"db{n}"] = dw, db
            return r
        L.compute = compute
        return L

    def _head(self, i, st):
        what = f"bops[{i}] HEAD_BWD"
        B, H, W, C, Co = st.B, st.H, st.W, st.C, st.Cout
        L = Launch([i], f"head_bwd B={B} {H}x{W} C={C} Cout={Co}")
        x = self.reg(st.x, (B, H * W, C), (H * W * C, C, 1), what + ".x")
        sc, sh = self.reg(st.gn_scale, (B, C), (C, 1), what + ".gn_scale"), self.reg(st.gn_shift, (B, C), (C, 1), what + ".gn_shift")
        w = self.param(st.w, what + ".w")
        dy = self.reg(st.dy, (B, Co, H * W), (Co * H * W, H * W, 1), what + ".dy")
        L.inputs += [x, sc, sh, w, dy]
        L.outs.append(Out("da", self.reg(st.da, (B, H * W, C), (H * W * C, C, 1), what + ".da"), False, BAR_HEAD))
        L.outs.append(Out("dw", self.pgrad(st.dw, (Co, C, 3, 3), what + ".dw"), True, BAR_HEAD_DW, "param"))
        L.outs.append(Out("db", self.pgrad(st.db, (Co,), what + ".db"), True, BAR_HEAD, "param"))

        def compute(dev):
            da, dw, db = head_backward(x.read(dev).reshape(B, H, W, C), sc.read(dev), sh.read(dev), w.read(dev), dy.read(dev).reshape(B, Co, H, W))
            return {"da": da.reshape(B, H * W, C), "dw": dw, "db": db}
        L.compute = compute
        return L

    def _stem(self, i, st):
        what = f"bops[{i}] STEM_BWD"
        B, H, W, Ci, Co = st.B, st.H, st.W, st.Cin, st.Cout
        L = Launch([i], f"stem_bwd B={B} {H}x{W} Cin={Ci} Cout={Co} dx={int(bool(st.dx))}")
        x = self.reg(st.x, (B, Ci, H * W), (Ci * H * W, H * W, 1), what + ".x")
        w = self.param(st.w, what + ".w")
        dy = self.reg(st.dy, (B, H * W, Co), (H * W * Co, Co, 1), what + ".dy")
        L.inputs += [x, w, dy]
        L.outs.append(Out("dw", self.pgrad(st.dw, (Co, Ci, 3, 3), what + ".dw"), True, BAR_HEAD, "param"))
        L.outs.append(Out("db", self.pgrad(st.db, (Co,), what + ".db"), True, BAR_HEAD, "param"))
        if st.dx:                                            # NCHW [B, Cin, H * W]: channels are the rows, judged per image
            L.outs.append(Out("dx", self.reg(st.dx, (B, Ci, H * W), (Ci * H * W, H * W, 1), what + ".dx"), False, BAR_HEAD,
                              z3=lambda t: t.reshape(t.shape[0], 1, -1).transpose(1, 2)))

        def compute(dev):
            dw, db, dx = stem_backward(x.read(dev).reshape(B, Ci, H, W), w.read(dev), dy.read(dev).reshape(B, H, W, Co))
            return {"dw": dw, "db": db, "dx": dx.reshape(B, Ci, H * W)}
        L.compute = compute
        return L

    def _attention_chain(self, i):
        """bops[i .. i + 6]: dP = dAtt v^T; T1 = P^T; dV = T1 dAtt; dP <- dS (in place); dQ = alpha dS k; T1 = dS^T; dK = alpha T1 q.
        Two buffers change their meaning on the way (dP: dP then dS; T1: P^T then dS^T), so the chain is evaluated in list order."""
        bops = self.plan.bops
        what = f"bops[{i}..{i + 6}] attention backward"
        want = [_lib.OP_IGEMM, _lib.OP_TRANSPOSE, _lib.OP_IGEMM, _lib.OP_SOFTMAX_BWD, _lib.OP_IGEMM, _lib.OP_TRANSPOSE, _lib.OP_IGEMM]
        if i + 7 > len(bops) or [c for c, _ in bops[i:i + 7]] != want:
            raise LedgerError(f"{what}: an activation-operand IGEMM outside the attention-backward chain has no statement")
        g1, tr, g2, sb, g4, tr2, g5 = [s for _, s in bops[i:i + 7]]
        B, heads, Lq = g1.B, g1.heads, g1.W
        Z = B * heads
        for g in (g1, g2, g4, g5):
            if g.ks != 1 or g.H != 1 or g.W != Lq or g.B != B or g.heads != heads or g.gn_scale or g.act or g.bias or g.temb or g.res or g.c1:
                raise LedgerError(f"{what}: unexpected GEMM form ks={g.ks} H={g.H} W={g.W} B={g.B} heads={g.heads} c1={g.c1} "
                                  f"gn={bool(g.gn_scale)} act={g.act} bias={bool(g.bias)} res={bool(g.res)}")
        ch = g1.c0

        def A(g, tag):
            return self.reg(g.a0, (B, heads, Lq, g.c0), (g.a0_bs, g.a0_hs, g.a0_ld, 1), f"{what}.{tag}.a")

        def Bm(g, tag):
            rows, cols = (g.N, g.c0) if g.b_mode == 1 else (g.c0, g.N)
            return self.reg(g.bmat, (B, heads, rows, cols), (g.b_bs, g.b_hs, g.ldb, 1), f"{what}.{tag}.b")

        def O(g, tag):
            return self.reg(g.out, (B, heads, Lq, g.N), (g.o_bs, g.o_hs, g.out_ld, 1), f"{what}.{tag}.out")
        sq = (B, heads, Lq, Lq), (heads * Lq * Lq, Lq * Lq, Lq, 1)
        Pm = self.reg(sb.p, *sq, what + ".p")
        dP = self.reg(sb.dp, *sq, what + ".dp")
        T1 = self.reg(tr.out, *sq, what + ".t1")
        ok = (g1.b_mode == 1 and g1.N == Lq and O(g1, "dP").key == dP.key and tr.inp == sb.p and tr.Z == Z and tr.L == Lq
              and g2.b_mode == 2 and A(g2, "dV").key == T1.key and sb.rows == Z * Lq and sb.L == Lq
              and g4.b_mode == 2 and A(g4, "dQ").key == dP.key and tr2.inp == sb.dp and tr2.out == tr.out and tr2.Z == Z and tr2.L == Lq
              and g5.b_mode == 2 and A(g5, "dK").key == T1.key and g2.N == g4.N == g5.N == ch and g4.alpha == g5.alpha and g1.alpha == 1.0
              and g2.alpha == 1.0)
        if not ok:
            raise LedgerError(f"{what}: the seven launches are not chained through P, dP and T1 as the statement assumes")
        datt, v, datt2, k, q = A(g1, "dP"), Bm(g1, "dP"), Bm(g2, "dV"), Bm(g4, "dQ"), Bm(g5, "dK")
        dV, dQ, dK = O(g2, "dV"), O(g4, "dQ"), O(g5, "dK")
        alpha = g4.alpha
        L = Launch(list(range(i, i + 7)), f"attention_bwd B={B} heads={heads} L={Lq} ch={ch}", "cfg=" + "/".join(str(g.cfg) for g in (g1, g2, g4, g5)) + " ksplit=" + "/".join(str(g.ksplit) for g in (g1, g2, g4, g5)))
        L.inputs += [datt, v, datt2, k, q, Pm]
        for name, r in (("dS", dP), ("dS^T", T1), ("dV", dV), ("dQ", dQ), ("dK", dK)):
            L.outs.append(Out(name, r, False, BAR_SOFTMAX if name == "dS" else BAR_CONV1))

        def compute(dev):
            p = Pm.read(dev)
            dS = softmax_backward(p, attn_gemm(datt.read(dev), v.read(dev), 1))           # against what the dP buffer ends as
            dS_dev = dP.read(dev)                                                       # dQ, dK: from the ACTUAL dS buffer
            return {"dS": dS, "dS^T": dS_dev.transpose(-1, -2), "dV": attn_gemm(p.transpose(-1, -2), datt2.read(dev), 2),
                    "dQ": attn_gemm(dS_dev, k.read(dev), 2, alpha), "dK": attn_gemm(T1.read(dev), q.read(dev), 2, alpha)}
        L.compute = compute
        return L

    # ------------------------------------------------------------------ static checks
    def regions(self):
        """Written regions in order of their first writer: key -> [(launch, out)] in list order."""
        groups = {}
        for L in self.launches:
            for o in L.outs:
                groups.setdefault(o.region.key, []).append((L, o))
        return groups

    def static_failures(self, first_writer=True):
        """Violations visible in the structs alone (no arithmetic): a first writer that accumulates / a later writer that does not,
        two different written regions that share elements, an output that overlaps an input outside the declared in-place forms, a
        parameter gradient the exempt weight-gradient launches write as well."""
        bad = []
        groups = self.regions()
        for key, ws in groups.items():
            for n, (L, o) in enumerate(ws):
                if o.kind == "param":
                    if not o.acc:
                        bad.append(f"{L.what} (bops{L.idx}): parameter gradient {o.region} is overwritten, not accumulated")
                elif first_writer and n == 0 and o.acc:
                    bad.append(f"{L.what} (bops{L.idx}): FIRST writer of {o.region} accumulates into memory nobody wrote this step")
                elif n > 0 and not o.acc:
                    bad.append(f"{L.what} (bops{L.idx}): writer {n + 1} of {o.region} overwrites what bops{ws[0][0].idx} wrote")
        firsts = [ws[0][1].region for ws in groups.values()]
        order = sorted(range(len(firsts)), key=lambda j: firsts[j].span())
        for a in range(len(order)):
            ra = firsts[order[a]]
            for b in range(a + 1, len(order)):
                rb = firsts[order[b]]
                if rb.span()[0] >= ra.span()[1]:
                    break
                if overlaps(ra, rb):
                    bad.append(f"written regions {ra} and {rb} share elements but are not the same region")
        for L in self.launches:
            for o in L.outs:
                for r in L.inputs:
                    if r.key == o.region.key and r.key in L.inplace:
                        continue
                    if overlaps(o.region, r):
                        bad.append(f"{L.what} (bops{L.idx}): output {o.region} overlaps its input {r}")
        # the reduction rows a data-gradient epilogue writes (gnb_partial) belong to ONE GroupNorm backward: same sources, affine
        # parameters and statistics on both sides, one row per 16 x 16 tile
        makers = {L.st.gnb_partial: L for L in self.launches if L.what.startswith("dgrad3") and L.st.gnb_partial}
        for L in self.launches:
            if L.what.startswith("gn_bwd") and L.st.partial_ready:
                g, M = L.st, makers.pop(L.st.partial, None)
                if M is None:
                    bad.append(f"{L.what} (bops{L.idx}): partial_ready, but no data-gradient launch writes its partial rows")
                    continue
                m = M.st
                same = ((m.gnb_x0, m.gnb_x1, m.gnb_gamma, m.gnb_beta, m.gnb_mean, m.gnb_rstd, m.gnb_c0, m.gnb_groups, m.out, m.N, m.B) ==
                        (g.x0, g.x1, g.gamma, g.beta, g.mean, g.rstd, g.c0, g.groups, g.da, g.c0 + g.c1, g.B))
                if not same or g.nslab != (m.H // 16) * (m.W // 16) or M.idx[0] > L.idx[0] or g.a_mode != 0 or g.act != 1:
                    bad.append(f"{M.what} (bops{M.idx}): its gnb_* fields are not those of the GroupNorm backward that consumes the rows "
                               f"({L.what}, bops{L.idx})")
        for M in makers.values():
            bad.append(f"{M.what} (bops{M.idx}): writes gnb_partial rows no GroupNorm backward consumes")
        pouts = [o.region for L in self.launches for o in L.outs if o.kind == "param"]
        for j in self.exempt:
            st = self.plan.bops[j][1]
            for f in ("dw", "dbias"):
                p = getattr(st, f, None)
                if p and any(r.span()[0] <= p < r.span()[1] for r in pouts):
                    bad.append(f"bops[{j}].{f} writes a parameter gradient an audited launch writes too")
        return bad

    # ------------------------------------------------------------------ arithmetic
    def audit(self, log=print):
        """Every region's ledger against the content of its buffer.  Returns (failures, figures): figures = [(launch, out name, writers,
        figure, bar, ok)]; one line per region goes to `log`."""
        groups = self.regions()
        pending, bad, figs = {}, [], []
        for L in self.launches:
            contrib = L.compute(self.dev)
            for o in L.outs:
                ws = groups[o.region.key]
                ref = contrib[o.name]
                if tuple(ref.shape) != o.region.shape:
                    raise LedgerError(f"{L.what}: statement of {o.name} has shape {tuple(ref.shape)}, the region {o.region.shape}")
                st = pending.setdefault(o.region.key, {"n": 0, "sum": None, "den": None, "budget": None, "tmax": 0.0, "tbud": 0.0})
                st["n"] += 1
                if o.kind == "param":
                    m = float(ref.abs().max())
                    st["tmax"], st["tbud"] = max(st["tmax"], m), st["tbud"] + o.bar * m
                    st["sum"] = ref if st["sum"] is None else st["sum"] + ref
                else:
                    r3 = o.z3(ref)
                    m = block_max(r3)
                    st["den"] = m if st["den"] is None else torch.maximum(st["den"], m)
                    st["budget"] = o.bar * m if st["budget"] is None else st["budget"] + o.bar * m
                    st["sum"] = r3 if st["sum"] is None else st["sum"] + r3
                if st["n"] < len(ws):
                    continue
                got = o.region.read(self.dev)
                if o.kind == "param":
                    fig, where, bar, ok = tensor_figure(got, st["sum"], st["tbud"] / st["tmax"] if st["tmax"] > 0 else o.bar)
                else:
                    fig, where, bar, ok = block_figure(o.z3(got), st["sum"], budget=st["budget"], den=st["den"])
                del pending[o.region.key]
                writers = [f"bops{w.idx}.{wo.name}" for w, wo in ws]
                log(f"  {L.what} [{L.cfg}] {o.name} {list(o.region.shape)} writers={len(ws)}{' ' + '+'.join(writers) if len(ws) > 1 else ''}: "
                    f"worst (image, channel)={where} figure {fig:.3e} bar {bar:.3g}{'' if ok else '   <-- FAIL'}")
                figs.append((L, o.name, len(ws), fig, bar, ok))
                if not ok:
                    bad.append((L.what, L.idx, o.name, fig, bar, where))
            del contrib
        if pending:
            raise LedgerError(f"regions with writers that never came: {list(pending)}")
        return bad, figs
