"""-m gpu: the seven small kernels every reverse-diffusion step launches -- anoddpm_posemb, anoddpm_linear_small, anoddpm_conv_stem,
anoddpm_conv_head, anoddpm_resample2x, anoddpm_softmax_rows, anoddpm_nhwc_to_nchw (csrc/unet_kernels.hip) -- through the C ABI by way
of tests/hipops.py on the cases of tests/infer_op_cases.py, each output against its fp64 statement.

Every element of every output is compared.  Every row (the batch row of the linear and of posemb, the (image, output channel) plane of
the stem and the head, the softmax row, the (image, channel) plane of out_act, the statistics row) is within its bar:
max |err| / max S <= max(FLOOR, 4 r32) <= the bar the same kernel has in tests/test_gpu_ops.py, S the sum of the absolute values of the
element's terms, r32 the worst row of the fp32 CPU restatement (computed at run time; tests/test_infer_op_reference.py holds
4 r32 <= CAP).  The statistics rows of the stem are held to the fp64 sums of their own contiguous pixel range of the buffer the launch
wrote.  Resample modes 1, 3, 4, mode 2's plain output, nhwc_to_nchw and the cleared range of posemb are bit for bit.  Every output
buffer, statistics included, is prefilled with NaN and ends in 64 NaN elements that must come back untouched; non-finite output fails.
Border pixels of the stem and the head are also reported on their own.  The variant selectors (anoddpm_internal_variant keys 4 and 9)
are set through a fixture that puts 0 back.  Every figure is printed before it is asserted; the module prints the worst figure per
class and regime at its end.

Measured on an MI355X: worst row figure per class of bar and regime over all shapes and outputs, in brackets its share of the case's
bar.
  class      bar's cap   iid              quiet_row        saturated        peaked
  linear     2e-5        7.21e-08 (0.13)  6.30e-08 (0.11)  8.44e-08 (0.15)  -
  posemb     2e-6 abs    5.14e-08 (0.36)  -                -                -
  stem       2e-5        2.04e-07 (0.26)  4.55e-07 (0.58)  -                -
  stats      1e-5        1.99e-07 (0.33)  1.87e-07 (0.31)  -                -            (the stem's sums and sums of squares)
  head       2e-5        6.79e-08 (0.11)  2.93e-07 (0.49)  1.10e-07 (0.18)  -
  act        2e-5        1.49e-07 (0.19)  1.60e-07 (0.20)  1.94e-07 (0.25)  -            (out_act of resample mode 2)
  softmax    2e-5        1.85e-07 (0.28)  1.78e-07 (0.27)  -                1.81e-07 (0.25)
One finding: the generic stem kernel (Cin > 2, W % 8 != 0 or an input that is not 16-byte aligned) summed its Cin * 9 products onto the
bias; at 2 x 6 x 8, Cin 16, Cout 12 under quiet_row the plane (image 0, channel 0) came back at 1.12e-06, 1.44 of its bar 7.8e-07 (two of
24 planes beyond it) -- 144 roundings at the ulp of a bias the products are small against.  It now adds the bias last: 8.4e-08 on that
case (iid: 3.1e-07 before, 1.1e-07 after).  No other row of any output is beyond its bar, no guard element was written, every refusal left its buffers alone, and the
bit-for-bit outputs (the map of 2 097 153 elements included) are the restatement's.  Wall time of the module on the device: 3.2 s for
the 328 items, the slowest 0.4 s (the first launch)."""
import pytest
import torch

import infer_op_cases as ic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
EINVAL = -1                 # ANODDPM_EINVAL of include/anoddpm_hip.h
LEDGER = {}
FAULT = []                  # the first launch that raised: nothing more is launched after it


def H():
    import hipops
    return hipops


@pytest.fixture(scope="module", autouse=True)
def ledger():
    yield
    print()
    for key in sorted(LEDGER):
        fig, ratio, where = LEDGER[key]
        print("worst", *key, f"{fig:.2e} ({ratio:.2f} of its bar) at {where}")


@pytest.fixture
def selector():
    """set(key, value) for the kernel-variant keys 4 (head kernel form) and 9 (stem trips); both are 0 again afterwards."""
    from anoddpm_amd._lib import lib

    def set_(key, value):
        assert key in (4, 9) and lib().anoddpm_internal_variant(key, value) == 0

    try:
        yield set_
    finally:
        lib().anoddpm_internal_variant(4, 0)
        lib().anoddpm_internal_variant(9, 0)


class Run:
    """The buffers, launches and comparisons of one case."""

    def __init__(self, item=None, tag=None):
        self.item, self.tag = item, tag or ic.case_id(item)
        self.p = ic.prepared(*item) if item else None
        self.fails, self.bufs = [], []

    def buf(self, what, numel, old=None, spare=0, dtype=torch.float32):
        """A flat device buffer of numel (+ spare) + GUARD elements: NaN, its first numel elements `old` if given."""
        t = torch.full((numel + spare + ic.GUARD,), NAN, device=DEV, dtype=dtype)
        if old is not None:
            t[:numel] = old.reshape(-1).to(DEV)
        self.bufs.append((what, t, numel))
        return t

    def call(self, fn, *args, **kw):
        assert not FAULT, f"not launched: an earlier launch raised ({FAULT[0]})"
        try:
            return fn(*args, **kw)
        except BaseException as err:
            FAULT.append(repr(err))
            raise

    def compare(self, name, got, out, mask=None):
        """got: shaped like out.ref ([rows, ...]), on either device."""
        got = got.detach().cpu()
        e = ic.row_error(got, out.ref, out.S)
        fig, row = ic.worst_row(e)
        bar, r32 = self.p["bar"][out.cls], self.p["r32"][out.cls]
        border = ""
        if mask is not None:
            eb = ic.border_error(got, out.ref, out.S, mask)
            border = f"; border pixels alone {eb.max().item():.3e} (row {eb.argmax().item()})"
        print(f"{self.tag} {name}: worst row {row} {fig:.3e}, r32 {r32:.3e}, bar {bar:.3e} ({fig / bar:.2f}); "
              f"global {ic.global_error(got, out.ref):.3e}{border}")
        key = (out.cls, self.item[2])
        LEDGER[key] = max(LEDGER.get(key, (0.0, -1.0, "")), (fig, fig / bar, f"{self.tag} {name}"), key=lambda v: v[1])
        if not (e <= bar).all():
            self.fails.append(f"{self.tag} {name}: row {row} {fig:.3e} > bar {bar:.3e} (r32 {r32:.3e}); "
                              f"{int((e > bar).sum())} of {e.numel()} rows beyond it{border}")

    def exact(self, name, got, out):
        got = got.detach().cpu().reshape(out.y.shape)
        bad = got.view(torch.int32) != out.y.contiguous().view(torch.int32)
        print(f"{self.tag} {name}: {int(bad.sum())} of {bad.numel()} elements differ from the restatement's bits")
        if bad.any():
            i = int(bad.reshape(-1).int().argmax())
            self.fails.append(f"{self.tag} {name}: {int(bad.sum())} of {bad.numel()} elements are not the restatement's bits; first at {i}: "
                              f"got {got.reshape(-1)[i].item()!r}, want {out.y.reshape(-1)[i].item()!r}")

    def untouched(self, what, t):
        if not torch.isnan(t).all():
            self.fails.append(f"{self.tag} {what}: a buffer of a refused or empty launch was written")

    def guards(self):
        for what, t, numel in self.bufs:
            if not torch.isnan(t[numel:]).all():
                self.fails.append(f"{self.tag} {what}: elements behind the buffer's end were written")
        self.bufs = []

    def done(self):
        assert not self.fails, "\n".join(self.fails)


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------------- linear, posemb
@pytest.mark.parametrize("item", ic.cases("linear"), ids=ic.case_id)
def test_linear_small(item):
    r = Run(item)
    o = r.p["o"]
    B, K, N = item[1][:3]
    out = r.buf("out", B * N)
    got = r.call(H().linear, dev(o["x"]), dev(o["w"]), dev(o["bias"]), o["act_in"], o["act_out"], out=out)
    r.compare("out", got, r.p["outs"]["out"])
    r.guards()
    r.done()


@pytest.mark.parametrize("item", ic.cases("posemb"), ids=ic.case_id)
def test_posemb(item):
    r = Run(item)
    o = r.p["o"]
    B, dim, scale, zd = item[1]
    out = r.buf("out", B * dim)
    zero = r.buf("zero", zd, dtype=torch.float64)
    got = r.call(H().posemb, dev(o["t"]), dev(o["freqs"]), dim, scale, zero=zero, zero_doubles=zd, out=out)
    r.compare("out", got, r.p["outs"]["out"])
    cleared = zero[:zd].view(torch.int64) == 0
    print(f"{r.tag} zero: {int(cleared.sum())} of {zd} doubles are +0")
    if not cleared.all():
        r.fails.append(f"{r.tag} zero: {int((~cleared).sum())} of {zd} doubles are not +0; first at {int((~cleared).int().argmax())}")
    r.guards()
    r.done()


# ---------------------------------------------------------------------------------------------------- stem and head
@pytest.mark.parametrize("item", ic.cases("stem"), ids=ic.case_id)
def test_conv_stem(item, selector):
    from anoddpm_amd._lib import lib
    r = Run(item)
    o, outs = r.p["o"], r.p["outs"]
    B, Hh, W, Cin, Cout, stats, off, key9 = item[1]
    rows = o["rows"]
    if stats < 0:
        assert lib().anoddpm_stem_stats_rows(Hh, W, Cin, Cout) == rows > 0
    x = dev(o["x"])
    if off:
        x = torch.cat([torch.full((off,), NAN, device=DEV), x.reshape(-1)])
        assert (x.data_ptr() + 4 * off) % 16
    out = r.buf("out", B * Hh * W * Cout)
    st = r.buf("stats", B * rows * Cout * 2)
    selector(9, key9)
    res = r.call(H().stem, x, dev(o["w"]), dev(o["bias"]), rows > 0, stats_rows=rows or None, stats=st, out=out, x_offset=off,
                 shape=(B, Cin, Hh, W))
    selector(9, 0)
    got = (res[0] if rows else res).permute(0, 3, 1, 2).contiguous()                  # NHWC -> [B, Cout, H, W]
    r.compare("out", got.flatten(0, 1), outs["out"], ic.border_mask(Hh, W))
    if rows:
        # every statistics row against the fp64 sums of its own pixel range of the buffer the launch wrote
        so = ic.stats_outputs(got.cpu(), rows)
        r.compare("stats sum", res[1][..., 0].reshape(B * rows, Cout), so["sum"])
        r.compare("stats sq", res[1][..., 1].reshape(B * rows, Cout), so["sq"])
    else:
        r.untouched("stats", st)
    r.guards()
    r.done()


@pytest.mark.parametrize("item", ic.cases("head"), ids=ic.case_id)
def test_conv_head(item, selector):
    r = Run(item)
    o = r.p["o"]
    B, Hh, W, C, Cout, key4 = item[1]
    out = r.buf("out", B * Cout * Hh * W)
    selector(4, key4)
    got = r.call(H().head, dev(o["x"]), dev(o["w"]), dev(o["bias"]), dev(o["scale"]), dev(o["shift"]), out=out)
    selector(4, 0)
    r.compare("out", got.flatten(0, 1), r.p["outs"]["out"], ic.border_mask(Hh, W))
    r.guards()
    r.done()


# ---------------------------------------------------------------------------------------------------- resample, softmax, layout
@pytest.mark.parametrize("item", ic.cases("resample"), ids=ic.case_id)
def test_resample(item):
    r = Run(item)
    o, outs = r.p["o"], r.p["outs"]
    mode = item[1][0]
    n = outs["out"].ref.numel()
    out = r.buf("out", n)
    if mode == 2:
        act = r.buf("out_act", n)
        got, ga = r.call(H().resample, dev(o["x"]), 2, gn=(dev(o["scale"]), dev(o["shift"])), out=out, act=act)
        r.compare("out_act", ga.permute(0, 3, 1, 2).flatten(0, 1), outs["act"])
    else:
        got = r.call(H().resample, dev(o["x"]), mode, out=out)
    r.exact("out", got, outs["out"])
    r.guards()
    r.done()


@pytest.mark.parametrize("item", ic.cases("softmax"), ids=ic.case_id)
def test_softmax_rows(item):
    r = Run(item)
    o, out = r.p["o"], r.p["outs"]["out"]
    rows, Lq = item[1]
    buf = r.buf("x", rows * Lq, o["x"], spare=ic.SOFTMAX_SPARE_ROWS * Lq)             # in place; three NaN rows behind `rows`
    got = r.call(H().softmax_rows, buf, rows, Lq)
    r.compare("in place", got, out)
    if not (got.cpu()[torch.isinf(o["x"])] == 0).all():
        r.fails.append(f"{r.tag}: a masked entry is not exactly 0")
    r.guards()
    r.call(H().softmax_rows, buf, 0, Lq)                                             # no rows: no launch
    r.done()


@pytest.mark.parametrize("item", ic.cases("layout"), ids=ic.case_id)
def test_nhwc_to_nchw(item):
    r = Run(item)
    o = r.p["o"]
    B, P, C, in_ld, first = item[1]
    out = r.buf("out", B * C * P)
    got = r.call(H().nhwc_to_nchw, dev(o["x"]), B, P, C, in_ld, first=first, out=out)
    r.exact("out", got, r.p["outs"]["out"])
    r.guards()
    r.done()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(selector):
    """Each is the bad-argument status with the kernel's name in anoddpm_last_error(), and nothing is launched: every output buffer
    keeps its NaN."""
    from anoddpm_amd._lib import lib
    h = H()
    r = Run(tag="refusals")
    out, out2 = r.buf("out", 1 << 16), r.buf("second output", 1 << 16)
    x = torch.zeros(1 << 16, device=DEV)
    t = torch.zeros(8, dtype=torch.int64, device=DEV)

    def stem(B, Hh, W, Cin, Cout, rows):
        return h.stem(x, x[:Cout * Cin * 9].view(Cout, Cin, 3, 3), x[:Cout], True, stats_rows=rows, stats=out2, out=out, shape=(B, Cin, Hh, W),
                      raw=True)

    def head(B, Hh, W, C, Cout):
        return h.head(x[:B * Hh * W * C].view(B, Hh, W, C), x[:Cout * C * 9].view(Cout, C, 3, 3), x[:Cout], x[:B * C].view(B, C),
                      x[:B * C].view(B, C), out=out, raw=True)

    def head_lds(*a):
        selector(4, 1)
        try:
            return head(*a)
        finally:
            selector(4, 0)

    cases = [
        ("linear K = 6", b"linear_small", lambda: h.linear(x[:24].view(4, 6), x[:12].view(2, 6), None, out=out, raw=True)),
        ("linear B = 0", b"linear_small", lambda: h.linear(x[:32].view(4, 8), x[:16].view(2, 8), None, out=out, B=0, raw=True)),
        ("linear B = 4097", b"linear_small", lambda: h.linear(x[:4097 * 8].view(4097, 8), x[:16].view(2, 8), None, out=out, raw=True)),
        ("posemb odd dim", b"posemb", lambda: h.posemb(t[:2], x[:4], 7, out=out, raw=True)),
        ("stem statistics with Cin = 3", b"conv_stem", lambda: stem(1, 8, 16, 3, 32, 1)),
        ("stem statistics with W = 12", b"conv_stem", lambda: stem(1, 8, 12, 1, 32, 1)),
        ("stem stats_rows 3 of 64 strips", b"conv_stem", lambda: stem(1, 16, 32, 1, 32, 3)),
        ("head H = 12", b"conv_head", lambda: head(1, 12, 8, 64, 1)),
        ("head Cout = 5", b"conv_head", lambda: head(1, 8, 8, 64, 5)),
        ("head LDS kernel at C = 128, Cout = 4", b"conv_head", lambda: head_lds(1, 8, 8, 128, 4)),
        ("resample mode 2 with odd H", b"resample2x", lambda: h.resample(x[:3 * 4 * 4].view(1, 3, 4, 4), 2, out=out, raw=True)),
        ("resample out_act in mode 1", b"resample2x", lambda: h.resample(x[:4 * 4 * 4].view(1, 4, 4, 4), 1, gn=(x[:4], x[:4]), out=out,
                                                                         act=out2, raw=True)),
        ("layout in_ld < C", b"nhwc_to_nchw", lambda: h.nhwc_to_nchw(x, 1, 8, 4, 3, out=out, raw=True)),
    ]
    for what, name, fn in cases:
        rc = r.call(fn)
        msg = lib().anoddpm_last_error() or b""
        print(f"{what}: status {rc}, {msg.decode(errors='replace')!r}")
        if rc != EINVAL or name not in msg:
            r.fails.append(f"{what}: status {rc} (want {EINVAL}), message {msg!r} (want {name!r} in it)")
    torch.cuda.synchronize()
    r.untouched("out", out)
    r.untouched("second output", out2)
    r.done()
