"""-m gpu: the small kernels a training step launches between the heavy ones -- csrc/train_kernels.hip (linear_small_backward and its
batched form, softmax_rows_backward, transpose_square, colsum_fold, conv_stem_backward, conv_head_backward), the backward modes of
resample2x and the dropout kernel of csrc/unet_kernels.hip -- straight through the C ABI on the cases of tests/train_op_cases.py, each
output against its fp64 statement.

Every element of every output is compared.  Every row (the batch row of dx / da / dimg, the output channel of dw / db / dbias, the
softmax row) is within its bar: max |err| / max S <= max(FLOOR, 4 r32) <= the bar of the same kernel in tests/test_gpu_train_ops.py, S
the sum of the absolute values of the element's terms plus |old value| where the launch adds, r32 the worst row of the fp32 CPU
restatement (computed at run time; tests/test_train_op_reference.py holds 4 r32 <= CAP).  A target the launch adds to is prefilled
with a seeded non-zero tensor, every other output and every workspace with NaN, and each buffer ends in 64 NaN elements that must
come back untouched; a NaN buffer the struct does not point to (db = NULL, dx = NULL) stays NaN.  Non-finite output fails.  Border
pixels of the stem's dx and the head's da are also reported on their own.  transpose_square and dropout mode 1 are bit for bit;
dropout's kept set is the numpy restatement of the documented hash.  Every figure is printed before it is asserted; the module prints
the worst figure per class at its end.

Measured on an MI355X: worst row figure per class of bar and regime over all shapes, outputs and launch forms, in brackets its
share of the case's bar.
  class      bar's cap   iid              quiet_row        saturated        peaked
  linear     1e-5        1.80e-07 (0.25)  1.87e-07 (0.25)  3.28e-07 (0.31)  -            (dw, db, dx; single and batched launch)
  softmax    1e-5        7.82e-08 (0.22)  6.88e-08 (0.19)  -                7.18e-08 (0.20)
  stem       2e-5        2.05e-07 (0.25)  2.63e-07 (0.32)  -                -            (dw, db, dx)
  head       2e-5        1.65e-07 (0.24)  1.84e-07 (0.27)  2.43e-07 (0.36)  -            (da, db)
  head_dw    5e-5        1.18e-07 (0.24)  9.40e-08 (0.20)  6.96e-08 (0.15)  -
  resample   1e-6        6.80e-08 (0.25)  5.59e-08 (0.21)  -                -
  colsum     1e-6        1.18e-07 (0.23)  1.32e-07 (0.25)  -                -            (dimg, dbias)
  dropout    2e-5        1.26e-07 (0.22)  -                1.02e-07 (0.18)  -            (mode 0)
No row of any output is beyond its bar, no guard element or unassigned buffer was written, transpose_square and dropout mode 1 are
bit for bit (the map of 8 388 620 elements included).  No kernel was changed.  Wall time of the module on the device: 3.8 s for the
488 items, the slowest 0.3 s (the first launch)."""
import ctypes

import numpy as np
import pytest
import torch

import train_op_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
LEDGER = {}
FAULT = []                  # the first launch that raised: nothing more is launched after it


def L():
    from anoddpm_amd import _lib
    return _lib, _lib.lib()


@pytest.fixture(scope="module", autouse=True)
def ledger():
    yield
    print()
    for key in sorted(LEDGER):
        fig, ratio, where = LEDGER[key]
        print("worst", *key, f"{fig:.2e} ({ratio:.2f} of its bar) at {where}")


class Run:
    """The buffers, launches and comparisons of one case."""

    def __init__(self, item=None, tag=None):
        self.item, self.tag = item, tag or tc.case_id(item)
        self.p = tc.prepared(*item) if item else None
        self.fails, self.bufs, self.keep = [], [], []

    def dev(self, t):
        t = t.to(DEV).contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def buf(self, what, numel, old=None, spare=0):
        """A flat device buffer of numel (+ spare) + GUARD floats: NaN, its first numel elements `old` if given."""
        t = torch.full((numel + spare + tc.GUARD,), NAN, device=DEV)
        if old is not None:
            t[:numel] = old.reshape(-1).to(DEV)
        self.bufs.append((what, t, numel))
        return t

    def launch(self, fn, st, want=0):
        assert not FAULT, f"not launched: an earlier launch raised ({FAULT[0]})"
        _lib, lib = L()
        try:
            rc = getattr(lib, fn)(ctypes.byref(st), _lib.current_stream())
            if want == 0:
                _lib.check(rc, fn)
            torch.cuda.synchronize()
        except BaseException as err:
            FAULT.append(repr(err))
            raise
        return rc

    def compare(self, form, name, t, out, acc, mask=None):
        ref, S, _ = tc.target(out, acc)
        got = t[:ref.numel()].cpu()
        e = tc.row_error(got, ref, S)
        fig, row = tc.worst_row(e)
        bar, r32 = self.p["bar"][out.cls], self.p["r32"][out.cls]
        border = ""
        if mask is not None:
            eb = tc.border_error(got, ref, S, mask)
            border = f"; border pixels alone {eb.max().item():.3e} (row {eb.argmax().item()})"
        print(f"{self.tag} [{form}] {name}: worst row {row} {fig:.3e}, r32 {r32:.3e}, bar {bar:.3e} ({fig / bar:.2f}); "
              f"global {tc.global_error(got, ref):.3e}{border}")
        key = (out.cls, self.item[2])
        LEDGER[key] = max(LEDGER.get(key, (0.0, -1.0, "")), (fig, fig / bar, f"{self.tag} [{form}] {name}"), key=lambda v: v[1])
        if not (e <= bar).all():
            self.fails.append(f"{self.tag} [{form}] {name}: row {row} {fig:.3e} > bar {bar:.3e} (r32 {r32:.3e}); "
                              f"{int((e > bar).sum())} of {e.numel()} rows beyond it{border}")
        return got

    def untouched(self, form, what, t):
        if not torch.isnan(t).all():
            self.fails.append(f"{self.tag} [{form}] {what}: a buffer the launch was not given was written")

    def guards(self, form):
        for what, t, numel in self.bufs:
            if not torch.isnan(t[numel:]).all():
                self.fails.append(f"{self.tag} [{form}] {what}: elements behind the buffer's end were written")
        self.bufs = []

    def done(self):
        assert not self.fails, "\n".join(self.fails)


def _struct_bytes(arr):
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


# ---------------------------------------------------------------------------------------------------- linear
@pytest.mark.parametrize("item", tc.cases("linear"), ids=tc.case_id)
def test_linear_small_backward(item):
    _lib, _ = L()
    r = Run(item)
    o, outs = r.p["o"], r.p["outs"]
    (B, K, N, act_in), job = item[1], r.p["o"]["jobs"][0]
    for acc_w, acc_x, with_db, with_dx in tc.LINEAR_FORMS:
        form = f"acc_w {acc_w} acc_x {acc_x}" + ("" if with_db else " db NULL") + ("" if with_dx else " dx NULL")
        dw = r.buf("dw", N * K, job["old_dw"] if acc_w else None)
        db = r.buf("db", N, job["old_db"] if acc_w and with_db else None)
        dx = r.buf("dx", B * K, o["old_dx"] if acc_x and with_dx else None)
        st = _lib.LinearBwdArgs()
        st.x, st.w, st.dy, st.dw = r.dev(o["x"]), r.dev(job["w"]), r.dev(job["dy"]), dw.data_ptr()
        st.db, st.dx = (db.data_ptr() if with_db else None), (dx.data_ptr() if with_dx else None)
        st.B, st.K, st.N, st.act_in, st.acc_w, st.acc_x = B, K, N, act_in, acc_w, acc_x
        r.launch("anoddpm_linear_small_backward", st)
        r.compare(form, "dw", dw, outs["dw0"], acc_w)
        r.compare(form, "db", db, outs["db0"], acc_w) if with_db else r.untouched(form, "db", db)
        r.compare(form, "dx", dx, outs["dx"], acc_x) if with_dx else r.untouched(form, "dx", dx)
        r.guards(form)
    r.done()


@pytest.mark.parametrize("item", tc.cases("linear_batch"), ids=tc.case_id)
def test_linear_small_backward_batch(item):
    _lib, _ = L()
    r = Run(item)
    o, outs = r.p["o"], r.p["outs"]
    (njobs, B, K), jobs = item[1], r.p["o"]["jobs"]
    Ns = tc.BATCH_N[:njobs]
    no_db = min(1, njobs - 1)
    for acc_w, acc_x, drop_db, with_dx in tc.BATCH_FORMS:
        form = f"acc_w {acc_w} acc_x {acc_x}" + (f" db NULL in job {no_db}" if drop_db else "") + ("" if with_dx else " dx NULL ws NULL")
        arr = (_lib.LinearBwdArgs * njobs)()
        dws, dbs = [], []
        for j, job in enumerate(jobs):
            has_db = not (drop_db and j == no_db)
            dws.append(r.buf(f"dw{j}", Ns[j] * K, job["old_dw"] if acc_w else None))
            dbs.append(r.buf(f"db{j}", Ns[j], job["old_db"] if acc_w and has_db else None))
            arr[j].w, arr[j].dy, arr[j].dw, arr[j].N = r.dev(job["w"]), r.dev(job["dy"]), dws[j].data_ptr(), Ns[j]
            arr[j].db = dbs[j].data_ptr() if has_db else None
        raw = _struct_bytes(arr)
        dx = r.buf("dx", B * K, o["old_dx"] if acc_x and with_dx else None)
        ws = r.buf("ws", njobs * B * K)
        st = _lib.LinearBwdBatchArgs()
        st.jobs, st.x = raw.data_ptr(), r.dev(o["x"])
        st.dx, st.ws = (dx.data_ptr(), ws.data_ptr()) if with_dx else (None, None)
        st.njobs, st.max_n, st.B, st.K, st.act_in, st.acc_w, st.acc_x = njobs, max(Ns), B, K, 1, acc_w, acc_x
        r.launch("anoddpm_linear_small_backward_batch", st)
        for j in range(njobs):
            r.compare(form, f"dw{j}", dws[j], outs[f"dw{j}"], acc_w)
            if drop_db and j == no_db:
                r.untouched(form, f"db{j}", dbs[j])
            else:
                r.compare(form, f"db{j}", dbs[j], outs[f"db{j}"], acc_w)
        if with_dx:
            r.compare(form, "dx", dx, outs["dx"], acc_x)
            if not torch.isfinite(ws[:njobs * B * K]).all():
                r.fails.append(f"{r.tag} [{form}] ws: a partial sum was left unwritten")
        else:
            r.untouched(form, "dx", dx)
            r.untouched(form, "ws", ws)
        r.guards(form)
    r.done()


def test_linear_small_backward_batch_needs_the_workspace_for_dx():
    """dx != NULL with ws == NULL is the bad-argument status, and nothing is launched: every buffer keeps its NaN."""
    _lib, _ = L()
    item = ("linear_batch", tc.BATCH[0], "iid")
    r = Run(item)
    o, job = r.p["o"], r.p["o"]["jobs"][0]
    njobs, B, K = item[1]
    N = tc.BATCH_N[0]
    dw, db, dx = r.buf("dw", N * K), r.buf("db", N), r.buf("dx", B * K)
    arr = (_lib.LinearBwdArgs * 1)()
    arr[0].w, arr[0].dy, arr[0].dw, arr[0].db, arr[0].N = r.dev(job["w"]), r.dev(job["dy"]), dw.data_ptr(), db.data_ptr(), N
    raw = _struct_bytes(arr)
    st = _lib.LinearBwdBatchArgs()
    st.jobs, st.x, st.dx, st.ws = raw.data_ptr(), r.dev(o["x"]), dx.data_ptr(), None
    st.njobs, st.max_n, st.B, st.K, st.act_in, st.acc_w, st.acc_x = 1, N, B, K, 1, 0, 0
    assert r.launch("anoddpm_linear_small_backward_batch", st, want=_lib_einval()) == _lib_einval()
    for what, t in (("dw", dw), ("db", db), ("dx", dx)):
        r.untouched("ws NULL", what, t)
    r.done()


def _lib_einval():
    return -1                                                # ANODDPM_EINVAL of include/anoddpm_hip.h


# ---------------------------------------------------------------------------------------------------- attention pieces
@pytest.mark.parametrize("item", tc.cases("softmax"), ids=tc.case_id)
def test_softmax_rows_backward(item):
    _lib, _ = L()
    r = Run(item)
    rows, Lq = item[1]
    o, out = r.p["o"], r.p["outs"]["dp"]
    dp = r.buf("dp", rows * Lq, o["dp"], spare=tc.SOFTMAX_SPARE_ROWS * Lq)          # in place; three NaN rows behind `rows`
    st = _lib.SoftmaxBwdArgs()
    st.p, st.dp, st.rows, st.L = r.dev(torch.cat([o["p"], torch.full((tc.SOFTMAX_SPARE_ROWS, Lq), NAN)])), dp.data_ptr(), rows, Lq
    r.launch("anoddpm_softmax_rows_backward", st)
    got = r.compare("in place", "dp", dp, out, False).view(rows, Lq)
    if not (got[o["p"] == 0] == 0).all():
        r.fails.append(f"{r.tag}: dp is not exactly 0 where p is 0")
    r.guards("in place")
    st.rows = 0
    assert r.launch("anoddpm_softmax_rows_backward", st) == 0
    r.done()


@pytest.mark.parametrize("Z,Lq", tc.TRANSPOSE)
def test_transpose_square(Z, Lq):
    _lib, _ = L()
    r = Run(tag=f"transpose-{Z}x{Lq}")
    src = torch.randn(Z, Lq, Lq, generator=torch.Generator().manual_seed(40 + Z * 1000 + Lq))
    out = r.buf("out", Z * Lq * Lq)
    st = _lib.TransposeArgs()
    st.inp, st.out, st.Z, st.L = r.dev(src), out.data_ptr(), Z, Lq
    r.launch("anoddpm_transpose_square", st)
    assert torch.equal(out[:Z * Lq * Lq].cpu().view(Z, Lq, Lq).view(torch.int32), src.transpose(1, 2).contiguous().view(torch.int32))
    r.guards("")
    r.done()


# ---------------------------------------------------------------------------------------------------- column-sum fold
@pytest.mark.parametrize("item", tc.cases("colsum"), ids=tc.case_id)
def test_colsum_fold(item):
    _lib, _ = L()
    r = Run(item)
    B, ipb, N = item[1]
    o, outs = r.p["o"], r.p["outs"]
    for with_bias in (True, False):
        form = "dbias prefilled" if with_bias else "dbias NULL"
        dimg = r.buf("dimg", B * N)
        dbias = r.buf("dbias", N, o["old_dbias"] if with_bias else None)
        st = _lib.ColsumFoldArgs()
        st.colsum, st.dimg, st.dbias = r.dev(o["colsum"]), dimg.data_ptr(), (dbias.data_ptr() if with_bias else None)
        st.B, st.ipb, st.N = B, ipb, N
        r.launch("anoddpm_colsum_fold", st)
        r.compare(form, "dimg", dimg, outs["dimg"], False)
        r.compare(form, "dbias", dbias, outs["dbias"], True) if with_bias else r.untouched(form, "dbias", dbias)
        r.guards(form)
    r.done()


# ---------------------------------------------------------------------------------------------------- stem and head
@pytest.mark.parametrize("item", tc.cases("stem"), ids=tc.case_id)
def test_conv_stem_backward(item):
    _lib, _ = L()
    r = Run(item)
    B, H, W, Cin, Cout = item[1]
    o, outs = r.p["o"], r.p["outs"]
    nblk = B * -(-(H * W) // 1024)
    for with_dx in (True, False):
        form = "dx given" if with_dx else "dx NULL"
        dw, db = r.buf("dw", Cout * Cin * 9, o["old_dw"]), r.buf("db", Cout, o["old_db"])
        dx = r.buf("dx", B * Cin * H * W)
        ws = r.buf("ws", nblk * (Cin * 9 + 1) * Cout)
        st = _lib.StemBwdArgs()
        st.x, st.w, st.dy, st.dw, st.db = r.dev(o["x"]), r.dev(o["w"]), r.dev(o["dy"]), dw.data_ptr(), db.data_ptr()
        st.dx, st.ws, st.ws_floats = (dx.data_ptr() if with_dx else None), ws.data_ptr(), nblk * (Cin * 9 + 1) * Cout
        st.B, st.H, st.W, st.Cin, st.Cout = B, H, W, Cin, Cout
        r.launch("anoddpm_conv_stem_backward", st)
        r.compare(form, "dw", dw, outs["dw"], True)
        r.compare(form, "db", db, outs["db"], True)
        r.compare(form, "dx", dx, outs["dx"], False, tc.pixel_mask("stem", item[1])["dx"]) if with_dx else r.untouched(form, "dx", dx)
        r.guards(form)
    r.done()


@pytest.mark.parametrize("item", tc.cases("head"), ids=tc.case_id)
def test_conv_head_backward(item):
    _lib, _ = L()
    r = Run(item)
    B, H, W, C, Cout = item[1]
    o, outs = r.p["o"], r.p["outs"]
    nblk = B * -(-(H * W) // 512)
    da, dw, db = r.buf("da", B * H * W * C), r.buf("dw", Cout * C * 9, o["old_dw"]), r.buf("db", Cout, o["old_db"])
    ws = r.buf("ws", nblk * 10 * Cout * C)
    st = _lib.HeadBwdArgs()
    st.x, st.gn_scale, st.gn_shift, st.w, st.dy = r.dev(o["x"]), r.dev(o["scale"]), r.dev(o["shift"]), r.dev(o["w"]), r.dev(o["dy"])
    st.da, st.dw, st.db, st.ws, st.ws_floats = da.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nblk * 10 * Cout * C
    st.B, st.H, st.W, st.C, st.Cout = B, H, W, C, Cout
    r.launch("anoddpm_conv_head_backward", st)
    r.compare("", "da", da, outs["da"], False, tc.pixel_mask("head", item[1])["da"])
    r.compare("", "dw", dw, outs["dw"], True)
    r.compare("", "db", db, outs["db"], True)
    r.guards("")
    r.done()


# ---------------------------------------------------------------------------------------------------- resample
@pytest.mark.parametrize("item", tc.cases("resample"), ids=tc.case_id)
def test_resample_backward_modes(item):
    _lib, _ = L()
    r = Run(item)
    mode, B, h, w, C = item[1]
    o, out = r.p["o"], r.p["outs"]["out"]
    for acc in (0, 1):
        form = f"accumulate {acc}"
        dst = r.buf("out", out.ref0.numel(), o["old"] if acc else None)
        st = _lib.ResampleArgs()
        st.inp, st.out, st.B, st.C, st.mode, st.scale, st.accumulate = r.dev(o["g"]), dst.data_ptr(), B, C, mode, o["scale"], acc
        st.H, st.W = o["g"].shape[1], o["g"].shape[2]
        r.launch("anoddpm_resample2x", st)
        r.compare(form, "out", dst, out, bool(acc))
        r.guards(form)
    r.done()


# ---------------------------------------------------------------------------------------------------- dropout
def _dropout(r, x_ptr, out_ptr, B, n, C, mode, p, seed, scale=None, shift=None):
    _lib, _ = L()
    st = _lib.DropoutArgs()
    st.x, st.out, st.gn_scale, st.gn_shift = x_ptr, out_ptr, scale, shift
    st.n, st.seed, st.B, st.C, st.mode, st.p = n, seed, B, C, mode, p
    return r.launch("anoddpm_dropout", st)


def _bits_differ(r, what, t, want):
    got = t[:want.size].cpu().numpy().view(np.uint32)
    bad = got != want.reshape(-1).view(np.uint32)
    if bad.any():
        i = int(np.argmax(bad))
        r.fails.append(f"{r.tag} {what}: {int(bad.sum())} of {bad.size} elements are not the restatement's bits; first at {i}: "
                       f"got {got[i]:#010x}, want {want.reshape(-1).view(np.uint32)[i]:#010x}")


@pytest.mark.parametrize("B,n,C", tc.DROPOUT_SHAPES + (tc.DROPOUT_BIG,), ids=lambda v: str(v))
def test_dropout_mode1_bit_for_bit(B, n, C):
    """Mask and kept values are the restatement's, out of place and in place (the backward form of the plan); p = 0 returns x."""
    r = Run(tag=f"dropout1-{B}x{n}x{C}")
    big = (B, n, C) == tc.DROPOUT_BIG
    for p in ((0.3,) if big else tc.DROPOUT_P):
        for seed in ((2 ** 63 + 5,) if big else tc.DROPOUT_SEEDS):
            x = tc.dropout_input(B, n, seed)
            keep = tc.dropout_keep(seed, B, n, p)
            want = tc.dropout_values(x, keep, p)
            if p == 0:
                assert np.array_equal(want.view(np.uint32), x.view(np.uint32))
            xd = torch.from_numpy(x).to(DEV)
            out = r.buf("out", B * n)
            _dropout(r, xd.data_ptr(), out.data_ptr(), B, n, C, 1, p, seed)
            _bits_differ(r, f"p {p} seed {seed}", out, want)
            inplace = r.buf("in place", B * n, torch.from_numpy(x))
            _dropout(r, inplace.data_ptr(), inplace.data_ptr(), B, n, C, 1, p, seed)
            _bits_differ(r, f"p {p} seed {seed} in place", inplace, want)
            print(f"{r.tag} p {p} seed {seed}: kept {keep.mean():.4f}")
            r.guards(f"p {p} seed {seed}")
    r.done()


def test_dropout_empty_launches():
    r = Run(tag="dropout-empty")
    x, out = r.buf("x", 16), r.buf("out", 16)
    assert _dropout(r, x.data_ptr(), out.data_ptr(), 0, 16, 4, 1, 0.5, 1) == 0
    assert _dropout(r, x.data_ptr(), out.data_ptr(), 2, 0, 4, 1, 0.5, 1) == 0
    r.untouched("B = 0, n = 0", "out", out)
    r.done()


@pytest.mark.parametrize("item", tc.cases("dropout0"), ids=tc.case_id)
def test_dropout_mode0(item):
    """The kept set is the restated mask (a dropped element is +0 bit for bit, a kept one is non-zero wherever its value is); the
    values meet silu(x * scale + shift) / (1 - p) under the row figure."""
    r = Run(item)
    B, n, C, p, seed = item[1]
    o, outs = r.p["o"], r.p["outs"]["out"]
    out = r.buf("out", B * n)
    _dropout(r, r.dev(o["x"]), out.data_ptr(), B, n, C, 0, p, seed, r.dev(o["scale"]), r.dev(o["shift"]))
    got = r.compare("", "out", out, outs, False).view(B, n)
    keep = o["keep"]
    if (got[~keep].view(torch.int32) != 0).any():
        r.fails.append(f"{r.tag}: {int((got[~keep].view(torch.int32) != 0).sum())} dropped elements are not +0")
    missing = keep & (got == 0) & (outs.ref0.abs() > 1e-30)
    if missing.any():
        r.fails.append(f"{r.tag}: {int(missing.sum())} kept elements came back 0")
    r.guards("")
    r.done()
