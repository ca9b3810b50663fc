"""-m gpu: the OpenSimplex entry points on every launch path, straight through the C ABI (anoddpm_simplex3_octaves_f64 / _f32 with
a hand-built anoddpm_simplex_args) and through the wrapper where the wrapper is what is tested, against the C oracle.

Bar: none.  f64 outputs equal the oracle as uint64 patterns, f32 outputs equal oracle.astype(float32) as uint32 patterns.

Every launch of a case of tests/simplex_cases.py is audited: the whole output allocation -- a guard of more than H * W elements in
front and behind, and the gaps between slices -- is filled with one NaN bit pattern before the launch; afterwards every element of
every slice is the oracle's and every other element still holds that pattern.  The `tables` and `zvals` allocations end with the
last element the documented contract reads.

What each test reaches in csrc/simplex.hip is said in its docstring; tests/test_simplex_reference.py shows on the CPU that the
cases do reach it (which lanes are SAFE, which conversion the others take, rows_per_block, the table set of each slice).
"""
import ctypes

import numpy as np
import pytest
import torch

import simplex_cases as sc
from anoddpm_amd._lib import SimplexArgs, current_stream, lib
from anoddpm_amd.simplex import perm_tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
PATTERN = {np.float64: 0x7FF80BADC0DE0001, np.float32: 0x7FC0BEEF}       # quiet NaNs with a payload no kernel produces
ITYPE = {np.float64: (torch.int64, np.uint64), np.float32: (torch.int32, np.uint32)}
_TABLES = {}


def bits(a, ftype=np.float64):
    return np.ascontiguousarray(a, dtype=ftype).view(ITYPE[ftype][1])


def device_tables(seeds):
    """int16[len(seeds) * 512] on the device: the sets of `seeds` back to back and nothing behind them."""
    if seeds not in _TABLES:
        _TABLES[seeds] = torch.from_numpy(np.concatenate([perm_tables(s) for s in seeds])).to(DEV)
    return _TABLES[seeds]


class Launch:
    """The device buffers of a case and the argument struct over them."""

    def __init__(self, case, ftype):
        self.case, self.ftype = case, ftype
        H, W, n = case["H"], case["W"], case["nslices"]
        self.hw, self.stride = H * W, H * W + case["out_pad"]
        self.guard = H * W + 7
        self.span = (n - 1) * self.stride + H * W                 # the last slice needs no gap behind it
        self.buf = torch.full((self.guard + self.span + self.guard,), PATTERN[ftype], dtype=ITYPE[ftype][0], device=DEV)
        self.tables = device_tables(case["seeds"])
        self.zvals = None if case["zvals"] is None else torch.from_numpy(case["zvals"].copy()).to(DEV)
        self.sel = None if case["table_sel"] is None else torch.tensor([case["table_sel"]], dtype=torch.int32, device=DEV)
        assert self.tables.numel() == 512 * (int(sc.table_index(case).max()) + 1)
        assert self.zvals is None or self.zvals.numel() == n

    def args(self):
        c, a = self.case, SimplexArgs()
        a.out = self.buf.data_ptr() + self.guard * self.buf.element_size()
        a.zvals = None if self.zvals is None else self.zvals.data_ptr()
        a.tables = self.tables.data_ptr() + 1024 * c["tab_offset"]
        a.table_sel = None if self.sel is None else self.sel.data_ptr()
        a.z0, a.out_slice_stride = c["z0"], self.stride
        a.nslices, a.H, a.W = c["nslices"], c["H"], c["W"]
        a.table_slice_stride, a.table_sel_scale = c["table_slice_stride"], c["table_sel_scale"]
        a.octaves, a.persistence, a.frequency = c["octaves"], c["persistence"], c["frequency"]
        return a

    def entry(self):
        return lib().anoddpm_simplex3_octaves_f64 if self.ftype is np.float64 else lib().anoddpm_simplex3_octaves_f32

    def run(self, a=None):
        a = a or self.args()
        rc = self.entry()(ctypes.byref(a), current_stream())
        torch.cuda.synchronize()
        return rc

    def expected(self):
        itype = ITYPE[self.ftype][1]
        exp = np.full(self.buf.numel(), PATTERN[self.ftype], dtype=itype)
        ref = bits(sc.oracle_field(self.case).astype(self.ftype), self.ftype).reshape(self.case["nslices"], self.hw)
        for s in range(self.case["nslices"]):
            o = self.guard + s * self.stride
            exp[o:o + self.hw] = ref[s]
        return exp

    def got(self):
        return self.buf.cpu().numpy().view(ITYPE[self.ftype][1])

    def failures(self):
        got, exp = self.got(), self.expected()
        bad = np.nonzero(got != exp)[0]
        lines = []
        for i in bad[:6]:
            rel = int(i) - self.guard
            if rel < 0 or rel >= self.span:
                where = f"guard element {rel} (relative to out)"
            else:
                s, e = divmod(rel, self.stride)
                where = f"gap behind slice {s}, element {e}" if e >= self.hw else \
                    f"slice {s} (z {sc.zvalues(self.case)[s]}, table set {sc.table_index(self.case)[s]}) y {e // self.case['W']} x {e % self.case['W']}"
            lines.append(f"{self.case['name']} {self.ftype.__name__}: {where}: got {int(got[i]):#x} want {int(exp[i]):#x}")
        if bad.size:
            lines.insert(0, f"{self.case['name']} {self.ftype.__name__}: {bad.size} of {got.size} elements differ")
        return lines


# ---------------------------------------------------------------------------- every case, both output types, audited
@pytest.mark.parametrize("ftype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sc.case_names())
def test_case_is_bit_exact_and_writes_nothing_else(name, ftype):
    """tiny-f / deep-octaves / huge-z / freq-2^-20: noise3<.., false> from the octave kernel, with (int) and (long long) lattice
    bases, SAFE and non-SAFE lanes in one wave, the edge of the `safe` bound; neg-z0, stride-pad5-z0, rows-*, max-slices: z0 + s
    with a NULL zvals (negative, crossing 0); freq-*: both sides of the power-of-two classification and of its exponent limit;
    geom-*: ragged tiles; rows-*: rows_per_block 1 / 2 / 2 / 4 at and one tile below both thresholds, every slice compared;
    tables-*: table_sel, table_sel_scale, table_slice_stride and an advanced `tables`; stride-pad5*: out_slice_stride > H * W;
    max-slices: the 65535 slices of the largest launch that is accepted."""
    run = Launch(sc.get(name), ftype)
    assert run.run() == 0, lib().anoddpm_last_error()
    bad = run.failures()
    assert not bad, "\n".join(bad)


def test_fp32_fill_into_one_channel_with_selected_tables():
    """fill_fixed_T_octaves_ as a multi-channel reverse chain calls it (diffusion.py: tables=self.tables[c:], table_sel=step_idx,
    table_sel_scale=in_channels): channel c of step 1 of a three-channel chain reads set 1 * 3 + c; the other channels' planes
    keep the pattern they held.  Then channel 1 alone with the instance's own tables."""
    from simplex import Simplex_CLASS
    from oracle.simplex_oracle import OracleSimplex
    B, C, H, W = 3, 3, 6, 65
    t = np.array([0, 437, 999])
    td = torch.from_numpy(t).to(DEV)
    tabs = device_tables(sc.SEEDS6)
    step = torch.tensor([1], dtype=torch.int32, device=DEV)
    s = Simplex_CLASS()
    s.newSeed(77)
    raw = torch.full((B, C, H, W), PATTERN[np.float32], dtype=torch.int32, device=DEV)
    out = raw.view(torch.float32)
    for c in range(C):
        before = raw.cpu().numpy().copy()
        s.fill_fixed_T_octaves_(out, td, 3, 0.8, 16, channel=c, tables=tabs[512 * c:], table_sel=step, table_sel_scale=C)
        torch.cuda.synchronize()
        after = raw.cpu().numpy()
        ref = OracleSimplex(sc.SEEDS6[3 + c]).rand_3d_fixed_T_octaves((H, W), t, 3, 0.8, 16)
        assert (after[:, c].view(np.uint32) == bits(ref.astype(np.float32), np.float32)).all(), c
        others = [k for k in range(C) if k != c]
        assert (after[:, others] == before[:, others]).all(), c
    raw.fill_(PATTERN[np.float32])
    s.fill_fixed_T_octaves_(out, td, 2, 0.5, 24, channel=1)
    torch.cuda.synchronize()
    after = raw.cpu().numpy()
    ref = OracleSimplex(77).rand_3d_fixed_T_octaves((H, W), t, 2, 0.5, 24)
    assert (after[:, 1].view(np.uint32) == bits(ref.astype(np.float32), np.float32)).all()
    assert (after[:, [0, 2]] == PATTERN[np.float32]).all()


# ---------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("ftype", [np.float64, np.float32], ids=["f64", "f32"])
def test_refusals_say_why_and_launch_nothing(ftype):
    case = sc.get("stride-pad5")

    def refused(message, **fields):
        run = Launch(case, ftype)
        a = run.args()
        for k, v in fields.items():
            setattr(a, k, v)
        assert run.run(a) == EINVAL, fields
        assert message in lib().anoddpm_last_error(), (fields, lib().anoddpm_last_error())
        assert (run.got() == PATTERN[ftype]).all(), fields

    refused(b"nslices > 65535", nslices=65536)
    refused(b"slice stride < H*W", out_slice_stride=case["H"] * case["W"] - 1)
    refused(b"slice stride < H*W", out_slice_stride=0)
    for field in ("nslices", "H", "W", "octaves"):
        refused(b"negative size", **{field: -1})
    refused(b"null pointer", out=None)
    refused(b"null pointer", tables=None)
    assert lib().anoddpm_simplex3_octaves_f64(None, current_stream()) == EINVAL
    # empty launches are accepted and write nothing
    for field in ("nslices", "H", "W"):
        run = Launch(case, ftype)
        a = run.args()
        setattr(a, field, 0)
        assert run.run(a) == 0
        assert (run.got() == PATTERN[ftype]).all()


# ---------------------------------------------------------------------------- the wrapper's 32768-slice chunks
def test_volume_deeper_than_one_launch():
    """rand_3d_octaves over 40000 slices: two launches, the second with z0 = 32768 and `out` moved on; every slice compared."""
    from simplex import Simplex_CLASS
    from oracle.simplex_oracle import OracleSimplex
    s = Simplex_CLASS()
    s.newSeed(12345)
    got = s.rand_3d_octaves((40000, 2, 3), 2, 0.5, 8)
    ref = OracleSimplex(12345).rand_3d_octaves((40000, 2, 3), 2, 0.5, 8)
    assert got.shape == ref.shape == (40000, 2, 3)
    bad = np.nonzero((bits(got) != bits(ref)).any(axis=(1, 2)))[0]
    assert bad.size == 0, (bad.size, bad[:5])
    assert bits(ref[32767]).tolist() != bits(ref[32768]).tolist() != bits(ref[0]).tolist()


def test_fixed_T_batch_longer_than_one_launch():
    """rand_3d_fixed_T_octaves with 40000 random timesteps: the second launch reads zvals from index 32768 on."""
    from simplex import Simplex_CLASS
    from oracle.simplex_oracle import OracleSimplex
    T = np.random.RandomState(5).randint(0, 1000, size=40000)
    assert (T[:7232] != T[32768:]).mean() > 0.99                 # a second launch that reads zvals from the start again shows
    s = Simplex_CLASS()
    s.newSeed(-987654321)
    got = s.rand_3d_fixed_T_octaves((2, 3), T, 3, 0.7, 24)
    ref = OracleSimplex(-987654321).rand_3d_fixed_T_octaves((2, 3), T, 3, 0.7, 24)
    bad = np.nonzero((bits(got) != bits(ref)).any(axis=(1, 2)))[0]
    assert bad.size == 0, (bad.size, bad[:5], T[bad[:5]])


# ---------------------------------------------------------------------------- the grid kernels
def test_noise3array_axis_order():
    """out[z][y][x] = noise3(X[x], Y[y], Z[z]) (the reference's _noise3a) with three different lengths and unsorted, partly negative
    vectors: any permutation of the axes in simplex3_grid_kernel's index decomposition gives another array."""
    from simplex import Simplex_CLASS
    from oracle.simplex_oracle import OracleSimplex
    x = np.array([3.25, -1.5, 0.1, 17.0, -8.875])
    y = np.array([-0.3, 12.5, 2.0, -7.75, 5.5, 0.0, -20.125])
    z = np.array([9.5, -4.25, 0.6])
    s = Simplex_CLASS()
    s.newSeed(12345)
    o = OracleSimplex(12345)
    got, ref = s.noise3array(x, y, z), o.noise3array(x, y, z)
    assert got.shape == ref.shape == (3, 7, 5)
    assert (bits(got) == bits(ref)).all()
    assert ref[2, 5, 1] == o.noise3(x[1], y[5], z[2]) and len(set(bits(ref).ravel().tolist())) == ref.size


def test_noise3array_second_trip_of_the_grid_stride_loop():
    """257 x 129 x 127 = 4 210 431 elements, just over the 16384 x 256 a full grid covers in one trip; the whole array compared."""
    from simplex import Simplex_CLASS
    from oracle.simplex_oracle import OracleSimplex
    rs = np.random.RandomState(257)
    x, y, z = rs.uniform(-50, 50, 257), rs.uniform(-50, 50, 129), rs.uniform(-50, 50, 127)
    assert x.size * y.size * z.size > 16384 * 256
    s = Simplex_CLASS()
    s.newSeed(-987654321)
    got = s.noise3array(x, y, z)
    ref = OracleSimplex(-987654321).noise3array(x, y, z)
    bad = np.nonzero(bits(got).ravel() != bits(ref).ravel())[0]
    assert bad.size == 0, (bad.size, bad[:5], bad[-5:])


@pytest.mark.parametrize("scale", [1e3, 1e6, 2.0 ** 31, 3e10, 1e13, 2.0 ** 52])
def test_noise3array_at_large_coordinates(scale):
    """The grid kernel is always non-SAFE: (int) lattice bases up to 2^31, (long long) & 0xFF beyond, up to the domain's 2^52."""
    from simplex import Simplex_CLASS
    from oracle.simplex_oracle import OracleSimplex
    rs = np.random.RandomState(int(np.log2(scale)))
    x, y, z = (rs.uniform(-scale, scale, 16) for _ in range(3))
    for v in (x, y, z):
        v[:4] = np.floor(v[:4])
    s = Simplex_CLASS()
    s.newSeed(12345)
    got = s.noise3array(x, y, z)
    ref = OracleSimplex(12345).noise3array(x, y, z)
    assert (bits(got) == bits(ref)).all()
    assert (ref != 0).mean() > 0.9


def test_noise2array_at_large_coordinates():
    from simplex import Simplex_CLASS
    from oracle.simplex_oracle import OracleSimplex
    rs = np.random.RandomState(300)
    scale = np.repeat([1e2, 1e6, 3e10], 100)
    x, y = rs.uniform(-1, 1, 300) * scale, rs.permutation(rs.uniform(-1, 1, 300) * scale)
    x[::10], y[::7] = np.floor(x[::10]), np.floor(y[::7])
    assert np.abs(x).max() > 2e10 and x.min() < -2e10 and y.min() < -2e10
    s = Simplex_CLASS()
    s.newSeed(12345)
    got = s.noise2array(x, y)
    ref = OracleSimplex(12345).noise2array(x, y)
    assert got.shape == (300, 300) and (bits(got) == bits(ref)).all()
    assert (ref != 0).mean() > 0.9


def test_rand_2d_octaves_second_trip_of_the_grid_stride_loop():
    """2050 x 2050 = 4 202 500 elements: simplex2_kernel's loop takes its second trip (from n = 2049 on)."""
    from simplex import Simplex_CLASS
    from oracle.simplex_oracle import OracleSimplex
    s = Simplex_CLASS()
    s.newSeed(3)
    got = s.rand_2d_octaves((2050, 2050), 1, 0.5, 64)
    ref = OracleSimplex(3).rand_2d_octaves((2050, 2050), 1, 0.5, 64)
    assert 2050 * 2050 > 16384 * 256
    bad = np.nonzero(bits(got).ravel() != bits(ref).ravel())[0]
    assert bad.size == 0, (bad.size, bad[:5], bad[-5:])
