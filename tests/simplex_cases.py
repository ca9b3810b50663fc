"""Shared by the OpenSimplex launch tests (tests/test_simplex_reference.py on the CPU, tests/test_gpu_simplex_launch.py on the
device): the named launches of anoddpm_simplex3_octaves_f64 / _f32, their expected fields from the C oracle, and a plain fp64
restatement of what csrc/simplex.hip decides per thread and per launch.  No device needed here.

A case is a dict: one launch described by the fields of anoddpm_simplex_args (include/anoddpm_hip.h) plus the seeds of the table
sets that lie behind its `tables` pointer:
    seeds                  one per table set of the device allocation, in order (perm_tables(seed) each)
    tab_offset             sets by which `tables` is advanced into that allocation (diffusion.py hands self.tables[c:])
    table_sel              the int32 that *table_sel holds, or None for a NULL pointer
    table_sel_scale, table_slice_stride
    zvals                  int64[nslices], or None: z of slice s is z0 + s
    z0, nslices, H, W, octaves, persistence, frequency
    out_pad                out_slice_stride - H * W
Slice s reads table set  tab_offset + table_sel * table_sel_scale + s * table_slice_stride  (`table_index`).

The bar is the same everywhere: the f64 field equals `oracle_field(case)` as uint64 patterns, the f32 field equals
oracle_field(case).astype(float32) as uint32 patterns.  The oracle (oracle/simplex_oracle.c) is pinned to the reference bit for
bit by tests/test_oracle_simplex.py.

Domain: |coordinate of any octave| <= 2^52 (`DOMAIN`); `cases()` asserts it for every case.  Up to there the oracle and the numpy
restatement of the kernel's table algorithm agree bit for bit (tests/test_simplex_tables.py); at 2^60 they no longer do (the
oracle sums the three lattice floors as int64 and rounds once, the kernel as doubles), so neither is a yardstick beyond.

What the kernel decides, restated from its expressions (tests/test_simplex_reference.py pins these lines of the source, so a
change to one of them fails there until this file follows):
    safe  per thread   fmin > 0 and max(|x|, |y|, |z|) * 2 < 2147483000 * fmin,  fmin = frequency / 2^(octaves - 1)
                       true: the lattice base comes from the low word of floor + 1.5 * 2^49 (needs |floor| < 2^48)
                       false: (int)floor while all three |floor| < 2147483000, else (long long)floor & 0xFF
    pow2  per launch   frexp(frequency) == (0.5, fe) and fe > -900 and fe - octaves > -900 and fe < 900
                       true: x * (1 / f) with 1 / f doubled per octave; false: the IEEE division x / f, f halved per octave
                       (frexp's exponent of 2^k is k + 1: the largest power-of-two frequency on the multiply path is 2^898)
    rows_per_block     per launch, from tiles = ceil(W / 64) * ceil(H / 4) * nslices: 4 from 49152 tiles, 2 from 24576, else 1
"""
import functools
import math

import numpy as np

DOMAIN = 2.0 ** 52
INT_LIMIT = 2147483000.0                                          # the kernel's bound on a floor for the 32-bit conversion
MAGIC = 1.5 * 2.0 ** 49
SEEDS6 = (11, -22, 333333, -4444444444, 5, 9876543210)           # the six table sets of the selection cases (no seed is 0: newSeed
                                                                  # would draw a random one)
FREQUENCIES = {"0.5": 0.5, "1": 1.0, "2^-20": 2.0 ** -20, "2^20": 2.0 ** 20, "3": 3.0, "96": 96.0, "0.1": 0.1, "1e-3": 1e-3,
               "64+ulp": float(np.nextafter(64.0, np.inf)), "64-ulp": float(np.nextafter(64.0, 0.0))}
EDGE_FREQUENCIES = {"2^898": 2.0 ** 898, "2^899": 2.0 ** 899, "2^900": 2.0 ** 900}
ROW_WALK = {6143: 1, 6144: 2, 12287: 2, 12288: 4}                # nslices of W=1, H=13 (4 tiles per slice) -> rows_per_block


# ---------------------------------------------------------------------------- the kernel's decisions, restated
def safe(x, y, z, f0, octaves):
    """simplex3_octaves_kernel's per-thread `safe`; x, y, z: float64 arrays (the pixel indices and the slice's z as doubles)."""
    fmin = math.ldexp(f0, -(octaves - 1 if octaves > 0 else 0))
    big = np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z))
    return (fmin > 0.0) & (big * 2.0 < INT_LIMIT * fmin)


def pow2(f0, octaves):
    """simplex3_octaves_kernel's per-launch `pow2`."""
    m, fe = math.frexp(f0)
    return m == 0.5 and fe > -900 and fe - octaves > -900 and fe < 900


def tiles(case):
    return ((case["W"] + 63) // 64) * ((case["H"] + 3) // 4) * case["nslices"]


def rows_per_block(case):
    t = tiles(case)
    return 4 if t >= 4 * 8 * 1536 else (2 if t >= 2 * 8 * 1536 else 1)


def octave_scales(f0, octaves):
    """Per octave (multiply, s): the kernel forms a coordinate as x * s (pow2) or x / s (otherwise), in fp64 like this."""
    out = []
    if pow2(f0, octaves):
        rf = 1.0 / f0
        for _ in range(octaves):
            out.append((True, rf))
            rf = rf * 2.0
    else:
        f = f0
        for _ in range(octaves):
            out.append((False, f))
            f = f / 2
    return out


def lattice_floors(xc, yc, zc):
    """noise3()'s floor(xs), floor(ys), floor(zs) of a coordinate, in its operation order."""
    stretch = (xc + yc + zc) * (-1.0 / 6)
    return np.floor(xc + stretch), np.floor(yc + stretch), np.floor(zc + stretch)


def pixel_grid(case):
    """float64 [nslices][H][W] each: the x, y, z a thread converts from its indices."""
    z = zvalues(case).astype(np.float64)                         # (double)zi: exact below 2^53
    y, x = np.arange(case["H"], dtype=np.float64), np.arange(case["W"], dtype=np.float64)
    return np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None])


def octave_coordinates(case):
    """Per octave the fp64 coordinates (xc, yc, zc) of every pixel, [nslices][H][W] each."""
    x, y, z = pixel_grid(case)
    for mul, s in octave_scales(case["frequency"], case["octaves"]):
        yield (x * s, y * s, z * s) if mul else (x / s, y / s, z / s)


def safe_lanes(case):
    """bool [nslices][H][W]: the threads that take the SAFE instantiation."""
    return safe(*pixel_grid(case), case["frequency"], case["octaves"])


def int_branch(case):
    """bool [nslices][H][W]: every octave of the pixel has all three |floor| < 2147483000 -- what a non-SAFE thread needs to stay
    on the (int) conversion in every octave; False: at least one octave goes through (long long) & 0xFF."""
    ok = np.ones((case["nslices"], case["H"], case["W"]), dtype=bool)
    for c in octave_coordinates(case):
        fx, fy, fz = lattice_floors(*c)
        ok &= (np.abs(fx) < INT_LIMIT) & (np.abs(fy) < INT_LIMIT) & (np.abs(fz) < INT_LIMIT)
    return ok


# ---------------------------------------------------------------------------- the cases
def zvalues(case):
    if case["zvals"] is not None:
        return case["zvals"]
    return case["z0"] + np.arange(case["nslices"], dtype=np.int64)


def table_index(case):
    """int64[nslices]: index into case['seeds'] of the table set slice s reads."""
    base = case["tab_offset"] + (0 if case["table_sel"] is None else case["table_sel"] * case["table_sel_scale"])
    return base + np.arange(case["nslices"], dtype=np.int64) * case["table_slice_stride"]


def make_case(name, H, W, octaves, persistence, frequency, zvals=None, z0=0, nslices=None, seeds=(12345,), tab_offset=0,
              table_sel=None, table_sel_scale=1, table_slice_stride=0, out_pad=0):
    if zvals is not None:
        zvals = np.array(zvals, dtype=np.int64)
        assert nslices is None or nslices == zvals.size
        nslices = zvals.size
    case = dict(name=name, H=H, W=W, octaves=octaves, persistence=float(persistence), frequency=float(frequency), zvals=zvals, z0=z0,
                nslices=nslices, seeds=tuple(seeds), tab_offset=tab_offset, table_sel=table_sel, table_sel_scale=table_sel_scale,
                table_slice_stride=table_slice_stride, out_pad=out_pad)
    idx = table_index(case)
    assert idx.min() >= 0 and idx.max() == len(case["seeds"]) - 1, (name, "the table allocation ends with the last set that is read")
    assert all(case["seeds"])
    return case


@functools.lru_cache(maxsize=1)
def cases():
    out = []
    # ---- unsafe and mixed lanes
    # fmin = 5e-9: lanes with max(x, y, z) <= 5 are safe; unsafe lanes with x <= 10 stay below 2^31, the others exceed it
    out.append(make_case("tiny-f", 9, 70, 2, 0.5, 1e-8, zvals=[0, 5]))
    # a power-of-two frequency whose late octaves are unsafe: fmin = 2^-33
    out.append(make_case("deep-octaves", 9, 70, 40, 0.8, 64.0, zvals=[3]))
    # 2 |z| < 2147483000 flips between the second and the third value
    out.append(make_case("huge-z", 5, 66, 1, 0.5, 1.0, zvals=[1073741498, 1073741499, 1073741500, 1073741501, 10 ** 9, 2 ** 40 + 3,
                                                                -(2 ** 40) - 5, -1073741500, -7]))
    out.append(make_case("neg-z0", 6, 65, 3, 0.7, 24.0, z0=-37, nslices=75))
    # ---- frequency classes
    for label, f in FREQUENCIES.items():
        out.append(make_case(f"freq-{label}", 7, 67, 4, 0.85, f, zvals=[0, 999]))
    for label, f in EDGE_FREQUENCIES.items():
        out.append(make_case(f"freq-{label}", 7, 67, 3, 0.85, f, zvals=[0, 999]))
    # ---- geometry: widths around the 64-pixel tile, heights around the 4-row tile
    for W in (1, 63, 64, 65, 129):
        for H in (1, 3, 4, 5):
            out.append(make_case(f"geom-{H}x{W}", H, W, 3, 0.6, 16.0, zvals=[7, 411], seeds=(-987654321,)))
    # ---- row walk: four 4-row tiles per slice, the last one ragged; the tile counts around both thresholds of launch_simplex
    for n in ROW_WALK:
        out.append(make_case(f"rows-{n}", 13, 1, 1, 0.5, 8.0, nslices=n, seeds=(3,)))
    # ---- table selection: six sets on the device; *table_sel = 1, scale 2, one set further per slice -> sets 2, 3, 4
    sel = dict(H=5, W=66, octaves=2, persistence=0.8, frequency=16.0, zvals=[3, 500, 999])
    out.append(make_case("tables-sel", seeds=SEEDS6[:5], table_sel=1, table_sel_scale=2, table_slice_stride=1, **sel))
    out.append(make_case("tables-sel-advanced", seeds=SEEDS6, tab_offset=1, table_sel=1, table_sel_scale=2, table_slice_stride=1, **sel))
    out.append(make_case("tables-nosel-stride1", seeds=SEEDS6[:3], table_slice_stride=1, **sel))
    out.append(make_case("tables-stride2", seeds=SEEDS6[:5], table_slice_stride=2, **sel))
    out.append(make_case("tables-sel-stride0", seeds=SEEDS6[:4], table_sel=3, table_sel_scale=1, table_slice_stride=0, **sel))
    # ---- strides
    out.append(make_case("stride-pad5", 6, 65, 2, 0.5, 32.0, zvals=[1, 250, 998], out_pad=5))
    out.append(make_case("stride-pad5-z0", 3, 5, 2, 0.5, 4.0, z0=40, nslices=4, out_pad=5))
    # ---- the largest launch the entry points accept
    out.append(make_case("max-slices", 1, 1, 1, 0.5, 8.0, z0=1, nslices=65535, seeds=(3,)))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        assert coordinate_extent(c) <= DOMAIN, c["name"]
    return out


def coordinate_extent(case):
    """Largest |coordinate| of any octave of any pixel."""
    return max(max(float(np.abs(a).max()) for a in c) for c in octave_coordinates(case))


def case_names():
    return [c["name"] for c in cases()]


def get(name):
    return next(c for c in cases() if c["name"] == name)


_FIELDS = {}


def oracle_field(case):
    """float64 [nslices][H][W] from OracleSimplex._octaves, each slice with the table set `table_index` names.  Computed once per
    case and not to be written to."""
    if case["name"] not in _FIELDS:
        from oracle.simplex_oracle import OracleSimplex
        idx, z = table_index(case), zvalues(case)
        out = np.empty((case["nslices"], case["H"], case["W"]), dtype=np.float64)
        for i in np.unique(idx):
            rows = np.nonzero(idx == i)[0]
            out[rows] = OracleSimplex(case["seeds"][i])._octaves(z[rows], case["H"], case["W"], case["octaves"], case["persistence"],
                                                                 case["frequency"])
        out.setflags(write=False)
        _FIELDS[case["name"]] = out
    return _FIELDS[case["name"]]
