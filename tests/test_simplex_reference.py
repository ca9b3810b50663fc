"""CPU: what csrc/simplex.hip rests on besides its generated tables (tests/test_simplex_tables.py), and what the cases of
tests/simplex_cases.py reach.  No device and no HIP library: numpy, exact rationals and the C oracle.

  * the lattice-base identity of the SAFE path: the low word of floor + 1.5 * 2^49 is 8 * floor in two's complement -- on every
    listed floor, and shown to stop at |floor| = 2^48, which is what `SAFE` may assume at most
  * the per-thread `safe` predicate implies |floor| < 2^31 in every octave, on every case and on a sweep around its threshold
  * div_norm3, the two-FMA division by 103, emulated with one rounding per operation on exact rationals, against v / 103.0 on
    random values and on quotients as close to a rounding midpoint as doubles allow
  * the power-of-two classification of the frequency and what the multiply path assumes of it
  * the restated predicates are the source's own expressions (the lines are pinned: a changed factor in the kernel fails here)
  * every case reaches the path it is named for, lies inside the 2^52 domain and has a field that is not trivially zero
"""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import simplex_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "anoddpm_amd", "csrc", "simplex.hip")
WRAPPER = os.path.join(ROOT, "anoddpm_amd", "simplex.py")


def lo32(a):
    return (np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def magic_offset(fx):
    """(lo32(fx + 1.5 * 2^49) & 0x7F8, 8 * (int(fx) & 255)): what the SAFE path takes as the table offset, and what it stands for."""
    fx = np.asarray(fx, dtype=np.float64)
    want = np.array([8 * (int(v) & 255) for v in fx], dtype=np.int64)
    return lo32(fx + sc.MAGIC) & 0x7F8, want


# ---------------------------------------------------------------------------- the magic constant
def test_low_word_of_floor_plus_magic_is_eight_times_the_floor():
    k = np.arange(0, 300, dtype=np.float64)
    floors = np.concatenate([np.arange(-600, 601, dtype=np.float64), [2147483000.0, -2147483000.0, 2.0 ** 31 - 1, -(2.0 ** 31)],
                             2.0 ** 40 + k, -(2.0 ** 40) - k, 2.0 ** 47 + k, -(2.0 ** 47) - k,
                             2.0 ** 48 - 1 - k, -(2.0 ** 48) + k])          # the last floors on which it holds
    assert (floors == np.floor(floors)).all()
    got, want = magic_offset(floors)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (floors[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert len({int(w) for w in want}) == 256                               # every table offset occurs


def test_the_identity_stops_at_two_to_the_48():
    """From 2^48 the sum leaves [2^49, 2^50), where one ulp is 1/8: above it the low word counts quarters, below -2^48 sixteenths.
    `safe` keeps |floor| below 2^31, seventeen binades inside."""
    k = np.arange(1, 256, dtype=np.float64)
    for floors in (2.0 ** 48 + k, -(2.0 ** 48) - k):
        assert (np.abs(floors) < 2.0 ** 53).all()
        got, want = magic_offset(floors)
        assert (got != want).all()
    assert np.spacing(sc.MAGIC + 2.0 ** 48 - 1) == 0.125 and np.spacing(sc.MAGIC + 2.0 ** 48) == 0.25
    assert np.spacing(sc.MAGIC - 2.0 ** 48) == 0.125 and np.spacing(sc.MAGIC - 2.0 ** 48 - 1) == 0.0625


# ---------------------------------------------------------------------------- safe
def _worst_floor(x, y, z, f0, octaves):
    worst = np.zeros(np.broadcast(x, y, z).shape)
    for mul, s in sc.octave_scales(f0, octaves):
        c = (x * s, y * s, z * s) if mul else (x / s, y / s, z / s)
        for f in sc.lattice_floors(*c):
            worst = np.maximum(worst, np.abs(f))
    return worst


@pytest.mark.parametrize("name", sc.case_names())
def test_safe_lanes_of_every_case_have_floors_below_two_to_the_31(name):
    case = sc.get(name)
    s = sc.safe_lanes(case)
    worst = _worst_floor(*sc.pixel_grid(case), case["frequency"], case["octaves"])
    assert (worst[s] < 2.0 ** 31).all()
    assert not (s & ~sc.int_branch(case)).any()                  # a safe lane would also pass the non-SAFE path's own 32-bit test


def test_safe_implies_the_bound_around_its_threshold():
    """Coordinates one step either side of max * 2 < 2147483000 * fmin, on each axis and in the sign patterns that stretch a
    coordinate furthest (x, y are pixel indices >= 0, z any int64): wherever the predicate holds every floor of every octave is
    below 2^31, and the predicate does flip inside each sweep that reaches its threshold."""
    flips = 0
    for f0 in (1.0, 3.0, 64.0, 24.0, 0.1, 1e-8, 2.0 ** -20, 2.0 ** 20, 1e-3):
        for octaves in (1, 2, 5, 9):
            fmin = math.ldexp(f0, -(octaves - 1))
            edge = sc.INT_LIMIT * fmin / 2.0
            near = np.unique(np.clip(np.floor(edge) + np.arange(-3, 4), 0, None))
            m = np.concatenate([near, np.floor(near / 2), [0.0, 1.0, 5.0]])
            zero = np.zeros_like(m)
            for x, y, z in ((m, zero, zero), (zero, m, zero), (zero, zero, m), (zero, zero, -m), (m, m, m), (m, m, -m), (m, zero, -m),
                            (zero, m, -m), (m, np.floor(m / 3), -np.floor(m / 2))):
                s = sc.safe(x, y, z, f0, octaves)
                worst = _worst_floor(x, y, z, f0, octaves)
                assert (worst[s] < 2.0 ** 31).all(), (f0, octaves, worst[s].max())
                flips += bool(s.any() and not s.all())
    assert flips >= 100


def _source_line(path, marker):
    lines = [" ".join(l.split()) for l in open(path) if marker in l]
    assert len(lines) == 1, (marker, lines)
    return lines[0]


def test_the_restated_predicates_are_the_source_s_expressions():
    """tests/simplex_cases.py restates these lines; whoever changes one of them changes the restatement with it."""
    assert _source_line(SOURCE, "const bool safe =") == \
        "const bool safe = fmin > 0.0 && fmax(fmax(fabs(xd), fabs(yd)), fabs(zd)) * 2.0 < 2147483000.0 * fmin;"
    assert _source_line(SOURCE, "const double fmin =") == "const double fmin = ldexp(f0, -(a.octaves > 0 ? a.octaves - 1 : 0));"
    assert _source_line(SOURCE, "const bool pow2 =") == \
        "const bool pow2 = (frexp(f0, &fe) == 0.5) && fe > -900 && fe - a.octaves > -900 && fe < 900;"
    assert _source_line(SOURCE, "if (fabs(fx) <") == \
        "if (fabs(fx) < 2147483000.0 && fabs(fy) < 2147483000.0 && fabs(fz) < 2147483000.0) {"
    assert _source_line(SOURCE, "constexpr double MAGIC") .startswith("constexpr double MAGIC = 844424930131968.0;")
    assert sc.MAGIC == 844424930131968.0
    assert _source_line(SOURCE, "const long long tiles =") == \
        "const long long tiles = (long long)((a->W + 63) / 64) * ((a->H + 3) / 4) * a->nslices;"
    assert _source_line(SOURCE, "const int rpb =") .startswith("const int rpb = tiles >= 4ll * 8 * 1536 ? 4 : (tiles >= 2ll * 8 * 1536 ? 2 : 1);")
    assert _source_line(SOURCE, "(long long)s * a.table_slice_stride") == "(long long)s * a.table_slice_stride;"
    assert _source_line(SOURCE, "long long tab =") == "long long tab = (a.table_sel ? (long long)(*a.table_sel) * a.table_sel_scale : 0) +"


def _chunks(wrapper_text, nslices, z0, limit=65535):
    """The launches of Simplex_CLASS._octaves_f64's chunk loop, run from the loop's own source lines on plain integers:
    [(first output slice, nslices, first zvals index, z0)]."""
    m = re.search(r"for s0 in range\(0, nslices, (\d+)\):.*?\n((?:\s+.*\n)+?)\s+check\(", wrapper_text)
    assert m, "the chunk loop of _octaves_f64"
    step, body = int(m.group(1)), m.group(2)
    assert step <= limit
    for needle in ("n = min(%d, nslices - s0)" % step, "a.out = out.data_ptr() + 8 * s0 * H * W", "a.nslices = n",
                   "a.zvals = zt.data_ptr() + 8 * s0", "a.z0 = int(z0) + s0"):
        assert needle in body, needle
    return [(s0, min(step, nslices - s0), s0, z0 + s0) for s0 in range(0, nslices, step)]


def test_the_wrapper_s_chunks_tile_the_volume():
    """_octaves_f64 splits a volume into launches of at most 32768 slices; the launches must cover every slice once, each with
    the z it had in the whole volume (z0 + s for a NULL zvals, zvals[s] otherwise) -- checked on the loop's own statements."""
    text = open(WRAPPER).read()
    for nslices, z0 in ((40000, 0), (32768, 5), (32769, -3), (1, 0), (98305, 7)):
        seen = np.full(nslices, -1, dtype=np.int64)
        zs = np.zeros(nslices, dtype=np.int64)
        for first, n, zfirst, zz0 in _chunks(text, nslices, z0):
            assert 0 < n <= 65535 and first == zfirst
            assert (seen[first:first + n] == -1).all()
            seen[first:first + n] = first
            zs[first:first + n] = zz0 + np.arange(n)
        assert (seen >= 0).all() and (zs == z0 + np.arange(nslices)).all()


# ---------------------------------------------------------------------------- division by 103
def _fma(a, b, c):
    """IEEE fma: a b + c rounded once (float(Fraction) rounds to nearest even).  An exact zero takes the common sign of the
    product and the addend when both are zeros of one sign, and is +0.0 otherwise."""
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact != 0:
        return float(exact)
    psign = math.copysign(1.0, a) * math.copysign(1.0, b)
    return -0.0 if (a == 0 or b == 0) and c == 0 and psign < 0 and math.copysign(1.0, c) < 0 else 0.0


def _div_norm3(v):
    """div_norm3 of csrc/simplex.hip on a normal-range double or a zero, one rounding per operation: q = fl(v r), then two FMAs."""
    r = 1.0 / 103.0
    q = v * r
    return _fma(_fma(-103.0, q, v), r, q)


def test_two_fma_division_by_103_is_the_ieee_quotient():
    rs = np.random.RandomState(103)
    # (a) random magnitudes over the range of a noise sum (attn^4 (g . d) >= 2^-208 11 d; |sum| < 1e4)
    a = np.exp(rs.uniform(math.log(1e-70), math.log(1e5), 20000)) * rs.choice([-1.0, 1.0], 20000)
    # (b) quotients next to a rounding midpoint: v = fl(103 (q + ulp(q) / 2)) and its two neighbours
    q = np.ldexp(rs.uniform(0.5, 1.0, 14000), rs.randint(-200, 15, 14000)) * rs.choice([-1.0, 1.0], 14000)
    mid = np.array([float(103 * (Fraction(x) + Fraction(float(np.spacing(x))) / 2)) for x in q])
    b = np.concatenate([mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf)])
    assert a.size >= 20000 and b.size >= 40000 and np.abs(q).min() < 2.0 ** -199 and np.abs(q).max() > 2.0 ** 13
    v = np.concatenate([a, b])
    got = np.array([_div_norm3(float(x)) for x in v])
    want = v / 103.0
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, (bad.size, v[bad[:5]], got[bad[:5]], want[bad[:5]])
    # (c) the zeros.  +0.0 gives +0.0 like the division.  -0.0 does NOT give the division's -0.0: the residual fma(-103, -0, -0) is
    # (+0) + (-0) = +0, and fma(+0, r, -0) = +0.  The kernel never asks: noise3's sum starts at +0.0, and neither adding a -0.0
    # term to it nor cancelling two terms can make a -0.0 (round to nearest), so div_norm3 sees +0.0 or a non-zero; the oracle's
    # sum is formed the same way and its fields hold no -0.0 either (asserted per case below).
    pz, nz = np.array([_div_norm3(0.0), 0.0 / 103.0]), np.array([_div_norm3(-0.0), -0.0 / 103.0])
    assert pz.view(np.uint64).tolist() == [0, 0]
    assert nz.view(np.uint64).tolist() == [0, 1 << 63]
    zero_sums = np.array([0.0 + -0.0, 0.0 + 1.0 * -0.0, 1.5 + -1.5, -1.5 + 1.5, _fma(-0.0, 1.0, 0.0), _fma(-2.5, 0.0, 0.0)])
    assert (zero_sums.view(np.uint64) == 0).all()


# ---------------------------------------------------------------------------- frequency classes
POW2_TRUE = [(0.5, 4), (1.0, 4), (2.0 ** -20, 4), (2.0 ** 20, 4), (2.0 ** 898, 3)]
POW2_FALSE = [(3.0, 4), (96.0, 4), (0.1, 4), (1e-3, 4), (sc.FREQUENCIES["64+ulp"], 4), (sc.FREQUENCIES["64-ulp"], 4),
              (2.0 ** 899, 3), (2.0 ** 900, 3)]


def test_power_of_two_classification():
    """frexp(2^k) is (0.5, k + 1): `fe < 900` admits 2^898 and sends 2^899 and 2^900 to the IEEE division -- the cases hold all
    three, so both sides of the edge are run."""
    assert sorted(f for f, _ in POW2_TRUE + POW2_FALSE) == sorted(list(sc.FREQUENCIES.values()) + list(sc.EDGE_FREQUENCIES.values()))
    for f, o in POW2_TRUE:
        assert sc.pow2(f, o), f
    for f, o in POW2_FALSE:
        assert not sc.pow2(f, o), f
    assert math.frexp(2.0 ** 898) == (0.5, 899) and math.frexp(2.0 ** 899) == (0.5, 900)
    # the lower limit: fe - octaves > -900 (with a launch's octaves >= 1 it is the one of the two that binds)
    assert sc.pow2(2.0 ** -899, 1) and not sc.pow2(2.0 ** -900, 1) and sc.pow2(2.0 ** -890, 10) and not sc.pow2(2.0 ** -890, 11)
    # the octave count alone takes a power-of-two frequency from all-safe to all-unsafe ('deep-octaves')
    x = np.array([69.0])
    assert sc.safe(x, x, x, 64.0, 8).all() and not sc.safe(x, x, x, 64.0, 40).any() and sc.pow2(64.0, 40)
    for case in sc.cases():
        if case["name"].startswith("freq-"):
            f = {**sc.FREQUENCIES, **sc.EDGE_FREQUENCIES}[case["name"][5:]]
            assert case["frequency"] == f and (f, case["octaves"]) in POW2_TRUE + POW2_FALSE


@pytest.mark.parametrize("f,octaves", POW2_TRUE + [(64.0, 40), (16.0, 3), (8.0, 1)])
def test_multiplying_by_the_reciprocal_is_the_division_on_the_power_of_two_path(f, octaves):
    x = np.arange(4096, dtype=np.float64)
    x = np.concatenate([x, -x, [2.0 ** 40 + 3, -(2.0 ** 40) - 5, 1073741499.0]])
    scales = sc.octave_scales(f, octaves)
    assert len(scales) == octaves and all(mul for mul, _ in scales)
    fo = f
    for _, rf in scales:
        assert rf == 1.0 / fo and Fraction(rf) * Fraction(fo) == 1           # 1 / f doubles exactly: it IS the reciprocal of f_o
        assert ((x * rf).view(np.uint64) == (x / fo).view(np.uint64)).all()
        fo = fo / 2


# ---------------------------------------------------------------------------- the cases reach what they are named for
def test_tiny_f_has_a_wave_with_safe_lanes_and_both_unsafe_conversions():
    case = sc.get("tiny-f")
    s, small = sc.safe_lanes(case), sc.int_branch(case)
    x, y, z = sc.pixel_grid(case)
    assert (s == (np.maximum(np.maximum(x, y), z) <= 5)).all()
    # x / fmin = 2e8 x; the stretch term takes up to (x + 13) / 6 of that off again: up to x = 10 every floor stays below 2^31,
    # from x = 16 the x floor is beyond it whatever y and z are
    assert small[~s & (x <= 10)].all() and (~s & (x <= 10)).sum() > 100 and not small[x >= 16].any()
    mixed = 0
    for sl in range(case["nslices"]):
        for row in range(case["H"]):
            lanes, lo = s[sl, row, :64], small[sl, row, :64]       # one wave: 64 consecutive x of one row
            mixed += bool(lanes.any() and (~lanes & lo).any() and (~lanes & ~lo).any())
    assert mixed >= 6
    assert not sc.pow2(case["frequency"], case["octaves"])


def test_deep_octaves_is_a_power_of_two_frequency_on_the_unsafe_path():
    case = sc.get("deep-octaves")
    assert sc.pow2(case["frequency"], case["octaves"]) and not sc.safe_lanes(case).any()
    # late octaves pass 2^31: both conversions of the non-SAFE path inside one thread's octave loop
    first = next(iter(sc.octave_coordinates(case)))
    assert all(np.abs(f).max() < sc.INT_LIMIT for f in sc.lattice_floors(*first)) and not sc.int_branch(case).any()


def test_huge_z_lies_on_both_sides_of_the_threshold():
    case = sc.get("huge-z")
    s = sc.safe_lanes(case)
    per_slice = s.all(axis=(1, 2))
    assert (per_slice == s.any(axis=(1, 2))).all()               # z alone decides
    assert per_slice.tolist() == [True, True, False, False, True, False, False, False, True]
    small = sc.int_branch(case).all(axis=(1, 2))
    assert small.tolist() == [True, True, True, True, True, False, False, True, True]
    assert (case["zvals"] < 0).sum() == 3


def test_neg_z0_crosses_zero_on_the_division_path():
    case = sc.get("neg-z0")
    z = sc.zvalues(case)
    assert case["zvals"] is None and z[0] == -37 and z[-1] == 37 and not sc.pow2(case["frequency"], case["octaves"])


def test_row_walk_and_geometry_cases():
    for n, rpb in sc.ROW_WALK.items():
        case = sc.get(f"rows-{n}")
        assert sc.tiles(case) == 4 * n and sc.rows_per_block(case) == rpb and case["H"] % 4 == 1
    assert [sc.tiles(sc.get(f"rows-{n}")) for n in sc.ROW_WALK] == [24572, 24576, 49148, 49152]
    assert sc.rows_per_block(sc.get("max-slices")) == 4 and sc.get("max-slices")["nslices"] == 65535
    assert {(c["H"], c["W"]) for c in sc.cases() if c["name"].startswith("geom-")} == \
        {(h, w) for h in (1, 3, 4, 5) for w in (1, 63, 64, 65, 129)}


def test_table_selection_cases_name_the_sets_they_say():
    assert sc.table_index(sc.get("tables-sel")).tolist() == [2, 3, 4]
    assert sc.table_index(sc.get("tables-sel-advanced")).tolist() == [3, 4, 5]
    assert sc.table_index(sc.get("tables-nosel-stride1")).tolist() == [0, 1, 2]
    assert sc.table_index(sc.get("tables-stride2")).tolist() == [0, 2, 4]
    assert sc.table_index(sc.get("tables-sel-stride0")).tolist() == [3, 3, 3]
    # the slices of a selection case differ from what any other of the six sets gives: a wrong set cannot pass
    from oracle.simplex_oracle import OracleSimplex
    case = sc.get("tables-sel-advanced")
    ref = sc.oracle_field(case)
    for s, z in enumerate(case["zvals"]):
        same = [i for i, seed in enumerate(sc.SEEDS6)
                if (OracleSimplex(seed)._octaves([z], case["H"], case["W"], case["octaves"], case["persistence"], case["frequency"])[0]
                    .view(np.uint64) == ref[s].view(np.uint64)).all()]
        assert same == [3 + s]


@pytest.mark.parametrize("name", sc.case_names())
def test_every_case_is_inside_the_domain_and_not_trivial(name):
    case = sc.get(name)
    assert sc.coordinate_extent(case) <= sc.DOMAIN
    ref = sc.oracle_field(case)
    assert ref.shape == (case["nslices"], case["H"], case["W"]) and np.isfinite(ref).all()
    assert (ref != 0).mean() >= 0.9
    assert not (np.signbit(ref) & (ref == 0)).any()              # a zero of a field is +0.0 (see the division test)
    if case["nslices"] > 1 and case["H"] * case["W"] > 1:
        assert len({ref[s].tobytes() for s in range(case["nslices"])}) == case["nslices"]      # no two slices alike
