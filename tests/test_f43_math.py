"""The F(4x4,3x3) transform arithmetic of anoddpm_amd/csrc/f43.h, compiled as plain C++ on the host (no HIP header) and checked
in float against the matrices of Lavin & Gray (interpolation points 0, +-1, +-2, inf) evaluated in fp64.  CPU only.

The header states each transform once for all F(4x4) kernels; this pins what it states.

Bounds.  u = 2^-24.  A result is a two-stage sum of products; with k roundings on the longest path of a result, the computed value
differs from the exact one by at most gamma_k = k u / (1 - k u) times the same expression evaluated on absolute values,
(|L| |x| |R|)[i][j] -- the largest term each result can contain, row by row.  Counted from the header's expressions:
  * B^T d B through the row table F43_BT_ROW + bt_cols.  Products by +-1, +-2, +-4 are exact, those by +-5 round.  First stage
    c0 d + c1 d + c2 d + c3 d: rows 0 and 5 round the product by 5 and two additions (their fourth term is an exact 0), rows 1..4
    round three additions -- at most 4.  Second stage: 4 t0 - 5 t2 + t4 rounds one product and two additions, p + q rounds p (or q)
    and the sum -- at most 3.  k = 7 (a compiler that fuses a product into the next addition only removes roundings).
  * the row-pair first stage (bt_row_pair) rounds at most 3 times (4 d0 - 5 d2 + d4) where the single-row form rounds 4: it obeys
    the same k = 7, so pair and single-row results lie within 2 gamma_7 of each other.
  * A^T m A through at6, columns then rows: 3 roundings per stage on the longest path (m1 +- m2, then two additions; the factors
    2, 4, 8 are exact): k = 6.
Measured on the 64 random tiles below (x86-64, clang -O2): the largest error is 0.35 of the B^T d B bound for the single-row and for
the row-pair form, 0.17 of the pair-against-single bound and 0.39 of the A^T m A bound."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BT = np.array([[4, 0, -5, 0, 1, 0],
               [0, -4, -4, 1, 1, 0],
               [0, 4, -4, -1, 1, 0],
               [0, -2, -1, 2, 1, 0],
               [0, 2, -1, -2, 1, 0],
               [0, 4, 0, -5, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0],
               [0, 1, -1, 2, -2, 0],
               [0, 1, 1, 4, 4, 0],
               [0, 1, -1, 8, -8, 1]], dtype=np.float64)
TILES = 64
U = 2.0 ** -24

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "f43.h"
using namespace anoddpm;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static float rnd()                       // xorshift64*: uniform in [-4, 4)
{
    state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
    return (float)((double)((state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 8.0 - 4.0);
}
static void put(const float *p, int n) { for (int i = 0; i < n; ++i) std::printf("%a ", (double)p[i]); std::printf("\n"); }

int main()
{
    for (int tile = 0; tile < TILES; ++tile) {
        float d[36], vs[36], vp[36], m[36], y[16];
        for (int i = 0; i < 36; ++i) d[i] = rnd();
        for (int i = 0; i < 36; ++i) m[i] = rnd();
        // single-row items: row u of B^T d from the (patch row, coefficient) terms, then the column pass
        for (int u = 0; u < 6; ++u) {
            float t[6];
            F43_BT_ROW(u);
            for (int j = 0; j < 6; ++j) t[j] = tc0 * d[tr0 * 6 + j] + tc1 * d[tr1 * 6 + j] + tc2 * d[tr2 * 6 + j] + tc3 * d[tr3 * 6 + j];
            bt_cols<1>(t, vs + u * 6);
        }
        // row-pair items
        for (int up = 0; up < 3; ++up) {
            float ta[6], tb[6];
            bt_row_pair<6, 1, false>(up, d, ta, tb);
            bt_cols<1>(ta, vp + bt_pair_first(up) * 6);
            bt_cols<1>(tb, vp + bt_pair_second(up) * 6);
        }
        // A^T m A: columns first, then rows
        float yc[4][6];
        for (int v = 0; v < 6; ++v) {
            float mu[6], o[4];
            for (int u = 0; u < 6; ++u) mu[u] = m[u * 6 + v];
            at6(mu, o);
            for (int i = 0; i < 4; ++i) yc[i][v] = o[i];
        }
        for (int i = 0; i < 4; ++i) {
            float o[4];
            at6(yc[i], o);
            for (int j = 0; j < 4; ++j) y[i * 4 + j] = o[j];
        }
        put(d, 36); put(vs, 36); put(vp, 36); put(m, 36); put(y, 16);
    }
    return 0;
}
"""


def host_clangxx():
    """The LLVM clang++ that ships with ROCm (next to the hipcc anoddpm_amd.build uses), else any clang++ on the PATH."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"),
              "/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    cxx = host_clangxx()
    assert cxx is not None, "no clang++: the ROCm toolchain that builds the library ships one"
    tmp = tmp_path_factory.mktemp("f43_math")
    src, exe = tmp / "f43_math.cpp", tmp / "f43_math"
    src.write_text(PROGRAM)
    r = subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-DTILES={TILES}",
                        "-I", os.path.join(ROOT, "anoddpm_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [np.array([float.fromhex(x) for x in line.split()], dtype=np.float64) for line in out if line.strip()]
    assert len(rows) == 5 * TILES
    pick = lambda k, shape: np.stack([rows[5 * t + k].reshape(shape) for t in range(TILES)])
    return {"d": pick(0, (6, 6)), "v_single": pick(1, (6, 6)), "v_pair": pick(2, (6, 6)), "m": pick(3, (6, 6)), "y": pick(4, (4, 4))}


def gamma(k):
    return k * U / (1.0 - k * U)


def worst(err, bound):
    ratio = float((err / bound).max())
    print(f"largest error / bound = {ratio:.3f}")
    return ratio


def test_bt_row_and_bt_cols_are_bt_d_b(tiles):
    d = tiles["d"]
    exact = BT @ d @ BT.T
    bound = gamma(7) * (np.abs(BT) @ np.abs(d) @ np.abs(BT.T))
    assert worst(np.abs(tiles["v_single"] - exact), bound) <= 1.0


def test_row_pair_form_equals_single_row_form(tiles):
    d = tiles["d"]
    exact = BT @ d @ BT.T
    bound = gamma(7) * (np.abs(BT) @ np.abs(d) @ np.abs(BT.T))
    assert worst(np.abs(tiles["v_pair"] - exact), bound) <= 1.0
    assert worst(np.abs(tiles["v_pair"] - tiles["v_single"]), 2.0 * bound) <= 1.0


def test_at6_columns_then_rows_is_at_m_a(tiles):
    m = tiles["m"]
    exact = AT @ m @ AT.T
    bound = gamma(6) * (np.abs(AT) @ np.abs(m) @ np.abs(AT.T))
    assert worst(np.abs(tiles["y"] - exact), bound) <= 1.0
