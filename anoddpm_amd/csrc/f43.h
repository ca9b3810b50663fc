// What the F(4x4,3x3) Winograd kernels share: winograd43.hip, winograd43r.hip, winograd43w.hip, winograd43b.hip (forward / data
// gradient) and wgrad43.hip (weight gradient).  Each kernel keeps its own structure -- accumulator ownership, K loop, rings,
// barriers, staging and epilogue; this header states once the transform arithmetic of
//     Y = A^T [ (G g G^T) (.) (B^T d B) ] A,   B^T 6x6, G 6x3, A^T 4x6  (Lavin & Gray, interpolation points 0, +-1, +-2, inf)
// as plain C++ (templates over float / float2), which tests/test_f43_math.py also compiles on the host, and -- for the device only --
// the activation of a staged operand value (f43_activate).
// A kernel uses a piece from here only where that leaves the machine code of every instantiation as it was
// (profiles/f43_shared_header_isa.txt lists which kernel keeps which piece written out, and why).
#pragma once

#ifdef __HIP__
#include "buf_load.h"
#include "common.h"
#define F43_FN __device__ __forceinline__
#define F43_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define F43_FN inline
#define F43_SCHED_FENCE() ((void)0)
#endif

// F43_PAIR_TRANSFORM=1 (measurement builds, ANODDPM_EXTRA_FLAGS): the product launches of winograd43.hip and winograd43r.hip use the
// row-pair input transform.  Measured equal to the single-row items (profiles/r6_f43_pair_transform_ab.txt).
#ifndef F43_PAIR_TRANSFORM
#define F43_PAIR_TRANSFORM 0
#endif

// Row u of B^T as four (patch row, coefficient) terms -- every row of B^T touches at most four patch rows:
//   u0: 4 d0 - 5 d2 + d4        u1: -4 d1 - 4 d2 + d3 + d4     u2: 4 d1 - 4 d2 - d3 + d4
//   u3: -2 d1 - d2 + 2 d3 + d4  u4: 2 d1 - d2 - 2 d3 + d4      u5: 4 d1 - 5 d3 + d5
// F43_BT_ROW(u) declares the patch rows tr0..tr3 and the coefficients tc0..tc3 of row u in the caller's scope:
//   (B^T d)[u][j] = tc0 d[tr0][j] + tc1 d[tr1][j] + tc2 d[tr2][j] + tc3 d[tr3][j], summed in this order.
// (A macro, not a function: every function or struct form of this table changed registers or wait instructions of some kernel.)
#define F43_BT_ROW(u)                                                                                                                  \
    const int tr0 = ((u) == 0) ? 0 : 1, tr1 = ((u) == 5) ? 3 : 2, tr2 = ((u) == 0) ? 4 : (((u) == 5) ? 5 : 3), tr3 = 4;                \
    const float tc0 = ((u) == 0) ? 4.f : ((u) == 1 ? -4.f : ((u) == 2 ? 4.f : ((u) == 3 ? -2.f : ((u) == 4 ? 2.f : 4.f))));            \
    const float tc1 = ((u) == 0 || (u) == 5) ? -5.f : (((u) == 1 || (u) == 2) ? -4.f : -1.f);                                          \
    const float tc2 = ((u) == 0 || (u) == 5) ? 1.f : ((u) == 1 ? 1.f : ((u) == 2 ? -1.f : ((u) == 3 ? 2.f : -2.f)));                   \
    const float tc3 = ((u) == 0 || (u) == 5) ? 0.f : 1.f

namespace anoddpm {

// A^T applied to six values: rows (1 1 1 1 1 0), (0 1 -1 2 -2 0), (0 1 1 4 4 0), (0 1 -1 8 -8 1)
template <typename T>
F43_FN void at6(const T (&m)[6], T (&o)[4])
{
    const T s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
    o[0] = m[0] + s12 + s34;
    o[1] = d12 + 2.f * d34;
    o[2] = s12 + 4.f * s34;
    o[3] = d12 + 8.f * d34 + m[5];
}

// Second stage of B^T d B: V[c * STRIDE] = sum_j t[j] B^T[c][j] for one row t of B^T d, c = 0..5 (STRIDE 1: into an array of six).
// Rows (1,2) and (3,4) share their partial sums.
template <int STRIDE, typename T>
F43_FN void bt_cols(const T (&t)[6], T *V)
{
    const T p = t[4] - 4.f * t[2], q = t[3] - 4.f * t[1], r = t[4] - t[2], s = t[3] - t[1];
    V[0 * STRIDE] = 4.f * t[0] - 5.f * t[2] + t[4];
    V[1 * STRIDE] = p + q;
    V[2 * STRIDE] = p - q;
    V[3 * STRIDE] = r + 2.f * s;
    V[4 * STRIDE] = r - 2.f * s;
    V[5 * STRIDE] = 4.f * t[1] - 5.f * t[3] + t[5];
}

// First stage as row PAIRS: up = 0 forms rows (0, 5) of B^T d, 1 rows (1, 2), 2 rows (3, 4) of a 6x6 tile at D (rows PROW, columns
// PP elements apart).  Rows (1,2) and (3,4) share their partial sums and (0,5) read disjoint patch rows: 4 operations per column
// and row pair where the single-row form spends 4 per row, and literal coefficients.  FENCE keeps one column of reads in flight.
F43_FN int bt_pair_first(int up) { return up == 0 ? 0 : (up == 1 ? 1 : 3); }
F43_FN int bt_pair_second(int up) { return up == 0 ? 5 : (up == 1 ? 2 : 4); }
template <int PROW, int PP, bool FENCE, typename T>
F43_FN void bt_row_pair(int up, const T *D, T (&ta)[6], T (&tb)[6])
{
    if (up == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const T d0 = D[j * PP], d1 = D[PROW + j * PP], d2 = D[2 * PROW + j * PP], d3 = D[3 * PROW + j * PP], d4 = D[4 * PROW + j * PP], d5 = D[5 * PROW + j * PP];
            ta[j] = 4.f * d0 - 5.f * d2 + d4;
            tb[j] = 4.f * d1 - 5.f * d3 + d5;
            if (FENCE) F43_SCHED_FENCE();
        }
    } else if (up == 1) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const T d1 = D[PROW + j * PP], d2 = D[2 * PROW + j * PP], d3 = D[3 * PROW + j * PP], d4 = D[4 * PROW + j * PP];
            const T p = d4 - 4.f * d2, q = d3 - 4.f * d1;
            ta[j] = p + q;
            tb[j] = p - q;
            if (FENCE) F43_SCHED_FENCE();
        }
    } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const T d1 = D[PROW + j * PP], d2 = D[2 * PROW + j * PP], d3 = D[3 * PROW + j * PP], d4 = D[4 * PROW + j * PP];
            const T r = d4 - d2, w = d3 - d1;
            ta[j] = r + 2.f * w;
            tb[j] = r - 2.f * w;
            if (FENCE) F43_SCHED_FENCE();
        }
    }
}

}  // namespace anoddpm

#ifdef __HIP__
namespace anoddpm {

// One staged operand value (four channels of a patch pixel): GroupNorm-apply with the channels' scale / shift, then SiLU.  FAST = the
// launch has both (no flags to test); the zero padding of the activated map is applied by the caller AFTER this.
template <bool FAST>
__device__ __forceinline__ f32x4 f43_activate(f32x4 v, const f32x4 asc, const f32x4 ash, bool affine, bool act)
{
    if (FAST) {
        v = v * asc + ash;
        v[0] = silu_f(v[0]); v[1] = silu_f(v[1]); v[2] = silu_f(v[2]); v[3] = silu_f(v[3]);
    } else {
        if (affine) v = v * asc + ash;
        if (act) { v[0] = silu_f(v[0]); v[1] = silu_f(v[1]); v[2] = silu_f(v[2]); v[3] = silu_f(v[3]); }
    }
    return v;
}

}  // namespace anoddpm
#endif
