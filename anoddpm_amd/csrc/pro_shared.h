// What csrc/pro.hip (one workgroup per segment) and csrc/pro_wide.hip (one segment over the whole chip) both compute, stated once:
// the key of an element with its precondition bits, the element of the descending walk with its weight 1 / area, the fp64 scan
// over a 64-lane group, a curve point's PRO value and the trapezoid term of a curve point.  The outputs of the two files are
// bit-identical because these are the same functions, compiled with -ffp-contract=off in both.
#pragma once
#include "common.h"

namespace anoddpm {
namespace pro {

// key = (bits(score + 0.0f) << 1) | (area != 0); the precondition bits of the element are OR-ed into st.  has_mask: m is the
// mask value the area came from, only checked
__device__ __forceinline__ uint32_t make_key(float s, int32_t ar, bool has_mask, float m, uint32_t &st)
{
    if (s != s) st |= ANODDPM_ROC_NAN;
    else if (s == INFINITY || s == -INFINITY) st |= ANODDPM_ROC_INF;
    if (s < 0.0f) st |= ANODDPM_ROC_NEGATIVE;
    if (has_mask && !(m == 0.0f || m == 1.0f)) st |= ANODDPM_ROC_BAD_MASK;
    return (__float_as_uint(s + 0.0f) << 1) | (ar != 0 ? 1u : 0u);       // -0.0 + 0.0 = +0.0
}

// inclusive fp64 scan over the 64 lanes of a wave, Hillis-Steele: the order of the additions is the same everywhere it is used
__device__ __forceinline__ double group_scan(double v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// element j of the descending order (sorted index n - 1 - j) of a walk that ends in front of position c1
struct Elem { bool valid, pos, end; uint32_t key; double w; };

__device__ __forceinline__ Elem elem_of(const uint32_t *__restrict__ key, const int32_t *__restrict__ area, uint32_t j, uint32_t c1, uint32_t n)
{
    Elem e;
    e.valid = j < c1;
    e.key = 0;
    e.pos = e.end = false;
    e.w = 0.0;
    if (e.valid) {
        const uint32_t i = n - 1 - j;
        e.key = key[i];
        e.pos = (e.key & 1u) != 0;
        e.end = i == 0 || (key[i - 1] >> 1) != (e.key >> 1);     // i - 1 may belong to another wave or tile
        if (e.pos) e.w = 1.0 / (double)area[i];
    }
    return e;
}

// PRO of the curve point whose inclusive weight sum is carry + incl
__device__ __forceinline__ double pro_value(double carry, double incl, unsigned long long K)
{
    return K == 0 ? (double)NAN : fmin((carry + incl) / (double)K, 1.0);
}

// the area between the curve points (x0, y0) and (x1, y1) below the FPR limit: the term of point q in the truncated trapezoid
__device__ __forceinline__ double trapezoid_term(double x0, double y0, double x1, double y1, double limit)
{
    double term = 0.0;
    if (x0 < limit) {
        if (x1 <= limit) term = (x1 - x0) * (y1 + y0) * 0.5;
        else {
            const double yl = y0 + (y1 - y0) * ((limit - x0) / (x1 - x0));
            term = (limit - x0) * (yl + y0) * 0.5;
        }
    }
    return term;
}

// the term of curve point q from the compact run arrays (point q - 1 is (0, 0) for q = 0)
__device__ __forceinline__ double term_of(const uint32_t *__restrict__ runfps, const double *__restrict__ runpro, uint32_t q, double dN, double limit)
{
    const double x1 = (double)runfps[q] / dN, y1 = runpro[q];
    const double x0 = q ? (double)runfps[q - 1] / dN : 0.0, y0 = q ? runpro[q - 1] : 0.0;
    return trapezoid_term(x0, y0, x1, y1, limit);
}

}  // namespace pro
}  // namespace anoddpm
