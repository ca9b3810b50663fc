// What csrc/roc.hip (one workgroup per segment) and csrc/roc_wide.hip (one segment over the whole chip) both compute, stated once:
// the key of an element with its precondition bits, the rank of a key among the equal digits of its 64-lane group, sklearn's
// drop rule for a curve point, the total order of the best Dice, and the two halving trees that end the average-precision sum.
// The outputs of the two files are bit-identical because these are the same functions.  Integer code except tree_add.
#pragma once
#include "common.h"

namespace anoddpm {
namespace roc {

__device__ __forceinline__ void wave_sync()
{
    // same-wave LDS hand-off (one lane writes what other lanes of the wave read): the hardware runs a wave's LDS operations in
    // order; this only keeps the compiler from moving them across the point or into divergent branches
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// key = (bits(score + 0.0f) << 1) | (mask != 0); the precondition bits of the element are OR-ed into st
__device__ __forceinline__ uint32_t make_key(float s, float m, uint32_t &st)
{
    if (s != s) st |= ANODDPM_ROC_NAN;
    else if (s == INFINITY || s == -INFINITY) st |= ANODDPM_ROC_INF;
    if (s < 0.0f) st |= ANODDPM_ROC_NEGATIVE;
    if (!(m == 0.0f || m == 1.0f)) st |= ANODDPM_ROC_BAD_MASK;
    return (__float_as_uint(s + 0.0f) << 1) | (m != 0.0f ? 1u : 0u);     // -0.0 + 0.0 = +0.0
}

// the valid lanes of this 64-lane group whose digit is dg (eight ballots); wave-uniform call
__device__ __forceinline__ uint64_t digit_peers(uint32_t dg, bool valid)
{
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (dg >> b) & 1u;
        const uint64_t bal = __ballot(valid && bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// exclusive prefix of v over a workgroup of NW waves in thread order (two barriers; wsum: NW words of LDS); total: the sum of all
template <int NW>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wsum, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
    for (int w = 0; w < NW; ++w) {
        const uint32_t t = wsum[w];
        if (w < wave) base += t;
        total += t;
    }
    __syncthreads();
    return base + incl - v;
}

// sum of the per-wave totals below `wave`, and of all of them
template <int NW>
__device__ __forceinline__ void wave_carry(const uint32_t *wtot, int wave, uint32_t &below, uint32_t &total)
{
    below = 0;
    total = 0;
    for (int w = 0; w < NW; ++w) {
        const uint32_t t = wtot[w];
        if (w < wave) below += t;
        total += t;
    }
}

// run r (ascending score) of the compacted run list: does sklearn's drop_intermediate keep its curve point?
__device__ __forceinline__ bool keep_point(const uint32_t *runpos, const uint32_t *runtp, uint32_t r, uint32_t R)
{
    if (r == 0 || r == R - 1) return true;                       // last / first point of the curve
    const uint32_t rsm = runpos[r - 1], rs = runpos[r], rs1 = runpos[r + 1];
    const uint32_t tpm = runtp[r - 1], tp = runtp[r], tp1 = runtp[r + 1];
    // second difference at this point = counts of the next lower run minus the counts of this run
    return (tp1 - tp) != (tp - tpm) || (rs1 - rs) != (rs - rsm);
}

// candidate (tps, cnt, r) of the best Dice: is a better than b?  den = cnt + P
__device__ __forceinline__ bool dice_better(uint32_t tpa, uint32_t ca, uint32_t ra, uint32_t tpb, uint32_t cb, uint32_t rb, uint32_t P)
{
    const unsigned long long x = (unsigned long long)tpa * ((unsigned long long)cb + P);
    const unsigned long long y = (unsigned long long)tpb * ((unsigned long long)ca + P);
    return x > y || (x == y && ra > rb);
}

// halving tree over the WIDTH lowest lanes of a wave (WIDTH = 64: the partials of a wave; WIDTH = 16: the wave sums of a
// workgroup): lane 0 ends with ((v0 + v[W/2]) + (v[W/4] + v[3W/4])) + ...  The order is part of the result's bits.
template <int WIDTH>
__device__ __forceinline__ double tree_add(double part)
{
#pragma unroll
    for (int off = WIDTH / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
    return part;
}

// the same tree for the best-Dice candidate; its order is total, so the shape does not matter
template <int WIDTH>
__device__ __forceinline__ void tree_dice(uint32_t &btp, uint32_t &bc, uint32_t &br, uint32_t P)
{
#pragma unroll
    for (int off = WIDTH / 2; off > 0; off >>= 1) {
        const uint32_t otp = __shfl_xor(btp, off), oc = __shfl_xor(bc, off), orr = __shfl_xor(br, off);
        if (dice_better(otp, oc, orr, btp, bc, br, P)) { btp = otp; bc = oc; br = orr; }
    }
}

}  // namespace roc
}  // namespace anoddpm
