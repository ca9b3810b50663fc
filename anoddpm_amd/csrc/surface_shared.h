// The pieces of the exact Euclidean distance transform and of the boundary statistics, stated once for the planes of
// csrc/surface.hip and the volumes of csrc/surface3d.hip (each file's head comment has the decomposition it builds from them):
//   column_kernel            a sweep down and a sweep up every column of a [rows][columns] view: g^2 per element
//   nearest / stage_row      min over x' of (x - x')^2 + row[x'], walking outwards while k^2 can still win; the row in LDS when it fits
//   dt_row_kernel            that search over every row of a g^2 buffer, into the transform's outputs
//   block_select / percentile95 / write_percentiles   the order statistics of the header's percentile, on integer squared distances
//   fold_pair / finish_pair  the two halving trees (64 lanes of a wave, then the 16 wave sums) and the words a pair's workgroup writes
// Nothing here knows how many dimensions the elements are laid out in.  Every kernel lives in an unnamed namespace: each file that
// includes this header compiles its own copy.  Compiled with -ffp-contract=off.
#pragma once
#include <math.h>
#include "common.h"

namespace {

constexpr int THREADS = 256, STAT_THREADS = 1024, STAT_WAVES = STAT_THREADS / 64, ROW_LDS = 4096, CHUNK = 8;
constexpr uint32_t FAR = 0x7fffffffu;                                // "no zero in reach"; every real squared distance is below it

// ---------------------------------------------------------------------------------------------------- column sweeps
// `planes` planes of H rows and W columns.  src != nullptr: the zero set is !(src > level) (NaN is not above any level); else the
// zeros already stored in g2.  A volume [D][H][W] handed over as D rows of H * W columns is swept along z.
__global__ __launch_bounds__(THREADS) void column_kernel(const float *__restrict__ src, int64_t src_stride, float level,
                                                         uint32_t *g2, int planes, int H, int W)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (int64_t)planes * W) return;
    const int q = (int)(i / W), x = (int)(i - (int64_t)q * W);
    uint32_t *col = g2 + (int64_t)q * H * W + x;
    const float *in = src ? src + (int64_t)q * src_stride + x : nullptr;
    uint32_t d = FAR;
    for (int y0 = 0; y0 < H; y0 += CHUNK) {
        bool zero[CHUNK];
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            const int y = y0 + j;
            zero[j] = y < H && (in ? !(in[(int64_t)y * W] > level) : col[(int64_t)y * W] == 0u);
        }
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            const int y = y0 + j;
            if (y < H) {
                d = zero[j] ? 0u : (d == FAR ? FAR : d + 1u);
                col[(int64_t)y * W] = d;
            }
        }
    }
    d = FAR;
    for (int y0 = H - 1; y0 >= 0; y0 -= CHUNK) {
        uint32_t t[CHUNK];
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            const int y = y0 - j;
            t[j] = y >= 0 ? col[(int64_t)y * W] : FAR;
        }
#pragma unroll
        for (int j = 0; j < CHUNK; ++j) {
            const int y = y0 - j;
            if (y >= 0) {
                d = t[j] == 0u ? 0u : (d == FAR ? FAR : d + 1u);
                const uint32_t m = min(t[j], d);                     // <= H - 1 or FAR
                col[(int64_t)y * W] = m == FAR ? FAR : m * m;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the search along one axis
// min over x' of (x - x')^2 + row[x' * stride], walking outwards from x while k^2 can still win: the bound holds for any
// non-negative row[].  k^2 < best <= FAR and row[] <= FAR: the sum stays below 2^32, and k^2 + FAR never wins.
__device__ __forceinline__ uint32_t nearest(const uint32_t *row, int x, int W, int64_t stride = 1)
{
    uint32_t best = row[x * stride];
    for (int k = 1; (uint32_t)k * (uint32_t)k < best; ++k) {         // k <= W <= 46341: k^2 fits 32 bits unsigned
        const int l = x - k, r = x + k;
        if (l < 0 && r >= W) break;
        const uint32_t kk = (uint32_t)k * (uint32_t)k;
        if (l >= 0) best = min(best, kk + row[l * stride]);
        if (r < W) best = min(best, kk + row[r * stride]);
    }
    return best;
}

// the row of g^2 a workgroup searches: in LDS when it fits
__device__ __forceinline__ const uint32_t *stage_row(const uint32_t *__restrict__ grow, uint32_t *tile, int W)
{
    if (W > ROW_LDS) return grow;                                    // block-uniform
    for (int x = threadIdx.x; x < W; x += THREADS) tile[x] = grow[x];
    __syncthreads();
    return tile;
}

// blockIdx.x = one row of W elements of g2 and of the outputs ([S][H][W], or [S][D][H][W] seen as S * D * H rows); of `a` only
// W, sq and dist are read
__global__ __launch_bounds__(THREADS) void dt_row_kernel(anoddpm_distance_args a, const uint32_t *__restrict__ g2)
{
    __shared__ uint32_t tile[ROW_LDS];
    const int W = a.W;
    const int64_t base = (int64_t)blockIdx.x * W;
    const uint32_t *row = stage_row(g2 + base, tile, W);
    for (int x = threadIdx.x; x < W; x += THREADS) {
        const uint32_t r = nearest(row, x, W);
        a.sq[base + x] = r >= FAR ? -1 : (int32_t)r;
        if (a.dist) a.dist[base + x] = r >= FAR ? (double)INFINITY : sqrt((double)r);
    }
}

// ---------------------------------------------------------------------------------------------------- per-pair statistics
// The value of rank `rank` (0-based, ascending) among the words v[0 ... n), all below 2^31: radix select from the top byte down.
__device__ uint32_t block_select(const uint32_t *v, uint32_t n, uint32_t rank, uint32_t *hist, uint32_t *sel)
{
    const int tid = threadIdx.x;
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < 256; i += STAT_THREADS) hist[i] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += STAT_THREADS) {
            const uint32_t w = v[i];
            if ((w & mask) == prefix) atomicAdd(&hist[(w >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t b = 0, r = rank;
            while (b < 255u && r >= hist[b]) { r -= hist[b]; ++b; }
            sel[0] = b;
            sel[1] = r;
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        rank = sel[1];
        mask |= 255u << shift;
        __syncthreads();
    }
    return prefix;
}

// the percentile of include/anoddpm_hip.h over the n squared distances v[0 ... n)
__device__ double percentile95(const uint32_t *v, uint32_t n, uint32_t *hist, uint32_t *sel)
{
    const unsigned long long k = 19ull * (n - 1u);
    const uint32_t lo = (uint32_t)(k / 20ull), r = (uint32_t)(k % 20ull), hi = min(lo + 1u, n - 1u);
    const uint32_t va = block_select(v, n, lo, hist, sel);
    const uint32_t vb = hi == lo ? va : block_select(v, n, hi, hist, sel);
    const double a = sqrt((double)va), b = sqrt((double)vb);
    return a + (b - a) * ((double)r / 20.0);
}

// p95[0 ... 3) of a pair whose squared distances lie packed, direction 1 (n1 words) directly behind direction 0 (n0 words): the
// pooled multiset is one array.  The whole workgroup calls it.
__device__ __forceinline__ void write_percentiles(const uint32_t *packed, uint32_t n0, uint32_t n1, double *p95, uint32_t *hist, uint32_t *sel)
{
    const double p0 = percentile95(packed, n0, hist, sel);
    const double p1 = percentile95(packed + n0, n1, hist, sel);
    const double pp = percentile95(packed, n0 + n1, hist, sel);
    if (threadIdx.x == 0) {
        p95[0] = p0;
        p95[1] = p1;
        p95[2] = pp;
    }
}

struct PairFold {                                                    // the LDS words of fold_pair
    uint32_t wcnt[2][STAT_WAVES];
    int32_t wmax[2][STAT_WAVES];
    double wsum[2][STAT_WAVES];
};

// The partial count, maximum and fp64 sum of every thread of a STAT_THREADS workgroup, per direction, folded by two halving
// trees: the 64 partials of each wave (lane i + lane i + 32, then + 16, ... + 1), then the 16 wave sums the same way.  Afterwards
// lane 0 of wave 0 holds the totals.  Ends with the workgroup past a barrier only for wave 0's reads: callers synchronise again
// before they reuse `f`.
__device__ __forceinline__ void fold_pair(uint32_t (&cnt)[2], int32_t (&mx)[2], double (&sum)[2], PairFold &f)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cnt[d] += __shfl_xor(cnt[d], off);
            mx[d] = max(mx[d], __shfl_xor(mx[d], off));
            sum[d] += __shfl_xor(sum[d], off);
        }
        if (lane == 0) { f.wcnt[d][wave] = cnt[d]; f.wmax[d][wave] = mx[d]; f.wsum[d][wave] = sum[d]; }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            cnt[d] = lane < STAT_WAVES ? f.wcnt[d][lane] : 0u;
            mx[d] = lane < STAT_WAVES ? f.wmax[d][lane] : -1;
            sum[d] = lane < STAT_WAVES ? f.wsum[d][lane] : 0.0;
#pragma unroll
            for (int off = STAT_WAVES / 2; off > 0; off >>= 1) {
                cnt[d] += __shfl_xor(cnt[d], off);
                mx[d] = max(mx[d], __shfl_xor(mx[d], off));
                sum[d] += __shfl_xor(sum[d], off);
            }
        }
    }
}

// What ONE thread writes for pair s from the folded totals: status, counts, max2, mean, and the NaN percentiles of a pair with an
// empty border.  s_n[d] = the number of squared distances of direction d the percentiles select from (0, 0 when the status is set).
__device__ __forceinline__ void finish_pair(int s, const uint32_t (&cnt)[2], const int32_t (&mx)[2], const double (&sum)[2],
                                            int32_t *counts, int32_t *max2, double *mean, double *p95, int32_t *status, uint32_t *s_n)
{
    const int st = (cnt[0] == 0 ? ANODDPM_SURFACE_EMPTY_PRED : 0) | (cnt[1] == 0 ? ANODDPM_SURFACE_EMPTY_REF : 0);
    status[s] = st;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        counts[(int64_t)s * 2 + d] = (int32_t)cnt[d];
        max2[(int64_t)s * 2 + d] = st ? -1 : mx[d];
        mean[(int64_t)s * 2 + d] = st ? (double)NAN : sum[d] / (double)cnt[d];
        s_n[d] = st ? 0u : cnt[d];
    }
    if (st) p95[(int64_t)s * 3] = p95[(int64_t)s * 3 + 1] = p95[(int64_t)s * 3 + 2] = (double)NAN;
}

}  // namespace
