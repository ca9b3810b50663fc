// GroupNorm(32) statistics: how per-channel {sum, sum of squares} are gathered into a statistics row and how they are finished
// into mean / rstd and the per-channel scale / shift, stated once for every kernel that does either (UNet.py:409-411:
// nn.GroupNorm(32, C), eps 1e-5, biased variance).
//
// There are TWO finishes, on purpose:
//   - the exact one (gn_moments / gn_affine below): mean = S / n, var = Q / n - mean^2, rstd = 1 / sqrt(var + eps), every step an
//     IEEE fp64 operation.  The finalize launches, the split-K tail and the prologues of the small-map kernels use it: it runs once
//     per launch or in a 32-thread phase nobody waits for long, and their results are the reference the tests compare with.
//   - the fast one (fold_affine_finish of gn_fold.h): S * (1 / n) and v_rsq_f64 + two Newton steps.  It sits in the prologue of
//     EVERY F(4x4,3x3) workgroup, redundantly in all threads of a group, where two fp64 divisions and a square root per thread
//     would be on the critical path.  It agrees with the exact one to an ulp or two of fp64, not bit for bit -- so the two are not
//     interchangeable under a plan whose outputs are compared bitwise, and their arithmetic stays separate.
#pragma once
#include "common.h"
#include "gn_fold.h"

namespace anoddpm {

// A kernel argument as a scalar VALUE.  `lane_cond ? a.x : a.y` on two fields of the argument struct is otherwise compiled as a select
// of the fields' ADDRESSES and a global_load from the kernarg segment, followed by s_waitcnt vmcnt(0): vmcnt retires in order, so that
// wait drains every operand request in flight (profiles/r7_small_kernel_waits.txt).
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <typename T>
__device__ __forceinline__ const T *uniform(const T *p)
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32));
    return reinterpret_cast<const T *>(((uint64_t)hi << 32) | lo);
}

// ---- the exact finish ----------------------------------------------------------------------------------------------------------
// Group moments from the group's {sum, sum of squares} over n = pixels * channels-per-group values.
__device__ __forceinline__ void gn_moments(double S, double Q, double n, float eps, double *mean_out, double *rstd_out)
{
    const double mean = S / n;
    double var = Q / n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    *mean_out = mean;
    *rstd_out = 1.0 / sqrt(var + (double)eps);
}

// x * scale + shift == (x - mean) * rstd * gamma + beta
__device__ __forceinline__ void gn_affine(double mean, double rstd, float gamma, float beta, float *scale, float *shift)
{
    const double sc = rstd * (double)gamma;
    *scale = (float)sc;
    *shift = (float)((double)beta - mean * sc);
}

// ---- finish in a consumer's prologue (small-map kernels) -----------------------------------------------------------------------
// The statistics sources of a (virtual concat) operand as scalar values: see uniform().
struct GnSources {
    const float *st0, *st1;
    int c0, c1, fmt0, fmt1, rows0, rows1;
};

__device__ __forceinline__ GnSources gn_sources(const anoddpm_igemm_args &a)
{
    return GnSources{uniform(a.fold_stats0), uniform(a.fold_stats1), uniform(a.c0),         uniform(a.c1),
                     uniform(a.fold_fmt0),   uniform(a.fold_fmt1),   uniform(a.fold_rows0), uniform(a.fold_rows1)};
}

// fp64 {sum, sumsq} of channel c of image b.  fmt 1: one fp64 row [B][cw][2] (a split-K tail's tail_csum).  fmt 0: fp32 rows
// [B][rows][cw][2] as the producers' epilogues write them, summed in row order.
__device__ __forceinline__ void gn_source_sums(const GnSources &g, int b, int c, double *s_out, double *q_out)
{
    const bool first = c < g.c0;
    const int cl = first ? c : c - g.c0, cw = first ? g.c0 : g.c1;
    const int fmt = first ? g.fmt0 : g.fmt1, rows = first ? g.rows0 : g.rows1;
    const float *st = first ? g.st0 : g.st1;
    double s = 0.0, qq = 0.0;
    if (fmt) {
        const double *sd = reinterpret_cast<const double *>(st) + ((int64_t)b * cw + cl) * 2;
        s = sd[0]; qq = sd[1];
    } else {
        const float *sr = st + ((int64_t)b * rows * cw + cl) * 2;
        for (int r0 = 0; r0 < rows; r0 += 4) {           // four independent row loads in flight; summed in row order
            float2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = r0 + u < rows ? r0 + u : rows - 1;
                v[u] = *reinterpret_cast<const float2 *>(sr + (int64_t)r * cw * 2);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r0 + u < rows) { s += (double)v[u].x; qq += (double)v[u].y; }
        }
    }
    *s_out = s; *q_out = qq;
}

// The operand's affine table aff_sc / aff_sh [Kfill] finished from the producers' statistics (a.fold_*) by the NT threads of a
// workgroup; entries K..Kfill are zero.  K <= 2 * NT.  n_pixels = pixels of the normalised tensor (the SOURCE resolution for a
// nearest-x2 operand).  csum [2 * K] and gst [2 * groups] are fp64 scratch nobody else touches before this returns.  Three barriers;
// the table is published when it returns.
template <int NT>
__device__ __forceinline__ void gn_fold_prologue(const anoddpm_igemm_args &a, int b, int tid, int K, int Kfill, int n_pixels, double *csum,
                                                 double *gst, float *aff_sc, float *aff_sh)
{
    const int groups = a.fold_groups, cpg = K / groups;
    const GnSources src = gn_sources(a);
    // gamma / beta of this thread's channels (at most two) ride with the statistics requests; they are used two barriers later,
    // by the same thread for the same channels
    float fgam[2], fbet[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + i * NT;
        fgam[i] = a.fold_gamma[c < K ? c : 0];
        fbet[i] = a.fold_beta[c < K ? c : 0];
    }
    for (int c = tid; c < K; c += NT) gn_source_sums(src, b, c, &csum[2 * c], &csum[2 * c + 1]);
    __syncthreads();
    if (tid < groups) {
        double S = 0.0, Q = 0.0;
        for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { S += csum[2 * c]; Q += csum[2 * c + 1]; }   // channel order
        gn_moments(S, Q, (double)n_pixels * cpg, a.fold_eps, &gst[2 * tid], &gst[2 * tid + 1]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + i * NT;
        if (c < Kfill) {
            float scv = 0.f, shv = 0.f;
            if (c < K) {
                const int g = c / cpg;
                gn_affine(gst[2 * g], gst[2 * g + 1], fgam[i], fbet[i], &scv, &shv);
            }
            aff_sc[c] = scv; aff_sh[c] = shv;
        }
    }
    __syncthreads();
}

// The same table copied from a finalize launch's scale / shift (a.gn_scale / a.gn_shift).  One barrier.
template <int NT>
__device__ __forceinline__ void gn_affine_table_copy(const anoddpm_igemm_args &a, int b, int tid, int K, int Kfill, float *aff_sc, float *aff_sh)
{
    for (int c = tid; c < Kfill; c += NT) {
        aff_sc[c] = c < K ? a.gn_scale[(int64_t)b * a.gn_ld + c] : 0.f;
        aff_sh[c] = c < K ? a.gn_shift[(int64_t)b * a.gn_ld + c] : 0.f;
    }
    __syncthreads();
}

// Launcher side of gn_fold_prologue.  `what` = the kernel's name in the error text.
static inline int check_fold_args(const anoddpm_igemm_args *a, int K, const char *what)
{
    if (!a->fold_gamma) return ANODDPM_OK;
    ANODDPM_REQUIRE(a->fold_beta && a->fold_stats0 && (a->c1 == 0 || a->fold_stats1), "%s: GroupNorm fold: null pointer", what);
    ANODDPM_REQUIRE(a->fold_groups >= 1 && a->fold_groups <= 64 && K % a->fold_groups == 0, "%s: GroupNorm fold: bad group count", what);
    ANODDPM_REQUIRE((a->fold_fmt0 != 0 || a->fold_rows0 >= 1) && (a->c1 == 0 || a->fold_fmt1 != 0 || a->fold_rows1 >= 1),
                    "%s: GroupNorm fold: statistics rows missing", what);
    return ANODDPM_OK;
}

// ---- producing a statistics row ------------------------------------------------------------------------------------------------
// One block of 256 threads owns a slab of the P pixels of one image and ALL C channels (C % 4 == 0) and writes one row
// `row` [C][2] of per-channel fp32 {sum, sumsq} of the values it visits.  Thread = (pixel row tr, channel quad tq): TQ =
// min(C / 4, 256) quads side by side, R = 256 / TQ pixel rows, ceil(C / 4 / TQ) passes over the channels.  Per-thread quads go
// through LDS and are summed per column in the fixed order r = 0..R-1 (deterministic, no atomics).  quad_fn(channel quad) returns
// the thread's pixel_fn for that quad (whatever does not depend on the pixel is computed once there); pixel_fn(pixel) returns the
// four values of that pixel -- a plain load, or a split-K tail that also stores them.
template <typename QuadFn>
__device__ __forceinline__ void slab_column_sums(int C, int P, int nslab, int slab, float *row, QuadFn quad_fn)
{
    __shared__ float lds_s[256 * 4];
    __shared__ float lds_q[256 * 4];
    const int C4 = C >> 2;
    const int TQ = C4 < 256 ? C4 : 256;
    const int R = 256 / TQ;
    const int npass = (C4 + TQ - 1) / TQ;
    const int tid = threadIdx.x;
    const int tq = tid % TQ, tr = tid / TQ;
    const int sp = (P + nslab - 1) / nslab;
    const int p0 = slab * sp;
    const int p1 = (p0 + sp < P) ? p0 + sp : P;
    for (int pass = 0; pass < npass; ++pass) {
        const int quad = pass * TQ + tq;
        gf_f32x4 cs = {0.f, 0.f, 0.f, 0.f}, cq = {0.f, 0.f, 0.f, 0.f};
        if (tr < R && quad < C4) {
            auto pixel_fn = quad_fn(quad);
            for (int p = p0 + tr; p < p1; p += R) {
                const gf_f32x4 v = pixel_fn(p);
                cs += v;
                cq += v * v;
            }
        }
        if (tr < R) {
            const int o = (tr * TQ + tq) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) { lds_s[o + e] = cs[e]; lds_q[o + e] = cq[e]; }
        }
        __syncthreads();
        for (int cl = tid; cl < TQ * 4; cl += 256) {
            const int c = pass * TQ * 4 + cl;
            if (c < C) {
                float s = 0.f, q = 0.f;
                for (int r = 0; r < R; ++r) { s += lds_s[r * TQ * 4 + cl]; q += lds_q[r * TQ * 4 + cl]; }
                row[c * 2] = s;
                row[c * 2 + 1] = q;
            }
        }
        __syncthreads();
    }
}

}  // namespace anoddpm
