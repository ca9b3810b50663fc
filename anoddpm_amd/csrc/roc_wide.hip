// ROC / PR scores of ONE long segment spread over the whole chip -- what csrc/roc.hip computes with one workgroup per segment,
// here as a sequence of launches with one workgroup per tile of `tile` keys (detection.py:538-643 roc_data: one curve pooled over
// the whole test set).  A launch boundary is the only ordering between workgroups: no kernel below waits for another workgroup,
// and none reads, within a launch, what another workgroup wrote in that launch.  Every loop is bounded by n or by the tile count.
//   keys        key as roc.hip (roc_shared.h), the tile's precondition bits, and the tile histogram of the first pass
//   4 x         scan, scatter (its key-only instantiation), hist of the next pass's digit: the sort pass of wide_shared.h
//   run_count   per tile: run starts (a tile's first key compares against the previous tile's last key) and positives
//   run_write   per tile: its carry is the sum of the counts of the tiles below; runpos / runtp compacted, with the sentinel
//   run_terms   per tile of runs, from the highest score down: its part of twoU (uint64), its number of kept curve points, its
//               best-Dice candidate, and the average-precision terms into an fp64 array
//   curve_write per tile of runs: the kept points, compactly, from the carry of the tiles above       (only with curve outputs)
//   lanes       16 workgroups, one per wave of roc.hip's step 6 (wide_shared.h): virtual lane t of 1024 adds the terms t,
//               t + 1024, ... in that order, then the 64-lane tree                                                (only with ap)
//   finish      one workgroup: folds the per-tile integers, the 16-wave tree, writes the outputs of the segment
// 16 launches per segment without curve and ap, 18 with both.  Every output has the bits anoddpm_roc_auc writes.
// Compiled with -ffp-contract=off.  There is no floating-point atomic in this file.
#include "common.h"
#include "roc_shared.h"
#include "wide_shared.h"

namespace {

using namespace anoddpm::roc;
using namespace anoddpm::wide;                                   // geometry, hist / scan / scatter<payload> and lanes: shared with pro_wide.hip

enum { H_SKIP = 0, H_R = 4, H_P = 5, H_WORDS = 64 };

struct wide_ws {                 // one segment's workspace
    double *terms;               // [W] average-precision term of run r
    unsigned long long *tile_u;  // [Tp]
    double *wavesum;             // [16]
    uint32_t *buf0, *buf1, *buf2;        // [W] each: keys ping / pong; then sorted keys, runpos, runtp
    uint32_t *table;             // [256][T]
    uint32_t *tile_b, *tile_p, *tile_k, *tile_st, *tile_best;   // [Tp], tile_best [3][Tp]
    uint32_t *hdr;               // H_WORDS
};

int64_t seg_words_of(int64_t n) { return (n + 1 + 63) / 64 * 64; }

int64_t carve(wide_ws *w, void *base, int64_t n, int64_t Ta)
{
    const int64_t W = seg_words_of(n), Tp = (Ta + 3) / 4 * 4;
    char *p = static_cast<char *>(base);
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *q = p ? p + o : nullptr; o += (bytes + 15) / 16 * 16; return q; };
    w->terms = (double *)take(W * 8);
    w->tile_u = (unsigned long long *)take(Tp * 8);
    w->wavesum = (double *)take(AP_WAVES * 8);
    w->buf0 = (uint32_t *)take(W * 4);
    w->buf1 = (uint32_t *)take(W * 4);
    w->buf2 = (uint32_t *)take(W * 4);
    w->table = (uint32_t *)take(RADIX * Tp * 4);
    w->tile_b = (uint32_t *)take(Tp * 4);
    w->tile_p = (uint32_t *)take(Tp * 4);
    w->tile_k = (uint32_t *)take(Tp * 4);
    w->tile_st = (uint32_t *)take(Tp * 4);
    w->tile_best = (uint32_t *)take(3 * Tp * 4);
    w->hdr = (uint32_t *)take(H_WORDS * 4);
    return o;
}

// ------------------------------------------------------------------------------------------------ sort
__global__ __launch_bounds__(WT) void keys_kernel(const float *__restrict__ score, const float *__restrict__ mask, wide_ws w, wide_geom g)
{
    __shared__ uint32_t hist[RADIX];
    __shared__ uint32_t s_status;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    hist[tid] = 0;
    if (tid == 0) s_status = 0;
    __syncthreads();
    const uint32_t i0 = b * g.tile, i1 = min(i0 + g.tile, g.n);
    uint32_t st = 0;
    for (uint32_t i = i0 + tid; i < i1; i += WT) {
        const uint32_t key = make_key(score[i], mask[i], st);
        w.buf0[i] = key;
        atomicAdd(&hist[key & 255u], 1u);
    }
    if (st) atomicOr(&s_status, st);
    __syncthreads();
    w.table[tid * g.T + b] = hist[tid];                          // digit-major
    if (tid == 0) w.tile_st[b] = s_status;
}

// ------------------------------------------------------------------------------------------------ runs
// sum of cnt[t] over the tiles t < b, and over all T tiles (s2: two words of LDS; three barriers)
__device__ __forceinline__ void tile_carry(const uint32_t *__restrict__ cnt, uint32_t T, uint32_t b, uint32_t *s2, uint32_t &below, uint32_t &total)
{
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { s2[0] = 0; s2[1] = 0; }
    __syncthreads();
    uint32_t lo = 0, all = 0;
    for (uint32_t t = tid; t < T; t += WT) {
        const uint32_t v = cnt[t];
        all += v;
        if (t < b) lo += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo += __shfl_xor(lo, off);
        all += __shfl_xor(all, off);
    }
    if ((tid & 63) == 0) { atomicAdd(&s2[0], lo); atomicAdd(&s2[1], all); }
    __syncthreads();
    below = s2[0];
    total = s2[1];
    __syncthreads();
}

__global__ __launch_bounds__(WT) void run_count_kernel(const uint32_t *__restrict__ key, wide_ws w, wide_geom g)
{
    __shared__ uint32_t s2[2];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) { s2[0] = 0; s2[1] = 0; }
    __syncthreads();
    const uint32_t i0 = b * g.tile, i1 = min(i0 + g.tile, g.n);
    uint32_t cp = 0, cb = 0;
    for (uint32_t i = i0 + tid; i < i1; i += WT) {
        const uint32_t k = key[i], kp = i > 0 ? key[i - 1] : 0u;   // i - 1 may lie in the previous tile
        cp += k & 1u;
        cb += (i == 0 || (k >> 1) != (kp >> 1)) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cp += __shfl_xor(cp, off);
        cb += __shfl_xor(cb, off);
    }
    if ((tid & 63) == 0) { atomicAdd(&s2[0], cb); atomicAdd(&s2[1], cp); }
    __syncthreads();
    if (tid == 0) { w.tile_b[b] = s2[0]; w.tile_p[b] = s2[1]; }
}

__global__ __launch_bounds__(WT) void run_write_kernel(const uint32_t *__restrict__ key, uint32_t *__restrict__ runpos, uint32_t *__restrict__ runtp,
                                                       wide_ws w, wide_geom g)
{
    __shared__ uint32_t s2[2], wtot_p[WW], wtot_b[WW];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = g.n;
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t tile_cb, tile_cp, R, P;
    tile_carry(w.tile_b, g.T, b, s2, tile_cb, R);
    tile_carry(w.tile_p, g.T, b, s2, tile_cp, P);
    const uint32_t i0 = b * g.tile, i1 = min(i0 + g.tile, n);
    const uint32_t chunk = g.tile / WW;
    const uint32_t c0 = min(i0 + wave * chunk, i1), c1 = min(c0 + chunk, i1);
    uint32_t cp = 0, cb = 0;
    for (uint32_t base = c0; base < c1; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < c1;
        const uint32_t k = valid ? key[i] : 0u, kp = (valid && i > 0) ? key[i - 1] : 0u;
        cp += __popcll(__ballot(valid && (k & 1u)));
        cb += __popcll(__ballot(valid && (i == 0 || (k >> 1) != (kp >> 1))));
    }
    if (lane == 0) { wtot_p[wave] = cp; wtot_b[wave] = cb; }
    __syncthreads();
    uint32_t carry_p, carry_b, tp_, tb_;
    wave_carry<WW>(wtot_p, wave, carry_p, tp_);
    wave_carry<WW>(wtot_b, wave, carry_b, tb_);
    carry_p += tile_cp;
    carry_b += tile_cb;
    for (uint32_t base = c0; base < c1; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < c1;
        const uint32_t k = valid ? key[i] : 0u, kp = (valid && i > 0) ? key[i - 1] : 0u;
        const bool bnd = valid && (i == 0 || (k >> 1) != (kp >> 1));
        const uint64_t bp = __ballot(valid && (k & 1u)), bb = __ballot(bnd);
        if (bnd) {
            const uint32_t r = carry_b + __popcll(bb & lt);
            if (r < n) {                                         // r < R <= n always; the guard keeps a bad carry inside the buffer
                runpos[r] = i;
                runtp[r] = carry_p + __popcll(bp & lt);
            }
        }
        carry_p += __popcll(bp);
        carry_b += __popcll(bb);
    }
    if (b == g.T - 1 && tid == 0) {
        if (R <= n) { runpos[R] = n; runtp[R] = P; }             // sentinel: the end of the last run (the buffers hold n + 1 words)
        w.hdr[H_R] = R;
        w.hdr[H_P] = P;
    }
}

// ------------------------------------------------------------------------------------------------ per run
struct wide_want { int curve, all, ap, best; };

__global__ __launch_bounds__(WT) void run_terms_kernel(const uint32_t *__restrict__ runpos, const uint32_t *__restrict__ runtp, wide_ws w, wide_geom g,
                                                       wide_want want)
{
    __shared__ unsigned long long wacc[WW];
    __shared__ uint32_t wk[WW], wbt[WW], wbc[WW], wbr[WW];
    const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = g.n;
    const uint32_t R = min(w.hdr[H_R], n), P = w.hdr[H_P];
    const uint32_t q0 = min(j * g.tile, R), q1 = min(q0 + g.tile, R);    // j * tile < n: no overflow
    const double dP = (double)P;
    unsigned long long acc = 0;
    uint32_t ck = 0, btp = 0, bc = 1, br = 0;                    // the candidate that loses against every run (roc.hip step 6)
    for (uint32_t q = q0 + tid; q < q1; q += WT) {
        const uint32_t r = R - 1 - q;
        const uint32_t rs = runpos[r], tp = runtp[r];
        const uint32_t pr = runtp[r + 1] - tp, nr = (runpos[r + 1] - rs) - pr;
        acc += (unsigned long long)pr * (2ull * (rs - tp) + nr);
        if (want.curve && (want.all || keep_point(runpos, runtp, r, R))) ++ck;
        const uint32_t tps = P - tp, cnt = n - rs;
        if (want.ap) w.terms[r] = pr != 0 ? ((double)pr / dP) * ((double)tps / (double)cnt) : 0.0;
        if (want.best && dice_better(tps, cnt, r, btp, bc, br, P)) { btp = tps; bc = cnt; br = r; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off);
        ck += __shfl_xor(ck, off);
    }
    tree_dice<64>(btp, bc, br, P);
    if (lane == 0) { wacc[wave] = acc; wk[wave] = ck; wbt[wave] = btp; wbc[wave] = bc; wbr[wave] = br; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < WW; ++k) {
            acc += wacc[k];
            ck += wk[k];
            if (dice_better(wbt[k], wbc[k], wbr[k], btp, bc, br, P)) { btp = wbt[k]; bc = wbc[k]; br = wbr[k]; }
        }
        const uint32_t Tp = (g.T + 3u) & ~3u;
        w.tile_u[j] = acc;
        w.tile_k[j] = ck;
        w.tile_best[j] = btp;
        w.tile_best[Tp + j] = bc;
        w.tile_best[2 * Tp + j] = br;
    }
}

struct wide_curve { int32_t *fps, *tps; float *thr; int64_t cap; };

__global__ __launch_bounds__(WT) void curve_write_kernel(const uint32_t *__restrict__ key, const uint32_t *__restrict__ runpos, const uint32_t *__restrict__ runtp,
                                                         wide_ws w, wide_geom g, wide_want want, wide_curve c)
{
    __shared__ uint32_t s2[2], wtot[WW];
    const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = g.n;
    const uint64_t lt = (1ull << lane) - 1ull;
    const uint32_t R = min(w.hdr[H_R], n), P = w.hdr[H_P];
    uint32_t tile_k, K;
    tile_carry(w.tile_k, g.T, j, s2, tile_k, K);
    const uint32_t t0 = min(j * g.tile, R), t1 = min(t0 + g.tile, R);
    const uint32_t chunk = g.tile / WW;
    const uint32_t q0 = min(t0 + wave * chunk, t1), q1 = min(q0 + chunk, t1);
    uint32_t ck = 0;
    for (uint32_t base = q0; base < q1; base += 64) {
        const uint32_t q = base + lane;
        const bool keep = q < q1 && (want.all || keep_point(runpos, runtp, R - 1 - q, R));
        ck += __popcll(__ballot(keep));
    }
    if (lane == 0) wtot[wave] = ck;
    __syncthreads();
    uint32_t carry_k, tk_;
    wave_carry<WW>(wtot, wave, carry_k, tk_);
    carry_k += tile_k;
    for (uint32_t base = q0; base < q1; base += 64) {
        const uint32_t q = base + lane;
        const bool valid = q < q1;
        uint32_t rs = 0, tp = 0;
        bool keep = false;
        if (valid) {
            const uint32_t r = R - 1 - q;
            rs = runpos[r];
            tp = runtp[r];
            keep = want.all || keep_point(runpos, runtp, r, R);
        }
        const uint64_t bk = __ballot(keep);
        const uint64_t idx = (uint64_t)carry_k + __popcll(bk & lt);
        if (keep && (int64_t)idx < c.cap && rs < n) {
            const uint32_t tps = P - tp;
            c.tps[idx] = (int32_t)tps;
            c.fps[idx] = (int32_t)((n - rs) - tps);
            c.thr[idx] = __uint_as_float(key[rs] >> 1);
        }
        carry_k += __popcll(bk);
    }
}

struct wide_out {                // the outputs of this segment
    double *auc; int64_t *counts; int32_t *status; int32_t *curve_len; int64_t curve_cap;
    double *ap; double *best_dice; float *best_thr; int64_t *best_counts;
};

__global__ __launch_bounds__(WT) void finish_kernel(const uint32_t *__restrict__ key, const uint32_t *__restrict__ runpos, const uint32_t *__restrict__ runtp,
                                                    wide_ws w, wide_geom g, wide_want want, wide_out o)
{
    __shared__ unsigned long long wacc[WW];
    __shared__ uint32_t wk[WW], wst[WW], wbt[WW], wbc[WW], wbr[WW];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = g.n;
    const uint32_t R = min(w.hdr[H_R], n), P = w.hdr[H_P], Tp = (g.T + 3u) & ~3u;
    unsigned long long acc = 0;
    uint32_t K = 0, st = 0, btp = 0, bc = 1, br = 0;
    for (uint32_t t = tid; t < g.T; t += WT) {
        acc += w.tile_u[t];
        K += w.tile_k[t];
        st |= w.tile_st[t];
        const uint32_t otp = w.tile_best[t], oc = w.tile_best[Tp + t], orr = w.tile_best[2 * Tp + t];
        if (want.best && dice_better(otp, oc, orr, btp, bc, br, P)) { btp = otp; bc = oc; br = orr; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off);
        K += __shfl_xor(K, off);
        st |= __shfl_xor(st, off);
    }
    tree_dice<64>(btp, bc, br, P);
    if (lane == 0) { wacc[wave] = acc; wk[wave] = K; wst[wave] = st; wbt[wave] = btp; wbc[wave] = bc; wbr[wave] = br; }
    __syncthreads();
    if (wave != 0) return;
    double part = (want.ap && lane < AP_WAVES) ? w.wavesum[lane] : 0.0;
    part = tree_add<AP_WAVES>(part);
    if (lane != 0) return;
    for (int k = 1; k < WW; ++k) {
        acc += wacc[k];
        K += wk[k];
        st |= wst[k];
        if (dice_better(wbt[k], wbc[k], wbr[k], btp, bc, br, P)) { btp = wbt[k]; bc = wbc[k]; br = wbr[k]; }
    }
    const uint32_t N = n - P;
    o.auc[0] = (P == 0 || N == 0) ? (double)NAN : (double)acc / (2.0 * (double)P * (double)N);
    o.counts[0] = P;
    o.counts[1] = N;
    o.counts[2] = (int64_t)acc;
    o.counts[3] = R;
    o.status[0] = (int32_t)(st | ((want.curve && (int64_t)K > o.curve_cap) ? ANODDPM_ROC_CURVE_TRUNCATED : 0u));
    if (want.curve) o.curve_len[0] = (int32_t)K;
    if (want.ap) o.ap[0] = P == 0 ? (double)NAN : (P == n ? 1.0 : part);
    if (want.best) {
        if (br >= R) br = 0;                                     // R >= 1; keeps a bad candidate inside the run list
        const uint32_t rs = min(runpos[br], n - 1), tps = P - runtp[br], cnt = n - runpos[br];
        o.best_dice[0] = P == 0 ? (double)NAN : (double)(2ull * tps) / (double)((unsigned long long)cnt + P);
        o.best_thr[0] = __uint_as_float(key[rs] >> 1);
        o.best_counts[0] = tps;
        o.best_counts[1] = cnt - tps;
    }
}

}  // namespace

extern "C" int64_t anoddpm_roc_wide_workspace_bytes(int32_t S, int64_t n, int32_t tile)
{
    if (S < 1 || n < 1 || n >= ((int64_t)1 << 31)) return -1;
    int32_t used;
    if (check_tile(n, tile, &used, "roc_wide_workspace_bytes") != ANODDPM_OK) return -1;
    wide_ws w;
    return carve(&w, nullptr, n, alloc_tiles(n, tile));
}

extern "C" int anoddpm_roc_auc_wide(const anoddpm_roc_args *a, int32_t tile, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "roc_auc_wide: null args");
    ANODDPM_REQUIRE(a->score && a->mask && a->workspace && a->auc && a->counts && a->status, "roc_auc_wide: null pointer");
    ANODDPM_REQUIRE(a->S >= 1, "roc_auc_wide: S must be >= 1");
    ANODDPM_REQUIRE(a->n >= 1, "roc_auc_wide: n must be >= 1");
    ANODDPM_REQUIRE(a->n < ((int64_t)1 << 31), "roc_auc_wide: n must be below 2^31 (32-bit positions, uint64 twoU)");
    ANODDPM_REQUIRE(a->S == 1 || a->score_stride >= a->n, "roc_auc_wide: score segments overlap (score_stride < n)");
    ANODDPM_REQUIRE(a->S == 1 || a->mask_stride == 0 || a->mask_stride >= a->n, "roc_auc_wide: mask_stride must be 0 (shared mask) or >= n");
    int32_t used;
    if (int rc = check_tile(a->n, tile, &used, "roc_auc_wide")) return rc;
    ANODDPM_REQUIRE(a->workspace_bytes >= anoddpm_roc_wide_workspace_bytes(a->S, a->n, tile), "roc_auc_wide: workspace too small");
    ANODDPM_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "roc_auc_wide: workspace must be 16-byte aligned");
    const bool any_curve = a->curve_fps || a->curve_tps || a->curve_thr || a->curve_len;
    if (any_curve) {
        ANODDPM_REQUIRE(a->curve_fps && a->curve_tps && a->curve_thr && a->curve_len, "roc_auc_wide: curve output needs curve_fps, curve_tps, curve_thr and curve_len");
        ANODDPM_REQUIRE(a->curve_cap >= 2, "roc_auc_wide: curve capacity must be >= 2 points per segment");
    }
    ANODDPM_REQUIRE(a->curve_mode == ANODDPM_ROC_CURVE_DROP || a->curve_mode == ANODDPM_ROC_CURVE_ALL, "roc_auc_wide: unknown curve_mode");
    ANODDPM_REQUIRE(a->curve_mode == ANODDPM_ROC_CURVE_DROP || any_curve, "roc_auc_wide: curve_mode needs the curve outputs");
    const bool any_best = a->best_dice || a->best_thr || a->best_counts;
    if (any_best) ANODDPM_REQUIRE(a->best_dice && a->best_thr && a->best_counts, "roc_auc_wide: best Dice output needs best_dice, best_thr and best_counts");

    hipStream_t s = as_stream(stream);
    wide_geom g;
    g.n = (uint32_t)a->n;
    g.tile = (uint32_t)used;
    g.T = (uint32_t)((a->n + used - 1) / used);
    wide_ws w;
    carve(&w, a->workspace, a->n, alloc_tiles(a->n, tile));
    wide_want want;
    want.curve = any_curve;
    want.all = a->curve_mode == ANODDPM_ROC_CURVE_ALL;
    want.ap = a->ap != nullptr;
    want.best = any_best;
    const dim3 tiles(g.T), wt(WT), one(1), st(ST);
    for (int32_t seg = 0; seg < a->S; ++seg) {
        const float *score = a->score + (int64_t)seg * a->score_stride, *mask = a->mask + (int64_t)seg * a->mask_stride;
        hipLaunchKernelGGL(keys_kernel, tiles, wt, 0, s, score, mask, w, g);
        uint32_t *src = w.buf0, *dst = w.buf1;
        for (int pass = 0; pass < 4; ++pass) {
            if (pass > 0) hipLaunchKernelGGL(hist_kernel, tiles, wt, 0, s, src, w.table, g, pass * 8);
            hipLaunchKernelGGL(scan_kernel, one, st, 0, s, w.table, w.hdr + H_SKIP + pass, g);
            hipLaunchKernelGGL(scatter_kernel<false>, tiles, wt, 0, s, src, dst, (const int32_t *)nullptr, (int32_t *)nullptr, w.table, w.hdr + H_SKIP + pass, g, pass * 8);
            uint32_t *t = src;
            src = dst;
            dst = t;
        }                                                        // four swaps: the sorted keys are in buf0
        uint32_t *runpos = w.buf1, *runtp = w.buf2;
        hipLaunchKernelGGL(run_count_kernel, tiles, wt, 0, s, src, w, g);
        hipLaunchKernelGGL(run_write_kernel, tiles, wt, 0, s, src, runpos, runtp, w, g);
        hipLaunchKernelGGL(run_terms_kernel, tiles, wt, 0, s, runpos, runtp, w, g, want);
        if (any_curve) {
            wide_curve c;
            c.fps = a->curve_fps + (int64_t)seg * a->curve_cap;
            c.tps = a->curve_tps + (int64_t)seg * a->curve_cap;
            c.thr = a->curve_thr + (int64_t)seg * a->curve_cap;
            c.cap = a->curve_cap;
            hipLaunchKernelGGL(curve_write_kernel, tiles, wt, 0, s, src, runpos, runtp, w, g, want, c);
        }
        if (want.ap) hipLaunchKernelGGL(lanes_kernel, dim3(AP_WAVES), st, 0, s, (const double *)w.terms, (const uint32_t *)(w.hdr + H_R), w.wavesum, g.n);
        wide_out o;
        o.auc = a->auc + seg;
        o.counts = a->counts + (int64_t)seg * 4;
        o.status = a->status + seg;
        o.curve_len = any_curve ? a->curve_len + seg : nullptr;
        o.curve_cap = a->curve_cap;
        o.ap = want.ap ? a->ap + seg : nullptr;
        o.best_dice = any_best ? a->best_dice + seg : nullptr;
        o.best_thr = any_best ? a->best_thr + seg : nullptr;
        o.best_counts = any_best ? a->best_counts + (int64_t)seg * 2 : nullptr;
        hipLaunchKernelGGL(finish_kernel, one, wt, 0, s, src, runpos, runtp, w, g, want, o);
        if (int rc = check_launch("roc_auc_wide")) return rc;
    }
    return ANODDPM_OK;
}
