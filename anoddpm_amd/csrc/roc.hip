// ROC curve and AUC of batched anomaly maps -- replaces, per segment (one flattened map, or a whole concatenated data set),
//   sklearn.metrics.roc_curve(mask, sqerr)                evaluation.py:79-82; detection.py:230, 553, 569, 583
//   sklearn.metrics.auc(fpr, tpr)                         evaluation.py:85-87; detection.py:231, 554, 570, 584
// One workgroup of 16 waves per segment, one launch, no cross-workgroup ordering of any kind:
//   1. key = (bits(score + 0.0f) << 1) | (mask != 0): for finite score >= 0 the bit pattern is monotone and the sign bit is free,
//      so one 32-bit word sorts by score and keeps the label (negatives before positives inside equal scores)
//   2. LSD radix sort, 8 bits per pass, global ping-pong buffers (a 256^2 segment is 256 KB of keys: L2-resident).  Every wave owns
//      a contiguous chunk of the segment and a private LDS histogram row, so the scatter is stable without a barrier inside the
//      loops: the rank of a key among the equal digits of its 64-lane group comes from eight ballots.  A pass whose histogram
//      has a single non-empty bin is skipped
//   3. runs of equal score: their start position and the number of positives below them, compacted in ascending order
//   4. twoU = sum_v P_v * (2 * N_below(v) + N_v) in uint64 (the tie-corrected Mann-Whitney statistic = the trapezoid area under
//      sklearn's curve, independent of summation order), AUC = twoU / (2 P N) in fp64
//   5. optionally the curve points sklearn keeps (drop_intermediate: first, last, and every point where the second difference of
//      fps or tps is non-zero, i.e. where the next lower run has other counts), written compactly from the highest score down;
//      curve mode ANODDPM_ROC_CURVE_ALL keeps every run instead (what sklearn.metrics.precision_recall_curve works on)
//   6. optionally one more walk over the run list (the EXTRA instantiation; a launch that asks for none of it runs the plain one):
//      per run r, tps_r = P - runtp[r] and cnt_r = n - runpos[r] = tps_r + fps_r are the counts of the prediction score >= thr_r
//      - average precision = sum_r (p_r / P) * (tps_r / cnt_r) in fp64: thread t adds the runs t, t + 1024, ... in that order, a
//        halving tree folds the 64 partials of a wave and then the 16 wave sums.  Fixed order, no atomics: same input, same bits
//      - best Dice = max_r 2 tps_r / (cnt_r + P): a > b iff tps_a * den_b > tps_b * den_a, exact in uint64 (tps < 2^31, den <
//        3 * 2^31); ties go to the higher score.  That order is total, so the reduction's shape does not matter
// All counters are integers: the result is deterministic.  Compiled with -ffp-contract=off like the other metric kernels.
#include "common.h"
#include "roc_shared.h"                                          // what this file shares with roc_wide.hip

namespace {

using namespace anoddpm::roc;

constexpr int THREADS = 1024, WAVES = THREADS / 64, RADIX = 256, UNROLL = 4;

template <bool EXTRA>
__global__ __launch_bounds__(THREADS) void roc_auc_kernel(anoddpm_roc_args a, int64_t seg_words)
{
    __shared__ uint32_t hist[WAVES * RADIX];                     // wave-private rows: digit counts, then scatter offsets
    __shared__ uint32_t wsum[WAVES], wtot_p[WAVES], wtot_b[WAVES];
    __shared__ unsigned long long wacc[WAVES];
    __shared__ uint32_t s_status, s_skip;

    const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = (uint32_t)a.n;
    const float *__restrict__ score = a.score + (int64_t)seg * a.score_stride;
    const float *__restrict__ mask = a.mask + (int64_t)seg * a.mask_stride;
    uint32_t *ws = static_cast<uint32_t *>(a.workspace) + (int64_t)seg * 3 * seg_words;
    uint32_t *src = ws, *dst = ws + seg_words, *third = ws + 2 * seg_words;
    const uint64_t lt = (1ull << lane) - 1ull;

    // contiguous chunk of this wave, a multiple of 64 long (n < 2^31: no 32-bit overflow below)
    const uint32_t chunk = ((n + WAVES - 1) / WAVES + 63u) & ~63u;
    const uint32_t c0 = min((uint32_t)wave * chunk, n), c1 = min(c0 + chunk, n);

    // ---- 1. keys + precondition check
    if (tid == 0) s_status = 0;
    __syncthreads();
    {
        uint32_t st = 0;
        for (uint32_t i = tid; i < n; i += THREADS) {
            src[i] = make_key(score[i], mask[i], st);
        }
        if (st) atomicOr(&s_status, st);
    }
    __syncthreads();

    // ---- 2. LSD radix sort of src[0..n)
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = pass * 8;
        for (int i = tid; i < WAVES * RADIX; i += THREADS) hist[i] = 0;
        if (tid == 0) s_skip = 0;
        __syncthreads();
        uint32_t *wh = hist + wave * RADIX;
        for (uint32_t i = c0 + lane; i < c1; i += 64) atomicAdd(&wh[(src[i] >> shift) & 255u], 1u);
        __syncthreads();
        // exclusive scan in (digit, wave) order: thread t owns digit t / 4 and the four waves (t % 4) * 4 ...
        {
            const int d = tid >> 2, w0 = (tid & 3) * 4;
            uint32_t h[4], sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { h[k] = hist[(w0 + k) * RADIX + d]; sum += h[k]; }
            uint32_t dt = sum;
            dt += __shfl_xor(dt, 1);
            dt += __shfl_xor(dt, 2);
            if (dt == n && (tid & 3) == 0) s_skip = 1;           // every key has this digit: the pass would move nothing
            uint32_t all;
            uint32_t ex = block_exclusive_scan<WAVES>(sum, wsum, all);
#pragma unroll
            for (int k = 0; k < 4; ++k) { hist[(w0 + k) * RADIX + d] = ex; ex += h[k]; }
        }
        __syncthreads();
        const bool skip = s_skip != 0;
        if (!skip) {
            for (uint32_t base = c0; base < c1; base += 64 * UNROLL) {
                uint32_t key[UNROLL];
                bool valid[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const uint32_t i = base + u * 64 + lane;
                    valid[u] = i < c1;
                    key[u] = valid[u] ? src[i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    if (base + u * 64 >= c1) break;              // wave-uniform
                    const uint32_t dg = (key[u] >> shift) & 255u;
                    const uint64_t m = digit_peers(dg, valid[u]);    // the valid lanes of this group with my digit
                    const uint32_t rank = __popcll(m & lt), cnt = __popcll(m);
                    uint32_t pos = 0;
                    if (valid[u]) pos = wh[dg] + rank;
                    wave_sync();
                    if (valid[u] && rank == cnt - 1) wh[dg] = pos + 1;
                    wave_sync();
                    if (valid[u] && pos < n) dst[pos] = key[u];   // pos < n always; the guard keeps a bad offset inside the buffer
                }
            }
            uint32_t *t = src;
            src = dst;
            dst = t;
        }
        __syncthreads();                                         // the scattered keys are visible to every wave; hist is free
    }
    uint32_t *runpos = dst, *runtp = third;                      // seg_words >= n + 1 each

    // ---- 3. runs of equal score, ascending: runpos[r] = first position, runtp[r] = positives below it
    uint32_t P, R;
    {
        uint32_t cp = 0, cb = 0;
        for (uint32_t base = c0; base < c1; base += 64) {
            const uint32_t i = base + lane;
            const bool valid = i < c1;
            const uint32_t k = valid ? src[i] : 0u, kp = (valid && i > 0) ? src[i - 1] : 0u;
            cp += __popcll(__ballot(valid && (k & 1u)));
            cb += __popcll(__ballot(valid && (i == 0 || (k >> 1) != (kp >> 1))));
        }
        if (lane == 0) { wtot_p[wave] = cp; wtot_b[wave] = cb; }
        __syncthreads();
        uint32_t carry_p, carry_b;
        wave_carry<WAVES>(wtot_p, wave, carry_p, P);
        wave_carry<WAVES>(wtot_b, wave, carry_b, R);
        for (uint32_t base = c0; base < c1; base += 64) {
            const uint32_t i = base + lane;
            const bool valid = i < c1;
            const uint32_t k = valid ? src[i] : 0u, kp = (valid && i > 0) ? src[i - 1] : 0u;
            const bool bnd = valid && (i == 0 || (k >> 1) != (kp >> 1));
            const uint64_t bp = __ballot(valid && (k & 1u)), bb = __ballot(bnd);
            if (bnd) {
                const uint32_t r = carry_b + __popcll(bb & lt);
                runpos[r] = i;
                runtp[r] = carry_p + __popcll(bp & lt);
            }
            carry_p += __popcll(bp);
            carry_b += __popcll(bb);
        }
        if (tid == 0) { runpos[R] = n; runtp[R] = P; }           // sentinel: the end of the last run
        __syncthreads();
    }

    // ---- 4. + 5. per run, from the highest score down (q = R - 1 - r): its term of twoU, and its curve point if kept
    const bool want_curve = a.curve_fps != nullptr;
    const bool all = EXTRA && a.curve_mode == ANODDPM_ROC_CURVE_ALL;     // every run is a curve point
    const uint32_t qchunk = ((R + WAVES - 1) / WAVES + 63u) & ~63u;
    const uint32_t q0 = min((uint32_t)wave * qchunk, R), q1 = min(q0 + qchunk, R);
    uint32_t carry_k = 0, K = 0;
    if (want_curve) {
        uint32_t ck = 0;
        for (uint32_t base = q0; base < q1; base += 64) {
            const uint32_t q = base + lane;
            const bool keep = q < q1 && (all || keep_point(runpos, runtp, R - 1 - q, R));
            ck += __popcll(__ballot(keep));
        }
        if (lane == 0) wtot_p[wave] = ck;                        // free since the barrier that ended step 3
        __syncthreads();
        wave_carry<WAVES>(wtot_p, wave, carry_k, K);
    }
    unsigned long long acc = 0;
    for (uint32_t base = q0; base < q1; base += 64) {
        const uint32_t q = base + lane;
        const bool valid = q < q1;
        uint32_t rs = 0, tp = 0;
        bool keep = false;
        if (valid) {
            const uint32_t r = R - 1 - q;
            rs = runpos[r];
            tp = runtp[r];
            const uint32_t pr = runtp[r + 1] - tp, nr = (runpos[r + 1] - rs) - pr;
            acc += (unsigned long long)pr * (2ull * (rs - tp) + nr);     // rs - tp = negatives with a lower score
            keep = want_curve && (all || keep_point(runpos, runtp, r, R));
        }
        if (want_curve) {
            const uint64_t bk = __ballot(keep);
            const uint64_t idx = (uint64_t)carry_k + __popcll(bk & lt);
            if (keep && (int64_t)idx < a.curve_cap) {
                const int64_t o = (int64_t)seg * a.curve_cap + (int64_t)idx;
                const uint32_t tps = P - tp;
                a.curve_tps[o] = (int32_t)tps;
                a.curve_fps[o] = (int32_t)((n - rs) - tps);
                a.curve_thr[o] = __uint_as_float(src[rs] >> 1);
            }
            carry_k += __popcll(bk);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) wacc[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        unsigned long long two_u = 0;
        for (int w = 0; w < WAVES; ++w) two_u += wacc[w];
        const uint32_t N = n - P;
        a.auc[seg] = (P == 0 || N == 0) ? (double)NAN : (double)two_u / (2.0 * (double)P * (double)N);
        int64_t *c = a.counts + (int64_t)seg * 4;
        c[0] = P;
        c[1] = N;
        c[2] = (int64_t)two_u;
        c[3] = R;
        a.status[seg] = (int32_t)(s_status | ((want_curve && (int64_t)K > a.curve_cap) ? ANODDPM_ROC_CURVE_TRUNCATED : 0u));
        if (want_curve) a.curve_len[seg] = (int32_t)K;
    }

    // ---- 6. average precision and best Dice: one more walk over the runs, ascending, thread t takes r = t, t + THREADS, ...
    if constexpr (EXTRA) {
        const bool want_ap = a.ap != nullptr, want_best = a.best_dice != nullptr;
        if (!want_ap && !want_best) return;                      // block-uniform
        __shared__ double wap[WAVES];
        __shared__ uint32_t wbt[WAVES], wbc[WAVES], wbr[WAVES];
        const double dP = (double)P;
        double part = 0.0;
        uint32_t btp = 0, bc = 1, br = 0;                         // loses against every run, or is run 0 itself when P == 0
        for (uint32_t r = tid; r < R; r += THREADS) {
            const uint32_t tp0 = runtp[r], tps = P - tp0, cnt = n - runpos[r], pr = runtp[r + 1] - tp0;
            // a run without positives adds +0.0, which leaves the bits of the partial as they are: skipped
            if (want_ap && pr != 0) part += ((double)pr / dP) * ((double)tps / (double)cnt);
            if (dice_better(tps, cnt, r, btp, bc, br, P)) { btp = tps; bc = cnt; br = r; }
        }
        part = tree_add<64>(part);
        tree_dice<64>(btp, bc, br, P);
        if (lane == 0) { wap[wave] = part; wbt[wave] = btp; wbc[wave] = bc; wbr[wave] = br; }
        __syncthreads();
        if (wave == 0) {
            part = lane < WAVES ? wap[lane] : 0.0;
            btp = lane < WAVES ? wbt[lane] : 0u;
            bc = lane < WAVES ? wbc[lane] : 1u;
            br = lane < WAVES ? wbr[lane] : 0u;
            part = tree_add<WAVES>(part);
            tree_dice<WAVES>(btp, bc, br, P);
            if (lane == 0) {
                if (want_ap) a.ap[seg] = P == 0 ? (double)NAN : (P == n ? 1.0 : part);
                if (want_best) {
                    const uint32_t rs = runpos[br], tps = P - runtp[br], cnt = n - rs;
                    a.best_dice[seg] = P == 0 ? (double)NAN : (double)(2ull * tps) / (double)((unsigned long long)cnt + P);
                    a.best_thr[seg] = __uint_as_float(src[rs] >> 1);
                    a.best_counts[(int64_t)seg * 2] = tps;
                    a.best_counts[(int64_t)seg * 2 + 1] = cnt - tps;
                }
            }
        }
    }
}

int64_t seg_words_of(int64_t n) { return (n + 1 + 63) / 64 * 64; }

}  // namespace

extern "C" int64_t anoddpm_roc_workspace_bytes(int32_t S, int64_t n)
{
    if (S < 1 || n < 1 || n >= ((int64_t)1 << 31)) return -1;
    return (int64_t)S * 3 * seg_words_of(n) * (int64_t)sizeof(uint32_t);
}

extern "C" int anoddpm_roc_auc(const anoddpm_roc_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "roc_auc: null args");
    ANODDPM_REQUIRE(a->score && a->mask && a->workspace && a->auc && a->counts && a->status, "roc_auc: null pointer");
    ANODDPM_REQUIRE(a->S >= 1, "roc_auc: S must be >= 1");
    ANODDPM_REQUIRE(a->n >= 1, "roc_auc: n must be >= 1");
    ANODDPM_REQUIRE(a->n < ((int64_t)1 << 31), "roc_auc: n must be below 2^31 (32-bit positions, uint64 twoU)");
    ANODDPM_REQUIRE(a->S == 1 || a->score_stride >= a->n, "roc_auc: score segments overlap (score_stride < n)");
    ANODDPM_REQUIRE(a->S == 1 || a->mask_stride == 0 || a->mask_stride >= a->n, "roc_auc: mask_stride must be 0 (shared mask) or >= n");
    ANODDPM_REQUIRE(a->workspace_bytes >= anoddpm_roc_workspace_bytes(a->S, a->n), "roc_auc: workspace too small");
    const bool any_curve = a->curve_fps || a->curve_tps || a->curve_thr || a->curve_len;
    if (any_curve) {
        ANODDPM_REQUIRE(a->curve_fps && a->curve_tps && a->curve_thr && a->curve_len, "roc_auc: curve output needs curve_fps, curve_tps, curve_thr and curve_len");
        ANODDPM_REQUIRE(a->curve_cap >= 2, "roc_auc: curve capacity must be >= 2 points per segment");
    }
    ANODDPM_REQUIRE(a->curve_mode == ANODDPM_ROC_CURVE_DROP || a->curve_mode == ANODDPM_ROC_CURVE_ALL, "roc_auc: unknown curve_mode");
    ANODDPM_REQUIRE(a->curve_mode == ANODDPM_ROC_CURVE_DROP || any_curve, "roc_auc: curve_mode needs the curve outputs");
    const bool any_best = a->best_dice || a->best_thr || a->best_counts;
    if (any_best) ANODDPM_REQUIRE(a->best_dice && a->best_thr && a->best_counts, "roc_auc: best Dice output needs best_dice, best_thr and best_counts");
    // the plain instantiation is the kernel as it was before average precision, best Dice and the full curve existed
    if (a->ap || any_best || a->curve_mode != ANODDPM_ROC_CURVE_DROP)
        hipLaunchKernelGGL(roc_auc_kernel<true>, dim3(a->S), dim3(THREADS), 0, as_stream(stream), *a, seg_words_of(a->n));
    else
        hipLaunchKernelGGL(roc_auc_kernel<false>, dim3(a->S), dim3(THREADS), 0, as_stream(stream), *a, seg_words_of(a->n));
    return check_launch("roc_auc");
}
