// Per-region overlap (PRO) curve and AUPRO of batched anomaly maps (Bergmann et al., "The MVTec Anomaly Detection Dataset", IJCV
// 2021; include/anoddpm_hip.h has the definition) -- replaces, per segment of m planes,
//   scipy.ndimage.label(plane) per plane + numpy.argsort(score) + cumsum(1 / area) / K + the trapezoid up to the FPR limit
// with the areas of anoddpm_component_areas (csrc/postproc.hip) as input.  One workgroup of 16 waves per segment, one launch, no
// cross-workgroup ordering of any kind -- the layout of csrc/roc.hip, whose sort is RESTATED here with a payload (roc.hip itself
// is untouched, so its key-only instantiation carries no payload traffic):
//   1. key = (bits(score + 0.0f) << 1) | (area != 0), the key of roc.hip; the pixel's int32 area travels with it as a payload.
//      (A 64-bit key (bits << 32) | area would need eight passes where four do: the area takes no part in the order.)
//   2. stable LSD radix sort, 8 bits per pass, global ping-pong buffers for keys and payloads: per-wave contiguous chunks and
//      wave-private LDS histogram rows, rank among the equal digits of a 64-lane group from eight ballots, single-bin passes skipped
//   3. one scan over the sorted elements from the highest score down, position j = 0 ... n - 1, each wave a contiguous chunk:
//        w_j = 1 / area_j (fp64, correctly rounded) on a positive, 0 on a negative
//        cw_j = inclusive sum of w, cp_j = inclusive count of positives, q_j = number of run ends before j
//      A run (one distinct score) ends at j when j = n - 1 or the next score differs; there the prediction score >= v holds
//      exactly the elements 0 ... j, so fps = j + 1 - cp_j and PRO = min(1, cw_j / K) are curve point q_j.
//      The fp64 sum has a FIXED order: a Hillis-Steele scan over the 64 lanes of a group, the groups of a wave's chunk added one
//      after the other to a running carry, the carry of a wave = the totals of the waves before it added in wave order.  The
//      totals come from a first walk with the same group scan.  No atomics on floating-point values: same input, same bits.
//   4. the truncated trapezoid over the curve points (fp64 FPR = fps / N, one division): thread t adds the terms of the points
//      t, t + 1024, ... in that order, a halving tree folds the 64 partials of a wave and then the 16 wave sums (the order of
//      roc.hip's average precision); AUPRO = sum / limit.
// K is folded from the per-plane region counts at the start of the launch.  Compiled with -ffp-contract=off.
// The key, the element of the walk with its weight, the group scan, the PRO value and the trapezoid term are the functions of
// pro_shared.h, which csrc/pro_wide.hip (one segment over the whole chip, the same bits) includes too.
#include "common.h"
#include "pro_shared.h"

namespace {

using namespace anoddpm::pro;                                    // make_key, group_scan, elem_of, pro_value, term_of: shared with pro_wide.hip

constexpr int THREADS = 1024, WAVES = THREADS / 64, RADIX = 256, UNROLL = 4;

__device__ __forceinline__ void wave_sync()
{
    // same-wave LDS hand-off (one lane writes what other lanes of the wave read): the hardware runs a wave's LDS operations in
    // order; this only keeps the compiler from moving them across the point or into divergent branches
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// exclusive prefix of v over the workgroup in thread order (two barriers; wsum: WAVES words of LDS)
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wsum)
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
    for (int w = 0; w < wave; ++w) base += wsum[w];
    __syncthreads();
    return base + incl - v;
}

// sum of the per-wave totals below `wave`, and of all of them
__device__ __forceinline__ void wave_carry(const uint32_t *wtot, int wave, uint32_t &below, uint32_t &total)
{
    below = 0;
    total = 0;
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t t = wtot[w];
        if (w < wave) below += t;
        total += t;
    }
}

__global__ __launch_bounds__(THREADS) void pro_auc_kernel(anoddpm_pro_args a, int64_t seg_words)
{
    __shared__ uint32_t hist[WAVES * RADIX];                     // wave-private rows: digit counts, then scatter offsets
    __shared__ uint32_t wsum[WAVES], wtot_p[WAVES], wtot_e[WAVES];
    __shared__ double wtot_w[WAVES];
    __shared__ unsigned long long s_K;
    __shared__ uint32_t s_status, s_skip;

    const int seg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t hw = (int64_t)a.H * a.W;
    const uint32_t n = (uint32_t)(hw * a.planes_per_segment);
    const float *__restrict__ score = a.score + (int64_t)seg * a.score_stride;
    const int32_t *__restrict__ area = a.area + (int64_t)seg * a.area_stride;
    const float *__restrict__ mask = a.mask ? a.mask + (int64_t)seg * a.mask_stride : nullptr;
    const int64_t *__restrict__ region_counts = a.region_counts + (a.area_stride == 0 ? 0 : (int64_t)seg * a.planes_per_segment);
    // per segment: seg_words doubles (the PRO of every curve point), then keys twice and payloads twice (seg_words words each)
    uint32_t *ws = static_cast<uint32_t *>(a.workspace) + (int64_t)seg * 6 * seg_words;
    double *runpro = reinterpret_cast<double *>(ws);
    uint32_t *src = ws + 2 * seg_words, *dst = ws + 3 * seg_words;
    int32_t *psrc = reinterpret_cast<int32_t *>(ws + 4 * seg_words), *pdst = reinterpret_cast<int32_t *>(ws + 5 * seg_words);
    const uint64_t lt = (1ull << lane) - 1ull;

    // contiguous chunk of this wave, a multiple of 64 long (n < 2^31: no 32-bit overflow below)
    const uint32_t chunk = ((n + WAVES - 1) / WAVES + 63u) & ~63u;
    const uint32_t c0 = min((uint32_t)wave * chunk, n), c1 = min(c0 + chunk, n);

    // ---- 1. keys, payloads, precondition check, K
    if (tid == 0) { s_status = 0; s_K = 0; }
    __syncthreads();
    {
        uint32_t st = 0;
        for (uint32_t i = tid; i < n; i += THREADS) {
            const float s = score[i];
            const int32_t ar = area[i];
            src[i] = make_key(s, ar, mask != nullptr, mask ? mask[i] : 0.0f, st);
            psrc[i] = ar;
        }
        if (st) atomicOr(&s_status, st);
        unsigned long long k = 0;
        for (int p = tid; p < a.planes_per_segment; p += THREADS) k += (unsigned long long)region_counts[p];
        if (k) atomicAdd(&s_K, k);
    }
    __syncthreads();

    // ---- 2. LSD radix sort of (src, psrc)[0..n)
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
            uint32_t ex = block_exclusive_scan(sum, wsum);
#pragma unroll
            for (int k = 0; k < 4; ++k) { hist[(w0 + k) * RADIX + d] = ex; ex += h[k]; }
        }
        __syncthreads();
        const bool skip = s_skip != 0;
        if (!skip) {
            for (uint32_t base = c0; base < c1; base += 64 * UNROLL) {
                uint32_t key[UNROLL];
                int32_t pay[UNROLL];
                bool valid[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const uint32_t i = base + u * 64 + lane;
                    valid[u] = i < c1;
                    key[u] = valid[u] ? src[i] : 0u;
                    pay[u] = valid[u] ? psrc[i] : 0;
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    if (base + u * 64 >= c1) break;              // wave-uniform
                    const uint32_t dg = (key[u] >> shift) & 255u;
                    uint64_t m = __ballot(valid[u]);
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        const bool bit = (dg >> b) & 1u;
                        const uint64_t bal = __ballot(valid[u] && bit);
                        m &= bit ? bal : ~bal;
                    }                                            // m: the valid lanes of this group with my digit
                    const uint32_t rank = __popcll(m & lt), cnt = __popcll(m);
                    uint32_t pos = 0;
                    if (valid[u]) pos = wh[dg] + rank;
                    wave_sync();
                    if (valid[u] && rank == cnt - 1) wh[dg] = pos + 1;
                    wave_sync();
                    if (valid[u] && pos < n) {                   // pos < n always; the guard keeps a bad offset inside the buffers
                        dst[pos] = key[u];
                        pdst[pos] = pay[u];
                    }
                }
            }
            uint32_t *t = src;
            src = dst;
            dst = t;
            int32_t *pt = psrc;
            psrc = pdst;
            pdst = pt;
        }
        __syncthreads();                                         // the scattered pairs are visible to every wave; hist is free
    }
    uint32_t *runfps = dst;                                      // the key buffer the sort left free: seg_words >= n words

    // ---- 3. the scan from the highest score down.  First walk: the totals of every wave
    uint32_t P, R;
    {
        uint32_t cp = 0, ce = 0;
        double cw = 0.0;
        for (uint32_t base = c0; base < c1; base += 64) {
            const Elem e = elem_of(src, psrc, base + lane, c1, n);
            cp += __popcll(__ballot(e.pos));
            ce += __popcll(__ballot(e.end));
            cw += __shfl(group_scan(e.w, lane), 63);
        }
        if (lane == 0) { wtot_p[wave] = cp; wtot_e[wave] = ce; wtot_w[wave] = cw; }
    }
    __syncthreads();
    const unsigned long long K = s_K;
    const uint32_t status = s_status;
    {
        uint32_t carry_p, carry_e;
        wave_carry(wtot_p, wave, carry_p, P);
        wave_carry(wtot_e, wave, carry_e, R);
        double carry_w = 0.0;
        for (int w = 0; w < wave; ++w) carry_w += wtot_w[w];
        const bool want_curve = a.curve_fps != nullptr;
        for (uint32_t base = c0; base < c1; base += 64) {
            const uint32_t j = base + lane;
            const Elem e = elem_of(src, psrc, j, c1, n);
            const uint64_t bp = __ballot(e.pos), be = __ballot(e.end);
            const double incl = group_scan(e.w, lane);
            if (e.end) {
                const uint32_t q = carry_e + __popcll(be & lt);
                const uint32_t fps = (j + 1) - (carry_p + __popcll(bp & lt) + (e.pos ? 1u : 0u));
                const double pro = pro_value(carry_w, incl, K);
                runfps[q] = fps;                                 // q < R <= n
                runpro[q] = pro;
                if (want_curve && (int64_t)q < a.curve_cap) {
                    const int64_t o = (int64_t)seg * a.curve_cap + (int64_t)q;
                    a.curve_fps[o] = (int32_t)fps;
                    a.curve_pro[o] = pro;
                    a.curve_thr[o] = __uint_as_float(e.key >> 1);
                }
            }
            carry_p += __popcll(bp);
            carry_e += __popcll(be);
            carry_w += __shfl(incl, 63);
        }
    }
    __syncthreads();

    // ---- 4. the trapezoid up to the limit: the term of point q is the area between the points q - 1 and q
    const uint32_t N = n - P;
    {
        const double dN = (double)N, limit = a.limit;
        double part = 0.0;
        if (K != 0 && N != 0) {
            for (uint32_t q = tid; q < R; q += THREADS) {
                part += term_of(runfps, runpro, q, dN, limit);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
        if (lane == 0) wtot_w[wave] = part;                      // free since the barrier that ended step 3
        __syncthreads();
        if (wave == 0) {
            part = lane < WAVES ? wtot_w[lane] : 0.0;
#pragma unroll
            for (int off = WAVES / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
            if (lane == 0) {
                a.aupro[seg] = (K == 0 || N == 0) ? (double)NAN : part / limit;
                int64_t *c = a.counts + (int64_t)seg * 4;
                c[0] = (int64_t)K;
                c[1] = N;
                c[2] = P;
                c[3] = R;
                const bool want_curve = a.curve_fps != nullptr;
                a.status[seg] = (int32_t)(status | ((want_curve && (int64_t)R > a.curve_cap) ? ANODDPM_ROC_CURVE_TRUNCATED : 0u));
                if (want_curve) a.curve_len[seg] = (int32_t)R;
            }
        }
    }
}

int64_t seg_words_of(int64_t n) { return (n + 63) / 64 * 64; }

}  // namespace

extern "C" int64_t anoddpm_pro_workspace_bytes(int32_t S, int64_t n)
{
    if (S < 1 || n < 1 || n >= ((int64_t)1 << 31)) return -1;
    return (int64_t)S * 6 * seg_words_of(n) * (int64_t)sizeof(uint32_t);
}

extern "C" int anoddpm_pro_auc(const anoddpm_pro_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "pro_auc: null args");
    ANODDPM_REQUIRE(a->score && a->area && a->region_counts && a->workspace && a->aupro && a->counts && a->status, "pro_auc: null pointer");
    ANODDPM_REQUIRE(a->S >= 1, "pro_auc: S must be >= 1");
    ANODDPM_REQUIRE(a->planes_per_segment >= 1 && a->H >= 1 && a->W >= 1, "pro_auc: planes_per_segment, H and W must be >= 1");
    const int64_t hw = (int64_t)a->H * a->W;
    ANODDPM_REQUIRE(hw < ((int64_t)1 << 31) && hw <= (((int64_t)1 << 31) - 1) / a->planes_per_segment,
                    "pro_auc: n = planes_per_segment * H * W must be below 2^31 (32-bit positions)");
    const int64_t n = hw * a->planes_per_segment;
    ANODDPM_REQUIRE(a->limit > 0.0 && a->limit <= 1.0, "pro_auc: limit must be in (0, 1]");
    ANODDPM_REQUIRE(a->S == 1 || a->score_stride >= n, "pro_auc: score segments overlap (score_stride < n)");
    ANODDPM_REQUIRE(a->S == 1 || a->area_stride == 0 || a->area_stride >= n, "pro_auc: area_stride must be 0 (shared mask) or >= n");
    ANODDPM_REQUIRE(!a->mask || a->S == 1 || a->mask_stride == 0 || a->mask_stride >= n, "pro_auc: mask_stride must be 0 (shared mask) or >= n");
    ANODDPM_REQUIRE(a->workspace_bytes >= anoddpm_pro_workspace_bytes(a->S, n), "pro_auc: workspace too small");
    if (a->curve_fps || a->curve_pro || a->curve_thr || a->curve_len) {
        ANODDPM_REQUIRE(a->curve_fps && a->curve_pro && a->curve_thr && a->curve_len, "pro_auc: curve output needs curve_fps, curve_pro, curve_thr and curve_len");
        ANODDPM_REQUIRE(a->curve_cap >= 1, "pro_auc: curve capacity must be >= 1 point per segment");
    }
    hipLaunchKernelGGL(pro_auc_kernel, dim3(a->S), dim3(THREADS), 0, as_stream(stream), *a, seg_words_of(n));
    return check_launch("pro_auc");
}
