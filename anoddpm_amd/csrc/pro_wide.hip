// Per-region overlap curve and AUPRO of ONE long segment spread over the whole chip -- what csrc/pro.hip computes with one
// workgroup per segment, here as a sequence of launches with one workgroup per tile of `tile` elements (several planes pooled into
// one curve: the data-set form of the score, Bergmann et al., IJCV 2021).  Replaces what anoddpm_pro_auc replaces: no call of the
// reference.  A launch boundary is the only ordering between workgroups: no kernel below waits for another workgroup, and none
// reads, within a launch, what another workgroup wrote in that launch.  Every loop is bounded by n, by the tile count or by the
// group count (a group: 64 consecutive positions of the descending walk).
//   keys        key as pro.hip (pro_shared.h) with the pixel's int32 area as a payload, the tile's precondition bits, and the
//               tile histogram of the first pass
//   4 x         scan, scatter (its payload instantiation), hist of the next pass's digit: the sort pass of wide_shared.h.  The
//               area moves with its key in the same pass, so equal keys keep the areas in input order (stable)
//   walk_count  per tile of the descending walk j = n - 1 - i: per group the lane-63 value of the group scan of w_j = 1 / area_j,
//               per tile its positives and run ends (a run end compares against key i - 1, across the tile border)
//   walk_carry  ONE workgroup of 1024: the sixteen serial chains of pro.hip's 16 waves.  Chain w adds the group totals of wave w's
//               chunk of pro.hip (((n + 15) / 16 + 63) & ~63 positions) in order from 0.0 (T_w), then starts from
//               ((0 + T_0) + ... + T_(w-1)) and writes the running carry in front of every group.  Also: exclusive scans of the
//               per-tile counts, K folded from region_counts, the OR of the per-tile status words
//   walk_write  per tile: carry in front of the group + group scan, PRO = min(1, cw / K) and fps at every run end into the
//               compact runfps / runpro arrays and the curve outputs (q < curve_cap)
//   terms       per tile of RUNS: the trapezoid term of curve point q (pro_shared.h), point q - 1 read across the tile border; a
//               term pro.hip skips is +0.0
//   lanes       16 workgroups (wide_shared.h): virtual lane t of 1024 adds the terms t, t + 1024, ... then the 64-lane tree
//   finish      one workgroup: the 16-wave tree, AUPRO = sum / limit, counts, status, curve_len
// 18 launches per segment.  Every output has the bits anoddpm_pro_auc writes: the weights, the group scan, the PRO value and the
// term are the functions of pro_shared.h, and every fp64 addition happens between the same operands in the same order (the group
// scan over the same 64 positions, the carries in wave-chunk order, the strided lane sum and the two trees).  H, W and
// planes_per_segment are read only through n = planes_per_segment * H * W and region_counts only through its sum.
// Compiled with -ffp-contract=off.  There is no floating-point atomic in this file.
#include "common.h"
#include "pro_shared.h"
#include "wide_shared.h"

namespace {

using namespace anoddpm::pro;
using namespace anoddpm::wide;

constexpr int CW = 1024, CWAVES = CW / 64;                       // walk_carry: the workgroup of pro.hip
enum { H_SKIP = 0, H_R = 4, H_P = 5, H_ST = 6, H_WORDS = 64 };

static_assert(CWAVES == 16 && 2 * CW == MAX_TILES, "walk_carry: pro.hip's 16 waves; one thread owns two tiles of the count scans");

struct pro_ws {                  // one segment's workspace
    double *runpro;              // [W] PRO of curve point q
    double *gtot, *gcarry;       // [W / 64] total of a group of the walk; running carry in front of it
    double *wavesum;             // [16]
    unsigned long long *K;       // [1]
    uint32_t *key0, *key1;       // [W] each: keys ping / pong; sorted keys end in key0
    int32_t *pay0, *pay1;        // [W] each: areas ping / pong.  key1 and pay1 are adjacent: W doubles of terms after the sort
    uint32_t *runfps;            // [W]
    uint32_t *table;             // [256][T]
    uint32_t *tile_p, *tile_e, *tile_cp, *tile_ce, *tile_st;    // [Tp]: counts, their exclusive prefixes, status
    uint32_t *hdr;               // H_WORDS
};

int64_t seg_words_of(int64_t n) { return (n + 63) / 64 * 64; }

int64_t carve(pro_ws *w, void *base, int64_t n, int64_t Ta)
{
    const int64_t W = seg_words_of(n), Tp = (Ta + 3) / 4 * 4;
    char *p = static_cast<char *>(base);
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *q = p ? p + o : nullptr; o += (bytes + 15) / 16 * 16; return q; };
    w->runpro = (double *)take(W * 8);
    w->gtot = (double *)take(W / 64 * 8);
    w->gcarry = (double *)take(W / 64 * 8);
    w->wavesum = (double *)take(AP_WAVES * 8);
    w->K = (unsigned long long *)take(8);
    w->key0 = (uint32_t *)take(W * 4);
    w->pay0 = (int32_t *)take(W * 4);
    w->key1 = (uint32_t *)take(2 * W * 4);                       // W * 4 bytes is a multiple of 16: pay1 follows without a gap
    w->pay1 = (int32_t *)(w->key1 ? w->key1 + W : nullptr);
    w->runfps = (uint32_t *)take(W * 4);
    w->table = (uint32_t *)take(RADIX * Tp * 4);
    w->tile_p = (uint32_t *)take(Tp * 4);
    w->tile_e = (uint32_t *)take(Tp * 4);
    w->tile_cp = (uint32_t *)take(Tp * 4);
    w->tile_ce = (uint32_t *)take(Tp * 4);
    w->tile_st = (uint32_t *)take(Tp * 4);
    w->hdr = (uint32_t *)take(H_WORDS * 4);
    return o;
}

// ------------------------------------------------------------------------------------------------ sort
__global__ __launch_bounds__(WT) void keys_kernel(const float *__restrict__ score, const int32_t *__restrict__ area, const float *__restrict__ mask,
                                                  pro_ws w, wide_geom g)
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
        const int32_t ar = area[i];
        const uint32_t key = make_key(score[i], ar, mask != nullptr, mask ? mask[i] : 0.0f, st);
        w.key0[i] = key;
        w.pay0[i] = ar;
        atomicAdd(&hist[key & 255u], 1u);
    }
    if (st) atomicOr(&s_status, st);
    __syncthreads();
    w.table[tid * g.T + b] = hist[tid];                          // digit-major
    if (tid == 0) w.tile_st[b] = s_status;
}

// ------------------------------------------------------------------------------------------------ walk
// the wave's part of tile b of the descending walk: a multiple of 64 positions, so its groups are the groups of pro.hip's waves
__device__ __forceinline__ void wave_part(const wide_geom &g, uint32_t b, uint32_t wave, uint32_t &c0, uint32_t &c1)
{
    const uint32_t j0 = b * g.tile, j1 = min(j0 + g.tile, g.n);
    const uint32_t chunk = g.tile / WW;
    c0 = min(j0 + wave * chunk, j1);
    c1 = min(c0 + chunk, j1);
}

__global__ __launch_bounds__(WT) void walk_count_kernel(const uint32_t *__restrict__ key, const int32_t *__restrict__ area, pro_ws w, wide_geom g)
{
    __shared__ uint32_t wtot_p[WW], wtot_e[WW];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t c0, c1;
    wave_part(g, b, wave, c0, c1);
    uint32_t cp = 0, ce = 0;
    for (uint32_t base = c0; base < c1; base += 64) {
        const Elem e = elem_of(key, area, base + lane, c1, g.n);
        cp += __popcll(__ballot(e.pos));
        ce += __popcll(__ballot(e.end));
        const double tot = __shfl(group_scan(e.w, lane), 63);
        if (lane == 0) w.gtot[base >> 6] = tot;                  // base < n: group index < W / 64
    }
    if (lane == 0) { wtot_p[wave] = cp; wtot_e[wave] = ce; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < WW; ++k) { cp += wtot_p[k]; ce += wtot_e[k]; }
        w.tile_p[b] = cp;
        w.tile_e[b] = ce;
    }
}

struct carry_in { const int64_t *region_counts; int32_t planes; };

constexpr int GR = 256, GPER = GR / 64, GPITCH = GR + 1;         // group totals staged per chain and round; the pitch spreads the chains over the banks

// The sixteen chains of pro.hip's waves, one lane of wave 0 each: a chain is serial by definition (every addition rounds), so all a
// workgroup can add is bandwidth -- wave c stages GR totals of chain c per round in LDS with coalesced loads (the next round's are
// in flight meanwhile), lane c of wave 0 walks them in order and, in the second sweep, leaves the carry in front of each group in
// their place, which wave c then stores.  A slot past the chain's end holds +0.0, which leaves a non-negative sum alone.
__global__ __launch_bounds__(CW) void walk_carry_kernel(pro_ws w, wide_geom g, carry_in in)
{
    __shared__ double stage[CWAVES * GPITCH];
    __shared__ uint32_t wsum[CWAVES];
    __shared__ unsigned long long s_K;
    __shared__ uint32_t s_status;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = g.n, T = g.T;
    if (tid == 0) { s_K = 0; s_status = 0; }
    // the groups of this wave's chunk of pro.hip
    const uint32_t NG = (n + 63u) >> 6;
    const uint32_t gpc = (((n + CWAVES - 1) / CWAVES + 63u) & ~63u) >> 6;
    const uint32_t g0 = min(wave * gpc, NG), g1 = min(g0 + gpc, NG);
    const uint32_t rounds = (gpc + GR - 1) / GR;                 // the same for every chain: the barriers below are uniform
    double *row = stage + wave * GPITCH, *mine = stage + lane * GPITCH;  // mine: the chain of this lane of wave 0
    const bool walker = wave == 0 && lane < CWAVES;
    double next[GPER];
    auto fetch = [&](uint32_t r) {
#pragma unroll
        for (int u = 0; u < GPER; ++u) {
            const uint32_t idx = g0 + r * GR + u * 64 + lane;    // < NG + rounds * GR: no overflow
            next[u] = (r < rounds && idx < g1) ? w.gtot[idx] : 0.0;
        }
    };
    // first sweep: T_c, the totals of chain c added one after the other from 0.0
    double carry = 0.0;
    fetch(0);
    for (uint32_t r = 0; r < rounds; ++r) {
#pragma unroll
        for (int u = 0; u < GPER; ++u) row[u * 64 + lane] = next[u];
        __syncthreads();
        fetch(r + 1);
        if (walker) {
#pragma unroll 16
            for (int k = 0; k < GR; ++k) carry += mine[k];
        }
        __syncthreads();
    }
    // chain c starts from ((0 + T_0) + T_1) + ... + T_(c-1)
    {
        const double tc = carry;
        carry = 0.0;
        for (int v = 0; v < CWAVES; ++v) {
            const double t = __shfl(tc, v);
            if ((int)lane > v) carry += t;
        }
    }
    // second sweep: the carry in front of every group
    fetch(0);
    for (uint32_t r = 0; r < rounds; ++r) {
#pragma unroll
        for (int u = 0; u < GPER; ++u) row[u * 64 + lane] = next[u];
        __syncthreads();
        fetch(r + 1);
        if (walker) {
#pragma unroll 16
            for (int k = 0; k < GR; ++k) {
                const double t = mine[k];
                mine[k] = carry;
                carry += t;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < GPER; ++u) {
            const uint32_t idx = g0 + r * GR + u * 64 + lane;
            if (idx < g1) w.gcarry[idx] = row[u * 64 + lane];
        }
    }
    // the integers: exclusive prefixes of the per-tile counts (thread t owns tiles 2 t and 2 t + 1), K, status
    uint32_t P, R;
    {
        const uint32_t t0 = 2 * tid;
        const uint32_t a = t0 < T ? w.tile_p[t0] : 0u, b = t0 + 1 < T ? w.tile_p[t0 + 1] : 0u;
        const uint32_t ex = block_exclusive_scan<CWAVES>(a + b, wsum, P);
        if (t0 < T) w.tile_cp[t0] = ex;
        if (t0 + 1 < T) w.tile_cp[t0 + 1] = ex + a;
    }
    {
        const uint32_t t0 = 2 * tid;
        const uint32_t a = t0 < T ? w.tile_e[t0] : 0u, b = t0 + 1 < T ? w.tile_e[t0 + 1] : 0u;
        const uint32_t ex = block_exclusive_scan<CWAVES>(a + b, wsum, R);
        if (t0 < T) w.tile_ce[t0] = ex;
        if (t0 + 1 < T) w.tile_ce[t0 + 1] = ex + a;
    }
    {
        unsigned long long k = 0;
        for (int32_t p = (int32_t)tid; p < in.planes; p += CW) k += (unsigned long long)in.region_counts[p];
        if (k) atomicAdd(&s_K, k);
        uint32_t st = 0;
        for (uint32_t t = tid; t < T; t += CW) st |= w.tile_st[t];
        if (st) atomicOr(&s_status, st);
    }
    __syncthreads();
    if (tid == 0) {
        *w.K = s_K;
        w.hdr[H_R] = R;
        w.hdr[H_P] = P;
        w.hdr[H_ST] = s_status;
    }
}

struct pro_curve { int32_t *fps; double *pro; float *thr; int64_t cap; };

__global__ __launch_bounds__(WT) void walk_write_kernel(const uint32_t *__restrict__ key, const int32_t *__restrict__ area, pro_ws w, wide_geom g, pro_curve c)
{
    __shared__ uint32_t wtot_p[WW], wtot_e[WW];
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = g.n;
    const uint64_t lt = (1ull << lane) - 1ull;
    const unsigned long long K = *w.K;
    uint32_t c0, c1;
    wave_part(g, b, wave, c0, c1);
    uint32_t cp = 0, ce = 0;
    for (uint32_t base = c0; base < c1; base += 64) {
        const Elem e = elem_of(key, area, base + lane, c1, n);
        cp += __popcll(__ballot(e.pos));
        ce += __popcll(__ballot(e.end));
    }
    if (lane == 0) { wtot_p[wave] = cp; wtot_e[wave] = ce; }
    __syncthreads();
    uint32_t carry_p, carry_e, tp_, te_;
    wave_carry<WW>(wtot_p, wave, carry_p, tp_);
    wave_carry<WW>(wtot_e, wave, carry_e, te_);
    carry_p += w.tile_cp[b];
    carry_e += w.tile_ce[b];
    for (uint32_t base = c0; base < c1; base += 64) {
        const uint32_t j = base + lane;
        const Elem e = elem_of(key, area, j, c1, n);
        const uint64_t bp = __ballot(e.pos), be = __ballot(e.end);
        const double incl = group_scan(e.w, lane);
        const double carry_w = w.gcarry[base >> 6];
        if (e.end) {
            const uint32_t q = carry_e + __popcll(be & lt);
            const uint32_t fps = (j + 1) - (carry_p + __popcll(bp & lt) + (e.pos ? 1u : 0u));
            const double pro = pro_value(carry_w, incl, K);
            if (q < n) {                                         // q < R <= n always; the guard keeps a bad carry inside the buffers
                w.runfps[q] = fps;
                w.runpro[q] = pro;
                if (c.fps && (int64_t)q < c.cap) {
                    c.fps[q] = (int32_t)fps;
                    c.pro[q] = pro;
                    c.thr[q] = __uint_as_float(e.key >> 1);
                }
            }
        }
        carry_p += __popcll(bp);
        carry_e += __popcll(be);
    }
}

// ------------------------------------------------------------------------------------------------ per run
__global__ __launch_bounds__(WT) void terms_kernel(double *__restrict__ terms, pro_ws w, wide_geom g, double limit)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x, n = g.n;
    const uint32_t R = min(w.hdr[H_R], n), N = n - min(w.hdr[H_P], n);
    const unsigned long long K = *w.K;
    const uint32_t q0 = min(b * g.tile, R), q1 = min(q0 + g.tile, R);    // b * tile < n: no overflow
    const bool live = K != 0 && N != 0;
    const double dN = (double)N;
    for (uint32_t q = q0 + tid; q < q1; q += WT) terms[q] = live ? term_of(w.runfps, w.runpro, q, dN, limit) : 0.0;
}

struct pro_out { double *aupro; int64_t *counts; int32_t *status; int32_t *curve_len; int64_t curve_cap; double limit; };

__global__ __launch_bounds__(64) void finish_kernel(pro_ws w, wide_geom g, pro_out o)
{
    const uint32_t lane = threadIdx.x, n = g.n;
    double part = lane < AP_WAVES ? w.wavesum[lane] : 0.0;
    part = tree_add<AP_WAVES>(part);
    if (lane != 0) return;
    const unsigned long long K = *w.K;
    const uint32_t R = w.hdr[H_R], P = w.hdr[H_P], N = n - P;
    o.aupro[0] = (K == 0 || N == 0) ? (double)NAN : part / o.limit;
    o.counts[0] = (int64_t)K;
    o.counts[1] = N;
    o.counts[2] = P;
    o.counts[3] = R;
    const bool want_curve = o.curve_len != nullptr;
    o.status[0] = (int32_t)(w.hdr[H_ST] | ((want_curve && (int64_t)R > o.curve_cap) ? ANODDPM_ROC_CURVE_TRUNCATED : 0u));
    if (want_curve) o.curve_len[0] = (int32_t)R;
}

}  // namespace

extern "C" int64_t anoddpm_pro_wide_workspace_bytes(int32_t S, int64_t n, int32_t tile)
{
    if (S < 1 || n < 1 || n >= ((int64_t)1 << 31)) return -1;
    int32_t used;
    if (check_tile(n, tile, &used, "pro_wide_workspace_bytes") != ANODDPM_OK) return -1;
    pro_ws w;
    return carve(&w, nullptr, n, alloc_tiles(n, tile));
}

extern "C" int anoddpm_pro_auc_wide(const anoddpm_pro_args *a, int32_t tile, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "pro_auc_wide: null args");
    ANODDPM_REQUIRE(a->score && a->area && a->region_counts && a->workspace && a->aupro && a->counts && a->status, "pro_auc_wide: null pointer");
    ANODDPM_REQUIRE(a->S >= 1, "pro_auc_wide: S must be >= 1");
    ANODDPM_REQUIRE(a->planes_per_segment >= 1 && a->H >= 1 && a->W >= 1, "pro_auc_wide: planes_per_segment, H and W must be >= 1");
    const int64_t hw = (int64_t)a->H * a->W;
    ANODDPM_REQUIRE(hw < ((int64_t)1 << 31) && hw <= (((int64_t)1 << 31) - 1) / a->planes_per_segment,
                    "pro_auc_wide: n = planes_per_segment * H * W must be below 2^31 (32-bit positions)");
    const int64_t n = hw * a->planes_per_segment;
    ANODDPM_REQUIRE(a->limit > 0.0 && a->limit <= 1.0, "pro_auc_wide: limit must be in (0, 1]");
    ANODDPM_REQUIRE(a->S == 1 || a->score_stride >= n, "pro_auc_wide: score segments overlap (score_stride < n)");
    ANODDPM_REQUIRE(a->S == 1 || a->area_stride == 0 || a->area_stride >= n, "pro_auc_wide: area_stride must be 0 (shared mask) or >= n");
    ANODDPM_REQUIRE(!a->mask || a->S == 1 || a->mask_stride == 0 || a->mask_stride >= n, "pro_auc_wide: mask_stride must be 0 (shared mask) or >= n");
    int32_t used;
    if (int rc = check_tile(n, tile, &used, "pro_auc_wide")) return rc;
    ANODDPM_REQUIRE(a->workspace_bytes >= anoddpm_pro_wide_workspace_bytes(a->S, n, tile), "pro_auc_wide: workspace too small");
    ANODDPM_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "pro_auc_wide: workspace must be 16-byte aligned");
    const bool any_curve = a->curve_fps || a->curve_pro || a->curve_thr || a->curve_len;
    if (any_curve) {
        ANODDPM_REQUIRE(a->curve_fps && a->curve_pro && a->curve_thr && a->curve_len, "pro_auc_wide: curve output needs curve_fps, curve_pro, curve_thr and curve_len");
        ANODDPM_REQUIRE(a->curve_cap >= 1, "pro_auc_wide: curve capacity must be >= 1 point per segment");
    }

    hipStream_t s = as_stream(stream);
    wide_geom g;
    g.n = (uint32_t)n;
    g.tile = (uint32_t)used;
    g.T = (uint32_t)((n + used - 1) / used);
    pro_ws w;
    carve(&w, a->workspace, n, alloc_tiles(n, tile));
    const dim3 tiles(g.T), wt(WT), one(1), st(ST);
    for (int32_t seg = 0; seg < a->S; ++seg) {
        const float *score = a->score + (int64_t)seg * a->score_stride;
        const int32_t *area = a->area + (int64_t)seg * a->area_stride;
        const float *mask = a->mask ? a->mask + (int64_t)seg * a->mask_stride : nullptr;
        carry_in in;
        in.region_counts = a->region_counts + (a->area_stride == 0 ? 0 : (int64_t)seg * a->planes_per_segment);
        in.planes = a->planes_per_segment;
        hipLaunchKernelGGL(keys_kernel, tiles, wt, 0, s, score, area, mask, w, g);
        uint32_t *src = w.key0, *dst = w.key1;
        int32_t *psrc = w.pay0, *pdst = w.pay1;
        for (int pass = 0; pass < 4; ++pass) {
            if (pass > 0) hipLaunchKernelGGL(hist_kernel, tiles, wt, 0, s, (const uint32_t *)src, w.table, g, pass * 8);
            hipLaunchKernelGGL(scan_kernel, one, st, 0, s, w.table, w.hdr + H_SKIP + pass, g);
            hipLaunchKernelGGL(scatter_kernel<true>, tiles, wt, 0, s, (const uint32_t *)src, dst, (const int32_t *)psrc, pdst, (const uint32_t *)w.table,
                               (const uint32_t *)(w.hdr + H_SKIP + pass), g, pass * 8);
            uint32_t *t = src;
            src = dst;
            dst = t;
            int32_t *pt = psrc;
            psrc = pdst;
            pdst = pt;
        }                                                        // four swaps: the sorted pairs are in key0 / pay0
        double *terms = reinterpret_cast<double *>(w.key1);     // key1 and pay1 are free from here on
        pro_curve c;
        c.fps = any_curve ? a->curve_fps + (int64_t)seg * a->curve_cap : nullptr;
        c.pro = any_curve ? a->curve_pro + (int64_t)seg * a->curve_cap : nullptr;
        c.thr = any_curve ? a->curve_thr + (int64_t)seg * a->curve_cap : nullptr;
        c.cap = a->curve_cap;
        hipLaunchKernelGGL(walk_count_kernel, tiles, wt, 0, s, (const uint32_t *)src, (const int32_t *)psrc, w, g);
        hipLaunchKernelGGL(walk_carry_kernel, one, dim3(CW), 0, s, w, g, in);
        hipLaunchKernelGGL(walk_write_kernel, tiles, wt, 0, s, (const uint32_t *)src, (const int32_t *)psrc, w, g, c);
        hipLaunchKernelGGL(terms_kernel, tiles, wt, 0, s, terms, w, g, a->limit);
        hipLaunchKernelGGL(lanes_kernel, dim3(AP_WAVES), st, 0, s, (const double *)terms, (const uint32_t *)(w.hdr + H_R), w.wavesum, g.n);
        pro_out o;
        o.aupro = a->aupro + seg;
        o.counts = a->counts + (int64_t)seg * 4;
        o.status = a->status + seg;
        o.curve_len = any_curve ? a->curve_len + seg : nullptr;
        o.curve_cap = a->curve_cap;
        o.limit = a->limit;
        hipLaunchKernelGGL(finish_kernel, one, dim3(64), 0, s, w, g, o);
        if (int rc = check_launch("pro_auc_wide")) return rc;
    }
    return ANODDPM_OK;
}
