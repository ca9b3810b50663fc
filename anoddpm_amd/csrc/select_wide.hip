// Order statistics of ONE long segment spread over the whole chip, and counts at thresholds that live on the device -- the last
// step of an unsupervised evaluation: calibrate an operating threshold on a pool of healthy maps (the value that a chosen share
// of healthy pixels exceeds), then score the test maps at it.  include/anoddpm_hip.h has the contract.
//   anoddpm_select_wide       what anoddpm_map_scores (csrc/smooth.hip) computes with one workgroup per segment, for Q ranks at
//                             once and any n below 2^31, as a sequence of launches with one workgroup per tile of `tile` values
//   anoddpm_threshold_counts  tp / fp of the predictions score > thr[j] for T thresholds read from device memory, one pass
// A launch boundary is the only ordering between workgroups: no kernel below waits for another workgroup, and none reads, within
// a launch, what another workgroup wrote in that launch.  Every loop is bounded by n or by the tile; every store of an output keeps
// its index guard.  Compiled with -ffp-contract=off.  There is no floating-point atomic in this file: counts, status bits and the
// maximum (on its bit pattern) cross workgroups as integer atomics, whose order of arrival cannot show.
//
// Select, per segment (11 launches whatever Q is):
//   clear     one workgroup: the four [Q][256] counter tables and the header (status, maximum) to zero
//   4 x hist  per tile: for every rank the 256-bin histogram of the byte of this pass among the elements that match the rank's
//             prefix so far (LDS integer atomics, the lanes of a wave that share a bin add through one atomic), then one integer
//             add per non-empty bin into the pass's [Q][256] table.  In the first pass no rank has a prefix yet: ONE histogram
//             serves all of them, and the pass also gives the status bits and the maximum.
//   4 x pick  one workgroup, wave q = rank q: the bin that holds the rank (one wave's scan, as map_scores_kernel), the prefix
//             extended by it, the rank that remains inside the bin.  After the last pass the prefix is the value, the rank that
//             remains is r - #{v > value} and the bin's count is #{v == value}.
//   sums      16 workgroups, one per wave of map_scores_kernel: lane l of workgroup v is virtual thread t = 64 v + l of 1024 and
//             adds the elements t, t + 1024, ... in that order, read from the fp32 segment in place.  The sixteen waves of the
//             workgroup fetch rows of 64 elements into LDS; wave q adds the ones above the value of rank q, wave 0 also all of
//             them; then the 64-lane tree (roc_shared.h tree_add).
//   finish    one workgroup: the 16-wave tree of every sum, and the outputs of the segment
// This file states its own kernels: map_scores_kernel's histogram update, scan and sums live in smooth.hip under that kernel's
// thread count and its one-workgroup loop over the whole segment, and sharing them would have meant editing that file.
#include <math.h>
#include "common.h"
#include "roc_shared.h"

namespace {

using namespace anoddpm::roc;                                    // tree_add

constexpr int WT = 256;                                          // workgroup of a tile
constexpr int ST = 1024, SW = ST / 64;                           // workgroup of clear / pick / sums / finish: 16 waves, one per rank
constexpr int MAXQ = ANODDPM_SELECT_MAX_RANKS;
constexpr int LANES = 1024, LANE_WAVES = LANES / 64;             // the workgroup of map_scores_kernel whose summation order is kept
constexpr int STAGE = 128, PER = STAGE / SW;                     // rows of 64 elements staged per round (32 KB of LDS), rows a wave fetches
constexpr int ADD = 16;                                          // staged rows a wave reads from LDS before it adds them
constexpr int BATCH = 8;                                         // loads in flight per thread in the histogram passes
constexpr uint32_t ABS = 0x7fffffffu;                            // -0.0 is +0.0; the order of the patterns is the order of the values
constexpr int32_t MIN_TILE = 1024, MAX_TILE = 16384, WANT_TILES = 2048;
enum { H_STATUS = 0, H_MAX = 1, H_WORDS = 4 };
enum { S_PREFIX = 0, S_RANK = 1, S_EQUAL = 2, S_BAD = 3, S_WORDS = 4 };

static_assert(MAXQ == SW, "pick, sums and finish give every rank a wave of their workgroup");
static_assert(LANE_WAVES == 16, "the trees of roc_shared.h are instantiated for 16 waves");
static_assert(STAGE % SW == 0 && STAGE % ADD == 0, "every wave fetches the same number of rows");

struct sel_ws {                  // one segment's workspace
    double *wavesum;             // [Q + 1][16]: row 0 the sum of all values, row q + 1 the sum of the values above rank q's
    uint32_t *table;             // [4][Q][256]: pass, rank, bin
    uint32_t *state;             // [Q][S_WORDS]
    uint32_t *hdr;               // H_WORDS
};

struct sel_geom { uint32_t n, tile, T; int32_t Q; };

int64_t carve(sel_ws *w, void *base, int32_t Q)
{
    char *p = static_cast<char *>(base);
    int64_t o = 0;
    auto take = [&](int64_t bytes) { char *q = p ? p + o : nullptr; o += (bytes + 15) / 16 * 16; return q; };
    w->wavesum = (double *)take((int64_t)(Q + 1) * LANE_WAVES * 8);
    w->table = (uint32_t *)take((int64_t)4 * Q * 256 * 4);
    w->state = (uint32_t *)take((int64_t)Q * S_WORDS * 4);
    w->hdr = (uint32_t *)take(H_WORDS * 4);
    return o;
}

// tile 0: n / 2048 rounded up to a multiple of 256, at least 1024 and at most 16384 values
int32_t default_tile(int64_t n)
{
    const int64_t t = ((n + WANT_TILES - 1) / WANT_TILES + 255) / 256 * 256;
    return (int32_t)(t < MIN_TILE ? MIN_TILE : (t > MAX_TILE ? MAX_TILE : t));
}

bool tile_ok(int32_t tile) { return tile >= 0 && tile % 256 == 0; }

// ------------------------------------------------------------------------------------------------ select
__global__ __launch_bounds__(ST) void clear_kernel(sel_ws w, sel_geom g)
{
    const uint32_t words = 4u * (uint32_t)g.Q * 256u;
    for (uint32_t i = threadIdx.x; i < words; i += ST) w.table[i] = 0;
    if (threadIdx.x < H_WORDS) w.hdr[threadIdx.x] = 0;
}

// ++hist[bin] for the lanes that `take` (wave-uniform call).  The lanes of a wave that share the first taker's bin add their count
// through one atomic, twice over; what is left adds one by one.  Maps concentrate in a few exponents (and a constant map in one
// pattern), where 64 single adds to one word would queue up behind each other.  Integer counts: the order of the adds cannot show.
__device__ __forceinline__ void hist_add(uint32_t *hist, bool take, uint32_t bin)
{
    const int lane = threadIdx.x & 63;
    unsigned long long left = __ballot(take);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (left == 0) break;                                    // wave-uniform
        const int leader = __ffsll(left) - 1;
        const uint32_t lb = __shfl(bin, leader);
        const bool same = take && bin == lb;
        const unsigned long long group = __ballot(same);
        if (lane == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(group));
        if (same) take = false;
        left &= ~group;
    }
    if (take) atomicAdd(&hist[bin], 1u);
}

// FIRST: the pass of the top byte, no prefix yet: one histogram (row 0 of the table) for every rank, status bits and maximum.
template <bool FIRST>
__global__ __launch_bounds__(WT) void hist_kernel(const float *__restrict__ v, sel_ws w, sel_geom g, int pass)
{
    __shared__ uint32_t hist[MAXQ * 256];
    __shared__ uint32_t s_prefix[MAXQ];
    __shared__ uint32_t s_status, s_max;
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const int rows = FIRST ? 1 : g.Q;                            // 1 <= Q <= MAXQ (host check)
    for (int i = tid; i < rows * 256; i += WT) hist[i] = 0;
    if (tid == 0) { s_status = 0; s_max = 0; }
    if (!FIRST && (int)tid < rows) s_prefix[tid] = w.state[tid * S_WORDS + S_PREFIX];
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t mask = FIRST ? 0u : 0xffffffffu << (shift + 8);   // the bytes above this pass's
    const uint32_t *__restrict__ bits = reinterpret_cast<const uint32_t *>(v);
    const uint32_t i0 = b * g.tile, i1 = min(i0 + g.tile, g.n);  // b * tile < n < 2^31: neither wraps
    uint32_t st = 0, mx = 0;
    for (uint32_t base = i0; base < i1; base += BATCH * WT) {    // every lane of a wave makes the same number of rounds
        uint32_t x[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const uint32_t i = base + u * WT + tid;
            x[u] = bits[min(i, i1 - 1)];                         // always inside the tile (i1 > i0): no branch, the loads overlap
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const bool valid = base + u * WT + tid < i1;         // past the end: the tile's last element again, counted once
            const uint32_t p = x[u] & ABS;
            if (FIRST) {
                const float f = __uint_as_float(x[u]);
                if (f != f) st |= ANODDPM_ROC_NAN;
                else if (f == INFINITY || f == -INFINITY) st |= ANODDPM_ROC_INF;
                if (f < 0.0f) st |= ANODDPM_ROC_NEGATIVE;
                mx = max(mx, p);
                hist_add(hist, valid, p >> 24);
            } else {
                const uint32_t bin = (p >> shift) & 255u;
                for (int q = 0; q < rows; ++q) hist_add(hist + q * 256, valid && (p & mask) == s_prefix[q], bin);
            }
        }
    }
    if (FIRST) {
        if (st) atomicOr(&s_status, st);
        atomicMax(&s_max, mx);
    }
    __syncthreads();
    uint32_t *table = w.table + (size_t)pass * g.Q * 256;
    for (int i = tid; i < rows * 256; i += WT) {
        const uint32_t c = hist[i];
        if (c) atomicAdd(&table[i], c);                          // at most n in all: no wrap
    }
    if (FIRST && tid == 0) {
        if (s_status) atomicOr(&w.hdr[H_STATUS], s_status);
        atomicMax(&w.hdr[H_MAX], s_max);
    }
}

// wave q = rank q.  Lane l owns the bins 4l ... 4l + 3; ranks count from the top bin down.
__global__ __launch_bounds__(ST) void pick_kernel(const uint32_t *__restrict__ ranks, sel_ws w, sel_geom g, int pass)
{
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    if (q >= g.Q) return;
    const int shift = 24 - 8 * pass;
    uint32_t *state = w.state + q * S_WORDS;
    uint32_t prefix = 0, rank;
    if (pass == 0) {
        rank = ranks[q];
        const bool bad = rank >= g.n;
        if (bad) rank = g.n - 1;                                 // outputs unspecified, status bit set; every count stays inside n
        if (lane == 0) state[S_BAD] = bad ? 1u : 0u;
    } else {
        prefix = state[S_PREFIX];
        rank = state[S_RANK];
    }
    const uint32_t *hist = w.table + ((size_t)pass * g.Q + (pass == 0 ? 0 : q)) * 256;
    const uint4 h = reinterpret_cast<const uint4 *>(hist)[lane];
    const uint32_t cnt[4] = {h.x, h.y, h.z, h.w};
    const uint32_t c = h.x + h.y + h.z + h.w;
    uint32_t incl = c;                                           // elements in this lane's bins and in all higher ones
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_down(incl, off);
        if (lane + off < 64) incl += up;
    }
    const uint32_t excl = incl - c;
    if (excl <= rank && rank < incl) {                           // exactly one lane: rank is below the number of elements counted
        int b = 3;
        uint32_t r = rank - excl;
#pragma unroll
        for (int j = 3; j > 0; --j)
            if (b == j && r >= cnt[j]) { r -= cnt[j]; b = j - 1; }
        const uint32_t eq = b == 3 ? cnt[3] : (b == 2 ? cnt[2] : (b == 1 ? cnt[1] : cnt[0]));
        state[S_PREFIX] = prefix | ((4u * lane + (uint32_t)b) << shift);
        state[S_RANK] = r;
        state[S_EQUAL] = eq;
    }
}

// workgroup v = wave v of map_scores_kernel.  Lane l of it is virtual thread t = 64 v + l and adds the elements t, t + 1024, ...
__global__ __launch_bounds__(ST) void sums_kernel(const float *__restrict__ src, sel_ws w, sel_geom g)
{
    __shared__ uint32_t stage[STAGE * 64];
    const uint32_t v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, sub = tid >> 6, n = g.n;
    const uint32_t *__restrict__ bits = reinterpret_cast<const uint32_t *>(src);
    const uint32_t rows = (n + LANES - 1) / LANES;               // <= 2^21
    const bool ranked = (int)sub < g.Q;
    const uint32_t vk = ranked ? w.state[sub * S_WORDS + S_PREFIX] : 0xffffffffu;   // no pattern is above 0xffffffff
    double total = 0.0, part = 0.0;
    uint32_t next[PER];
    auto row_of = [&](uint32_t k0, int u) { return k0 + sub * PER + u; };
    auto fetch = [&](uint32_t k0) {                              // the rows of the next round, in flight while this one is added:
#pragma unroll
        for (int u = 0; u < PER; ++u) {                          // raw words only, nothing here waits for them
            const uint32_t r = row_of(k0, u) * LANES + v * 64 + lane;    // < 2^31 + 2^18
            next[u] = bits[min(r, n - 1)];                       // always inside the segment: no branch, the loads overlap
        }
    };
    fetch(0);
    for (uint32_t k0 = 0; k0 < rows; k0 += STAGE) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const uint32_t k = row_of(k0, u), r = k * LANES + v * 64 + lane;
            stage[(sub * PER + u) * 64 + lane] = (k < rows && r < n) ? next[u] & ABS : 0u;   // + 0.0 leaves a non-negative partial alone
        }
        __syncthreads();
        if (k0 + STAGE < rows) fetch(k0 + STAGE);
        if (ranked || sub == 0) {
            for (int k = 0; k < STAGE; k += ADD) {               // ADD LDS reads in flight, then their additions in row order
                uint32_t p[ADD];
#pragma unroll
                for (int j = 0; j < ADD; ++j) p[j] = stage[(k + j) * 64 + lane];
#pragma unroll
                for (int j = 0; j < ADD; ++j) {
                    const double x = (double)__uint_as_float(p[j]);
                    if (sub == 0) total += x;
                    part += p[j] > vk ? x : 0.0;                 // + 0.0 leaves a non-negative partial alone
                }
            }
        }
        __syncthreads();
    }
    if (ranked) {
        part = tree_add<64>(part);
        if (lane == 0) w.wavesum[(sub + 1) * LANE_WAVES + v] = part;
    }
    if (sub == 0) {
        total = tree_add<64>(total);
        if (lane == 0) w.wavesum[v] = total;
    }
}

struct sel_out {                 // the outputs of this segment
    float *value; int64_t *above, *equal; double *topk_mean;     // [Q]
    float *max; double *mean; int32_t *status;
};

__global__ __launch_bounds__(ST) void finish_kernel(const uint32_t *__restrict__ ranks, sel_ws w, sel_geom g, sel_out o)
{
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    if (q == 0) {
        double total = lane < LANE_WAVES ? w.wavesum[lane] : 0.0;
        total = tree_add<LANE_WAVES>(total);
        if (lane == 0) {
            uint32_t st = w.hdr[H_STATUS];
            for (int j = 0; j < g.Q; ++j)
                if (w.state[j * S_WORDS + S_BAD]) st |= ANODDPM_SELECT_BAD_RANK;
            o.status[0] = (int32_t)st;
            o.max[0] = __uint_as_float(w.hdr[H_MAX]);
            o.mean[0] = total / (double)g.n;
        }
    }
    if (q >= g.Q) return;
    double part = lane < LANE_WAVES ? w.wavesum[(q + 1) * LANE_WAVES + lane] : 0.0;
    part = tree_add<LANE_WAVES>(part);
    if (lane == 0) {
        const uint32_t *state = w.state + q * S_WORDS;
        const uint32_t r = min(ranks[q], g.n - 1), k = r + 1u;   // a bad rank was selected as n - 1
        const uint32_t above = r - min(state[S_RANK], r);        // the rank that remains inside the last bin is r - #{v > value}
        const float value = __uint_as_float(state[S_PREFIX]);
        o.value[q] = value;
        o.above[q] = above;
        o.equal[q] = state[S_EQUAL];
        const double rest = (double)(k - above) * (double)value;
        o.topk_mean[q] = (part + rest) / (double)k;
    }
}

// ------------------------------------------------------------------------------------------------ counts at thresholds
constexpr int TC_TILE = 4096, TC_MAX = ANODDPM_THRESHOLD_COUNTS_MAX;

__global__ __launch_bounds__(WT) void tc_clear_kernel(anoddpm_threshold_counts_args a)
{
    const int64_t i = (int64_t)blockIdx.x * WT + threadIdx.x;
    if (i < (int64_t)a.S * a.T * 2) a.counts[i] = 0;
    if (i < (int64_t)a.S * 2) a.totals[i] = 0;
    if (i < a.S) a.status[i] = 0;
}

__global__ __launch_bounds__(WT) void tc_kernel(anoddpm_threshold_counts_args a, uint32_t tiles)
{
    __shared__ uint32_t s_pred[TC_MAX], s_tp[TC_MAX], s_pos, s_status;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const int64_t s = blockIdx.x / tiles;
    const uint32_t t = blockIdx.x % tiles, n = (uint32_t)a.n;
    const int T = a.T;                                           // 1 <= T <= TC_MAX (host check)
    if (tid < TC_MAX) { s_pred[tid] = 0; s_tp[tid] = 0; }
    if (tid == 0) { s_pos = 0; s_status = 0; }
    __syncthreads();
    const float *__restrict__ score = a.score + s * a.score_stride;
    const float *__restrict__ mask = a.mask + s * a.mask_stride;
    const float *__restrict__ thr = a.thr + s * a.thr_stride;
    float th[TC_MAX];
#pragma unroll
    for (int j = 0; j < TC_MAX; ++j) th[j] = j < T ? thr[j] : NAN;   // nothing is above NaN
    uint32_t pred[TC_MAX], tp[TC_MAX], pos = 0, st = 0;
#pragma unroll
    for (int j = 0; j < TC_MAX; ++j) { pred[j] = 0; tp[j] = 0; }
    const uint32_t i0 = t * TC_TILE, i1 = min(i0 + TC_TILE, n);  // t * TC_TILE < n < 2^31
    for (uint32_t i = i0 + tid; i < i1; i += WT) {
        const float x = score[i], m = mask[i];
        if (x != x) st |= ANODDPM_ROC_NAN;
        if (!(m == 0.0f || m == 1.0f)) st |= ANODDPM_ROC_BAD_MASK;
        const uint32_t p = m != 0.0f ? 1u : 0u;
        pos += p;
#pragma unroll
        for (int j = 0; j < TC_MAX; ++j) {
            const uint32_t hit = x > th[j] ? 1u : 0u;            // strict; false for a NaN score
            pred[j] += hit;
            tp[j] += hit & p;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        pos += __shfl_xor(pos, off);
        st |= __shfl_xor(st, off);
#pragma unroll
        for (int j = 0; j < TC_MAX; ++j) {
            pred[j] += __shfl_xor(pred[j], off);
            tp[j] += __shfl_xor(tp[j], off);
        }
    }
    if (lane == 0) {
        atomicAdd(&s_pos, pos);
        if (st) atomicOr(&s_status, st);
#pragma unroll
        for (int j = 0; j < TC_MAX; ++j) {
            if (pred[j]) atomicAdd(&s_pred[j], pred[j]);
            if (tp[j]) atomicAdd(&s_tp[j], tp[j]);
        }
    }
    __syncthreads();
    if ((int)tid < T) {                                          // integer adds: the order of the workgroups cannot show
        unsigned long long *c = reinterpret_cast<unsigned long long *>(a.counts + (s * T + tid) * 2);
        if (s_tp[tid]) atomicAdd(&c[0], (unsigned long long)s_tp[tid]);
        if (s_pred[tid] - s_tp[tid]) atomicAdd(&c[1], (unsigned long long)(s_pred[tid] - s_tp[tid]));
    }
    if (tid == 64) {
        unsigned long long *c = reinterpret_cast<unsigned long long *>(a.totals + s * 2);
        if (s_pos) atomicAdd(&c[0], (unsigned long long)s_pos);
        if ((i1 - i0) - s_pos) atomicAdd(&c[1], (unsigned long long)((i1 - i0) - s_pos));
        if (s_status) atomicOr(&a.status[s], (int)s_status);
    }
}

}  // namespace

extern "C" int64_t anoddpm_select_wide_workspace_bytes(int64_t n, int32_t Q, int32_t tile)
{
    if (n < 1 || n >= ((int64_t)1 << 31) || Q < 1 || Q > MAXQ || !tile_ok(tile)) return -1;
    sel_ws w;
    return carve(&w, nullptr, Q);
}

extern "C" int anoddpm_select_wide(const anoddpm_select_args *a, int32_t tile, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "select_wide: null args");
    ANODDPM_REQUIRE(a->src && a->ranks && a->workspace && a->value && a->above && a->equal && a->topk_mean && a->max && a->mean && a->status,
                    "select_wide: null pointer");
    ANODDPM_REQUIRE(a->S >= 1, "select_wide: S must be >= 1");
    ANODDPM_REQUIRE(a->n >= 1 && a->n < ((int64_t)1 << 31), "select_wide: n must be in 1 ... 2^31 - 1 (32-bit positions and counts)");
    ANODDPM_REQUIRE(a->Q >= 1 && a->Q <= MAXQ, "select_wide: Q must be in 1 ... %d", MAXQ);
    ANODDPM_REQUIRE(tile_ok(tile), "select_wide: tile must be a multiple of 256, or 0 for the default");
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= a->n, "select_wide: segments overlap (src_stride < n)");
    ANODDPM_REQUIRE(a->workspace_bytes >= anoddpm_select_wide_workspace_bytes(a->n, a->Q, tile), "select_wide: workspace too small");
    ANODDPM_REQUIRE((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "select_wide: workspace must be 16-byte aligned");
    if (a->ranks_host)
        for (int32_t q = 0; q < a->Q; ++q)
            ANODDPM_REQUIRE((int64_t)a->ranks_host[q] < a->n, "select_wide: rank %u (entry %d of ranks_host) is not below n", (unsigned)a->ranks_host[q], (int)q);

    hipStream_t s = as_stream(stream);
    const int32_t used = tile == 0 ? default_tile(a->n) : tile;
    sel_geom g;
    g.n = (uint32_t)a->n;
    g.tile = (uint32_t)used;
    g.T = (uint32_t)((a->n + used - 1) / used);                  // <= 2^23
    g.Q = a->Q;
    sel_ws w;
    carve(&w, a->workspace, a->Q);
    const dim3 tiles(g.T), wt(WT), one(1), st(ST);
    for (int32_t seg = 0; seg < a->S; ++seg) {
        const float *src = a->src + (int64_t)seg * (a->S == 1 ? 0 : a->src_stride);
        hipLaunchKernelGGL(clear_kernel, one, st, 0, s, w, g);
        for (int pass = 0; pass < 4; ++pass) {
            if (pass == 0) hipLaunchKernelGGL(hist_kernel<true>, tiles, wt, 0, s, src, w, g, pass);
            else hipLaunchKernelGGL(hist_kernel<false>, tiles, wt, 0, s, src, w, g, pass);
            hipLaunchKernelGGL(pick_kernel, one, st, 0, s, a->ranks, w, g, pass);
        }
        hipLaunchKernelGGL(sums_kernel, dim3(LANE_WAVES), st, 0, s, src, w, g);
        sel_out o;
        o.value = a->value + (int64_t)seg * a->Q;
        o.above = a->above + (int64_t)seg * a->Q;
        o.equal = a->equal + (int64_t)seg * a->Q;
        o.topk_mean = a->topk_mean + (int64_t)seg * a->Q;
        o.max = a->max + seg;
        o.mean = a->mean + seg;
        o.status = a->status + seg;
        hipLaunchKernelGGL(finish_kernel, one, st, 0, s, a->ranks, w, g, o);
        if (int rc = check_launch("select_wide")) return rc;
    }
    return ANODDPM_OK;
}

extern "C" int anoddpm_threshold_counts(const anoddpm_threshold_counts_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "threshold_counts: null args");
    ANODDPM_REQUIRE(a->score && a->mask && a->thr && a->counts && a->totals && a->status, "threshold_counts: null pointer");
    ANODDPM_REQUIRE(a->S >= 1, "threshold_counts: S must be >= 1");
    ANODDPM_REQUIRE(a->n >= 1 && a->n < ((int64_t)1 << 31), "threshold_counts: n must be in 1 ... 2^31 - 1");
    ANODDPM_REQUIRE(a->T >= 1 && a->T <= TC_MAX, "threshold_counts: T must be in 1 ... %d", TC_MAX);
    ANODDPM_REQUIRE(a->S == 1 || a->score_stride >= a->n, "threshold_counts: score segments overlap (score_stride < n)");
    ANODDPM_REQUIRE(a->S == 1 || a->mask_stride == 0 || a->mask_stride >= a->n, "threshold_counts: mask_stride must be 0 (shared mask) or >= n");
    ANODDPM_REQUIRE(a->S == 1 || a->thr_stride == 0 || a->thr_stride >= a->T, "threshold_counts: thr_stride must be 0 (shared table) or >= T");
    const int64_t tiles = (a->n + TC_TILE - 1) / TC_TILE;
    ANODDPM_REQUIRE(tiles <= 0x7fffffff / (int64_t)a->S, "threshold_counts: S * tiles must be below 2^31");
    anoddpm_threshold_counts_args k = *a;
    if (k.S == 1) k.score_stride = k.mask_stride = k.thr_stride = 0;
    hipStream_t s = as_stream(stream);
    const int64_t words = (int64_t)k.S * k.T * 2;
    hipLaunchKernelGGL(tc_clear_kernel, dim3((unsigned)((words + WT - 1) / WT)), dim3(WT), 0, s, k);
    hipLaunchKernelGGL(tc_kernel, dim3((unsigned)(k.S * tiles)), dim3(WT), 0, s, k, (uint32_t)tiles);
    return check_launch("threshold_counts");
}
