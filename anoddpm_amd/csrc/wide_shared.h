// What csrc/roc_wide.hip (pooled ROC / PR) and csrc/pro_wide.hip (pooled AUPRO) both launch, stated once: the geometry of a segment
// cut into tiles, one LSD radix pass over the whole chip (hist, scan, scatter) and the 1024-lane fp64 sum that ends both files.
//   hist     per tile: the histogram of the pass's digit (LDS integer atomics) into the digit-major [256][tiles] counter table
//   scan     one workgroup: exclusive scan of the table in (digit, tile) order; a pass in which the WHOLE segment has one digit
//            sets the pass's skip flag
//   scatter  per tile: its waves own contiguous chunks, rank among equal digits from ballots (stable); a skipped pass copies the
//            tile, so the sorted keys always end in the first buffer.  Templated on "has a payload": the key-only instantiation
//            (roc_wide.hip) holds no payload load, register or store; with a payload (pro_wide.hip) the int32 word of an element
//            goes to the position of its key in the same pass, through ping-pong buffers of its own.
//   lanes    16 workgroups, one per wave of the one-workgroup kernels' last step: virtual lane t of 1024 adds the terms t,
//            t + 1024, ... in that order, then the 64-lane tree (roc_shared.h tree_add)
// hist and scan see neither payload nor mask.  A launch boundary is the only ordering between workgroups; every loop is bounded
// by n or by the tile count; every scatter store keeps the pos < n guard.  The kernels live in an unnamed namespace: each file that
// includes this header compiles its own copies.
#pragma once
#include "common.h"
#include "roc_shared.h"

namespace anoddpm {
namespace wide {
namespace {

using namespace anoddpm::roc;

constexpr int WT = 256, WW = WT / 64, RADIX = 256, UNROLL = 4;   // workgroup of a tile: one thread per digit
constexpr int ST = 1024, SW = ST / 64;                           // workgroup of the table scan and of the lane sum
constexpr int AP_LANES = 1024, AP_WAVES = AP_LANES / 64;         // the workgroup of roc.hip / pro.hip whose summation order is kept
constexpr int AP_STAGE = 64;                                     // rows of 64 terms staged per round
constexpr int32_t MAX_TILES = ANODDPM_ROC_WIDE_MAX_TILES, DEFAULT_TILE = 4096;

static_assert(2 * ST == MAX_TILES, "scan_kernel: one thread owns two rows of the counter table");
static_assert(AP_WAVES == 16 && SW == 16, "the trees of roc_shared.h are instantiated for 16 waves");

struct wide_geom { uint32_t n, tile, T; };

int32_t default_tile(int64_t n)
{
    const int64_t per = (n + MAX_TILES - 1) / MAX_TILES;
    const int64_t t = (per + 255) / 256 * 256;
    return (int32_t)(t > DEFAULT_TILE ? t : DEFAULT_TILE);
}

// tiles the workspace is sized for: with the default tile a count that never shrinks as n grows
int64_t alloc_tiles(int64_t n, int32_t tile)
{
    if (tile == 0) {
        const int64_t t = (n + DEFAULT_TILE - 1) / DEFAULT_TILE;
        return t < MAX_TILES ? t : MAX_TILES;
    }
    return (n + tile - 1) / tile;
}

int check_tile(int64_t n, int32_t tile, int32_t *used, const char *who)
{
    ANODDPM_REQUIRE(tile >= 0 && tile % WT == 0, "%s: tile must be a multiple of 256, or 0 for the default", who);
    const int32_t t = tile == 0 ? default_tile(n) : tile;
    ANODDPM_REQUIRE((n + t - 1) / t <= MAX_TILES, "%s: tile %d cuts n into more than %d tiles", who, (int)tile, (int)MAX_TILES);
    *used = t;
    return ANODDPM_OK;
}

__global__ __launch_bounds__(WT) void hist_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ table, wide_geom g, int shift)
{
    __shared__ uint32_t hist[RADIX];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    const uint32_t i0 = b * g.tile, i1 = min(i0 + g.tile, g.n);
    for (uint32_t i = i0 + tid; i < i1; i += WT) atomicAdd(&hist[(src[i] >> shift) & 255u], 1u);
    __syncthreads();
    table[tid * g.T + b] = hist[tid];
}

// one workgroup: table[0 .. 256 T) -> its exclusive prefix, in place; *skip = the whole segment has one digit in this pass.
// The table is T rows of 256 words, one 16-byte load per lane: a wave sums its rows, the row totals are scanned in LDS, and a
// second sweep writes each row's prefix -- five barriers however long the table is.
__global__ __launch_bounds__(ST) void scan_kernel(uint32_t *table, uint32_t *skip, wide_geom g)
{
    __shared__ uint32_t rowsum[MAX_TILES];
    __shared__ uint32_t wsum[SW];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = g.T;     // T <= MAX_TILES rows
    uint4 *rows = reinterpret_cast<uint4 *>(table);
    if (tid == 0) *skip = 0;
#pragma unroll 4
    for (uint32_t row = wave; row < T; row += SW) {
        const uint4 v = rows[row * 64 + lane];
        uint32_t sum = v.x + v.y + v.z + v.w;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) rowsum[row] = sum;
    }
    __syncthreads();
    {
        const uint32_t r0 = 2 * tid;                             // 2 * ST = MAX_TILES: every row has an owner
        const uint32_t a = r0 < T ? rowsum[r0] : 0u, b = r0 + 1 < T ? rowsum[r0 + 1] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<SW>(a + b, wsum, total);
        if (r0 < T) rowsum[r0] = ex;
        if (r0 + 1 < T) rowsum[r0 + 1] = ex + a;
    }
    __syncthreads();
#pragma unroll 4
    for (uint32_t row = wave; row < T; row += SW) {
        const uint4 v = rows[row * 64 + lane];
        const uint32_t sum = v.x + v.y + v.z + v.w;
        uint32_t incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        uint4 o;
        o.x = rowsum[row] + incl - sum;
        o.y = o.x + v.x;
        o.z = o.y + v.y;
        o.w = o.z + v.z;
        rows[row * 64 + lane] = o;
    }
    __syncthreads();                                             // this workgroup's own stores, read back below
    if (tid < RADIX) {
        const uint32_t end = tid == RADIX - 1 ? g.n : table[(tid + 1) * T];
        if (end - table[tid * T] == g.n) *skip = 1;              // at most one digit can hold every key
    }
}

// psrc / pdst: the payload's ping-pong buffers; never read without a payload (the key-only launch passes null pointers)
template <bool PAYLOAD>
__global__ __launch_bounds__(WT) void scatter_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, const int32_t *__restrict__ psrc,
                                                     int32_t *__restrict__ pdst, const uint32_t *__restrict__ table, const uint32_t *__restrict__ skip,
                                                     wide_geom g, int shift)
{
    __shared__ uint32_t hist[WW * RADIX];                        // wave-private rows: digit counts, then scatter offsets
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = g.n;
    const uint32_t i0 = b * g.tile, i1 = min(i0 + g.tile, n);
    if (*skip != 0) {                                            // written by the scan launch: uniform over the grid
        for (uint32_t i = i0 + tid; i < i1; i += WT) {
            dst[i] = src[i];
            if constexpr (PAYLOAD) pdst[i] = psrc[i];
        }
        return;
    }
    const uint64_t lt = (1ull << lane) - 1ull;
    const uint32_t chunk = g.tile / WW;                          // a multiple of 64
    const uint32_t c0 = min(i0 + wave * chunk, i1), c1 = min(c0 + chunk, i1);
    for (int i = tid; i < WW * RADIX; i += WT) hist[i] = 0;
    __syncthreads();
    uint32_t *wh = hist + wave * RADIX;
    for (uint32_t i = c0 + lane; i < c1; i += 64) atomicAdd(&wh[(src[i] >> shift) & 255u], 1u);
    __syncthreads();
    {
        uint32_t ex = table[tid * g.T + b];                      // thread = digit: where this tile's keys of the digit begin
#pragma unroll
        for (int k = 0; k < WW; ++k) {
            const uint32_t h = hist[k * RADIX + tid];
            hist[k * RADIX + tid] = ex;
            ex += h;
        }
    }
    __syncthreads();
    for (uint32_t base = c0; base < c1; base += 64 * UNROLL) {
        uint32_t key[UNROLL];
        int32_t word[PAYLOAD ? UNROLL : 1];
        bool valid[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t i = base + u * 64 + lane;
            valid[u] = i < c1;
            key[u] = valid[u] ? src[i] : 0u;
            if constexpr (PAYLOAD) word[u] = valid[u] ? psrc[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (base + u * 64 >= c1) break;                      // wave-uniform
            const uint32_t dg = (key[u] >> shift) & 255u;
            const uint64_t m = digit_peers(dg, valid[u]);
            const uint32_t rank = __popcll(m & lt), cnt = __popcll(m);
            uint32_t pos = 0;
            if (valid[u]) pos = wh[dg] + rank;
            wave_sync();
            if (valid[u] && rank == cnt - 1) wh[dg] = pos + 1;
            wave_sync();
            if (valid[u] && pos < n) {                           // pos < n always; the guard keeps a bad offset inside the buffers
                dst[pos] = key[u];
                if constexpr (PAYLOAD) pdst[pos] = word[u];
            }
        }
    }
}

// workgroup v = wave v of the one-workgroup kernel's last step.  Lane l of it is virtual lane t = 64 v + l and adds the terms t,
// t + 1024, ... of terms[0 .. min(*count, n)) in that order; the sixteen waves here only fetch AP_STAGE rows of those terms into
// LDS, wave 0 adds them row by row.  wavesum[v] = the 64-lane tree of its partials.
__global__ __launch_bounds__(ST) void lanes_kernel(const double *__restrict__ terms, const uint32_t *__restrict__ count, double *__restrict__ wavesum, uint32_t n)
{
    __shared__ double stage[AP_STAGE * 64];
    const uint32_t v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, sub = tid >> 6;
    const uint32_t R = min(*count, n);
    const uint32_t rows = (R + AP_LANES - 1) / AP_LANES;         // <= 2^21
    constexpr int PER = AP_STAGE / SW;
    double part = 0.0, next[PER];
    auto fetch = [&](uint32_t k0) {                              // the rows of the next round, in flight while wave 0 adds this one
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const uint32_t k = k0 + sub * PER + u;
            const uint32_t r = k * AP_LANES + v * 64 + lane;     // < 2^31 + 2^18
            next[u] = (k < rows && r < R) ? terms[r] : 0.0;      // + 0.0 leaves a non-negative partial alone
        }
    };
    fetch(0);
    for (uint32_t k0 = 0; k0 < rows; k0 += AP_STAGE) {
#pragma unroll
        for (int u = 0; u < PER; ++u) stage[(sub * PER + u) * 64 + lane] = next[u];
        __syncthreads();
        if (k0 + AP_STAGE < rows) fetch(k0 + AP_STAGE);
        if (sub == 0)
            for (int k = 0; k < AP_STAGE; ++k) part += stage[k * 64 + lane];
        __syncthreads();
    }
    if (sub == 0) {
        part = tree_add<64>(part);
        if (lane == 0) wavesum[v] = part;
    }
}

}  // namespace
}  // namespace wide
}  // namespace anoddpm
