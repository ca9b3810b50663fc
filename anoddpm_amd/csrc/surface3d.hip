// Exact Euclidean distance transform and boundary distances (Hausdorff, HD95, average symmetric surface distance) of batched
// D x H x W volumes in voxel units -- replaces, per volume or per pair of volumes,
//   scipy.ndimage.distance_transform_edt(vol > level)                                              anoddpm_distance_transform3d
//   m & ~scipy.ndimage.binary_erosion(m) twice + distance_transform_edt twice + numpy.percentile   anoddpm_surface_distance3d
// (include/anoddpm_hip.h has the contract; csrc/surface.hip is the plane form, csrc/surface_shared.h what the two share).  Every
// distance is an integer squared distance until its one fp64 square root: the same bits every launch and wherever a volume sits.
//
// The transform is separable over three axes.  With g(z, y, x) the distance from (z, y, x) to the nearest zero of its z column,
//   h2(z, y, x) = min over y' of (y - y')^2 + g(z, y', x)^2        and        d2(z, y, x) = min over x' of (x - x')^2 + h2(z, y, x').
//   z sweep   column_kernel over the volume seen as D rows of H * W columns: g^2, FAR where the column has no zero
//   y pass    one workgroup per (volume, z, 64 columns): lanes on consecutive x, the four waves on y, y + 4, ...; a thread walks
//             y' = y -+ k while k^2 < best (`nearest` with the row stride as its step), so every step of a wave is one 256-byte
//             row segment.  Up to Y_LDS rows the H x 64 tile is staged in LDS first, above that it is read through L2.  It reads
//             a whole y column of its input, so it writes a SECOND buffer, never in place.
//   x pass    dt_row_kernel over S * D * H rows.
// (D - 1)^2 + (H - 1)^2 + (W - 1)^2 < 2^31 keeps every partial sum inside 31 bits; k^2 < best <= FAR keeps k^2 + FAR inside 32.
//
// Surface distances.  The border of a mask is its foreground with one of the 6 face neighbours background or outside the volume
// (D = 1: both z neighbours are outside, every foreground voxel is border); the transform runs with the BORDER as its zero set:
//   border    one thread per voxel of every prediction and every reference volume (one when it is shared): 0 / 1 into buffer A
//   z sweep   in place in A;   y pass   A -> B.  B is 0 exactly on the border voxels.
//   x pass    one workgroup per (pair, direction, z, y) row: counts the row's own border voxels into cnt[]; a row without one
//             ends there, the others search the other side's row of B and write d^2 at the own border voxels, -1 elsewhere,
//             into A (dead since the y pass)
//   scan      one workgroup per pair: exclusive prefix sums of its 2 * D * H row counts, direction 1 behind direction 0
//   pack      one wave per row with a count: its d^2 values to B (dead since the x pass) at the row's offset, in x order -- the
//             pair's list is then in (direction, voxel index) order, its rank order
//   stats     one workgroup of 1024 threads per pair, on the packed list only: thread t adds sqrt(d2) of the ranks t, t + 1024,
//             ... of a direction in that order, the two halving trees fold the partials; the percentiles are selected on the
//             list.  Beyond the dense passes the work per pair grows with its border voxels and its rows, not with its voxels.
// Seven launches whatever the batch (the transform alone: three); integer atomics only (the LDS histogram of the select); no
// allocation, no host synchronisation.  Compiled with -ffp-contract=off.
#include "surface_shared.h"

#ifndef ANODDPM_SURFACE3D_Y_LDS
#define ANODDPM_SURFACE3D_Y_LDS 128                                  // rows of the y pass's LDS tile (x 64 columns x 4 bytes = 32 KB)
#endif

namespace {

constexpr int Y_COLS = 64, Y_LDS = ANODDPM_SURFACE3D_Y_LDS;
static_assert(Y_LDS >= 1 && Y_LDS * Y_COLS * 4 <= 65536, "the y tile is a static __shared__ array");

// ---------------------------------------------------------------------------------------------------- y pass
// blockIdx.x = (volume * D + z) * xtiles + xtile; in and out are [volumes][D][H][W] and must not overlap.
__global__ __launch_bounds__(THREADS) void y_pass_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int H, int W, int xtiles)
{
    __shared__ uint32_t tile[Y_LDS * Y_COLS];
    const int lane = threadIdx.x & (Y_COLS - 1), wave = threadIdx.x / Y_COLS;
    const int64_t slice = blockIdx.x / (unsigned)xtiles;
    const int x0 = (int)(blockIdx.x % (unsigned)xtiles) * Y_COLS, x = x0 + lane;
    const int64_t base = slice * H * W;
    const bool staged = H <= Y_LDS;                                  // block-uniform
    if (staged) {
        for (int y = wave; y < H; y += THREADS / Y_COLS) tile[y * Y_COLS + lane] = x < W ? in[base + (int64_t)y * W + x] : FAR;
        __syncthreads();
    }
    if (x >= W) return;
    const uint32_t *col = staged ? tile + lane : in + base + x;
    const int64_t stride = staged ? Y_COLS : W;
    for (int y = wave; y < H; y += THREADS / Y_COLS) out[base + (int64_t)y * W + x] = nearest(col, y, H, stride);
}

// ---------------------------------------------------------------------------------------------------- border
// blockIdx.x = volume * bpv + block of the volume; volumes 0 ... S - 1 are the predictions, the references follow.
__global__ __launch_bounds__(THREADS) void border3d_kernel(anoddpm_surface3d_args a, int shared_ref, uint32_t *__restrict__ g2, int bpv)
{
    const int D = a.D, H = a.H, W = a.W;
    const int64_t hw = (int64_t)H * W, n = hw * D;
    const int q = (int)(blockIdx.x / (unsigned)bpv);
    const int64_t p = (int64_t)(blockIdx.x % (unsigned)bpv) * THREADS + threadIdx.x;
    if (p >= n) return;
    const float *__restrict__ src = q < a.S ? a.pred + (int64_t)q * a.pred_stride : a.ref + (shared_ref ? 0 : (int64_t)(q - a.S) * a.ref_stride);
    const int z = (int)(p / hw), y = (int)((p - z * hw) / W), x = (int)(p - z * hw - (int64_t)y * W);
    bool border = false;
    if (src[p] > a.level) {
        const bool inner = x > 0 && x + 1 < W && y > 0 && y + 1 < H && z > 0 && z + 1 < D &&
                           src[p - 1] > a.level && src[p + 1] > a.level && src[p - W] > a.level && src[p + W] > a.level &&
                           src[p - hw] > a.level && src[p + hw] > a.level;
        border = !inner;
    }
    g2[(int64_t)q * n + p] = border ? 0u : 1u;
}

// ---------------------------------------------------------------------------------------------------- x pass of a surface run
// blockIdx.x = (pair * 2 + direction) * rows + row, rows = D * H.  h2 is buffer B ([volumes][rows][W], 0 on the border voxels),
// d2 buffer A seen as [pair][direction][rows][W].
__global__ __launch_bounds__(THREADS) void surface3d_row_kernel(const uint32_t *__restrict__ h2, int32_t *__restrict__ d2,
                                                                uint32_t *__restrict__ cnt, int S, int shared_ref, int rows, int W)
{
    __shared__ uint32_t tile[ROW_LDS];
    __shared__ uint32_t wsum[THREADS / 64];
    const int64_t row = blockIdx.x % (unsigned)rows;
    const int dir = (int)((blockIdx.x / (unsigned)rows) & 1u);
    const int s = (int)(blockIdx.x / (2u * (unsigned)rows));
    const int64_t n = (int64_t)rows * W, off = row * W;
    const uint32_t *hp = h2 + (int64_t)s * n + off;
    const uint32_t *hr = h2 + (int64_t)(S + (shared_ref ? 0 : s)) * n + off;
    const uint32_t *__restrict__ own = dir == 0 ? hp : hr;
    const uint32_t *__restrict__ other = dir == 0 ? hr : hp;
    uint32_t mine = 0;
    for (int x = threadIdx.x; x < W; x += THREADS) mine += own[x] == 0u ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = mine;
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) total += wsum[w];
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
    if (total == 0) return;                                          // block-uniform: nothing of this row is ever read
    int32_t *__restrict__ out = d2 + (int64_t)blockIdx.x * W;
    const uint32_t *r = stage_row(other, tile, W);
    for (int x = threadIdx.x; x < W; x += THREADS)
        out[x] = own[x] == 0u ? (int32_t)min(nearest(r, x, W), FAR) : -1;
}

// ---------------------------------------------------------------------------------------------------- scan of the row counts
// One workgroup per pair: off[] = the exclusive prefix sums of its R = 2 * rows counts (direction 1 follows direction 0),
// tot[pair] = {n0, n1}.  Thread t sums the counts [t * per, (t + 1) * per); a Hillis-Steele scan in LDS orders the 1024 partials.
__global__ __launch_bounds__(STAT_THREADS) void surface3d_scan_kernel(const uint32_t *__restrict__ cnt, uint32_t *__restrict__ off,
                                                                      uint32_t *__restrict__ tot, int rows)
{
    __shared__ uint32_t part[STAT_THREADS];
    const int tid = threadIdx.x;
    const int64_t R = 2 * (int64_t)rows, base = (int64_t)blockIdx.x * R;
    const int64_t per = (R + STAT_THREADS - 1) / STAT_THREADS, lo = tid * per < R ? tid * per : R, hi = lo + per < R ? lo + per : R;
    uint32_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += cnt[base + i];
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < STAT_THREADS; o <<= 1) {
        const uint32_t add = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    uint32_t run = part[tid] - sum;                                  // exclusive
    for (int64_t i = lo; i < hi; ++i) {
        if (i == rows) tot[(int64_t)blockIdx.x * 2] = run;           // where direction 1 begins: n0
        off[base + i] = run;
        run += cnt[base + i];
    }
    if (tid == STAT_THREADS - 1) tot[(int64_t)blockIdx.x * 2 + 1] = part[tid];   // n0 + n1 until the statistics launch reads it
}

// ---------------------------------------------------------------------------------------------------- pack
// One wave per (pair, direction, row): the row's d^2 values >= 0 to packed[pair] + off[row], in x order.
__global__ __launch_bounds__(THREADS) void surface3d_pack_kernel(const int32_t *__restrict__ d2, const uint32_t *__restrict__ cnt,
                                                                 const uint32_t *__restrict__ off, uint32_t *__restrict__ packed,
                                                                 int64_t all_rows, int rows, int W)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);       // wave-uniform
    if (g >= all_rows || cnt[g] == 0u) return;
    const int64_t pair = g / (2 * (int64_t)rows);
    const int32_t *__restrict__ src = d2 + g * W;
    uint32_t *__restrict__ dst = packed + pair * 2 * rows * W + off[g];
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t run = 0;
    for (int x0 = 0; x0 < W; x0 += 64) {                             // wave-uniform trip count: ballots inside
        const int32_t w = x0 + lane < W ? src[x0 + lane] : -1;
        const unsigned long long take = __ballot(w >= 0);
        if (w >= 0) dst[run + (uint32_t)__popcll(take & below)] = (uint32_t)w;
        run += (uint32_t)__popcll(take);
    }
}

// ---------------------------------------------------------------------------------------------------- per-pair statistics
__global__ __launch_bounds__(STAT_THREADS) void surface3d_stats_kernel(anoddpm_surface3d_args a, const uint32_t *__restrict__ packed_all,
                                                                       const uint32_t *__restrict__ tot)
{
    __shared__ uint32_t hist[256], sel[2], s_n[2];
    __shared__ PairFold fold;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int64_t n = (int64_t)a.D * a.H * a.W;
    const uint32_t *packed = packed_all + (int64_t)s * 2 * n;
    const uint32_t c0 = tot[(int64_t)s * 2], c1 = tot[(int64_t)s * 2 + 1] - c0;
    uint32_t cnt[2] = {0, 0};
    int32_t mx[2] = {-1, -1};
    double sum[2] = {0.0, 0.0};
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const uint32_t *v = packed + (d ? c0 : 0u);
        const uint32_t m = d ? c1 : c0;
        for (uint32_t i = tid; i < m; i += STAT_THREADS) {           // ranks t, t + 1024, ... in that order
            const int32_t w = (int32_t)v[i];
            ++cnt[d];
            mx[d] = max(mx[d], w);
            sum[d] += sqrt((double)w);
        }
    }
    fold_pair(cnt, mx, sum, fold);
    if (tid == 0) finish_pair(s, cnt, mx, sum, a.counts, a.max2, a.mean, a.p95, a.status, s_n);
    __syncthreads();
    const uint32_t n0 = s_n[0], n1 = s_n[1];
    if (n0 == 0) return;                                             // block-uniform: an empty border on either side
    write_percentiles(packed, n0, n1, a.p95 + (int64_t)s * 3, hist, sel);
}

// ---------------------------------------------------------------------------------------------------- host side
constexpr int64_t LIMIT = (int64_t)1 << 31;

// extents >= 1, one volume indexable and every squared distance below 2^31
bool volume_ok(int32_t S, int32_t D, int32_t H, int32_t W)
{
    if (S < 1 || D < 1 || H < 1 || W < 1) return false;
    if ((int64_t)D * H >= LIMIT || (int64_t)D * H * W >= LIMIT) return false;
    const int64_t dz = D - 1, dy = H - 1, dx = W - 1;
    return dz * dz + dy * dy + dx * dx < LIMIT;
}

int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// every grid of a run over `volumes` volumes stays below 2^31 workgroups (the largest have one workgroup per row or per 256 voxels)
bool grids_ok(int64_t volumes, int32_t D, int32_t H, int32_t W)
{
    const int64_t n = (int64_t)D * H * W;
    for (int64_t grid : {volumes * D * H, volumes * cdiv(n, THREADS), volumes * D * cdiv(W, Y_COLS), cdiv(volumes * H * W, THREADS)})
        if (grid >= LIMIT) return false;
    return true;
}

// Per-launch HIP events for tools/bench_surface3d.py (anoddpm_internal_surface3d_profile below; not part of the public ABI): while
// switched on, an entry point records event i in front of its launch i and one behind the last.  Off in normal operation.
constexpr int MAX_MARKS = 8;
hipEvent_t g_marks[MAX_MARKS];
bool g_profile = false;
int g_marked = 0;

void mark(int i, hipStream_t s)
{
    if (!g_profile) return;
    (void)hipEventRecord(g_marks[i], s);
    g_marked = i + 1;
}

void transform_passes(const float *src, int64_t src_stride, float level, uint32_t *A, uint32_t *B, int volumes, int D, int H, int W, hipStream_t s,
                      int first_mark)
{
    const int64_t cols = (int64_t)volumes * H * W;
    const int xtiles = (int)cdiv(W, Y_COLS);
    mark(first_mark, s);
    hipLaunchKernelGGL(column_kernel, dim3((unsigned)cdiv(cols, THREADS)), dim3(THREADS), 0, s, src, src_stride, level, A, volumes, D, H * W);
    mark(first_mark + 1, s);
    hipLaunchKernelGGL(y_pass_kernel, dim3((unsigned)((int64_t)volumes * D * xtiles)), dim3(THREADS), 0, s, (const uint32_t *)A, B, H, W, xtiles);
}

}  // namespace

extern "C" int64_t anoddpm_surface3d_workspace_bytes(int32_t S, int32_t D, int32_t H, int32_t W)
{
    if (!volume_ok(S, D, H, W) || !grids_ok(2 * (int64_t)S, D, H, W)) return -1;
    // buffers A and B of 2 S volumes each, the counts and the offsets of 2 S D H rows, two totals per pair: 4-byte words
    return (int64_t)16 * S * D * H * W + (int64_t)16 * S * D * H + (int64_t)8 * S;
}

extern "C" int anoddpm_distance_transform3d(const anoddpm_distance3d_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "distance_transform3d: null args");
    ANODDPM_REQUIRE(a->src && a->sq && a->workspace, "distance_transform3d: null pointer");
    ANODDPM_REQUIRE(volume_ok(a->S, a->D, a->H, a->W) && grids_ok(a->S, a->D, a->H, a->W),
                    "distance_transform3d: S, D, H, W must be >= 1, (D-1)^2 + (H-1)^2 + (W-1)^2 and D*H*W below 2^31, S * D * H rows below 2^31");
    const int64_t n = (int64_t)a->D * a->H * a->W;
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= n, "distance_transform3d: volumes overlap (src_stride < D*H*W)");
    ANODDPM_REQUIRE(a->workspace_bytes >= 8 * n * a->S, "distance_transform3d: workspace too small (8 * S * D * H * W bytes)");
    uint32_t *A = static_cast<uint32_t *>(a->workspace), *B = A + n * a->S;
    hipStream_t s = as_stream(stream);
    transform_passes(a->src, a->src_stride, a->level, A, B, a->S, a->D, a->H, a->W, s, 0);
    anoddpm_distance_args rows = {};
    rows.sq = a->sq;
    rows.dist = a->dist;
    rows.W = a->W;
    mark(2, s);
    hipLaunchKernelGGL(dt_row_kernel, dim3((unsigned)((int64_t)a->S * a->D * a->H)), dim3(THREADS), 0, s, rows, (const uint32_t *)B);
    mark(3, s);
    return check_launch("distance_transform3d");
}

extern "C" int anoddpm_surface_distance3d(const anoddpm_surface3d_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "surface_distance3d: null args");
    ANODDPM_REQUIRE(a->pred && a->ref && a->workspace && a->counts && a->max2 && a->mean && a->p95 && a->status,
                    "surface_distance3d: null pointer");
    const int64_t need = anoddpm_surface3d_workspace_bytes(a->S, a->D, a->H, a->W);
    ANODDPM_REQUIRE(need > 0, "surface_distance3d: S, D, H, W must be >= 1, (D-1)^2 + (H-1)^2 + (W-1)^2 and D*H*W below 2^31, 2 * S * D * H rows below 2^31");
    const int64_t n = (int64_t)a->D * a->H * a->W, rows = (int64_t)a->D * a->H, all_rows = 2 * rows * a->S;
    ANODDPM_REQUIRE(a->S == 1 || a->pred_stride >= n, "surface_distance3d: volumes overlap (pred_stride < D*H*W)");
    ANODDPM_REQUIRE(a->S == 1 || a->ref_stride == 0 || a->ref_stride >= n, "surface_distance3d: ref_stride must be 0 (shared reference) or >= D*H*W");
    ANODDPM_REQUIRE(a->workspace_bytes >= need, "surface_distance3d: workspace too small");
    const int shared_ref = a->S > 1 && a->ref_stride == 0 ? 1 : 0;
    const int volumes = a->S + (shared_ref ? 1 : a->S);
    uint32_t *A = static_cast<uint32_t *>(a->workspace), *B = A + 2 * n * a->S;
    uint32_t *cnt = B + 2 * n * a->S, *off = cnt + all_rows, *tot = off + all_rows;
    hipStream_t s = as_stream(stream);
    const int bpv = (int)cdiv(n, THREADS);
    mark(0, s);
    hipLaunchKernelGGL(border3d_kernel, dim3((unsigned)((int64_t)volumes * bpv)), dim3(THREADS), 0, s, *a, shared_ref, A, bpv);
    transform_passes(nullptr, 0, a->level, A, B, volumes, a->D, a->H, a->W, s, 1);
    mark(3, s);
    hipLaunchKernelGGL(surface3d_row_kernel, dim3((unsigned)all_rows), dim3(THREADS), 0, s, (const uint32_t *)B, reinterpret_cast<int32_t *>(A),
                       cnt, a->S, shared_ref, (int)rows, a->W);
    mark(4, s);
    hipLaunchKernelGGL(surface3d_scan_kernel, dim3((unsigned)a->S), dim3(STAT_THREADS), 0, s, (const uint32_t *)cnt, off, tot, (int)rows);
    mark(5, s);
    hipLaunchKernelGGL(surface3d_pack_kernel, dim3((unsigned)cdiv(all_rows, THREADS / 64)), dim3(THREADS), 0, s,
                       (const int32_t *)reinterpret_cast<int32_t *>(A), (const uint32_t *)cnt, (const uint32_t *)off, B, all_rows, (int)rows, a->W);
    mark(6, s);
    hipLaunchKernelGGL(surface3d_stats_kernel, dim3((unsigned)a->S), dim3(STAT_THREADS), 0, s, *a, (const uint32_t *)B, (const uint32_t *)tot);
    mark(7, s);
    return check_launch("surface_distance3d");
}

// Measurement hook of tools/bench_surface3d.py; NOT part of the public ABI (include/anoddpm_hip.h does not declare it).
// on = 1: create the events and record them in every later call of the two entry points above; on = 0: stop and destroy them.
extern "C" int anoddpm_internal_surface3d_profile(int32_t on)
{
    if ((on != 0) == g_profile) return 0;
    for (int i = 0; i < MAX_MARKS; ++i)
        if ((on ? hipEventCreate(&g_marks[i]) : hipEventDestroy(g_marks[i])) != hipSuccess) return -1;
    g_profile = on != 0;
    g_marked = 0;
    return 0;
}

// Waits for the last recorded call and writes the time of each of its launches in ms; returns their number (3 or 7), -1 on error.
extern "C" int anoddpm_internal_surface3d_times(float *ms)
{
    if (!g_profile || g_marked < 2 || ms == nullptr) return -1;
    if (hipEventSynchronize(g_marks[g_marked - 1]) != hipSuccess) return -1;
    for (int i = 0; i + 1 < g_marked; ++i)
        if (hipEventElapsedTime(&ms[i], g_marks[i], g_marks[i + 1]) != hipSuccess) return -1;
    return g_marked - 1;
}
