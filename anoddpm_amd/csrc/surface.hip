// Exact Euclidean distance transform and boundary distances (Hausdorff, HD95, average symmetric surface distance) of batched
// H x W planes -- replaces, per plane or per pair of planes,
//   scipy.ndimage.distance_transform_edt(plane > level)                                    anoddpm_distance_transform
//   m & ~scipy.ndimage.binary_erosion(m) twice + distance_transform_edt twice + numpy.percentile   anoddpm_surface_distance
// (include/anoddpm_hip.h has the contract).  Every distance is an integer squared distance until its one fp64 square root, so
// the outputs are statements about integers: the same bits every launch and wherever a plane sits in a batch.
//
// The transform is separable: the squared distance of (y, x) to the nearest zero of a 0 / 1 plane is
//   min over x' of (x - x')^2 + g(y, x')^2,      g(y, x') = distance from (y, x') to the nearest zero of column x'.
//   column   one thread per (plane, column), lanes on consecutive columns: a sweep down and a sweep up, eight rows loaded before
//            the eight dependent steps that use them; writes g^2 as uint32, FAR = 2^31 - 1 where the column has no zero.
//   row      one workgroup per (plane, row): the row of g^2 goes to LDS (rows above 4096 columns are read from global memory
//            instead), and a thread walks outwards from its own column, x' = x -+ k, while k^2 < best -- no farther than its
//            own g.  Integer adds and minima only; (H - 1)^2 + (W - 1)^2 < 2^31 keeps every sum inside 32 bits.
// A plane without a zero keeps FAR everywhere: squared distance -1, distance +inf.
//
// Surface distances.  The border of a mask is its foreground with a 4-neighbour that is background or outside the image; the
// transform above runs with the BORDER as its zero set:
//   border   one thread per pixel of every prediction plane and every reference plane (one plane when it is shared): 0 on the
//            border, 1 elsewhere, into the g^2 buffer
//   column   as above, in place
//   row      one workgroup per (pair, direction, row), only for rows that hold a border pixel of the own side: the squared
//            distance to the other side's border at every own border pixel, -1 elsewhere
//   stats    one workgroup of 1024 threads per pair: counts, the largest squared distance, the mean and the percentiles.
//            Mean: thread t adds sqrt(d2) of the pixels t, t + 1024, ... of the plane in that order (pixels off the border add
//            nothing), a halving tree folds the 64 partials of a wave and then the 16 wave sums (the order of roc.hip's average
//            precision); one division by the count.  Percentile: the order statistics lo and hi are SELECTED on the integer
//            squared distances by a radix select (four passes of 8 bits over an LDS histogram; integer atomics only), and only
//            the two selected values get a square root.  Before the selects the workgroup packs the border pixels' squared
//            distances of both directions, one behind the other, into its share of the g^2 buffer (dead by then), so a select
//            pass walks the border pixels instead of the plane and the pooled multiset is one array.
// Four launches whatever the batch; no floating-point atomics; no host synchronisation.  Compiled with -ffp-contract=off.
#include "surface_shared.h"                                          // the column sweep, the row search, the selects, the trees

namespace {

// ---------------------------------------------------------------------------------------------------- border
__global__ __launch_bounds__(THREADS) void border_kernel(anoddpm_surface_args a, int shared_ref, uint32_t *__restrict__ g2, int bpp)
{
    const int H = a.H, W = a.W, hw = H * W;
    const int q = blockIdx.x / bpp;
    const int p = (int)(blockIdx.x % bpp) * THREADS + (int)threadIdx.x;
    if (p >= hw) return;
    const float *__restrict__ src = q < a.S ? a.pred + (int64_t)q * a.pred_stride : a.ref + (shared_ref ? 0 : (int64_t)(q - a.S) * a.ref_stride);
    const int y = p / W, x = p - y * W;
    bool border = false;
    if (src[p] > a.level) {
        const bool inner = x > 0 && x + 1 < W && y > 0 && y + 1 < H &&
                           src[p - 1] > a.level && src[p + 1] > a.level && src[p - W] > a.level && src[p + W] > a.level;
        border = !inner;
    }
    g2[(int64_t)q * hw + p] = border ? 0u : 1u;
}

// ---------------------------------------------------------------------------------------------------- row pass
__global__ __launch_bounds__(THREADS) void surface_row_kernel(const uint32_t *__restrict__ g2, int32_t *__restrict__ d2,
                                                              int S, int shared_ref, int H, int W)
{
    __shared__ uint32_t tile[ROW_LDS];
    const int y = (int)(blockIdx.x % (unsigned)H);
    const int dir = (int)((blockIdx.x / (unsigned)H) & 1u);
    const int s = (int)(blockIdx.x / (2u * (unsigned)H));
    const int64_t hw = (int64_t)H * W, off = (int64_t)y * W;
    const uint32_t *gp = g2 + (int64_t)s * hw + off;
    const uint32_t *gr = g2 + (int64_t)(S + (shared_ref ? 0 : s)) * hw + off;
    const uint32_t *__restrict__ own = dir == 0 ? gp : gr;
    const uint32_t *__restrict__ other = dir == 0 ? gr : gp;
    int32_t *__restrict__ out = d2 + ((int64_t)s * 2 + dir) * hw + off;
    int any = 0;
    for (int x = threadIdx.x; x < W; x += THREADS) any |= own[x] == 0u ? 1 : 0;
    if (!__syncthreads_or(any)) {                                    // no border pixel of the own side in this row
        for (int x = threadIdx.x; x < W; x += THREADS) out[x] = -1;
        return;
    }
    const uint32_t *row = stage_row(other, tile, W);
    for (int x = threadIdx.x; x < W; x += THREADS)
        out[x] = own[x] == 0u ? (int32_t)min(nearest(row, x, W), FAR) : -1;
}

// ---------------------------------------------------------------------------------------------------- per-pair statistics
__global__ __launch_bounds__(STAT_THREADS) void surface_stats_kernel(anoddpm_surface_args a, const int32_t *__restrict__ d2, uint32_t *g2)
{
    __shared__ uint32_t hist[256], sel[2], s_n[2], s_fill[2];
    __shared__ PairFold fold;

    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const uint32_t hw = (uint32_t)(a.H * a.W);
    const int32_t *__restrict__ v = d2 + (int64_t)s * 2 * hw;       // direction 0, then direction 1

    if (tid < 2) s_fill[tid] = 0;
    uint32_t cnt[2] = {0, 0};
    int32_t mx[2] = {-1, -1};
    double sum[2] = {0.0, 0.0};
    for (uint32_t i = tid; i < hw; i += STAT_THREADS) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const int32_t w = v[(int64_t)d * hw + i];
            if (w >= 0) {
                ++cnt[d];
                mx[d] = max(mx[d], w);
                sum[d] += sqrt((double)w);
            }
        }
    }
    fold_pair(cnt, mx, sum, fold);
    if (tid == 0) finish_pair(s, cnt, mx, sum, a.counts, a.max2, a.mean, a.p95, a.status, s_n);
    __syncthreads();
    const uint32_t n0 = s_n[0], n1 = s_n[1];
    if (n0 == 0) return;                                             // block-uniform: an empty border on either side
    // The squared distances of the two directions, packed one behind the other into the pair's share of the g^2 buffer, which
    // nothing reads any more: the selects walk n0 + n1 words instead of two planes.  Their order in the buffer varies from run
    // to run; an order statistic of integers does not depend on it.
    uint32_t *packed = g2 + (int64_t)s * 2 * hw;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t base = 0; base < hw; base += STAT_THREADS) {       // wave-uniform trip count: ballots inside
        const uint32_t i = base + tid;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const int32_t w = i < hw ? v[(int64_t)d * hw + i] : -1;
            const unsigned long long take = __ballot(w >= 0);
            if (take == 0) continue;
            const int leader = __ffsll(take) - 1;
            uint32_t at = 0;
            if (lane == leader) at = atomicAdd(&s_fill[d], (uint32_t)__popcll(take));
            at = __shfl(at, leader);
            if (w >= 0) packed[(d ? n0 : 0u) + at + (uint32_t)__popcll(take & below)] = (uint32_t)w;
        }
    }
    __syncthreads();
    write_percentiles(packed, n0, n1, a.p95 + (int64_t)s * 3, hist, sel);
}

// S, H, W >= 1, every squared distance below 2^31 and both planes sets of a surface run indexable with 31 bits
bool extents_ok(int32_t S, int32_t H, int32_t W)
{
    if (S < 1 || H < 1 || W < 1) return false;
    const int64_t hw = (int64_t)H * W, dy = H - 1, dx = W - 1;
    if (hw >= ((int64_t)1 << 31) || dy * dy + dx * dx >= ((int64_t)1 << 31)) return false;
    return 2 * hw <= (((int64_t)1 << 31) - 1) / S;
}

}  // namespace

extern "C" int64_t anoddpm_surface_workspace_bytes(int32_t S, int32_t H, int32_t W)
{
    if (!extents_ok(S, H, W)) return -1;
    return (int64_t)16 * S * H * W;                                  // g^2 of 2 S planes and d2 of S pairs x 2 directions, 4 bytes each
}

extern "C" int anoddpm_distance_transform(const anoddpm_distance_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "distance_transform: null args");
    ANODDPM_REQUIRE(a->src && a->sq && a->workspace, "distance_transform: null pointer");
    ANODDPM_REQUIRE(extents_ok(a->S, a->H, a->W),
                    "distance_transform: S, H, W must be >= 1, (H-1)^2 + (W-1)^2 and H*W below 2^31, 2 * S * H * W below 2^31");
    const int64_t hw = (int64_t)a->H * a->W;
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= hw, "distance_transform: planes overlap (src_stride < H*W)");
    ANODDPM_REQUIRE(a->workspace_bytes >= 4 * hw * a->S, "distance_transform: workspace too small (4 * S * H * W bytes)");
    uint32_t *g2 = static_cast<uint32_t *>(a->workspace);
    hipStream_t s = as_stream(stream);
    const int64_t cols = (int64_t)a->S * a->W;
    hipLaunchKernelGGL(column_kernel, dim3((unsigned)((cols + THREADS - 1) / THREADS)), dim3(THREADS), 0, s,
                       a->src, a->src_stride, a->level, g2, a->S, a->H, a->W);
    hipLaunchKernelGGL(dt_row_kernel, dim3((unsigned)((int64_t)a->S * a->H)), dim3(THREADS), 0, s, *a, g2);
    return check_launch("distance_transform");
}

extern "C" int anoddpm_surface_distance(const anoddpm_surface_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "surface_distance: null args");
    ANODDPM_REQUIRE(a->pred && a->ref && a->workspace && a->counts && a->max2 && a->mean && a->p95 && a->status,
                    "surface_distance: null pointer");
    const int64_t need = anoddpm_surface_workspace_bytes(a->S, a->H, a->W);
    ANODDPM_REQUIRE(need > 0, "surface_distance: S, H, W must be >= 1, (H-1)^2 + (W-1)^2 and H*W below 2^31, 2 * S * H * W below 2^31");
    const int64_t hw = (int64_t)a->H * a->W;
    ANODDPM_REQUIRE(a->S == 1 || a->pred_stride >= hw, "surface_distance: planes overlap (pred_stride < H*W)");
    ANODDPM_REQUIRE(a->S == 1 || a->ref_stride == 0 || a->ref_stride >= hw, "surface_distance: ref_stride must be 0 (shared reference) or >= H*W");
    ANODDPM_REQUIRE(a->workspace_bytes >= need, "surface_distance: workspace too small");
    const int shared_ref = a->S > 1 && a->ref_stride == 0 ? 1 : 0;
    const int planes = a->S + (shared_ref ? 1 : a->S);
    uint32_t *g2 = static_cast<uint32_t *>(a->workspace);
    int32_t *d2 = reinterpret_cast<int32_t *>(g2 + (int64_t)2 * a->S * hw);
    hipStream_t s = as_stream(stream);
    const int bpp = (int)((hw + THREADS - 1) / THREADS);
    const int64_t cols = (int64_t)planes * a->W;
    hipLaunchKernelGGL(border_kernel, dim3((unsigned)((int64_t)planes * bpp)), dim3(THREADS), 0, s, *a, shared_ref, g2, bpp);
    hipLaunchKernelGGL(column_kernel, dim3((unsigned)((cols + THREADS - 1) / THREADS)), dim3(THREADS), 0, s,
                       (const float *)nullptr, (int64_t)0, a->level, g2, planes, a->H, a->W);
    hipLaunchKernelGGL(surface_row_kernel, dim3((unsigned)((int64_t)a->S * 2 * a->H)), dim3(THREADS), 0, s,
                       (const uint32_t *)g2, d2, a->S, shared_ref, a->H, a->W);
    hipLaunchKernelGGL(surface_stats_kernel, dim3((unsigned)a->S), dim3(STAT_THREADS), 0, s, *a, (const int32_t *)d2, g2);
    return check_launch("surface_distance");
}
