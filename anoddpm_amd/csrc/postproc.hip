// Post-processing of anomaly maps before they are scored -- replaces, per H x W plane,
//   scipy.ndimage.median_filter(plane, size=k)                                   anoddpm_median2d
//   scipy.ndimage.binary_erosion(plane > level, iterations=n)                    anoddpm_erode2d
//   scipy.ndimage.label(plane > level, structure) + numpy.bincount + a size cut  anoddpm_small_components
// (include/anoddpm_hip.h has the contract).  Every step selects or counts, so the outputs equal scipy's bit for bit.
//
// Median.  A workgroup of 256 threads owns a TH x TW = 16 x 32 tile of one plane: the tile and its k/2 halo go to LDS once as
// 31-bit patterns (reflect indexing at the plane's edges; the sign bit is dropped, which turns -0.0 into +0.0 and makes the
// unsigned order of the patterns the order of the non-negative floats).  A thread takes the k*k patterns of a pixel into
// registers and builds the middle one bit by bit from the top: x | bit stays when at most k*k/2 patterns are below it -- the
// largest x with count(v < x) <= m is the m-th smallest value itself.  31 rounds of k*k compare-and-add, no data-dependent
// branch, the same bits whatever the order of equal values.  Bound by VALU issue (62 k^2 instructions per pixel) and the k^2
// LDS reads in front of them; every input word is read from HBM about once.  Lanes of a wave read consecutive LDS words.
//
// Erosion.  n passes of the cross = one pass of the L1 ball of radius n over a zero-padded plane.  The tile and an n-pixel halo
// are staged as 0 / 1; pass 1 gives every staged row cell its horizontal run radius (how far the ones extend to BOTH sides,
// capped at n, -1 on a zero); pass 2 keeps a pixel when row dy of its column has radius >= n - |dy| for every |dy| <= n.
// 2 (2n + 1) LDS reads per pixel instead of the ball's 2n(n + 1) + 1.
//
// Small components.  Union-find on 32-bit labels in global memory, one launch per phase:
//   clear    label = own index on the foreground, -1 elsewhere; size = 0; counts = 0
//   link     every foreground pixel with its right / down (connectivity 2: and both lower diagonal) neighbours: find both roots,
//            atomicMin the smaller root into the larger one's label, retry with the value found there when it was no root any more
//   flatten  label = root
//   sizes    atomicAdd at the root (one add per wave when the whole wave has one root)
//   filter   keep the pixels whose root has size >= min_size; count the roots found and kept
// A label never grows and always names a pixel of the same component, so a stale read costs a retry, never a wrong answer; no
// workgroup waits on another, and the launch boundaries are the only ordering between workgroups.  The result is a set and two
// integers: independent of the order the atomics land in.
//
// Component areas (anoddpm_component_areas, the first half of the per-region overlap score of csrc/pro.hip).  The same link,
// flatten and sizes launches between a clear of its own (one counter per plane instead of two) and a final launch that writes
// size[root] at every foreground pixel, 0 elsewhere, and counts the roots of each plane.
#include <math.h>
#include "common.h"
#include "cc_shared.h"

namespace {

constexpr int THREADS = 256, TH = 16, TW = 32;
constexpr int MAX_K = 7, MAX_N = 8;

__device__ __forceinline__ int reflect(int i, int n)
{
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return min(max(i, 0), n - 1);                                    // tile overhang past the reflected band: any valid pixel
}

// ---------------------------------------------------------------------------------------------------- median
template <int K>
__global__ __launch_bounds__(THREADS) void median_kernel(anoddpm_median_args a, int tiles_x, int tiles_y)
{
    constexpr int R = K / 2, RH = TH + 2 * R, RW = TW + 2 * R, M = K * K / 2;
    __shared__ uint32_t tile[RH][RW];
    __shared__ int s_status;

    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int t = blockIdx.x % tiles;
    const int64_t plane = blockIdx.x / tiles;
    const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
    const int H = a.H, W = a.W;
    const float *__restrict__ src = a.src + plane * a.src_stride;
    const float *__restrict__ roi = a.roi ? a.roi + plane * a.roi_stride : nullptr;
    float *__restrict__ dst = a.dst + plane * (int64_t)H * W;

    if (tid == 0) s_status = 0;
    __syncthreads();
    int st = 0;
    for (int i = tid; i < RH * RW; i += THREADS) {
        const int r = i / RW, c = i - r * RW;
        const float s = src[(int64_t)reflect(y0 - R + r, H) * W + reflect(x0 - R + c, W)];
        if (s != s) st |= ANODDPM_ROC_NAN;
        else if (s == INFINITY || s == -INFINITY) st |= ANODDPM_ROC_INF;
        if (s < 0.0f) st |= ANODDPM_ROC_NEGATIVE;
        tile[r][c] = __float_as_uint(s) & 0x7fffffffu;
    }
    __syncthreads();

    for (int i = tid; i < TH * TW; i += THREADS) {
        const int r = i / TW, c = i % TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        bool inside = true;
        if (roi) {
            const float m = roi[(int64_t)gy * W + gx];
            if (!(m == 0.0f || m == 1.0f)) st |= ANODDPM_ROC_BAD_MASK;
            inside = m == 1.0f;
        }
        uint32_t x = 0;
        if (inside) {
            uint32_t v[K * K];
#pragma unroll
            for (int dy = 0; dy < K; ++dy)
#pragma unroll
                for (int dx = 0; dx < K; ++dx) v[dy * K + dx] = tile[r + dy][c + dx];
#pragma unroll 1
            for (int bit = 30; bit >= 0; --bit) {
                const uint32_t trial = x | (1u << bit);
                int below = 0;
#pragma unroll
                for (int j = 0; j < K * K; ++j) below += v[j] < trial ? 1 : 0;
                if (below <= M) x = trial;
            }
        }
        dst[(int64_t)gy * W + gx] = __uint_as_float(x);
    }
    if (st) atomicOr(&s_status, st);
    __syncthreads();
    if (tid == 0 && s_status) atomicOr(&a.status[plane], s_status);
}

// ---------------------------------------------------------------------------------------------------- erosion
__global__ __launch_bounds__(THREADS) void erode_kernel(anoddpm_erode_args a, int tiles_x, int tiles_y)
{
    constexpr int RH = TH + 2 * MAX_N, RW = TW + 2 * MAX_N;
    __shared__ int in[RH][RW];                                       // 0 / 1, zero outside the plane
    __shared__ int radius[RH][TW];                                   // horizontal run radius of the tile's columns, every staged row

    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int t = blockIdx.x % tiles;
    const int64_t plane = blockIdx.x / tiles;
    const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
    const int H = a.H, W = a.W, n = a.n;
    const int rh = TH + 2 * n, rw = TW + 2 * n;
    const float *__restrict__ src = a.src + plane * a.src_stride;
    float *__restrict__ dst = a.dst + plane * (int64_t)H * W;

    for (int i = tid; i < rh * rw; i += THREADS) {
        const int r = i / rw, c = i - r * rw;
        const int gy = y0 - n + r, gx = x0 - n + c;
        const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
        in[r][c] = ok && src[(int64_t)gy * W + gx] > a.level ? 1 : 0;
    }
    __syncthreads();
    for (int i = tid; i < rh * TW; i += THREADS) {
        const int r = i / TW, c = i % TW, cc = c + n;
        int h = -1;
        if (in[r][cc]) {
            h = 0;
            while (h < n && in[r][cc - h - 1] && in[r][cc + h + 1]) ++h;
        }
        radius[r][c] = h;
    }
    __syncthreads();
    for (int i = tid; i < TH * TW; i += THREADS) {
        const int r = i / TW, c = i % TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        bool keep = true;
        for (int dy = -n; dy <= n; ++dy) keep = keep && radius[r + n + dy][c] >= n - (dy < 0 ? -dy : dy);
        dst[(int64_t)gy * W + gx] = keep ? 1.0f : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------- small components
// Every kernel: blocks_per_plane workgroups per plane, thread -> pixel p of its plane, global index plane * H*W + p < 2^31.  The
// union-find primitives are those of cc_shared.h, shared with the volumes of postproc3d.hip.
using anoddpm::cc::Pixel;
using anoddpm::cc::pixel_of;
using anoddpm::cc::load_label;
using anoddpm::cc::find_root;
using anoddpm::cc::link;
using anoddpm::cc::add_sizes;
static_assert(THREADS == anoddpm::cc::THREADS, "pixel_of counts in workgroups of cc::THREADS");

__global__ __launch_bounds__(THREADS) void cc_clear_kernel(anoddpm_components_args a, int *label, int *size, int bpp)
{
    const int hw = a.H * a.W;
    const Pixel q = pixel_of(bpp, hw);
    if (!q.valid) return;
    label[q.idx] = a.src[q.plane * a.src_stride + q.p] > a.level ? q.idx : -1;
    size[q.idx] = 0;
    if (q.p == 0) a.counts[q.plane * 2] = a.counts[q.plane * 2 + 1] = 0;
}

__global__ __launch_bounds__(THREADS) void cc_link_kernel(anoddpm_components_args a, int *label, int bpp)
{
    const int hw = a.H * a.W, W = a.W;
    const Pixel q = pixel_of(bpp, hw);
    if (!q.valid || load_label(label, q.idx) < 0) return;
    const int y = q.p / W, x = q.p - y * W;
    const bool down = y + 1 < a.H;
    if (x + 1 < W && load_label(label, q.idx + 1) >= 0) link(label, q.idx, q.idx + 1);
    if (down && load_label(label, q.idx + W) >= 0) link(label, q.idx, q.idx + W);
    if (a.connectivity == 2 && down) {
        if (x > 0 && load_label(label, q.idx + W - 1) >= 0) link(label, q.idx, q.idx + W - 1);
        if (x + 1 < W && load_label(label, q.idx + W + 1) >= 0) link(label, q.idx, q.idx + W + 1);
    }
}

__global__ __launch_bounds__(THREADS) void cc_flatten_kernel(anoddpm_components_args a, int *label, int bpp)
{
    const Pixel q = pixel_of(bpp, a.H * a.W);
    if (!q.valid || load_label(label, q.idx) < 0) return;
    const int root = find_root(label, q.idx);
    __hip_atomic_store(label + q.idx, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(THREADS) void cc_size_kernel(anoddpm_components_args a, const int *__restrict__ label, int *size, int bpp)
{
    const Pixel q = pixel_of(bpp, a.H * a.W);
    add_sizes(size, q.valid ? label[q.idx] : -1);
}

__global__ __launch_bounds__(THREADS) void cc_filter_kernel(anoddpm_components_args a, const int *__restrict__ label,
                                                            const int *__restrict__ size, int bpp)
{
    __shared__ int s_found, s_kept;
    const int hw = a.H * a.W;
    const Pixel q = pixel_of(bpp, hw);
    if (threadIdx.x == 0) { s_found = 0; s_kept = 0; }
    __syncthreads();
    if (q.valid) {
        const int root = label[q.idx];
        const bool keep = root >= 0 && size[root] >= a.min_size;
        a.dst[q.plane * hw + q.p] = keep ? 1.0f : 0.0f;
        if (root == q.idx) {
            atomicAdd(&s_found, 1);
            if (keep) atomicAdd(&s_kept, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_found) {
        unsigned long long *c = reinterpret_cast<unsigned long long *>(a.counts + q.plane * 2);
        atomicAdd(c, (unsigned long long)s_found);
        if (s_kept) atomicAdd(c + 1, (unsigned long long)s_kept);
    }
}

// ---------------------------------------------------------------------------------------------------- component areas
__global__ __launch_bounds__(THREADS) void cc_areas_clear_kernel(anoddpm_component_areas_args a, int *label, int *size, int bpp)
{
    const int hw = a.H * a.W;
    const Pixel q = pixel_of(bpp, hw);
    if (!q.valid) return;
    label[q.idx] = a.src[q.plane * a.src_stride + q.p] > a.level ? q.idx : -1;
    size[q.idx] = 0;
    if (q.p == 0) a.counts[q.plane] = 0;
}

__global__ __launch_bounds__(THREADS) void cc_areas_kernel(anoddpm_component_areas_args a, const int *__restrict__ label,
                                                           const int *__restrict__ size, int bpp)
{
    __shared__ int s_found;
    const Pixel q = pixel_of(bpp, a.H * a.W);
    if (threadIdx.x == 0) s_found = 0;
    __syncthreads();
    if (q.valid) {
        const int root = label[q.idx];
        a.area[q.idx] = root >= 0 ? size[root] : 0;
        if (root == q.idx) atomicAdd(&s_found, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_found)
        atomicAdd(reinterpret_cast<unsigned long long *>(a.counts + q.plane), (unsigned long long)s_found);
}

// one workgroup per (plane, tile): a 1-D grid
bool tiles_ok(int32_t S, int32_t H, int32_t W)
{
    if (S < 1 || H < 1 || W < 1) return false;
    const int64_t tiles = (int64_t)((H + TH - 1) / TH) * ((W + TW - 1) / TW);
    return tiles <= 0x7fffffff / (int64_t)S;
}

}  // namespace

extern "C" int anoddpm_median2d(const anoddpm_median_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "median2d: null args");
    ANODDPM_REQUIRE(a->src && a->dst && a->status, "median2d: null pointer");
    ANODDPM_REQUIRE(tiles_ok(a->S, a->H, a->W), "median2d: S, H, W must be >= 1 and S * tiles below 2^31");
    ANODDPM_REQUIRE(a->k == 3 || a->k == 5 || a->k == MAX_K, "median2d: k must be 3, 5 or 7");
    ANODDPM_REQUIRE(a->k <= a->H && a->k <= a->W, "median2d: k exceeds the plane (k > min(H, W))");
    const int64_t hw = (int64_t)a->H * a->W;
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= hw, "median2d: planes overlap (src_stride < H*W)");
    ANODDPM_REQUIRE(!a->roi || a->S == 1 || a->roi_stride == 0 || a->roi_stride >= hw, "median2d: roi_stride must be 0 (shared ROI) or >= H*W");
    hipStream_t s = as_stream(stream);
    hipError_t e = hipMemsetAsync(a->status, 0, sizeof(int32_t) * (size_t)a->S, s);
    if (e != hipSuccess) {
        set_error("median2d: hipMemsetAsync(status): %s", hipGetErrorString(e));
        return ANODDPM_ELAUNCH;
    }
    const int tiles_x = (a->W + TW - 1) / TW, tiles_y = (a->H + TH - 1) / TH;
    const dim3 grid((unsigned)(a->S * tiles_x * tiles_y));
    if (a->k == 3) hipLaunchKernelGGL(median_kernel<3>, grid, dim3(THREADS), 0, s, *a, tiles_x, tiles_y);
    else if (a->k == 5) hipLaunchKernelGGL(median_kernel<5>, grid, dim3(THREADS), 0, s, *a, tiles_x, tiles_y);
    else hipLaunchKernelGGL(median_kernel<7>, grid, dim3(THREADS), 0, s, *a, tiles_x, tiles_y);
    return check_launch("median2d");
}

extern "C" int anoddpm_erode2d(const anoddpm_erode_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "erode2d: null args");
    ANODDPM_REQUIRE(a->src && a->dst, "erode2d: null pointer");
    ANODDPM_REQUIRE(tiles_ok(a->S, a->H, a->W), "erode2d: S, H, W must be >= 1 and S * tiles below 2^31");
    ANODDPM_REQUIRE(a->n >= 1 && a->n <= MAX_N, "erode2d: n must be in 1 ... 8");
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= (int64_t)a->H * a->W, "erode2d: planes overlap (src_stride < H*W)");
    const int tiles_x = (a->W + TW - 1) / TW, tiles_y = (a->H + TH - 1) / TH;
    hipLaunchKernelGGL(erode_kernel, dim3((unsigned)(a->S * tiles_x * tiles_y)), dim3(THREADS), 0, as_stream(stream), *a, tiles_x, tiles_y);
    return check_launch("erode2d");
}

extern "C" int64_t anoddpm_small_components_workspace_bytes(int32_t S, int32_t H, int32_t W)
{
    if (S < 1 || H < 1 || W < 1) return -1;
    const int64_t hw = (int64_t)H * W;
    if (hw >= ((int64_t)1 << 31) || hw > (((int64_t)1 << 31) - 1) / S) return -1;
    return (int64_t)S * hw * 8;
}

extern "C" int anoddpm_small_components(const anoddpm_components_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "small_components: null args");
    ANODDPM_REQUIRE(a->src && a->dst && a->counts && a->workspace, "small_components: null pointer");
    const int64_t need = anoddpm_small_components_workspace_bytes(a->S, a->H, a->W);
    ANODDPM_REQUIRE(need > 0, "small_components: S, H, W must be >= 1 and S * H * W below 2^31");
    ANODDPM_REQUIRE(a->min_size >= 0, "small_components: min_size must be >= 0");
    ANODDPM_REQUIRE(a->connectivity == 1 || a->connectivity == 2, "small_components: connectivity must be 1 (4 neighbours) or 2 (8 neighbours)");
    const int64_t hw = (int64_t)a->H * a->W;
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= hw, "small_components: planes overlap (src_stride < H*W)");
    ANODDPM_REQUIRE(a->workspace_bytes >= need, "small_components: workspace too small");
    int *label = static_cast<int *>(a->workspace);
    int *size = label + (int64_t)a->S * hw;
    const int bpp = (int)((hw + THREADS - 1) / THREADS);
    const dim3 grid((unsigned)((int64_t)a->S * bpp)), block(THREADS);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(cc_clear_kernel, grid, block, 0, s, *a, label, size, bpp);
    hipLaunchKernelGGL(cc_link_kernel, grid, block, 0, s, *a, label, bpp);
    hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, s, *a, label, bpp);
    hipLaunchKernelGGL(cc_size_kernel, grid, block, 0, s, *a, label, size, bpp);
    hipLaunchKernelGGL(cc_filter_kernel, grid, block, 0, s, *a, label, size, bpp);
    return check_launch("small_components");
}

extern "C" int anoddpm_component_areas(const anoddpm_component_areas_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "component_areas: null args");
    ANODDPM_REQUIRE(a->src && a->area && a->counts && a->workspace, "component_areas: null pointer");
    const int64_t need = anoddpm_small_components_workspace_bytes(a->S, a->H, a->W);
    ANODDPM_REQUIRE(need > 0, "component_areas: S, H, W must be >= 1 and S * H * W below 2^31");
    ANODDPM_REQUIRE(a->connectivity == 1 || a->connectivity == 2, "component_areas: connectivity must be 1 (4 neighbours) or 2 (8 neighbours)");
    const int64_t hw = (int64_t)a->H * a->W;
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= hw, "component_areas: planes overlap (src_stride < H*W)");
    ANODDPM_REQUIRE(a->workspace_bytes >= need, "component_areas: workspace too small");
    int *label = static_cast<int *>(a->workspace);
    int *size = label + (int64_t)a->S * hw;
    const int bpp = (int)((hw + THREADS - 1) / THREADS);
    const dim3 grid((unsigned)((int64_t)a->S * bpp)), block(THREADS);
    hipStream_t s = as_stream(stream);
    anoddpm_components_args c = {};                                  // what the shared phases read: H, W, connectivity
    c.S = a->S;
    c.H = a->H;
    c.W = a->W;
    c.connectivity = a->connectivity;
    hipLaunchKernelGGL(cc_areas_clear_kernel, grid, block, 0, s, *a, label, size, bpp);
    hipLaunchKernelGGL(cc_link_kernel, grid, block, 0, s, c, label, bpp);
    hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, s, c, label, bpp);
    hipLaunchKernelGGL(cc_size_kernel, grid, block, 0, s, c, label, size, bpp);
    hipLaunchKernelGGL(cc_areas_kernel, grid, block, 0, s, *a, label, size, bpp);
    return check_launch("component_areas");
}
