// Volume-wise post-processing of anomaly maps -- replaces, per D x H x W volume,
//   scipy.ndimage.median_filter(vol, size=k)                                               anoddpm_median3d
//   scipy.ndimage.binary_erosion(vol > level, iterations=n)                                anoddpm_erode3d
//   scipy.ndimage.label(vol > level, generate_binary_structure(3, c)) + bincount + a cut   anoddpm_small_components3d
//   ... + bincount[lab]                                                                    anoddpm_component_areas3d
// (include/anoddpm_hip.h has the contract).  The plane-wise forms are csrc/postproc.hip; a volume's result is not the stack of its
// slices' results.  Every step selects or counts, so the outputs equal scipy's bit for bit.
//
// Median.  A workgroup of 256 threads owns a TD x TH x TW = 4 x 8 x 32 tile of one volume: the tile and its k/2 halo go to LDS
// once as 31-bit patterns, reflect indexing on all three axes with period 2 * extent (a volume of one slice mirrors onto itself
// as often as the window asks).  A thread owns one (y, x) of the tile and walks its TD slices: it holds the k planes of k*k
// patterns of the window in registers, and a step along depth replaces one plane of them -- the selection does not care which
// register holds which value, so the slot is a compile-time index of the unrolled walk.  k*k LDS reads per voxel after the
// first instead of k*k*k.  The selection is that of median_kernel (postproc.hip): the middle pattern built bit by bit from the
// top, x | bit stays when at most k*k*k/2 patterns are below it; 31 rounds of k*k*k compare-and-add, no data-dependent branch.
// Bound by VALU issue (62 k^3 instructions per voxel).  The 125 values of k = 5 all live in registers (135 VGPRs, three waves per
// SIMD, no scratch); the candidate set is not narrowed first.
//
// Erosion.  n passes of the 6-neighbour cross = one AND over the L1 ball (octahedron) of radius n over a zero-padded volume.
// A workgroup owns a TD x TH x TW = 8 x 16 x 32 tile and visits the TD + 2n slices around it one after another: a slice is
// staged as 0 / 1 with an n-pixel halo, every staged row cell gets its horizontal run radius (erode_kernel's first pass), and
// every tile pixel the 2-D L1 radius of its slice,  r2 = min(n, min over |dy| <= n of (run radius of row y + dy) + |dy|), -1 on
// a zero -- the largest r for which erode_kernel's vertical condition holds.  r2 stays in LDS as one byte per staged voxel; a
// slice outside the volume is -1 throughout.  A voxel is kept when slice z + dz has r2 >= n - |dz| for every |dz| <= n.
// 2 (2n + 1) LDS reads per staged pixel and 2n + 1 per voxel instead of the ball's (2n + 1)(2n^2 + 2n + 3) / 3.
//
// Components.  The union-find of postproc.hip (primitives: cc_shared.h) with one segment per volume: clear, link, flatten, sizes,
// filter / areas.  Only the link launch knows the layout: it joins a foreground voxel with its forward neighbours, the offsets
// (dz, dy, dx) > (0, 0, 0) in lexicographic order with |dz| + |dy| + |dx| <= c -- 3 / 9 / 13 of them for c = 1 / 2 / 3.
#include <math.h>
#include "common.h"
#include "cc_shared.h"

namespace {

using anoddpm::cc::Pixel;
using anoddpm::cc::pixel_of;
using anoddpm::cc::load_label;
using anoddpm::cc::find_root;
using anoddpm::cc::link;
using anoddpm::cc::add_sizes;

constexpr int THREADS = anoddpm::cc::THREADS;
constexpr int MAX_N = 8;

// d c b a | a b c d | d c b a | a b c d ...: period 2n, any i (numpy.pad(mode="symmetric"), scipy's "reflect")
__device__ __forceinline__ int reflect_any(int i, int n)
{
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// ---------------------------------------------------------------------------------------------------- median
constexpr int MTD = 4, MTH = 8, MTW = 32;
static_assert(MTH * MTW == THREADS, "one thread per (y, x) of the tile");

template <int K>
__global__ __launch_bounds__(THREADS) void median3d_kernel(anoddpm_median3d_args a, int tiles_x, int tiles_y, int tiles_z)
{
    constexpr int R = K / 2, RD = MTD + 2 * R, RH = MTH + 2 * R, RW = MTW + 2 * R, KK = K * K, M = K * K * K / 2;
    __shared__ uint32_t tile[RD][RH][RW];
    __shared__ int s_status;

    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y * tiles_z;
    const int t = blockIdx.x % tiles;
    const int64_t vol = blockIdx.x / tiles;
    const int x0 = (t % tiles_x) * MTW, y0 = ((t / tiles_x) % tiles_y) * MTH, z0 = (t / (tiles_x * tiles_y)) * MTD;
    const int D = a.D, H = a.H, W = a.W;
    const int64_t hw = (int64_t)H * W;
    const float *__restrict__ src = a.src + vol * a.src_stride;
    float *__restrict__ dst = a.dst + vol * D * hw;

    if (tid == 0) s_status = 0;
    __syncthreads();
    int st = 0;
    for (int i = tid; i < RD * RH * RW; i += THREADS) {
        const int d = i / (RH * RW), rem = i - d * (RH * RW), r = rem / RW, c = rem - r * RW;
        const float s = src[reflect_any(z0 - R + d, D) * hw + (int64_t)reflect_any(y0 - R + r, H) * W + reflect_any(x0 - R + c, W)];
        if (s != s) st |= ANODDPM_ROC_NAN;
        else if (s == INFINITY || s == -INFINITY) st |= ANODDPM_ROC_INF;
        if (s < 0.0f) st |= ANODDPM_ROC_NEGATIVE;
        tile[d][r][c] = __float_as_uint(s) & 0x7fffffffu;
    }
    __syncthreads();

    const int r = tid / MTW, c = tid % MTW;
    const int gy = y0 + r, gx = x0 + c;
    if (gy < H && gx < W) {                                          // no barrier below
        const float *__restrict__ roi = a.roi ? a.roi + vol * a.roi_stride + (int64_t)gy * W + gx : nullptr;
        uint32_t v[K * KK];
#pragma unroll
        for (int dz = 0; dz < K - 1; ++dz)
#pragma unroll
            for (int dy = 0; dy < K; ++dy)
#pragma unroll
                for (int dx = 0; dx < K; ++dx) v[dz * KK + dy * K + dx] = tile[dz][r + dy][c + dx];
#pragma unroll
        for (int z = 0; z < MTD; ++z) {
            const int slot = (z + K - 1) % K;                        // the plane that left the window is overwritten
#pragma unroll
            for (int dy = 0; dy < K; ++dy)
#pragma unroll
                for (int dx = 0; dx < K; ++dx) v[slot * KK + dy * K + dx] = tile[z + K - 1][r + dy][c + dx];
            const int gz = z0 + z;
            if (gz >= D) break;
            bool inside = true;
            if (roi) {
                const float m = roi[gz * a.roi_slice_stride];
                if (!(m == 0.0f || m == 1.0f)) st |= ANODDPM_ROC_BAD_MASK;
                inside = m == 1.0f;
            }
            uint32_t x = 0;
            if (inside) {
#pragma unroll 1
                for (int bit = 30; bit >= 0; --bit) {
                    const uint32_t trial = x | (1u << bit);
                    int below = 0;
#pragma unroll
                    for (int j = 0; j < K * KK; ++j) below += v[j] < trial ? 1 : 0;
                    if (below <= M) x = trial;
                }
            }
            dst[gz * hw + (int64_t)gy * W + gx] = __uint_as_float(x);
        }
    }
    if (st) atomicOr(&s_status, st);
    __syncthreads();
    if (tid == 0 && s_status) atomicOr(&a.status[vol], s_status);
}

// ---------------------------------------------------------------------------------------------------- erosion
constexpr int ETD = 8, ETH = 16, ETW = 32;

__global__ __launch_bounds__(THREADS) void erode3d_kernel(anoddpm_erode3d_args a, int tiles_x, int tiles_y, int tiles_z)
{
    constexpr int RH = ETH + 2 * MAX_N, RW = ETW + 2 * MAX_N, RD = ETD + 2 * MAX_N;
    __shared__ int in[RH][RW];                                       // one slice: 0 / 1, zero outside the plane
    __shared__ int radius[RH][ETW];                                  // its horizontal run radius, the tile's columns of every staged row
    __shared__ signed char r2[RD][ETH][ETW];                         // 2-D L1 radius of every staged voxel in its slice, capped at n; -1: a zero

    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y * tiles_z;
    const int t = blockIdx.x % tiles;
    const int64_t vol = blockIdx.x / tiles;
    const int x0 = (t % tiles_x) * ETW, y0 = ((t / tiles_x) % tiles_y) * ETH, z0 = (t / (tiles_x * tiles_y)) * ETD;
    const int D = a.D, H = a.H, W = a.W, n = a.n;
    const int rh = ETH + 2 * n, rw = ETW + 2 * n, rd = ETD + 2 * n;
    const int64_t hw = (int64_t)H * W;
    const float *__restrict__ src = a.src + vol * a.src_stride;
    float *__restrict__ dst = a.dst + vol * D * hw;

    for (int d = 0; d < rd; ++d) {                                   // d, gz: the same in every thread, so are the barriers
        const int gz = z0 - n + d;
        if (gz < 0 || gz >= D) {
            for (int i = tid; i < ETH * ETW; i += THREADS) r2[d][i / ETW][i % ETW] = -1;
            continue;
        }
        const float *__restrict__ slice = src + gz * hw;
        for (int i = tid; i < rh * rw; i += THREADS) {
            const int r = i / rw, c = i - r * rw;
            const int gy = y0 - n + r, gx = x0 - n + c;
            const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
            in[r][c] = ok && slice[(int64_t)gy * W + gx] > a.level ? 1 : 0;
        }
        __syncthreads();
        for (int i = tid; i < rh * ETW; i += THREADS) {
            const int r = i / ETW, c = i % ETW, cc = c + n;
            int h = -1;
            if (in[r][cc]) {
                h = 0;
                while (h < n && in[r][cc - h - 1] && in[r][cc + h + 1]) ++h;
            }
            radius[r][c] = h;
        }
        __syncthreads();                                             // the next slice's staging overwrites `in` only after this
        for (int i = tid; i < ETH * ETW; i += THREADS) {
            const int r = i / ETW, c = i % ETW;
            int m = n;
            for (int dy = -n; dy <= n; ++dy) m = min(m, radius[r + n + dy][c] + (dy < 0 ? -dy : dy));
            r2[d][r][c] = (signed char)m;                            // radius is rewritten after the next slice's first barrier
        }
    }
    __syncthreads();
    for (int i = tid; i < ETD * ETH * ETW; i += THREADS) {
        const int d = i / (ETH * ETW), rem = i % (ETH * ETW), r = rem / ETW, c = rem % ETW;
        const int gz = z0 + d, gy = y0 + r, gx = x0 + c;
        if (gz >= D || gy >= H || gx >= W) continue;
        bool keep = true;
        for (int dz = -n; dz <= n; ++dz) keep = keep && r2[d + n + dz][r][c] >= n - (dz < 0 ? -dz : dz);
        dst[gz * hw + (int64_t)gy * W + gx] = keep ? 1.0f : 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------- components
// Every kernel: bpv workgroups per volume, thread -> voxel p of its volume, global index vol * D*H*W + p < 2^31.
__global__ __launch_bounds__(THREADS) void cc3_clear_kernel(const float *__restrict__ src, int64_t src_stride, float level, int n,
                                                            int *label, int *size, int64_t *counts, int ncounts, int bpv)
{
    const Pixel q = pixel_of(bpv, n);
    if (!q.valid) return;
    label[q.idx] = src[q.plane * src_stride + q.p] > level ? q.idx : -1;
    size[q.idx] = 0;
    if (q.p == 0)
        for (int j = 0; j < ncounts; ++j) counts[q.plane * ncounts + j] = 0;
}

__global__ __launch_bounds__(THREADS) void cc3_link_kernel(int D, int H, int W, int connectivity, int *label, int bpv)
{
    const int hw = H * W;
    const Pixel q = pixel_of(bpv, D * hw);
    if (!q.valid || load_label(label, q.idx) < 0) return;
    const int z = q.p / hw, rem = q.p - z * hw, y = rem / W, x = rem - y * W;
    for (int dz = 0; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const bool forward = dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx > 0)));
                if (!forward || dz + (dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx) > connectivity) continue;
                const int zz = z + dz, yy = y + dy, xx = x + dx;
                if (zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                const int o = q.idx + dz * hw + dy * W + dx;
                if (load_label(label, o) >= 0) link(label, q.idx, o);
            }
}

__global__ __launch_bounds__(THREADS) void cc3_flatten_kernel(int n, int *label, int bpv)
{
    const Pixel q = pixel_of(bpv, n);
    if (!q.valid || load_label(label, q.idx) < 0) return;
    const int root = find_root(label, q.idx);
    __hip_atomic_store(label + q.idx, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(THREADS) void cc3_size_kernel(int n, const int *__restrict__ label, int *size, int bpv)
{
    const Pixel q = pixel_of(bpv, n);
    add_sizes(size, q.valid ? label[q.idx] : -1);
}

// FILTER: dst = 0 / 1 and counts[vol] = {found, kept}; else area = size[root] and counts[vol] = found
template <bool FILTER>
__global__ __launch_bounds__(THREADS) void cc3_final_kernel(int n, int min_size, const int *__restrict__ label, const int *__restrict__ size,
                                                            float *dst, int32_t *area, int64_t *counts, int bpv)
{
    __shared__ int s_found, s_kept;
    const Pixel q = pixel_of(bpv, n);
    if (threadIdx.x == 0) { s_found = 0; s_kept = 0; }
    __syncthreads();
    if (q.valid) {
        const int root = label[q.idx];
        const int sz = root >= 0 ? size[root] : 0;
        const bool keep = root >= 0 && sz >= min_size;
        if (FILTER) dst[q.idx] = keep ? 1.0f : 0.0f;
        else area[q.idx] = sz;
        if (root == q.idx) {
            atomicAdd(&s_found, 1);
            if (FILTER && keep) atomicAdd(&s_kept, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_found) {
        unsigned long long *c = reinterpret_cast<unsigned long long *>(counts + q.plane * (FILTER ? 2 : 1));
        atomicAdd(c, (unsigned long long)s_found);
        if (FILTER && s_kept) atomicAdd(c + 1, (unsigned long long)s_kept);
    }
}

// one workgroup per (volume, tile): a 1-D grid
bool tiles_ok(int32_t S, int32_t D, int32_t H, int32_t W, int td, int th, int tw)
{
    if (S < 1 || D < 1 || H < 1 || W < 1) return false;
    const int64_t per_slab = (int64_t)((H + th - 1) / th) * ((W + tw - 1) / tw);       // below 2^31 * 2^31 / 256
    const int64_t slabs = (D + td - 1) / td;
    if (per_slab > 0x7fffffff / slabs) return false;
    return per_slab * slabs <= 0x7fffffff / (int64_t)S;
}

bool volume_ok(int32_t D, int32_t H, int32_t W)                     // D*H*W addressable with the int64 arithmetic of the kernels
{
    return (int64_t)H * W <= (((int64_t)1 << 40)) / D;
}

int components3d_launch(const char *what, const float *src, int64_t src_stride, float level, int S, int D, int H, int W, int connectivity,
                        int min_size, void *workspace, float *dst, int32_t *area, int64_t *counts, void *stream)
{
    using namespace anoddpm;
    const int n = D * H * W;
    int *label = static_cast<int *>(workspace);
    int *size = label + (int64_t)S * n;
    const int bpv = (int)(((int64_t)n + THREADS - 1) / THREADS);
    const dim3 grid((unsigned)((int64_t)S * bpv)), block(THREADS);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(cc3_clear_kernel, grid, block, 0, s, src, src_stride, level, n, label, size, counts, dst ? 2 : 1, bpv);
    hipLaunchKernelGGL(cc3_link_kernel, grid, block, 0, s, D, H, W, connectivity, label, bpv);
    hipLaunchKernelGGL(cc3_flatten_kernel, grid, block, 0, s, n, label, bpv);
    hipLaunchKernelGGL(cc3_size_kernel, grid, block, 0, s, n, label, size, bpv);
    if (dst) hipLaunchKernelGGL(cc3_final_kernel<true>, grid, block, 0, s, n, min_size, label, size, dst, area, counts, bpv);
    else hipLaunchKernelGGL(cc3_final_kernel<false>, grid, block, 0, s, n, min_size, label, size, dst, area, counts, bpv);
    return check_launch(what);
}

}  // namespace

extern "C" int anoddpm_median3d(const anoddpm_median3d_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "median3d: null args");
    ANODDPM_REQUIRE(a->src && a->dst && a->status, "median3d: null pointer");
    ANODDPM_REQUIRE(tiles_ok(a->S, a->D, a->H, a->W, MTD, MTH, MTW) && volume_ok(a->D, a->H, a->W),
                    "median3d: S, D, H, W must be >= 1 and S * tiles below 2^31");
    ANODDPM_REQUIRE(a->k == 3 || a->k == 5, "median3d: k must be 3 or 5");
    ANODDPM_REQUIRE(a->k <= a->H && a->k <= a->W, "median3d: k exceeds the plane (k > min(H, W))");
    const int64_t hw = (int64_t)a->H * a->W, dhw = hw * a->D;
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= dhw, "median3d: volumes overlap (src_stride < D*H*W)");
    if (a->roi) {
        ANODDPM_REQUIRE(a->roi_slice_stride == 0 || a->roi_slice_stride == hw, "median3d: roi_slice_stride must be 0 (one plane) or H*W");
        ANODDPM_REQUIRE(a->roi_slice_stride != 0 || a->roi_stride == 0, "median3d: a ROI of one plane is shared by all volumes (roi_stride must be 0)");
        ANODDPM_REQUIRE(a->S == 1 || a->roi_stride == 0 || a->roi_stride >= dhw, "median3d: roi_stride must be 0 (shared ROI) or >= D*H*W");
    }
    hipStream_t s = as_stream(stream);
    hipError_t e = hipMemsetAsync(a->status, 0, sizeof(int32_t) * (size_t)a->S, s);
    if (e != hipSuccess) {
        set_error("median3d: hipMemsetAsync(status): %s", hipGetErrorString(e));
        return ANODDPM_ELAUNCH;
    }
    const int tiles_x = (a->W + MTW - 1) / MTW, tiles_y = (a->H + MTH - 1) / MTH, tiles_z = (a->D + MTD - 1) / MTD;
    const dim3 grid((unsigned)((int64_t)a->S * tiles_x * tiles_y * tiles_z));
    if (a->k == 3) hipLaunchKernelGGL(median3d_kernel<3>, grid, dim3(THREADS), 0, s, *a, tiles_x, tiles_y, tiles_z);
    else hipLaunchKernelGGL(median3d_kernel<5>, grid, dim3(THREADS), 0, s, *a, tiles_x, tiles_y, tiles_z);
    return check_launch("median3d");
}

extern "C" int anoddpm_erode3d(const anoddpm_erode3d_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "erode3d: null args");
    ANODDPM_REQUIRE(a->src && a->dst, "erode3d: null pointer");
    ANODDPM_REQUIRE(tiles_ok(a->S, a->D, a->H, a->W, ETD, ETH, ETW) && volume_ok(a->D, a->H, a->W),
                    "erode3d: S, D, H, W must be >= 1 and S * tiles below 2^31");
    ANODDPM_REQUIRE(a->n >= 1 && a->n <= MAX_N, "erode3d: n must be in 1 ... 8");
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= (int64_t)a->D * a->H * a->W, "erode3d: volumes overlap (src_stride < D*H*W)");
    const int tiles_x = (a->W + ETW - 1) / ETW, tiles_y = (a->H + ETH - 1) / ETH, tiles_z = (a->D + ETD - 1) / ETD;
    hipLaunchKernelGGL(erode3d_kernel, dim3((unsigned)((int64_t)a->S * tiles_x * tiles_y * tiles_z)), dim3(THREADS), 0, as_stream(stream), *a,
                       tiles_x, tiles_y, tiles_z);
    return check_launch("erode3d");
}

extern "C" int64_t anoddpm_components3d_workspace_bytes(int32_t S, int32_t D, int32_t H, int32_t W)
{
    if (S < 1 || D < 1 || H < 1 || W < 1) return -1;
    const int64_t limit = ((int64_t)1 << 31) - 1;
    const int64_t hw = (int64_t)H * W;
    if (hw > limit / D) return -1;
    const int64_t n = hw * D;
    if (n > limit / S) return -1;
    return (int64_t)S * n * 8;
}

extern "C" int anoddpm_small_components3d(const anoddpm_components3d_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "small_components3d: null args");
    ANODDPM_REQUIRE(a->src && a->dst && a->counts && a->workspace, "small_components3d: null pointer");
    const int64_t need = anoddpm_components3d_workspace_bytes(a->S, a->D, a->H, a->W);
    ANODDPM_REQUIRE(need > 0, "small_components3d: S, D, H, W must be >= 1 and S * D * H * W below 2^31");
    ANODDPM_REQUIRE(a->min_size >= 0, "small_components3d: min_size must be >= 0");
    ANODDPM_REQUIRE(a->connectivity >= 1 && a->connectivity <= 3, "small_components3d: connectivity must be 1 (6 neighbours), 2 (18) or 3 (26)");
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= (int64_t)a->D * a->H * a->W, "small_components3d: volumes overlap (src_stride < D*H*W)");
    ANODDPM_REQUIRE(a->workspace_bytes >= need, "small_components3d: workspace too small");
    return components3d_launch("small_components3d", a->src, a->src_stride, a->level, a->S, a->D, a->H, a->W, a->connectivity, a->min_size,
                               a->workspace, a->dst, nullptr, a->counts, stream);
}

extern "C" int anoddpm_component_areas3d(const anoddpm_component_areas3d_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "component_areas3d: null args");
    ANODDPM_REQUIRE(a->src && a->area && a->counts && a->workspace, "component_areas3d: null pointer");
    const int64_t need = anoddpm_components3d_workspace_bytes(a->S, a->D, a->H, a->W);
    ANODDPM_REQUIRE(need > 0, "component_areas3d: S, D, H, W must be >= 1 and S * D * H * W below 2^31");
    ANODDPM_REQUIRE(a->connectivity >= 1 && a->connectivity <= 3, "component_areas3d: connectivity must be 1 (6 neighbours), 2 (18) or 3 (26)");
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= (int64_t)a->D * a->H * a->W, "component_areas3d: volumes overlap (src_stride < D*H*W)");
    ANODDPM_REQUIRE(a->workspace_bytes >= need, "component_areas3d: workspace too small");
    return components3d_launch("component_areas3d", a->src, a->src_stride, a->level, a->S, a->D, a->H, a->W, a->connectivity, 0,
                               a->workspace, nullptr, a->area, a->counts, stream);
}
