// Gaussian smoothing of whole volumes -- the step the volume-wise protocols put in front of the 3-D median, the cut and the
// boundary distances.  Replaces, per D x H x W volume,
//   scipy.ndimage.gaussian_filter(vol, (sz, sy, sx), truncate=truncate)                    anoddpm_gauss3d
// (include/anoddpm_hip.h has the contract).  Compiled with -ffp-contract=off: a statement about a fixed sequence of fp64
// operations.
//
// scipy filters axis 0 (D) into an fp32 array, axis 1 (H) from it into another and axis 2 (W) from that; a line is read as fp64
// and the symmetric kernel is applied as  acc = v[i] w[r];  acc += (v[i+j] + v[i-j]) w[r+j]  for j = -r ... -1, every product and
// sum rounded once (csrc/smooth.hip's statement, with a radius per axis).  The z pass of a volume is exactly the axis-0 pass of a
// 2-D filter on the plane D x (H W), so ONE separable tile kernel with independent radii (r0, r1), either of which may be 0, serves
// both launches:
//   launch 1   S planes of D x HW, radii (rz, 0), src -> tmp: the fp32 store is scipy's rounding between axis 0 and axis 1
//   launch 2   S D planes of H x W, radii (ry, rx), tmp -> dst
// and a volume whose z axis (or whose y and x axes) is skipped takes one launch, src -> dst.  A workgroup of 256 threads owns a
// TILE x TILE = 32 x 32 tile of one plane:
//   stage    the tile and its halo, (32 + 2 r0) x (32 + 2 r1) fp32 words, with the reflection resolved (m = i mod 2n; m >= n ->
//            2n-1-m), so an extent below the radius -- one slice -- reflects as often as it has to
//   axis 0   (r0 > 0) the 32 tile rows of every staged column into an fp32 LDS buffer, or straight to memory when r1 == 0
//   axis 1   (r1 > 0) the 32 x 32 outputs from that buffer, or from the staged tile when r0 == 0
// Lanes sit on consecutive x in every pass of both launches (x is the fastest index of the volume and of the plane D x HW):
// consecutive LDS words, no bank conflict, one broadcast read per tap weight, coalesced loads and stores.  Rows of a ragged tile
// that lie outside the plane are not computed (D = 4 at rz = 16 runs 4 of the 32 rows).
// Bound by the fp64 VALU.  Per output voxel and filtered axis: r + 1 multiplies and 2r adds, in front of each tap two LDS reads and
// two fp32 -> fp64 conversions; the axis-0 pass of launch 2 also runs over the 2 r1 halo columns, (32 + 2 r1) / 32 of that.
// LDS: ((32 + 2 r0)(32 + 2 r1) + 32 (32 + 2 r1)) * 4 + 528 bytes, asked for per launch (the second buffer only when both radii
// are set) -- 49680 at radius 32 on both axes, inside the 64 KB a workgroup gets without an attribute.
//
// The reflection and the tap loop are stated here on their own: smooth.hip's take an int index and a plane whose extents stay
// below 2^30, this file's plane D x HW has a width of up to 2^31 - 1, and that file is left as it is.
#include "common.h"

namespace {

constexpr int THREADS = 256, TILE = 32, MAX_R = ANODDPM_GAUSS_MAX_RADIUS;

// index i of a line of n, n up to 2^31 - 1; inside the line (all but the border tiles) nothing is divided
__device__ __forceinline__ int reflect_periodic(int64_t i, int n)
{
    if (i >= 0 && i < n) return (int)i;
    const int64_t p = 2 * (int64_t)n;
    int64_t m = i % p;
    if (m < 0) m += p;
    return (int)(m >= n ? p - 1 - m : m);
}

// the symmetric kernel at c[0], the taps `step` words apart, from the edge inwards
__device__ __forceinline__ float taps(const float *c, int step, const double *wl, int r)
{
    double acc = (double)c[0] * wl[r];
    for (int j = r; j >= 1; --j) acc += ((double)c[-j * step] + (double)c[j * step]) * wl[r - j];
    return (float)acc;
}

struct pass_args {
    const float *src;               // plane p at src + (p / G) * group_stride + (p % G) * P0 * P1
    float *dst;                     // contiguous planes
    const double *w0, *w1;          // not read where the radius is 0
    int64_t group_stride;
    int32_t G, P0, P1, r0, r1;      // a plane is P0 rows of P1 contiguous words
    int32_t tiles_x, tiles_y;
};

__global__ __launch_bounds__(THREADS) void gauss_pass_kernel(pass_args a)
{
    extern __shared__ double smem[];
    const int r0 = a.r0, r1 = a.r1, RW = TILE + 2 * r1, RH = TILE + 2 * r0;       // staged tile: RH x RW
    double *wl0 = smem, *wl1 = smem + MAX_R + 1;                     // [MAX_R + 1] each
    float *tile = reinterpret_cast<float *>(smem + 2 * (MAX_R + 1));  // [RH][RW]
    float *mid = tile + RH * RW;                                     // [TILE][RW]: axis 0 done, rounded to fp32 (r0 > 0 and r1 > 0 only)

    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int t = blockIdx.x % tiles;
    const int64_t plane = blockIdx.x / tiles;
    const int y0 = (t / a.tiles_x) * TILE;
    const int64_t x0 = (int64_t)(t % a.tiles_x) * TILE;
    const int P0 = a.P0, P1 = a.P1;
    const int64_t psize = (int64_t)P0 * P1;
    const float *__restrict__ src = a.src + (plane / a.G) * a.group_stride + (plane % a.G) * psize;
    float *__restrict__ dst = a.dst + plane * psize;
    const int rows = min(TILE, P0 - y0);                             // tile rows inside the plane: the others are not computed

    if (r0 > 0 && tid <= r0) wl0[tid] = a.w0[tid];
    if (r1 > 0 && tid <= r1) wl1[tid] = a.w1[tid];
    for (int i = tid; i < (rows + 2 * r0) * RW; i += THREADS) {
        const int y = i / RW, x = i - y * RW;
        tile[i] = src[(int64_t)reflect_periodic((int64_t)y0 - r0 + y, P0) * P1 + reflect_periodic(x0 - r1 + x, P1)];
    }
    __syncthreads();

    if (r1 == 0) {                                                   // axis 0 only: RW == TILE, straight to memory
        for (int i = tid; i < rows * TILE; i += THREADS) {
            const int y = i / TILE, x = i % TILE;
            if (x0 + x >= P1) continue;
            dst[(int64_t)(y0 + y) * P1 + x0 + x] = taps(tile + (y + r0) * TILE + x, TILE, wl0, r0);
        }
        return;
    }
    const float *from = tile;                                        // axis 1 reads [rows][RW]
    if (r0 > 0) {
        for (int i = tid; i < rows * RW; i += THREADS) {
            const int y = i / RW, x = i - y * RW;
            mid[i] = taps(tile + (y + r0) * RW + x, RW, wl0, r0);
        }
        __syncthreads();
        from = mid;
    }
    for (int i = tid; i < rows * TILE; i += THREADS) {
        const int y = i / TILE, x = i % TILE;
        if (x0 + x >= P1) continue;
        dst[(int64_t)(y0 + y) * P1 + x0 + x] = taps(from + y * RW + x + r1, 1, wl1, r1);
    }
}

// one workgroup per (plane, tile): a 1-D grid.  planes * P0 * P1 < 2^31 (checked by the caller), so the tile count is too.
void launch_pass(const float *src, float *dst, const double *w0, const double *w1, int64_t group_stride, int G, int64_t planes,
                 int P0, int P1, int r0, int r1, hipStream_t stream)
{
    pass_args p;
    p.src = src, p.dst = dst, p.w0 = w0, p.w1 = w1, p.group_stride = group_stride;
    p.G = G, p.P0 = P0, p.P1 = P1, p.r0 = r0, p.r1 = r1;
    p.tiles_x = (int)(((int64_t)P1 + TILE - 1) / TILE), p.tiles_y = (P0 + TILE - 1) / TILE;
    const int rw = TILE + 2 * r1, rh = TILE + 2 * r0;
    const size_t lds = sizeof(double) * 2 * (MAX_R + 1) + sizeof(float) * (size_t)(rh * rw + (r0 > 0 && r1 > 0 ? TILE * rw : 0));
    hipLaunchKernelGGL(gauss_pass_kernel, dim3((unsigned)(planes * p.tiles_x * p.tiles_y)), dim3(THREADS), lds, stream, p);
}

bool overlap(const void *p, int64_t pn, const void *q, int64_t qn)  // [p, p + pn) and [q, q + qn) fp32 elements
{
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(p), q0 = reinterpret_cast<uintptr_t>(q);
    return !(p0 + sizeof(float) * (uintptr_t)pn <= q0 || q0 + sizeof(float) * (uintptr_t)qn <= p0);
}

}  // namespace

extern "C" int anoddpm_gauss3d(const anoddpm_gauss3d_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "gauss3d: null args");
    ANODDPM_REQUIRE(a->rz >= 0 && a->rz <= MAX_R && a->ry >= 0 && a->ry <= MAX_R && a->rx >= 0 && a->rx <= MAX_R,
                    "gauss3d: every radius must be in 0 ... 32");
    ANODDPM_REQUIRE(a->rz > 0 || a->ry > 0 || a->rx > 0, "gauss3d: all three radii are 0 (nothing to filter: the result is the input)");
    ANODDPM_REQUIRE(a->S >= 1 && a->D >= 1 && a->H >= 1 && a->W >= 1, "gauss3d: S, D, H, W must be >= 1");
    constexpr int64_t LIMIT = (int64_t)1 << 31;
    const int64_t hw = (int64_t)a->H * a->W;                         // each factor below 2^31: no product here leaves an int64
    ANODDPM_REQUIRE(hw < LIMIT && hw * a->D < LIMIT && hw * a->D * a->S < LIMIT, "gauss3d: S*D*H*W must be below 2^31");
    const int64_t vol = hw * a->D, total = vol * a->S;
    const bool plane_pass = a->ry > 0 || a->rx > 0, two = a->rz > 0 && plane_pass;
    ANODDPM_REQUIRE(a->src && a->dst, "gauss3d: null pointer (src, dst)");
    ANODDPM_REQUIRE((a->rz == 0 || a->wz) && (a->ry == 0 || a->wy) && (a->rx == 0 || a->wx), "gauss3d: null pointer (the tap table of a filtered axis)");
    ANODDPM_REQUIRE(!two || a->tmp, "gauss3d: null pointer (tmp: the z pass and a plane pass both run)");
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= vol, "gauss3d: volumes overlap (src_stride < D*H*W)");
    const int64_t src_span = (a->S - 1) * (a->S == 1 ? 0 : a->src_stride) + vol;
    ANODDPM_REQUIRE(!overlap(a->src, src_span, a->dst, total), "gauss3d: dst overlaps src (the filter does not run in place)");
    ANODDPM_REQUIRE(!a->tmp || !overlap(a->src, src_span, a->tmp, total), "gauss3d: tmp overlaps src");
    ANODDPM_REQUIRE(!a->tmp || !overlap(a->dst, total, a->tmp, total), "gauss3d: tmp overlaps dst");
    const hipStream_t s = as_stream(stream);
    if (a->rz > 0)
        launch_pass(a->src, two ? a->tmp : a->dst, a->wz, nullptr, a->src_stride, 1, a->S, a->D, (int)hw, a->rz, 0, s);
    if (plane_pass)
        launch_pass(two ? a->tmp : a->src, a->dst, a->wy, a->wx, two ? vol : a->src_stride, a->D, (int64_t)a->S * a->D, a->H, a->W, a->ry, a->rx, s);
    return check_launch("gauss3d");
}
