// Mean structural similarity (Wang et al. 2004) of batched image pairs -- replaces, per segment (one [C][H][W] pair),
//   skimage.metrics.structural_similarity(real, recon, channel_axis=...)          evaluation.py:46-47; detection.py:241-246,
//                                                                                  360-362, 765-768, 855-858
// Definition (the contract; x = real, y = recon, fp32 in memory, every operation after the load in fp64):
//   separable window w of odd length win (weights sum to 1) along W then along H, boundary rule "reflect"
//   (d c b a | a b c d | d c b a, scipy.ndimage mode "reflect");
//   ux = F(x), uy = F(y), uxx = F(x*x), uyy = F(y*y), uxy = F(x*y)
//   vx = cn*(uxx - ux*ux), vy = cn*(uyy - uy*uy), vxy = cn*(uxy - ux*uy)
//   C1 = (K1*R)^2, C2 = (K2*R)^2, R = data_range
//   S = ((2*ux*uy + C1) * (2*vxy + C2)) / ((ux*ux + uy*uy + C1) * (vx + vy + C2))
//   mssim = mean of S over all channels and the interior p <= i < H-p, p <= j < W-p, p = (win-1)/2
// Window modes: uniform (w = 1/win, cn = win^2/(win^2-1) as skimage's sample covariance) and gaussian (sigma 1.5, win 11, cn 1).
//
// Arrangement: a workgroup of 256 threads owns a TH x TW = 16 x 32 output tile of one channel of one segment.
//   1. the tile plus its win-1 halo of x and y goes to LDS once as fp32 (reflect indexing at the image edges): 2 x 30 x 46 words
//   2. row pass: the five planes F_W(x), F_W(y), F_W(x*x), F_W(y*y), F_W(x*y) of the (TH + win - 1) x TW region as fp64 in LDS
//      (5 x 30 x 32 doubles = 37.5 KB; about 51 KB of LDS in all, three workgroups per CU).  Each value is
//      w[0]*v[0] + w[1]*v[1] + ... accumulated from tap 0 upwards, never a sliding add/subtract recurrence; the three
//      second-order planes are formed the same way, so real == recon gives uxx == uyy == uxy bit for bit and S == 1.0 exactly
//   3. column pass over the planes in the same tap order, S, the optional fp32 map (all pixels, boundary included)
//   4. interior S values (others count as +0.0) are summed per thread in pixel order, then over the workgroup by a halving tree
//      in LDS; the workgroup writes ONE partial.  A second tiny launch folds the partials of a segment in a fixed order (thread t
//      takes partials t, t + 256, ... in turn, then the same halving tree) and divides by the interior count.
// Lanes of a wave touch consecutive LDS words in every pass (no bank conflicts).  No atomics, no ordering between workgroups, no
// allocation and no host synchronisation: capturable in a hipGraph.  Same input, same bits, every run.  NaN / inf in the images
// propagate into that segment's mssim only.
// Bound by LDS traffic and fp64 VALU issue (about 28 * win fp64 operations per output pixel, halo rows included), not by HBM:
// every input word is read once per tile that covers it.  Compiled with -ffp-contract=off like the other metric kernels.
#include <math.h>
#include "common.h"

namespace {

constexpr int THREADS = 256, TH = 16, TW = 32, MAXWIN = 15;
constexpr int RH = TH + MAXWIN - 1, RW = TW + MAXWIN - 1;           // staged region: at most 30 x 46

struct Weights { double w[MAXWIN]; };

__device__ __forceinline__ int reflect(int i, int n)
{
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return min(max(i, 0), n - 1);                                    // tile overhang past the reflected band: any valid pixel
}

// sum of red[0 .. THREADS) by a halving tree: red[t] += red[t + off], off = 128, 64, ... 1
__device__ __forceinline__ double block_tree_sum(double *red, int tid)
{
    __syncthreads();
    for (int off = THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] = red[tid] + red[tid + off];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(THREADS) void ssim_tile_kernel(anoddpm_ssim_args a, Weights wt, int tiles_x, int tiles_y, double c1,
                                                            double c2, double *__restrict__ partial)
{
    __shared__ float sx[RH][RW], sy[RH][RW];
    __shared__ double plane[5][RH][TW];
    __shared__ double red[THREADS];

    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int tile = blockIdx.x % tiles;
    const int64_t sc = blockIdx.x / tiles;                           // segment * C + channel
    const int seg = (int)(sc / a.C), ch = (int)(sc % a.C);
    const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
    const int win = a.win, p = (win - 1) / 2, H = a.H, W = a.W;
    const int rh = TH + win - 1, rw = TW + win - 1;
    const int64_t img = (int64_t)H * W;
    const float *__restrict__ x = a.real + (int64_t)seg * a.real_stride + (int64_t)ch * img;
    const float *__restrict__ y = a.recon + (int64_t)seg * a.recon_stride + (int64_t)ch * img;

    // ---- 1. stage the tile and its halo
    for (int i = tid; i < rh * rw; i += THREADS) {
        const int r = i / rw, c = i - r * rw;
        const int64_t o = (int64_t)reflect(y0 - p + r, H) * W + reflect(x0 - p + c, W);
        sx[r][c] = x[o];
        sy[r][c] = y[o];
    }
    __syncthreads();

    // ---- 2. row pass
    for (int i = tid; i < rh * TW; i += THREADS) {
        const int r = i / TW, c = i % TW;
        double fx = 0.0, fy = 0.0, fxx = 0.0, fyy = 0.0, fxy = 0.0;
        for (int k = 0; k < win; ++k) {
            const double w = wt.w[k], xv = (double)sx[r][c + k], yv = (double)sy[r][c + k];
            const double tx = w * xv, ty = w * yv, txx = w * (xv * xv), tyy = w * (yv * yv), txy = w * (xv * yv);
            if (k == 0) { fx = tx; fy = ty; fxx = txx; fyy = tyy; fxy = txy; }
            else { fx = fx + tx; fy = fy + ty; fxx = fxx + txx; fyy = fyy + tyy; fxy = fxy + txy; }
        }
        plane[0][r][c] = fx;
        plane[1][r][c] = fy;
        plane[2][r][c] = fxx;
        plane[3][r][c] = fyy;
        plane[4][r][c] = fxy;
    }
    __syncthreads();

    // ---- 3. column pass, S, map; 4. the thread's interior sum in pixel order
    double acc = 0.0;
    for (int i = tid; i < TH * TW; i += THREADS) {
        const int r = i / TW, c = i % TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        double u[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double f = wt.w[0] * plane[q][r][c];
            for (int k = 1; k < win; ++k) f = f + wt.w[k] * plane[q][r + k][c];
            u[q] = f;
        }
        const double ux = u[0], uy = u[1];
        const double vx = a.cn * (u[2] - ux * ux), vy = a.cn * (u[3] - uy * uy), vxy = a.cn * (u[4] - ux * uy);
        const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2;
        const double b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
        const double s = (a1 * a2) / (b1 * b2);
        if (a.map) a.map[sc * img + (int64_t)gy * W + gx] = (float)s;
        const bool interior = gy >= p && gy < H - p && gx >= p && gx < W - p;
        acc = acc + (interior ? s : 0.0);
    }
    red[tid] = acc;
    const double total = block_tree_sum(red, tid);
    if (tid == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(THREADS) void ssim_fold_kernel(const double *__restrict__ partial, double *__restrict__ mssim,
                                                            int per_segment, double count)
{
    __shared__ double red[THREADS];
    const int tid = threadIdx.x;
    const double *p = partial + (int64_t)blockIdx.x * per_segment;
    double acc = 0.0;
    for (int i = tid; i < per_segment; i += THREADS) acc = acc + p[i];
    red[tid] = acc;
    const double total = block_tree_sum(red, tid);
    if (tid == 0) mssim[blockIdx.x] = total / count;
}

bool dims_ok(int32_t S, int32_t C, int32_t H, int32_t W)
{
    if (S < 1 || C < 1 || H < 1 || W < 1) return false;
    const int64_t tiles = (int64_t)((H + TH - 1) / TH) * ((W + TW - 1) / TW);
    return tiles * C <= 0x7fffffff / (int64_t)S;                     // one workgroup per (segment, channel, tile): a 1-D grid
}

}  // namespace

extern "C" int64_t anoddpm_ssim_workspace_bytes(int32_t S, int32_t C, int32_t H, int32_t W)
{
    if (!dims_ok(S, C, H, W)) return -1;
    return (int64_t)S * C * ((H + TH - 1) / TH) * ((W + TW - 1) / TW) * (int64_t)sizeof(double);
}

extern "C" int anoddpm_ssim(const anoddpm_ssim_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "ssim: null args");
    ANODDPM_REQUIRE(a->real && a->recon && a->workspace && a->mssim, "ssim: null pointer");
    ANODDPM_REQUIRE(a->S >= 1, "ssim: S must be >= 1");
    ANODDPM_REQUIRE(dims_ok(a->S, a->C, a->H, a->W), "ssim: C, H, W must be >= 1 and S * C * tiles below 2^31");
    ANODDPM_REQUIRE(a->win >= 3 && a->win <= MAXWIN && (a->win & 1), "ssim: win must be odd and in 3 ... 15");
    ANODDPM_REQUIRE(a->win <= a->H && a->win <= a->W, "ssim: win exceeds the image (win > min(H, W))");
    ANODDPM_REQUIRE(a->mode == ANODDPM_SSIM_UNIFORM || a->mode == ANODDPM_SSIM_GAUSSIAN, "ssim: mode must be uniform (0) or gaussian (1)");
    ANODDPM_REQUIRE(a->mode != ANODDPM_SSIM_GAUSSIAN || a->win == 11, "ssim: the gaussian window (sigma 1.5, truncate 3.5) has win 11");
    const int64_t n = (int64_t)a->C * a->H * a->W;
    ANODDPM_REQUIRE(a->S == 1 || a->recon_stride >= n, "ssim: recon segments overlap (recon_stride < C*H*W)");
    ANODDPM_REQUIRE(a->S == 1 || a->real_stride == 0 || a->real_stride >= n, "ssim: real_stride must be 0 (shared real) or >= C*H*W");
    ANODDPM_REQUIRE(a->workspace_bytes >= anoddpm_ssim_workspace_bytes(a->S, a->C, a->H, a->W), "ssim: workspace too small");

    Weights wt;
    for (int k = 0; k < MAXWIN; ++k) wt.w[k] = 0.0;
    if (a->mode == ANODDPM_SSIM_GAUSSIAN) {
        // scipy.ndimage's _gaussian_kernel1d(sigma = 1.5, radius = 5): exp(-0.5 / sigma^2 * k^2), normalised by the sum
        const double sigma = 1.5;
        double sum = 0.0;
        for (int k = 0; k < a->win; ++k) {
            const double d = (double)(k - (a->win - 1) / 2);
            wt.w[k] = exp(-0.5 / (sigma * sigma) * (d * d));
            sum += wt.w[k];
        }
        for (int k = 0; k < a->win; ++k) wt.w[k] /= sum;
    } else {
        for (int k = 0; k < a->win; ++k) wt.w[k] = 1.0 / (double)a->win;
    }
    const double c1 = (a->K1 * a->data_range) * (a->K1 * a->data_range), c2 = (a->K2 * a->data_range) * (a->K2 * a->data_range);
    const int tiles_x = (a->W + TW - 1) / TW, tiles_y = (a->H + TH - 1) / TH;
    const int per_segment = a->C * tiles_x * tiles_y;
    const int p = (a->win - 1) / 2;
    const double count = (double)a->C * (double)(a->H - 2 * p) * (double)(a->W - 2 * p);
    double *partial = static_cast<double *>(a->workspace);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(a->S * per_segment)), dim3(THREADS), 0, s, *a, wt, tiles_x, tiles_y, c1, c2, partial);
    hipLaunchKernelGGL(ssim_fold_kernel, dim3(a->S), dim3(THREADS), 0, s, partial, a->mssim, per_segment, count);
    return check_launch("ssim");
}
