// The step between the two passes of a two-pass detection: from a score plane and a threshold that lives on the
// device to the keep bytes a KnownRegion stores, the stitched start image of the second pass and the size of the region that
// is regenerated -- anoddpm_keep_mask (include/anoddpm_hip.h has the contract).  Per H x W plane it replaces
//   seed  = (score > thr) & roi;  grown = scipy.ndimage.binary_dilation(seed, iterations=r);  regen = grown & roi
//   keep  = ~regen;  stitched = numpy.where(regen, recon, real);  regen.sum()
// in ONE launch.  Every step compares, selects or counts integers: the outputs equal scipy's bit for bit, the same bits every run.
//
// Dilation.  r passes of the cross = one pass of the L1 ball of radius r, nothing outside the plane contributing (the mirror
// image of erode_kernel in postproc.hip, which counts the outside as 0 under an AND and so cannot be turned into a dilation by
// complementing).  A workgroup of 256 threads owns a TH x TW = 16 x 32 tile of one plane.  The staging loop loads the scores of
// the tile and its r-pixel halo, compares them with the plane's threshold (read once per workgroup), tests the roi and leaves
// two bits per cell in LDS: seed, inside-roi; zero outside the plane.  Pass 1 gives every staged row cell of the tile's columns
// its horizontal distance to the nearest seed, capped at r + 1; pass 2 marks a pixel when some row offset dy, |dy| <= r, has a
// distance <= r - |dy|.  2 (2r + 1) LDS reads per pixel instead of the ball's 2r(r + 1) + 1; lanes of a wave read consecutive
// LDS words.  The keep bytes and the C selects of the stitch follow with the 32 pixels of a tile row in consecutive lanes.
// The count is one ballot per wave, one LDS add per wave and one integer atomic add per workgroup; the status bits an atomic OR.
//
// What bounds it (profiles/keepmask_ab.txt).  The counts of a call share one or two cache lines, and adds from all over the chip
// to one line are carried out one after the other, about 8 ns each: with a workgroup per tile, 8192 of them took 64 of the 97 us
// of a 16 x 3 x 512^2 call that moves its 172 MB in 33 us without them.  So a workgroup takes `span` consecutive tiles of a tile
// row, one after the other, and adds once: span is 1 until the grid exceeds the 2048 workgroups the chip holds at a time (eight
// on each of 256 CUs; one plane of 256^2 is 128), then as large as keeps that many.  A single plane is bound by launch latency.
#include <math.h>
#include "common.h"

namespace {

constexpr int THREADS = 256, TH = 16, TW = 32, MAX_R = 8;
constexpr int SEED = 1, INSIDE = 2;                                  // the two bits of a staged cell
constexpr int64_t RESIDENT = 2048;                                   // workgroups the chip holds at a time: 8 on each of 256 CUs

__global__ __launch_bounds__(THREADS) void keep_mask_kernel(anoddpm_keep_mask_args a, int tiles_x, int tiles_y, int span)
{
    constexpr int RH = TH + 2 * MAX_R, RW = TW + 2 * MAX_R;
    static_assert(TH * TW == 2 * THREADS, "two pixels per thread, no ragged last round: the ballots below are wave-uniform");
    __shared__ int cell[RH][RW];                                     // SEED | INSIDE, zero outside the plane
    __shared__ int dist[RH][TW];                                     // horizontal distance to the nearest seed, r + 1: none within r
    __shared__ int s_status, s_count;

    const int tid = threadIdx.x;
    const int strips_x = (tiles_x + span - 1) / span;
    const int strips = strips_x * tiles_y;
    const int t = blockIdx.x % strips;
    const int64_t plane = blockIdx.x / strips;
    const int y0 = (t / strips_x) * TH;
    const int tx0 = (t % strips_x) * span, tx1 = min(tx0 + span, tiles_x);
    const int H = a.H, W = a.W, C = a.C, n = a.r;
    const int rh = TH + 2 * n, rw = TW + 2 * n;
    const int64_t hw = (int64_t)H * W;
    const float *__restrict__ score = a.score + plane * a.score_stride;
    const float *__restrict__ roi = a.roi ? a.roi + plane * a.roi_stride : nullptr;
    const float *__restrict__ real = a.real ? a.real + plane * a.real_stride : nullptr;
    const float *__restrict__ recon = a.real ? a.recon + plane * C * hw : nullptr;
    float *__restrict__ stitched = a.real ? a.stitched + plane * C * hw : nullptr;
    uint8_t *__restrict__ keep = a.keep + plane * hw;
    const float thr = a.threshold[plane * a.thr_stride];

    int st = 0, count = 0;
    if (tid == 0) {
        s_status = 0;
        s_count = 0;
        if (thr != thr) st |= ANODDPM_ROC_NAN;
    }
    for (int tx = tx0; tx < tx1; ++tx) {
        const int x0 = tx * TW;
        for (int i = tid; i < rh * rw; i += THREADS) {
            const int r = i / rw, c = i - r * rw;
            const int gy = y0 - n + r, gx = x0 - n + c;
            int v = 0;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const float s = score[(int64_t)gy * W + gx];
                if (s != s) st |= ANODDPM_ROC_NAN;
                bool inside = true;
                if (roi) {
                    const float m = roi[(int64_t)gy * W + gx];
                    if (!(m == 0.0f || m == 1.0f)) st |= ANODDPM_ROC_BAD_MASK;
                    inside = m == 1.0f;
                }
                v = (inside ? INSIDE : 0) | (inside && s > thr ? SEED : 0);
            }
            cell[r][c] = v;
        }
        __syncthreads();
        for (int i = tid; i < rh * TW; i += THREADS) {
            const int r = i / TW, c = i % TW, cc = c + n;
            int h = 0;
            while (h <= n && !((cell[r][cc - h] | cell[r][cc + h]) & SEED)) ++h;
            dist[r][c] = h;
        }
        __syncthreads();
        for (int i = tid; i < TH * TW; i += THREADS) {               // exactly two rounds for every thread
            const int r = i / TW, c = i % TW;
            const int gy = y0 + r, gx = x0 + c;
            const bool valid = gy < H && gx < W;
            bool grown = false;
            for (int dy = -n; dy <= n; ++dy) grown = grown || dist[r + n + dy][c] <= n - (dy < 0 ? -dy : dy);
            const bool regen = valid && grown && (cell[r + n][c + n] & INSIDE);
            if (valid) {
                const int64_t at = (int64_t)gy * W + gx;
                keep[at] = regen ? 0 : 1;
                if (real)
                    for (int ch = 0; ch < C; ++ch) {
                        const int64_t e = ch * hw + at;
                        const float x = real[e], y = recon[e];
                        stitched[e] = regen ? y : x;
                    }
            }
            count += __popcll(__ballot(regen));
        }
        __syncthreads();                                             // the next tile's staging overwrites cell and dist
    }
    if ((tid & 63) == 0 && count) atomicAdd(&s_count, count);
    if (st) atomicOr(&s_status, st);
    __syncthreads();
    if (tid == 0) {
        if (s_count) atomicAdd(&a.regen_count[plane], s_count);
        if (s_status) atomicOr(&a.status[plane], s_status);
    }
}

}  // namespace

extern "C" int anoddpm_keep_mask(const anoddpm_keep_mask_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "keep_mask: null args");
    ANODDPM_REQUIRE(a->score && a->threshold && a->keep && a->regen_count && a->status, "keep_mask: null pointer (score, threshold, keep, regen_count and status are required)");
    ANODDPM_REQUIRE(a->r >= 0 && a->r <= MAX_R, "keep_mask: r must be in 0 ... 8");
    ANODDPM_REQUIRE(a->S >= 1 && a->H >= 1 && a->W >= 1 && a->C >= 1, "keep_mask: S, H, W and C must be >= 1");
    const int64_t tiles = (int64_t)((a->H + TH - 1) / TH) * ((a->W + TW - 1) / TW);
    ANODDPM_REQUIRE(tiles <= 0x7fffffff / (int64_t)a->S, "keep_mask: S * tiles must be below 2^31");
    const int64_t hw = (int64_t)a->H * a->W;
    ANODDPM_REQUIRE(a->S == 1 || a->score_stride >= hw, "keep_mask: planes overlap (score_stride < H*W)");
    ANODDPM_REQUIRE(a->thr_stride == 0 || a->thr_stride == 1, "keep_mask: thr_stride must be 0 (one threshold) or 1 (one per plane)");
    ANODDPM_REQUIRE(!a->roi || a->roi_stride == 0 || a->roi_stride == hw, "keep_mask: roi_stride must be 0 (shared ROI) or H*W");
    const int set = (a->real != nullptr) + (a->recon != nullptr) + (a->stitched != nullptr);
    ANODDPM_REQUIRE(set == 0 || set == 3, "keep_mask: real, recon and stitched come together: all three or none");
    ANODDPM_REQUIRE(set == 0 || a->real_stride == 0 || a->real_stride == (int64_t)a->C * hw, "keep_mask: real_stride must be 0 (one image) or C*H*W");
    hipStream_t s = as_stream(stream);
    hipError_t e = hipMemsetAsync(a->regen_count, 0, sizeof(int32_t) * (size_t)a->S, s);
    if (e == hipSuccess) e = hipMemsetAsync(a->status, 0, sizeof(int32_t) * (size_t)a->S, s);
    if (e != hipSuccess) {
        set_error("keep_mask: hipMemsetAsync(regen_count / status): %s", hipGetErrorString(e));
        return ANODDPM_ELAUNCH;
    }
    const int tiles_x = (a->W + TW - 1) / TW, tiles_y = (a->H + TH - 1) / TH;
    const int span = (int)min((int64_t)tiles_x, max((int64_t)1, a->S * tiles / RESIDENT));
    const int strips_x = (tiles_x + span - 1) / span;
    hipLaunchKernelGGL(keep_mask_kernel, dim3((unsigned)(a->S * strips_x * tiles_y)), dim3(THREADS), 0, s, *a, tiles_x, tiles_y, span);
    return check_launch("keep_mask");
}
