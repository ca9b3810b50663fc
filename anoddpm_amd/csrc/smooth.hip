// Gaussian smoothing and image-level scores of anomaly maps -- the two steps the texture protocol (Bergmann et al., MVTec AD)
// puts between a map and its scores.  Replaces, per H x W plane or per image,
//   scipy.ndimage.gaussian_filter(plane, sigma, truncate=truncate)                         anoddpm_gauss2d
//   numpy.max / numpy.mean / numpy.partition(image.ravel(), n - k)[n - k:].mean()           anoddpm_map_scores
// (include/anoddpm_hip.h has the contract).  Compiled with -ffp-contract=off: both are statements about a fixed sequence of
// fp64 operations.
//
// Gaussian.  scipy filters axis 0 into an fp32 array and then axis 1 from it; a line is read as fp64 and the symmetric kernel
// is applied as  acc = v[i] w[r];  acc += (v[i+j] + v[i-j]) w[r+j]  for j = -r ... -1, every product and sum rounded once.  A
// workgroup of 256 threads owns a TILE x TILE = 32 x 32 tile of one plane:
//   stage    the tile and its r-halo, (32 + 2r)^2 fp32 words, with the reflection resolved (m = i mod 2n; m >= n -> 2n-1-m), so a
//            plane narrower than the radius reflects as often as it has to
//   axis 0   the 32 tile rows of every staged column, (32 + 2r) columns wide, into an fp32 LDS buffer: that store is scipy's
//            rounding between the axes
//   axis 1   the 32 x 32 outputs from that buffer
// In both passes the lanes of a wave sit on consecutive columns and walk the taps together: consecutive LDS words, no bank
// conflict, and the weight of a tap is one broadcast read.  Bound by the fp64 VALU: (2 TILE + 2r)/TILE * (r + 1) multiplies
// and (2 TILE + 2r)/TILE * 2r adds per output pixel (r + 1 products per axis; the axis-0 pass also runs over the 2r halo
// columns), each tap with two LDS reads and two fp32 -> fp64 conversions in front of it.  LDS:
// ((32 + 2r)^2 + 32 (32 + 2r)) * 4 + 264 bytes, asked for per launch -- 24840 at sigma 4 (r = 16), 49416 at r = 32, inside the
// 64 KB a workgroup gets without an attribute; a 32 x 64 tile at r = 32 would need exactly 64 KB and leave no room for the weights.
//
// Scores.  One workgroup of 1024 threads per image, five passes over it, eight loads in flight per thread.  The k-th largest
// value v_k: a radix select on the 31-bit patterns, four passes of 8 bits over an LDS histogram (integer atomics only; the lanes
// of a wave that hit the same bin add through one atomic) -- the select of csrc/surface.hip restated for fp32 input read in place
// and a rank counted from the top, the bin found by one wave's scan instead of one thread's walk; that one walks packed uint32
// words under its own kernel's thread count, and sharing it would have meant editing that file.  The first pass also gives the
// status bits, the maximum (on the bit pattern) and the sum; the last pass the count and sum of the values above v_k.  Sums:
// per-thread strided partials, then the halving tree of surface.hip's means.
#include <math.h>
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------- gaussian
constexpr int THREADS = 256, TILE = 32, MAX_R = ANODDPM_GAUSS_MAX_RADIUS;

__device__ __forceinline__ int reflect_periodic(int i, int n)
{
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m >= n ? p - 1 - m : m;
}

__global__ __launch_bounds__(THREADS) void gauss_kernel(anoddpm_gauss_args a, int tiles_x, int tiles_y)
{
    extern __shared__ double smem[];
    const int r = a.radius, RW = TILE + 2 * r;                       // staged tile: RW x RW
    double *wl = smem;                                               // [MAX_R + 1]
    float *tile = reinterpret_cast<float *>(smem + MAX_R + 1);       // [RW][RW]
    float *mid = tile + RW * RW;                                     // [TILE][RW]: axis 0 done, rounded to fp32

    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int t = blockIdx.x % tiles;
    const int64_t plane = blockIdx.x / tiles;
    const int y0 = (t / tiles_x) * TILE, x0 = (t % tiles_x) * TILE;
    const int H = a.H, W = a.W;
    const float *__restrict__ src = a.src + plane * a.src_stride;
    float *__restrict__ dst = a.dst + plane * (int64_t)H * W;

    if (tid <= r) wl[tid] = a.w[tid];
    for (int i = tid; i < RW * RW; i += THREADS) {
        const int y = i / RW, x = i - y * RW;
        tile[i] = src[(int64_t)reflect_periodic(y0 - r + y, H) * W + reflect_periodic(x0 - r + x, W)];
    }
    __syncthreads();

    const double wc = wl[r];
    for (int i = tid; i < TILE * RW; i += THREADS) {
        const int y = i / RW, x = i - y * RW;
        const float *col = tile + (y + r) * RW + x;                  // the centre tap
        double acc = (double)col[0] * wc;
        for (int j = r; j >= 1; --j) acc += ((double)col[-j * RW] + (double)col[j * RW]) * wl[r - j];
        mid[i] = (float)acc;
    }
    __syncthreads();

    for (int i = tid; i < TILE * TILE; i += THREADS) {
        const int y = i / TILE, x = i % TILE;
        const int gy = y0 + y, gx = x0 + x;
        if (gy >= H || gx >= W) continue;
        const float *row = mid + y * RW + x + r;
        double acc = (double)row[0] * wc;
        for (int j = r; j >= 1; --j) acc += ((double)row[-j] + (double)row[j]) * wl[r - j];
        dst[(int64_t)gy * W + gx] = (float)acc;
    }
}

// ---------------------------------------------------------------------------------------------------- image-level scores
constexpr int STAT_THREADS = 1024, STAT_WAVES = STAT_THREADS / 64;

// sum over the workgroup in the fixed order of include/anoddpm_hip.h; every thread returns the total
template <typename T>
__device__ T block_sum(T v, T *wsum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();                                                 // wsum may still be read from the call before
    if (lane == 0) wsum[wave] = v;
    __syncthreads();
    v = wsum[lane & (STAT_WAVES - 1)];
#pragma unroll
    for (int off = STAT_WAVES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Every element of the segment, BATCH loads in flight per thread: f(valid, raw bits) for the elements tid, tid + 1024, ... in that
// order.  All lanes of a wave call f the same number of times (f may ballot); `valid` is false past the end.
constexpr int BATCH = 8;
template <typename F>
__device__ __forceinline__ void for_each_element(const float *__restrict__ v, uint32_t n, F f)
{
    const uint32_t *__restrict__ bits = reinterpret_cast<const uint32_t *>(v);
    for (uint32_t base = 0; base < n; base += BATCH * STAT_THREADS) {          // n <= 2^24: no index wraps
        uint32_t w[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const uint32_t i = base + u * STAT_THREADS + threadIdx.x;
            w[u] = i < n ? bits[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u) f(base + u * STAT_THREADS + threadIdx.x < n, w[u]);
    }
}

// ++hist[bin] for the lanes that `take`.  The lanes of a wave that share the first taker's bin add their count through one
// atomic, twice over; what is left adds one by one.  Maps concentrate in a few exponents (and a constant map in one pattern), where
// 64 single adds to one word would queue up behind each other.  Integer counts: the order of the adds cannot show.
__device__ __forceinline__ void hist_add(uint32_t *hist, bool take, uint32_t bin)
{
    const int lane = threadIdx.x & 63;
    unsigned long long left = __ballot(take);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (left == 0) break;                                        // wave-uniform
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

__global__ __launch_bounds__(STAT_THREADS) void map_scores_kernel(anoddpm_map_scores_args a)
{
    __shared__ uint32_t hist[256], sel[2], s_max;
    __shared__ int s_status;
    __shared__ double wsum[STAT_WAVES];
    __shared__ uint32_t wcnt[STAT_WAVES];

    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const uint32_t n = (uint32_t)a.n, k = (uint32_t)a.k;
    const float *__restrict__ v = a.src + (int64_t)s * a.src_stride;
    constexpr uint32_t ABS = 0x7fffffffu;                            // -0.0 is +0.0; the order of the patterns is the order of the values

    // v_k: the pattern of descending rank k - 1, from the top byte down.  The first pass over the data also gives the status
    // bits, the maximum and the sum.
    int st = 0;
    uint32_t mx = 0;
    double sum = 0.0;
    uint32_t prefix = 0, mask = 0, rank = k - 1u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        if (tid == 0 && shift == 24) { s_max = 0; s_status = 0; }
        __syncthreads();
        if (shift == 24) {
            for_each_element(v, n, [&](bool valid, uint32_t raw) {
                const float x = __uint_as_float(raw);
                if (x != x) st |= ANODDPM_ROC_NAN;
                else if (x == INFINITY || x == -INFINITY) st |= ANODDPM_ROC_INF;
                if (x < 0.0f) st |= ANODDPM_ROC_NEGATIVE;
                const uint32_t w = raw & ABS;
                mx = max(mx, w);
                sum += (double)__uint_as_float(w);                   // +0.0 past the end: the partial is >= 0, nothing changes
                hist_add(hist, valid, w >> 24);
            });
            if (st) atomicOr(&s_status, st);
            atomicMax(&s_max, mx);
        } else {
            for_each_element(v, n, [&](bool valid, uint32_t raw) {
                const uint32_t w = raw & ABS;
                hist_add(hist, valid && (w & mask) == prefix, (w >> shift) & 255u);
            });
        }
        __syncthreads();
        if (tid < 64) {                                              // lane l owns the bins 4l ... 4l + 3; ranks count from the top bin down
            const uint32_t c = hist[4 * lane] + hist[4 * lane + 1] + hist[4 * lane + 2] + hist[4 * lane + 3];
            uint32_t incl = c;                                       // elements in this lane's bins and in all higher ones
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t up = __shfl_down(incl, off);
                if (lane + off < 64) incl += up;
            }
            const uint32_t excl = incl - c;
            if (excl <= rank && rank < incl) {                       // exactly one lane: rank is below the number of elements counted
                uint32_t b = 4u * lane + 3u, q = rank - excl;
                while (b > 4u * lane && q >= hist[b]) { q -= hist[b]; --b; }
                sel[0] = b;
                sel[1] = q;
            }
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        rank = sel[1];
        mask |= 255u << shift;
    }
    const uint32_t vk = prefix;
    sum = block_sum(sum, wsum);

    uint32_t above = 0;
    double sum_above = 0.0;
    for_each_element(v, n, [&](bool valid, uint32_t raw) {
        const uint32_t w = raw & ABS;
        if (valid && w > vk) {
            ++above;
            sum_above += (double)__uint_as_float(w);
        }
    });
    sum_above = block_sum(sum_above, wsum);
    above = block_sum(above, wcnt);
    if (tid == 0) {
        a.status[s] = s_status;
        a.max[s] = __uint_as_float(s_max);
        a.mean[s] = sum / (double)n;
        const double rest = (double)(k - above) * (double)__uint_as_float(vk);
        a.topk_mean[s] = (sum_above + rest) / (double)k;
    }
}

// one workgroup per (plane, tile): a 1-D grid
bool tiles_ok(int32_t S, int32_t H, int32_t W)
{
    if (S < 1 || H < 1 || W < 1 || H >= (1 << 30) || W >= (1 << 30)) return false;       // 2 H and 2 W, the reflection's period, fit an int
    const int64_t tiles = (int64_t)((H + TILE - 1) / TILE) * ((W + TILE - 1) / TILE);
    return tiles <= 0x7fffffff / (int64_t)S;
}

}  // namespace

extern "C" int anoddpm_gauss2d(const anoddpm_gauss_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "gauss2d: null args");
    ANODDPM_REQUIRE(a->src && a->dst && a->w, "gauss2d: null pointer");
    ANODDPM_REQUIRE(a->radius >= 1 && a->radius <= MAX_R, "gauss2d: radius must be in 1 ... 32");
    ANODDPM_REQUIRE(tiles_ok(a->S, a->H, a->W), "gauss2d: S, H, W must be >= 1, H and W below 2^30 and S * tiles below 2^31");
    const int64_t hw = (int64_t)a->H * a->W;
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= hw, "gauss2d: planes overlap (src_stride < H*W)");
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(a->src), d0 = reinterpret_cast<uintptr_t>(a->dst);
    const uintptr_t s1 = s0 + sizeof(float) * (uintptr_t)((a->S - 1) * (a->S == 1 ? 0 : a->src_stride) + hw);
    const uintptr_t d1 = d0 + sizeof(float) * (uintptr_t)(a->S * hw);
    ANODDPM_REQUIRE(s1 <= d0 || d1 <= s0, "gauss2d: dst overlaps src (the filter does not run in place)");
    const int rw = TILE + 2 * a->radius;
    const size_t lds = sizeof(double) * (MAX_R + 1) + sizeof(float) * (size_t)(rw * rw + TILE * rw);
    const int tiles_x = (a->W + TILE - 1) / TILE, tiles_y = (a->H + TILE - 1) / TILE;
    hipLaunchKernelGGL(gauss_kernel, dim3((unsigned)(a->S * tiles_x * tiles_y)), dim3(THREADS), lds, as_stream(stream), *a, tiles_x, tiles_y);
    return check_launch("gauss2d");
}

extern "C" int anoddpm_map_scores(const anoddpm_map_scores_args *a, void *stream)
{
    using namespace anoddpm;
    ANODDPM_REQUIRE(a != nullptr, "map_scores: null args");
    ANODDPM_REQUIRE(a->src && a->max && a->mean && a->topk_mean && a->status, "map_scores: null pointer");
    ANODDPM_REQUIRE(a->S >= 1, "map_scores: S must be >= 1");
    ANODDPM_REQUIRE(a->n >= 1 && a->n <= ANODDPM_MAP_SCORES_MAX_N, "map_scores: n must be in 1 ... 16777216 (one workgroup per segment)");
    ANODDPM_REQUIRE(a->k >= 1 && a->k <= a->n, "map_scores: k must be in 1 ... n");
    ANODDPM_REQUIRE(a->S == 1 || a->src_stride >= a->n, "map_scores: segments overlap (src_stride < n)");
    hipLaunchKernelGGL(map_scores_kernel, dim3((unsigned)a->S), dim3(STAT_THREADS), 0, as_stream(stream), *a);
    return check_launch("map_scores");
}
