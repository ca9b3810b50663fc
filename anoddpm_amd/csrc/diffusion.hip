// Fused forward / reverse diffusion updates -- replaces the ~25 ATen dispatches per step of
// GaussianDiffusion.py:32-36 (extract), :361-382 (sample_q, sample_q_gradual), :228-230
// (predict_x_0_from_eps), :253-267 (posterior mean), :287 (clamp) and :314-317 (sample_p).
// HBM-bound elementwise work: sample_q moves 12 B/pixel, the reverse update 16 B/pixel.
// Compiled with -ffp-contract=off so every product and sum rounds exactly as the reference's
// separate fp32 ATen kernels do (results are bit-identical to its CPU path).
// Seeded Gaussian noise: the *_gauss forms generate their normals in registers from a counter-based stream instead
// of reading a noise tensor (reverse update 12 B/pixel, no noise launch).
#include "common.h"

namespace {

// ---------------------------------------------------------------- Philox4x32-10 (Random123) -> Box-Muller normals
struct PhiloxWords {
    uint32_t w[4];
};

__host__ __device__ __forceinline__ PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return PhiloxWords{{c0, c1, c2, c3}};
}

// The key block of the C ABI as the kernels receive it (seed and stream ids are read from device memory at run time).
struct PhiloxKey {
    const uint64_t *seed;
    const int32_t *streams;
    uint32_t stream0, domain;
};

// What one sample's threads share: the key and the three counter words that do not depend on the element.
struct PhiloxSample {
    uint32_t k0, k1, stream, step, domain;
};

__device__ __forceinline__ PhiloxSample philox_sample(const PhiloxKey &key, int b, uint32_t step)
{
    const uint64_t seed = *key.seed;
    PhiloxSample s;
    s.k0 = (uint32_t)seed;
    s.k1 = (uint32_t)(seed >> 32);
    s.stream = key.streams ? (uint32_t)key.streams[b] : key.stream0 + (uint32_t)b;
    s.step = step;
    s.domain = key.domain;
    return s;
}

__device__ __forceinline__ float philox_unit(uint32_t w)
{
    return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f;      // ((w >> 9) + 0.5) * 2^-23: exact, in (0, 1)
}

// The four normals of one quad.  The ONLY place normals are made: anoddpm_philox_fill and the fused kernels share it, which
// (with -ffp-contract=off) is what makes fused == fill + unfused bit for bit.
__device__ __forceinline__ void philox_normals(const PhiloxSample &s, uint32_t quad, float z[4])
{
    const PhiloxWords p = philox4x32_10(quad, s.stream, s.step, s.domain, s.k0, s.k1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float r = sqrtf(-2.0f * logf(philox_unit(p.w[2 * h])));
        float sn, cs;
        sincospif(2.0f * philox_unit(p.w[2 * h + 1]), &sn, &cs);
        z[2 * h] = r * cs;
        z[2 * h + 1] = r * sn;
    }
}

// python-style step of sample b (the update kernels' own normalisation): t < 0 means t + T; out of range -> 0 (those samples are
// NaN in the update kernels)
__device__ __forceinline__ uint32_t philox_step_of(long long ti, int T)
{
    if (T > 0) {
        ti = ti < 0 ? ti + T : ti;
        if (ti < 0 || ti >= T) ti = 0;
    }
    return (uint32_t)ti;
}

template <int VEC>
__global__ __launch_bounds__(256) void philox_fill_kernel(uint32_t *__restrict__ out, int kind, int64_t n, PhiloxKey key,
                                                          const int64_t *__restrict__ t, uint32_t step0, int T)
{
    const int b = blockIdx.y;
    const PhiloxSample s = philox_sample(key, b, t ? philox_step_of(t[b], T) : step0);
    out += (int64_t)b * n;
    const int64_t nq = (n + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        uint32_t v[4];
        if (kind == 0) {
            const PhiloxWords p = philox4x32_10((uint32_t)q, s.stream, s.step, s.domain, s.k0, s.k1);
#pragma unroll
            for (int l = 0; l < 4; ++l) v[l] = p.w[l];
        } else {
            float z[4];
            philox_normals(s, (uint32_t)q, z);
#pragma unroll
            for (int l = 0; l < 4; ++l) v[l] = __float_as_uint(z[l]);
        }
        if (VEC == 4) {
            *reinterpret_cast<uint4 *>(out + 4 * q) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (4 * q + l < n) out[4 * q + l] = v[l];
        }
    }
}

// GAUSS: `noise` is not read; the normals come from `key` (one thread owns whole quads) and go to noise_out if that is given.
template <int VEC, bool GAUSS>
__global__ __launch_bounds__(256) void q_sample_kernel(float *__restrict__ out, const float *__restrict__ x,
                                                       const float *__restrict__ noise,
                                                       const int64_t *__restrict__ t,
                                                       const float *__restrict__ ca,
                                                       const float *__restrict__ cb, int64_t n, int T,
                                                       float *__restrict__ noise_out, PhiloxKey key)
{
    const int b = blockIdx.y;
    long long ti = t[b];
    ti = ti < 0 ? ti + T : ti;                       // python-style negative index
    // the reference's extract() raises IndexError for t outside [-T, T); a kernel cannot raise, so it never reads out
    // of bounds and poisons the sample with NaN instead (the host wrappers validate host-built t, see diffusion.py)
    const bool bad = ti < 0 || ti >= T;
    ti = bad ? 0 : ti;
    const float qnan = __builtin_nanf("");
    const float a = bad ? qnan : ca[ti], c = bad ? qnan : cb[ti];
    const int64_t base = (int64_t)b * n;
    if (GAUSS) {
        const PhiloxSample ps = philox_sample(key, b, (uint32_t)ti);
        const int64_t nq = (n + 3) >> 2;
        for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
            float z[4];
            philox_normals(ps, (uint32_t)q, z);
            const int64_t i = base + 4 * q;
            if (VEC == 4) {
                const float4 xv = *reinterpret_cast<const float4 *>(x + i);
                float4 o;
                o.x = a * xv.x + c * z[0];
                o.y = a * xv.y + c * z[1];
                o.z = a * xv.z + c * z[2];
                o.w = a * xv.w + c * z[3];
                *reinterpret_cast<float4 *>(out + i) = o;
                if (noise_out) *reinterpret_cast<float4 *>(noise_out + i) = make_float4(z[0], z[1], z[2], z[3]);
            } else {
#pragma unroll
                for (int l = 0; l < 4; ++l) {
                    if (4 * q + l < n) {
                        out[i + l] = a * x[i + l] + c * z[l];
                        if (noise_out) noise_out[i + l] = z[l];
                    }
                }
            }
        }
        return;
    }
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC; i < n; i += (int64_t)gridDim.x * 256 * VEC) {
        if (VEC == 4) {
            const float4 xv = *reinterpret_cast<const float4 *>(x + base + i);
            const float4 nv = *reinterpret_cast<const float4 *>(noise + base + i);
            float4 o;
            o.x = a * xv.x + c * nv.x;
            o.y = a * xv.y + c * nv.y;
            o.z = a * xv.z + c * nv.z;
            o.w = a * xv.w + c * nv.w;
            *reinterpret_cast<float4 *>(out + base + i) = o;
        } else {
            out[base + i] = a * x[base + i] + c * noise[base + i];
        }
    }
}

struct StepCoef {
    float recip, recipm1, coef1, coef2, sigma;
};

// The strided sampler's operands, all read on the device at run time: the fp64 alphas_cumprod table, one stride word
// and one eta word.  Unused (zero) in the ancestral instantiations.
struct StridedArgs {
    const double *acp;
    const int32_t *stride;
    const float *eta;
};

// Coefficients of one strided step from t to s = t - stride (Song et al., DDIM, eq. 12 / 16), fp64, each rounded to fp32 once:
// out = {sqrt(a_s), sqrt(max(1 - a_s - var, 0)), sqrt(var)}, var = eta^2 (1 - a_s) / (1 - a_t) (1 - a_t / a_s), a_s = 1 for s < 0
// (that step lands on x_0).  `ti` is the normalised, in-range timestep.  A bad sample or a stride < 1 poisons the first
// coefficient, and with it every element of the sample, with NaN; it never reads outside the table.
__device__ __forceinline__ void strided_coef(const StridedArgs &sa, long long ti, bool bad, float out[3])
{
    const long long stride = *sa.stride;
    const double eta = (double)*sa.eta;
    const bool poison = bad || stride < 1;
    const long long si = poison ? -1 : ti - stride;
    const double at = sa.acp[ti], as = si < 0 ? 1.0 : sa.acp[si];
    const double var = (eta * eta) * ((1.0 - as) / (1.0 - at)) * (1.0 - at / as);
    out[0] = poison ? __builtin_nanf("") : (float)sqrt(as);
    out[1] = (float)sqrt(fmax((1.0 - as) - var, 0.0));
    out[2] = (float)sqrt(var);
}

// STRIDED: coef1 / coef2 are the x_0 and direction coefficients, the direction is the eps consistent with the clipped x_0, and a
// zero sigma adds no noise term at all.
template <bool STRIDED>
__device__ __forceinline__ float reverse_one(float xt, float e, float nz, const StepCoef &k, float *px0, float *pmean)
{
    const float p = k.recip * xt;
    const float raw = p - k.recipm1 * e;
    const float x0 = fminf(fmaxf(raw, -1.0f), 1.0f);
    float mean;
    if (STRIDED) {
        const float dir = x0 == raw ? e : (p - x0) / k.recipm1;
        mean = k.coef1 * x0 + k.coef2 * dir;
    } else {
        mean = k.coef1 * x0 + k.coef2 * xt;
    }
    *px0 = x0;
    *pmean = mean;
    if (STRIDED && k.sigma == 0.0f) return mean;
    return mean + k.sigma * nz;
}

template <bool STRIDED>
__device__ __forceinline__ void reverse_store4(const anoddpm_p_update_args &a, const StepCoef &k, int64_t i, const float4 nv)
{
    const float4 xv = *reinterpret_cast<const float4 *>(a.x_t + i);
    const float4 ev = *reinterpret_cast<const float4 *>(a.eps + i);
    float4 o, p0, mu;
    o.x = reverse_one<STRIDED>(xv.x, ev.x, nv.x, k, &p0.x, &mu.x);
    o.y = reverse_one<STRIDED>(xv.y, ev.y, nv.y, k, &p0.y, &mu.y);
    o.z = reverse_one<STRIDED>(xv.z, ev.z, nv.z, k, &p0.z, &mu.z);
    o.w = reverse_one<STRIDED>(xv.w, ev.w, nv.w, k, &p0.w, &mu.w);
    *reinterpret_cast<float4 *>(a.x_prev + i) = o;
    if (a.pred_x0) *reinterpret_cast<float4 *>(a.pred_x0 + i) = p0;
    if (a.mean_out) *reinterpret_cast<float4 *>(a.mean_out + i) = mu;
}

template <bool STRIDED>
__device__ __forceinline__ void reverse_store1(const anoddpm_p_update_args &a, const StepCoef &k, int64_t i, float nz)
{
    float p0, mu;
    const float o = reverse_one<STRIDED>(a.x_t[i], a.eps[i], nz, k, &p0, &mu);
    a.x_prev[i] = o;
    if (a.pred_x0) a.pred_x0[i] = p0;
    if (a.mean_out) a.mean_out[i] = mu;
}

// The prologue of every update kernel: sample b's timestep normalised (`ti`; 0 where it was out of range, `bad`) and the step's
// coefficients.  STRIDED: they come from `sa` (thread 0 forms them in fp64, once per workgroup) instead of c_coef1 / c_coef2 /
// c_sigma.
template <bool STRIDED>
__device__ __forceinline__ StepCoef step_coef(const anoddpm_p_update_args &a, const StridedArgs &sa, int b, long long &ti, bool &bad)
{
    ti = a.t[b];
    const bool nonzero = (ti != 0);
    ti = ti < 0 ? ti + a.T : ti;
    bad = ti < 0 || ti >= a.T;                       // out of range: no out-of-bounds read, NaN result (see q_sample_kernel)
    ti = bad ? 0 : ti;
    StepCoef k;
    k.recip = bad ? __builtin_nanf("") : a.c_recip[ti];
    k.recipm1 = a.c_recipm1[ti];
    if constexpr (STRIDED) {
        __shared__ float coef[3];
        if (threadIdx.x == 0) strided_coef(sa, ti, bad, coef);
        __syncthreads();
        k.coef1 = coef[0];
        k.coef2 = coef[1];
        k.sigma = coef[2];
    } else {
        k.coef1 = a.c_coef1[ti];
        k.coef2 = a.c_coef2[ti];
        k.sigma = nonzero ? a.c_sigma[ti] : 0.0f;    // (t != 0).float() * exp(0.5*logvar)
    }
    return k;
}

// GAUSS: a.noise is NULL; the step noise comes from `key` at (stream of sample b, step = normalised t[b]).  It is generated at
// t == 0 too, where sigma is 0: mean + 0 * nz keeps the sign-of-zero behaviour of the unfused pair.
// STRIDED: the coefficients come from `sa` (step_coef); where sigma is 0 the noise is neither read nor generated.
template <int VEC, bool GAUSS, bool STRIDED>
__global__ __launch_bounds__(256) void p_update_kernel(anoddpm_p_update_args a, PhiloxKey key, StridedArgs sa)
{
    const int b = blockIdx.y;
    long long ti;
    bool bad;
    const StepCoef k = step_coef<STRIDED>(a, sa, b, ti, bad);
    const bool noisy = !STRIDED || k.sigma != 0.0f;
    const int64_t base = (int64_t)b * a.n;
    if (GAUSS) {
        const PhiloxSample ps = philox_sample(key, b, (uint32_t)ti);
        const int64_t nq = (a.n + 3) >> 2;
        for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (noisy) philox_normals(ps, (uint32_t)q, z);
            if (VEC == 4) {
                reverse_store4<STRIDED>(a, k, base + 4 * q, make_float4(z[0], z[1], z[2], z[3]));
            } else {
#pragma unroll
                for (int l = 0; l < 4; ++l)
                    if (4 * q + l < a.n) reverse_store1<STRIDED>(a, k, base + 4 * q + l, z[l]);
            }
        }
        return;
    }
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC; i < a.n; i += (int64_t)gridDim.x * 256 * VEC) {
        if (VEC == 4) {
            float4 nv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.noise && noisy) nv = *reinterpret_cast<const float4 *>(a.noise + base + i);
            reverse_store4<STRIDED>(a, k, base + i, nv);
        } else {
            reverse_store1<STRIDED>(a, k, base + i, a.noise && noisy ? a.noise[base + i] : 0.0f);
        }
    }
}

// ---------------------------------------------------------------- known-region conditioning
// RePaint (Lugmayr et al., CVPR 2022, Algorithm 1 / eq. 8) and the "stitch" of AutoDDPM (Bercea et al., 2023) on the reverse update
// of GaussianDiffusion.py:298-318: the pixels marked "keep" leave the step as the input image noised to the timestep s the step
// lands on (the q-sample of GaussianDiffusion.py:361-371), every other pixel as the ordinary update.  One sample's share of it:
struct KnownSample {
    const float *x0, *noise;     // this sample's planes; noise NULL: not read (s < 0, a poisoned sample, or generated)
    const uint8_t *keep;
    float qa, qc;                // ca[s], cb[s]
    bool exact, poison;          // s < 0: the kept pixels are x0 itself; poison: every element of the sample is NaN
};

// x_prev of one element: a select, so that a NaN in `u` under a kept pixel, or in `x0` / `kz` under any other, stays where it is
__device__ __forceinline__ float known_one(float u, float x0, float kz, bool kept, const KnownSample &ks)
{
    const float kn = ks.exact ? x0 : ks.qa * x0 + ks.qc * kz;
    return ks.poison ? __builtin_nanf("") : (kept ? kn : u);
}

// A sibling of p_update_kernel over the same prologue and reverse_one, one thread per quad in every form.  GAUSS: the step noise is
// generated as there (domain 0, step ti); the known-region noise is kr.noise, or with GAUSS and kr.noise NULL generated from the same
// key in domain 3 at step s.
template <int VEC, bool GAUSS, bool STRIDED>
__global__ __launch_bounds__(256) void p_update_known_kernel(anoddpm_p_update_args a, anoddpm_known_args kr, PhiloxKey key, StridedArgs sa)
{
    const int b = blockIdx.y;
    long long ti;
    bool bad;
    const StepCoef k = step_coef<STRIDED>(a, sa, b, ti, bad);
    const bool noisy = !STRIDED || k.sigma != 0.0f;
    long long stride = 1;
    if constexpr (STRIDED) stride = *sa.stride;
    KnownSample ks;
    ks.poison = bad || stride < 1;
    const long long s = ks.poison ? -1 : ti - stride;          // < a.T: never outside the tables
    const bool noised = s >= 0;
    ks.exact = !ks.poison && !noised;
    ks.qa = noised ? kr.ca[s] : 0.0f;
    ks.qc = noised ? kr.cb[s] : 0.0f;
    ks.x0 = kr.x0 + (int64_t)b * kr.x0_stride;
    ks.keep = kr.keep + (int64_t)b * kr.keep_stride;
    ks.noise = noised && kr.noise ? kr.noise + (int64_t)b * kr.noise_stride : nullptr;
    const bool kgen = GAUSS && noised && !kr.noise;
    PhiloxSample ps = {}, pk = {};
    if (GAUSS) {
        ps = philox_sample(key, b, (uint32_t)ti);
        pk = ps;
        pk.step = (uint32_t)(noised ? s : 0);
        pk.domain = 3u;                                          // known-region noise
    }
    const float *step_noise = !GAUSS && a.noise && noisy ? a.noise + (int64_t)b * a.n : nullptr;
    const int64_t base = (int64_t)b * a.n;
    const int64_t nq = (a.n + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        float z[4] = {0.f, 0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f};
        if (GAUSS && noisy) philox_normals(ps, (uint32_t)q, z);
        if (kgen) philox_normals(pk, (uint32_t)q, w);
        const int64_t j = 4 * q, i = base + j;
        if (VEC == 4) {
            if (step_noise) {
                const float4 nv = *reinterpret_cast<const float4 *>(step_noise + j);
                z[0] = nv.x, z[1] = nv.y, z[2] = nv.z, z[3] = nv.w;
            }
            if (ks.noise) {
                const float4 nv = *reinterpret_cast<const float4 *>(ks.noise + j);
                w[0] = nv.x, w[1] = nv.y, w[2] = nv.z, w[3] = nv.w;
            }
            const float4 xv = *reinterpret_cast<const float4 *>(a.x_t + i);
            const float4 ev = *reinterpret_cast<const float4 *>(a.eps + i);
            const float4 cv = *reinterpret_cast<const float4 *>(ks.x0 + j);
            const uint32_t kb = *reinterpret_cast<const uint32_t *>(ks.keep + j);
            float4 o, p0, mu;
            o.x = known_one(reverse_one<STRIDED>(xv.x, ev.x, z[0], k, &p0.x, &mu.x), cv.x, w[0], (kb & 0x000000ffu) != 0, ks);
            o.y = known_one(reverse_one<STRIDED>(xv.y, ev.y, z[1], k, &p0.y, &mu.y), cv.y, w[1], (kb & 0x0000ff00u) != 0, ks);
            o.z = known_one(reverse_one<STRIDED>(xv.z, ev.z, z[2], k, &p0.z, &mu.z), cv.z, w[2], (kb & 0x00ff0000u) != 0, ks);
            o.w = known_one(reverse_one<STRIDED>(xv.w, ev.w, z[3], k, &p0.w, &mu.w), cv.w, w[3], (kb & 0xff000000u) != 0, ks);
            *reinterpret_cast<float4 *>(a.x_prev + i) = o;
            if (a.pred_x0) *reinterpret_cast<float4 *>(a.pred_x0 + i) = p0;
            if (a.mean_out) *reinterpret_cast<float4 *>(a.mean_out + i) = mu;
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                if (j + l < a.n) {
                    float p0, mu;
                    const float nz = step_noise ? step_noise[j + l] : z[l];
                    const float u = reverse_one<STRIDED>(a.x_t[i + l], a.eps[i + l], nz, k, &p0, &mu);
                    a.x_prev[i + l] = known_one(u, ks.x0[j + l], ks.noise ? ks.noise[j + l] : w[l], ks.keep[j + l] != 0, ks);
                    if (a.pred_x0) a.pred_x0[i + l] = p0;
                    if (a.mean_out) a.mean_out[i + l] = mu;
                }
            }
        }
    }
}

// ---------------------------------------------------------------- resampling jumps
// The jump schedule of RePaint's sampler (Lugmayr et al., CVPR 2022, Algorithm 1) decided per sample on the device: an update that
// lands on level s jumps back up to s + J when s is a jump point of the chain (s >= 0, s % J == 0, s + J <= top) and the chain
// still has repetitions left.  The update kernel and the advance kernel evaluate THIS predicate from the same words.
__device__ __forceinline__ bool resample_jumps(long long s, long long J, long long R, long long top, long long rep)
{
    return J >= 1 && R >= 1 && s >= 0 && s % J == 0 && s + J <= top && rep > 0;
}

// A sibling of p_update_known_kernel (ancestral only): the conditioned image x_s of the step, and where the step jumps the
// re-noising q(x_land | x_s) = A x_s + C rz of EVERY pixel in the same pass.  Philox domains carry the visit index v of the sample:
// 8 v (step noise, step ti), 3 + 8 v (known-region noise, step s), 4 + 8 v (re-noise, step land).
template <int VEC, bool GAUSS>
__global__ __launch_bounds__(256) void p_update_resample_kernel(anoddpm_p_update_args a, anoddpm_known_args kr, anoddpm_resampling_args r,
                                                                PhiloxKey key)
{
    const int b = blockIdx.y;
    long long ti;
    bool bad;
    const StepCoef k = step_coef<false>(a, StridedArgs{}, b, ti, bad);
    const long long J = *r.jump, R = *r.reps;
    KnownSample ks;
    ks.poison = bad || J < 1 || R < 1;
    const long long s = ks.poison ? -1 : ti - 1;               // < a.T: never outside the tables
    bool jump = !ks.poison && resample_jumps(s, J, R, r.top[b], r.rep[b]);
    if (jump && s + J >= a.T) {                                 // a `top` beyond the schedule: poisoned, no table read
        ks.poison = true;
        jump = false;
    }
    const long long land = jump ? s + J : s;
    const uint32_t v8 = 8u * (uint32_t)r.visit[b];
    const bool noised = !ks.poison && s >= 0;
    ks.exact = !ks.poison && !noised;
    ks.qa = noised ? kr.ca[s] : 0.0f;
    ks.qc = noised ? kr.cb[s] : 0.0f;
    ks.x0 = kr.x0 + (int64_t)b * kr.x0_stride;
    ks.keep = kr.keep + (int64_t)b * kr.keep_stride;
    ks.noise = noised && kr.noise ? kr.noise + (int64_t)b * kr.noise_stride : nullptr;
    float A = 1.0f, C = 0.0f;
    if (jump) {                                                  // uniform over the workgroup: `jump` depends on b alone
        __shared__ float renoise[2];
        if (threadIdx.x == 0) {                                  // fp64, each rounded to fp32 once (as strided_coef)
            const double ratio = r.alphas_cumprod[land] / r.alphas_cumprod[s];
            renoise[0] = (float)sqrt(ratio);
            renoise[1] = (float)sqrt(1.0 - ratio);
        }
        __syncthreads();
        A = renoise[0], C = renoise[1];
    }
    const float *rnoise = jump && r.noise ? r.noise + (int64_t)b * r.noise_stride : nullptr;
    const bool kgen = GAUSS && noised && !kr.noise, rgen = GAUSS && jump && !r.noise;
    PhiloxSample ps = {}, pk = {}, pr = {};
    if (GAUSS) {
        ps = philox_sample(key, b, (uint32_t)ti);
        ps.domain = v8;                                          // step noise
        pk = ps;
        pk.step = (uint32_t)(noised ? s : 0);
        pk.domain = 3u + v8;                                     // known-region noise
        pr = ps;
        pr.step = (uint32_t)(jump ? land : 0);
        pr.domain = 4u + v8;                                     // re-noise
    }
    const float *step_noise = !GAUSS && a.noise ? a.noise + (int64_t)b * a.n : nullptr;
    const int64_t base = (int64_t)b * a.n;
    const int64_t nq = (a.n + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
        float z[4] = {0.f, 0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f}, y[4] = {0.f, 0.f, 0.f, 0.f};
        if (GAUSS) philox_normals(ps, (uint32_t)q, z);
        if (kgen) philox_normals(pk, (uint32_t)q, w);
        if (rgen) philox_normals(pr, (uint32_t)q, y);
        const int64_t j = 4 * q, i = base + j;
        if (VEC == 4) {
            if (step_noise) {
                const float4 nv = *reinterpret_cast<const float4 *>(step_noise + j);
                z[0] = nv.x, z[1] = nv.y, z[2] = nv.z, z[3] = nv.w;
            }
            if (ks.noise) {
                const float4 nv = *reinterpret_cast<const float4 *>(ks.noise + j);
                w[0] = nv.x, w[1] = nv.y, w[2] = nv.z, w[3] = nv.w;
            }
            if (rnoise) {
                const float4 nv = *reinterpret_cast<const float4 *>(rnoise + j);
                y[0] = nv.x, y[1] = nv.y, y[2] = nv.z, y[3] = nv.w;
            }
            const float4 xv = *reinterpret_cast<const float4 *>(a.x_t + i);
            const float4 ev = *reinterpret_cast<const float4 *>(a.eps + i);
            const float4 cv = *reinterpret_cast<const float4 *>(ks.x0 + j);
            const uint32_t kb = *reinterpret_cast<const uint32_t *>(ks.keep + j);
            float4 o, p0, mu;
            o.x = known_one(reverse_one<false>(xv.x, ev.x, z[0], k, &p0.x, &mu.x), cv.x, w[0], (kb & 0x000000ffu) != 0, ks);
            o.y = known_one(reverse_one<false>(xv.y, ev.y, z[1], k, &p0.y, &mu.y), cv.y, w[1], (kb & 0x0000ff00u) != 0, ks);
            o.z = known_one(reverse_one<false>(xv.z, ev.z, z[2], k, &p0.z, &mu.z), cv.z, w[2], (kb & 0x00ff0000u) != 0, ks);
            o.w = known_one(reverse_one<false>(xv.w, ev.w, z[3], k, &p0.w, &mu.w), cv.w, w[3], (kb & 0xff000000u) != 0, ks);
            if (jump) {
                o.x = A * o.x + C * y[0];
                o.y = A * o.y + C * y[1];
                o.z = A * o.z + C * y[2];
                o.w = A * o.w + C * y[3];
            }
            *reinterpret_cast<float4 *>(a.x_prev + i) = o;
            if (a.pred_x0) *reinterpret_cast<float4 *>(a.pred_x0 + i) = p0;
            if (a.mean_out) *reinterpret_cast<float4 *>(a.mean_out + i) = mu;
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                if (j + l < a.n) {
                    float p0, mu;
                    const float nz = step_noise ? step_noise[j + l] : z[l];
                    const float u = reverse_one<false>(a.x_t[i + l], a.eps[i + l], nz, k, &p0, &mu);
                    const float xs = known_one(u, ks.x0[j + l], ks.noise ? ks.noise[j + l] : w[l], ks.keep[j + l] != 0, ks);
                    a.x_prev[i + l] = jump ? A * xs + C * (rnoise ? rnoise[j + l] : y[l]) : xs;
                    if (a.pred_x0) a.pred_x0[i + l] = p0;
                    if (a.mean_out) a.mean_out[i + l] = mu;
                }
            }
        }
    }
}

// The only writer of a resampled chain's state: one thread per sample.  A landing that jumps goes back up to s + J with
// one repetition less and the next visit index; a landing on a multiple of J that does not jump refills the repetitions; everything
// else counts down, floored at 0 as chain_advance_strided floors it.
__global__ void chain_advance_resample_kernel(int64_t *t, int B, int32_t *step, const int32_t *jump, const int32_t *reps,
                                              const int32_t *top, int32_t *rep, int32_t *visit)
{
    const int i = threadIdx.x;
    if (i < B) {
        const long long J = *jump, R = *reps, s = (long long)t[i] - 1;
        if (resample_jumps(s, J, R, top[i], rep[i])) {
            t[i] = s + J;
            rep[i] -= 1;
            visit[i] += 1;
        } else {
            if (J >= 1 && R >= 1 && s >= 0 && s % J == 0) rep[i] = (int32_t)(R - 1);
            t[i] = s < 0 ? 0 : s;
        }
    }
    if (i == 0 && step) *step += 1;
}

__global__ void chain_advance_kernel(int64_t *t, int B, int32_t *step)
{
    const int i = threadIdx.x;
    if (i < B) t[i] -= 1;
    if (i == 0 && step) *step += 1;
}

__global__ void chain_advance_strided_kernel(int64_t *t, int B, int32_t *step, const int32_t *stride)
{
    const int i = threadIdx.x;
    if (i < B) {
        const long long next = (long long)t[i] - (long long)*stride;
        t[i] = next < 0 ? 0 : next;
    }
    if (i == 0 && step) *step += 1;
}


// ---------------------------------------------------------------- VLB terms (GaussianDiffusion.py:384-397, 445-478)
// One pass per reverse step of calc_total_vlb: per sample the KL( q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t) ) or, at t = 0, the
// discretised decoder NLL, in bits per dimension; plus mean((pred_x_0 - x_0)^2) and mean((eps' - noise)^2).
// Replaces ~45 ATen dispatches per step.  fp32 element math in the reference's operation order; the per-sample
// means are fp64 partial sums folded in a fixed order.
constexpr int VLB_BLOCKS = 64;

// torch.clamp(x, -1, 1): a NaN stays a NaN (fminf / fmaxf return the other operand, which would turn the NaN of an out-of-range
// t, or of a NaN model output, into -1 and a finite term).
__device__ __forceinline__ float clamp_unit(float x) { return x != x ? x : fminf(fmaxf(x, -1.0f), 1.0f); }

__device__ __forceinline__ float approx_cdf(float x)
{
    // 0.5 * (1 + tanh(sqrt(2/pi) * (x + 0.044715 * x^3)))          GaussianDiffusion.py:56-61
    const float c = 0.7978845608028654f;
    return 0.5f * (1.0f + tanhf(c * (x + 0.044715f * (x * x * x))));
}

__global__ __launch_bounds__(256) void vlb_kernel(anoddpm_vlb_args a, double *__restrict__ partial)
{
    const int b = blockIdx.y;
    long long ti = a.t[b];
    const bool t0 = (ti == 0);
    ti = ti < 0 ? ti + a.T : ti;
    const bool bad = ti < 0 || ti >= a.T;            // out of range: no out-of-bounds read, NaN result (see q_sample_kernel)
    ti = bad ? 0 : ti;
    const float recip = bad ? __builtin_nanf("") : a.c_recip[ti], recipm1 = a.c_recipm1[ti], coef1 = a.c_coef1[ti], coef2 = a.c_coef2[ti];
    const float lv1 = a.c_post_logvar[ti], lv2 = a.c_model_logvar[ti];
    const float kbase = (-1.0f + lv2) - lv1;                    // -1 + logvar2 - logvar1
    const float e1 = expf(lv1 - lv2), e2 = expf(-lv2);
    const float inv_std = expf(-(0.5f * lv2));
    const int64_t base = (int64_t)b * a.n;
    double s_vlb = 0.0, s_x0 = 0.0, s_eps = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const float xt = a.xt[base + i], x0 = a.x0[base + i], e = a.eps[base + i];
        float pred = recip * xt - recipm1 * e;                   // :228-230
        pred = clamp_unit(pred);                                 // :287
        const float mean = coef1 * pred + coef2 * xt;            // :253-267 (model mean)
        const float tmean = coef1 * x0 + coef2 * xt;             // true posterior mean
        float term;
        if (!t0) {
            const float d = tmean - mean;
            term = 0.5f * ((kbase + e1) + (d * d) * e2);         // normal_kl, :43-53
        } else {
            const float cen = x0 - mean;                         // discretised_gaussian_log_likelihood, :64-93
            const float cp = approx_cdf(inv_std * (cen + 1.0f / 255.0f));
            const float cm = approx_cdf(inv_std * (cen - 1.0f / 255.0f));
            const float lcp = logf(fmaxf(cp, 1e-12f));
            const float l1m = logf(fmaxf(1.0f - cm, 1e-12f));
            const float ld = logf(fmaxf(cp - cm, 1e-12f));
            term = -(x0 < -0.999f ? lcp : (x0 > 0.999f ? l1m : ld));
        }
        s_vlb += (double)term;
        const float dx = pred - x0;
        s_x0 += (double)(dx * dx);
        if (a.noise) {
            const float er = (recip * xt - pred) / recipm1;      // predict_eps_from_x_0, :232-235
            const float de = er - a.noise[base + i];
            s_eps += (double)(de * de);
        }
        if (a.pred_x0) a.pred_x0[base + i] = pred;
    }
    __shared__ double red[4][3];
    double v[3] = {s_vlb, s_x0, s_eps};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        partial[((int64_t)b * gridDim.x + blockIdx.x) * 3 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

__global__ void vlb_fold_kernel(const double *__restrict__ partial, float *__restrict__ out, int nblocks, int B, double n)
{
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= 3) return;
    double v = 0.0;
    for (int j = 0; j < nblocks; ++j) v += partial[((int64_t)b * nblocks + j) * 3 + k];
    v /= n;
    if (k == 0) v /= 0.6931471805599453;                        // / np.log(2.0): bits per dimension
    out[(int64_t)k * B + b] = (float)v;
}

// ---------------------------------------------------------------- training loss (GaussianDiffusion.py:399-434) + its gradient
// calc_loss's per-sample terms and p_loss's weighted mean in one pass over [B][n] (+ a tiny fold), and d(total)/d(eps) in one
// more: replaces the ~15 ATen elementwise / reduction dispatches of the loss expression and the ~25 of its autograd backward
// (the "hybrid" loss's VLB term alone is ~45 forward dispatches).  Element math in fp32, sums in fp64 with a fixed order.
constexpr int LOSS_BLOCKS = 64;

struct VlbCoef {
    float recip, recipm1, coef1, coef2, kbase, e1, e2, inv_std;
    bool t0;
};

__device__ __forceinline__ VlbCoef vlb_coef(const anoddpm_loss_args &a, int b)
{
    VlbCoef k;
    long long ti = a.t[b];
    k.t0 = (ti == 0);
    ti = ti < 0 ? ti + a.T : ti;
    const bool bad = ti < 0 || ti >= a.T;
    ti = bad ? 0 : ti;
    k.recip = bad ? __builtin_nanf("") : a.c_recip[ti];
    k.recipm1 = a.c_recipm1[ti];
    k.coef1 = a.c_coef1[ti];
    k.coef2 = a.c_coef2[ti];
    const float lv1 = a.c_post_logvar[ti], lv2 = a.c_model_logvar[ti];
    k.kbase = (-1.0f + lv2) - lv1;
    k.e1 = expf(lv1 - lv2);
    k.e2 = expf(-lv2);
    k.inv_std = expf(-(0.5f * lv2));
    return k;
}

// d/dx of approx_cdf: 0.5 * (1 - tanh(u)^2) * c * (1 + 3 * 0.044715 x^2),  u = c * (x + 0.044715 x^3)
__device__ __forceinline__ float approx_cdf_grad(float x)
{
    const float c = 0.7978845608028654f;
    const float th = tanhf(c * (x + 0.044715f * (x * x * x)));
    return 0.5f * (1.0f - th * th) * (c * (1.0f + 3.0f * 0.044715f * (x * x)));
}

// One element of the VLB term (calc_vlb_xt, :384-397): returns the term (nats, before mean_flat and / ln 2); *dterm_deps
// receives its derivative with respect to the model output eps (through mean = coef1 * clamp(recip x_t - recipm1 eps) + coef2 x_t;
// torch.clamp passes the gradient on [-1, 1] inclusive, clamp(min=1e-12) on [1e-12, inf)).
__device__ __forceinline__ float vlb_element(const VlbCoef &k, float x0, float xt, float e, float *dterm_deps)
{
    const float raw = k.recip * xt - k.recipm1 * e;
    const float pred = clamp_unit(raw);
    const float dpred = (raw >= -1.0f && raw <= 1.0f) ? -k.recipm1 : 0.0f;
    const float mean = k.coef1 * pred + k.coef2 * xt;
    float term, dmean;
    if (!k.t0) {
        const float tmean = k.coef1 * x0 + k.coef2 * xt;
        const float d = tmean - mean;
        term = 0.5f * ((k.kbase + k.e1) + (d * d) * k.e2);
        dmean = -(d * k.e2);
    } else {
        const float cen = x0 - mean;
        const float zp = k.inv_std * (cen + 1.0f / 255.0f), zm = k.inv_std * (cen - 1.0f / 255.0f);
        const float cp = approx_cdf(zp), cm = approx_cdf(zm);
        float lp, dcen;                              // log-probability and its derivative w.r.t. cen
        if (x0 < -0.999f) {
            lp = logf(fmaxf(cp, 1e-12f));
            dcen = cp >= 1e-12f ? approx_cdf_grad(zp) * k.inv_std / cp : 0.0f;
        } else if (x0 > 0.999f) {
            const float om = 1.0f - cm;
            lp = logf(fmaxf(om, 1e-12f));
            dcen = om >= 1e-12f ? -(approx_cdf_grad(zm) * k.inv_std) / om : 0.0f;
        } else {
            const float dl = cp - cm;
            lp = logf(fmaxf(dl, 1e-12f));
            dcen = dl >= 1e-12f ? (approx_cdf_grad(zp) - approx_cdf_grad(zm)) * k.inv_std / dl : 0.0f;
        }
        term = -lp;
        dmean = dcen;                                // term = -lp(cen), cen = x0 - mean  ->  d term / d mean = + d lp / d cen
    }
    *dterm_deps = dmean * k.coef1 * dpred;
    return term;
}

__global__ __launch_bounds__(256) void loss_fwd_kernel(anoddpm_loss_args a)
{
    const int b = blockIdx.y;
    const bool hybrid = a.kind == 2;
    VlbCoef k = {};
    if (hybrid) k = vlb_coef(a, b);
    const int64_t base = (int64_t)b * a.n;
    double s_main = 0.0, s_vlb = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const float e = a.eps[base + i];
        const float d = e - a.noise[base + i];
        s_main += (double)(a.kind == 0 ? fabsf(d) : d * d);
        if (hybrid) {
            float unused;
            s_vlb += (double)vlb_element(k, a.x0[base + i], a.xt[base + i], e, &unused);
        }
    }
    __shared__ double red[4][2];
    double v[2] = {s_main, s_vlb};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        for (int off = 32; off > 0; off >>= 1) v[j] += __shfl_xor(v[j], off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int j = threadIdx.x;
        a.workspace[((int64_t)b * gridDim.x + blockIdx.x) * 2 + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    }
}

// one block: per-sample values (thread b, b + 256, ...) then the weighted mean over the batch in index order
__global__ __launch_bounds__(256) void loss_fold_kernel(anoddpm_loss_args a, int nblocks)
{
    __shared__ double acc[256];
    double mine = 0.0;
    for (int b = threadIdx.x; b < a.B; b += 256) {
        double m = 0.0, v = 0.0;
        for (int j = 0; j < nblocks; ++j) {
            m += a.workspace[((int64_t)b * nblocks + j) * 2 + 0];
            v += a.workspace[((int64_t)b * nblocks + j) * 2 + 1];
        }
        const float main_f = (float)(m / (double)a.n);
        float per = main_f;
        if (a.kind == 2) {
            const float vlb_f = (float)(v / (double)a.n / 0.6931471805599453);
            if (a.vlb) a.vlb[b] = vlb_f;
            per = vlb_f + main_f;                    // loss["vlb"] + mean_flat(mse), :414
        }
        a.per_sample[b] = per;
        mine += (double)(a.weights ? per * a.weights[b] : per);
    }
    acc[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        const int nt = a.B < 256 ? a.B : 256;
        for (int i = 0; i < nt; ++i) s += acc[i];
        if (a.total) a.total[0] = (float)(s / (double)a.B);
    }
}

// d_eps[b][i] = c_b * d(main term)/d(eps) / n + v_b * d(vlb term)/d(eps) / (n ln 2) with
//   c_b = g_per[b] + g_total * w_b / B     (loss["loss"][b] and the weighted batch mean both contain sample b's terms)
//   v_b = (hybrid: c_b) + g_vlb[b]
__global__ __launch_bounds__(256) void loss_bwd_kernel(anoddpm_loss_args a)
{
    const int b = blockIdx.y;
    const bool hybrid = a.kind == 2;
    float cb = a.g_per ? a.g_per[b] : 0.0f;
    if (a.g_total) cb += a.g_total[0] * (a.weights ? a.weights[b] : 1.0f) / (float)a.B;
    float vb = hybrid ? cb : 0.0f;
    if (hybrid && a.g_vlb) vb += a.g_vlb[b];
    const float inv_n = 1.0f / (float)a.n;
    const float cm = cb * inv_n, cv = vb * inv_n / 0.6931471805599453f;
    VlbCoef k = {};
    if (hybrid) k = vlb_coef(a, b);
    const int64_t base = (int64_t)b * a.n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * 256) {
        const float e = a.eps[base + i];
        const float d = e - a.noise[base + i];
        float g = a.kind == 0 ? cm * (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f)) : cm * (2.0f * d);
        if (hybrid) {
            float dv;
            (void)vlb_element(k, a.x0[base + i], a.xt[base + i], e, &dv);
            g += cv * dv;
        }
        a.d_eps[base + i] = g;
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// grid.x of the elementwise launches: one thread per unit of work, at most 4096 blocks (grid-stride beyond)
inline unsigned grid_x(int64_t work) { return (unsigned)((work + 255) / 256 > 4096 ? 4096 : (work + 255) / 256); }

static int philox_key_check(const uint64_t *seed, int64_t n, const char *who)
{
    ANODDPM_REQUIRE(seed, "%s: null seed pointer", who);
    ANODDPM_REQUIRE(n <= ((int64_t)1 << 34), "%s: more than 2^34 elements per sample (the quad counter is 32 bits)", who);
    return ANODDPM_OK;
}

extern "C" int anoddpm_philox_bits_host(uint64_t seed, uint32_t stream, uint32_t step, uint32_t domain, uint32_t quad0,
                                        int64_t nquads, uint32_t *out)
{
    ANODDPM_REQUIRE(nquads >= 0 && (nquads == 0 || out), "philox_bits_host: bad arguments");
    for (int64_t j = 0; j < nquads; ++j) {
        const PhiloxWords p = philox4x32_10(quad0 + (uint32_t)j, stream, step, domain, (uint32_t)seed, (uint32_t)(seed >> 32));
        for (int l = 0; l < 4; ++l) out[4 * j + l] = p.w[l];
    }
    return ANODDPM_OK;
}

extern "C" int anoddpm_philox_fill(void *out, int32_t kind, int32_t B, int64_t n, const uint64_t *seed, const int32_t *streams,
                                   uint32_t stream0, uint32_t domain, const int64_t *t, uint32_t step0, int32_t T, void *stream)
{
    ANODDPM_REQUIRE(B >= 0 && n >= 0 && T >= 0 && (kind == 0 || kind == 1), "philox_fill: bad sizes / kind");
    if (B == 0 || n == 0) return ANODDPM_OK;
    ANODDPM_REQUIRE(out, "philox_fill: null pointer");
    ANODDPM_REQUIRE(B <= 65535, "philox_fill: B > 65535");
    if (const int rc = philox_key_check(seed, n, "philox_fill")) return rc;
    const PhiloxKey key = {seed, streams, stream0, domain};
    const unsigned gx = grid_x((n + 3) / 4);
    uint32_t *o = static_cast<uint32_t *>(out);
    if ((n % 4 == 0) && aligned16(out))
        hipLaunchKernelGGL(philox_fill_kernel<4>, dim3(gx, B), dim3(256), 0, anoddpm::as_stream(stream), o, kind, n, key, t, step0, T);
    else
        hipLaunchKernelGGL(philox_fill_kernel<1>, dim3(gx, B), dim3(256), 0, anoddpm::as_stream(stream), o, kind, n, key, t, step0, T);
    return anoddpm::check_launch("philox_fill");
}

extern "C" int anoddpm_q_sample(float *out, const float *x, const float *noise, const int64_t *t,
                                const float *ca, const float *cb, int32_t B, int64_t n, int32_t T, void *stream)
{
    ANODDPM_REQUIRE(B >= 0 && n >= 0 && T > 0, "q_sample: bad sizes");
    if (B == 0 || n == 0) return ANODDPM_OK;            // empty batch: nothing to do (pointers may be null)
    ANODDPM_REQUIRE(out && x && noise && t && ca && cb, "q_sample: null pointer");
    ANODDPM_REQUIRE(B <= 65535, "q_sample: B > 65535");
    const bool v4 = (n % 4 == 0) && aligned16(out) && aligned16(x) && aligned16(noise);
    const unsigned gx = grid_x(v4 ? n / 4 : n);
    const PhiloxKey none = {};
    if (v4)
        hipLaunchKernelGGL((q_sample_kernel<4, false>), dim3(gx, B), dim3(256), 0, anoddpm::as_stream(stream), out, x, noise, t, ca, cb, n, T, (float *)nullptr, none);
    else
        hipLaunchKernelGGL((q_sample_kernel<1, false>), dim3(gx, B), dim3(256), 0, anoddpm::as_stream(stream), out, x, noise, t, ca, cb, n, T, (float *)nullptr, none);
    return anoddpm::check_launch("q_sample");
}

extern "C" int anoddpm_q_sample_gauss(float *out, float *noise_out, const float *x, const int64_t *t, const float *ca,
                                      const float *cb, int32_t B, int64_t n, int32_t T, const uint64_t *seed,
                                      const int32_t *streams, uint32_t stream0, void *stream)
{
    ANODDPM_REQUIRE(B >= 0 && n >= 0 && T > 0, "q_sample_gauss: bad sizes");
    if (B == 0 || n == 0) return ANODDPM_OK;
    ANODDPM_REQUIRE(out && x && t && ca && cb, "q_sample_gauss: null pointer");
    ANODDPM_REQUIRE(B <= 65535, "q_sample_gauss: B > 65535");
    if (const int rc = philox_key_check(seed, n, "q_sample_gauss")) return rc;
    const PhiloxKey key = {seed, streams, stream0, 1u};       // domain 1: forward / training noise
    const bool v4 = (n % 4 == 0) && aligned16(out) && aligned16(x) && (!noise_out || aligned16(noise_out));
    const unsigned gx = grid_x((n + 3) / 4);
    if (v4)
        hipLaunchKernelGGL((q_sample_kernel<4, true>), dim3(gx, B), dim3(256), 0, anoddpm::as_stream(stream), out, x, (const float *)nullptr, t, ca, cb, n, T, noise_out, key);
    else
        hipLaunchKernelGGL((q_sample_kernel<1, true>), dim3(gx, B), dim3(256), 0, anoddpm::as_stream(stream), out, x, (const float *)nullptr, t, ca, cb, n, T, noise_out, key);
    return anoddpm::check_launch("q_sample_gauss");
}

template <bool GAUSS, bool STRIDED>
static void p_update_dispatch(bool v4, unsigned gx, const anoddpm_p_update_args &a, const PhiloxKey &key, const StridedArgs &sa,
                              void *stream)
{
    if (v4)
        hipLaunchKernelGGL((p_update_kernel<4, GAUSS, STRIDED>), dim3(gx, a.B), dim3(256), 0, anoddpm::as_stream(stream), a, key, sa);
    else
        hipLaunchKernelGGL((p_update_kernel<1, GAUSS, STRIDED>), dim3(gx, a.B), dim3(256), 0, anoddpm::as_stream(stream), a, key, sa);
}

// The argument checks every update launch shares.  -> EINVAL, 1 for an empty batch (nothing to launch), else 0.
static int p_update_check(const anoddpm_p_update_args *a, const PhiloxKey *key, const StridedArgs *sa, const char *who)
{
    ANODDPM_REQUIRE(a, "%s: null argument struct", who);
    ANODDPM_REQUIRE(a->B >= 0 && a->n >= 0 && a->T > 0, "%s: bad sizes", who);
    if (a->B == 0 || a->n == 0) return 1;
    ANODDPM_REQUIRE(a->x_prev && a->x_t && a->eps && a->t, "%s: null pointer", who);
    ANODDPM_REQUIRE(a->c_recip && a->c_recipm1, "%s: null table", who);
    if (sa)
        ANODDPM_REQUIRE(sa->acp && sa->stride && sa->eta, "%s: null alphas_cumprod / stride / eta", who);
    else
        ANODDPM_REQUIRE(a->c_coef1 && a->c_coef2 && a->c_sigma, "%s: null table", who);
    ANODDPM_REQUIRE(a->B <= 65535, "%s: B > 65535", who);
    if (key) {
        if (const int rc = philox_key_check(key->seed, a->n, who)) return rc;
        ANODDPM_REQUIRE(!a->noise, "%s: a noise tensor was given as well", who);
    }
    return 0;
}

static bool p_update_v4(const anoddpm_p_update_args *a)
{
    return (a->n % 4 == 0) && aligned16(a->x_prev) && aligned16(a->x_t) && aligned16(a->eps) &&
           (!a->noise || aligned16(a->noise)) && (!a->pred_x0 || aligned16(a->pred_x0)) && (!a->mean_out || aligned16(a->mean_out));
}

// key == nullptr: the noise tensor a->noise (or none); else the step noise is generated in the kernel.  sa == nullptr: the
// ancestral update from the c_coef1 / c_coef2 / c_sigma tables; else the strided sampler's, which ignores those three.
static int p_update_launch(const anoddpm_p_update_args *a, const PhiloxKey *key, const StridedArgs *sa, void *stream, const char *who)
{
    if (const int rc = p_update_check(a, key, sa, who)) return rc < 0 ? rc : ANODDPM_OK;
    const bool v4 = p_update_v4(a);
    const StridedArgs no_stride = {};
    if (key) {
        const unsigned gx = grid_x((a->n + 3) / 4);
        if (sa)
            p_update_dispatch<true, true>(v4, gx, *a, *key, *sa, stream);
        else
            p_update_dispatch<true, false>(v4, gx, *a, *key, no_stride, stream);
        return anoddpm::check_launch(who);
    }
    const unsigned gx = grid_x(v4 ? a->n / 4 : a->n);
    const PhiloxKey none = {};
    if (sa)
        p_update_dispatch<false, true>(v4, gx, *a, none, *sa, stream);
    else
        p_update_dispatch<false, false>(v4, gx, *a, none, no_stride, stream);
    return anoddpm::check_launch(who);
}

extern "C" int anoddpm_p_sample_update(const anoddpm_p_update_args *a, void *stream)
{
    return p_update_launch(a, nullptr, nullptr, stream, "p_sample_update");
}

extern "C" int anoddpm_p_sample_update_gauss(const anoddpm_p_update_args *a, const uint64_t *seed, const int32_t *streams,
                                             uint32_t stream0, void *stream)
{
    const PhiloxKey key = {seed, streams, stream0, 0u};       // domain 0: reverse-step noise
    return p_update_launch(a, &key, nullptr, stream, "p_sample_update_gauss");
}

extern "C" int anoddpm_strided_update(const anoddpm_p_update_args *a, const double *alphas_cumprod, const int32_t *stride,
                                      const float *eta, const uint64_t *seed, const int32_t *streams, uint32_t stream0, void *stream)
{
    const StridedArgs sa = {alphas_cumprod, stride, eta};
    if (!seed) return p_update_launch(a, nullptr, &sa, stream, "strided_update");
    const PhiloxKey key = {seed, streams, stream0, 0u};       // domain 0, as the ancestral update: the keying is the same
    return p_update_launch(a, &key, &sa, stream, "strided_update");
}

template <bool GAUSS, bool STRIDED>
static void p_update_known_dispatch(bool v4, unsigned gx, const anoddpm_p_update_args &a, const anoddpm_known_args &k,
                                    const PhiloxKey &key, const StridedArgs &sa, void *stream)
{
    if (v4)
        hipLaunchKernelGGL((p_update_known_kernel<4, GAUSS, STRIDED>), dim3(gx, a.B), dim3(256), 0, anoddpm::as_stream(stream), a, k, key, sa);
    else
        hipLaunchKernelGGL((p_update_known_kernel<1, GAUSS, STRIDED>), dim3(gx, a.B), dim3(256), 0, anoddpm::as_stream(stream), a, k, key, sa);
}

extern "C" int anoddpm_p_sample_update_known(const anoddpm_p_update_args *a, const anoddpm_known_args *k, const double *alphas_cumprod,
                                             const int32_t *stride, const float *eta, const uint64_t *seed, const int32_t *streams,
                                             uint32_t stream0, void *stream)
{
    const char *who = "p_sample_update_known";
    ANODDPM_REQUIRE(k, "%s: null known-region struct", who);
    const bool strided = alphas_cumprod || stride || eta;
    ANODDPM_REQUIRE(!strided || (alphas_cumprod && stride && eta), "%s: alphas_cumprod, stride and eta are all set or all NULL", who);
    ANODDPM_REQUIRE(seed || k->noise, "%s: no known-region noise tensor and no seed to generate it from", who);
    const StridedArgs sa = {alphas_cumprod, stride, eta};
    const PhiloxKey key = {seed, streams, stream0, 0u};       // domain 0 for the step noise; the kernel takes domain 3 for the known region's
    const int rc = p_update_check(a, seed ? &key : nullptr, strided ? &sa : nullptr, who);
    if (rc < 0) return rc;
    ANODDPM_REQUIRE(k->x0 && k->keep && k->ca && k->cb, "%s: null x0 / keep / ca / cb", who);
    for (const int64_t w : {k->x0_stride, k->keep_stride, k->noise_stride})
        ANODDPM_REQUIRE(w == 0 || w == a->n, "%s: a sample stride of %lld is neither 0 nor n", who, (long long)w);
    if (rc) return ANODDPM_OK;
    const bool v4 = p_update_v4(a) && aligned16(k->x0) && (!k->noise || aligned16(k->noise)) && ((uintptr_t)k->keep & 3) == 0;
    const unsigned gx = grid_x((a->n + 3) / 4);
    if (seed)
        strided ? p_update_known_dispatch<true, true>(v4, gx, *a, *k, key, sa, stream)
                : p_update_known_dispatch<true, false>(v4, gx, *a, *k, key, sa, stream);
    else
        strided ? p_update_known_dispatch<false, true>(v4, gx, *a, *k, key, sa, stream)
                : p_update_known_dispatch<false, false>(v4, gx, *a, *k, key, sa, stream);
    return anoddpm::check_launch(who);
}

extern "C" int anoddpm_p_sample_update_resample(const anoddpm_p_update_args *a, const anoddpm_known_args *k,
                                                const anoddpm_resampling_args *r, const uint64_t *seed, const int32_t *streams,
                                                uint32_t stream0, void *stream)
{
    const char *who = "p_sample_update_resample";
    ANODDPM_REQUIRE(k, "%s: null known-region struct", who);
    ANODDPM_REQUIRE(r, "%s: null resampling struct", who);
    ANODDPM_REQUIRE(seed || k->noise, "%s: no known-region noise tensor and no seed to generate it from", who);
    ANODDPM_REQUIRE(seed || r->noise, "%s: no re-noise tensor and no seed to generate it from", who);
    const PhiloxKey key = {seed, streams, stream0, 0u};       // the kernel forms the three domains from the visit index
    const int rc = p_update_check(a, seed ? &key : nullptr, nullptr, who);
    if (rc < 0) return rc;
    ANODDPM_REQUIRE(k->x0 && k->keep && k->ca && k->cb, "%s: null x0 / keep / ca / cb", who);
    ANODDPM_REQUIRE(r->jump && r->reps && r->top && r->rep && r->visit && r->alphas_cumprod,
                    "%s: null jump / reps / top / rep / visit / alphas_cumprod", who);
    for (const int64_t w : {k->x0_stride, k->keep_stride, k->noise_stride, r->noise_stride})
        ANODDPM_REQUIRE(w == 0 || w == a->n, "%s: a sample stride of %lld is neither 0 nor n", who, (long long)w);
    if (rc) return ANODDPM_OK;
    const bool v4 = p_update_v4(a) && aligned16(k->x0) && (!k->noise || aligned16(k->noise)) && ((uintptr_t)k->keep & 3) == 0 &&
                    (!r->noise || aligned16(r->noise));
    const dim3 grid(grid_x((a->n + 3) / 4), a->B);
    if (seed && v4)
        hipLaunchKernelGGL((p_update_resample_kernel<4, true>), grid, dim3(256), 0, anoddpm::as_stream(stream), *a, *k, *r, key);
    else if (seed)
        hipLaunchKernelGGL((p_update_resample_kernel<1, true>), grid, dim3(256), 0, anoddpm::as_stream(stream), *a, *k, *r, key);
    else if (v4)
        hipLaunchKernelGGL((p_update_resample_kernel<4, false>), grid, dim3(256), 0, anoddpm::as_stream(stream), *a, *k, *r, key);
    else
        hipLaunchKernelGGL((p_update_resample_kernel<1, false>), grid, dim3(256), 0, anoddpm::as_stream(stream), *a, *k, *r, key);
    return anoddpm::check_launch(who);
}

extern "C" int anoddpm_chain_advance_resample(int64_t *t, int32_t B, int32_t *step, const int32_t *jump, const int32_t *reps,
                                              const int32_t *top, int32_t *rep, int32_t *visit, void *stream)
{
    ANODDPM_REQUIRE(t && jump && reps && top && rep && visit && B >= 0 && B <= 1024, "chain_advance_resample: bad arguments");
    hipLaunchKernelGGL(chain_advance_resample_kernel, dim3(1), dim3(B < 64 ? 64 : ((B + 63) / 64) * 64), 0,
                       anoddpm::as_stream(stream), t, (int)B, step, jump, reps, top, rep, visit);
    return anoddpm::check_launch("chain_advance_resample");
}

extern "C" int anoddpm_chain_advance(int64_t *t, int32_t B, int32_t *step, void *stream)
{
    ANODDPM_REQUIRE(t && B >= 0 && B <= 1024, "chain_advance: bad arguments");
    hipLaunchKernelGGL(chain_advance_kernel, dim3(1), dim3(B < 64 ? 64 : ((B + 63) / 64) * 64), 0,
                       anoddpm::as_stream(stream), t, B, step);
    return anoddpm::check_launch("chain_advance");
}

extern "C" int anoddpm_chain_advance_strided(int64_t *t, int32_t B, int32_t *step, const int32_t *stride, void *stream)
{
    ANODDPM_REQUIRE(t && stride && B >= 0 && B <= 1024, "chain_advance_strided: bad arguments");
    hipLaunchKernelGGL(chain_advance_strided_kernel, dim3(1), dim3(B < 64 ? 64 : ((B + 63) / 64) * 64), 0,
                       anoddpm::as_stream(stream), t, B, step, stride);
    return anoddpm::check_launch("chain_advance_strided");
}

extern "C" int anoddpm_vlb_terms(const anoddpm_vlb_args *a, void *stream)
{
    ANODDPM_REQUIRE(a, "vlb_terms: null argument struct");
    ANODDPM_REQUIRE(a->B >= 0 && a->n >= 0 && a->T > 0, "vlb_terms: bad sizes");
    if (a->B == 0 || a->n == 0) return ANODDPM_OK;
    ANODDPM_REQUIRE(a->x0 && a->xt && a->eps && a->t && a->out && a->workspace, "vlb_terms: null pointer");
    ANODDPM_REQUIRE(a->c_recip && a->c_recipm1 && a->c_coef1 && a->c_coef2 && a->c_post_logvar && a->c_model_logvar, "vlb_terms: null table");
    ANODDPM_REQUIRE(a->B <= 65535, "vlb_terms: B > 65535");
    ANODDPM_REQUIRE(a->workspace_doubles >= (int64_t)a->B * VLB_BLOCKS * 3, "vlb_terms: workspace too small");
    hipStream_t s = anoddpm::as_stream(stream);
    hipLaunchKernelGGL(vlb_kernel, dim3(VLB_BLOCKS, a->B), dim3(256), 0, s, *a, a->workspace);
    hipLaunchKernelGGL(vlb_fold_kernel, dim3(a->B), dim3(64), 0, s, a->workspace, a->out, VLB_BLOCKS, a->B, (double)a->n);
    return anoddpm::check_launch("vlb_terms");
}

static int loss_check(const anoddpm_loss_args *a, const char *who)
{
    ANODDPM_REQUIRE(a, "%s: null argument struct", who);
    ANODDPM_REQUIRE(a->B >= 0 && a->n >= 0 && a->kind >= 0 && a->kind <= 2, "%s: bad sizes / kind", who);
    if (a->B == 0 || a->n == 0) return 1;
    ANODDPM_REQUIRE(a->eps && a->noise, "%s: null eps / noise", who);
    ANODDPM_REQUIRE(a->B <= 65535, "%s: B > 65535", who);
    if (a->kind == 2) {
        ANODDPM_REQUIRE(a->x0 && a->xt && a->t && a->T > 0, "%s: the hybrid loss needs x0, xt, t", who);
        ANODDPM_REQUIRE(a->c_recip && a->c_recipm1 && a->c_coef1 && a->c_coef2 && a->c_post_logvar && a->c_model_logvar, "%s: null table", who);
    }
    return 0;
}

extern "C" int anoddpm_loss_forward(const anoddpm_loss_args *a, void *stream)
{
    const int rc = loss_check(a, "loss_forward");
    if (rc) return rc < 0 ? rc : ANODDPM_OK;
    ANODDPM_REQUIRE(a->per_sample && a->workspace, "loss_forward: null output / workspace");
    ANODDPM_REQUIRE(a->workspace_doubles >= (int64_t)a->B * LOSS_BLOCKS * 2, "loss_forward: workspace too small");
    hipStream_t s = anoddpm::as_stream(stream);
    hipLaunchKernelGGL(loss_fwd_kernel, dim3(LOSS_BLOCKS, a->B), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(loss_fold_kernel, dim3(1), dim3(256), 0, s, *a, LOSS_BLOCKS);
    return anoddpm::check_launch("loss_forward");
}

extern "C" int anoddpm_loss_backward(const anoddpm_loss_args *a, void *stream)
{
    const int rc = loss_check(a, "loss_backward");
    if (rc) return rc < 0 ? rc : ANODDPM_OK;
    ANODDPM_REQUIRE(a->d_eps, "loss_backward: null d_eps");
    const int64_t want = (a->n + 255) / 256;
    const unsigned gx = (unsigned)(want > 1024 ? 1024 : want);
    hipLaunchKernelGGL(loss_bwd_kernel, dim3(gx, a->B), dim3(256), 0, anoddpm::as_stream(stream), *a);
    return anoddpm::check_launch("loss_backward");
}
