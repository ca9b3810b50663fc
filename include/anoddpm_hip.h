/*
 * anoddpm_hip.h -- C ABI of libanoddpm_hip.so, the MI355X (gfx950) implementation of the
 * AnoDDPM hot path.  Plain pointers and sizes only: no torch / C++ types cross this boundary.
 *
 * The upstream reference (Julian-Wyatt/AnoDDPM) is pure Python and has no FFI of its own; the
 * drop-in boundary its callers see is the Python module surface (GaussianDiffusion / UNet /
 * simplex).  This header is the layer directly below that surface: each entry point replaces
 * the reference code cited next to it.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every function returns ANODDPM_OK (0) or a negative ANODDPM_E* code; nothing throws,
 *     nothing allocates device memory, nothing synchronises (safe under hipGraph capture)
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream)
 *   - device pointers are marked [dev]; host pointers [host]
 *   - activations are NHWC fp32 ("pixels x channels"); an image is H*W pixels
 */
#ifndef ANODDPM_HIP_H
#define ANODDPM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANODDPM_OK 0
#define ANODDPM_EINVAL (-1)   /* bad argument (shape/alignment/range)          */
#define ANODDPM_ELAUNCH (-2)  /* HIP reported a launch / runtime error          */
#define ANODDPM_ENODEV (-3)   /* no HIP device visible                          */

/* The version of this file, stated here only: the library returns it and the Python binding, which derives its ctypes structs,
 * constants and prototypes from this file, compares the two at load time.  It moves whenever a struct or a prototype below changes.
 * The binding reads the restricted C written here: scalar and pointer fields, enum entries and macros with integer values,
 * plain prototypes.  It refuses anything else (arrays, nested structs, bit-fields, function pointers) at import. */
#define ANODDPM_ABI_VERSION 43

int anoddpm_abi_version(void);          /* ANODDPM_ABI_VERSION of the header the library was built from */
const char *anoddpm_last_error(void);   /* [host] text of the last failure on this thread */
int anoddpm_device_count(void);
int anoddpm_struct_size(const char *name);   /* sizeof of the struct typedef'd as `name` ("anoddpm_igemm_args"); -1 for any other name,
                                                 for NULL, and for the small index this function took until version 31 */

/* ------------------------------------------------------------------ simplex ------------ */

/* simplex.py:166-192 (_init): seed -> permutation + gradient-index tables.  HOST function.
 * `seed` is the already int64-wrapped seed.  perm / pgi3: [host] int16[256] each. */
int anoddpm_simplex_perm_init(int64_t seed, int16_t *perm, int16_t *pgi3);

/* simplex.py:75-93 (rand_3d_fixed_T_octaves), :37-54 (rand_3d_octaves), :833-840 (_noise3a),
 * :321-830 (_noise3), :202-208 (_extrapolate3): multi-octave OpenSimplex-3D field.
 *   out[s][y][x] = sum_o persistence^o * noise3(x/f_o, y/f_o, z_s/f_o),  f_o = frequency/2^o
 * evaluated in fp64 in the reference's exact operation order (bit-exact), octave 0 first.
 * One launch fills `nslices` slices of H x W.
 *   zvals   [dev] int64[nslices] integer z index of each slice (timesteps, or 0..D-1);
 *           NULL means z_s = z0 + s
 *   tables  [dev] int16: table set n at tables + n*512 = {perm[256], pgi3[256]}
 *   table_sel [dev] int32* or NULL: *table_sel = index of the table set for this launch
 *           (lets a captured graph walk through pre-generated per-step tables)
 *   table_slice_stride: table set used by slice s = base + s*table_slice_stride (0 = shared)
 *   out_slice_stride: elements between consecutive slices in `out` (>= H*W)
 * _f64 stores doubles (Simplex_CLASS API); _f32 stores the fp64 result rounded to fp32
 * (what generate_simplex_noise's assignment into a float tensor does, GaussianDiffusion.py:125). */
typedef struct {
    void *out;                 /* [dev] double* or float* */
    const int64_t *zvals;      /* [dev] or NULL */
    const int16_t *tables;     /* [dev] */
    const int32_t *table_sel;  /* [dev] or NULL */
    int64_t z0;
    int64_t out_slice_stride;
    int32_t nslices, H, W;
    int32_t table_slice_stride;
    int32_t table_sel_scale;   /* table index = (*table_sel) * table_sel_scale + ... */
    int32_t octaves;
    double persistence;
    double frequency;
} anoddpm_simplex_args;

int anoddpm_simplex3_octaves_f64(const anoddpm_simplex_args *a, void *stream);
int anoddpm_simplex3_octaves_f32(const anoddpm_simplex_args *a, void *stream);

/* simplex.py:833-840 (_noise3a) / :31-35 (noise3, noise3array): one octave on arbitrary fp64
 * coordinate vectors, out[z][y][x] = noise3(X[x], Y[y], Z[z]); all pointers [dev]; tables = one
 * 512-entry set. */
int anoddpm_simplex3_grid_f64(double *out, const double *X, int32_t nx, const double *Y, int32_t ny,
                              const double *Z, int32_t nz, const int16_t *tables, void *stream);

/* 2-D OpenSimplex on a SQUARE n x n grid (upstream's _noise2a / rand_2d_octaves are only well defined for square
 * shapes: simplex.py:315-318 indexes noise[i * y.size + j], :69 adds a (W,H) array to a (H,W) field).
 *   octaves: out[i][j] = sum_o persistence^o * noise2(j / f_o, i / f_o), f_o = frequency / 2^o   (simplex.py:56-73)
 *   grid:    out[i][j] = noise2(X[j], Y[i])                                                       (simplex.py:311-318)
 * tables: the int16[512] table of anoddpm_simplex_perm_init (only perm[256] is used).  Bit-exact fp64. */
int anoddpm_simplex2_octaves_f64(double *out, int32_t n, const int16_t *tables, int32_t octaves,
                                 double persistence, double frequency, void *stream);
int anoddpm_simplex2_grid_f64(double *out, const double *X, const double *Y, int32_t n, const int16_t *tables,
                              void *stream);

/* ------------------------------------------------------------------ diffusion ---------- */

/* GaussianDiffusion.py:361-371 (sample_q) and :373-382 (sample_q_gradual):
 *   out = ca[t[b]] * x + cb[t[b]] * noise        (separate mul, mul, add: no FMA)
 * x, noise, out: [dev] fp32 [B][n]; t: [dev] int64[B]; ca, cb: [dev] fp32[T] (the reference's
 * fp64 tables rounded to fp32, which is what extract() does after its gather, :32-36). */
int anoddpm_q_sample(float *out, const float *x, const float *noise, const int64_t *t,
                     const float *ca, const float *cb, int32_t B, int64_t n, int32_t T,
                     void *stream);

/* GaussianDiffusion.py:269-318 (p_mean_variance + sample_p) with the model output given:
 *   pred_x0 = clamp(c_recip[t]*x_t - c_recipm1[t]*eps, -1, 1)
 *   mean    = c_coef1[t]*pred_x0 + c_coef2[t]*x_t
 *   x_prev  = mean + (t != 0) * sigma[t] * noise ,  sigma = exp(0.5*model_log_variance)
 * all fp32 with the reference's operation order (bit-exact vs. its CPU path).
 * x_prev may alias x_t.  pred_x0 and mean_out may be NULL.  noise may be NULL (treated as 0). */
typedef struct {
    float *x_prev;
    float *pred_x0;
    float *mean_out;
    const float *x_t;
    const float *eps;
    const float *noise;
    const int64_t *t;          /* [dev] int64[B] */
    const float *c_recip;      /* sqrt_recip_alphas_cumprod      fp32[T] */
    const float *c_recipm1;    /* sqrt_recipm1_alphas_cumprod    fp32[T] */
    const float *c_coef1;      /* posterior_mean_coef1           fp32[T] */
    const float *c_coef2;      /* posterior_mean_coef2           fp32[T] */
    const float *c_sigma;      /* exp(0.5*log(model_var))        fp32[T] */
    int64_t n;                 /* elements per sample */
    int32_t B, T;
} anoddpm_p_update_args;

int anoddpm_p_sample_update(const anoddpm_p_update_args *a, void *stream);

/* Advance a device-resident chain state after a reverse step: t[b] -= 1 for all b, *step += 1.
 * (The reference rebuilds t on the host every step, GaussianDiffusion.py:351-352.) */
int anoddpm_chain_advance(int64_t *t, int32_t B, int32_t *step, void *stream);

/* ------------------------------------------------------------------ seeded Gaussian noise */

/* Counter-based standard normals: a sample is a pure function of (seed, stream, step, element index).
 *   generator  Philox4x32-10 (Random123: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85)
 *   key        k0 = seed & 0xffffffff, k1 = seed >> 32
 *   counter    (c0, c1, c2, c3) = (quad, stream, step, domain); quad = i >> 2, i the element index inside ONE sample
 *   normals    u(w) = ((w >> 9) + 0.5) * 2^-23;  r = sqrtf(-2 logf(u(w0)));  elements 4 quad + 0 / 1 = r cos / sin(2 pi u(w1)),
 *              elements 4 quad + 2 / 3 the same from (w2, w3).  A partial last quad uses its leading lanes.
 *   domain     0 reverse-step noise, 1 forward / training noise, 2 plain fill, 3 known-region noise (the step is the timestep
 *              the step LANDS on; see anoddpm_p_sample_update_known at the end of this file), 4 re-noise of a resampling jump.
 *              A resampled chain adds 8 * visit to 0, 3 and 4 (anoddpm_p_sample_update_resample).
 * Key block, the same four arguments in every entry point below:
 *   seed     [dev] one 64-bit seed
 *   streams  [dev] int32[B] read as uint32: the stream of sample b; NULL: stream0 + b
 *   stream0, domain
 * Seed and stream ids are read on the DEVICE at run time: a captured graph that contains one of these launches follows a
 * re-written seed or stream id on its next replay. */

/* out: [dev] [B][n], uint32 words (kind 0) or fp32 normals (kind 1).  t: [dev] int64[B], the step of sample b, or NULL: step0 for
 * every sample.  T > 0: a negative t[b] means t[b] + T, as in the update kernels; T == 0: t[b] is taken as it is. */
int anoddpm_philox_fill(void *out, int32_t kind, int32_t B, int64_t n,
                        const uint64_t *seed, const int32_t *streams, uint32_t stream0, uint32_t domain,
                        const int64_t *t, uint32_t step0, int32_t T, void *stream);

/* The same words on the HOST (no GPU): out[4 j + k] = word k of counter (quad0 + j, stream, step, domain), j < nquads. */
int anoddpm_philox_bits_host(uint64_t seed, uint32_t stream, uint32_t step, uint32_t domain, uint32_t quad0, int64_t nquads,
                             uint32_t *out);

/* anoddpm_p_sample_update with the step noise generated in the kernel: a->noise must be NULL, the domain is 0, the step is the
 * kernel's own normalised t[b].  Bit-identical to anoddpm_philox_fill (kind 1, same key, domain 0, T = a->T) followed by
 * anoddpm_p_sample_update; 12 B/pixel and one launch instead of 4 + 16 B/pixel and two. */
int anoddpm_p_sample_update_gauss(const anoddpm_p_update_args *a, const uint64_t *seed, const int32_t *streams, uint32_t stream0,
                                  void *stream);

/* One step of the strided, DDIM-style sampler (Song et al., "Denoising Diffusion Implicit Models", eq. 12 and 16), the
 * same launch shape as anoddpm_p_sample_update: from t = t[b] to s = t - *stride, with a_t = alphas_cumprod[t] and a_s = 1 for s < 0,
 *   var     = eta^2 * (1 - a_s) / (1 - a_t) * (1 - a_t / a_s)            fp64, once per workgroup; the three coefficients
 *   c_x0, c_dir, sigma = sqrt(a_s), sqrt(max(1 - a_s - var, 0)), sqrt(var)        are each rounded to fp32 once
 *   pred_x0 = clamp(c_recip[t]*x_t - c_recipm1[t]*eps, -1, 1)            (bit-identical to anoddpm_p_sample_update's)
 *   e'      = eps where the clamp did not bind, (c_recip[t]*x_t - pred_x0) / c_recipm1[t] where it did
 *   mean    = c_x0*pred_x0 + c_dir*e'
 *   x_prev  = mean + sigma*noise ;  with sigma == 0 x_prev = mean and the noise is neither read nor generated
 * a: the struct of anoddpm_p_sample_update; c_coef1, c_coef2 and c_sigma are ignored (may be NULL).
 * alphas_cumprod [dev] fp64[a->T]; stride [dev] one int32 >= 1; eta [dev] one float in [0, 1].  Stride and eta are read on the
 * DEVICE at run time: a captured graph follows a re-written word on its next replay.  A stride < 1 read there gives a NaN sample,
 * as an out-of-range t[b] does; neither reads out of bounds.
 * seed == NULL: the noise is a->noise, or none when that is NULL too.  Otherwise it is generated in the kernel from the key block
 * (seed, streams, stream0) exactly as in anoddpm_p_sample_update_gauss -- domain 0, step = normalised t[b] -- and a->noise must
 * be NULL. */
int anoddpm_strided_update(const anoddpm_p_update_args *a, const double *alphas_cumprod, const int32_t *stride, const float *eta,
                           const uint64_t *seed, const int32_t *streams, uint32_t stream0, void *stream);

/* anoddpm_chain_advance for the strided sampler: t[b] = max(t[b] - *stride, 0) for all b, *step += 1; stride [dev] one int32.
 * The floor keeps idle and finished chain slots inside the tables. */
int anoddpm_chain_advance_strided(int64_t *t, int32_t B, int32_t *step, const int32_t *stride, void *stream);

/* anoddpm_q_sample with N generated in the kernel: out = ca[t[b]] * x + cb[t[b]] * N, domain 1, step = normalised t[b];
 * noise_out ([dev] [B][n] or NULL) receives N.  Bit-identical to anoddpm_philox_fill (domain 1) + anoddpm_q_sample. */
int anoddpm_q_sample_gauss(float *out, float *noise_out, const float *x, const int64_t *t, const float *ca, const float *cb,
                           int32_t B, int64_t n, int32_t T,
                           const uint64_t *seed, const int32_t *streams, uint32_t stream0, void *stream);

/* ------------------------------------------------------------------ UNet ops ----------- */

/* Operation codes for anoddpm_run_ops: one UNet forward is a flat list of these. */
enum {
    ANODDPM_OP_IGEMM = 1,        /* anoddpm_igemm_args       */
    ANODDPM_OP_GN_STATS = 2,     /* anoddpm_gn_args          */
    ANODDPM_OP_SOFTMAX = 3,      /* anoddpm_softmax_args     */
    ANODDPM_OP_RESAMPLE = 4,     /* anoddpm_resample_args    */
    ANODDPM_OP_LINEAR = 5,       /* anoddpm_linear_args      */
    ANODDPM_OP_POSEMB = 6,       /* anoddpm_posemb_args      */
    ANODDPM_OP_STEM = 7,         /* anoddpm_stem_args        */
    ANODDPM_OP_LAYOUT = 8,       /* anoddpm_layout_args      */
    ANODDPM_OP_CHAN_STATS = 9,   /* anoddpm_chan_stats_args  */
    ANODDPM_OP_GN_FINALIZE = 10, /* anoddpm_gn_finalize_args */
    ANODDPM_OP_HEAD = 11,        /* anoddpm_head_args        */
    /* 12 / 14 are the profiler's slots for the Winograd F(2x2) / F(4x4) launches of ANODDPM_OP_IGEMM, 13 for its cfg 5 launches */
    /* training step (backward twins and per-step weight packing) */
    ANODDPM_OP_WGRAD3 = 16,      /* anoddpm_wgrad_args        */
    ANODDPM_OP_WGRAD1 = 17,      /* anoddpm_wgrad1_args       */
    ANODDPM_OP_GN_BWD = 18,      /* anoddpm_gn_bwd_args       */
    ANODDPM_OP_PACK = 19,        /* anoddpm_pack_args         */
    ANODDPM_OP_SOFTMAX_BWD = 20, /* anoddpm_softmax_bwd_args  */
    ANODDPM_OP_TRANSPOSE = 21,   /* anoddpm_transpose_args    */
    ANODDPM_OP_LINEAR_BWD = 22,  /* anoddpm_linear_bwd_args   */
    ANODDPM_OP_STEM_BWD = 23,    /* anoddpm_stem_bwd_args     */
    ANODDPM_OP_HEAD_BWD = 24,    /* anoddpm_head_bwd_args     */
    ANODDPM_OP_COLSUM_FOLD = 25, /* anoddpm_colsum_fold_args  */
    ANODDPM_OP_ATTENTION = 26,   /* anoddpm_attention_args    */
    ANODDPM_OP_PACK_BATCH = 27,  /* anoddpm_pack_batch_args   */
    ANODDPM_OP_LINEAR_BWD_BATCH = 28, /* anoddpm_linear_bwd_batch_args */
    ANODDPM_OP_DROPOUT = 29,     /* anoddpm_dropout_args      */
    ANODDPM_OP_MAX = 32
};

/* Implicit-GEMM convolution / GEMM on the f32 MFMA pipe (v_mfma_f32_32x32x2_f32: exact fp32).
 *   out[z][p][n] = alpha * sum_{tap,k} A(z, p shifted by tap, k) * Bmat(tap, k, n)
 *                  + bias[n] + temb[b][n] + res[z][p][n]
 * Replaces: nn.Conv2d 3x3 / 1x1 (UNet.py:172,193,200,280,387), nn.Conv1d k=1 (UNet.py:115,117),
 * the two einsums of QKVAttention (UNet.py:148-152), and -- fused into the A load -- GroupNorm32
 * apply + SiLU (UNet.py:170-171,190-191,386,409-411), AvgPool2d / nearest x2 (UNet.py:70,89)
 * and torch.cat([h, skip]) (UNet.py:402: the two sources are read in place).
 * z = blockIdx.z decomposes as b = z / heads, head = z % heads. */
typedef struct {
    /* A operand: up to two NHWC sources concatenated along channels */
    const float *a0, *a1;           /* a1 NULL when single source */
    const float *gn_scale, *gn_shift; /* [B][K] per-sample per-channel affine or NULL */
    /* B operand */
    const float *bmat;              /* packed weights, or activations for b_mode 1/2 */
    /* epilogue */
    const float *bias;              /* [N] or NULL */
    const float *temb;              /* [B][temb_ld] or NULL */
    const float *res;               /* residual, same layout as out, or NULL */
    float *out;
    float *ws;                      /* split-K workspace [ksplit][Z][P][N] or NULL */
    int64_t a0_bs, a0_hs, a1_bs, a1_hs;   /* batch / head strides (floats) */
    int64_t b_bs, b_hs;
    int64_t o_bs, o_hs, r_bs, r_hs;
    int32_t c0, c1;                 /* channels taken from a0 / a1 (K = c0 + c1) */
    int32_t a0_ld, a1_ld;           /* floats between consecutive pixels */
    int32_t H, W;                   /* OUTPUT image dims; P = H*W                */
    int32_t ks;                     /* 1 or 3 (square, stride 1, pad ks/2)       */
    int32_t a_mode;                 /* 0 same-res, 1 source is half-res (nearest x2), 2 source is double-res (avg 2x2) */
    int32_t act;                    /* 1: SiLU on the A operand (after the affine) */
    int32_t b_mode;                 /* 0 packed [taps][K/4][N][4]; 1 rows [N][K] (ldb); 2 rows [K][N] (ldb) */
    int32_t ldb;
    int32_t N;
    int32_t temb_ld;
    int32_t out_ld, res_ld;
    int32_t B, heads;               /* Z = B*heads */
    int32_t ksplit;                 /* >= 1 */
    int32_t cfg;                    /* 0: 128x128 tile, 1: 64x64 tile, 2: Winograd F(2x2,3x3): ks 3, a_mode 0/1, H,W % 16 == 0,
                                       bmat = transformed weights [16][K/4][N][4] (G g G^T); 3: Winograd F(4x4,3x3): as 2 with
                                       N % 64 == 0, ksplit 1, bmat [36][K/4][N][4]; statistics: one row per 16x16 patch;
                                       4: streaming 1x1 for large maps (pointwise.hip): ks 1, a_mode 0, b_mode 0, heads 1, ksplit 1,
                                       no gn / act / stats, K % 128 == 0, K <= 512, c0 % 32 == 0, H*W % 32 == 0, N % 64 == 0;
                                       5: small maps without split-K (smallmap.hip), see anoddpm_smallmap_tile;
                                       6: Winograd F(2x2,3x3) on 16x16 / 32x32 maps without split-K (wino23s.hip), see anoddpm_wino23s_tile;
                                       bmat as cfg 2;
                                       7: OPT-IN side configuration, never chosen by default: cfg 3's layer with every fp32 operand split into
                                       three bf16 pieces and six products on v_mfma_f32_16x16x32_bf16 (winograd43b.hip): NOT the reference's
                                       arithmetic class.  N % 128 == 0, K % 32 == 0 per source, ksplit 1; bmat = anoddpm_pack_wino43_bf16x3 */
    float alpha;
    int32_t gn_ld;                  /* row length of gn_scale/gn_shift (= K) */
    float *stats;                   /* or NULL: per-channel partial sums of the OUTPUT, [B][tiles*2][N][2]
                                       {sum, sum of squares} per wave-row of each pixel tile (needs ksplit==1,
                                       heads==1); consumed by anoddpm_gn_finalize -- GroupNorm statistics
                                       without re-reading the tensor.  With ksplit > 1 the split-K reduction
                                       emits them instead, as [B][stats_rows][N][2] */
    int32_t stats_rows;             /* split-K only: number of pixel slabs (= rows) of the statistics */
    /* Split-K tail with the consumer's GroupNorm folded in (ksplit > 1, heads == 1, N % 128 == 0; `stats` must be NULL).  With
     * tail_csum set, the tail launch is partitioned by (GroupNorm group, image) instead of pixel slabs: a workgroup folds the K
     * slabs of its channels over ALL pixels of its image, so it owns complete per-channel sums -- it writes them to tail_csum and,
     * when tail_gamma is set, finishes GroupNorm(tail_groups, N + tail_c1) of torch.cat([out, other], 1) on the spot (UNet.py:409-411,
     * 402): scale / shift of its group's channels, the other source's channels taken from ITS folded sums.  One launch replaces the
     * statistics rows + anoddpm_gn_finalize of the plain tail.  (N + tail_c1) / tail_groups must be a multiple of 4. */
    double *tail_csum;              /* [B][N][2] {sum, sum of squares} over the image, fp64 */
    const double *tail_other;       /* [B][tail_c1][2] of the second source, or NULL */
    const float *tail_gamma, *tail_beta;   /* [N + tail_c1], or NULL: folded sums only */
    float *tail_scale, *tail_shift; /* [B][N + tail_c1] */
    float *tail_mean, *tail_rstd;   /* optional [B][tail_groups] (training) */
    int32_t tail_c1, tail_groups;
    float tail_eps;
    /* cfg 5 / 6 (smallmap.hip, wino23s.hip), and cfg 3 with fp64 sums (fold_fmt* == 1, see stats_csum): the GroupNorm of the A operand FINISHED IN THE KERNEL'S PROLOGUE from its producers' statistics
     * (UNet.py:409-411 over torch.cat([h, skip], 1)) -- the arguments of anoddpm_gn_finalize, consumed in place: no finalize
     * launch between producer and consumer.  With fold_gamma set, gn_scale / gn_shift are ignored.  fp64 fold in a fixed order
     * (rows ascending per channel, channels ascending per group), biased variance, fold_eps. */
    const float *fold_stats0, *fold_stats1;   /* as anoddpm_gn_finalize_args.stats0 / stats1 */
    const float *fold_gamma, *fold_beta;      /* [K], or NULL: no fold */
    int32_t fold_rows0, fold_rows1, fold_fmt0, fold_fmt1;
    int32_t fold_groups;
    float fold_eps;
    /* cfg 3 only: res_mode 1 = the residual is the block input at HALF resolution and is repeated 2x2 on the read (the
     * `x_upd = Upsample(x)` skip path of an up-sampling ResBlock, UNet.py:196-198, 89: F.interpolate(scale_factor=2, mode="nearest")
     * is never materialised); res: [B][(H/2)*(W/2)][res_ld], r_bs its batch stride.  0: res has the output's resolution. */
    int32_t res_mode;
    /* cfg 3 only, ksplit == 1, heads == 1, `stats` NULL (round 6): per-channel {sum, sum of squares} of the OUTPUT, added to
     * [B][N][2] fp64 with device-scope atomic adds, one pair per workgroup and channel (fp32 sums over the workgroup's 256 pixels,
     * as the `stats` rows hold them).  The buffer must be ZERO before the launch (anoddpm_posemb_args.zero clears a whole plan's
     * buffers at the start of a forward).  It is the fmt-1 statistics source of anoddpm_gn_finalize / fold_*: a cfg 3 consumer
     * finishes the GroupNorm in its prologue from it (fold_* with fold_fmt0 = fold_fmt1 = 1 -- the only formats cfg 3 folds),
     * so that no finalize launch sits between two F(4x4,3x3) layers.  fp64 sums of fp32 partials: the order of the atomic adds
     * changes the result by at most an ulp of the double. */
    double *stats_csum;
    /* cfg 3 on the 128-channel grid (anoddpm_f43_channel_sliced(...) == 1), ksplit == 1, heads == 1, plain operand (no gn / act),
     * no bias / temb / res (round 6, training): the launch is the DATA GRADIENT da of a 3x3 convolution whose operand was
     * a = SiLU(GroupNorm(x)) (diffusion_training.py:102 through UNet.py:170-172, 190-193), and the epilogue -- which holds da in
     * registers -- also performs the REDUCTION pass of anoddpm_gn_silu_backward: it reads x (the GroupNorm's input, one value per
     * output it stores; two concatenated sources as there), forms dy = da * silu'(gamma * xhat + beta), xhat = (x - mean) * rstd,
     * and writes gnb_partial[b][tile][c] = { sum dy, sum dy * xhat } over the workgroup's 16 x 16 pixels (fp32 sums of 256 values,
     * stored as fp64): exactly the `partial` rows of anoddpm_gn_bwd_args with nslab = (H / 16) * (W / 16), which is then called
     * with partial_ready = 1 and runs its fold + elementwise launches only.  One pass over x and da less per layer.
     * N (this launch's output channels) = gnb_c0 + the second source's channels; gnb_c0 % 16 == 0. */
    double *gnb_partial;            /* or NULL: plain launch */
    const float *gnb_x0, *gnb_x1;   /* the GroupNorm's input sources, NHWC at the OUTPUT resolution of this launch */
    const float *gnb_gamma, *gnb_beta;   /* [N] */
    const float *gnb_mean, *gnb_rstd;    /* [B][gnb_groups] */
    int64_t gnb_x0_bs, gnb_x1_bs;
    int32_t gnb_c0, gnb_x0_ld, gnb_x1_ld, gnb_groups;
} anoddpm_igemm_args;

int anoddpm_igemm(const anoddpm_igemm_args *a, void *stream);
/* Statistics rows per image the launch `a` writes to `stats` ([B][rows][N][2]), from cfg, ksplit, H, W, ks, c0, c1, N, B and
 * stats_rows -- the tile count its launcher takes its grid from, times the rows a tile writes: stats_rows for split-K, 0 for a
 * configuration that writes none (cfg 4), a negative ANODDPM_E* code (anoddpm_last_error) for a shape the configuration refuses.
 * The caller sizes the buffer with it; pointers of `a` are not read. */
int anoddpm_igemm_stats_rows(const anoddpm_igemm_args *a);
/* 1 when a cfg 3 launch of this shape (ksplit 1) runs on the channel-sliced 128-channel kernel (winograd43r.hip) -- the one that
 * takes gnb_partial -- 0 when the launcher picks 64-channel workgroups (grids that would leave CUs idle, N % 128 != 0) */
int anoddpm_f43_channel_sliced(int32_t H, int32_t W, int32_t N, int32_t B);

/* cfg 5 of anoddpm_igemm: contractions on maps of <= 256 pixels WITHOUT split-K (smallmap.hip) -- the batch is folded into the
 * GEMM's M, a workgroup owns TM output rows x TN channels over all of K' = taps * K and its eight waves split K' (fold through
 * LDS, fixed order): one launch per layer instead of main + split-K tail (+ GroupNorm finalize, see fold_*).  ks 1 or 3, a_mode 0,
 * b_mode 0, heads 1, ksplit 1, H * W <= 256, W in {4, 8, 16}, K % 16 == 0, 16 <= K <= 1024, N % 32 == 0.  `stats` rows: one per
 * TM-pixel tile, [B][P / TM][N][2].  Returns the tile the launch will use as (TM / 16) * 16 + TN / 16, or 0 when the shape is
 * not taken (the caller then uses cfg 0 / 1 / 2). */
int anoddpm_smallmap_tile(int32_t ks, int32_t H, int32_t W, int32_t K, int32_t c0, int32_t N, int32_t B);

/* Weights of cfg 7: OIHW [N][K][3][3] fp32 -> U = G g G^T of F(4x4,3x3) (fp64 transform, rounded once to fp32) split into three bf16
 * planes, out = [3 pieces][36][K/8][N][8] bf16 (3 * 36 * N * K * 2 bytes).  K % 8 == 0. */
int anoddpm_pack_wino43_bf16x3(const float *w, void *out, int32_t N, int32_t K, void *stream);

/* cfg 6 of anoddpm_igemm: the 3x3 convolutions on 16x16 and 32x32 maps as Winograd F(2x2,3x3) WITHOUT split-K (wino23s.hip):
 * a workgroup owns 8x8 output pixels of one image x 32 or 64 channels over all of K, its eight waves split the sixteen transform
 * positions; one launch instead of main + split-K tail (+ GroupNorm finalize: fold_* as cfg 5).  a_mode 0 / 1, b_mode 0, heads 1,
 * ksplit 1, K % 32 == 0, 64 <= K <= 1024, N % 32 == 0; bmat = the F(2x2,3x3) weights of cfg 2.  `stats` rows: one per workgroup
 * tile, [B][(H / 8) * (W / 8)][N][2].  Returns the channel tiles per workgroup (2 or 4), or 0 when the shape is not taken. */
int anoddpm_wino23s_tile(int32_t H, int32_t W, int32_t K, int32_t c0, int32_t N, int32_t B, int32_t a_mode);

/* GroupNorm statistics -> per-sample per-channel affine (UNet.py:409-411 / nn.GroupNorm(32,C),
 * eps 1e-5, biased variance), over up to two concatenated NHWC sources:
 *   scale[b][c] = rstd[b,g(c)] * gamma[c];  shift[b][c] = beta[c] - mean[b,g(c)] * scale[b][c]
 * `partial` is scratch: double[B][nslab][64]. */
typedef struct {
    const float *a0, *a1;
    const float *gamma, *beta;      /* [C] */
    float *scale, *shift;           /* [B][C] */
    double *partial;
    int64_t a0_bs, a1_bs;
    int32_t c0, c1, a0_ld, a1_ld;
    int32_t P;                      /* pixels per image */
    int32_t B, groups, nslab;
    float eps;
} anoddpm_gn_args;

int anoddpm_gn_stats(const anoddpm_gn_args *a, void *stream);

/* Per-channel partial sums of an NHWC tensor in the format the igemm epilogue emits:
 * stats[b][slab][c] = {sum, sum of squares} over the slab's pixels (fp32 pairs). */
typedef struct {
    const float *a;
    float *stats;                   /* [B][nslab][C][2] */
    int64_t a_bs;
    int32_t C, a_ld, P, B, nslab;
} anoddpm_chan_stats_args;

int anoddpm_chan_stats(const anoddpm_chan_stats_args *a, void *stream);

/* GroupNorm(32, C) affine from per-channel partial sums of one or two concatenated sources
 * (UNet.py:409-411 over torch.cat([h, skip], 1), UNet.py:402): fp64 fold, biased variance, eps. */
typedef struct {
    const float *stats0, *stats1;   /* [B][rows][c][2]; stats1 NULL when single source */
    const float *gamma, *beta;      /* [C] */
    float *scale, *shift;           /* [B][C] */
    int32_t rows0, rows1, c0, c1;
    int32_t P, B, groups;
    float eps;
    float *mean_out, *rstd_out;     /* optional [B][groups]: saved for anoddpm_gn_silu_backward (training) */
    int32_t fmt0, fmt1;             /* 0: statsN = fp32 rows as above; 1: statsN = ONE row of fp64 pairs [B][c][2] (the tail_csum of
                                       anoddpm_igemm_args; rowsN is ignored) */
} anoddpm_gn_finalize_args;

int anoddpm_gn_finalize(const anoddpm_gn_finalize_args *a, void *stream);

/* Row softmax in place (UNet.py:151): x[r][0..L) <- softmax(x[r][:]); rows = B*heads*L. */
typedef struct {
    float *x;
    int64_t rows;
    int32_t L;
} anoddpm_softmax_args;

int anoddpm_softmax_rows(const anoddpm_softmax_args *a, void *stream);

/* Fused QKVAttention core (UNet.py:137-153; QKVAttentionLegacy channel order): per (image, head)
 *     weight = softmax(scale * q^T k),   a = weight v
 * in one launch: qkv [B][L][3*heads*ch] holds, for head h, q at channel h*3*ch, k at +ch, v at +2*ch (the output of the to_qkv
 * convolution, UNet.py:115,122); out [B][L][heads*ch]; probs (or NULL) receives the softmax [B*heads][L][L] (the training
 * backward reads it).  scale = 1/sqrt(ch) (the reference scales q and k by ch^-1/4 each, UNet.py:147-150).
 * Needs L % 16 == 0, 16 <= L <= 1024 (the score rows of a 16-query block live in LDS), ch a power of two in [16, 512].
 * Other shapes: three anoddpm_igemm / anoddpm_softmax_rows launches (b_mode 1 / 2). */
typedef struct {
    const float *qkv;
    float *out;
    float *probs;
    int32_t B, L, heads, ch;
    float scale;
} anoddpm_attention_args;

int anoddpm_attention(const anoddpm_attention_args *a, void *stream);

/* 2x resampling of an NHWC tensor (the x_upd path of ResBlock, UNet.py:177-181,207):
 * mode 1: nearest x2 up (in H x W -> out 2H x 2W); mode 2: 2x2 average pool (in -> H/2 x W/2); mode 3: the even pixels
 * (2i, 2j) -> H/2 x W/2, i.e. a stride-2 convolution's outputs picked from the stride-1 result (Downsample, UNet.py:60-75);
 * mode 4: the adjoint of mode 3 -- in H x W -> out 2H x 2W with out[2i][2j] = in[i][j] and zeros elsewhere (the gradient of the
 * stride-2 convolution's output placed on the stride-1 grid).
 * scale (0 is read as 1) multiplies the result and accumulate != 0 adds it to `out`: the backward of one mode is the
 * other one scaled -- d(avg pool) = nearest-up * 0.25, d(nearest-up) = avg pool * 4 (the sum of the four children). */
typedef struct {
    const float *in;
    float *out;
    int32_t B, H, W, C;             /* INPUT dims */
    int32_t mode;
    float scale;
    int32_t accumulate;
    /* optional second output of mode 2: out_act = 2x2 average of silu(gn_scale[b][c] * in + gn_shift[b][c]) -- the operand the
     * first 3x3 convolution of a down block consumes (UNet.py:170-171, 70, 206), produced in the same pass over `in` so that
     * the convolution itself can run on the Winograd kernels */
    const float *gn_scale, *gn_shift;   /* [B][C] or NULL */
    float *out_act;                     /* [B][H/2][W/2][C] or NULL */
} anoddpm_resample_args;

int anoddpm_resample2x(const anoddpm_resample_args *a, void *stream);

/* Small-batch linear layer (UNet.py:273-275 time MLP; :185-188 per-block embedding projections,
 * all blocks batched into one launch by concatenating their weight rows):
 *   out[b][n] = act_out( sum_k act_in(in[b][k]) * w[n][k] + bias[n] ); 16 batch rows per launch (larger B: one launch per 16 rows). */
typedef struct {
    const float *in;                /* [B][K] */
    const float *w;                 /* [N][K] (nn.Linear layout) */
    const float *bias;              /* [N] or NULL */
    float *out;                     /* [B][N] */
    int32_t B, K, N;
    int32_t act_in, act_out;        /* 1 = SiLU */
} anoddpm_linear_args;

int anoddpm_linear_small(const anoddpm_linear_args *a, void *stream);

/* Sinusoidal timestep features (UNet.py:50-57): out[b][i] = sin(t_b*f_i), out[b][half+i] = cos(t_b*f_i),
 * f_i = exp(-i * ln(1e4)/half) in fp32 (table supplied by the caller so that it is bit-identical
 * to the host-computed one; t_b*f_i is one fp32 multiply as in torch.outer). */
typedef struct {
    const int64_t *t;               /* [dev] int64[B] */
    const float *freqs;             /* [dev] fp32[dim/2]: f_i, precomputed once on the host */
    float *out;                     /* [B][dim] */
    int32_t B, dim;
    float scale;
    /* optional (round 6): `zero_doubles` doubles at `zero` are cleared by the same launch -- the statistics accumulators
     * (anoddpm_igemm_args.stats_csum) of a whole forward plan, whose first op this is */
    double *zero;
    int64_t zero_doubles;
} anoddpm_posemb_args;

int anoddpm_posemb(const anoddpm_posemb_args *a, void *stream);

/* Stem convolution (UNet.py:280): 3x3, pad 1, Cin <= 4 NCHW input -> Cout NHWC output.
 * w: [9][Cin][Cout] fp32. */
typedef struct {
    const float *x;                 /* [B][Cin][H][W] (NCHW, as the caller hands it over) */
    const float *w;
    const float *bias;
    float *out;                     /* [B][H][W][Cout] */
    int32_t B, H, W, Cin, Cout;
    /* optional (Cin <= 2, W % 8 == 0, x 16-byte aligned): GroupNorm partial sums of the output, [B][stats_rows][Cout][2] floats
     * {sum, sum of squares}, one row per workgroup range -- the row format of anoddpm_chan_stats / the contraction epilogues.
     * stats_rows must be anoddpm_stem_stats_rows() of the shape. */
    float *stats;
    int32_t stats_rows;
} anoddpm_stem_args;

/* rows per image the fused stem statistics use for this shape, 0 when the shape has no fused form */
int anoddpm_stem_stats_rows(int H, int W, int Cin, int Cout);

int anoddpm_conv_stem(const anoddpm_stem_args *a, void *stream);

/* Head convolution (UNet.py:384-388): silu(GroupNorm affine(x)) -> 3x3 pad 1 -> Cout <= 4 channels.
 * x: NHWC [B][H][W][C]; w: [9][C][Cout]; out: NCHW [B][Cout][H][W] (the caller's layout). HBM-bound. */
typedef struct {
    const float *x;
    const float *w;
    const float *bias;              /* [Cout] or NULL */
    const float *gn_scale, *gn_shift; /* [B][C] */
    float *out;
    int32_t B, H, W, C, Cout;
} anoddpm_head_args;

int anoddpm_conv_head(const anoddpm_head_args *a, void *stream);

/* Layout change at the API edge: NHWC [B][P][C] -> NCHW [B][C][P] (C small, UNet output). */
typedef struct {
    const float *in;
    float *out;
    int32_t B, P, C;
    int32_t in_ld;
} anoddpm_layout_args;

int anoddpm_nhwc_to_nchw(const anoddpm_layout_args *a, void *stream);

/* Flat op list: the native executor behind UNetModel.forward (UNet.py:390-406). */
typedef struct {
    int32_t code;                   /* ANODDPM_OP_* */
    int32_t flags;
    const void *args;               /* [host] pointer to the matching *_args struct */
} anoddpm_op;

int anoddpm_run_ops(const anoddpm_op *ops, int32_t n, void *stream);

/* Per-class kernel timing with HIP events on the launch stream (bench.py roofline leg).
 * enable=1 starts recording one event pair per launched op; collect() synchronises the events
 * and returns accumulated milliseconds and launch counts per op code (arrays of ANODDPM_OP_MAX = 32); ANODDPM_OP_IGEMM
 * launches that run the Winograd kernels are booked under index 12 (cfg 2) / 14 (cfg 3) instead of 1, and the Winograd-domain
 * launches of ANODDPM_OP_WGRAD3 (algo 1) under index 15 instead of 16. */
int anoddpm_prof_enable(int32_t enable);
int anoddpm_prof_active(void);             /* 1 while event recording is on (graph capture must be avoided) */
int anoddpm_prof_collect(double *ms_per_code, int64_t *launches_per_code);
/* the ops recorded up to the last anoddpm_prof_collect, in launch order: profiler slot + milliseconds each; returns their count */
int anoddpm_prof_list(int32_t *codes, float *ms, int32_t cap);

/* ------------------------------------------------------------------ training ----------- */

/* Fused AdamW + EMA over a flat fp32 parameter buffer (diffusion_training.py:75,105,107 and
 * UNet.py:423-427): decoupled weight decay, bias-corrected moments, then
 * ema = decay*ema + (1-decay)*p.  grad_scale multiplies g first (global-norm clip factor).
 * The hyper-parameters are doubles: the constants the kernel multiplies by (1 - beta, 1 - beta^step, 1 - ema_decay,
 * 1 - lr*weight_decay, lr / (1 - beta1^step)) are formed from them in double and rounded to fp32 once, as torch.optim.AdamW
 * forms them from its Python floats. */
typedef struct {
    float *p, *m, *v, *ema;
    const float *g;
    const float *grad_scale;        /* [dev] fp32 scalar or NULL */
    int64_t n;
    double lr, beta1, beta2, eps, weight_decay, ema_decay;
    int32_t step;                   /* 1-based */
} anoddpm_adamw_args;

int anoddpm_adamw_ema(const anoddpm_adamw_args *a, void *stream);

/* Global gradient norm and clip factor of a flat fp32 buffer (clip_grad_norm_(params, max_norm), diffusion_training.py:104):
 *   out[0] = sum of squares, out[1] = its square root, out[2] = min(max_norm / (out[1] + 1e-6), 1)   (1 when max_norm <= 0)
 * out: [dev] fp32[3]; workspace: [dev] >= 2048 doubles.  Two-stage fp64 reduction in a fixed order, no atomics: replicas that
 * hold identical gradients compute identical clip factors. */
int anoddpm_sumsq(const float *g, int64_t n, float *out, double *workspace, float max_norm, void *stream);

/* ------------------------------------------------------------------ anomaly map + segmentation counts
 * One pass over an image and its `navg` reconstructions (the (t_distance, avg) chains of detection_A/B):
 *   mean over the chains                                  GaussianDiffusion.py:517, 572
 *   sqerr = (mean - real)^2                                detection.py:229; evaluation.py:31
 *   mse_img = sqerr*2 - 1 ; thr_img = (mse_img > 0)*2 - 1  GaussianDiffusion.py:518-520, 581-583; evaluation.py:13-15
 *   pred = (sqerr > threshold)                             detection.py:232 (threshold 0.5)
 * and the sums behind dice_coeff / IoU / precision / recall / FPR / PSNR (evaluation.py:26-76) as
 * counts[b][ANODDPM_ANOMALY_NCOUNTS] (fp64):
 *   0 sum(pred)  1 sum(mask)  2 sum(pred*mask)  3 #(mask==1&pred==1)  4 #(mask==1&pred==0)  5 #(mask==0&pred==1)
 *   6 #(mask==0&pred==0)  7 #(mask!=0 & pred!=0)  8 #(mask!=0 | pred!=0)  9 sum(sqerr)  10 max(real)  11 reserved (never written)
 * The mean is the sequential fp32 sum in chain order followed by one division: within navg * 2^-24 * mean_k|recon_k| of the exact
 * mean always, and equal to CPU ATen's torch.mean(dim=0) for the sizes tests/test_anomaly_reference.py found (navg <= 16 on slices
 * of a multiple of 64 floats).  max(real) is NaN when the image holds a NaN, like torch.max; sum(sqerr) likewise.
 * recon: [navg] slices of n floats per image, slice stride recon_as, image stride recon_bs (elements).
 * Any of mean / sqerr / mse_img / thr_img / pred may be NULL.  mask may be NULL (treated as all zero).
 * workspace: ANODDPM_ANOMALY_BLOCKS * B * NCOUNTS doubles [dev].  Deterministic (fixed-order fold). */
#define ANODDPM_ANOMALY_NCOUNTS 12
#define ANODDPM_ANOMALY_BLOCKS 64
typedef struct anoddpm_anomaly_args {
    const float *recon;
    const float *real;
    const float *mask;
    float *mean, *sqerr, *mse_img, *thr_img, *pred;
    double *counts;                 /* [B][ANODDPM_ANOMALY_NCOUNTS] */
    double *workspace;
    int64_t workspace_doubles;
    int64_t n;                      /* pixels (x channels) per image */
    int64_t recon_as, recon_bs;
    int32_t navg, B;
    float threshold;
} anoddpm_anomaly_args;

int anoddpm_anomaly_map(const anoddpm_anomaly_args *a, void *stream);

/* ------------------------------------------------------------------ what every metric / post-processing entry point below keeps
 * anoddpm_roc_auc, anoddpm_pro_auc, anoddpm_component_areas, anoddpm_ssim, anoddpm_distance_transform, anoddpm_surface_distance,
 * anoddpm_median2d, anoddpm_erode2d, anoddpm_small_components, anoddpm_gauss2d, anoddpm_map_scores, anoddpm_median3d,
 * anoddpm_erode3d, anoddpm_small_components3d, anoddpm_component_areas3d (tests/contract_cases.py holds the table that
 * tests/test_gpu_contract.py audits them by):
 *   memory     a call reads only the elements of its inputs the field comments name (n per segment, the strides between them
 *              are never touched) and writes only its outputs and its workspace: nothing in front of, between or behind them
 *   outputs    every element of every output is written by an accepted call, in every defined case (P == 0, K == 0, an empty
 *              border, a plane without foreground or background, a segment that breaks the precondition), except the curve
 *              arrays: entries [s][min(curve_len[s], curve_cap) ... curve_cap) are left untouched
 *   workspace  its contents need no initialisation on entry and are unspecified on exit; the outputs do not depend on them.
 *              `workspace_bytes` as reported is enough; nothing outside it is touched
 *   alignment  every pointer is aligned to its element type, and that is all: segments may start at any element (odd strides).
 *              The workspace is 4-byte aligned, 8-byte for anoddpm_pro_auc and anoddpm_ssim (they keep fp64 values in it)
 *   refusal    a call that returns an error has launched nothing and written nothing, neither outputs nor workspace */

/* ------------------------------------------------------------------ ROC curve + AUC of anomaly maps
 * Replaces sklearn.metrics.roc_curve / auc as the reference calls them on a flattened mask and squared-error map
 * (evaluation.py:79-87 ROC_AUC / AUC_score; detection.py:230-231 and :553-554, :569-570, :583-584 per test image, :640-643
 * for the concatenated data set).  S segments of n elements; one workgroup sorts one segment, one launch, deterministic.
 *   score  fp32, finite and >= 0 (-0.0 counts as +0.0); mask fp32, 0 or 1.  Elements that break this set bits of status[s]
 *          (ANODDPM_ROC_*); the other outputs of such a segment are not meaningful.
 *   score_stride / mask_stride: elements between consecutive segments (>= n; mask_stride 0 = one mask for every segment)
 *   auc[s]     twoU / (2 P N) in fp64, NaN when P == 0 or N == 0 (sklearn: NaN after a warning)
 *   counts[s]  {P, N, twoU, number of distinct scores}; twoU = sum over distinct scores v of P_v * (2 * N_below(v) + N_v):
 *              the tie-corrected Mann-Whitney statistic, exactly twice P N times the trapezoid area under sklearn's curve
 *   curve_*    optional (all four or none): the points roc_curve keeps with drop_intermediate=True, from the highest score
 *              down, WITHOUT the (0, 0, inf) point it prepends: curve_fps / curve_tps [S][curve_cap] counts, curve_thr
 *              [S][curve_cap] thresholds, curve_len[s] = points of segment s.  A segment with more than curve_cap points
 *              gets its first curve_cap points, its full count in curve_len and ANODDPM_ROC_CURVE_TRUNCATED; curve_cap = n
 *              (at least 2) always suffices.
 *   curve_mode ANODDPM_ROC_CURVE_DROP (0): the points above.  ANODDPM_ROC_CURVE_ALL: one point per distinct score, nothing
 *              dropped -- what sklearn.metrics.precision_recall_curve works on; needs the curve_* outputs
 *   ap[s]      optional: average precision = sum over distinct scores v of (P_v / P) * (tps_v / (tps_v + fps_v)), the counts
 *              being those of the prediction score >= v (sklearn.metrics.average_precision_score).  fp64, fixed summation
 *              order (same input, same bits).  NaN when P == 0 (sklearn: 0.0 after a warning), 1.0 when N == 0
 *   best_*     optional (all three or none): the largest Dice 2 tps / (tps + fps + P) over all thresholds, found by exact
 *              integer comparison, ties to the highest threshold: best_dice[s] (one fp64 division; NaN when P == 0),
 *              best_thr[s] that threshold, best_counts[s] = {tps, fps} of the prediction score >= best_thr[s]
 *   workspace  [dev] anoddpm_roc_workspace_bytes(S, n) bytes (three uint32 buffers of n + 1 words per segment)
 * n < 2^31.  twoU is exact in uint64; its conversion to fp64 is exact up to 2^53 (n <= 2^26 always is).  A launch with
 * curve_mode 0 and none of ap / best_* runs the same kernel as before these fields existed. */
#define ANODDPM_ROC_CURVE_DROP 0
#define ANODDPM_ROC_CURVE_ALL 1
#define ANODDPM_ROC_NAN 1
#define ANODDPM_ROC_INF 2
#define ANODDPM_ROC_NEGATIVE 4
#define ANODDPM_ROC_BAD_MASK 8
#define ANODDPM_ROC_CURVE_TRUNCATED 16
typedef struct anoddpm_roc_args {
    const float *score;             /* [dev] */
    const float *mask;              /* [dev] */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    double *auc;                    /* [dev] [S] */
    int64_t *counts;                /* [dev] [S][4] */
    int32_t *status;                /* [dev] [S] */
    int32_t *curve_fps, *curve_tps; /* [dev] [S][curve_cap] or NULL */
    float *curve_thr;               /* [dev] [S][curve_cap] or NULL */
    int32_t *curve_len;             /* [dev] [S] or NULL */
    int64_t curve_cap;
    int64_t n, score_stride, mask_stride;
    int32_t S;
    int32_t curve_mode;             /* ANODDPM_ROC_CURVE_* */
    double *ap;                     /* [dev] [S] or NULL */
    double *best_dice;              /* [dev] [S] or NULL */
    float *best_thr;                /* [dev] [S] or NULL */
    int64_t *best_counts;           /* [dev] [S][2] or NULL */
} anoddpm_roc_args;

int anoddpm_roc_auc(const anoddpm_roc_args *a, void *stream);
int64_t anoddpm_roc_workspace_bytes(int32_t S, int64_t n);   /* HOST function; -1 for S < 1, n < 1 or n >= 2^31 */

/* The same scores with every segment sorted by the whole chip (csrc/roc_wide.hip): for one long segment -- the curve pooled over a
 * whole test set, detection.py:538-643 roc_data -- where anoddpm_roc_auc keeps 255 of 256 compute units idle.  Same argument
 * struct, every field with the meaning above (strides, shared mask, all optional outputs); the S segments are processed one after
 * another on `stream`, each as a sequence of 16 to 18 launches with one workgroup per tile of `tile` keys, and share ONE segment's
 * workspace.  A launch boundary is the only ordering between workgroups.
 *   tile       keys per workgroup: a multiple of 256 from 256 up, or 0 for the library's choice.  One workgroup scans the
 *              [256][tiles] counter table of a sort pass, so n may be cut into at most ANODDPM_ROC_WIDE_MAX_TILES tiles: an
 *              explicit tile that needs more is refused; tile 0 is 4096 keys and grows with n so that every n < 2^31 is accepted
 *   workspace  [dev] anoddpm_roc_wide_workspace_bytes(S, n, tile) bytes, 16-byte aligned; about 20 n bytes (keys, run records and
 *              one fp64 average-precision term per run) whatever S is; never smaller for a larger n at the same tile
 * For every accepted input every output has the bits anoddpm_roc_auc writes for the same arguments, the status word of a segment
 * that breaks the precondition included (its other outputs stay not meaningful).  Argument checks as anoddpm_roc_auc, made before
 * anything is launched. */
#define ANODDPM_ROC_WIDE_MAX_TILES 2048
int anoddpm_roc_auc_wide(const anoddpm_roc_args *a, int32_t tile, void *stream);
int64_t anoddpm_roc_wide_workspace_bytes(int32_t S, int64_t n, int32_t tile);   /* HOST function; -1 where the call would be refused */

/* ------------------------------------------------------------------ mean structural similarity (SSIM) of image pairs
 * Replaces skimage.metrics.structural_similarity as the reference calls it (evaluation.py:46-47 SSIM; detection.py:241-246,
 * 360-362, 765-768, 855-858).  S segments, each one pair x = real, y = recon of [C][H][W] fp32; every operation after the load
 * is fp64 in a fixed order (deterministic):
 *   separable window w of odd length win (weights sum to 1) along W, then along H, boundary rule "reflect"
 *   (d c b a | a b c d | d c b a, scipy.ndimage mode "reflect");
 *   ux = F(x), uy = F(y), uxx = F(x*x), uyy = F(y*y), uxy = F(x*y)
 *   vx = cn*(uxx - ux*ux), vy = cn*(uyy - uy*uy), vxy = cn*(uxy - ux*uy)
 *   C1 = (K1*data_range)^2, C2 = (K2*data_range)^2            (skimage: K1 0.01, K2 0.03)
 *   S = ((2*ux*uy + C1) * (2*vxy + C2)) / ((ux*ux + uy*uy + C1) * (vx + vy + C2))
 *   mssim[s] = mean of S over all channels and the interior p <= i < H-p, p <= j < W-p, p = (win-1)/2
 * mode ANODDPM_SSIM_UNIFORM: w = 1/win, win odd in 3 ... 15 (skimage's default 7; cn = win^2/(win^2-1) is its sample covariance);
 * mode ANODDPM_SSIM_GAUSSIAN: w = exp(-k^2/(2*1.5^2)) normalised, k = -5 ... 5, win 11 (gaussian_weights=True; cn = 1).
 *   real_stride / recon_stride: elements between consecutive segments (>= C*H*W; real_stride 0 = one real for every segment)
 *   map        optional [S][C][H][W] fp32: S at every pixel, boundary included (skimage's full=True image)
 *   workspace  [dev] anoddpm_ssim_workspace_bytes(S, C, H, W) bytes (one fp64 partial sum per 16 x 32 tile)
 * win <= min(H, W).  NaN / inf in a segment's images propagate into that segment's mssim only; there is no status word.
 * Two launches (tiles, then a fixed-order fold), no atomics, no host synchronisation, no allocation: capturable in a hipGraph. */
#define ANODDPM_SSIM_UNIFORM 0
#define ANODDPM_SSIM_GAUSSIAN 1
typedef struct anoddpm_ssim_args {
    const float *real;              /* [dev] */
    const float *recon;             /* [dev] */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    double *mssim;                  /* [dev] [S] */
    float *map;                     /* [dev] [S][C][H][W] or NULL */
    int64_t real_stride, recon_stride;
    double cn, data_range, K1, K2;
    int32_t S, C, H, W;
    int32_t win, mode;
} anoddpm_ssim_args;

int anoddpm_ssim(const anoddpm_ssim_args *a, void *stream);
int64_t anoddpm_ssim_workspace_bytes(int32_t S, int32_t C, int32_t H, int32_t W);   /* HOST function; -1 for a dimension < 1 or S*C*tiles >= 2^31 */

/* ------------------------------------------------------------------ per-region overlap (PRO) curve and AUPRO of anomaly maps
 * The localisation score of Bergmann et al., "The MVTec Anomaly Detection Dataset", IJCV 2021: every connected ground-truth
 * region counts the same whatever its size, and the curve is integrated up to a false-positive rate `limit` (0.3 there).  The
 * reference has no counterpart.  Two entry points: the areas of the mask's regions, then the sort and the curve.
 *
 * anoddpm_component_areas: area[p] = pixel count of the connected component of (plane > level) that holds pixel p, 0 on the
 *   background -- numpy.bincount(lab.ravel())[lab] with lab, m = scipy.ndimage.label(plane > level, structure) and area 0 where
 *   lab == 0; counts[p] = m.  S planes of H x W at src + p * src_stride; connectivity 1: 4 neighbours, 2: 8 neighbours (the
 *   published choice).  The union-find of anoddpm_small_components (link, flatten, sizes) between a clear and a final launch
 *   of its own: five launches.  Integers only: independent of the order the atomics land in, same bits every run.
 *   workspace  [dev] anoddpm_small_components_workspace_bytes(S, H, W) bytes (declared with the post-processing entry points
 *              below, like anoddpm_small_components)
 *
 * anoddpm_pro_auc: S segments of m = planes_per_segment planes of H x W (n = m*H*W < 2^31 elements; m > 1 pools a data set
 *   into one curve).  A region is a component of one plane; components never link across planes.  With
 *     K = regions of the segment's planes, P = pixels inside a region (area != 0), N = n - P,
 *   the curve has one point per distinct score v, from the highest down, for the prediction score >= v:
 *     fps(v) = negatives predicted (an integer), FPR(v) = fps(v) / N (one fp64 division),
 *     PRO(v) = min(1, (sum over positives p with score(p) >= v of 1 / area(p)) / K)  -- the mean over the regions of the fraction
 *              of the region that is predicted; the clamp only removes an excess of an ulp.
 *   aupro[s] = the trapezoid area under the polyline (0, 0), (FPR, PRO)... for FPR <= limit, the segment that crosses the limit
 *   cut there by linear interpolation (a point exactly at the limit needs none), divided by limit.  NaN when K == 0 or N == 0.
 *   The sums of 1 / area are formed by a workgroup-wide fp64 scan in sorted order and the integral by a fixed-order sum: no
 *   atomics on floating-point values, same input, same bits, whatever else the launch holds.
 *   score      fp32, finite and >= 0 (-0.0 counts as +0.0), segment s at score + s * score_stride (>= n)
 *   area       int32 from anoddpm_component_areas, segment s at area + s * area_stride; area_stride 0 = one mask shared by
 *              every segment (a sweep's maps share their mask: its areas are computed once)
 *   region_counts  int64 per plane from anoddpm_component_areas: planes s*m ... s*m + m-1 belong to segment s (0 ... m-1 for
 *              every segment when area_stride is 0); K is folded from them inside the launch
 *   mask       optional: the fp32 mask the areas came from, at mask + s * mask_stride (0 = shared), only checked: a value other
 *              than 0 / 1 sets ANODDPM_ROC_BAD_MASK.  Scores that break the precondition set ANODDPM_ROC_NAN / _INF /
 *              _NEGATIVE in status[s]; the other outputs of such a segment are not meaningful, other segments are untouched
 *   counts[s]  {K, N, P, number of distinct scores}
 *   curve_*    optional (all four or none): every point of the curve without the (0, 0) point: curve_fps [S][curve_cap] int32,
 *              curve_pro [S][curve_cap] fp64, curve_thr [S][curve_cap] fp32, curve_len[s]; more than curve_cap points: the
 *              first curve_cap, the full count and ANODDPM_ROC_CURVE_TRUNCATED, as for anoddpm_roc_auc
 *   workspace  [dev] anoddpm_pro_workspace_bytes(S, n) bytes (keys and areas twice, one fp64 per curve point)
 * One workgroup per segment, one launch, no allocation, no host synchronisation: capturable in a hipGraph. */
typedef struct anoddpm_component_areas_args {
    const float *src;               /* [dev] */
    int32_t *area;                  /* [dev] [S][H][W] */
    int64_t *counts;                /* [dev] [S] */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    int64_t src_stride;
    int32_t S, H, W;
    int32_t connectivity;
    float level;
} anoddpm_component_areas_args;

typedef struct anoddpm_pro_args {
    const float *score;             /* [dev] */
    const int32_t *area;            /* [dev] */
    const int64_t *region_counts;   /* [dev] [S * planes_per_segment], or [planes_per_segment] when area_stride == 0 */
    const float *mask;              /* [dev] or NULL */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    double *aupro;                  /* [dev] [S] */
    int64_t *counts;                /* [dev] [S][4] */
    int32_t *status;                /* [dev] [S] */
    int32_t *curve_fps;             /* [dev] [S][curve_cap] or NULL */
    double *curve_pro;              /* [dev] [S][curve_cap] or NULL */
    float *curve_thr;               /* [dev] [S][curve_cap] or NULL */
    int32_t *curve_len;             /* [dev] [S] or NULL */
    int64_t curve_cap;
    int64_t score_stride, area_stride, mask_stride;
    double limit;                   /* 0 < limit <= 1 */
    int32_t S, planes_per_segment, H, W;
} anoddpm_pro_args;

int anoddpm_component_areas(const anoddpm_component_areas_args *a, void *stream);
int anoddpm_pro_auc(const anoddpm_pro_args *a, void *stream);
int64_t anoddpm_pro_workspace_bytes(int32_t S, int64_t n);   /* HOST function; -1 for S < 1, n < 1 or n >= 2^31 */

/* The same curve and AUPRO with every segment sorted and walked by the whole chip (csrc/pro_wide.hip): for one long segment -- a
 * whole test set pooled into one curve, which is how the score is defined -- where anoddpm_pro_auc keeps all but one compute unit
 * idle.  Like anoddpm_pro_auc it replaces no call of the reference, which has no counterpart.  Same argument struct, every field
 * with the meaning above (strides, shared mask, optional mask check, optional curve outputs); the S segments are processed one
 * after another on `stream`, each as a sequence of 18 launches with one workgroup per tile of `tile` elements, and share ONE
 * segment's workspace.  A launch boundary is the only ordering between workgroups; nothing allocates or synchronises, so the call
 * is capturable in a hipGraph.
 *   tile       elements per workgroup: a multiple of 256 from 256 up, or 0 for the library's choice, with the rules of
 *              anoddpm_roc_auc_wide: at most ANODDPM_ROC_WIDE_MAX_TILES tiles, an explicit tile that needs more is refused, tile
 *              0 is 4096 and grows with n so that every n < 2^31 is accepted
 *   workspace  [dev] anoddpm_pro_wide_workspace_bytes(S, n, tile) bytes, 16-byte aligned, whatever S is: with W = n rounded up
 *              to 64, 28 W bytes (keys and areas twice, the false-positive count and the fp64 PRO of every curve point; the fp64
 *              trapezoid terms lie in the key and area buffers the sort left free) + W / 4 bytes (two fp64 words per group of 64
 *              elements) + 1044 bytes per tile (the 256 counters of a sort pass and five words) + less than 1 KB; never
 *              smaller for a larger n at the same tile
 * H, W and planes_per_segment are read only through n = planes_per_segment * H * W, and region_counts only through the sum of
 * the segment's planes_per_segment entries: a caller that pools planes of several shapes passes planes_per_segment = 1, H = 1,
 * W = n and one entry that holds the number of regions.
 * For every accepted input every output has the bits anoddpm_pro_auc writes for the same arguments: aupro, counts, status,
 * curve_fps / curve_pro / curve_thr / curve_len, ANODDPM_ROC_CURVE_TRUNCATED, and the status word of a segment that breaks the
 * precondition (its other outputs stay not meaningful).  Argument checks as anoddpm_pro_auc, made before anything is launched. */
int anoddpm_pro_auc_wide(const anoddpm_pro_args *a, int32_t tile, void *stream);
int64_t anoddpm_pro_wide_workspace_bytes(int32_t S, int64_t n, int32_t tile);   /* HOST function; -1 where the call would be refused */

/* ------------------------------------------------------------------ distance transform and boundary distances of anomaly maps
 * The Hausdorff distance, its 95th-percentile form (HD95) and the average symmetric surface distance (ASSD): how far the
 * predicted outline lies from the true one, which no overlap score says.  The reference has no counterpart.  Pixel units, 2-D
 * planes, one threshold per call.  Every quantity is an integer squared distance or the fp64 square root of one.
 *
 * anoddpm_distance_transform: S planes of H x W fp32 at src + p * src_stride.  Foreground is value > level (NaN is background).
 *   sq[p][y][x]    int32: the squared Euclidean distance from (y, x) to the nearest background pixel of the same plane, exact;
 *                  0 on the background
 *   dist[p][y][x]  optional fp64: sqrt(sq), correctly rounded.  With at least one background pixel in the plane it equals
 *                  scipy.ndimage.distance_transform_edt(plane > level) bit for bit
 *   A plane without a background pixel has no defined answer (scipy measures to a virtual pixel at (-1, -1)): sq is -1 and
 *   dist is +inf everywhere in it.
 *   workspace      [dev] 4 * S * H * W bytes (a quarter of anoddpm_surface_workspace_bytes(S, H, W))
 *   Two launches: a sweep down and up every column, then per row the minimum over x' of (x - x')^2 + g(y, x')^2 in integers.
 *
 * anoddpm_surface_distance: S pairs of planes, pred at pred + s * pred_stride and ref at ref + s * ref_stride; ref_stride 0 =
 *   one reference plane shared by every prediction (its border and column distances are computed once).  With m = plane > level:
 *     border(m)  the pixels of m with at least one of the 4 neighbours background or outside the image
 *                = m & ~scipy.ndimage.binary_erosion(m, iterations=1, border_value=0)  (medpy's and DeepMind's surface)
 *     d_pr       for every pixel of border(pred) the distance to the nearest pixel of border(ref); d_rp the reverse
 *   counts[s]  {|border(pred)|, |border(ref)|}
 *   max2[s]    the largest SQUARED distance of d_pr and of d_rp (Hausdorff distance = sqrt(max(max2)))
 *   mean[s]    the mean of d_pr and of d_rp: the fp64 sum of the square roots divided by the count.  Order of the sum: thread t
 *              of 1024 adds the plane's border pixels t, t + 1024, ... (row-major pixel index) in that order, a halving tree
 *              folds the 64 partials of each wave (lane i + lane i+32, then +16, ... +1) and then the 16 wave sums the same way.
 *              ASSD = (mean[0] + mean[1]) / 2
 *   p95[s]     the 95th percentile of d_pr, of d_rp, and of the two pooled into one multiset (medpy's hd95).  For n sorted values
 *              v:  k = 19 (n - 1), lo = k div 20, r = k mod 20, hi = min(lo + 1, n - 1);  value = a + (b - a) * (r / 20) with
 *              a = sqrt(v[lo]), b = sqrt(v[hi]) in fp64, every operation rounded once (numpy.percentile(d, 95) within a few
 *              ulp).  v[lo] and v[hi] are selected exactly on the integer squared distances; sqrt is monotone.
 *   status[s]  ANODDPM_SURFACE_EMPTY_PRED: border(pred) is empty; ANODDPM_SURFACE_EMPTY_REF: border(ref) is empty.  When it is
 *              non-zero every fp64 output of the pair is NaN and both max2 are -1 (counts are still counts); no other pair is
 *              touched.
 *   workspace  [dev] anoddpm_surface_workspace_bytes(S, H, W) bytes
 *   Four launches whatever S; integer atomics only; no allocation, no host synchronisation; the same bits on every launch and
 *   wherever a pair sits in a batch.
 * Both need (H - 1)^2 + (W - 1)^2 < 2^31 (every squared distance fits int32), H * W < 2^31 and 2 * S * H * W < 2^31. */
#define ANODDPM_SURFACE_EMPTY_PRED 1
#define ANODDPM_SURFACE_EMPTY_REF 2

typedef struct anoddpm_distance_args {
    const float *src;               /* [dev] */
    int32_t *sq;                    /* [dev] [S][H][W] */
    double *dist;                   /* [dev] [S][H][W] or NULL */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    int64_t src_stride;
    int32_t S, H, W;
    float level;
} anoddpm_distance_args;

typedef struct anoddpm_surface_args {
    const float *pred;              /* [dev] */
    const float *ref;               /* [dev] */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    int32_t *counts;                /* [dev] [S][2] */
    int32_t *max2;                  /* [dev] [S][2] */
    double *mean;                   /* [dev] [S][2] */
    double *p95;                    /* [dev] [S][3] */
    int32_t *status;                /* [dev] [S] */
    int64_t pred_stride, ref_stride;
    int32_t S, H, W;
    float level;
} anoddpm_surface_args;

int anoddpm_distance_transform(const anoddpm_distance_args *a, void *stream);
int anoddpm_surface_distance(const anoddpm_surface_args *a, void *stream);
int64_t anoddpm_surface_workspace_bytes(int32_t S, int32_t H, int32_t W);   /* HOST function; -1 when the extents break the conditions above */

/* ------------------------------------------------------------------ distance transform and boundary distances of whole volumes
 * The two entry points above for D x H x W volumes in VOXEL units: one Hausdorff distance, one HD95 and one ASSD per volume, as
 * the protocols that report one Dice per volume report them (taking the planes one by one gives another answer: an outline on
 * slice z is often nearest to the other outline on slice z +- 1).  Every quantity is an integer squared distance or the fp64
 * square root of one, so what is said above about bits holds unchanged.
 *
 * anoddpm_distance_transform3d: S volumes of D x H x W fp32 at src + s * src_stride.  Foreground is value > level (NaN is
 *   background).
 *   sq[s][z][y][x]    int32: the squared Euclidean distance from (z, y, x) to the nearest background voxel of the same volume,
 *                     exact; 0 on the background
 *   dist[s][z][y][x]  optional fp64: sqrt(sq), correctly rounded.  With at least one background voxel in the volume it equals
 *                     scipy.ndimage.distance_transform_edt(vol > level) bit for bit (scipy's 3-D output is the square root of the
 *                     integer minimum)
 *   A volume without a background voxel gets sq = -1 and dist = +inf everywhere; no other volume of the batch is touched.
 *   workspace         [dev] 8 * S * D * H * W bytes: two buffers of squared distances, half of the 16 * S * D * H * W bytes that
 *                     lead anoddpm_surface3d_workspace_bytes(S, D, H, W)
 *   Three launches: the sweep along z (the column sweep of the plane transform over H * W columns), per (z, 64 columns) the
 *   minimum over y' of (y - y')^2 + g(z, y', x)^2 into the SECOND buffer (it reads whole y columns, so it never runs in place),
 *   and per row the minimum over x' as in the plane transform.  Integer adds and minima only.
 *
 * anoddpm_surface_distance3d: S pairs of volumes, pred at pred + s * pred_stride and ref at ref + s * ref_stride; ref_stride 0 =
 *   one reference volume shared by every prediction (its border and its z and y passes are computed once).  With m = vol > level:
 *     border(m)  the voxels of m with at least one of the 6 FACE neighbours background or outside the volume
 *                = m & ~scipy.ndimage.binary_erosion(m, iterations=1, border_value=0) on the 3-D array.
 *                D = 1 IS NOT THE PLANE CASE: both z neighbours lie outside the volume, so every foreground voxel is on the
 *                border (as scipy answers for a [1, H, W] array); anoddpm_surface_distance is the entry point for planes.
 *     d_pr       for every voxel of border(pred) the distance to the nearest voxel of border(ref); d_rp the reverse
 *   counts, max2, mean, p95, status: as anoddpm_surface_distance, with the same status bits and the same percentile (lo and hi
 *   are selected on the integer squared distances; only the two selected values get a square root).
 *   mean[s]    the fp64 sum of the square roots divided by the count, in THIS order: the border voxels of one direction are
 *              ranked by their linear voxel index (z * H + y) * W + x; thread t of 1024 adds sqrt(d^2) of the ranks t, t + 1024,
 *              ... in that order; the two halving trees of anoddpm_surface_distance fold the 1024 partials.  (The plane kernel
 *              strides over pixels, this one over ranks: no workgroup walks a whole volume.)
 *   workspace  [dev] anoddpm_surface3d_workspace_bytes(S, D, H, W) bytes = 16 * S * D * H * W (two buffers of 2 S volumes)
 *              + 16 * S * D * H (a count and an offset per pair, direction and row) + 8 * S (two totals per pair); 4-byte words
 *   Seven launches whatever S: border, z sweep, y pass, the x pass (which writes d^2 at the own border voxels and one count per
 *   row; rows without an own border voxel skip the search), a scan of the counts, a pack of every row's values to its offset in
 *   voxel order (direction 1 directly behind direction 0: the pooled multiset is one array), and one workgroup per pair over
 *   the packed list.  Integer atomics only; no allocation, no host synchronisation; the same bits on every launch, whatever
 *   the workspace held before and wherever a pair sits in a batch.
 * Both need D, H, W, S >= 1, D * H * W < 2^31, (D - 1)^2 + (H - 1)^2 + (W - 1)^2 < 2^31 (every squared distance fits int32) and
 * every grid below 2^31 workgroups (S * D * H rows; 2 * S * D * H for the surface call); S > 1 needs strides >= D * H * W
 * (ref_stride 0 excepted).  Indices are 64-bit.  Refused before anything is launched otherwise.
 * Still open: spacing in millimetres (the squared distances become rounded fp64 values and the equality with scipy needs a new
 * argument), 18- / 26-neighbour surfaces, several thresholds per call, and a chip-wide select for borders of many millions of
 * voxels (one workgroup per pair selects today). */
typedef struct anoddpm_distance3d_args {
    const float *src;               /* [dev] */
    int32_t *sq;                    /* [dev] [S][D][H][W] */
    double *dist;                   /* [dev] [S][D][H][W] or NULL */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    int64_t src_stride;
    int32_t S, D, H, W;
    float level;
} anoddpm_distance3d_args;

typedef struct anoddpm_surface3d_args {
    const float *pred;              /* [dev] */
    const float *ref;               /* [dev] */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    int32_t *counts;                /* [dev] [S][2] */
    int32_t *max2;                  /* [dev] [S][2] */
    double *mean;                   /* [dev] [S][2] */
    double *p95;                    /* [dev] [S][3] */
    int32_t *status;                /* [dev] [S] */
    int64_t pred_stride, ref_stride;
    int32_t S, D, H, W;
    float level;
} anoddpm_surface3d_args;

int anoddpm_distance_transform3d(const anoddpm_distance3d_args *a, void *stream);
int anoddpm_surface_distance3d(const anoddpm_surface3d_args *a, void *stream);
int64_t anoddpm_surface3d_workspace_bytes(int32_t S, int32_t D, int32_t H, int32_t W);   /* HOST function; -1 where the call would be refused */

/* ------------------------------------------------------------------ post-processing of anomaly maps before they are scored
 * The three steps published brain-MRI anomaly-segmentation pipelines apply between the squared error and AP / Dice (the
 * reference has no counterpart: it scores the raw map).  All three select or count, so each output equals scipy's bit for bit.
 * S planes of H x W fp32, plane p at src + p * src_stride (src_stride >= H*W); outputs are contiguous [S][H][W].
 *
 * anoddpm_median2d replaces scipy.ndimage.median_filter(plane, size=k) (default mode="reflect": d c b a | a b c d | d c b a),
 *   k in {3, 5, 7}, min(H, W) >= k: dst = the middle one of the k*k values of the window, selected, never averaged.
 *   Precondition as anoddpm_roc_auc: values finite and >= 0 (-0.0 is reported as +0.0); a plane that breaks it sets bits of
 *   status[p] (ANODDPM_ROC_NAN / _INF / _NEGATIVE) and its output is unspecified; no other plane is touched.
 *   roi     optional fp32 0/1 planes at roi + p * roi_stride (roi_stride 0 = one ROI for every plane): dst is +0.0 where the
 *           ROI is 0 (the filter itself sees the unmasked plane).  A value other than 0 / 1 sets ANODDPM_ROC_BAD_MASK.
 *   One launch (after an asynchronous clear of status): a workgroup stages a 16 x 32 tile and its k/2 halo in LDS; the grid is
 *   tiles x planes.
 *
 * anoddpm_erode2d replaces scipy.ndimage.binary_erosion(plane > level, iterations=n) with scipy's defaults (the 4-neighbour
 *   cross, border_value=0), 1 <= n <= 8: n passes of the cross are one pass of the L1 ball of radius n with everything outside
 *   the image counting as 0.  dst is fp32 0 / 1.  NaN is not above any level.  One launch, n-pixel LDS halo.
 *
 * anoddpm_small_components replaces  lab, m = scipy.ndimage.label(plane > level, structure);  sizes = numpy.bincount(lab.ravel());
 *   plane * (sizes >= min_size)[lab]  (with label 0 cleared): dst is fp32 0 / 1, the foreground without its connected
 *   components of fewer than min_size pixels.  connectivity 1: 4 neighbours (label's default structure), 2: 8 neighbours.
 *   counts[p] = {components found, components kept}.  Union-find on 32-bit labels in global memory: clear, link (atomic minimum
 *   on roots), flatten, sizes (atomic add at the root), filter -- five launches, and launch boundaries are the only ordering
 *   between workgroups.  The outputs are a set and two integers: independent of execution order, same bits every run.
 *   workspace  [dev] anoddpm_small_components_workspace_bytes(S, H, W) bytes = 8 per pixel (label and size words)
 * No allocation and no host synchronisation in any of them. */
typedef struct anoddpm_median_args {
    const float *src;               /* [dev] */
    const float *roi;               /* [dev] or NULL */
    float *dst;                     /* [dev] [S][H][W] */
    int32_t *status;                /* [dev] [S] */
    int64_t src_stride, roi_stride;
    int32_t S, H, W, k;
} anoddpm_median_args;

typedef struct anoddpm_erode_args {
    const float *src;               /* [dev] */
    float *dst;                     /* [dev] [S][H][W] */
    int64_t src_stride;
    int32_t S, H, W, n;
    float level;
} anoddpm_erode_args;

typedef struct anoddpm_components_args {
    const float *src;               /* [dev] */
    float *dst;                     /* [dev] [S][H][W] */
    int64_t *counts;                /* [dev] [S][2] */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    int64_t src_stride;
    int32_t S, H, W;
    int32_t min_size, connectivity;
    float level;
} anoddpm_components_args;

int anoddpm_median2d(const anoddpm_median_args *a, void *stream);
int anoddpm_erode2d(const anoddpm_erode_args *a, void *stream);
int anoddpm_small_components(const anoddpm_components_args *a, void *stream);
int64_t anoddpm_small_components_workspace_bytes(int32_t S, int32_t H, int32_t W);  /* HOST function; -1 for an extent < 1 or S*H*W >= 2^31 */

/* ------------------------------------------------------------------ volume-wise post-processing of anomaly maps
 * The same three steps on whole volumes, as the published brain-MRI protocols that report one Dice per volume apply them: the
 * residual volume is median-filtered, the brain mask eroded and small components dropped in 3-D.  The results are NOT those of
 * the plane-wise entry points above applied slice by slice.  All three select or count: every output equals scipy's bit for bit.
 * S volumes of D x H x W fp32, volume v at src + v * src_stride (src_stride >= D*H*W), slices and rows contiguous; outputs are
 * contiguous [S][D][H][W].  D >= 1: a single slice is a volume.
 *
 * anoddpm_median3d replaces scipy.ndimage.median_filter(vol, size=k) (mode="reflect" on all three axes), k in {3, 5},
 *   min(H, W) >= k as for anoddpm_median2d; along depth any D >= 1 is taken and the index is reflected as often as needed
 *   (period 2 D: ... b a | a b ... | ... b a | a b ..., what numpy.pad(mode="symmetric") does for a pad wider than the axis).
 *   dst = the (k*k*k / 2)-th smallest of the k*k*k values of the window, selected on the 31-bit pattern exactly as
 *   anoddpm_median2d selects (-0.0 is reported as +0.0).  Precondition and status bits as there, one status word per VOLUME.
 *   roi     optional fp32 0 / 1, voxel (v, z, y, x) at roi + v * roi_stride + z * roi_slice_stride + y * W + x:
 *           roi_slice_stride 0 and roi_stride 0: one plane for every slice of every volume; roi_slice_stride H*W and roi_stride
 *           0: one volume shared by the batch; roi_slice_stride H*W and roi_stride >= D*H*W: one per volume.  dst is +0.0 where
 *           the ROI is 0 (the filter itself sees the unmasked volume); a value other than 0 / 1 sets ANODDPM_ROC_BAD_MASK.
 *   One launch (after an asynchronous clear of status): a workgroup stages a 4 x 8 x 32 tile and its k/2 halo in LDS once; a
 *   thread walks the tile's four slices of one (y, x), keeps the k*k*k patterns in registers and replaces one k*k plane of them
 *   per step.  The grid is tiles x volumes, below 2^31 workgroups.
 *
 * anoddpm_erode3d replaces scipy.ndimage.binary_erosion(vol > level, iterations=n) with scipy's defaults (the 6-neighbour cross,
 *   border_value=0), 1 <= n <= 8: one AND over the L1 ball (octahedron) of radius n with everything outside the volume counting
 *   as 0.  dst is fp32 0 / 1.  NaN is not above any level.  One launch.
 *
 * anoddpm_small_components3d replaces  lab, m = scipy.ndimage.label(vol > level, scipy.ndimage.generate_binary_structure(3, c));
 *   sizes = numpy.bincount(lab.ravel());  (sizes >= min_size)[lab]  (with label 0 cleared): dst is fp32 0 / 1.  connectivity
 *   c = 1: 6 neighbours (label's default), 2: 18, 3: 26.  counts[v] = {components found, components kept} per volume.
 * anoddpm_component_areas3d: area = numpy.bincount(lab.ravel())[lab], 0 where lab == 0; counts[v] = m.
 *   Both are the five launches of anoddpm_small_components / anoddpm_component_areas with a link launch that visits the 3 / 9 /
 *   13 forward neighbours; components never link across volumes.
 *   workspace  [dev] anoddpm_components3d_workspace_bytes(S, D, H, W) bytes = 8 per voxel; S * D * H * W must be below 2^31
 * No allocation and no host synchronisation in any of them: capturable in a hipGraph. */
typedef struct anoddpm_median3d_args {
    const float *src;               /* [dev] */
    const float *roi;               /* [dev] or NULL */
    float *dst;                     /* [dev] [S][D][H][W] */
    int32_t *status;                /* [dev] [S] */
    int64_t src_stride, roi_stride, roi_slice_stride;
    int32_t S, D, H, W, k;
} anoddpm_median3d_args;

typedef struct anoddpm_erode3d_args {
    const float *src;               /* [dev] */
    float *dst;                     /* [dev] [S][D][H][W] */
    int64_t src_stride;
    int32_t S, D, H, W, n;
    float level;
} anoddpm_erode3d_args;

typedef struct anoddpm_components3d_args {
    const float *src;               /* [dev] */
    float *dst;                     /* [dev] [S][D][H][W] */
    int64_t *counts;                /* [dev] [S][2] */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    int64_t src_stride;
    int32_t S, D, H, W;
    int32_t min_size, connectivity;
    float level;
} anoddpm_components3d_args;

typedef struct anoddpm_component_areas3d_args {
    const float *src;               /* [dev] */
    int32_t *area;                  /* [dev] [S][D][H][W] */
    int64_t *counts;                /* [dev] [S] */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    int64_t src_stride;
    int32_t S, D, H, W;
    int32_t connectivity;
    float level;
} anoddpm_component_areas3d_args;

int anoddpm_median3d(const anoddpm_median3d_args *a, void *stream);
int anoddpm_erode3d(const anoddpm_erode3d_args *a, void *stream);
int anoddpm_small_components3d(const anoddpm_components3d_args *a, void *stream);
int anoddpm_component_areas3d(const anoddpm_component_areas3d_args *a, void *stream);
int64_t anoddpm_components3d_workspace_bytes(int32_t S, int32_t D, int32_t H, int32_t W);  /* HOST function; -1 for an extent < 1 or S*D*H*W >= 2^31 */

/* ------------------------------------------------------------------ Gaussian smoothing and image-level scores of anomaly maps
 * The two steps the texture protocol (Bergmann et al., MVTec AD) puts between an anomaly map and its scores; the reference has
 * no counterpart.
 *
 * anoddpm_gauss2d replaces scipy.ndimage.gaussian_filter(plane, sigma, truncate=truncate) with scipy's defaults (order 0,
 *   mode="reflect": d c b a | a b c d | d c b a, the same sigma on both axes, fp32 in, fp32 out) on S planes of H x W fp32, plane p
 *   at src + p * src_stride (src_stride >= H*W); dst is contiguous [S][H][W].  Bit for bit scipy's for finite inputs:
 *     w       [dev] radius + 1 fp64 weights, w[0] the outermost tap and w[radius] the centre: with r = int(truncate * sigma + 0.5),
 *             x = -r ... 0:  exp(-0.5 / sigma^2 * x^2) / (sum over all 2 r + 1 taps), as numpy computes them in fp64.  The kernel
 *             only reads them.
 *     axis 0  (along H) first:  acc = v[i] * w[r];  for j = -r ... -1 in that order:  acc += (v[i+j] + v[i-j]) * w[r+j];  v is the
 *             line as fp64, no fused multiply-add; the result is ROUNDED TO fp32.  Axis 1 the same on that result.
 *     border  index i of a line of n:  m = i mod 2n (non-negative);  m >= n -> 2n - 1 - m.  A plane narrower than the radius
 *             reflects several times; min(H, W) > radius is NOT required.
 *   Preconditions: 1 <= radius <= ANODDPM_GAUSS_MAX_RADIUS, S, H, W >= 1, S * tiles below 2^31, dst does not overlap src.  A
 *   non-finite input propagates by IEEE rules within its radius (no status word); no other plane is touched.
 *   One launch: a workgroup of 256 threads stages a 32 x 32 tile and its radius halo in LDS with the border resolved, runs the
 *   axis-0 pass into an fp32 LDS buffer (that buffer is the rounding between the axes) and the axis-1 pass from it; the grid is
 *   tiles x planes.  LDS: ((32 + 2r)^2 + 32 (32 + 2r)) * 4 + 264 bytes, 49416 at radius 32.
 *
 * anoddpm_map_scores: one score per image.  S segments of n contiguous fp32 values (one image, all its channels pooled) at
 *   src + s * src_stride, and 1 <= k <= n:
 *     max[s]        fp32, the largest value
 *     mean[s]       fp64, sum / n
 *     topk_mean[s]  fp64, the mean of the k largest values as a multiset:  v_k, the k-th largest, is SELECTED on the bit pattern
 *                   (radix select, integer atomics only);  (sum over v > v_k of v  +  (k - #{v > v_k}) * v_k) / k
 *     status[s]     precondition as anoddpm_roc_auc: values finite and >= 0 (-0.0 counts as +0.0); a segment that breaks it sets
 *                   ANODDPM_ROC_NAN / _INF / _NEGATIVE and its other outputs are unspecified; no other segment is touched.
 *   Both sums are fp64 in a fixed order: thread t of 1024 adds the elements t, t + 1024, ... in that order, a halving tree folds
 *   the 64 partials of a wave (lane i + lane i+32, then +16, ... +1) and then the 16 wave sums the same way -- the same input
 *   gives the same bits.  One launch, one workgroup per segment: n <= ANODDPM_MAP_SCORES_MAX_N (64 maps of 512 x 512), above it
 *   the call is refused.
 * No allocation and no host synchronisation in either. */
#define ANODDPM_GAUSS_MAX_RADIUS 32
#define ANODDPM_MAP_SCORES_MAX_N 16777216
typedef struct anoddpm_gauss_args {
    const float *src;               /* [dev] */
    float *dst;                     /* [dev] [S][H][W] */
    const double *w;                /* [dev] [radius + 1] */
    int64_t src_stride;
    int32_t S, H, W, radius;
} anoddpm_gauss_args;

typedef struct anoddpm_map_scores_args {
    const float *src;               /* [dev] */
    float *max;                     /* [dev] [S] */
    double *mean;                   /* [dev] [S] */
    double *topk_mean;              /* [dev] [S] */
    int32_t *status;                /* [dev] [S] */
    int64_t src_stride, n, k;
    int32_t S;
} anoddpm_map_scores_args;

int anoddpm_gauss2d(const anoddpm_gauss_args *a, void *stream);
int anoddpm_map_scores(const anoddpm_map_scores_args *a, void *stream);

/* ------------------------------------------------------------------ Gaussian smoothing of whole volumes
 * The smoothing the volume-wise protocols apply before the median, the cut and the distances; the reference has no counterpart.
 * csrc/gauss3d.hip.
 *
 * anoddpm_gauss3d replaces scipy.ndimage.gaussian_filter(vol, (sz, sy, sx), truncate=t) with scipy's defaults (order 0,
 *   mode="reflect", fp32 in, fp32 out) on S volumes of D x H x W fp32, volume v at src + v * src_stride (src_stride >= D*H*W, the
 *   slices of a volume contiguous); dst is contiguous [S][D][H][W].  Bit for bit scipy's for finite inputs:
 *     rz, ry, rx   the radius int(t * sigma + 0.5) of each axis, 0 ... ANODDPM_GAUSS_MAX_RADIUS.  An axis of radius 0 is SKIPPED
 *                  (scipy skips it for sigma <= 1e-15 and otherwise applies the one-tap kernel [1.0], the identity on fp32).
 *     wz, wy, wx   [dev] the taps of each axis in anoddpm_gauss2d's format: radius + 1 fp64 values, the outermost first, the centre
 *                  last.  The kernel only reads them; the table of an axis of radius 0 is not read and may be NULL.
 *     order        the axes run in scipy's order: D, then H, then W.
 *     a line       anoddpm_gauss2d's statement:  acc = v[i] * w[r];  for j = -r ... -1 in that order:  acc += (v[i+j] + v[i-j]) *
 *                  w[r+j];  v is the line as fp64, every product and sum rounded once, no fused multiply-add; the result is
 *                  ROUNDED TO fp32 AFTER EACH AXIS.
 *     border       index i of a line of n:  m = i mod 2n (non-negative);  m >= n -> 2n - 1 - m, as often as it takes: D = 1 and
 *                  D < rz are legal (as are H, W below their radii).
 *     tmp          [dev] fp32 workspace of S*D*H*W elements: the volumes after the z pass.  Needed only when two launches run (rz
 *                  > 0 and ry or rx > 0); NULL is accepted otherwise.
 *   Launches: one separable tile kernel, a workgroup of 256 threads on a 32 x 32 tile of a plane with independent radii (r0, r1)
 *   per axis, either of which may be 0 --
 *     1. the S planes of D x (H*W), radii (rz, 0), src -> tmp: the z pass of a volume IS the axis-0 pass of that plane, and the
 *        fp32 store is scipy's rounding between axis 0 and axis 1;
 *     2. the S*D planes of H x W, radii (ry, rx), tmp -> dst (anoddpm_gauss2d's structure).
 *   With rz == 0 only launch 2 runs, with ry == rx == 0 only launch 1; either goes src -> dst.  LDS per workgroup:
 *   ((32 + 2 r0)(32 + 2 r1) + 32 (32 + 2 r1)) * 4 + 528 bytes, 49680 at radius 32 on both axes.
 *   Refused before anything is launched: a NULL pointer where one is needed, rz == ry == rx == 0, a radius outside 0 ... 32, an
 *   extent below 1, S*D*H*W >= 2^31, src_stride < D*H*W with S > 1, dst or tmp overlapping src, tmp overlapping dst.
 *   A non-finite input spreads by IEEE rules within the radii (no status word); no other volume is touched.  No allocation and no
 *   host synchronisation; capturable. */
typedef struct anoddpm_gauss3d_args {
    const float *src;               /* [dev] */
    float *dst;                     /* [dev] [S][D][H][W] */
    float *tmp;                     /* [dev] [S][D][H][W], or NULL when one launch runs */
    const double *wz, *wy, *wx;     /* [dev] [radius + 1] each */
    int64_t src_stride;
    int32_t S, D, H, W;
    int32_t rz, ry, rx;
} anoddpm_gauss3d_args;

int anoddpm_gauss3d(const anoddpm_gauss3d_args *a, void *stream);

/* ------------------------------------------------------------------ operating thresholds from a pooled segment, scores at them
 * The evaluation protocol of unsupervised anomaly segmentation (the reference has no counterpart: it cuts every map at 0.5): the
 * operating threshold is the value that a chosen share of the pixels of a HEALTHY validation set exceeds, and the test maps are
 * scored at it.  csrc/select_wide.hip.
 *
 * anoddpm_select_wide: order statistics of S segments of n contiguous fp32 values at src + s * src_stride, 1 <= n < 2^31, each
 *   selected by the whole chip; the S segments are processed one after another on `stream` and share ONE segment's workspace.
 *     ranks       [dev] Q uint32 ranks, 1 <= Q <= ANODDPM_SELECT_MAX_RANKS, one table for all segments; the kernels only read it.
 *                 Rank r is the 0-based position from the top: 0 is the maximum, k - 1 is anoddpm_map_scores' v_k.  Ranks may
 *                 repeat.  Every rank must be below n:
 *     ranks_host  [host] the same Q ranks, or NULL.  Given, a rank >= n is refused before anything is launched.  NULL, such a
 *                 rank sets ANODDPM_SELECT_BAD_RANK in status[s] and leaves value / above / equal / topk_mean of THAT rank
 *                 unspecified; nothing is read or written outside the buffers either way.
 *     value[s][q]      fp32, the value of descending rank r_q, SELECTED on the 31-bit pattern (sign dropped: -0.0 is +0.0)
 *     above[s][q]      int64, #{v > value};  equal[s][q]  int64, #{v == value}.   above <= r_q < above + equal
 *     topk_mean[s][q]  fp64, with k = r_q + 1:  (sum over v > value of v  +  (k - above) * value) / k
 *     max[s]  fp32,  mean[s]  fp64 sum / n,  status[s]: ANODDPM_ROC_NAN / _INF / _NEGATIVE as anoddpm_map_scores (the other
 *                 outputs of such a segment are unspecified; no other segment is touched), and ANODDPM_SELECT_BAD_RANK
 *   Order of additions: anoddpm_map_scores', continued beyond its limit -- virtual thread t of 1024 adds the elements t, t + 1024,
 *   ... in that order, a halving tree folds the 64 partials of a wave and then the 16 wave sums.  So for n <=
 *   ANODDPM_MAP_SCORES_MAX_N and Q = 1 every output shared with anoddpm_map_scores has the bits it writes for k = r + 1.
 *   Launches, 11 per segment whatever Q is: a clear; four times a histogram launch with one workgroup per tile (for every rank the
 *   256 bins of the pass's byte among the values that match the rank's prefix, LDS integer atomics, then integer adds into a
 *   [Q][256] table) and a one-workgroup launch that picks every rank's bin; the sums, 16 workgroups that are the 16 waves of the
 *   order above and read the segment in place; a one-workgroup finish.  Counts, status bits and the maximum cross workgroups as
 *   integers only; a launch boundary is the only ordering between workgroups.
 *     tile        values per workgroup of the histogram launches: any multiple of 256, or 0 for the library's choice -- n / 2048
 *                 rounded up to a multiple of 256, at least 1024 and at most 16384.  There is no cap on the tile count (at most
 *                 2^23 workgroups), so every n < 2^31 is accepted at every tile.
 *     workspace   [dev] anoddpm_select_wide_workspace_bytes(n, Q, tile) bytes, 16-byte aligned: four [Q][256] counter tables,
 *                 Q state records and (Q + 1) x 16 wave sums -- 4240 Q + 144 bytes, whatever n and S are.
 *   Refused before anything is launched: null pointers, S < 1, n outside 1 ... 2^31 - 1, Q outside 1 ... 16, a tile that is
 *   negative or no multiple of 256, src_stride < n with S > 1, a workspace too small or misaligned, a rank >= n in ranks_host.
 *
 * anoddpm_threshold_counts: S score segments of n fp32 values (score_stride) against a 0 / 1 fp32 mask (mask_stride, 0 = one
 *   mask for every segment) at T thresholds read from DEVICE memory, 1 <= T <= ANODDPM_THRESHOLD_COUNTS_MAX: thr + s * thr_stride,
 *   thr_stride 0 = one table for every segment, else >= T.  The prediction at threshold j is score > thr[j] -- strict, as
 *   detection.py:232: a score equal to the threshold is not predicted, nor is a NaN score.
 *     counts[s][j]  int64 {tp, fp}: predicted pixels with mask != 0 / with mask == 0
 *     totals[s]     int64 {P, N}: pixels with mask != 0 / with mask == 0
 *     status[s]     ANODDPM_ROC_BAD_MASK (a mask value other than 0 and 1), ANODDPM_ROC_NAN (a NaN score)
 *   All counts are exact.  Two launches: a clear of the outputs, then ONE pass over the data whatever T is, grid segments x tiles
 *   of 4096 values; counts are reduced per wave and per workgroup and added to the outputs as integers.  1 <= n < 2^31, S * tiles
 *   below 2^31.
 * No allocation and no host synchronisation in either: both are legal inside stream capture. */
#define ANODDPM_SELECT_MAX_RANKS 16
#define ANODDPM_SELECT_BAD_RANK 32
#define ANODDPM_THRESHOLD_COUNTS_MAX 16
typedef struct anoddpm_select_args {
    const float *src;               /* [dev] */
    const uint32_t *ranks;          /* [dev] [Q] */
    const uint32_t *ranks_host;     /* [host] [Q] or NULL */
    void *workspace;                /* [dev] */
    int64_t workspace_bytes;
    float *value;                   /* [dev] [S][Q] */
    int64_t *above, *equal;         /* [dev] [S][Q] */
    double *topk_mean;              /* [dev] [S][Q] */
    float *max;                     /* [dev] [S] */
    double *mean;                   /* [dev] [S] */
    int32_t *status;                /* [dev] [S] */
    int64_t src_stride, n;
    int32_t S, Q;
} anoddpm_select_args;

typedef struct anoddpm_threshold_counts_args {
    const float *score;             /* [dev] */
    const float *mask;              /* [dev] */
    const float *thr;               /* [dev] [T], or [S] tables thr_stride apart */
    int64_t *counts;                /* [dev] [S][T][2] */
    int64_t *totals;                /* [dev] [S][2] */
    int32_t *status;                /* [dev] [S] */
    int64_t n, score_stride, mask_stride, thr_stride;
    int32_t S, T;
} anoddpm_threshold_counts_args;

int anoddpm_select_wide(const anoddpm_select_args *a, int32_t tile, void *stream);
int64_t anoddpm_select_wide_workspace_bytes(int64_t n, int32_t Q, int32_t tile);   /* HOST function; -1 where the call would be refused */
int anoddpm_threshold_counts(const anoddpm_threshold_counts_args *a, void *stream);

/* Variational-bound terms of one reverse step (GaussianDiffusion.py:384-397 calc_vlb_xt, and the two MSE curves of
 * calc_total_vlb :445-478): per sample b
 *   out[0*B + b] = mean_flat( t==0 ? -discretised_gaussian_log_likelihood(x_0; mean, 0.5*logvar)
 *                                  : normal_kl(true_mean, post_logvar, mean, model_logvar) ) / ln 2
 *   out[1*B + b] = mean_flat((pred_x_0 - x_0)^2)
 *   out[2*B + b] = mean_flat((predict_eps_from_x_0(x_t, t, pred_x_0) - noise)^2)        (0 when noise == NULL)
 * with pred_x_0 = clamp(c_recip[t]*x_t - c_recipm1[t]*eps, -1, 1) and mean = c_coef1[t]*pred_x_0 + c_coef2[t]*x_t.
 * Tables are fp32 copies of the reference's fp64 tables (sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod,
 * posterior_mean_coef1/2, posterior_log_variance_clipped, log(append(posterior_variance[1], betas[1:]))).
 * workspace: >= 64 * B * 3 doubles [dev].  Deterministic. */
typedef struct anoddpm_vlb_args {
    const float *x0, *xt, *eps, *noise;
    const int64_t *t;
    const float *c_recip, *c_recipm1, *c_coef1, *c_coef2, *c_post_logvar, *c_model_logvar;
    float *pred_x0;                 /* optional [B][n] */
    float *out;                     /* [3][B] */
    double *workspace;
    int64_t workspace_doubles;
    int64_t n;
    int32_t B, T;
} anoddpm_vlb_args;

int anoddpm_vlb_terms(const anoddpm_vlb_args *a, void *stream);

/* Training loss of one batch and its gradient (GaussianDiffusion.py:399-417 calc_loss, :419-434 p_loss; the hybrid loss's
 * VLB term is calc_vlb_xt :384-397):
 *   kind 0 (l1):  per_sample[b] = mean_flat(|eps - noise|)
 *   kind 1 (l2):  per_sample[b] = mean_flat((eps - noise)^2)
 *   kind 2 (hybrid): vlb[b] as anoddpm_vlb_terms' out[0]; per_sample[b] = vlb[b] + mean_flat((eps - noise)^2)
 *   total[0] = mean_b(per_sample[b] * weights[b])                          (weights NULL = 1: loss_weight "none")
 * anoddpm_loss_backward writes d_eps[b][i] = d( sum_b g_per[b] per_sample[b] + sum_b g_vlb[b] vlb[b] + g_total total ) / d eps[b][i]
 * (each upstream gradient may be NULL = 0) -- the tensor loss.backward() hands to the UNet's backward.
 * Element math fp32, per-sample sums fp64 folded in a fixed order (deterministic).  workspace: >= 64 * B * 2 doubles [dev]. */
typedef struct anoddpm_loss_args {
    const float *eps, *noise;       /* [B][n] */
    const float *x0, *xt;           /* [B][n], hybrid only */
    const int64_t *t;               /* [B], hybrid only */
    const float *weights;           /* [B] or NULL */
    const float *c_recip, *c_recipm1, *c_coef1, *c_coef2, *c_post_logvar, *c_model_logvar;   /* fp32[T], hybrid only */
    float *per_sample;              /* [B] */
    float *vlb;                     /* [B] or NULL */
    float *total;                   /* [1] or NULL */
    double *workspace;
    int64_t workspace_doubles;
    const float *g_per, *g_vlb, *g_total;   /* backward: upstream gradients [B], [B], [1]; each may be NULL */
    float *d_eps;                   /* backward: [B][n] */
    int64_t n;
    int32_t B, T, kind;
} anoddpm_loss_args;

int anoddpm_loss_forward(const anoddpm_loss_args *a, void *stream);
int anoddpm_loss_backward(const anoddpm_loss_args *a, void *stream);

/* nn.Dropout(p) of ResBlock.out_layers (UNet.py:192: GroupNorm32 -> SiLU -> Dropout -> conv) in training mode.  The mask is a
 * counter-based hash of (seed, element index): the same (seed, index) gives the same mask in the forward and the backward launch,
 * no mask tensor exists.  keep probability 1 - p, kept values scaled by 1 / (1 - p) (torch semantics; the random STREAM is this
 * library's own -- no implementation reproduces torch's philox offsets, parity tests inject the mask they read back).
 *   mode 0 (forward):  out[b][i] = keep ? silu(x[b][i] * gn_scale[b][c] + gn_shift[b][c]) / (1 - p) : 0      (c = i % C)
 *   mode 1 (backward): out[b][i] = keep ? x[b][i] / (1 - p) : 0                                             (x = d(out), may alias out)
 * x, out: NHWC [B][n]; n = pixels * C. */
typedef struct anoddpm_dropout_args {
    const float *x;
    float *out;
    const float *gn_scale, *gn_shift;   /* [B][C], mode 0 */
    int64_t n;                      /* elements per image */
    uint64_t seed;
    int32_t B, C, mode;
    float p;
} anoddpm_dropout_args;

int anoddpm_dropout(const anoddpm_dropout_args *a, void *stream);

/* ------------------------------------------------------------------ backward twins (training, diffusion_training.py:102)
 * Weight gradient of a 3x3 / stride 1 / pad 1 convolution whose input the forward consumed through the fused operand
 * load of anoddpm_igemm (GroupNorm-apply + SiLU, nearest x2, two-source concat):
 *   dw[co][ci][ky][kx] (OIHW) = sum_{b,y,x} dy[b][y][x][co] * A[b][y+ky-1][x+kx-1][ci]
 * The data gradient needs no entry point of its own: it is anoddpm_igemm on dy with the spatially flipped,
 * channel-transposed weights.  ws: [B * (W/TW) * ceil(H/band)][9][K][N] floats (TW = the largest of 32, 16, 8, 4, 2 dividing W);
 * the partial tiles are folded in a fixed order (deterministic).  accumulate != 0 adds into dw. */
typedef struct anoddpm_wgrad_args {
    const float *a0, *a1;           /* the conv's input sources (NHWC), a1 NULL when single source */
    const float *gn_scale, *gn_shift; /* [B][gn_ld] per-sample per-channel affine or NULL */
    const float *dy;                /* [B][H*W][dy_ld] gradient w.r.t. the conv output */
    float *dw;                      /* [N][K][3][3] */
    float *ws;
    int64_t ws_floats;
    int64_t a0_bs, a1_bs, dy_bs;    /* batch strides (floats) */
    int32_t c0, c1, a0_ld, a1_ld, dy_ld;
    int32_t H, W;                   /* OUTPUT image dims */
    int32_t N, B;
    int32_t a_mode;                 /* 0 same-res, 1 source is half-res (nearest x2), 2 source is double-res (2x2 average) */
    int32_t act;                    /* 1: SiLU after the affine */
    int32_t gn_ld;
    int32_t band;                   /* image rows per work item (split-K granularity) */
    int32_t accumulate;
    float *colsum;                  /* optional [items][N]: per work item sum over its pixels of dy (items of one image are
                                       consecutive: item = (b * nband + band) * nseg + segment) -> bias / embedding gradients */
    int32_t algo;                   /* 0: direct (nine-tap MFMA tiles, any shape above); 1: Winograd F(4x4,3x3) domain (wgrad43.hip),
                                       the adjoint of the cfg-3 forward kernel: dU = sum_tiles V (.) Z, dg = G^T dU G -- needs
                                       gn + act == 1, a_mode 0 / 1, H % 8 == 0, W % 16 == 0, K % 32 == 0, N % 64 == 0,
                                       c0 % 16 == 0, B <= 15; ws: anoddpm_wgrad43_groups(...) * 9 * K * N floats; colsum:
                                       [B][anoddpm_wgrad43_colsum_items(...)][N], one row per workgroup set and tile row (the
                                       kernel sums over its patches of an image); `band` is ignored */
    float *dimg, *dbias;            /* algo 1 only, optional (need colsum): dimg[B][N] = per-image sums of dy (embedding gradient),
                                       dbias[N] += their sum over the images -- anoddpm_colsum_fold done by N / 32 extra
                                       workgroups of the fold launch instead of a launch of its own (round 6) */
} anoddpm_wgrad_args;

int anoddpm_conv3x3_wgrad(const anoddpm_wgrad_args *a, void *stream);
int anoddpm_wgrad43_groups(int32_t K, int32_t N, int32_t B, int32_t H, int32_t W);   /* workgroup sets (workspace slabs) of algo 1 */
int anoddpm_wgrad43_colsum_items(int32_t K, int32_t N, int32_t B, int32_t H, int32_t W);   /* column-sum rows per image of algo 1 */

/* Device-side weight packing for the 3x3 kernels (training re-packs after every optimizer step).  w: OIHW [N][K][3][3].
 * mode 0: direct layout [9][I/4][O][4]; mode 1: Winograd F(2x2,3x3) U = G g G^T as [16][I/4][O][4]; mode 2: Winograd
 * F(4x4,3x3) as [36][I/4][O][4].  bwd != 0 packs the
 * data-gradient weights W'[o=k][i=n][a][b] = w[n][k][2-a][2-b] (I = N, O = K), else I = K, O = N. */
int anoddpm_pack_conv3x3(const float *w, float *out, int32_t N, int32_t K, int32_t mode, int32_t bwd, void *stream);

/* Backward of a = SiLU(GroupNorm32(x)) (UNet.py:170-171,190-191,409-411; act == 0: GroupNorm alone, UNet.py:113) as the
 * fused operand load of anoddpm_igemm consumed it, over up to two concatenated NHWC sources:
 *   y = gamma*xhat + beta, xhat = (x - mean)*rstd;   dy = da * silu'(y);
 *   dgamma[c] += sum_{b,p} dy*xhat;   dbeta[c] += sum_{b,p} dy;
 *   dx = rstd * (gamma*dy - mean_g(gamma*dy) - xhat * mean_g(gamma*dy*xhat))          (means over the group, per image)
 * `da` is the gradient w.r.t. the tensor the conv read: with a_mode 1 (forward nearest-x2 of a) it is at twice the
 * source resolution and the four children are summed; with a_mode 2 (forward 2x2 average) it is at half resolution and
 * each source pixel takes a quarter of its parent.  dx0 / dx1 receive the gradient w.r.t. the sources (acc_dx != 0:
 * added to what is there -- gradient fan-in of skip connections and residuals).  Three launches: per-channel partial
 * sums (deterministic two-stage fp64 fold), then the elementwise pass.
 * partial: double[B][nslab][C][2]; coef: float[B][C][4] scratch. */
typedef struct anoddpm_gn_bwd_args {
    const float *x0, *x1;           /* forward sources (x1 NULL when single) */
    const float *da;                /* [B][Pa][C] with row length da_ld */
    const float *gamma, *beta;      /* [C] */
    const float *mean, *rstd;       /* [B][groups] from anoddpm_gn_finalize */
    float *dx0, *dx1;
    float *dgamma, *dbeta;          /* [C], accumulated into */
    double *partial;
    float *coef;
    int64_t x0_bs, x1_bs, da_bs, dx0_bs, dx1_bs;
    int32_t c0, c1, x0_ld, x1_ld, da_ld, dx0_ld, dx1_ld;
    int32_t Hs, Ws;                 /* SOURCE image dims (P = Hs*Ws) */
    int32_t B, groups, nslab;
    int32_t act, a_mode;
    int32_t acc_dx;                 /* bit 0: add into dx0, bit 1: add into dx1 (else overwrite) */
    const float *dres;              /* optional [B][P][C] (row length dres_ld, batch stride dres_bs): added to the source
                                       gradient -- the identity residual of a block (UNet.py:216 / :125) */
    int64_t dres_bs;
    int32_t dres_ld;
    int32_t partial_ready;          /* 1: `partial` was written by the producer of da (anoddpm_igemm_args.gnb_partial): no reduction launch */
} anoddpm_gn_bwd_args;

int anoddpm_gn_silu_backward(const anoddpm_gn_bwd_args *a, void *stream);

/* Weight gradient of a pointwise (1x1 / Conv1d k=1) convolution (UNet.py:115,117,200) whose input was consumed through
 * the fused operand load (optional GroupNorm-apply, optional SiLU, two-source concat):
 *   dw[n][k] (+)= sum_{b,p} dy[b][p][n] * A[b][p][k]            dbias[n] += sum_{b,p} dy[b][p][n]
 * Contraction over pixels on the fp32 matrix pipe: a workgroup owns a 128 x 128 (k, n) tile of one work item
 * (image, `span` consecutive pixels); partial tiles go to ws[item][K][N] and are folded in a fixed order.
 * ws: >= (B * ceil(P/span)) * (K*N + N) floats. */
typedef struct anoddpm_wgrad1_args {
    const float *a0, *a1;
    const float *gn_scale, *gn_shift; /* [B][gn_ld] or NULL */
    const float *dy;                /* [B][P][dy_ld] */
    float *dw;                      /* [N][K] */
    float *dbias;                   /* [N], accumulated into; or NULL */
    float *ws;
    int64_t ws_floats;
    int64_t a0_bs, a1_bs, dy_bs;
    int32_t c0, c1, a0_ld, a1_ld, dy_ld;
    int32_t P, N, B;
    int32_t act, gn_ld;
    int32_t span;                   /* pixels per work item, multiple of 32 */
    int32_t accumulate;             /* != 0: add into dw */
} anoddpm_wgrad1_args;

int anoddpm_wgrad_pointwise(const anoddpm_wgrad1_args *a, void *stream);

/* Device-side weight packing (training re-packs after every optimizer step).
 *   kind 0: 3x3 direct   (anoddpm_pack_conv3x3 mode 0)       w OIHW [N][K][3][3]
 *   kind 1: 3x3 Winograd (anoddpm_pack_conv3x3 mode 1)
 *   kind 2: pointwise    w [N][K] -> [K/4][N][4]; bwd != 0: the data-gradient matrix W'[i=n][o] = w[n][k0 + o],
 *           o < kc, packed [N/4][kc][4] (a column range: the two sources of a concatenated input get separate matrices)
 *   kind 3: small conv   w OIHW [N][K][3][3] -> [9][K][N] (stem / head kernels)
 *   kind 4: plain copy of N*K floats
 *   kind 5: 3x3 Winograd F(4x4,3x3) (anoddpm_pack_conv3x3 mode 2): [36][I/4][O][4] */
typedef struct anoddpm_pack_args {
    const float *w;
    float *out;
    int32_t N, K, kind, bwd, k0, kc;
} anoddpm_pack_args;

int anoddpm_pack_weights(const anoddpm_pack_args *a, void *stream);

/* All pack jobs of a model in one launch: `jobs` is a DEVICE array of njobs anoddpm_pack_args (each validated on the host the way
 * anoddpm_pack_weights does), `block0` a DEVICE array of njobs + 1 prefix sums of anoddpm_pack_job_blocks(job) (256-thread blocks),
 * nblocks = block0[njobs]. */
typedef struct anoddpm_pack_batch_args {
    const anoddpm_pack_args *jobs;
    const int32_t *block0;
    int32_t njobs, nblocks;
} anoddpm_pack_batch_args;

int anoddpm_pack_batch(const anoddpm_pack_batch_args *b, void *stream);
int64_t anoddpm_pack_job_blocks(const anoddpm_pack_args *a);

/* Backward of the row softmax (UNet.py:151), in place on the incoming gradient:
 *   ds[r][j] = p[r][j] * (dp[r][j] - sum_j dp[r][j] p[r][j]) */
typedef struct anoddpm_softmax_bwd_args {
    const float *p;                 /* softmax output [rows][L] */
    float *dp;                      /* in: dL/dp, out: dL/ds */
    int64_t rows;
    int32_t L;
} anoddpm_softmax_bwd_args;

int anoddpm_softmax_rows_backward(const anoddpm_softmax_bwd_args *a, void *stream);

/* out[z][j][i] = in[z][i][j] for Z square L x L matrices (attention weights / their gradients, so that every
 * backward contraction of QKVAttention reads its A operand row-major). */
typedef struct anoddpm_transpose_args {
    const float *in;
    float *out;
    int32_t Z, L;
} anoddpm_transpose_args;

int anoddpm_transpose_square(const anoddpm_transpose_args *a, void *stream);

/* Backward of anoddpm_linear_small with act_out == 0: y = act_in(x) W^T + b.
 *   dw[n][k] (+)= sum_b dy[b][n] * act_in(x[b][k]);  db[n] (+)= sum_b dy[b][n];
 *   dx[b][k] (+)= act_in'(x[b][k]) * sum_n dy[b][n] * w[n][k]            (dx may be NULL) */
typedef struct anoddpm_linear_bwd_args {
    const float *x;                 /* [B][K] the forward INPUT (before act_in) */
    const float *w;                 /* [N][K] */
    const float *dy;                /* [B][N] */
    float *dw, *db, *dx;
    int32_t B, K, N, act_in;
    int32_t acc_w, acc_x;           /* != 0: add into dw+db / dx */
} anoddpm_linear_bwd_args;

int anoddpm_linear_small_backward(const anoddpm_linear_bwd_args *a, void *stream);

/* The same for njobs linear layers that share the input x (the per-block embedding projections, UNet.py:185-188, 213: one launch in
 * the forward): `jobs` is a DEVICE array of anoddpm_linear_bwd_args of which w, dy, dw, db and N are read; x, B, K, act_in, acc_w
 * come from this header.  dx (or NULL) receives act_in'(x) * sum over the jobs, folded in job order through ws [njobs][B][K]. */
typedef struct anoddpm_linear_bwd_batch_args {
    const anoddpm_linear_bwd_args *jobs;
    const float *x;
    float *dx;
    float *ws;
    int32_t njobs, max_n;           /* max_n: the largest N among the jobs */
    int32_t B, K, act_in, acc_w, acc_x;
} anoddpm_linear_bwd_batch_args;

int anoddpm_linear_small_backward_batch(const anoddpm_linear_bwd_batch_args *h, void *stream);

/* Backward of anoddpm_conv_stem (UNet.py:280): dw (OIHW [Cout][Cin][3][3]) += x (*) dy, db[co] += sum dy, and optionally
 * dx (NCHW) = dy (*) flipped w.  ws: >= nblk * (Cin * 9 + 1) * Cout floats with nblk = B * ceil(H*W / 1024). */
typedef struct anoddpm_stem_bwd_args {
    const float *x;                 /* [B][Cin][H][W] */
    const float *w;                 /* OIHW (the parameter itself) */
    const float *dy;                /* [B][H*W][Cout] */
    float *dw, *db;                 /* accumulated into */
    float *dx;                      /* [B][Cin][H][W] or NULL (overwritten) */
    float *ws;
    int64_t ws_floats;
    int32_t B, H, W, Cin, Cout;
} anoddpm_stem_bwd_args;

int anoddpm_conv_stem_backward(const anoddpm_stem_bwd_args *a, void *stream);

/* Backward of anoddpm_conv_head (UNet.py:384-388) up to the activated tensor a = silu(scale*x + shift):
 *   da[b][p][c] = sum_{o,tap} w[o][c][tap] * dy[b][o][p - off(tap)]           (NHWC, overwritten)
 *   dw[o][c][tap] += sum_{b,p} a[b][p + off(tap)][c] * dy[b][o][p];  db[o] += sum dy
 * ws: >= nblk * (9 * C + 1) * Cout floats with nblk = B * ceil(H*W / 512). */
typedef struct anoddpm_head_bwd_args {
    const float *x;                 /* [B][H*W][C] */
    const float *gn_scale, *gn_shift; /* [B][C] */
    const float *w;                 /* OIHW [Cout][C][3][3] (the parameter itself) */
    const float *dy;                /* [B][Cout][H][W] */
    float *da;                      /* [B][H*W][C] */
    float *dw, *db;                 /* accumulated into */
    float *ws;
    int64_t ws_floats;
    int32_t B, H, W, C, Cout;
} anoddpm_head_bwd_args;

int anoddpm_conv_head_backward(const anoddpm_head_bwd_args *a, void *stream);

/* Fold of the per-work-item column sums anoddpm_conv3x3_wgrad publishes ([B][ipb][N]: items of an image are
 * consecutive): dimg[b][n] = sum_items (written: the embedding-projection gradient, UNet.py:213) and
 * dbias[n] += sum_b dimg[b][n] (optional). */
typedef struct anoddpm_colsum_fold_args {
    const float *colsum;
    float *dimg;                    /* [B][N], written (scratch when only the bias gradient is wanted) */
    float *dbias;                   /* [N] or NULL, accumulated into */
    int32_t B, ipb, N;
} anoddpm_colsum_fold_args;

int anoddpm_colsum_fold(const anoddpm_colsum_fold_args *a, void *stream);

/* ------------------------------------------------------------------ MRI slice loader (dataset.py:575-643) ----------
 * Volume normalisation of MRIDataset.__getitem__ (dataset.py:585-592): clip to [mean - std, mean + 2 std] (population
 * std, fp64 two-pass), divide by the range, store fp32.  workspace: >= 2*256 + 4 doubles [dev]. */
int anoddpm_volume_normalise(const double *vol, int64_t n, float *out, double *workspace, void *stream);

/* Slice cut (dataset.py:621: image[:, s:s+1, :].reshape(X, Z)), optional RandomAffine resampling (PIL AFFINE / NEAREST:
 * affine = six 16.16 fixed-point coefficients per item, source = (a2 + a0 x + a1 y) >> 16, (a5 + a3 x + a4 y) >> 16, fill 0)
 * and torchvision CenterCrop(crop) with its zero padding: out[b][oy][ox] = img[oy + crop_top][ox - pad_left]. */
typedef struct anoddpm_mri_slice_args {
    const float *const *vols;       /* [dev] B pointers to resident fp32 volumes [X][Y_b][Z] */
    const int32_t *ydim;            /* [dev] Y_b */
    const int32_t *slice_idx;       /* [dev] */
    const long long *affine;        /* [dev] [B][6] or NULL (no augmentation) */
    float *out;                     /* [B][crop][crop] */
    int32_t B, X, Z, crop, pad_left, crop_top;
} anoddpm_mri_slice_args;

int anoddpm_mri_slice_prepare(const anoddpm_mri_slice_args *a, void *stream);

/* PIL Image.resize(BILINEAR) on fp32 images (what torchvision Resize does to a mode-"F" image), then optionally
 * Normalize: out = (v - mean) / std.  Coefficient tables are PIL's precompute_coeffs (host, fp64): for output index o the
 * taps in[kmin[o] .. kmin[o] + kn[o]) with weights k[o][0 .. kn[o]), row length kmax.  tmp: [B][in_h][out_w] floats. */
typedef struct anoddpm_resize_args {
    const float *in;                /* [B][in_h][in_w] */
    float *tmp, *out;               /* out: [B][out_h][out_w] */
    const double *kx;               /* [out_w][kmax_x] */
    const int32_t *kx_min, *kx_n;
    const double *ky;               /* [out_h][kmax_y] */
    const int32_t *ky_min, *ky_n;
    int32_t B, in_h, in_w, out_h, out_w, kmax_x, kmax_y;
    float mean, std;
    int32_t normalize;
} anoddpm_resize_args;

int anoddpm_resize_bilinear_pil(const anoddpm_resize_args *a, void *stream);

/* Anomalous test-set slices and their masks (AnomalousMRIDataset.__getitem__, dataset.py:646-790) in ONE launch: per item the plane
 * vols[i][slice_idx[i]] of a resident fp32 volume [S_i][R][C] (axis 0 is sliced, planes are contiguous), torchvision
 * CenterCrop((crop_h, crop_w)) with its zero padding, PIL Image.resize(BILINEAR) -- horizontal pass, then vertical pass, fp64
 * sums in ascending tap order, an fp32 rounding after each pass, exactly as anoddpm_resize_bilinear_pil -- and Normalize:
 *   img[i][oy][ox]  = (v - mean) / std
 *   mask[i][oy][ox] = ((m - mean) / std > 0) ? 1.f : 0.f      the mask plane through the same transform, then `> 0` (:748-754)
 * The cropped image is crop[y][x] = plane[y + crop_top][x + crop_left] where that lies inside the plane and 0 elsewhere; both
 * offsets are signed (negative where the plane is smaller than the crop and torchvision pads).  Coefficient tables as in
 * anoddpm_resize_args, for crop_w -> out_w (kx) and crop_h -> out_h (ky).  No intermediate goes to global memory.
 * The caller guarantees 0 <= slice_idx[i] < S_i; a NULL entry of masks[] reads as a plane of zeros. */
typedef struct anoddpm_ano_slices_args {
    const float *const *vols;       /* [dev] n pointers to resident fp32 volumes [S_i][R][C] */
    const float *const *masks;      /* [dev] n pointers to mask volumes of the same shapes, or NULL: no mask output */
    const int32_t *slice_idx;       /* [dev] n */
    float *img;                     /* [n][out_h][out_w] */
    float *mask;                    /* [n][out_h][out_w]; required when masks is given, else unused */
    const double *kx;               /* [out_w][kmax_x] */
    const int32_t *kx_min, *kx_n;
    const double *ky;               /* [out_h][kmax_y] */
    const int32_t *ky_min, *ky_n;
    int32_t n, R, C, crop_h, crop_w, crop_top, crop_left, out_h, out_w, kmax_x, kmax_y;
    float mean, std;
} anoddpm_ano_slices_args;

int anoddpm_ano_slices(const anoddpm_ano_slices_args *a, void *stream);

/* ------------------------------------------------------------------ known-region conditioning */

/* Known-region conditioning of one reverse step: the pixels marked "keep" are tied to an input image at every step,
 * the rest comes from the ordinary reverse update -- RePaint (Lugmayr et al., CVPR 2022, Algorithm 1 / eq. 8) and the "stitch" of
 * AutoDDPM (Bercea et al., 2023), on the update of GaussianDiffusion.py:298-318 and the q-sample of :361-371.  ONE launch, per
 * sample b with ti the normalised t[b] and s = ti - 1 (ancestral) or ti - *stride (strided):
 *   u      = what anoddpm_p_sample_update / _gauss / anoddpm_strided_update with the same `a`, strided block and key block writes
 *            to x_prev, its step noise included (a->noise, or domain 0 at step ti)
 *   kz     = k->noise, or -- when that is NULL -- generated in the kernel from the key block with domain 3 at step s
 *   kn     = s < 0 ? x0 : ca[s] * x0 + cb[s] * kz           (separate mul, mul, add: no FMA, as anoddpm_q_sample)
 *   x_prev = keep ? kn : u                                  a select, not a blend: a NaN on one side never reaches the other
 * pred_x0 and mean_out are those of the unconditioned update at every pixel.  With s < 0 the known noise is neither read nor
 * generated.  An out-of-range t[b] or a stride < 1 makes every element of x_prev of that sample NaN, kept pixels included; nothing
 * is read out of bounds.  x_prev may alias x_t.  Bit-identical to the unconditioned launch, anoddpm_philox_fill (kind 1, domain 3,
 * step s), anoddpm_q_sample at s and a select -- four launches that move 41 B/pixel -- in one launch that moves 17 B/pixel (x_t, eps,
 * x0, one keep byte, x_prev), plus 4 for each noise that is read from a plane instead of being generated.
 * alphas_cumprod / stride / eta: all NULL for the ancestral update, all set for the strided one.  seed == NULL: the step noise is
 * a->noise (or none) and k->noise is required; otherwise a->noise must be NULL. */
typedef struct anoddpm_known_args {
    const float *x0;           /* [dev] fp32; sample b at x0 + b * x0_stride */
    const uint8_t *keep;       /* [dev] bytes; nonzero = keep this pixel; sample b at keep + b * keep_stride */
    const float *noise;        /* [dev] fp32 known-region noise, sample b at noise + b * noise_stride; or NULL */
    const float *ca, *cb;      /* sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, fp32[a->T] */
    int64_t x0_stride, keep_stride, noise_stride;      /* each 0 (one plane for all samples) or a->n */
} anoddpm_known_args;

int anoddpm_p_sample_update_known(const anoddpm_p_update_args *a, const anoddpm_known_args *k, const double *alphas_cumprod,
                                  const int32_t *stride, const float *eta, const uint64_t *seed, const int32_t *streams,
                                  uint32_t stream0, void *stream);

/* ------------------------------------------------------------------ resampling jumps */

/* The resampling loop of RePaint (Lugmayr et al., CVPR 2022, Algorithm 1) on the conditioned step above, ancestral
 * only.  A chain carries, per sample, the level `top` it started from, the repetitions `rep` it has left and the count `visit` of
 * jumps it has taken; `jump` (J) and `reps` (R) are one word each.  ONE launch, per sample b with ti the normalised t[b],
 * s = ti - 1 and v = visit[b]:
 *   x_s    = what anoddpm_p_sample_update_known (ancestral) writes to x_prev, except that generated noise uses Philox domain
 *            0 + 8 v (step noise, step ti) and 3 + 8 v (known-region noise, step s)
 *   jumps  = s >= 0 && s % J == 0 && s + J <= top[b] && rep[b] > 0
 *   land   = jumps ? s + J : s
 *   x_prev = jumps ? A * x_s + C * rz : x_s                       separate mul, mul, add; EVERY pixel, kept ones included
 *   A, C   = (float)sqrt(acp[land] / acp[s]), (float)sqrt(1 - acp[land] / acp[s])      fp64, each rounded to fp32 once
 *   rz     = r->noise, or -- when that is NULL -- generated from the key block in domain 4 + 8 v at step land
 * pred_x0 and mean_out are those of the unconditioned update.  With v == 0 and no jump the launch writes the bits of
 * anoddpm_p_sample_update_known.  The launch reads the state and writes none of it: anoddpm_chain_advance_resample is its only
 * writer.  An out-of-range t[b], a J or R word < 1, or a jump that would land beyond the schedule (a `top` >= a->T) makes every
 * element of x_prev of that sample NaN; such a sample takes no jump and nothing is read out of bounds.
 * seed == NULL: a->noise (or none), k->noise and r->noise are read, the latter two are required; otherwise a->noise must be NULL. */
/* (anoddpm_resample_args is the 2x up / down resampling of the UNet: this one is named for the schedule.) */
typedef struct anoddpm_resampling_args {
    const int32_t *jump, *reps;        /* [dev] one word each, read at run time: a kept graph follows re-written words */
    const int32_t *top, *rep, *visit;  /* [dev] int32[B] chain state */
    const float *noise;                /* [dev] fp32 re-noise, sample b at noise + b * noise_stride; or NULL */
    const double *alphas_cumprod;      /* [dev] fp64[a->T] */
    int64_t noise_stride;              /* 0 (one plane for all samples) or a->n */
} anoddpm_resampling_args;

int anoddpm_p_sample_update_resample(const anoddpm_p_update_args *a, const anoddpm_known_args *k, const anoddpm_resampling_args *r,
                                     const uint64_t *seed, const int32_t *streams, uint32_t stream0, void *stream);

/* The state rules of a resampled chain, one thread per sample (B <= 1024), then *step += 1 (step may be NULL).  With s = t[b] - 1:
 *   jumps (the predicate above)               t[b] = s + J, rep[b] -= 1, visit[b] += 1
 *   else s >= 0 && s % J == 0                 rep[b] = R - 1, t[b] = s
 *   else                                      t[b] = max(s, 0)
 * With a J or R word < 1 only the last rule applies. */
int anoddpm_chain_advance_resample(int64_t *t, int32_t B, int32_t *step, const int32_t *jump, const int32_t *reps,
                                   const int32_t *top, int32_t *rep, int32_t *visit, void *stream);

/* ------------------------------------------------------------------ keep mask of a two-pass detection */

/* The step between the two passes of a two-pass detection (the mask / stitch of AutoDDPM, Bercea et al., 2023): a first
 * reconstruction says where the image looks abnormal, that region grown by a margin is regenerated in a second, conditioned pass
 * (anoddpm_p_sample_update_known) and everything else stays tied to the input.  ONE launch, per plane p of S; the plane is H x W
 * fp32 at score + p * score_stride, score_stride >= H*W:
 *   thr        = threshold[p * thr_stride]            device memory, thr_stride 0 or 1; never a host value
 *   seed(y,x)  = score(y,x) > thr  &&  (roi == NULL || roi(y,x) == 1)
 *                NaN is above nothing; -0.0 is not above +0.0; strictly greater
 *   grown      = scipy.ndimage.binary_dilation(seed, iterations=r) with scipy's defaults (4-neighbour cross, border_value=0),
 *                0 <= r <= 8: r passes of the cross are ONE pass of the L1 ball of radius r, the outside of the image contributing
 *                nothing; r = 0: grown = seed
 *   regen(y,x) = grown(y,x)  &&  (roi == NULL || roi(y,x) == 1)
 *   keep[p][y][x]        = regen ? 0 : 1              uint8, contiguous [S][H][W]: the byte format anoddpm_known_args.keep reads
 *   stitched[p][c][y][x] = regen ? recon[p][c][y][x] : real[p][c][y][x]
 *                optional, all three pointers or none; C >= 1 channels share the plane's mask; a select, so a NaN on one side
 *                never reaches the other
 *   regen_count[p]       = number of pixels with keep == 0   (int32)
 *   status[p]            = ANODDPM_ROC_NAN if the plane's score or its threshold holds a NaN; ANODDPM_ROC_BAD_MASK for a roi value
 *                other than 0 / 1
 * roi: optional fp32 0/1 planes at roi + p * roi_stride, roi_stride 0 (one plane for all) or H*W, as in anoddpm_median2d.  real is
 * at real + p * real_stride, real_stride 0 or C*H*W; recon and stitched are contiguous [S][C][H][W].  A NaN threshold marks
 * nothing: all comparisons are false, every pixel is kept, and the status bit is set.  No allocation and no host synchronisation:
 * regen_count and status are cleared by an asynchronous memset on the stream before the launch.  A workgroup stages a 16 x 32 tile
 * of a plane with an r-pixel LDS halo (several tiles of a tile row, one after the other, once the grid would exceed what the chip
 * holds at a time) and adds its count once; outputs are a set and integers, so the bits are the same every run.
 * Refused (ANODDPM_EINVAL): null args; null score, threshold, keep, regen_count or status; r outside 0 ... 8; S, H, W or C < 1, or
 * S * tiles >= 2^31; score_stride < H*W with S > 1; thr_stride not 0 / 1; roi_stride not 0 / H*W; real_stride not 0 / C*H*W; only
 * one or two of real, recon, stitched. */
typedef struct anoddpm_keep_mask_args {
    const float *score;             /* [dev] */
    const float *threshold;         /* [dev] one word, or [S] */
    const float *roi;               /* [dev] or NULL */
    const float *real;              /* [dev] or NULL */
    const float *recon;             /* [dev] [S][C][H][W] or NULL */
    uint8_t *keep;                  /* [dev] [S][H][W] */
    float *stitched;                /* [dev] [S][C][H][W] or NULL */
    int32_t *regen_count;           /* [dev] [S] */
    int32_t *status;                /* [dev] [S] */
    int64_t score_stride, thr_stride, roi_stride, real_stride;
    int32_t S, H, W, C, r;
} anoddpm_keep_mask_args;

int anoddpm_keep_mask(const anoddpm_keep_mask_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ANODDPM_HIP_H */
