// Native executor + library plumbing: error reporting, flat op-list runner (the C++ side of
// UNetModel.forward, UNet.py:390-406 -- one call per forward instead of ~1000 ATen dispatches),
// and HIP-event timing per op class for bench.py's roofline leg.
#include <stdarg.h>
#include <string.h>
#include <vector>
#include "common.h"

namespace anoddpm {

static thread_local char g_err[512] = "";
int g_debug[16] = {0};

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

struct ProfState {
    bool on = false;
    std::vector<hipEvent_t> pool;       // pairs: start, stop
    std::vector<int> codes;
    std::vector<float> last_ms;         // per recorded op of the last collect, in launch order
    std::vector<int> last_codes;
    size_t used = 0;
    double ms[ANODDPM_OP_MAX] = {0};
    int64_t launches[ANODDPM_OP_MAX] = {0};
};
static ProfState g_prof;

// Every op anoddpm_run_ops executes, named once: ANODDPM_OP_<code>, the struct its `args` points to, the entry point that takes it.
#define ANODDPM_OPS(X) \
    X(IGEMM,            anoddpm_igemm_args,            anoddpm_igemm) \
    X(GN_STATS,         anoddpm_gn_args,               anoddpm_gn_stats) \
    X(SOFTMAX,          anoddpm_softmax_args,          anoddpm_softmax_rows) \
    X(RESAMPLE,         anoddpm_resample_args,         anoddpm_resample2x) \
    X(LINEAR,           anoddpm_linear_args,           anoddpm_linear_small) \
    X(POSEMB,           anoddpm_posemb_args,           anoddpm_posemb) \
    X(STEM,             anoddpm_stem_args,             anoddpm_conv_stem) \
    X(LAYOUT,           anoddpm_layout_args,           anoddpm_nhwc_to_nchw) \
    X(CHAN_STATS,       anoddpm_chan_stats_args,       anoddpm_chan_stats) \
    X(HEAD,             anoddpm_head_args,             anoddpm_conv_head) \
    X(GN_FINALIZE,      anoddpm_gn_finalize_args,      anoddpm_gn_finalize) \
    X(WGRAD3,           anoddpm_wgrad_args,            anoddpm_conv3x3_wgrad) \
    X(WGRAD1,           anoddpm_wgrad1_args,           anoddpm_wgrad_pointwise) \
    X(GN_BWD,           anoddpm_gn_bwd_args,           anoddpm_gn_silu_backward) \
    X(PACK,             anoddpm_pack_args,             anoddpm_pack_weights) \
    X(SOFTMAX_BWD,      anoddpm_softmax_bwd_args,      anoddpm_softmax_rows_backward) \
    X(TRANSPOSE,        anoddpm_transpose_args,        anoddpm_transpose_square) \
    X(LINEAR_BWD,       anoddpm_linear_bwd_args,       anoddpm_linear_small_backward) \
    X(STEM_BWD,         anoddpm_stem_bwd_args,         anoddpm_conv_stem_backward) \
    X(HEAD_BWD,         anoddpm_head_bwd_args,         anoddpm_conv_head_backward) \
    X(COLSUM_FOLD,      anoddpm_colsum_fold_args,      anoddpm_colsum_fold) \
    X(ATTENTION,        anoddpm_attention_args,        anoddpm_attention) \
    X(PACK_BATCH,       anoddpm_pack_batch_args,       anoddpm_pack_batch) \
    X(DROPOUT,          anoddpm_dropout_args,          anoddpm_dropout) \
    X(LINEAR_BWD_BATCH, anoddpm_linear_bwd_batch_args, anoddpm_linear_small_backward_batch)

static int dispatch(const anoddpm_op &op, void *stream)
{
    switch (op.code) {
#define X(code, args_t, fn) case ANODDPM_OP_##code: return fn(static_cast<const args_t *>(op.args), stream);
        ANODDPM_OPS(X)
#undef X
        default: set_error("run_ops: unknown op code %d", op.code); return ANODDPM_EINVAL;
    }
}

}  // namespace anoddpm

using namespace anoddpm;

// Kernel-variant selector for tests and measurements; NOT part of the public ABI (include/anoddpm_hip.h does not declare it).
// In a product build only the keys whose every value still computes the right result are accepted (0: F(2x2) workgroup
// shape, 4: head kernel form, 5: F(4x4) position- vs channel-sliced, 8: weight-gradient fold form); the timing ablations
// that skip work (keys 1, 2, 3, 6, 7) exist only in a -DANODDPM_ABLATE build (ANODDPM_ABLATE=1 python -m anoddpm_amd.build).
extern "C" int anoddpm_internal_variant(int32_t key, int32_t value)
{
    if (key < 0 || key >= 16) return ANODDPM_EINVAL;
#ifndef ANODDPM_ABLATE
    if (!(key == 0 || key == 4 || key == 5 || key == 8 || key == 9)) {
        set_error("internal_variant: key %d selects a timing ablation; this library was built without ANODDPM_ABLATE", key);
        return ANODDPM_EINVAL;
    }
#endif
    g_debug[key] = value;
    return ANODDPM_OK;
}

extern "C" int anoddpm_ablate_build(void)
{
#ifdef ANODDPM_ABLATE
    return 1;
#else
    return 0;
#endif
}

extern "C" int anoddpm_abi_version(void) { return ANODDPM_ABI_VERSION; }

extern "C" const char *anoddpm_last_error(void) { return g_err; }

extern "C" int anoddpm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

extern "C" int anoddpm_run_ops(const anoddpm_op *ops, int32_t n, void *stream)
{
    ANODDPM_REQUIRE(ops || n == 0, "run_ops: null op list");
    for (int i = 0; i < n; ++i) {
        ANODDPM_REQUIRE(ops[i].args, "run_ops: op %d has null args", i);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        const bool prof = g_prof.on && ops[i].code > 0 && ops[i].code < ANODDPM_OP_MAX;
        if (prof) {
            if (g_prof.used + 2 > g_prof.pool.size()) {
                hipEvent_t a, b;
                if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
                    set_error("run_ops: hipEventCreate failed");
                    return ANODDPM_ELAUNCH;
                }
                g_prof.pool.push_back(a);
                g_prof.pool.push_back(b);
            }
            e0 = g_prof.pool[g_prof.used];
            e1 = g_prof.pool[g_prof.used + 1];
            g_prof.used += 2;
            // Winograd launches of anoddpm_igemm are booked under code 12 (F(2x2,3x3)) / 14 (F(4x4,3x3)) so the dominant kernels can be priced alone
            // ... and the Winograd-domain launches of anoddpm_conv3x3_wgrad (algo 1) under code 15
            const int icfg = ops[i].code == ANODDPM_OP_IGEMM ? static_cast<const anoddpm_igemm_args *>(ops[i].args)->cfg : 0;
            const bool w43 = ops[i].code == ANODDPM_OP_WGRAD3 && static_cast<const anoddpm_wgrad_args *>(ops[i].args)->algo == 1;
            // ... the small-map no-split launches (cfg 5) under code 13
            g_prof.codes.push_back((icfg == 2 || icfg == 6) ? 12 : ((icfg == 3 || icfg == 7) ? 14 : (icfg == 5 ? 13 : (w43 ? 15 : ops[i].code))));
            (void)hipEventRecord(e0, as_stream(stream));
        }
        const int rc = dispatch(ops[i], stream);
        if (prof) (void)hipEventRecord(e1, as_stream(stream));
        if (rc != ANODDPM_OK) {
            char tmp[400];
            strncpy(tmp, g_err, sizeof(tmp) - 1);
            tmp[sizeof(tmp) - 1] = 0;
            set_error("op %d (code %d): %s", i, ops[i].code, tmp);
            return rc;
        }
    }
    return ANODDPM_OK;
}

extern "C" int anoddpm_prof_enable(int32_t enable)
{
    g_prof.on = enable != 0;
    if (enable) {
        g_prof.used = 0;
        g_prof.codes.clear();
        memset(g_prof.ms, 0, sizeof(g_prof.ms));
        memset(g_prof.launches, 0, sizeof(g_prof.launches));
    }
    return ANODDPM_OK;
}

extern "C" int anoddpm_prof_active(void) { return g_prof.on ? 1 : 0; }

extern "C" int anoddpm_prof_collect(double *ms_per_code, int64_t *launches_per_code)
{
    ANODDPM_REQUIRE(ms_per_code && launches_per_code, "prof_collect: null pointer");
    g_prof.last_ms.clear();
    g_prof.last_codes.clear();
    for (size_t i = 0; i < g_prof.codes.size(); ++i) {
        hipEvent_t e0 = g_prof.pool[2 * i], e1 = g_prof.pool[2 * i + 1];
        if (hipEventSynchronize(e1) != hipSuccess) { set_error("prof_collect: event sync failed"); return ANODDPM_ELAUNCH; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { set_error("prof_collect: elapsed failed"); return ANODDPM_ELAUNCH; }
        g_prof.ms[g_prof.codes[i]] += ms;
        g_prof.launches[g_prof.codes[i]] += 1;
        g_prof.last_ms.push_back(ms);
        g_prof.last_codes.push_back(g_prof.codes[i]);
    }
    g_prof.codes.clear();
    g_prof.used = 0;
    for (int c = 0; c < ANODDPM_OP_MAX; ++c) { ms_per_code[c] = g_prof.ms[c]; launches_per_code[c] = g_prof.launches[c]; }
    return ANODDPM_OK;
}

// The ops of the last anoddpm_prof_collect in launch order: their profiler code and HIP-event time.  Returns the count (at most cap
// entries are written); with a plan's op list beside it this is a per-layer profile without an external tracer.
extern "C" int anoddpm_prof_list(int32_t *codes, float *ms, int32_t cap)
{
    const int n = (int)g_prof.last_ms.size();
    for (int i = 0; i < n && i < cap; ++i) {
        if (codes) codes[i] = g_prof.last_codes[i];
        if (ms) ms[i] = g_prof.last_ms[i];
    }
    return n;
}

// sizeof() of every struct of the ABI by its name, so that the Python binding can verify the layouts it derives from the header at
// load time.  Each struct is named once; the order does not matter.
#define ANODDPM_STRUCTS(X) \
    X(anoddpm_simplex_args) X(anoddpm_p_update_args) X(anoddpm_igemm_args) X(anoddpm_gn_args) X(anoddpm_softmax_args) \
    X(anoddpm_resample_args) X(anoddpm_linear_args) X(anoddpm_posemb_args) X(anoddpm_stem_args) X(anoddpm_layout_args) \
    X(anoddpm_op) X(anoddpm_adamw_args) X(anoddpm_chan_stats_args) X(anoddpm_gn_finalize_args) X(anoddpm_head_args) \
    X(anoddpm_anomaly_args) X(anoddpm_vlb_args) X(anoddpm_wgrad_args) X(anoddpm_gn_bwd_args) X(anoddpm_wgrad1_args) \
    X(anoddpm_pack_args) X(anoddpm_softmax_bwd_args) X(anoddpm_transpose_args) X(anoddpm_linear_bwd_args) \
    X(anoddpm_stem_bwd_args) X(anoddpm_head_bwd_args) X(anoddpm_colsum_fold_args) X(anoddpm_mri_slice_args) \
    X(anoddpm_resize_args) X(anoddpm_attention_args) X(anoddpm_pack_batch_args) X(anoddpm_linear_bwd_batch_args) \
    X(anoddpm_loss_args) X(anoddpm_dropout_args) X(anoddpm_roc_args) X(anoddpm_ssim_args) X(anoddpm_component_areas_args) \
    X(anoddpm_pro_args) X(anoddpm_distance_args) X(anoddpm_surface_args) X(anoddpm_median_args) X(anoddpm_erode_args) \
    X(anoddpm_components_args) X(anoddpm_gauss_args) X(anoddpm_map_scores_args) \
    X(anoddpm_ano_slices_args) X(anoddpm_select_args) X(anoddpm_threshold_counts_args) X(anoddpm_known_args) \
    X(anoddpm_resampling_args) X(anoddpm_keep_mask_args) X(anoddpm_median3d_args) X(anoddpm_erode3d_args) \
    X(anoddpm_components3d_args) X(anoddpm_component_areas3d_args) X(anoddpm_distance3d_args) X(anoddpm_surface3d_args) \
    X(anoddpm_gauss3d_args)

extern "C" int anoddpm_struct_size(const char *name)
{
    // Until ABI 31 the argument was an index (0 ... 42).  A caller written for that form hands one over as the pointer: no string
    // lives in the first page, so such a value (NULL included) is answered with -1 like any unknown name, not dereferenced.
    if (reinterpret_cast<uintptr_t>(name) < 4096) return -1;
#define X(s) if (strcmp(name, #s) == 0) return (int)sizeof(s);
    ANODDPM_STRUCTS(X)
#undef X
    return -1;
}
