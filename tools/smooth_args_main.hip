// The argument checks of anoddpm_gauss2d and anoddpm_map_scores (csrc/smooth.hip) as a stand-alone host program, for a run under
// AddressSanitizer / UBSan on a machine without a GPU: every call below is refused before anything is launched, so no device is
// touched and the pointers are made-up addresses that are never read.  The program includes smooth.hip itself (the checks under
// test are the ones the library ships) and supplies the two symbols it takes from executor.hip.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/smooth_args_main.hip -o /tmp/smooth_args && /tmp/smooth_args
//
// Prints one line per refused call and "N refusals, 0 accepted"; exits 1 if a call was accepted or a message does not name its reason.
#include <stdarg.h>
#include <string.h>

#include "../anoddpm_amd/csrc/smooth.hip"

namespace anoddpm {
static char g_err[512];
int g_debug[16] = {0};
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace anoddpm

static int failures = 0, refusals = 0;

static void expect(int rc, const char *what, const char *word)
{
    const bool ok = rc == ANODDPM_EINVAL && strstr(anoddpm::g_err, word) != nullptr;
    printf("%-44s rc %d  %s%s\n", what, rc, anoddpm::g_err, ok ? "" : "   <-- UNEXPECTED");
    refusals += ok ? 1 : 0;
    failures += ok ? 0 : 1;
    anoddpm::g_err[0] = 0;
}

static anoddpm_gauss_args gauss()
{
    anoddpm_gauss_args a = {};
    a.src = reinterpret_cast<const float *>(0x10000);
    a.dst = reinterpret_cast<float *>(0x90000);
    a.w = reinterpret_cast<const double *>(0x8000);
    a.src_stride = 64;
    a.S = 2;
    a.H = a.W = 8;
    a.radius = 16;
    return a;
}

static anoddpm_map_scores_args scores()
{
    anoddpm_map_scores_args a = {};
    a.src = reinterpret_cast<const float *>(0x10000);
    a.max = reinterpret_cast<float *>(0x90000);
    a.mean = reinterpret_cast<double *>(0x91000);
    a.topk_mean = reinterpret_cast<double *>(0x92000);
    a.status = reinterpret_cast<int32_t *>(0x93000);
    a.src_stride = a.n = 100;
    a.k = 3;
    a.S = 2;
    return a;
}

int main()
{
    expect(anoddpm_gauss2d(nullptr, nullptr), "gauss2d(NULL)", "null args");
#define GAUSS(change, word) { anoddpm_gauss_args a = gauss(); change; expect(anoddpm_gauss2d(&a, nullptr), "gauss2d: " #change, word); }
    GAUSS(a.src = nullptr, "null pointer")
    GAUSS(a.dst = nullptr, "null pointer")
    GAUSS(a.w = nullptr, "null pointer")
    GAUSS(a.radius = 0, "radius")
    GAUSS(a.radius = 33, "radius")
    GAUSS(a.radius = INT32_MIN, "radius")
    GAUSS(a.S = 0, "S, H, W")
    GAUSS(a.H = 0, "S, H, W")
    GAUSS(a.W = -1, "S, H, W")
    GAUSS(a.W = INT32_MAX, "below 2^30")
    GAUSS(a.S = INT32_MAX; a.H = 4096; a.W = 4096; a.src_stride = (int64_t)1 << 24, "tiles")
    GAUSS(a.src_stride = 63, "src_stride")
    GAUSS(a.src_stride = INT64_MIN, "src_stride")
    GAUSS(a.dst = const_cast<float *>(a.src), "overlaps")
    GAUSS(a.dst = const_cast<float *>(a.src) + 100, "overlaps")
    GAUSS(a.dst = const_cast<float *>(a.src) - 100, "overlaps")
    GAUSS(a.S = 1; a.src_stride = 0; a.dst = const_cast<float *>(a.src) + 63, "overlaps")
#undef GAUSS
    expect(anoddpm_map_scores(nullptr, nullptr), "map_scores(NULL)", "null args");
#define SCORES(change, word) { anoddpm_map_scores_args a = scores(); change; expect(anoddpm_map_scores(&a, nullptr), "map_scores: " #change, word); }
    SCORES(a.src = nullptr, "null pointer")
    SCORES(a.max = nullptr, "null pointer")
    SCORES(a.mean = nullptr, "null pointer")
    SCORES(a.topk_mean = nullptr, "null pointer")
    SCORES(a.status = nullptr, "null pointer")
    SCORES(a.S = 0, "S must")
    SCORES(a.S = INT32_MIN, "S must")
    SCORES(a.n = 0, "n must")
    SCORES(a.n = INT64_MIN, "n must")
    SCORES(a.n = a.src_stride = ANODDPM_MAP_SCORES_MAX_N + 1, "n must")
    SCORES(a.n = a.src_stride = INT64_MAX, "n must")
    SCORES(a.k = 0, "k must")
    SCORES(a.k = 101, "k must")
    SCORES(a.k = INT64_MIN, "k must")
    SCORES(a.src_stride = 99, "src_stride")
#undef SCORES
    printf("%d refusals, %d accepted or misworded\n", refusals, failures);
    return failures ? 1 : 0;
}
