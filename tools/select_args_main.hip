// The argument checks of anoddpm_select_wide, anoddpm_select_wide_workspace_bytes and anoddpm_threshold_counts
// (csrc/select_wide.hip) as a stand-alone host program, for a run under AddressSanitizer / UBSan on a machine without a GPU: every
// call below is refused before anything is launched, so no device is touched and the device pointers are made-up addresses that
// are never read; ranks_host is a real host array, which the checks do read.  The program includes select_wide.hip itself (the
// checks under test are the ones the library ships) and supplies the two symbols it takes from executor.hip.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/select_args_main.hip -o /tmp/select_args && /tmp/select_args
//
// Prints one line per refused call and "N refusals, 0 accepted"; exits 1 if a call was accepted or a message does not name its reason.
#include <stdarg.h>
#include <string.h>

#include "../anoddpm_amd/csrc/select_wide.hip"

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
static uint32_t good_ranks[3] = {0, 5, 99}, past_ranks[3] = {0, 100, 0xffffffffu};

static void expect(int rc, const char *what, const char *word)
{
    const bool ok = rc == ANODDPM_EINVAL && strstr(anoddpm::g_err, word) != nullptr;
    printf("%-60s rc %d  %s%s\n", what, rc, anoddpm::g_err, ok ? "" : "   <-- UNEXPECTED");
    refusals += ok ? 1 : 0;
    failures += ok ? 0 : 1;
    anoddpm::g_err[0] = 0;
}

static anoddpm_select_args select_args()
{
    anoddpm_select_args a = {};
    a.src = reinterpret_cast<const float *>(0x10000);
    a.ranks = reinterpret_cast<const uint32_t *>(0x20000);
    a.ranks_host = good_ranks;
    a.workspace = reinterpret_cast<void *>(0x30000);
    a.workspace_bytes = 1 << 20;
    a.value = reinterpret_cast<float *>(0x40000);
    a.above = reinterpret_cast<int64_t *>(0x41000);
    a.equal = reinterpret_cast<int64_t *>(0x42000);
    a.topk_mean = reinterpret_cast<double *>(0x43000);
    a.max = reinterpret_cast<float *>(0x44000);
    a.mean = reinterpret_cast<double *>(0x45000);
    a.status = reinterpret_cast<int32_t *>(0x46000);
    a.src_stride = a.n = 100;
    a.S = 2;
    a.Q = 3;
    return a;
}

static anoddpm_threshold_counts_args counts_args()
{
    anoddpm_threshold_counts_args a = {};
    a.score = reinterpret_cast<const float *>(0x10000);
    a.mask = reinterpret_cast<const float *>(0x20000);
    a.thr = reinterpret_cast<const float *>(0x30000);
    a.counts = reinterpret_cast<int64_t *>(0x40000);
    a.totals = reinterpret_cast<int64_t *>(0x41000);
    a.status = reinterpret_cast<int32_t *>(0x42000);
    a.n = a.score_stride = a.mask_stride = 100;
    a.thr_stride = 4;
    a.S = 2;
    a.T = 4;
    return a;
}

int main()
{
    int32_t tile = 0;
    expect(anoddpm_select_wide(nullptr, 0, nullptr), "select_wide(NULL)", "null args");
#define SELECT(change, word) { anoddpm_select_args a = select_args(); tile = 0; change; expect(anoddpm_select_wide(&a, tile, nullptr), "select_wide: " #change, word); }
    SELECT(a.src = nullptr, "null pointer")
    SELECT(a.ranks = nullptr, "null pointer")
    SELECT(a.workspace = nullptr, "null pointer")
    SELECT(a.value = nullptr, "null pointer")
    SELECT(a.above = nullptr, "null pointer")
    SELECT(a.equal = nullptr, "null pointer")
    SELECT(a.topk_mean = nullptr, "null pointer")
    SELECT(a.max = nullptr, "null pointer")
    SELECT(a.mean = nullptr, "null pointer")
    SELECT(a.status = nullptr, "null pointer")
    SELECT(a.S = 0, "S must")
    SELECT(a.S = INT32_MIN, "S must")
    SELECT(a.n = 0, "n must")
    SELECT(a.n = INT64_MIN, "n must")
    SELECT(a.n = a.src_stride = (int64_t)1 << 31, "n must")
    SELECT(a.n = a.src_stride = INT64_MAX, "n must")
    SELECT(a.Q = 0, "Q must")
    SELECT(a.Q = 17, "Q must")
    SELECT(a.Q = INT32_MIN, "Q must")
    SELECT(tile = 100, "tile")
    SELECT(tile = -256, "tile")
    SELECT(tile = INT32_MIN, "tile")
    SELECT(tile = INT32_MAX, "tile")
    SELECT(a.src_stride = 99, "src_stride")
    SELECT(a.src_stride = INT64_MIN, "src_stride")
    SELECT(a.workspace_bytes = 64, "workspace too small")
    SELECT(a.workspace_bytes = INT64_MIN, "workspace too small")
    SELECT(a.workspace = reinterpret_cast<void *>(0x30008), "aligned")
    SELECT(a.ranks_host = past_ranks, "not below n")
    SELECT(a.n = a.src_stride = 99, "not below n")
    SELECT(a.ranks_host = past_ranks + 2; a.Q = 1; a.n = a.src_stride = ((int64_t)1 << 31) - 1, "not below n")
#undef SELECT
    struct { int64_t n; int32_t Q, tile; } bad[] = {{0, 1, 0}, {-1, 1, 0}, {(int64_t)1 << 31, 1, 0}, {INT64_MAX, 1, 0}, {INT64_MIN, 1, 0}, {100, 0, 0},
                                                    {100, 17, 0}, {100, INT32_MIN, 0}, {100, 1, 100}, {100, 1, -256}, {100, 1, INT32_MAX}};
    for (const auto &b : bad) {
        const int64_t got = anoddpm_select_wide_workspace_bytes(b.n, b.Q, b.tile);
        printf("select_wide_workspace_bytes(%lld, %d, %d) = %lld%s\n", (long long)b.n, (int)b.Q, (int)b.tile, (long long)got, got == -1 ? "" : "   <-- UNEXPECTED");
        refusals += got == -1;
        failures += got != -1;
    }
    if (anoddpm_select_wide_workspace_bytes(((int64_t)1 << 31) - 1, 16, INT32_MAX - 255) <= 0) { printf("the largest accepted call is refused\n"); ++failures; }

    expect(anoddpm_threshold_counts(nullptr, nullptr), "threshold_counts(NULL)", "null args");
#define COUNTS(change, word) { anoddpm_threshold_counts_args a = counts_args(); change; expect(anoddpm_threshold_counts(&a, nullptr), "threshold_counts: " #change, word); }
    COUNTS(a.score = nullptr, "null pointer")
    COUNTS(a.mask = nullptr, "null pointer")
    COUNTS(a.thr = nullptr, "null pointer")
    COUNTS(a.counts = nullptr, "null pointer")
    COUNTS(a.totals = nullptr, "null pointer")
    COUNTS(a.status = nullptr, "null pointer")
    COUNTS(a.S = 0, "S must")
    COUNTS(a.S = INT32_MIN, "S must")
    COUNTS(a.n = 0, "n must")
    COUNTS(a.n = INT64_MIN, "n must")
    COUNTS(a.n = a.score_stride = a.mask_stride = (int64_t)1 << 31, "n must")
    COUNTS(a.n = a.score_stride = a.mask_stride = INT64_MAX, "n must")
    COUNTS(a.T = 0, "T must")
    COUNTS(a.T = 17; a.thr_stride = 17, "T must")
    COUNTS(a.T = INT32_MIN, "T must")
    COUNTS(a.score_stride = 99, "score_stride")
    COUNTS(a.score_stride = INT64_MIN, "score_stride")
    COUNTS(a.mask_stride = 50, "mask_stride")
    COUNTS(a.mask_stride = -1, "mask_stride")
    COUNTS(a.thr_stride = 3, "thr_stride")
    COUNTS(a.thr_stride = INT64_MIN, "thr_stride")
    COUNTS(a.n = a.score_stride = ((int64_t)1 << 31) - 1; a.mask_stride = 0; a.S = INT32_MAX, "S * tiles")
#undef COUNTS
    printf("%d refusals, %d accepted or misworded\n", refusals, failures);
    return failures ? 1 : 0;
}
