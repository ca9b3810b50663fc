"""Shared by the element tests of the device weight packers (csrc/pack_items.h, anoddpm_pack_conv3x3, anoddpm_pack_weights,
anoddpm_pack_batch, anoddpm_pack_job_blocks, anoddpm_pack_wino43_bf16x3) -- tests/test_pack_reference.py on the CPU,
tests/test_gpu_pack_elements.py on the device.  Seeded weights, every layout restated in numpy fp64 from the text of
include/anoddpm_hip.h alone, the bars, the job tables of the batched launch.  numpy only; the library is not imported.

Why: since refresh_weights became one anoddpm_pack_batch launch every packed weight of every plan is written by these kernels, both
ledgers keep the packed buffers out of their poison step, and the direct tests cover modes 0 / 1 at three shapes under allclose and
kinds 2 / 3 at one shape each: nothing tests kind 5, kind 4, the batch's bisection, anoddpm_pack_job_blocks or the bf16 planes, which
are seen only through a convolution held to 1e-4 (a wrong or missing third plane, 2^-16 per weight, passes).

Layouts (w is OIHW [N][K][3][3], or [N][K]):
  W' = w (O = N, I = K);  bwd: W'[o = k][i = n][a][b] = w[n][k][2 - a][2 - b] (O = K, I = N)
  kind 0  out[t = 3 a + b][i / 4][o][i % 4] = W'[o][i][a][b]                                              a permutation
  kind 1  out[xi = 4 u + v][i / 4][o][i % 4] = (G g G^T)[u][v], g = W'[o][i], G the 4 x 3 matrix of F(2x2,3x3)
  kind 5  out[xi = 6 u + v][i / 4][o][i % 4] = (G g G^T)[u][v], G the 6 x 3 matrix of F(4x4,3x3) (points 0, +-1, +-2, inf)
  kind 2  out[k / 4][n][k % 4] = w[n][k];  bwd: out[n / 4][o][n % 4] = w[n][k0 + o], o < kc                permutations
  kind 3  out[t][k][n] = w[n][k][t]                                                                       a permutation
  kind 4  out[i] = w[i], i < N K
  bf16    [piece][xi][k / 8][n][k % 8] bf16: piece 0 / 1 / 2 = hi / mid / lo of the kind 5 forward value rounded once to fp32

Bars, all derived:
  permutations: bit for bit.
  Winograd: |got - U64| <= 2^-24 |U64| + 2^-45 S, S = |G| |g| |G|^T: one fp32 rounding of an fp64 value (unit roundoff 2^-24) plus
    the fp64 evaluation itself (five products and four additions per stage, two stages, any order, any contraction: below
    16 x 2^-53 S < 2^-45 S; the entries of G are rounded to fp64 once, inside the same bound).
  bf16 planes, f the once-rounded fp32 value, the pieces widened exactly: |f - (h + m + l)| <= 2^-24 |f|, |f - h| <= 2^-8 |f|,
    |m| <= 2^-8 |f|, |l| <= 2^-16 |f| (swapped or missing planes fail the last three).  f = fp32 of an fp64 evaluation of U, which
    lies within 2^-45 S of U64: one fp32 value, except where U is in exact arithmetic a tie between two fp32 neighbours (about one
    value in a hundred: -(g0 + g1 + g2) / 24 with a sum divisible by 3), where both neighbours are once-rounded values -- the fp32
    layout of the device and the host packer of tests/hipops.py differ there.  split3 (csrc/winograd43b.hip) rounds each piece to nearest
    bf16, which is tighter whichever way a tie of a piece goes: with f = +-2^e (1.x), |f - h| <= 2^(e-8), so m (8 bits) takes
    f - h to within 2^(e-16), and what is left is a multiple of f's last place 2^(e-23) of at most 2^(e-16): at most 8 bits, so l
    holds it exactly -- h + m + l = f, which the test asserts wherever |f| >= 2^-100 (no piece is subnormal), and on the device that
    sum is bit for bit the fp32 value of the kind 5 layout.  (The pieces themselves are not asserted bit for bit: the one piece of the
    74 880 values of the 130 x 16 case that is an exact bf16 tie, 0xb6078000, came back from the device rounded to the odd neighbour.)"""
import numpy as np

GUARD = 64                                                   # NaN elements behind every output
QUIET = 2.0 ** -10
G23 = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])
G43 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1.0]])
# the input and output transforms of the two algorithms (Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks"): the
# convolution identity of test_pack_reference.py, Y = A^T [(G g G^T) o (B^T d B)] A
BT23 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1.0]])
AT23 = np.array([[1, 1, 1, 0], [0, 1, -1, -1.0]])
BT43 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1.0]])
AT43 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1.0]])
TAPS = {0: 9, 1: 16, 5: 36}
WINO_G = {1: G23, 5: G43}

CONV_SHAPES = ((4, 4), (64, 32), (96, 36), (12, 20), (260, 8), (3, 8))            # (N, K)
POINTWISE_BWD = (24, 40, ((0, 40), (8, 16), (3, 5), (39, 1)))                      # N, K, (k0, kc)
SMALL_SHAPES = ((6, 5), (1, 1), (64, 3), (3, 64))
COPY_SIZES = (1, 257, 1000)
BF16_SHAPES = ((128, 8), (4, 32), (130, 16))

# a pack job: (kind, bwd, N, K, k0, kc)
JOBS13 = ((0, 0, 4, 4, 0, 0), (1, 0, 64, 32, 0, 0), (5, 0, 260, 8, 0, 0), (2, 0, 96, 36, 0, 0), (3, 0, 6, 5, 0, 0), (4, 0, 257, 1, 0, 0),
          (5, 1, 64, 32, 0, 0), (0, 1, 12, 20, 0, 0), (1, 1, 260, 8, 0, 0), (2, 1, 24, 40, 8, 16), (3, 0, 1, 1, 0, 0), (4, 0, 1, 1, 0, 0),
          (5, 0, 3, 8, 0, 0))
JOB_TABLES = ((JOBS13[6],), (JOBS13[2], (2, 1, 24, 40, 3, 5)), JOBS13)


def conv_jobs():
    """Every (kind, bwd, N, K) of the 3x3 layouts: forward where K % 4 == 0, backward where N % 4 == 0."""
    return [(kind, bwd, N, K, 0, 0) for kind in (0, 1, 5) for N, K in CONV_SHAPES for bwd in (0, 1) if (N if bwd else K) % 4 == 0]


def single_jobs():
    N, K, ranges = POINTWISE_BWD
    return (conv_jobs() + [(2, 0, N, K, 0, 0) for N, K in CONV_SHAPES if K % 4 == 0] + [(2, 1, N, K, k0, kc) for k0, kc in ranges]
            + [(3, 0, N, K, 0, 0) for N, K in SMALL_SHAPES] + [(4, 0, n, 1, 0, 0) for n in COPY_SIZES])


def job_id(job):
    kind, bwd, N, K, k0, kc = job
    return f"kind{kind}-{'bwd' if bwd else 'fwd'}-{N}x{K}" + (f"-cols{k0}+{kc}" if kind == 2 and bwd else "")


def weights(job, seed=0):
    """fp32 weights of a job: N(0, 1 / (9 K)), filters n % 4 == 1 scaled by 2^-10; [N][K][3][3], kinds 2 / 4: [N][K]."""
    kind, bwd, N, K, _, _ = job
    rng = np.random.default_rng(5000 + seed + 17 * kind + 1000 * N + K)
    w = rng.standard_normal((N, K, 3, 3) if kind in (0, 1, 3, 5) else (N, K)) / np.sqrt(9.0 * K)
    w[np.arange(N) % 4 == 1] *= QUIET
    return w.astype(np.float32)


def items(job):
    """Threads a job needs (one item each), from the header's layouts: a 3x3 item is one (o, input-channel quad)."""
    kind, bwd, N, K, k0, kc = job
    if kind in (0, 1, 5):
        return N * K // 4
    if kind == 2:
        return N * kc if bwd else N * K
    return 9 * N * K if kind == 3 else N * K


def blocks(job):
    return -(-items(job) // 256)


def out_floats(job):
    kind, bwd, N, K, k0, kc = job
    if kind in TAPS:
        return TAPS[kind] * N * K
    if kind == 2:
        return N * kc if bwd else N * K
    return 9 * N * K if kind == 3 else N * K


def effective(w, bwd):
    """W' [O][I][3][3] fp64."""
    w = np.asarray(w, dtype=np.float64)
    return w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1] if bwd else w


def _quads(v):
    """[T][O][I] -> [T][I / 4][O][4]"""
    T, O, I = v.shape
    return np.ascontiguousarray(v.reshape(T, O, I // 4, 4).transpose(0, 2, 1, 3))


def transform(wp, G):
    """(U, S) fp64 [u][v][O][I]: U = G g G^T and S = |G| |g| |G|^T."""
    return np.einsum("ua,oiab,vb->uvoi", G, wp, G), np.einsum("ua,oiab,vb->uvoi", np.abs(G), np.abs(wp), np.abs(G))


def restate(job, w):
    """(value fp64, S fp64 or None) of the packed buffer, flat: S is None for a permutation (bit for bit)."""
    kind, bwd, N, K, k0, kc = job
    w64 = np.asarray(w, dtype=np.float64)
    if kind in (0, 1, 5):
        wp = effective(w64, bwd)
        O, I = wp.shape[:2]
        if kind == 0:
            return _quads(wp.reshape(O, I, 9).transpose(2, 0, 1)).reshape(-1), None
        U, S = transform(wp, WINO_G[kind])
        return _quads(U.reshape(-1, O, I)).reshape(-1), _quads(S.reshape(-1, O, I)).reshape(-1)
    if kind == 2:
        if not bwd:
            return np.ascontiguousarray(w64.reshape(N, K // 4, 4).transpose(1, 0, 2)).reshape(-1), None
        return np.ascontiguousarray(w64[:, k0:k0 + kc].reshape(N // 4, 4, kc).transpose(0, 2, 1)).reshape(-1), None
    if kind == 3:
        return np.ascontiguousarray(w64.reshape(N, K, 9).transpose(2, 1, 0)).reshape(-1), None
    return w64.reshape(-1).copy(), None


def judge(job, w, got):
    """[] or the failures of a packed buffer `got` (fp32, flat, out_floats(job) long) against the restatement."""
    want, S = restate(job, w)
    got = np.asarray(got)
    if got.shape != want.shape:
        return [f"{got.size} floats, expected {want.size}"]
    if not np.isfinite(got).all():
        return [f"{int((~np.isfinite(got)).sum())} of {got.size} elements are not finite (unwritten)"]
    if S is None:
        bad = got.view(np.uint32) != want.astype(np.float32).view(np.uint32)
        return [f"{int(bad.sum())} of {bad.size} elements are not the restatement's bits; first at {int(np.argmax(bad))}"] if bad.any() else []
    err, bar = np.abs(got.astype(np.float64) - want), 2.0 ** -24 * np.abs(want) + 2.0 ** -45 * S
    bad = err > bar
    if bad.any():
        i = int(np.argmax(err - bar))
        return [f"{int(bad.sum())} of {bad.size} elements beyond 2^-24 |U| + 2^-45 S; worst at {i}: got {got[i]!r}, U {want[i]!r}, "
                f"error {err[i]:.3e}, allowed {bar[i]:.3e}"]
    return []


def worst_ulp(job, w, got):
    """max |got - U64| / (2^-24 |U64| + 2^-45 S) of a Winograd layout (1 is the bar), 0 for a permutation."""
    want, S = restate(job, w)
    if S is None:
        return 0.0
    bar = 2.0 ** -24 * np.abs(want) + 2.0 ** -45 * S
    ok = bar > 0
    return float((np.abs(np.asarray(got, dtype=np.float64) - want)[ok] / bar[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------------- bf16 planes
def bf16_rne(f):
    """fp32 -> the nearest-even bf16, widened back to fp32."""
    b = np.asarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def split3(f):
    """(hi, mid, lo) fp32-widened: the nearest-even split of csrc/winograd43b.hip."""
    f = np.asarray(f, dtype=np.float32)
    h = bf16_rne(f)
    r1 = f - h
    m = bf16_rne(r1)
    return h, m, bf16_rne(r1 - m)


def widen(u16):
    return (np.asarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_restate(N, K, w):
    """(U64, S) in the plane layout [36][K / 8][N][8], flat."""
    U, S = transform(np.asarray(w, dtype=np.float64), G43)

    def lay(v):
        return np.ascontiguousarray(v.reshape(36, N, K // 8, 8).transpose(0, 2, 1, 3)).reshape(-1)
    return lay(U), lay(S)


def judge_bf16(N, K, w, planes):
    """planes: uint16 [3 * 36 * N * K].  -> failures."""
    U, S = bf16_restate(N, K, w)
    n = U.size
    if np.asarray(planes).size != 3 * n:
        return [f"{np.asarray(planes).size} bf16 elements, expected {3 * n}"]
    h, m, lo = (widen(planes[i * n:(i + 1) * n]) for i in range(3))
    fails = []
    if not (np.isfinite(h).all() and np.isfinite(m).all() and np.isfinite(lo).all()):
        return ["a plane holds non-finite (unwritten) elements"]
    h64, m64, l64 = h.astype(np.float64), m.astype(np.float64), lo.astype(np.float64)
    # f, the once-rounded value: fp32 of an fp64 evaluation of U, which lies within 2^-45 S of U64.  Where U is, in exact arithmetic, a
    # tie between two fp32 neighbours (a sum of three fp32 weights divisible by 3, over 24: about one value in a hundred) both
    # neighbours are once-rounded values; everywhere else there is one.  Of the admissible values the one nearest the planes' sum.
    f_lo, f_hi = ((U + s * 2.0 ** -45 * S).astype(np.float32).astype(np.float64) for s in (-1.0, 1.0))
    f = np.clip(h64 + m64 + l64, np.minimum(f_lo, f_hi), np.maximum(f_lo, f_hi))
    a = np.abs(f)
    for what, lhs, rhs in (("|f - (h + m + l)| <= 2^-24 |f|", np.abs(f - (h64 + m64 + l64)), 2.0 ** -24 * a),
                           ("|f - h| <= 2^-8 |f|", np.abs(f - h64), 2.0 ** -8 * a), ("|m| <= 2^-8 |f|", np.abs(m64), 2.0 ** -8 * a),
                           ("|l| <= 2^-16 |f|", np.abs(l64), 2.0 ** -16 * a)):
        bad = lhs > rhs
        if bad.any():
            i = int(np.argmax(lhs - rhs))
            fails.append(f"{what}: {int(bad.sum())} of {n} elements; worst at {i}: f {f[i]!r}, h {h[i]!r}, m {m[i]!r}, l {lo[i]!r}")
    total = h64 + m64 + l64                                  # exact in fp64
    bad = np.abs(total - U) > 2.0 ** -24 * np.abs(U) + 2.0 ** -45 * S
    if bad.any():
        fails.append(f"h + m + l beyond 2^-24 |U| + 2^-45 S: {int(bad.sum())} of {n} elements; first at {int(np.argmax(bad))}")
    bad = (f != total) & (np.abs(f) >= 2.0 ** -100)
    if bad.any():
        fails.append(f"h + m + l is not exactly f at {int(bad.sum())} of {n} elements; first at {int(np.argmax(bad))}")
    return fails
