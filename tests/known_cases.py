"""Known-region conditioning of one reverse step restated in numpy fp32 -- one rounding per operation, select by mask --
and the seeded cases that the CPU and GPU tests share.  Pure numpy: no torch, no GPU, nothing of the package under test.

Per sample, ti the normalised t and s = ti - 1 (ancestral) or ti - stride (strided):
    u      = the unconditioned update (ancestral: GaussianDiffusion.py:287-288, 314-317; strided: sampler_cases.step in fp32)
    kn     = x0 where s < 0, else ca[s] * x0 + cb[s] * kz          (mul, mul, add)
    x_prev = kn where keep != 0, else u                            (a select)
An out-of-range t, or a stride < 1, makes the whole sample NaN.  The table VALUES are inputs taken as exact (hand in the fp32 device
tables)."""
import itertools

import numpy as np

F = np.float32
T_SMALL, T_BIG = 8, 1000
NS = (1, 3, 4, 5, 1024, 1028)
# The launch is one thread per quad, 256 threads per workgroup, at most 4096 workgroups: the smallest n whose grid-stride loop takes a
# second trip is one quad more than 4096 * 256 quads.
N_SECOND_TRIP = 4 * 256 * 4096 + 4
BATCHES = (1, 3)
MASKS = ("zeros", "ones", "checker", "random")
FORMS = ("tensor", "gauss", "fresh")           # step noise / known noise: both tensors; generated / tensor; both generated
SEED = 0x0123456789ABCDEF


def t_rows(B, T):
    """Timestep rows: 0, 1, T - 1, -1 (= T - 1), -T (= 0), and the out-of-range T and -T - 1, mixed inside a batch of 3."""
    if B == 1:
        return [(0,), (1,), (T - 1,), (-1,), (-T,), (T,), (-T - 1,)]
    return [(0, 1, T - 1), (-1, -T, T), (-T - 1, T - 1, 1)]


def samplers(T):
    """None (ancestral) and (stride, eta): strides 1, 3 and one that passes t = 0 from every timestep, eta 0 and 1."""
    return [None] + [(k, eta) for k in (1, 3, T + 1) for eta in (0.0, 1.0)]


def aux_cases():
    """What is cycled over the base cases, every combination once per cycle: (mask kind, (x0, keep, noise) stride words at n?,
    offset mode 0 none / 1 every fp32 pointer by one float / 2 the keep pointer by one byte, x_prev aliases x_t?, pred_x0 and
    mean_out given?), in a fixed shuffled order."""
    combos = list(itertools.product(MASKS, itertools.product((True, False), repeat=3), (0, 1, 2), (False, True), (True, False)))
    order = np.random.default_rng(20241021).permutation(len(combos))
    return [combos[i] for i in order]


def normalise(t, T):
    """Python-style index -> (index, in range?)."""
    t = int(t)
    t = t + T if t < 0 else t
    return (t, True) if 0 <= t < T else (0, False)


def landing(t, T, stride=1):
    """-> (s, poisoned?): the timestep the step from t lands on; s is -1 for a poisoned sample (nothing is read for it)."""
    ti, ok = normalise(t, T)
    if not ok or stride < 1:
        return -1, True
    return ti - stride, False


def keep_plane(kind, B, n, seed=0):
    """uint8 [B, n]; nonzero bytes are not all 1 (any nonzero value keeps)."""
    if kind == "zeros":
        return np.zeros((B, n), dtype=np.uint8)
    if kind == "ones":
        return np.full((B, n), 1, dtype=np.uint8)
    if kind == "checker":
        return ((np.arange(n)[None, :] + np.arange(B)[:, None]) % 2 * 255).astype(np.uint8)
    rng = np.random.default_rng([77, seed, B, n])
    return (rng.integers(0, 3, size=(B, n)) * rng.integers(1, 128, size=(B, n))).astype(np.uint8)


def inputs(B, n, seed=0):
    """Seeded fp32 (x_t, eps, z, x0, kz), each [B, n]: x_t wide enough that the clamp binds on part of the elements."""
    rng = np.random.default_rng([20241021, seed, B, n])
    x_t = (1.5 * rng.standard_normal((B, n))).astype(F)
    eps, z, kz = (rng.standard_normal((B, n)).astype(F) for _ in range(3))
    x0 = rng.uniform(-1.0, 1.0, (B, n)).astype(F)
    return x_t, eps, z, x0, kz


def strided_coef(acp, ti, stride, eta):
    """The strided step's (c_x0, c_dir, sigma): fp64, each rounded to fp32 once (sampler_cases.coefficients)."""
    s = ti - stride
    a_t, a_s = acp[ti], (1.0 if s < 0 else acp[s])
    var = (float(F(eta)) ** 2) * ((1.0 - a_s) / (1.0 - a_t)) * (1.0 - a_t / a_s)
    return F(np.sqrt(a_s)), F(np.sqrt(max((1.0 - a_s) - var, 0.0))), F(np.sqrt(var))


def update(x_t, eps, z, t, tb, T, sampler=None):
    """The unconditioned update of ONE sample in fp32, one rounding per operation -> (x_prev, pred_x0, mean); all NaN for an
    out-of-range t or a stride < 1.  tb: fp32 tables recip, recipm1, coef1, coef2, sigma and the fp64 acp."""
    x_t, eps = np.asarray(x_t, dtype=F), np.asarray(eps, dtype=F)
    z = np.zeros_like(x_t) if z is None else np.asarray(z, dtype=F)
    ti, ok = normalise(t, T)
    if not ok or (sampler is not None and sampler[0] < 1):
        nan = np.full_like(x_t, np.nan)
        return nan, nan.copy(), nan.copy()
    p = tb["recip"][ti] * x_t
    raw = p - tb["recipm1"][ti] * eps
    pred = np.clip(raw, F(-1.0), F(1.0))
    if sampler is None:
        mean = tb["coef1"][ti] * pred + tb["coef2"][ti] * x_t
        sigma = tb["sigma"][ti] if int(t) != 0 else F(0.0)
        return mean + sigma * z, pred, mean
    c_x0, c_dir, sigma = strided_coef(tb["acp"], ti, *sampler)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(pred == raw, eps, (p - pred) / tb["recipm1"][ti])
    mean = c_x0 * pred + c_dir * e
    return (mean if sigma == 0.0 else mean + sigma * z), pred, mean


def known_step(x_t, eps, z, x0, keep, kz, t, tb, T, sampler=None):
    """The conditioned step of a batch: arrays [B, n] (x0 / keep / kz may be [1, n]: one plane for all samples), t a sequence of B.
    -> (x_prev, pred_x0, mean) fp32 [B, n].  tb as in update() plus ca, cb."""
    B, n = x_t.shape
    out = [np.empty((B, n), dtype=F) for _ in range(3)]
    for b in range(B):
        u, pred, mean = update(x_t[b], eps[b], None if z is None else z[b], t[b], tb, T, sampler)
        s, poisoned = landing(t[b], T, 1 if sampler is None else sampler[0])
        c, k, w = (a[b if a.shape[0] > 1 else 0] for a in (x0, keep, kz))
        if poisoned:
            x_prev = np.full(n, np.nan, dtype=F)
        else:
            kn = c.astype(F) if s < 0 else tb["ca"][s] * c + tb["cb"][s] * w
            x_prev = np.where(k != 0, kn, u)
        out[0][b], out[1][b], out[2][b] = x_prev, pred, mean
    return tuple(out)


def same_bits(a, b):
    """The comparison of the GPU tests: every element bit for bit, a NaN equal to any NaN.  -> bool array."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
