"""The strided sampler restated in fp64 numpy -- one step and a whole chain -- and the seeded inputs that the CPU and
GPU tests share.  Pure numpy: no torch, no GPU, nothing of the package under test.

One step from t to s = t - stride (Song et al., "Denoising Diffusion Implicit Models", eq. 12 / 16), a_s = 1 for s < 0:
    var   = eta^2 (1 - a_s) / (1 - a_t) (1 - a_t / a_s);  c_x0 = sqrt(a_s);  c_dir = sqrt(max(1 - a_s - var, 0));  sigma = sqrt(var)
    p = c_recip[t] x_t;  q = c_recipm1[t] eps;  x0 = clamp(p - q, -1, 1)
    e' = eps where the clamp did not bind, (p - x0) / c_recipm1[t] where it did
    mean = c_x0 x0 + c_dir e';  x_prev = mean + sigma z (sigma != 0) or mean (sigma == 0)
The c_recip / c_recipm1 table VALUES are inputs taken as exact: hand in the kernel's fp32 tables to predict the kernel, the
fp64 tables to check identities."""
import numpy as np

T = 100
SHAPES = [(3, 5), (3, 37, 41), (3, 1, 64, 64)]                  # scalar tail, odd n, float4
T_ROWS = [(0, 4, 5), (T - 1, -1, 57), (30, T + 2, 7)]            # the last row holds the out-of-range entry (sample 1)
BAD = {2: 1}                                                     # row index -> the sample that is out of range
STRIDES = [1, 5, T + 3]
ETAS = [0.0, 0.5, 1.0]
CHAINS = [(23, 5), (99, 7), (50, 50), (10, 64)]                  # (t_distance, stride)


def betas():
    """The package's "linear" schedule at T = 100, restated (1000 / T * [1e-4, 2e-2])."""
    k = 1000.0 / T
    return np.linspace(k * 0.0001, k * 0.02, T, dtype=np.float64)


def alphas_cumprod():
    return np.cumprod(1.0 - betas())


def recip_tables(acp, dtype=np.float64):
    """sqrt(1 / a), sqrt(1 / a - 1): in fp64, or rounded to fp32 as the device tables are."""
    return np.sqrt(1.0 / acp).astype(dtype), np.sqrt(1.0 / acp - 1.0).astype(dtype)


def normalise(t, n=T):
    """Python-style index -> (index, in range?)."""
    t = int(t)
    t = t + n if t < 0 else t
    return (t, True) if 0 <= t < n else (0, False)


def coefficients(acp, t, stride, eta):
    """(c_x0, c_dir, sigma, var) of the step that leaves the normalised timestep t, fp64."""
    s = t - stride
    a_t, a_s = acp[t], (1.0 if s < 0 else acp[s])
    var = (eta * eta) * ((1.0 - a_s) / (1.0 - a_t)) * (1.0 - a_t / a_s)
    return np.sqrt(a_s), np.sqrt(max((1.0 - a_s) - var, 0.0)), np.sqrt(var), var


def step(x_t, eps, z, t, stride, eta, acp, c_recip, c_recipm1):
    """One step of ONE sample (t: its normalised timestep) -> dict of every intermediate, fp64 arrays shaped like x_t.  `z` may
    be None (no noise term)."""
    x_t, eps = np.asarray(x_t, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    c_x0, c_dir, sigma, var = coefficients(acp, t, stride, eta)
    r, m = float(c_recip[t]), float(c_recipm1[t])
    p, q = r * x_t, m * eps
    raw = p - q
    x0 = np.clip(raw, -1.0, 1.0)
    bound = raw != x0
    e = np.where(bound, (p - x0) / m, eps)
    mean = c_x0 * x0 + c_dir * e
    noise = sigma * np.asarray(z, dtype=np.float64) if (sigma != 0.0 and z is not None) else np.zeros_like(mean)
    return dict(c_x0=c_x0, c_dir=c_dir, sigma=sigma, var=var, recipm1=m, p=p, q=q, raw=raw, x0=x0, bound=bound, e=e, mean=mean,
                noise=noise, x_prev=mean + noise if sigma != 0.0 else mean)


def error_bound(r):
    """The per-element bound on |kernel - restatement| of x_prev for fp32 element arithmetic, from the intermediates of step():
        2^-23 [(c_x0 + 2 c_dir / c_recipm1) (|p| + |q|) + 2.5 (|c_x0 x0| + |c_dir e'| + |sigma z|)]
    Two roundings (the products p and q) reach p - q, which rounds once more: at most 2^-23 (|p| + |q|).  The clamp is
    1-Lipschitz, so x0 carries that error times c_x0.  e' costs at most two such errors over c_recipm1 (the difference p - x0 and
    the quotient), times c_dir; c_dir / c_recipm1 <= sqrt(a_t) <= 1, so the term stays of the size of the first.  The same holds
    where the fp32 and the fp64 clamp decide differently: both forms of e' agree at the boundary.  One rounding each goes to the
    fp32 coefficients, the three products and the two sums: 5 x 2^-24 = 2.5 x 2^-23 of each term's magnitude."""
    return 2.0 ** -23 * ((r["c_x0"] + 2.0 * r["c_dir"] / r["recipm1"]) * (np.abs(r["p"]) + np.abs(r["q"])) +
                         2.5 * (np.abs(r["c_x0"] * r["x0"]) + np.abs(r["c_dir"] * r["e"]) + np.abs(r["noise"])))


def visited(t_distance, stride):
    """Timesteps a chain visits: t_distance - 1, t_distance - 1 - stride, ... >= 0."""
    return list(range(int(t_distance) - 1, -1, -int(stride)))


def chain(x_start, eps_fn, t_distance, stride, eta, acp, c_recip, c_recipm1, z_fn=None):
    """A whole chain of one sample: eps_fn(x, t) is the model, z_fn(t) the step noise (None: none).  -> (x, timesteps visited)."""
    x = np.asarray(x_start, dtype=np.float64)
    ts = visited(t_distance, stride)
    for t in ts:
        x = step(x, eps_fn(x, t), z_fn(t) if z_fn else None, t, stride, eta, acp, c_recip, c_recipm1)["x_prev"]
    return x, ts


def inputs(shape, row):
    """Seeded (x_t, eps, z) for T_ROWS[row], float32 arrays of `shape`.  Sample b is x_t = sqrt(a_t) x0 + sqrt(1 - a_t) eps with
    x0 = 2 U(-1, 1), eps and z ~ N(0, 1), t = its normalised timestep: the predicted x_0 is then x0 up to rounding at every t, so
    the clamp binds on about half of the elements and is slack on the rest whatever the noise level (with x_t itself drawn as
    2 U(-1, 1) the clamp binds on 92 % of the elements at t = 57 and 99.8 % at t = T - 1)."""
    acp = alphas_cumprod()
    rng = np.random.default_rng([20240919, row, int(np.prod(shape))])
    x0 = 2.0 * rng.uniform(-1.0, 1.0, size=shape)
    eps = rng.standard_normal(size=shape).astype(np.float32)
    z = rng.standard_normal(size=shape).astype(np.float32)
    x_t = np.empty(shape, dtype=np.float32)
    for b, t in enumerate(T_ROWS[row]):
        a = acp[normalise(t)[0]]
        x_t[b] = (np.sqrt(a) * x0[b] + np.sqrt(1.0 - a) * eps[b].astype(np.float64)).astype(np.float32)
    return x_t, eps, z


def reference(shape, row, stride, eta, with_noise=True):
    """step() of every in-range sample of inputs(shape, row) with the fp32 tables -> list over b (None: out of range)."""
    acp = alphas_cumprod()
    c_recip, c_recipm1 = recip_tables(acp, np.float32)
    x_t, eps, z = inputs(shape, row)
    out = []
    for b, t in enumerate(T_ROWS[row]):
        ti, ok = normalise(t)
        out.append(step(x_t[b], eps[b], z[b] if with_noise else None, ti, stride, eta, acp, c_recip, c_recipm1) if ok else None)
    return out
