"""`GaussianDiffusionModel` & friends -- the reference diffusion process (GaussianDiffusion.py)
driven from PyTorch-ROCm host code with the arithmetic in fused HIP kernels.

Kept from the reference (names, signatures, return structures, RNG consumption order):
  get_beta_schedule, extract, mean_flat, normal_kl, approx_standard_normal_cdf,
  discretised_gaussian_log_likelihood, generate_simplex_noise, random_noise,
  GaussianDiffusionModel.{sample_t_with_weights, predict_x_0_from_eps, predict_eps_from_x_0,
  q_mean_variance, q_posterior_mean_variance, p_mean_variance, sample_p, forward_backward,
  sample_q, sample_q_gradual, calc_vlb_xt, calc_loss, p_loss, prior_vlb, calc_total_vlb,
  detection_A_fixedT} plus the north-star aliases q_sample / p_sample_loop.

What changed underneath (MI355X-first):
  * the 14 fp64 schedule tables are built exactly as GaussianDiffusion.py:184-217 and uploaded
    ONCE per device as fp32 (the reference uploads an 8 KB table 8x per step, :32-36);
  * sample_q is one kernel (12 B/pixel), the whole reverse update of sample_p -- predict x0, clamp,
    posterior mean, sigma*noise -- is one kernel (16 B/pixel) instead of ~25 dispatches;
  * simplex noise is generated on the GPU straight into the noise tensor (no D2H of t, no numba,
    no H2D), seeded from the global numpy stream exactly like Simplex_CLASS.newSeed();
  * forward_backward keeps `t` on the device and, for the built-in UNetModel, replays one captured
    HIP graph per reverse step.

All tensors must live on a HIP device: there is no CPU fallback (CPU tensors raise AnoddpmError).
"""
import ctypes
import random

import numpy as np
import torch

from . import _lib, philox
from ._lib import KnownArgs, LossArgs, PUpdateArgs, ResamplingArgs, VlbArgs, check, current_stream, lib, ptr
from .simplex import Simplex_CLASS, perm_tables

__all__ = ["SimplexNoiseFn", "GaussNoiseFn", "ReverseChain", "StridedSampler", "KnownRegion", "Resampling", "get_beta_schedule", "extract", "mean_flat", "normal_kl", "approx_standard_normal_cdf",
           "discretised_gaussian_log_likelihood", "generate_simplex_noise", "random_noise",
           "GaussianDiffusionModel"]

_RANDOM_PARAMS = [(2, 0.6, 16), (6, 0.6, 32), (7, 0.7, 32), (10, 0.8, 64), (5, 0.8, 16), (4, 0.6, 16),
                  (1, 0.6, 64), (7, 0.8, 128), (6, 0.9, 64), (2, 0.85, 128), (2, 0.85, 64), (2, 0.85, 32),
                  (2, 0.85, 16), (2, 0.85, 8), (2, 0.85, 4), (2, 0.85, 2), (1, 0.85, 128), (1, 0.85, 64),
                  (1, 0.85, 32), (1, 0.85, 16), (1, 0.85, 8), (1, 0.85, 4), (1, 0.85, 2)]


def get_beta_schedule(num_diffusion_steps, name="cosine"):
    """GaussianDiffusion.py:12-29 (host, fp64)."""
    if name == "cosine":
        def abar(u):
            return np.cos((u + 0.008) / 1.008 * np.pi / 2) ** 2
        n = num_diffusion_steps
        return np.array([min(1 - abar((i + 1) / n) / abar(i / n), 0.999) for i in range(n)])
    if name == "linear":
        k = 1000 / num_diffusion_steps
        return np.linspace(k * 0.0001, k * 0.02, num_diffusion_steps, dtype=np.float64)
    raise NotImplementedError(f"unknown beta schedule: {name}")


def extract(arr, timesteps, broadcast_shape, device):
    """GaussianDiffusion.py:32-36: gather in fp64, then cast to fp32, broadcast to `broadcast_shape`."""
    res = torch.from_numpy(np.asarray(arr)).to(device=timesteps.device)[timesteps].float()
    return res.reshape(res.shape + (1,) * (len(broadcast_shape) - res.dim())).expand(broadcast_shape).to(device)


def mean_flat(tensor):
    """GaussianDiffusion.py:39-40: mean over everything but the batch dimension."""
    if tensor.dim() < 2:
        return torch.mean(tensor, dim=[])                        # what the reference's empty dim list does
    return tensor.reshape(tensor.shape[0], -1).mean(dim=1)


def normal_kl(mean1, logvar1, mean2, logvar2):
    """KL(N(mean1, e^logvar1) || N(mean2, e^logvar2)) in nats, elementwise (GaussianDiffusion.py:43-53).  API surface only: the
    training / logging paths evaluate this inside anoddpm_vlb_terms / anoddpm_loss_forward."""
    dl = logvar2 - logvar1
    return 0.5 * (dl - 1.0 + torch.exp(-dl) + torch.exp(-logvar2) * (mean1 - mean2) ** 2)


_SQRT_2_OVER_PI = float(np.sqrt(2.0 / np.pi))


def approx_standard_normal_cdf(x):
    """tanh approximation of the standard normal CDF (GaussianDiffusion.py:56-61)."""
    return 0.5 * (1.0 + torch.tanh(_SQRT_2_OVER_PI * (x + 0.044715 * x * x * x)))


def discretised_gaussian_log_likelihood(x, means, log_scales):
    """log-likelihood of a Gaussian discretised to 8-bit bins of width 2/255 on [-1, 1], open-ended at +-1
    (GaussianDiffusion.py:64-93).  API surface only (see normal_kl)."""
    if not (x.shape == means.shape == log_scales.shape):
        raise AssertionError("discretised_gaussian_log_likelihood: shape mismatch")
    z = torch.exp(-log_scales)
    upper = approx_standard_normal_cdf(z * (x - means + 1.0 / 255.0))
    lower = approx_standard_normal_cdf(z * (x - means - 1.0 / 255.0))
    floor = 1e-12
    inner = torch.log((upper - lower).clamp(min=floor))
    left = torch.log(upper.clamp(min=floor))                     # x at the lower edge: everything below counts
    right = torch.log((1.0 - lower).clamp(min=floor))            # x at the upper edge: everything above counts
    return torch.where(x < -0.999, left, torch.where(x > 0.999, right, inner))


def generate_simplex_noise(Simplex_instance, x, t, random_param=False, octave=6, persistence=0.8, frequency=64,
                           in_channels=1):
    """GaussianDiffusion.py:96-137 on the device.

    Per channel: a fresh seed from the global numpy stream (newSeed), then the multi-octave field at
    z = t written as fp32 into noise[:, i].  `random_param=True` draws `random.choice` like the
    reference does; the reference then overwrites that field with the default-parameter one
    (:125-136 has no else), so only the RNG draw is observable and only it is reproduced.
    Batch > 1: sample b gets the field at z = t[b] (all equal inside forward_backward, which is the
    reference's `.repeat(B,1,1,1)` behaviour); the reference itself only runs at batch 1.
    """
    _lib.require_cuda(x, "generate_simplex_noise")
    noise = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    for i in range(in_channels):
        Simplex_instance.newSeed()
        if random_param:
            random.choice(_RANDOM_PARAMS)
        Simplex_instance.fill_fixed_T_octaves_(noise, t, octave, persistence, frequency, channel=i)
    return noise


def random_noise(Simplex_instance, x, t):
    """GaussianDiffusion.py:140-147."""
    if random.choice(["gauss", "simplex"]) == "gauss":
        return torch.randn_like(x)
    return generate_simplex_noise(Simplex_instance, x, t)


class SimplexNoiseFn:
    """A `denoise_fn` / `noise_fn` callable equivalent to
    `lambda x, t: generate_simplex_noise(simplex, x, t, False, octave, persistence, frequency, in_channels)`
    that the reverse chain can recognise: its seeds are then drawn up front (same numpy-stream order,
    one per step per channel) and the permutation tables of all steps are uploaded once."""

    def __init__(self, simplex, octave=6, persistence=0.8, frequency=64, in_channels=1):
        self.simplex, self.octave, self.persistence, self.frequency, self.in_channels = \
            simplex, octave, persistence, frequency, in_channels

    def __call__(self, x, t):
        return generate_simplex_noise(self.simplex, x, t, False, self.octave, self.persistence, self.frequency,
                                      self.in_channels)


class GaussNoiseFn:
    """The `noise_fn` of a noise="gauss" model, and the one detection_B installs: `lambda x, t: torch.randn_like(x)` until the
    owner is seeded (GaussianDiffusionModel.seed_gauss); then the counter-based stream of DESIGN 9g in the forward-noise domain,
    one fresh stream id per sample, step = t.  An object (not a lambda) so that a deep copy follows its own owner's seed and so
    that `_run_chains` can recognise it and generate the forward noise inside the q-sample kernel."""

    def __init__(self, owner):
        self.owner = owner

    def __call__(self, x, t):
        if self.owner.gauss_seed is None:
            return torch.randn_like(x)
        return self.owner._seeded_normal(x, t, _lib.PHILOX_FORWARD)


class StridedSampler:
    """Opt-in reverse sampler that strides over timesteps (Song et al., "Denoising Diffusion Implicit Models", eq. 12 and 16;
    DESIGN 9h); immutable.  `stride` >= 1: a step goes from t to t - stride, so a chain of t_distance d visits d-1, d-1-stride, ...
    and takes ceil(d / stride) steps; the step that would pass t = 0 lands on the predicted x_0.  `eta` in [0, 1] scales the step
    noise; 0 is deterministic.  The UNet sees the original timestep values, so a trained checkpoint is used as it is.

    This is a DIFFERENT sampler, not a faster spelling of the reference's: at stride 1, eta 1 the mean is algebraically the
    reference's posterior mean, but the variance is the posterior variance, not the reference's fixed-large `model_variance`.
    What a stride does to detection quality (AUC, Dice) has not been measured."""
    __slots__ = ("stride", "eta")

    def __init__(self, stride, eta=0.0):
        if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or stride < 1 or stride > 2 ** 31 - 1:
            raise ValueError(f"StridedSampler: stride must be an integer >= 1, got {stride!r}")
        if isinstance(eta, bool) or not isinstance(eta, (int, float, np.integer, np.floating)) or not 0.0 <= eta <= 1.0:
            raise ValueError(f"StridedSampler: eta must be a number in [0, 1], got {eta!r}")
        object.__setattr__(self, "stride", int(stride))
        object.__setattr__(self, "eta", float(eta))

    @classmethod
    def parse(cls, text):
        """"<stride>[,<eta>]", the form of the ANODDPM_SAMPLER environment variable."""
        parts = [p.strip() for p in str(text).split(",")]
        try:
            if not 1 <= len(parts) <= 2:
                raise ValueError
            return cls(int(parts[0], 10), float(parts[1]) if len(parts) == 2 else 0.0)
        except ValueError:
            raise ValueError(f"ANODDPM_SAMPLER={text!r}: expected '<stride>[,<eta>]' with an integer stride >= 1 and "
                             "0 <= eta <= 1") from None

    def steps(self, t_distance):
        """Reverse steps of a chain of `t_distance` timesteps: ceil(t_distance / stride)."""
        return -(-int(t_distance) // self.stride)

    def timesteps(self, t_distance):
        """The timesteps such a chain visits: t_distance - 1, t_distance - 1 - stride, ... down to the last one >= 0."""
        return list(range(int(t_distance) - 1, -1, -self.stride))

    def __setattr__(self, name, value):
        raise AttributeError("StridedSampler is immutable")

    def __delattr__(self, name):
        raise AttributeError("StridedSampler is immutable")

    def _key(self):
        return (self.stride, self.eta)

    def __eq__(self, other):
        return isinstance(other, StridedSampler) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"StridedSampler(stride={self.stride!r}, eta={self.eta!r})"

    def __reduce__(self):
        return StridedSampler, self._key()


def _check_sampler(sampler):
    if sampler is not None and not isinstance(sampler, StridedSampler):
        raise TypeError(f"sampler must be None or a StridedSampler, got {type(sampler).__name__}")
    return sampler


class KnownRegion:
    """Opt-in known-region conditioning of the reverse chain (RePaint, Lugmayr et al., CVPR 2022, Algorithm 1 / eq. 8; the
    "stitch" of AutoDDPM, Bercea et al., 2023); immutable.  At the step from t to s (t - 1, or t - stride) the pixels
    marked in `keep` leave the step as `x_0` noised to s -- `x_0` itself once s < 0 -- and every other pixel as the ordinary update;
    both happen in the one fused update launch.
      x_0    [B or 1, C, H, W], stored as fp32
      keep   [B or 1, C or 1, H, W], any dtype: stored as bytes `!= 0`, broadcast over the channels here, once
      noise  "fixed": one plane per sample for the whole chain -- the chain's forward noise (forward_backward hands over the one
             it noised `x` with; a chain built directly draws `noise_fn(x_0, t_distance - 1)` once);
             "fresh": a new draw per step, made inside the kernel from the seeded stream (domain 3): seeded owners only;
             a tensor [B or 1, C, H, W]: that plane, as "fixed".
    A hard select.  Resampling jumps are a `Resampling` handed over next to it; the slot-batched detection sweeps take one through
    `_run_chains(known=)` / the `detection_keep` attribute.  What it does to detection quality has not been measured."""
    __slots__ = ("x_0", "keep", "noise")

    def __init__(self, x_0, keep, noise="fixed"):
        if not torch.is_tensor(x_0) or x_0.dim() != 4 or not x_0.is_floating_point():
            raise ValueError("KnownRegion: x_0 must be a floating-point tensor [B or 1, C, H, W]")
        C, H, W = x_0.shape[1:]
        if not torch.is_tensor(keep) or keep.dim() != 4 or tuple(keep.shape[2:]) != (H, W) or keep.shape[1] not in (1, C):
            raise ValueError(f"KnownRegion: keep must be [B or 1, C or 1, {H}, {W}] for x_0 {tuple(x_0.shape)}, got "
                             f"{tuple(keep.shape) if torch.is_tensor(keep) else type(keep).__name__}")
        if torch.is_tensor(noise):
            if noise.dim() != 4 or tuple(noise.shape[1:]) != (C, H, W):
                raise ValueError(f"KnownRegion: a noise tensor must be [B or 1, {C}, {H}, {W}], got {tuple(noise.shape)}")
            noise = noise.detach().to(device=x_0.device, dtype=torch.float32).contiguous()
        elif noise not in ("fixed", "fresh"):
            raise ValueError(f"KnownRegion: noise must be 'fixed', 'fresh' or a tensor, got {noise!r}")
        object.__setattr__(self, "x_0", x_0.detach().float().contiguous())
        object.__setattr__(self, "keep", (keep.detach().to(x_0.device) != 0).expand(keep.shape[0], C, H, W).to(torch.uint8).contiguous())
        object.__setattr__(self, "noise", noise)

    @property
    def mode(self):
        """"fresh", or "fixed" for everything that is one plane per sample (a tensor included): what a captured step depends on."""
        return "fresh" if isinstance(self.noise, str) and self.noise == "fresh" else "fixed"

    def check_batch(self, shape):
        """The planes fit a chain / step of batch shape `shape`: the same image shape, batch 1 or `shape[0]` each."""
        for name, p in (("x_0", self.x_0), ("keep", self.keep), ("noise", self.noise)):
            if torch.is_tensor(p) and (tuple(p.shape[1:]) != tuple(shape[1:]) or p.shape[0] not in (1, shape[0])):
                raise ValueError(f"KnownRegion: {name} {tuple(p.shape)} does not fit a batch of shape {tuple(shape)}")

    def __setattr__(self, name, value):
        raise AttributeError("KnownRegion is immutable")

    def __delattr__(self, name):
        raise AttributeError("KnownRegion is immutable")

    def __repr__(self):
        noise = self.noise if isinstance(self.noise, str) else f"tensor{tuple(self.noise.shape)}"
        return f"KnownRegion(x_0={tuple(self.x_0.shape)}, keep={tuple(self.keep.shape)}, noise={noise!r})"


def _check_known(known):
    if known is not None and not isinstance(known, KnownRegion):
        raise TypeError(f"known must be None or a KnownRegion, got {type(known).__name__}")
    return known


class Resampling:
    """Opt-in resampling jumps of a conditioned reverse chain (RePaint, Lugmayr et al., CVPR 2022, Algorithm 1);
    immutable.  `jump` >= 1: the length of a jump; `reps` >= 1: how often each segment is sampled (1: no resampling).  A chain that
    starts at level top = t_distance - 1 has a jump point at every level p >= 0 with p % jump == 0 and p + jump <= top.  The update
    that lands on a jump point with repetitions left re-noises its image back up to p + jump -- q(x_{p+jump} | x_p), every pixel --
    and the chain comes down the same `jump` levels again, `reps` times in all, each pass with its own noise (the pass count,
    `visit`, is part of the Philox domain).  The device decides and carries out the jump per sample, inside the fused update
    launch (anoddpm_p_sample_update_resample) and its advance launch.  Only with a KnownRegion, only the ancestral sampler, only
    gaussian step noise.  What it does to detection quality has not been measured."""
    __slots__ = ("jump", "reps")

    def __init__(self, jump, reps):
        for name, v in (("jump", jump), ("reps", reps)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 or v > 2 ** 31 - 1:
                raise ValueError(f"Resampling: {name} must be an integer >= 1, got {v!r}")
        object.__setattr__(self, "jump", int(jump))
        object.__setattr__(self, "reps", int(reps))

    @classmethod
    def parse(cls, text):
        """"<jump>,<reps>", the form of the ANODDPM_RESAMPLE environment variable."""
        parts = [p.strip() for p in str(text).split(",")]
        try:
            if len(parts) != 2:
                raise ValueError
            return cls(int(parts[0], 10), int(parts[1], 10))
        except ValueError:
            raise ValueError(f"ANODDPM_RESAMPLE={text!r}: expected '<jump>,<reps>' with two integers >= 1") from None

    def steps(self, t_distance):
        """UNet evaluations of a chain of `t_distance` timesteps: every jump point adds (reps - 1) passes over `jump` levels."""
        L = int(t_distance)
        return L + ((L - 1) // self.jump) * (self.reps - 1) * self.jump if L >= 1 else 0

    def timesteps(self, t_distance):
        """[(ti, land, visit)] of every evaluation, in order: the level the UNet sees, the level the update leaves the image at
        (-1: the clean image) and the visit index the step's noise is drawn with.  Written segment by segment, from the highest
        jump point down; the device runs the same schedule as a per-sample state machine (anoddpm_chain_advance_resample)."""
        top, J = int(t_distance) - 1, self.jump
        out, cur, visit = [], top, 0
        for p in range(((top - J) // J) * J if top >= J else -1, -1, -J):
            for r in range(self.reps):
                jumps = r < self.reps - 1
                for ti in range(cur, p, -1):
                    out.append((ti, p + J if jumps and ti - 1 == p else ti - 1, visit))
                visit += jumps
                cur = p + J if jumps else p
        out.extend((ti, ti - 1, visit) for ti in range(cur, -1, -1))
        return out

    def __setattr__(self, name, value):
        raise AttributeError("Resampling is immutable")

    def __delattr__(self, name):
        raise AttributeError("Resampling is immutable")

    def _key(self):
        return (self.jump, self.reps)

    def __eq__(self, other):
        return isinstance(other, Resampling) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"Resampling(jump={self.jump!r}, reps={self.reps!r})"

    def __reduce__(self):
        return Resampling, self._key()


def _check_resampling(resampling):
    if resampling is not None and not isinstance(resampling, Resampling):
        raise TypeError(f"resampling must be None or a Resampling, got {type(resampling).__name__}")
    return resampling


def plan_chain_slots(lengths, slots):
    """Longest-first list schedule of reverse chains on `slots` chain slots (host logic of `_run_chains`).

    lengths[i] > 0: steps of chain i.  Returns (makespan, [(slot, first_step), ...] per chain): a chain occupies one slot for
    `lengths[i]` consecutive global steps; a freed slot takes the longest pending chain.  makespan <= ceil(sum / slots) + max - 1
    (Graham's bound for list scheduling), and with the detection sweeps' lengths the slots end within one short chain of each other."""
    import heapq
    if slots < 1:
        raise ValueError("plan_chain_slots: slots must be >= 1")
    if any(int(l) <= 0 for l in lengths):
        raise ValueError("plan_chain_slots: chain lengths must be positive")
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    free = [(0, s) for s in range(slots)]
    heapq.heapify(free)
    place = [None] * len(lengths)
    makespan = 0
    for i in order:
        t0, slot = heapq.heappop(free)
        place[i] = (slot, t0)
        t1 = t0 + int(lengths[i])
        makespan = max(makespan, t1)
        heapq.heappush(free, (t1, slot))
    return makespan, place


def choose_slots(steps, n, per_slot_bytes, free_bytes):
    """Slot count of an automatic sweep of `n` chains of `steps` reverse steps (zeros ignored); the caller clamps it to `n`.  A batched
    step costs about (2 + G) image-units (a batch-independent floor worth two images): the slot count among the
    quantisation-free sizes whose longest-first schedule is cheapest -- and whose plan fits: a slot costs `per_slot_bytes` (the activation
    buffers of one image: about 0.8 GB at 256^2 / base 128; 512^2 models at batch 16 are 50 GB), and sizes that would take more than
    half of `free_bytes`, the free device memory, are skipped."""
    pos = [l for l in steps if l > 0] or [1]
    cands = [g for g in (16, 12, 8) if g <= max(n, 8) and (g == 8 or g * per_slot_bytes <= 0.5 * free_bytes)]
    while cands[-1] > 1 and cands[-1] * per_slot_bytes > 0.5 * free_bytes:
        cands.append(cands[-1] // 2)                                 # even eight images do not fit: 4, 2, 1 slots
    cands = [g for g in cands if g * per_slot_bytes <= 0.5 * free_bytes] or [1]
    return min(cands, key=lambda g: plan_chain_slots(pos, min(g, len(pos)))[0] * (2 + min(g, len(pos))))


def slot_events(place, steps, slots):
    """What the stepping loop does at each global step of a `plan_chain_slots` schedule; steps[i]: length of chain i.
    -> (refill {step: [(slot, i)]}: chains that start, harvest {step: [(slot, i)]}: chains that take their last step,
    last_busy[slot]: the first global step at which the slot has nothing left to do, 0 for a slot without a chain)."""
    refill, harvest, last_busy = {}, {}, [0] * slots
    for i, (slot, start) in enumerate(place):
        refill.setdefault(start, []).append((slot, i))
        harvest.setdefault(start + steps[i] - 1, []).append((slot, i))
        last_busy[slot] = max(last_busy[slot], start + steps[i])
    return refill, harvest, last_busy


class ReverseChain:
    """Device-resident state of the reverse loop (GaussianDiffusion.py:351-357): x, t and a step counter
    live in HBM; one step = model forward + noise + ONE fused update launch + t -= 1.  With a `sampler` (StridedSampler) the
    update is the strided one, t -= stride (floored at 0), and `remaining` counts ceil(t_distance / stride) steps.  With `known`
    (KnownRegion) the update is the conditioned one; the image, the keep bytes and the fixed noise live in static
    buffers of the chain, so a kept graph follows the `known` of every reset().  With `resampling` (Resampling) the
    conditioned update also carries out the schedule's jumps: `t` is then not monotone, the per-sample state (top, rep, visit) and
    the two schedule words live in static buffers, and `remaining` counts UNet evaluations.  `shared_planes`: the image and the
    keep bytes are ONE plane for the whole batch (the slot-batched sweep of one image)."""

    def __init__(self, owner, model, x, t_distance, denoise_fn, use_graph=None, stream_base=None, sampler=None, known=None,
                 resampling=None, shared_planes=False):
        """Everything a chain allocates, once; `_start` (shared with reset()) then begins the chain itself."""
        _lib.require_cuda(x, "ReverseChain")
        self.owner, self.model, self.denoise_fn = owner, model, denoise_fn
        import os
        self.graph = None
        self._graph_state = 0          # 0: next step eager (warm-up), 1: capture, 2: replay
        self.B = x.shape[0]
        self.x = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        self.t = torch.empty((self.B,), device=x.device, dtype=torch.int64)
        self.step_idx = torch.empty(1, device=x.device, dtype=torch.int32)
        self.sampler = _check_sampler(sampler)
        # a train()-mode model with dropout draws a fresh mask per forward from the host generator (UNet.py:192): it goes
        # through model.forward (eager), not through the captured inference plan
        self.hip_model = hasattr(model, "forward_hip") and not self._draws_dropout(model)
        self._plan = None              # the inference plan a captured graph points into (set at capture)
        self.noise = None
        self.tables = None
        # Which noise sources may run inside a captured HIP graph: device-side philox draws ("gauss" / "random":
        # torch.randn_like registers its generator state with the capture) and SimplexNoiseFn, whose per-step seeds are
        # drawn up front and whose tables are selected by the device-resident step counter.  Anything else -- a plain
        # callable, a user-replaced `noise_fn`, the randParam / random mixtures -- draws from numpy / `random` on the
        # host every step (newSeed(), GaussianDiffusion.py:102) and uploads a table: captured once, every replay
        # would reuse the first step's seed.  Those run eagerly.
        fn, capture_safe = self._resolve_noise(owner, denoise_fn)
        if isinstance(fn, SimplexNoiseFn):
            self.simplex_fn = fn
            self.noise = torch.empty_like(self.x)
            # room for the permutation tables of a full-length chain, so that reset() can start another chain on the same buffers
            self.tables = torch.empty((owner.num_timesteps * fn.in_channels, 512), dtype=torch.int16, device=x.device)
        self.resampling = self._check_resample_request(owner, denoise_fn, sampler, known, resampling)
        self.reuse_key = self._reuse_key_of(owner, denoise_fn, sampler, known, resampling, shared_planes)
        self.capture_safe = capture_safe
        # known-region conditioning: static planes, allocated here and copied into by _start, never inside a capture
        self.known_mode = self._known_mode_of(owner, denoise_fn, known)
        self.k_x0 = self.k_keep = self.k_noise = None
        self.shared_planes = bool(shared_planes) and self.known_mode is not None
        if self.known_mode is not None:
            plane = (1,) + tuple(x.shape[1:]) if self.shared_planes else tuple(x.shape)
            self.k_x0 = torch.empty(plane, device=x.device, dtype=torch.float32)
            self.k_keep = torch.empty(plane, device=x.device, dtype=torch.uint8)
            if self.known_mode == "fixed":
                self.k_noise = torch.empty_like(self.x)
        # resampling: the per-sample state and the two schedule words, written by _start (and by the sweep's refills), read by the
        # update launch, advanced by anoddpm_chain_advance_resample alone
        self.rs_top = self.rs_rep = self.rs_visit = self.rs_jump = self.rs_reps = None
        if self.resampling is not None:
            self.rs_top, self.rs_rep, self.rs_visit = (torch.empty((self.B,), dtype=torch.int32, device=x.device) for _ in range(3))
            self.rs_jump, self.rs_reps = (torch.empty(1, dtype=torch.int32, device=x.device) for _ in range(2))
            owner._sampler_words(x.device, None)                    # the fp64 alphas_cumprod table: allocated now
        # A seeded owner's gaussian step noise is generated inside the update kernel: no noise buffer, no ATen launch.
        # The kernel reads the seed and this chain's per-sample stream ids from device memory, so a kept graph follows
        # seed_gauss() and every reset() / slot refill without a recapture.
        self.streams = None
        if self._seeded_gauss(owner, fn, capture_safe):
            self.streams = torch.empty((self.B,), dtype=torch.int32, device=x.device)
            owner._gauss_seed_dev(x.device)                         # allocated now, not inside a capture
        self._start(x, t_distance, stream_base, known)
        # HIP-graph replay of the step: on by default for the built-in UNetModel (every launch of a step is
        # stream-ordered, allocation-free C-ABI work) with a capture-safe noise source; ANODDPM_NO_GRAPH=1 forces
        # eager launches.  An explicit use_graph=True with an unsafe noise source is refused, not silently wrong.
        if use_graph is None:
            use_graph = self.hip_model and capture_safe and os.environ.get("ANODDPM_NO_GRAPH", "0") != "1"
        elif use_graph and not capture_safe:
            raise ValueError("ReverseChain(use_graph=True): this denoise_fn draws host-side random numbers every step "
                             "and cannot be replayed from a captured graph; pass a SimplexNoiseFn or 'gauss'")
        elif use_graph and not self.hip_model:
            # a train()-mode dropout model seeds its masks on the host per forward: captured once, every replay would repeat
            # the first step's mask; a foreign callable's launches are not known to be capture-safe at all
            raise ValueError("ReverseChain(use_graph=True): the model is not the built-in UNetModel in a dropout-free "
                             "mode (model.eval(), or dropout == 0); its forward cannot be replayed from a captured graph")
        self.use_graph = bool(use_graph)

    @staticmethod
    def _draws_dropout(model):
        return bool(getattr(model, "training", False) and getattr(model, "dropout", 0) > 0)

    @staticmethod
    def _resolve_noise(owner, denoise_fn):
        """-> (SimplexNoiseFn or the original denoise_fn, capture_safe): how the reverse loop's noise request is served."""
        fn = denoise_fn
        capture_safe = False
        if type(fn) == str:
            if fn in ("gauss", "random"):
                capture_safe = True
            elif fn == "noise_fn":
                nf = owner.noise_fn
                if isinstance(nf, SimplexNoiseFn):
                    fn = nf
                elif nf is getattr(owner, "_default_noise_fn", None) and owner.noise_kind == "gauss":
                    capture_safe = True                                      # torch.randn_like
                elif nf is getattr(owner, "_default_noise_fn", None) and owner.noise_kind not in ("simplex_randParam", "random"):
                    fn = SimplexNoiseFn(owner.simplex, in_channels=owner.img_channels)      # :179-181 defaults
            else:
                fn = SimplexNoiseFn(owner.simplex, in_channels=owner.img_channels)          # :310 defaults
        if isinstance(fn, SimplexNoiseFn):
            capture_safe = True
        return fn, capture_safe

    @staticmethod
    def _seeded_gauss(owner, fn, capture_safe):
        """The resolved noise request is the gaussian one ("gauss", "random", a gauss model's own "noise_fn") of a seeded owner."""
        return capture_safe and not isinstance(fn, SimplexNoiseFn) and getattr(owner, "gauss_seed", None) is not None

    @staticmethod
    def _known_mode_of(owner, denoise_fn, known):
        """None, "fixed" or "fresh": which conditioned launch serves `known` for this noise request.  "fresh" is generated inside
        the kernel from the seeded stream, so it is refused for anything else."""
        if _check_known(known) is None:
            return None
        if known.mode == "fresh":
            fn, capture_safe = ReverseChain._resolve_noise(owner, denoise_fn)
            if isinstance(fn, SimplexNoiseFn):
                raise ValueError("KnownRegion(noise='fresh'): the step noise is a simplex field; a second simplex field per step "
                                 "for the known region is not provided -- use 'fixed' or a tensor")
            if not ReverseChain._seeded_gauss(owner, fn, capture_safe):
                raise ValueError("KnownRegion(noise='fresh'): the per-step draw is made inside the update kernel from the seeded "
                                 "gaussian stream; this owner is not seeded (seed_gauss) or the noise request is not the gaussian one")
        return known.mode

    @staticmethod
    def _check_resample_request(owner, denoise_fn, sampler, known, resampling):
        """`resampling` as a chain may run it: with a KnownRegion, the ancestral sampler and gaussian step noise only."""
        if _check_resampling(resampling) is None:
            return None
        if known is None:
            raise ValueError("resampling: the jumps harmonise a generated region with a kept one; without `known` (a KnownRegion) "
                             "there is nothing to harmonise")
        if sampler is not None:
            raise ValueError("resampling: a strided sampler is refused -- the jump schedule is stated in single ancestral steps "
                             "(a level lands on level - 1); resampling under a stride is not provided")
        fn, _ = ReverseChain._resolve_noise(owner, denoise_fn)
        if isinstance(fn, SimplexNoiseFn):
            raise ValueError("resampling: the step noise is a simplex field; the re-noise of a jump takes the chain's step-noise "
                             "kind and a simplex re-noise is not provided -- use the gaussian step noise")
        return resampling

    @staticmethod
    def _reuse_key_of(owner, denoise_fn, sampler=None, known=None, resampling=None, shared_planes=False):
        """Key under which a graph-replaying chain for this noise request may be restarted with reset() (None: never).  A graph
        captured with torch.randn_like is never replayed for a seeded run, nor the reverse: the keys differ.  Likewise an
        ancestral graph and a strided one (tag "strided"); stride and eta are NOT in the key -- the strided launches read them
        from device words, so one strided graph serves every stride.  A conditioned graph carries ("known", mode): it is never
        replayed for an unconditioned request, nor the reverse, and "fixed" and "fresh" are different launches.  A resampled
        graph carries ("resample",) -- other launches -- but not (jump, reps): they are device words.  ("shared",): the image and
        keep planes of a slot chain have a sample stride of 0, which a capture bakes in."""
        fn, capture_safe = ReverseChain._resolve_noise(owner, denoise_fn)
        if isinstance(fn, SimplexNoiseFn):
            key = ("simplex", id(fn.simplex), fn.octave, fn.persistence, fn.frequency, fn.in_channels)
        elif ReverseChain._seeded_gauss(owner, fn, capture_safe):
            key = ("gauss", "seeded")
        else:
            key = ("gauss",) if capture_safe else None
        if key is not None and sampler is not None:
            key += ("strided",)
        if key is not None and known is not None:
            key += (("known", ReverseChain._known_mode_of(owner, denoise_fn, known)),)
        if key is not None and resampling is not None:
            key += ("resample",)
        if key is not None and known is not None and shared_planes:
            key += ("shared",)
        return key

    def _set_streams(self, stream_base):
        """Sample b of a seeded chain draws from stream `stream_base + b`; None: B fresh ids from the owner's allocator."""
        if stream_base is None:
            stream_base = self.owner._take_streams(self.B)
        self.streams.copy_(philox.stream_ids(stream_base, self.B))

    def _draw_tables(self, nsteps):
        """Every seed of the chain, drawn now in the order the per-step newSeed() calls would (numpy global stream), and the
        permutation tables uploaded in one copy."""
        import time
        t0 = time.perf_counter()
        fn = self.simplex_fn
        n = nsteps * fn.in_channels
        tabs = np.empty((n, 512), dtype=np.int16)
        self._last_seed = None
        for i in range(n):
            seed = np.random.randint(-10000000000, 10000000000)
            tabs[i] = perm_tables(seed)
            self._last_seed = seed
        if n:
            self.tables[:n].copy_(torch.from_numpy(tabs))
        # host time of the whole chain's newSeed() work, paid before the first step (upstream pays one newSeed() per step):
        # bench.py reports it beside the per-step time
        self.table_setup_ms = 1000.0 * (time.perf_counter() - t0)
        self.table_setup_steps = nsteps

    def reset(self, x, t_distance, stream_base=None, sampler=None, known=None, resampling=None):
        """Start another chain of the same batch shape on this chain's device buffers: the captured HIP graph (and the plan behind
        it) is reused instead of being built again -- the detection loops run hundreds of chains of one shape.  A strided chain
        may be handed another `sampler` (None: keep its own): the kept graph follows the re-written stride / eta words.  A
        conditioned chain may be handed another `known` of its own mode (None: the planes stay as they are), a resampled one
        another `resampling` (None: keep its own): the kept graph reads (jump, reps) from the re-written device words."""
        if resampling is not None:
            if self.resampling is None:
                raise ValueError("ReverseChain.reset: a chain without resampling cannot be restarted as a resampled one")
            self.resampling = _check_resampling(resampling)
        if known is not None:
            if self.known_mode is None:
                raise ValueError("ReverseChain.reset: an unconditioned chain cannot be restarted as a conditioned one")
            if self._known_mode_of(self.owner, self.denoise_fn, known) != self.known_mode:
                raise ValueError(f"ReverseChain.reset: this chain's known-region noise is {self.known_mode!r}, not {known.mode!r}")
        if sampler is not None:
            if self.sampler is None:
                raise ValueError("ReverseChain.reset: an ancestral chain cannot be restarted as a strided one")
            self.sampler = _check_sampler(sampler)
        if tuple(x.shape) != tuple(self.x.shape) or x.device != self.x.device:
            raise ValueError("ReverseChain.reset: shape / device differ from the chain's buffers")
        self._start(x, t_distance, stream_base, known)
        if self.hip_model and self._graph_state == 2:
            # the replayed graph reads the packed weights of the plan it was captured with (NOT whatever _plan_for would pick
            # now -- ANODDPM_ARITH may have changed since): let THAT plan re-pack them if the parameters moved since
            self._plan.refresh_weights()
        return self

    def _start(self, x, t_distance, stream_base, known=None):
        """Begin a chain of `t_distance` timesteps from `x` on this chain's buffers.  The order is fixed: `_draw_tables` consumes
        the global numpy stream and `_set_streams` the owner's stream allocator; a "fixed" known-region noise that the chain
        draws itself comes after both.  Never runs inside a capture: the sampler words are allocated and written here, and the
        known-region planes are copied here."""
        if known is not None:
            known.check_batch(self.x.shape)
        if not 0 <= int(t_distance) <= self.owner.num_timesteps:
            # extract() of the reference indexes the T-entry tables with t_distance - 1 and raises for anything else
            raise IndexError(f"t_distance {t_distance} is out of range for a {self.owner.num_timesteps}-step schedule")
        self.x.copy_(self.owner._f32(x.detach()))
        self.t.fill_(int(t_distance) - 1)
        self.step_idx.zero_()
        self.remaining = int(t_distance) if self.sampler is None else self.sampler.steps(t_distance)
        if self.resampling is not None:
            self.remaining = self.resampling.steps(t_distance)
            self.rs_top.fill_(int(t_distance) - 1)
            self.rs_rep.fill_(self.resampling.reps - 1)
            self.rs_visit.zero_()
            self.rs_jump.fill_(self.resampling.jump)
            self.rs_reps.fill_(self.resampling.reps)
        if self.sampler is not None:
            self.owner._sampler_words(self.x.device, self.sampler)
        if self.tables is not None:
            self._draw_tables(self.remaining)
        if self.streams is not None:
            self._set_streams(stream_base)
        if known is not None:
            self.k_x0.copy_(known.x_0)                              # a batch of 1 is broadcast over the chain's
            self.k_keep.copy_(known.keep)
            if self.k_noise is not None:
                if torch.is_tensor(known.noise):
                    self.k_noise.copy_(known.noise)
                elif int(t_distance) > 0 and not self.shared_planes:      # a slot chain's planes are filled per refill
                    t_top = torch.full((self.B,), int(t_distance) - 1, device=self.x.device, dtype=torch.int64)
                    self.k_noise.copy_(self.owner.noise_fn(self.k_x0, t_top).float())

    def step(self):
        if self.sampler is not None:
            # host-side comparison; a copy only when another strided call on this owner re-wrote the words since (never in a capture)
            self.owner._sampler_words(self.x.device, self.sampler)
        if self.use_graph and lib().anoddpm_prof_active() == 0:
            if self._graph_state == 2:
                self.graph.replay()
                self.remaining -= 1
                return self.x
            if self._graph_state == 1:
                # everything a step touches is static (x, t, step counter, noise, tables, plan buffers)
                torch.cuda.synchronize()
                if self.hip_model:
                    self._plan = self.model._plan_for(self.B, self.x.shape[2], self.x.device)
                g = torch.cuda.CUDAGraph()
                # No cyclic garbage collection INSIDE the capture (round 6: a sporadic `Fatal Python error: Aborted` with the
                # interpreter "Garbage-collecting" under _step_body, about one GPU test run in five): the collector may pick that
                # moment to destroy an older chain's captured graph / plan buffers left unreachable by an earlier caller, and HIP
                # API calls made by those destructors are illegal while a stream capture is open in global mode.  Collect first
                # (twice: C++ owners release further Python cycles), then keep the collector off until the capture has ended.
                import gc
                gc.collect()
                gc.collect()
                gc_was_enabled = gc.isenabled()
                gc.disable()
                try:
                    with torch.cuda.graph(g):
                        self._step_body()
                finally:
                    if gc_was_enabled:
                        gc.enable()
                self.graph = g
                self._graph_state = 2
                g.replay()                      # capture does not execute: run the captured step once
                self.remaining -= 1
                return self.x
            self._graph_state = 1               # first step runs eagerly (builds the plan, packs weights)
        self._step_body()
        self.remaining -= 1
        return self.x

    def _step_body(self):
        o = self.owner

        with torch.no_grad():
            # (forking the step's simplex field -- it depends on t and the step counter only -- onto a second stream beside the
            # denoiser's latency-bound timestep MLP was measured: the captured graph gains a second branch and replays 0.14 ms
            # SLOWER, 9.52 vs 9.38 ms per step)
            eps = self.model.forward_hip(self.x, self.t, borrow=True) if self.hip_model else self.model(self.x, self.t)
            if self.tables is not None:
                fn = self.simplex_fn
                for c in range(fn.in_channels):
                    fn.simplex.fill_fixed_T_octaves_(self.noise, self.t, fn.octave, fn.persistence, fn.frequency,
                                                     channel=c, tables=self.tables[c:], table_sel=self.step_idx,
                                                     table_sel_scale=fn.in_channels)
                noise = self.noise
            elif self.streams is not None:
                noise = None                                        # generated inside the update kernel
            else:
                noise = o._denoise_noise(self.x, self.t, self.denoise_fn)
            words = o._sampler_words(self.x.device, None) if self.sampler is not None else None
            if self.resampling is not None:
                # an unseeded chain draws the re-noise plane next to its step-noise plane; a seeded one generates both in the launch
                renoise = torch.randn_like(self.x) if self.streams is None else None
                state = (self.rs_jump, self.rs_reps, self.rs_top, self.rs_rep, self.rs_visit)
                o._known_update(self.x, self.t, eps, noise, (self.k_x0, self.k_keep, self.k_noise), None, want_pred=False,
                                out=self.x, gauss_streams=self.streams, resample=state + (renoise,))
                check(lib().anoddpm_chain_advance_resample(ptr(self.t), self.B, ptr(self.step_idx), *(ptr(w) for w in state),
                                                           current_stream()), "chain_advance_resample")
                return
            if self.known_mode is not None:
                o._known_update(self.x, self.t, eps, noise, (self.k_x0, self.k_keep, self.k_noise), words, want_pred=False,
                                out=self.x, gauss_streams=self.streams)
            elif self.sampler is not None:
                o._strided_update(self.x, self.t, eps, noise, None, want_pred=False, out=self.x, gauss_streams=self.streams)
            else:
                o._reverse_update(self.x, self.t, eps, noise, want_pred=False, out=self.x, gauss_streams=self.streams)     # in place
            if self.sampler is not None:
                check(lib().anoddpm_chain_advance_strided(ptr(self.t), self.B, ptr(self.step_idx), ptr(words.stride),
                                                          current_stream()), "chain_advance_strided")
            else:
                check(lib().anoddpm_chain_advance(ptr(self.t), self.B, ptr(self.step_idx), current_stream()), "chain_advance")

    def finish(self):
        if self.tables is not None and self._last_seed is not None:
            self.simplex_fn.simplex.newSeed(self._last_seed)       # leave the generator where upstream would


class _DeviceTables:
    """fp32 device copies of the schedule tables (one upload per device, not eight per step)."""

    NAMES = ("sqrt_alphas", "sqrt_betas", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
             "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
             "posterior_mean_coef2", "model_variance", "model_log_variance", "sigma")

    def __init__(self, owner, device):
        def up(a):
            # extract() gathers in fp64 and casts the gathered value: casting the table is the same thing
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float().to(device)
        for n in self.NAMES[:8]:
            setattr(self, n, up(getattr(owner, n)))
        model_var = np.append(owner.posterior_variance[1], owner.betas[1:])       # :282-283
        model_logvar = np.log(model_var)
        self.model_variance = up(model_var)
        self.model_log_variance = up(model_logvar)
        self.posterior_log_variance_clipped = up(owner.posterior_log_variance_clipped)
        # exp(0.5*log_variance) evaluated by the same fp32 torch expression the reference uses (:317)
        self.sigma = torch.exp(0.5 * torch.from_numpy(model_logvar).float()).to(device)


class _SamplerWords:
    """What the strided launches read on one device: the fp64 alphas_cumprod table and the stride / eta words (kept for the life
    of the instance: captured graphs point at them), with a host copy of what the words hold."""

    def __init__(self, owner, device):
        self.acp = torch.from_numpy(np.ascontiguousarray(owner.alphas_cumprod, dtype=np.float64)).to(device)
        self.stride = torch.zeros(1, dtype=torch.int32, device=device)      # 0 until written: a launch before that gives NaN
        self.eta = torch.zeros(1, dtype=torch.float32, device=device)
        self.held = None

    def write(self, sampler):
        if sampler != self.held:
            self.stride.copy_(torch.tensor([sampler.stride], dtype=torch.int32))
            self.eta.copy_(torch.tensor([sampler.eta], dtype=torch.float32))
            self.held = sampler


class _FusedLoss(torch.autograd.Function):
    """(per-sample loss [B], vlb [B], weighted batch mean []) of calc_loss / p_loss from the model output, and in backward the
    gradient with respect to the model output -- anoddpm_loss_forward / anoddpm_loss_backward.  kind: 0 l1, 1 l2, 2 hybrid,
    3 = the VLB term alone (calc_vlb_xt).  Only `eps` is differentiable."""

    @staticmethod
    def _args(owner, eps, noise, x0, xt, t, weights, kind):
        tb = owner._tables(eps.device)
        a = LossArgs()
        a.eps, a.noise = ptr(eps), ptr(noise if noise is not None else eps)
        a.weights = ptr(weights) if weights is not None else None
        if kind >= 2:
            a.x0, a.xt, a.t = ptr(x0), ptr(xt), ptr(t)
            a.c_recip, a.c_recipm1 = ptr(tb.sqrt_recip_alphas_cumprod), ptr(tb.sqrt_recipm1_alphas_cumprod)
            a.c_coef1, a.c_coef2 = ptr(tb.posterior_mean_coef1), ptr(tb.posterior_mean_coef2)
            a.c_post_logvar, a.c_model_logvar = ptr(tb.posterior_log_variance_clipped), ptr(tb.model_log_variance)
        B = eps.shape[0]
        a.n, a.B, a.T, a.kind = (eps[0].numel() if B else 0), B, owner.num_timesteps, min(kind, 2)
        return a

    @staticmethod
    def forward(ctx, eps, noise, x0, xt, t, weights, owner, kind):
        _lib.require_cuda(eps, "GaussianDiffusionModel loss")
        f32 = owner._f32
        e = f32(eps.detach())
        nz = f32(noise.detach()) if noise is not None else None
        x0c, xtc, tt = (f32(x0.detach()), f32(xt.detach()), owner._t64(t, e.device)) if kind >= 2 else (None, None, None)
        w = f32(weights.detach().to(e.device)) if weights is not None else None
        B = e.shape[0]
        out = torch.empty((2 * B + 1,), dtype=torch.float32, device=e.device)
        ws = torch.empty((max(B, 1) * 64 * 2,), dtype=torch.float64, device=e.device)
        a = _FusedLoss._args(owner, e, nz, x0c, xtc, tt, w, kind)
        a.per_sample, a.vlb, a.total = ptr(out[:B]), ptr(out[B:2 * B]), ptr(out[2 * B:])
        a.workspace, a.workspace_doubles = ptr(ws), ws.numel()
        if B:
            check(lib().anoddpm_loss_forward(ctypes.byref(a), current_stream()), "loss_forward")
        ctx.owner, ctx.kind, ctx.saved = owner, kind, (e, nz, x0c, xtc, tt, w)
        ctx.set_materialize_grads(False)
        per, vlb, total = out[:B], out[B:2 * B], out[2 * B]
        if kind == 3:
            # the VLB term alone: the fused kernel's per-sample value is vlb + mse(eps, eps) = vlb
            return per, vlb, total
        return per, vlb, total

    @staticmethod
    def backward(ctx, g_per, g_vlb, g_total):
        e, nz, x0c, xtc, tt, w = ctx.saved
        kind = ctx.kind
        a = _FusedLoss._args(ctx.owner, e, nz, x0c, xtc, tt, w, kind)
        keep = []

        def dev(g):
            if g is None:
                return None
            g = g.detach().float().contiguous()
            keep.append(g)
            return ptr(g)
        if kind == 3:
            # per == vlb here (no main term): fold both upstream gradients into g_vlb, and leave the main-term coefficient at zero
            gv = g_vlb if g_per is None else (g_per if g_vlb is None else g_per + g_vlb)
            a.g_per, a.g_vlb, a.g_total = None, dev(gv), None
            if g_total is not None:
                raise _lib.AnoddpmError("calc_vlb_xt: only the per-sample output is differentiable")
        else:
            a.g_per, a.g_vlb, a.g_total = dev(g_per), dev(g_vlb), dev(g_total)
        d = torch.empty_like(e)
        a.d_eps = ptr(d)
        if e.shape[0]:
            check(lib().anoddpm_loss_backward(ctypes.byref(a), current_stream()), "loss_backward")
        return d, None, None, None, None, None, None, None


class GaussianDiffusionModel:
    # opt-in post-processing of the detection records (metrics.PostProcess, and an optional 0 / 1 region-of-interest tensor shaped
    # like one image or like x_0): see _score_settings.  Plain attributes: pickled and deep-copied with the instance.
    postprocess = None
    postprocess_roi = None
    # opt-in per-region overlap score of the detection records: a false-positive-rate limit in (0, 1] (0.3 in the literature); see
    # _score_settings.  A plain attribute like `postprocess`.
    pro_limit = None
    # opt-in boundary distances of the detection records (Hausdorff, HD95, average symmetric surface distance of the thresholded
    # map against the mask); see _score_settings.  A plain attribute like `postprocess`.
    surface_metrics = False
    # opt-in image-level scores of the detection records (metrics.image_scores' `top`: an int k or a fraction in (0, 1]): the maximum
    # and the top-k mean of every image's squared-error map; see _score_settings.  A plain attribute like `pro_limit`.
    image_top = None
    # opt-in scores at calibrated operating thresholds (an fp32 device tensor [T], e.g. metrics.HealthyPool.thresholds; never read on
    # the host): `dice_at`, `precision_at`, `recall_at`, `fpr_at` in every detection record; see _score_settings.
    operating_thresholds = None
    # opt-in strided reverse sampler (StridedSampler; None: the reference's ancestral sampler, and none of the strided code runs).
    # Read by ReverseChain / reverse_chain / forward_backward and the detection loops unless they are handed `sampler=`; also set at
    # construction from ANODDPM_SAMPLER="<stride>[,<eta>]".  A plain attribute like `postprocess`.
    sampler = None
    # opt-in known-region conditioning of the detection sweeps: `detection_keep`, a mask tensor [1 or C, H, W] or
    # [1, 1 or C, H, W] (nonzero = keep), ties those pixels of every chain of detection_A / detection_B to the input image
    # (KnownRegion(x_0, keep, "fixed")); `resampling` (Resampling; also ANODDPM_RESAMPLE="<jump>,<reps>") adds the jumps.  Both
    # None: the sweeps issue exactly the unconditioned launches.  `resampling` without `detection_keep` is refused by the sweep.
    detection_keep = None
    resampling = None

    def __init__(self, img_size, betas, img_channels=1, loss_type="l2", loss_weight='none', noise="gauss"):
        super().__init__()
        if noise == "gauss":
            self.noise_fn = GaussNoiseFn(self)
        else:
            self.simplex = Simplex_CLASS()
            if noise == "simplex_randParam":
                self.noise_fn = lambda x, t: generate_simplex_noise(self.simplex, x, t, True, in_channels=img_channels)
            elif noise == "random":
                self.noise_fn = lambda x, t: random_noise(self.simplex, x, t)
            else:
                self.noise_fn = lambda x, t: generate_simplex_noise(self.simplex, x, t, False, in_channels=img_channels)
        self.noise_kind = noise
        self._default_noise_fn = self.noise_fn      # lets the reverse chain tell a user-replaced noise_fn from this one

        self.img_size = img_size
        self.img_channels = img_channels
        self.loss_type = loss_type
        self.num_timesteps = len(betas)

        if loss_weight == 'prop-t':
            self.weights = np.arange(self.num_timesteps, 0, -1)
        elif loss_weight == "uniform":
            self.weights = np.ones(self.num_timesteps)
        self.loss_weight = loss_weight

        # fp64 host tables, GaussianDiffusion.py:184-217
        betas = np.asarray(betas, dtype=np.float64)
        alphas = 1 - betas
        self.betas = betas
        self.sqrt_alphas = np.sqrt(alphas)
        self.sqrt_betas = np.sqrt(betas)
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
        self._dev = {}
        import os
        env = os.environ.get("ANODDPM_GAUSS_SEED")
        self.seed_gauss(int(env, 0) if env else None)
        env = os.environ.get("ANODDPM_SAMPLER")
        if env:
            self.sampler = StridedSampler.parse(env)
        env = os.environ.get("ANODDPM_RESAMPLE")
        if env:
            self.resampling = Resampling.parse(env)

    # ------------------------------------------------------------------ seeded gaussian noise
    def seed_gauss(self, seed):
        """Opt in to reproducible gaussian noise: with a 64-bit `seed` every gaussian draw of this instance -- the "gauss" /
        "random" step noise, the gauss `noise_fn` -- comes from the counter-based stream of DESIGN 9g instead of torch's generator,
        the reverse-step noise generated inside the update kernel.  Chain / sample c since this call draws from stream c, whatever
        slot or batch it runs in.  `None` returns to torch.randn_like.  Both attributes are plain: they pickle and deep-copy."""
        self.gauss_seed = None if seed is None else int(seed) & ((1 << 64) - 1)
        self.gauss_next_stream = 0
        if self.gauss_seed is not None:
            # kept graphs read the seed through these device words: rewrite them in place
            for dev, word in self.__dict__.get("_gauss_dev", {}).items():
                word.copy_(philox.seed_tensor(self.gauss_seed, "cpu"))

    def _take_streams(self, count):
        """`count` consecutive stream ids from the allocator -> the first."""
        base = self.gauss_next_stream
        self.gauss_next_stream = (base + int(count)) & 0xFFFFFFFF
        return base

    def _gauss_seed_dev(self, device):
        """The device word that holds the seed (one per device for the life of the instance: captured graphs point at it)."""
        words = self.__dict__.setdefault("_gauss_dev", {})
        if device not in words:
            words[device] = philox.seed_tensor(self.gauss_seed, device)
        return words[device]

    def _seeded_normal(self, x, t, domain):
        """Seeded stand-in for torch.randn_like(x) outside a chain: sample b from a fresh stream id, at step t[b]."""
        _lib.require_cuda(x, "GaussianDiffusionModel seeded noise")
        B = x.shape[0]
        return philox.normal(self._gauss_seed_dev(x.device), x.shape, stream=self._take_streams(B), step=self._t64(t, x.device),
                             domain=domain, T=self.num_timesteps)

    # ------------------------------------------------------------------ strided sampler
    def _sampler_words(self, device, sampler):
        """The device's _SamplerWords, holding `sampler`'s stride and eta (None: as they are).  Never called inside a capture with
        a sampler that differs from what the words hold."""
        words = self.__dict__.setdefault("_sampler_dev", {})
        device = torch.device(device)
        w = words.get(device)
        if w is None:
            w = words[device] = _SamplerWords(self, device)
        if sampler is not None:
            w.write(_check_sampler(sampler))
        return w

    def _strided_update(self, x_t, t, eps, noise, sampler, want_pred=True, want_mean=False, out=None, gauss_streams=None):
        """One fused launch of the strided step (anoddpm_strided_update), the counterpart of `_reverse_update`.  `sampler` None:
        the stride / eta words are used as they are (a chain wrote them before its step).  -> (x_prev, pred_x_0, mean)."""
        _lib.require_cuda(x_t, "GaussianDiffusionModel.sample_p_strided")
        tb = self._tables(x_t.device)
        words = self._sampler_words(x_t.device, sampler)
        x_t, eps = self._f32(x_t.detach()), self._f32(eps.detach())
        if noise is not None:
            noise = self._f32(noise.detach())
        t = self._t64(t, x_t.device)
        a = PUpdateArgs()
        x_prev = out if out is not None else torch.empty_like(x_t)
        pred = torch.empty_like(x_t) if want_pred else None
        mean = torch.empty_like(x_t) if want_mean else None
        a.x_prev, a.pred_x0, a.mean_out = x_prev.data_ptr(), pred.data_ptr() if want_pred else None, mean.data_ptr() if want_mean else None
        a.x_t, a.eps, a.noise, a.t = x_t.data_ptr(), eps.data_ptr(), noise.data_ptr() if noise is not None else None, t.data_ptr()
        a.c_recip, a.c_recipm1 = tb.sqrt_recip_alphas_cumprod.data_ptr(), tb.sqrt_recipm1_alphas_cumprod.data_ptr()
        a.B, a.T = x_t.shape[0], self.num_timesteps
        a.n = x_t.numel() // max(x_t.shape[0], 1)
        seed = ptr(self._gauss_seed_dev(x_t.device)) if gauss_streams is not None else None
        check(lib().anoddpm_strided_update(ctypes.byref(a), ptr(words.acp), ptr(words.stride), ptr(words.eta), seed,
                                           ptr(gauss_streams), 0, current_stream()), "strided_update")
        return x_prev, pred, mean

    def sample_p_strided(self, model, x_t, t, sampler, denoise_fn="gauss"):
        """One step of the strided sampler from t to t - sampler.stride: model -> noise -> ONE fused launch.  The counterpart of
        `sample_p`; see StridedSampler for what this sampler is and is not.  With eta == 0 no noise is drawn."""
        if _check_sampler(sampler) is None:
            raise TypeError("sample_p_strided: a StridedSampler is required")
        eps = model(x_t, t)
        noise = self._denoise_noise(x_t, t, denoise_fn) if sampler.eta != 0.0 else None
        sample, pred, _ = self._strided_update(x_t, t, eps, noise, sampler)
        return {"sample": sample, "pred_x_0": pred}

    # ------------------------------------------------------------------ known-region conditioning
    def _known_update(self, x_t, t, eps, noise, planes, words, want_pred=True, want_mean=False, out=None, gauss_streams=None,
                      stream0=None, resample=None):
        """One fused launch of the conditioned step (anoddpm_p_sample_update_known), the counterpart of `_reverse_update`
        (`words` None) and `_strided_update` (`words`: the device's sampler words, used as they are).  planes = (x_0, keep bytes,
        known-region noise or None: generated in the launch), each fp32 / uint8, contiguous, batch 1 or B.  The seeded key block is
        handed over with `gauss_streams` (device int32[B]) or `stream0` (sample b draws from stream0 + b).
        resample = (jump word, reps word, top, rep, visit, re-noise or None: generated), device tensors: the launch is
        anoddpm_p_sample_update_resample (ancestral only, `words` None), which also carries out the samples' jumps.
        -> (x_prev, pred_x_0, mean)."""
        _lib.require_cuda(x_t, "GaussianDiffusionModel.sample_p_known")
        tb = self._tables(x_t.device)
        x_t, eps = self._f32(x_t.detach()), self._f32(eps.detach())
        if noise is not None:
            noise = self._f32(noise.detach())
        t = self._t64(t, x_t.device)
        a = PUpdateArgs()
        x_prev = out if out is not None else torch.empty_like(x_t)
        pred = torch.empty_like(x_t) if want_pred else None
        mean = torch.empty_like(x_t) if want_mean else None
        a.x_prev, a.pred_x0, a.mean_out = x_prev.data_ptr(), pred.data_ptr() if want_pred else None, mean.data_ptr() if want_mean else None
        a.x_t, a.eps, a.noise, a.t = x_t.data_ptr(), eps.data_ptr(), noise.data_ptr() if noise is not None else None, t.data_ptr()
        a.c_recip, a.c_recipm1 = tb.sqrt_recip_alphas_cumprod.data_ptr(), tb.sqrt_recipm1_alphas_cumprod.data_ptr()
        if words is None:
            a.c_coef1, a.c_coef2, a.c_sigma = tb.posterior_mean_coef1.data_ptr(), tb.posterior_mean_coef2.data_ptr(), tb.sigma.data_ptr()
        a.B, a.T = x_t.shape[0], self.num_timesteps
        a.n = x_t.numel() // max(x_t.shape[0], 1)
        x_0, keep, kz = planes
        for p in planes:
            if p is not None and (p.device != x_t.device or not p.is_contiguous()):
                raise _lib.AnoddpmError("sample_p_known: the known-region planes must be contiguous tensors on the device of x_t")
        k = KnownArgs()
        k.x0, k.keep, k.noise = x_0.data_ptr(), keep.data_ptr(), kz.data_ptr() if kz is not None else None
        k.ca, k.cb = tb.sqrt_alphas_cumprod.data_ptr(), tb.sqrt_one_minus_alphas_cumprod.data_ptr()
        k.x0_stride, k.keep_stride = (a.n if x_0.shape[0] == a.B else 0), (a.n if keep.shape[0] == a.B else 0)
        k.noise_stride = a.n if kz is not None and kz.shape[0] == a.B else 0
        seeded = gauss_streams is not None or stream0 is not None
        if resample is not None:
            if words is not None:
                raise ValueError("sample_p_known: resampling is refused under a strided sampler")
            r = ResamplingArgs()
            rz = resample[5]
            if rz is not None:
                rz = self._f32(rz.detach())
            r.jump, r.reps, r.top, r.rep, r.visit = (w.data_ptr() for w in resample[:5])
            r.noise, r.noise_stride = (rz.data_ptr() if rz is not None else None), (a.n if rz is not None and rz.shape[0] == a.B else 0)
            r.alphas_cumprod = self._sampler_words(x_t.device, None).acp.data_ptr()
            check(lib().anoddpm_p_sample_update_resample(
                ctypes.byref(a), ctypes.byref(k), ctypes.byref(r), ptr(self._gauss_seed_dev(x_t.device)) if seeded else None,
                ptr(gauss_streams), int(stream0 or 0) & 0xFFFFFFFF, current_stream()), "p_sample_update_resample")
            return x_prev, pred, mean
        check(lib().anoddpm_p_sample_update_known(
            ctypes.byref(a), ctypes.byref(k), ptr(words.acp) if words else None, ptr(words.stride) if words else None,
            ptr(words.eta) if words else None, ptr(self._gauss_seed_dev(x_t.device)) if seeded else None, ptr(gauss_streams),
            int(stream0 or 0) & 0xFFFFFFFF, current_stream()), "p_sample_update_known")
        return x_prev, pred, mean

    def sample_p_known(self, model, x_t, t, known, denoise_fn="gauss", sampler=None):
        """One conditioned reverse step from t to s = t - 1, or t - sampler.stride: model -> noise -> ONE fused launch.  The pixels
        `known.keep` marks leave it as `known.x_0` noised to s with `known.noise` (a tensor, or "fresh" on a seeded instance), the
        rest as `sample_p` / `sample_p_strided` would leave them; "pred_x_0" is the unconditioned one at every pixel.  On a seeded
        instance the gaussian step noise is drawn as `sample_p` draws it -- B fresh stream ids -- inside the launch."""
        if _check_known(known) is None:
            raise TypeError("sample_p_known: a KnownRegion is required")
        sampler = _check_sampler(sampler)
        known.check_batch(x_t.shape)
        mode = ReverseChain._known_mode_of(self, denoise_fn, known)
        if mode == "fixed" and not torch.is_tensor(known.noise):
            raise ValueError("sample_p_known: noise='fixed' is a chain's forward noise; a single step needs the tensor itself "
                             "(or 'fresh' on a seeded instance)")
        eps = model(x_t, t)
        drawn = sampler is None or sampler.eta != 0.0             # sample_p_strided draws nothing at eta == 0
        fn, capture_safe = ReverseChain._resolve_noise(self, denoise_fn)
        stream0 = noise = None
        if ReverseChain._seeded_gauss(self, fn, capture_safe) and (drawn or mode == "fresh"):
            stream0 = self._take_streams(x_t.shape[0])
        elif drawn:
            noise = self._denoise_noise(x_t, t, denoise_fn)
        words = self._sampler_words(x_t.device, sampler) if sampler is not None else None
        planes = (known.x_0, known.keep, known.noise if mode == "fixed" else None)
        sample, pred, _ = self._known_update(x_t, t, eps, noise, planes, words, stream0=stream0)
        return {"sample": sample, "pred_x_0": pred}

    # ------------------------------------------------------------------ device plumbing
    def _tables(self, device):
        tb = self._dev.get(device)
        if tb is None:
            tb = self._dev[device] = _DeviceTables(self, device)
        return tb

    @staticmethod
    def _t64(t, device):
        if t.dtype != torch.int64 or t.device != device or not t.is_contiguous():
            t = t.to(device=device, dtype=torch.int64).contiguous()
        return t

    @staticmethod
    def _f32(x):
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        return x

    def _axpby(self, ca, cb, x, t, noise):
        _lib.require_cuda(x, "GaussianDiffusionModel.sample_q")
        x = self._f32(x.detach() if not x.requires_grad else x)
        noise = self._f32(noise).to(x.device)
        t = self._t64(t, x.device)
        out = torch.empty_like(x)
        B = x.shape[0]
        check(lib().anoddpm_q_sample(ptr(out), ptr(x), ptr(noise), ptr(t), ptr(ca), ptr(cb), B,
                                     x.numel() // max(B, 1), self.num_timesteps, current_stream()), "q_sample")
        return out

    def _q_sample_gauss(self, x, t, stream_base, want_noise=False):
        """sample_q with the forward noise of streams `stream_base + b` generated inside the kernel -> (x_t, noise or None)."""
        _lib.require_cuda(x, "GaussianDiffusionModel.sample_q")
        tb = self._tables(x.device)
        x, t = self._f32(x.detach()), self._t64(t, x.device)
        out = torch.empty_like(x)
        noise = torch.empty_like(x) if want_noise else None
        B = x.shape[0]
        check(lib().anoddpm_q_sample_gauss(ptr(out), ptr(noise), ptr(x), ptr(t), ptr(tb.sqrt_alphas_cumprod),
                                           ptr(tb.sqrt_one_minus_alphas_cumprod), B, x.numel() // max(B, 1), self.num_timesteps,
                                           ptr(self._gauss_seed_dev(x.device)), None, int(stream_base) & 0xFFFFFFFF,
                                           current_stream()), "q_sample_gauss")
        return out, noise

    def _reverse_update(self, x_t, t, eps, noise, want_pred=True, want_mean=False, out=None, gauss_streams=None):
        """One fused launch for GaussianDiffusion.py:287-288 + :314-317.  gauss_streams (device int32[B], with noise None): the
        step noise is generated inside the launch from the seeded stream of those ids."""
        _lib.require_cuda(x_t, "GaussianDiffusionModel.sample_p")
        tb = self._tables(x_t.device)
        x_t, eps = self._f32(x_t.detach()), self._f32(eps.detach())
        if noise is not None:
            noise = self._f32(noise.detach())
        t = self._t64(t, x_t.device)
        a = PUpdateArgs()
        x_prev = out if out is not None else torch.empty_like(x_t)
        pred = torch.empty_like(x_t) if want_pred else None
        mean = torch.empty_like(x_t) if want_mean else None
        a.x_prev, a.pred_x0, a.mean_out = x_prev.data_ptr(), pred.data_ptr() if want_pred else None, mean.data_ptr() if want_mean else None
        a.x_t, a.eps, a.noise, a.t = x_t.data_ptr(), eps.data_ptr(), noise.data_ptr() if noise is not None else None, t.data_ptr()
        a.c_recip, a.c_recipm1 = tb.sqrt_recip_alphas_cumprod.data_ptr(), tb.sqrt_recipm1_alphas_cumprod.data_ptr()
        a.c_coef1, a.c_coef2, a.c_sigma = tb.posterior_mean_coef1.data_ptr(), tb.posterior_mean_coef2.data_ptr(), tb.sigma.data_ptr()
        a.B, a.T = x_t.shape[0], self.num_timesteps
        a.n = x_t.numel() // max(x_t.shape[0], 1)
        if gauss_streams is not None:
            check(lib().anoddpm_p_sample_update_gauss(ctypes.byref(a), ptr(self._gauss_seed_dev(x_t.device)), ptr(gauss_streams), 0,
                                                      current_stream()), "p_sample_update_gauss")
        else:
            check(lib().anoddpm_p_sample_update(ctypes.byref(a), current_stream()), "p_sample_update")
        return x_prev, pred, mean

    # ------------------------------------------------------------------ reference API
    def sample_t_with_weights(self, b_size, device):
        """GaussianDiffusion.py:220-226: timesteps drawn with probability proportional to `self.weights` from the global numpy
        stream, plus the importance weights p[t] / T (fp64 product, then fp32)."""
        prob = self.weights / np.sum(self.weights)
        drawn = np.random.choice(prob.size, size=b_size, p=prob)
        return (torch.from_numpy(drawn).long().to(device),
                torch.from_numpy(1 / prob.size * prob[drawn]).float().to(device))

    def _at(self, table, t, like):
        """extract() on a host table: gather in fp64, cast, shape [B,1,...] broadcastable against `like`."""
        return extract(table, t, like.shape, like.device)

    def predict_x_0_from_eps(self, x_t, t, eps):
        """GaussianDiffusion.py:228-230 (differentiable API form; the sampling path fuses it into anoddpm_p_sample_update)."""
        a, b = self._at(self.sqrt_recip_alphas_cumprod, t, x_t), self._at(self.sqrt_recipm1_alphas_cumprod, t, x_t)
        return a * x_t - b * eps

    def predict_eps_from_x_0(self, x_t, t, pred_x_0):
        """GaussianDiffusion.py:232-235."""
        a, b = self._at(self.sqrt_recip_alphas_cumprod, t, x_t), self._at(self.sqrt_recipm1_alphas_cumprod, t, x_t)
        return (a * x_t - pred_x_0) / b

    def q_mean_variance(self, x_0, t):
        """q(x_t | x_0): mean, variance, log-variance (GaussianDiffusion.py:237-251)."""
        return (self._at(self.sqrt_alphas_cumprod, t, x_0) * x_0, self._at(1.0 - self.alphas_cumprod, t, x_0),
                self._at(self.log_one_minus_alphas_cumprod, t, x_0))

    def q_posterior_mean_variance(self, x_0, x_t, t):
        """q(x_{t-1} | x_t, x_0): mean, variance, clipped log-variance (GaussianDiffusion.py:253-267)."""
        c1, c2 = self._at(self.posterior_mean_coef1, t, x_t), self._at(self.posterior_mean_coef2, t, x_t)
        return (c1 * x_0 + c2 * x_t, self._at(self.posterior_variance, t, x_t),
                self._at(self.posterior_log_variance_clipped, t, x_t))

    def p_mean_variance(self, model, x_t, t, estimate_noise=None):
        """GaussianDiffusion.py:269-296; mean / pred_x_0 come from the fused update kernel."""
        if estimate_noise is None:
            estimate_noise = model(x_t, t)
        if torch.is_grad_enabled() and (x_t.requires_grad or estimate_noise.requires_grad):
            # differentiable API form (the training losses do not come through here: anoddpm_loss_backward carries the VLB
            # term's gradient); fixed-large variance of :282-283
            fixed_var = np.append(self.posterior_variance[1], self.betas[1:])
            pred_x_0 = torch.clamp(self.predict_x_0_from_eps(x_t, t, estimate_noise), -1, 1)
            return {"mean": self.q_posterior_mean_variance(pred_x_0, x_t, t)[0], "variance": self._at(fixed_var, t, x_t),
                    "log_variance": self._at(np.log(fixed_var), t, x_t), "pred_x_0": pred_x_0}
        tb = self._tables(x_t.device)
        tt = self._t64(t, x_t.device)
        _, pred, mean = self._reverse_update(x_t, tt, estimate_noise, None, want_pred=True, want_mean=True)
        shape = x_t.shape
        view = (-1,) + (1,) * (len(shape) - 1)
        return {"mean": mean, "variance": tb.model_variance[tt].view(view).expand(shape),
                "log_variance": tb.model_log_variance[tt].view(view).expand(shape), "pred_x_0": pred}

    def _denoise_noise(self, x_t, t, denoise_fn):
        """Noise selection of sample_p (GaussianDiffusion.py:301-312)."""
        if type(denoise_fn) == str:
            if denoise_fn in ("gauss", "random") and self.gauss_seed is not None:
                return self._seeded_normal(x_t, t, _lib.PHILOX_REVERSE)
            if denoise_fn == "gauss":
                return torch.randn_like(x_t)
            if denoise_fn == "noise_fn":
                return self.noise_fn(x_t, t).float()
            if denoise_fn == "random":
                return torch.randn_like(x_t)
            return generate_simplex_noise(self.simplex, x_t, t, False, in_channels=self.img_channels).float()
        return denoise_fn(x_t, t)

    def sample_p(self, model, x_t, t, denoise_fn="gauss"):
        """One reverse step (GaussianDiffusion.py:298-318): model -> noise -> ONE fused update launch."""
        eps = model(x_t, t)
        noise = self._denoise_noise(x_t, t, denoise_fn)
        sample, pred, _ = self._reverse_update(x_t, t, eps, noise)
        return {"sample": sample, "pred_x_0": pred}

    def forward_backward(self, model, x, see_whole_sequence="half", t_distance=None, denoise_fn="gauss", sampler=None, keep=None,
                         known_noise="fixed", resampling=None):
        """GaussianDiffusion.py:320-359.  `t` lives on the device for the whole chain.  `sampler` (else `self.sampler`): a
        StridedSampler runs the reverse half in ceil(t_distance / stride) steps, and `seq` then holds one image per step.
        `keep` ([B or 1, C or 1, H, W], nonzero = keep): the reverse half is conditioned on `x` itself (KnownRegion) --
        with known_noise "fixed" on the forward noise drawn here for sample_q (the "whole" form, which noises gradually, draws one
        more `noise_fn(x, t_distance - 1)` for it), with "fresh" on a new seeded draw per step.  `resampling` (a Resampling, with
        `keep` only, and never under a sampler -- `self.sampler` included): the reverse half takes the schedule's jumps (DESIGN
        9r), and `seq` holds one image per UNet evaluation."""
        sampler = _check_sampler(sampler) if sampler is not None else self.sampler
        if _check_resampling(resampling) is not None and keep is None:
            raise ValueError("forward_backward: resampling requires `keep` (a known region)")
        assert see_whole_sequence == "whole" or see_whole_sequence == "half" or see_whole_sequence == None

        if t_distance == 0:
            return x.detach()
        if t_distance is None:
            t_distance = self.num_timesteps
        _lib.require_cuda(x, "GaussianDiffusionModel.forward_backward")
        seq = [x.cpu().detach()]
        B = x.shape[0]
        x_in, fwd_noise = x, None
        if see_whole_sequence == "whole":
            for t in range(int(t_distance)):
                t_batch = torch.full((B,), t, device=x.device, dtype=torch.int64)
                noise = self.noise_fn(x, t_batch).float()
                with torch.no_grad():
                    x = self.sample_q_gradual(x, t_batch, noise)
                seq.append(x.cpu().detach())
        else:
            t_tensor = torch.full((B,), t_distance - 1, device=x.device, dtype=torch.int64)
            fwd_noise = self.noise_fn(x, t_tensor).float()
            x = self.sample_q(x, t_tensor, fwd_noise)
            if see_whole_sequence == "half":
                seq.append(x.cpu().detach())

        known = None
        if keep is not None:
            if known_noise == "fixed":
                if fwd_noise is None:
                    fwd_noise = self.noise_fn(x_in, torch.full((B,), t_distance - 1, device=x.device, dtype=torch.int64)).float()
                known_noise = fwd_noise
            known = KnownRegion(x_in, keep, known_noise)
        with torch.no_grad():
            x = self._reverse_chain(model, x, int(t_distance), denoise_fn, seq if see_whole_sequence else None, sampler, known,
                                    resampling)
        return x.detach() if not see_whole_sequence else seq

    p_sample_loop = forward_backward          # north-star alias

    def _chain_for(self, model, x, t_distance, denoise_fn, stream_base=None, sampler=None, known=None, resampling=None,
                   shared_planes=False):
        """A ReverseChain for (model, batch shape, noise source): chains that replay a captured graph are kept -- at most eight,
        oldest dropped first; they hold their model -- and restarted with reset() (same device buffers, same graph); anything
        else is built fresh."""
        cache = self.__dict__.setdefault("_chains", {})
        ReverseChain._check_resample_request(self, denoise_fn, sampler, known, resampling)
        want = ReverseChain._reuse_key_of(self, denoise_fn, sampler, known, resampling, shared_planes)
        if want is not None:
            key = (id(model), tuple(x.shape), str(x.device), want)
            chain = cache.get(key)
            # a kept chain replays the dropout-free inference graph: not for a model that has since been put in train() mode
            # with dropout > 0 (it gets a fresh eager chain below, which is not kept)
            if chain is not None and chain.model is model and not ReverseChain._draws_dropout(model):
                return chain.reset(x, t_distance, stream_base, sampler, known, resampling)
        chain = ReverseChain(self, model, x, t_distance, denoise_fn, stream_base=stream_base, sampler=sampler, known=known,
                             resampling=resampling, shared_planes=shared_planes)
        if chain.use_graph and chain.reuse_key is not None:
            if len(cache) >= 8:
                if x.is_cuda:
                    torch.cuda.synchronize(x.device)              # its captured graph may still be replaying (see _run_chains)
                cache.pop(next(iter(cache)))
            cache[(id(model), tuple(x.shape), str(x.device), chain.reuse_key)] = chain
        return chain

    def _reverse_chain(self, model, x, t_distance, denoise_fn, seq, sampler=None, known=None, resampling=None):
        """t = t_distance-1 ... 0 of sample_p with a device-resident timestep (no per-step H2D); with a `sampler` the
        ceil(t_distance / stride) strided steps."""
        chain = self._chain_for(model, x, t_distance, denoise_fn, sampler=sampler, known=known, resampling=resampling)
        for _ in range(chain.remaining):
            chain.step()
            if seq is not None:
                seq.append(chain.x.cpu().detach())
        chain.finish()
        # a kept chain's buffer is overwritten by the next reset(): hand the caller its own tensor (the reference returns a fresh
        # one from every call, GaussianDiffusion.py:351-359); an un-kept chain's buffer dies with the chain, no copy needed
        return chain.x.clone() if chain in self.__dict__.get("_chains", {}).values() else chain.x

    def release_chains(self):
        """Drop every kept ReverseChain (captured HIP graph + the device buffers and plan it holds: about 3.4 GB per chain at
        config 2); the next forward_backward / detection call builds and captures a fresh one."""
        if self.__dict__.get("_chains") and torch.cuda.is_available():
            torch.cuda.synchronize()                               # no captured graph may be destroyed while a replay is in flight
        self.__dict__.pop("_chains", None)

    def __getstate__(self):
        """Pickle / deepcopy without the device-side caches: kept chains hold CUDAGraph objects, `_dev` holds device tensors.
        `postprocess` / `postprocess_roi` travel like every other plain attribute (they are in `__dict__` once assigned)."""
        d = dict(self.__dict__)
        d.pop("_chains", None)
        d.pop("_gauss_dev", None)
        d.pop("_sampler_dev", None)
        d["_dev"] = {}
        return d

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__getstate__().items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def reverse_chain(self, model, x_t, t_distance, denoise_fn="gauss", sampler=None, known=None, resampling=None):
        """Stepping form of the reverse loop of forward_backward (:351-357): returns a ReverseChain whose
        .step() performs one sample_p on the device-resident state (bench.py times K of these).  `sampler` (else `self.sampler`):
        a StridedSampler makes each step a strided one.  `known`: a KnownRegion makes each step a conditioned one; `resampling`: a
        Resampling adds the schedule's jumps to a conditioned ancestral chain (`remaining` then counts UNet evaluations)."""
        sampler = _check_sampler(sampler) if sampler is not None else self.sampler
        return ReverseChain(self, model, x_t, int(t_distance), denoise_fn, sampler=sampler, known=known, resampling=resampling)

    def sample_q(self, x_0, t, noise):
        """q(x_t | x_0), GaussianDiffusion.py:361-371 -- one fused launch."""
        if torch.is_grad_enabled() and (x_0.requires_grad or noise.requires_grad):
            return self._at(self.sqrt_alphas_cumprod, t, x_0) * x_0 + self._at(self.sqrt_one_minus_alphas_cumprod, t, x_0) * noise
        _lib.require_cuda(x_0, "GaussianDiffusionModel.sample_q")
        tb = self._tables(x_0.device)
        return self._axpby(tb.sqrt_alphas_cumprod, tb.sqrt_one_minus_alphas_cumprod, x_0, t, noise)

    q_sample = sample_q                       # north-star alias

    def sample_q_gradual(self, x_t, t, noise):
        """q(x_t | x_{t-1}), GaussianDiffusion.py:373-382."""
        _lib.require_cuda(x_t, "GaussianDiffusionModel.sample_q_gradual")
        tb = self._tables(x_t.device)
        return self._axpby(tb.sqrt_alphas, tb.sqrt_betas, x_t, t, noise)

    def vlb_terms(self, x_0, x_t, t, eps, noise=None, want_pred=True):
        """Fused variational-bound terms of one step (anoddpm_vlb_terms): returns (vlb [B] in bits/dim,
        mean((pred_x_0-x_0)^2) [B], mean((eps'-noise)^2) [B], pred_x_0 or None).  No autograd."""
        _lib.require_cuda(x_t, "GaussianDiffusionModel.vlb_terms")
        tb = self._tables(x_t.device)
        B = x_t.shape[0]
        x_0, x_t, eps = self._f32(x_0), self._f32(x_t), self._f32(eps)
        noise = self._f32(noise) if noise is not None else None
        tt = self._t64(t, x_t.device)
        out = torch.empty((3, B), dtype=torch.float32, device=x_t.device)
        ws = torch.empty((64 * B * 3,), dtype=torch.float64, device=x_t.device)
        pred = torch.empty_like(x_t) if want_pred else None
        a = VlbArgs()
        a.x0, a.xt, a.eps, a.noise, a.t = ptr(x_0), ptr(x_t), ptr(eps), (ptr(noise) if noise is not None else None), ptr(tt)
        a.c_recip, a.c_recipm1 = ptr(tb.sqrt_recip_alphas_cumprod), ptr(tb.sqrt_recipm1_alphas_cumprod)
        a.c_coef1, a.c_coef2 = ptr(tb.posterior_mean_coef1), ptr(tb.posterior_mean_coef2)
        a.c_post_logvar, a.c_model_logvar = ptr(tb.posterior_log_variance_clipped), ptr(tb.model_log_variance)
        a.pred_x0 = ptr(pred) if pred is not None else None
        a.out, a.workspace, a.workspace_doubles = ptr(out), ptr(ws), ws.numel()
        a.n, a.B, a.T = (x_t[0].numel() if B else 0), B, self.num_timesteps
        check(lib().anoddpm_vlb_terms(ctypes.byref(a), current_stream()), "vlb_terms")
        return out[0], out[1], out[2], pred

    def calc_vlb_xt(self, model, x_0, x_t, t, estimate_noise=None):
        """GaussianDiffusion.py:384-397: KL(q(x_{t-1}|x_t,x_0) || p(x_{t-1}|x_t)) or, at t = 0, the discretised decoder NLL, in
        bits per dimension -- one fused launch after the model call (anoddpm_vlb_terms).  With autograd recording the term is
        differentiable with respect to the model output (anoddpm_loss_backward); `pred_x_0` is returned detached."""
        eps = model(x_t, t) if estimate_noise is None else estimate_noise
        if torch.is_grad_enabled() and eps.requires_grad:
            _, vlb, _ = _FusedLoss.apply(eps, None, x_0, x_t, t, None, self, 3)
            with torch.no_grad():
                pred = self._reverse_update(x_t, t, eps, None, want_pred=True)[1]
            return {"output": vlb, "pred_x_0": pred}
        vlb, _, _, pred = self.vlb_terms(x_0, x_t, t, eps)
        return {"output": vlb, "pred_x_0": pred}

    _LOSS_KINDS = {"l1": 0, "l2": 1, "hybrid": 2}

    def _loss_terms(self, model, x_0, t, weights=None):
        """calc_loss + the weighted batch mean of p_loss: noise draw, q-sample, model call, then ONE fused launch (+ fold) for the
        per-sample terms and the scalar; its autograd backward is one more launch producing d(loss)/d(eps)."""
        noise = self.noise_fn(x_0, t).float()
        x_t = self.sample_q(x_0, t, noise)
        eps = model(x_t, t)
        kind = self._LOSS_KINDS.get(self.loss_type, 1)           # unknown strings mean l2, as upstream's final else (:415-416)
        per, vlb, total = _FusedLoss.apply(eps, noise, x_0, x_t, t, weights, self, kind)
        terms = {"loss": per}
        if kind == 2:
            terms = {"vlb": vlb, "loss": per}
        return terms, x_t, eps, total

    def calc_loss(self, model, x_0, t):
        """GaussianDiffusion.py:399-417 -> (loss dict, x_t, estimate_noise)."""
        terms, x_t, eps, _ = self._loss_terms(model, x_0, t)
        return terms, x_t, eps

    def p_loss(self, model, x_0, args):
        """GaussianDiffusion.py:419-434: draws t (torch.randint, or the weighted numpy draw), returns
        (mean over the batch of loss * weights, (loss dict, x_t, estimate_noise))."""
        B = x_0.shape[0]
        if self.loss_weight == "none":
            hi = min(args["sample_distance"], self.num_timesteps) if args["train_start"] else self.num_timesteps
            t, weights = torch.randint(0, hi, (B,), device=x_0.device), None
        else:
            t, weights = self.sample_t_with_weights(B, x_0.device)
        terms, x_t, eps, total = self._loss_terms(model, x_0, t, weights)
        return total, (terms, x_t, eps)

    def prior_vlb(self, x_0, args):
        """GaussianDiffusion.py:436-443: KL(q(x_T | x_0) || N(0, I)) in bits per dimension."""
        t = torch.full((args["Batch_Size"],), self.num_timesteps - 1, device=x_0.device, dtype=torch.int64)
        mean, _, logvar = self.q_mean_variance(x_0, t)
        zero = torch.zeros((), device=x_0.device)
        return mean_flat(normal_kl(mean, logvar, zero, zero)) / np.log(2.0)

    def calc_total_vlb(self, x_0, model, args):
        """GaussianDiffusion.py:445-478: T model calls; everything after each call (KL / decoder NLL, the two MSE
        curves) is one fused launch, and `t` is the only host-built tensor per step."""
        vb, x_0_mse, mse = [], [], []
        for t in reversed(list(range(self.num_timesteps))):
            t_batch = torch.tensor([t] * args["Batch_Size"], device=x_0.device)
            noise = torch.randn_like(x_0)
            x_t = self.sample_q(x_0=x_0, t=t_batch, noise=noise)
            with torch.no_grad():
                eps = model(x_t, t_batch)
                v, m0, me, _ = self.vlb_terms(x_0, x_t, t_batch, eps, noise=noise, want_pred=False)
            vb.append(v)
            x_0_mse.append(m0)
            mse.append(me)
        vb = torch.stack(vb, dim=1)
        x_0_mse = torch.stack(x_0_mse, dim=1)
        mse = torch.stack(mse, dim=1)
        prior_vlb = self.prior_vlb(x_0, args)
        total_vlb = vb.sum(dim=1) + prior_vlb
        return {"total_vlb": total_vlb, "prior_vlb": prior_vlb, "vb": vb, "x_0_mse": x_0_mse, "mse": mse}

    # ------------------------------------------------------------------ detection compute loops
    def detection_A_fixedT(self, model, x_0, args, mask, end_freq=6):
        """GaussianDiffusion.py:596-623 (pure compute; no file output upstream either)."""
        t_distance = 250
        output = torch.empty((6 * end_freq, 1, *args["img_size"]), device=x_0.device)
        for i in range(1, end_freq + 1):
            freq = 2 ** i
            # == lambda x, t: generate_simplex_noise(self.simplex, x, t, False, frequency=freq).float()   (:602), as an
            # object the reverse chain recognises (per-step seeds pre-drawn in the same numpy-stream order)
            noise_fn = SimplexNoiseFn(self.simplex, frequency=freq)
            t_tensor = torch.tensor([t_distance - 1], device=x_0.device).repeat(x_0.shape[0])
            x = self.sample_q(x_0, t_tensor, noise_fn(x_0, t_tensor).float())
            x_noised = x.clone().detach()
            with torch.no_grad():
                x = self._reverse_chain(model, x, t_distance, noise_fn, None, self.sampler)
            mse = ((x_0 - x).square() * 2) - 1
            mse_threshold = mse > 0
            mse_threshold = (mse_threshold.float() * 2) - 1
            output[(i - 1) * 6:i * 6, ...] = torch.cat((x_0, x_noised, x, mse, mse_threshold, mask))
        return output

    # The (t_distance, avg) loops of detection_A / detection_B.  Upstream runs every chain of one image one after the other
    # (:499-514, :554-569).  The chains are independent of each other -- every (t_distance, avg) pair, and in detection_A every
    # frequency too -- so ALL chains of a call share one batched reverse loop: `slots` device-resident chain slots
    # with a per-slot timestep (the UNet and the fused update take per-sample `t`), stepped together by ONE captured graph; a slot
    # whose chain reaches t = 0 hands its image over and starts the next pending chain (longest first, so the slots drain together).
    # The batch size is therefore constant (the quantisation-free sizes of DESIGN 10-6: 16 by default) whatever `total_avg` and the
    # t_distance sweep are.  The mean / mse / threshold images and the segmentation counts of a setting come from one fused pass
    # (metrics.anomaly_maps).  RNG: the same generators are consumed (np.random for simplex seeds, torch's for randn), the forward
    # noise in upstream's order, but the reverse-step draws of different chains interleave differently from the serial loop, so
    # unseeded outputs are equal in distribution, not sample-for-sample.  After seed_gauss() the gaussian draws of chain c are a
    # function of (seed, stream id of c, timestep, pixel) alone: a sweep is then sample-for-sample the same whatever the
    # slot count and the schedule are, up to the kernels' batch-dependent tiling (1e-4), and bit-identical at equal slot counts.
    def _avg_chains(self, model, x_0, t_distance, total_avg, sampler=None):
        """One setting: `total_avg` chains of the same length as one batch (all slots start and end together)."""
        sampler = _check_sampler(sampler) if sampler is not None else self.sampler
        _lib.require_cuda(x_0, "GaussianDiffusionModel.detection")
        if x_0.shape[0] != 1:
            raise ValueError("detection loops take one image (upstream stores each chain into output[avg], :514)")
        t_tensor = torch.full((1,), int(t_distance), device=x_0.device, dtype=torch.int64)
        noise = torch.cat([self.noise_fn(x_0, t_tensor).float() for _ in range(total_avg)])
        x = self.sample_q(x_0.repeat(total_avg, 1, 1, 1), t_tensor.repeat(total_avg), noise)
        with torch.no_grad():
            return self._reverse_chain(model, x, int(t_distance), "gauss", None, sampler)      # sample_p default noise, :508

    def _forward_noise(self, x_0, t_distance, n):
        """`n` draws of the forward noise of one setting, in upstream's order (:501-505, :556-560).  None from the seeded gaussian
        `noise_fn`: `_run_chains` then generates the forward noise of its chains inside the q-sample kernel."""
        if self.gauss_seed is not None and isinstance(self.noise_fn, GaussNoiseFn):
            return []
        t_tensor = torch.full((1,), int(t_distance), device=x_0.device, dtype=torch.int64)
        return [self.noise_fn(x_0, t_tensor).float() for _ in range(n)]

    def _run_chains(self, model, x_0, t_distances, noise, slots=None, sampler=None, known=None, resampling=None):
        """Reverse chains of ONE image with individual lengths, batched over `slots` chain slots.

        t_distances[c] / noise[c]: chain c is `sample_q(x_0, t_distances[c], noise[c])` followed by t_distances[c] steps of
        `sample_p(model, x, t)` with the default gaussian step noise (GaussianDiffusion.py:501-512, 556-567).  On a seeded instance
        (seed_gauss) chain c draws its step noise from stream `base + c`, `base` being the allocator position at the call, and
        `noise=None` asks for the seeded forward noise of the same streams.  Returns the final
        images, [len(t_distances), C, H, W].  The schedule (which slot, which global step) is kept in `self.last_chain_schedule`.
        `sampler` (else `self.sampler`): with a StridedSampler chain c takes ceil(t_distances[c] / stride) strided steps, and the
        schedule counts those.
        `known` (a KnownRegion of ONE image: x_0 and keep of batch 1, noise "fixed" or "fresh"): every step is the conditioned one
        (DESIGN 9q), the image and keep planes shared by all slots; with "fixed" the known-region noise of chain c is the forward
        noise chain c was noised with, copied into the slot's plane on refill.  `resampling` (a Resampling, with `known`, never
        with a sampler): chain c takes resampling.steps(t_distances[c]) evaluations, the schedule counts those, and a refill also
        writes the slot's (top, rep, visit).  Neither is taken from `self`: the detection routines hand them over."""
        import os
        _lib.require_cuda(x_0, "GaussianDiffusionModel.detection")
        if x_0.shape[0] != 1:
            raise ValueError("detection loops take one image (upstream stores each chain into output[avg], :514)")
        sampler = _check_sampler(sampler) if sampler is not None else self.sampler
        ReverseChain._check_resample_request(self, "gauss", sampler, _check_known(known), resampling)
        if known is not None:
            known.check_batch((1,) + tuple(x_0.shape[1:]))
            if torch.is_tensor(known.noise):
                raise ValueError("_run_chains: the fixed known-region noise of a sweep is each chain's own forward noise; a noise "
                                 "tensor is refused -- use noise='fixed' or 'fresh'")
            known_mode = ReverseChain._known_mode_of(self, "gauss", known)
        n = len(t_distances)
        lens = [int(d) for d in t_distances]
        steps = lens if sampler is None else [sampler.steps(l) for l in lens]      # reverse steps of each chain
        if resampling is not None:
            steps = [resampling.steps(l) for l in lens]
        out = torch.empty((n,) + tuple(x_0.shape[1:]), device=x_0.device, dtype=torch.float32)
        if n == 0:
            return out
        if min(lens) < 0 or max(lens) > self.num_timesteps - 1:
            # sample_q at t = t_distance reads the T-entry tables: upstream's extract() raises for t_distance >= T
            raise IndexError(f"t_distance {max(lens)} is out of range for a {self.num_timesteps}-step schedule")
        if slots is None and os.environ.get("ANODDPM_DET_SLOTS"):
            try:
                slots = int(os.environ["ANODDPM_DET_SLOTS"])
            except ValueError:
                slots = 0
            if slots < 1:
                raise ValueError(f"ANODDPM_DET_SLOTS={os.environ['ANODDPM_DET_SLOTS']!r}: expected an integer >= 1")
        if slots is not None and int(slots) < 1:
            raise ValueError("_run_chains: slots must be >= 1")
        auto = slots is None
        if auto:
            per_slot = 24.0 * 4.0 * float(getattr(model, "model_channels", 128)) * x_0.shape[-1] * x_0.shape[-2]
            free = torch.cuda.mem_get_info(x_0.device)[0] if x_0.is_cuda else float("inf")
            slots = choose_slots(steps, n, per_slot, free)
        G = max(1, min(int(slots), n))
        t_all = torch.tensor(lens, device=x_0.device, dtype=torch.int64)
        seeded = self.gauss_seed is not None
        base = self._take_streams(n) if seeded else None
        fixed = known is not None and known_mode == "fixed"                # the chains' forward noise is kept for the known region
        if noise is None and seeded:
            x_start, noise = self._q_sample_gauss(x_0.repeat(n, 1, 1, 1), t_all, base, want_noise=fixed)
        else:
            x_start = self.sample_q(x_0.repeat(n, 1, 1, 1), t_all, noise)
        if fixed:
            noise = self._f32(noise).to(x_0.device)
        live = [c for c in range(n) if lens[c] > 0]
        live_steps = [steps[c] for c in live]
        for c in range(n):
            if lens[c] == 0:
                out[c].copy_(x_start[c])                               # no reverse step: the noised image itself
        cache = self.__dict__.setdefault("_chains", {})
        while live:                                                    # until a chain AND its plan for G slots are secured
            # kept slot chains of this model at OTHER slot counts are superseded (each holds a plan + captured graph: 3.4 GB per
            # four images at config 2): drop them before the new plan is allocated (round-5 advisor finding)
            stale = [k for k, ch in cache.items() if getattr(ch, "slot_chain", False) and k[0] == id(model)
                     and k[1][1:] == tuple(x_start.shape[1:]) and k[1][0] != G]
            if stale:
                # the dropped chains' captured graphs may still have replays (and the copies that harvested their last images) in
                # flight on this stream: let the device finish before their hipGraphExec objects are destroyed
                torch.cuda.synchronize(x_start.device)
                for key in stale:
                    cache.pop(key)
            try:
                with torch.no_grad():
                    chain = self._chain_for(model, x_start[:1].expand(G, -1, -1, -1).contiguous(), 1, "gauss", stream_base=base,
                                            sampler=sampler, known=known, resampling=resampling, shared_planes=known is not None)
                    chain.slot_chain = True
                    if chain.hip_model:
                        model._plan_for(G, x_start.shape[2], x_start.device)     # the large allocation: not left to the first step
                break
            except torch.cuda.OutOfMemoryError:
                if not auto or G == 1:
                    raise
            # the estimate was too optimistic: halve the slots (the next turn drops the chain just kept as superseded).  Here, outside
            # the `except` block, the traceback no longer pins the failed allocations: emptying the cache returns them to the device
            torch.cuda.empty_cache()
            G //= 2
        makespan, place = plan_chain_slots(live_steps, G)
        self.last_chain_schedule = {"slots": G, "steps": makespan, "chain_steps": sum(steps), "place": dict(zip(live, place))}
        if not live:
            return out
        refill, harvest, last_busy = slot_events(place, live_steps, G)
        with torch.no_grad():
            chain.remaining = makespan
            for slot in range(G):
                if last_busy[slot] == 0:                                # no chain (n counts the zero-length ones): a valid timestep to idle on
                    chain.t[slot:slot + 1].fill_(makespan - 1)
            if resampling is not None:
                chain.rs_top.fill_(-1)                                  # a slot without a chain never jumps; refills write the rest
            for k in range(makespan):
                for slot, i in refill.get(k, ()):
                    c = live[i]
                    chain.x[slot].copy_(x_start[c])
                    chain.t[slot:slot + 1].fill_(lens[c] - 1)
                    if seeded:
                        chain.streams[slot:slot + 1].fill_(philox.signed32(base + c))
                    if fixed:
                        chain.k_noise[slot].copy_(noise[c])
                    if resampling is not None:
                        chain.rs_top[slot:slot + 1].fill_(lens[c] - 1)
                        chain.rs_rep[slot:slot + 1].fill_(resampling.reps - 1)
                        chain.rs_visit[slot:slot + 1].zero_()
                chain.step()
                for slot, i in harvest.get(k, ()):
                    out[live[i]].copy_(chain.x[slot])
                    if last_busy[slot] == k + 1 and k + 1 < makespan and resampling is not None:
                        chain.rs_top[slot:slot + 1].fill_(-1)           # idle: never jumps; the advance floors its t at 0
                    elif last_busy[slot] == k + 1 and k + 1 < makespan and sampler is None:
                        # nothing left for this slot: it idles on its last image with a timestep that stays >= 0 to the end
                        # (a strided chain's advance floors t at 0 by itself)
                        chain.t[slot:slot + 1].fill_(makespan - k - 2)
            chain.finish()
        return out

    # A record's scores, under the names `metrics.score_maps` gives them: (key, the options that put the key into every record --
    # None where nothing fills it; None: only when it is filled).  Row j of the result belongs to record j.
    _RECORD_SCORES = tuple((k, ()) for k in ("auc", "auc_status", "ap", "best_dice", "best_threshold", "ssim")) \
        + tuple((k, ("postprocess",)) for k in ("sqerr_pp", "auc_pp", "ap_pp", "best_dice_pp", "best_threshold_pp")) \
        + (("aupro", ("pro_limit",)), ("aupro_pp", ("pro_limit", "postprocess"))) \
        + tuple((k, None) for k in ("hd", "hd95", "assd", "hd_pp", "hd95_pp", "assd_pp")) \
        + tuple((k, ("image_top",)) for k in ("image_max", "image_topk")) \
        + tuple((k, ("image_top", "postprocess")) for k in ("image_max_pp", "image_topk_pp"))

    def _score_settings(self, settings, outputs, total_avg, x_0, mask):
        """The end of detection_A / detection_B: settings[j] (the keys that name a setting) owns the `total_avg` chains
        outputs[j * total_avg:(j + 1) * total_avg]; one record per setting, in that order -> `self.last_detection`.  The mean / mse /
        threshold images and the counts come from one fused pass per setting, every score of `_RECORD_SCORES` from ONE
        `metrics.score_maps` over all settings (one launch per step for the whole sweep; fp64 device scalars, `ssim` [B] per record;
        never synchronises).  `auc` ... `ssim` stay None where nothing fills them (no mask, images below the SSIM window); the opt-in
        `self.postprocess` (with `self.postprocess_roi`) and `self.pro_limit` add their keys, None without a mask;
        `self.surface_metrics` adds `hd`, `hd95`, `assd` (and `_pp`) only with a mask; `self.image_top` adds `image_max` and
        `image_topk` (and `_pp`), [B] per record, mask or not.  All unset: exactly the first six.
        `self.operating_thresholds` ([T], on the device) adds `dice_at`, `precision_at`, `recall_at`, `fpr_at`, fp64 [T] per record:
        `metrics.scores_at` of every setting's squared-error map (its B images pooled, as `auc` pools them) from ONE
        `anoddpm_threshold_counts` call for the whole sweep; without a mask every pixel is a negative and only `fpr_at` is a number."""
        from . import metrics
        self.last_detection, stacks = [], {"mean": [], "sqerr": [], "thr_img": []}
        for j, extra in enumerate(settings):
            output = outputs[j * total_avg:(j + 1) * total_avg].clone()
            maps, counts = metrics.anomaly_maps(x_0, output, mask, threshold=0.5)
            self.last_detection.append(dict(extra, output=output, mean=maps["mean"], mse=maps["mse_img"], threshold=maps["thr_img"], counts=counts))
            for k, stack in stacks.items():
                stack.append(maps[k])
        if not settings:
            return
        scores = metrics.score_maps(x_0, *(torch.stack(stacks[k]) for k in ("mean", "sqerr", "thr_img")), mask, postprocess=self.postprocess,
                                    roi=self.postprocess_roi, pro_limit=self.pro_limit, surface=bool(self.surface_metrics),
                                    image_top=self.image_top)
        for j, rec in enumerate(self.last_detection):
            for key, options in self._RECORD_SCORES:
                if key in scores:
                    rec[key] = scores[key][j]
                elif options is not None and all(getattr(self, o) is not None for o in options):
                    rec[key] = None
        if self.operating_thresholds is not None:
            sq = torch.stack(stacks["sqerr"]).reshape(len(settings), -1)
            at = metrics.scores_at(mask if mask is not None else torch.zeros_like(sq[0]), sq, self.operating_thresholds.reshape(-1), batched=True)
            for j, rec in enumerate(self.last_detection):
                rec.update({k + "_at": at[k][j] for k in ("dice", "precision", "recall", "fpr")})

    def _detection_conditioning(self, x_0):
        """What `detection_keep` / `resampling` add to the sweep's `_run_chains` call; both unset: nothing at all."""
        if self.detection_keep is None:
            if self.resampling is not None:
                raise ValueError("detection: `resampling` is set without `detection_keep`; resampling needs a known region")
            return {}
        keep = self.detection_keep
        if not torch.is_tensor(keep) or keep.dim() not in (3, 4):
            raise ValueError("detection_keep must be a mask tensor [1 or C, H, W] or [1, 1 or C, H, W]")
        keep = keep if keep.dim() == 4 else keep[None]
        return {"known": KnownRegion(x_0, keep.to(x_0.device), noise="fixed"), "resampling": self.resampling}

    def detection_A(self, model, x_0, args, file, mask, total_avg=2):
        """GaussianDiffusion.py:480-529: simplex frequencies 2^7..2^1 x t_distance 50..0.6T step 50, `total_avg` chains each -- all
        of them one batched reverse loop (`_run_chains`).  Returns None as upstream; the per-setting results upstream only plots
        (the figure files are file / plot I/O, out of scope) are kept in `self.last_detection`, in upstream's loop order: mean /
        mse / threshold images, the segmentation counts and (with a mask) the ROC AUC of the squared-error map, on the device."""
        settings, dists, noise = [], [], []
        for i in range(7, 0, -1):
            freq = 2 ** i
            self.noise_fn = SimplexNoiseFn(self.simplex, frequency=freq, in_channels=self.img_channels)     # :491-494
            for t_distance in range(50, int(args["T"] * 0.6), 50):
                settings.append({"freq": i, "t_distance": t_distance})
                dists += [t_distance] * total_avg
                noise += self._forward_noise(x_0, t_distance, total_avg)
        outputs = self._run_chains(model, x_0, dists, torch.cat(noise) if noise else None, **self._detection_conditioning(x_0))
        self._score_settings(settings, outputs, total_avg, x_0, mask)

    def detection_B(self, model, x_0, args, file, mask, denoise_fn="gauss", total_avg=5):
        """GaussianDiffusion.py:531-594: t_distance 50..end step 50 with gaussian or 6-octave simplex forward noise,
        `total_avg` chains each -- all (t_distance, avg) chains one batched reverse loop (`_run_chains`).  Returns the list upstream
        returns -- the values of `evaluation.heatmap(...)`, which are None -- and keeps the device-side results in
        `self.last_detection` (the figures upstream writes are out of scope)."""
        assert type(file) == tuple
        if denoise_fn == "octave":
            end = int(args["T"] * 0.6)
            self.noise_fn = SimplexNoiseFn(self.simplex, octave=6, persistence=0.8, frequency=64)           # :547-550
        else:
            end = int(args["T"] * 0.8)
            self.noise_fn = GaussNoiseFn(self)
        settings = list(range(50, end, 50))
        dists, noise = [], []
        for t_distance in settings:
            dists += [t_distance] * total_avg
            noise += self._forward_noise(x_0, t_distance, total_avg)
        outputs = self._run_chains(model, x_0, dists, torch.cat(noise) if noise else None, **self._detection_conditioning(x_0))
        self._score_settings([{"t_distance": t_distance} for t_distance in settings], outputs, total_avg, x_0, mask)
        return [None] * len(settings)                               # evaluation.heatmap() returns None (evaluation.py:12-22)

    def detection_two_pass(self, model, x_0, mask, threshold, t_first, t_second, total_avg=5, dilate=2, smooth=None, roi=None,
                           resampling=None, denoise_fn="gauss"):
        """Two-pass detection (the mask / stitch / resample of AutoDDPM, Bercea et al., 2023) of ONE image; no
        counterpart upstream.  Pass 1: `total_avg` unconditioned chains of length `t_first`, forward noise drawn as detection_B
        draws it (`denoise_fn` "gauss" or "octave").  Their squared error against `x_0` (the maximum over the channels; with
        `smooth=sigma` through `metrics.gaussian_filter`) is the score plane; `metrics.keep_mask(score, threshold, dilate, roi)` marks
        what exceeds `threshold` (a number or a device tensor, e.g. `HealthyPool.thresholds`; never read on the host), grown by
        `dilate` pixels, as the region to regenerate and stitches the start image: the first pass's mean there, `x_0` elsewhere.
        Pass 2: for every entry of `t_second` (an int or a list) `total_avg` chains from the stitched image, every step conditioned
        on it outside the region (KnownRegion(stitched, keep, "fixed")), with `resampling` (else `self.resampling`) and
        `self.sampler` as in any conditioned sweep -- all in one `_run_chains` call, on pass 1's slot count so that neither pass
        drops the other's kept graph.  Nothing exceeds the threshold: pass 2 keeps everything and returns the input, "nothing found".
        Returns None; `self.last_detection` holds one record for pass 1 ({"t_distance": t_first, "pass": 1, ...}) and one per entry
        of `t_second` ({"t_distance": t2, "pass": 2, "t_first": t_first, ...}), scored against `x_0` and `mask` by one
        `_score_settings`; every record also carries `keep` (uint8 [1, 1, H, W]) and `regen` (int32 [1], on the device).  On a seeded
        owner stream ids are taken in order: pass 1's chains, then pass 2's in setting order.  Between the passes and through the
        scoring nothing synchronises with the host.  What this does to detection quality has not been measured."""
        from . import metrics
        if denoise_fn not in ("gauss", "octave"):
            raise ValueError(f"detection_two_pass: denoise_fn must be 'gauss' or 'octave', got {denoise_fn!r}")
        if isinstance(dilate, bool) or not isinstance(dilate, (int, np.integer)) or not 0 <= dilate <= _lib.KEEP_DILATE_MAX:
            raise ValueError(f"detection_two_pass: dilate must be an integer in 0 ... {_lib.KEEP_DILATE_MAX}, got {dilate!r}")
        if not torch.is_tensor(x_0) or x_0.dim() != 4 or x_0.shape[0] != 1:
            raise ValueError("detection_two_pass: x_0 must be one image [1, C, H, W] (the detection loops take one image)")
        if isinstance(total_avg, bool) or not isinstance(total_avg, (int, np.integer)) or total_avg < 1:
            raise ValueError(f"detection_two_pass: total_avg must be an integer >= 1, got {total_avg!r}")
        seconds = [t_second] if isinstance(t_second, (int, np.integer)) and not isinstance(t_second, bool) else list(t_second)
        for name, v in [("t_first", t_first)] + [("t_second", v) for v in seconds]:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= self.num_timesteps - 1:
                raise ValueError(f"detection_two_pass: {name} {v!r} is outside the schedule (an integer in 0 ... {self.num_timesteps - 1})")
        resampling = _check_resampling(resampling) if resampling is not None else self.resampling
        # what pass 2's sweep refuses (a sampler together with a resampling), before pass 1 is run: pass 2 always has a known region
        ReverseChain._check_resample_request(self, "gauss", self.sampler, True, resampling)
        t_first, seconds = int(t_first), [int(v) for v in seconds]
        if denoise_fn == "octave":
            self.noise_fn = SimplexNoiseFn(self.simplex, octave=6, persistence=0.8, frequency=64)
        else:
            self.noise_fn = GaussNoiseFn(self)
        noise = self._forward_noise(x_0, t_first, total_avg)
        outputs1 = self._run_chains(model, x_0, [t_first] * total_avg, torch.cat(noise) if noise else None)
        slots = self.last_chain_schedule["slots"]
        maps, _ = metrics.anomaly_maps(x_0, outputs1, None, want=("mean", "sqerr"))
        score = maps["sqerr"] if x_0.shape[1] == 1 else maps["sqerr"].amax(dim=1, keepdim=True)
        if smooth is not None:
            score = metrics.gaussian_filter(score, sigma=smooth)
        km = metrics.keep_mask(score[:, 0], threshold, dilate, roi, real=x_0, recon=maps["mean"])
        stitched, keep = km["stitched"], km["keep"]
        dists, noise = [], []
        for t2 in seconds:
            dists += [t2] * total_avg
            noise += self._forward_noise(stitched, t2, total_avg)
        outputs2 = self._run_chains(model, stitched, dists, torch.cat(noise) if noise else None, slots=slots,
                                    known=KnownRegion(stitched, keep, "fixed"), resampling=resampling)
        settings = [{"t_distance": t_first, "pass": 1}] + [{"t_distance": t2, "pass": 2, "t_first": t_first} for t2 in seconds]
        self._score_settings(settings, torch.cat((outputs1, outputs2)), total_avg, x_0, mask)
        for rec in self.last_detection:
            rec["keep"], rec["regen"] = keep, km["regen"]
