"""Seeded, counter-based Gaussian noise: thin wrappers over anoddpm_philox_fill / anoddpm_philox_bits_host.

A value is a pure function of (seed, stream, step, domain, element index inside the sample): it does not depend on the batch a
sample is generated in, on the launch shape or on what was generated before.  The diffusion kernels generate the same values in
registers (anoddpm_p_sample_update_gauss, anoddpm_q_sample_gauss); these functions materialise them."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import PHILOX_FILL, PHILOX_FORWARD, PHILOX_REVERSE, check, current_stream, lib, ptr

__all__ = ["bits", "normal", "host_bits", "PHILOX_REVERSE", "PHILOX_FORWARD", "PHILOX_FILL"]

_U64 = (1 << 64) - 1
_U32 = (1 << 32) - 1


def seed_tensor(seed, device):
    """The 64-bit seed as the device word the kernels read (int64 holding the same bits)."""
    seed = int(seed) & _U64
    return torch.tensor([seed - (1 << 64) if seed >> 63 else seed], dtype=torch.int64, device=device)


def signed32(v):
    """v mod 2^32 as the int32 value with the same bits (what an int32 tensor of stream ids holds)."""
    v = int(v) & _U32
    return v - (1 << 32) if v >> 31 else v


def stream_ids(base, count):
    """`count` consecutive stream ids from `base` (mod 2^32) as the int32 words the kernels reinterpret: host tensor."""
    ids = (np.arange(count, dtype=np.uint64) + np.uint64(int(base) & _U32)).astype(np.uint32)
    return torch.from_numpy(ids.view(np.int32))


def _per_sample(v, B, device, words, what):
    """int -> None (passed by value); tensor / sequence -> contiguous device tensor [B]: int32 words (`words`, values taken
    mod 2^32) or int64."""
    if isinstance(v, (int, np.integer)):
        return None
    if not torch.is_tensor(v):
        v = np.asarray(v, dtype=np.int64).reshape(-1)
        v = torch.from_numpy(v.astype(np.uint32).view(np.int32) if words else v)
    elif words and v.dtype != torch.int32:
        v = v.to(torch.int64) & _U32
        v = torch.where(v > 0x7FFFFFFF, v - (1 << 32), v).to(torch.int32)
    elif not words:
        v = v.to(torch.int64)
    v = v.to(device).reshape(-1)
    if v.numel() == 1 and B != 1:
        v = v.expand(B)
    if v.numel() != B:
        raise ValueError(f"philox: {what} has {v.numel()} entries for {B} samples")
    return v.contiguous()


def _fill(kind, seed, shape, stream, step, domain, device, T):
    shape = tuple(int(s) for s in shape)
    if not shape:
        raise ValueError("philox: shape needs a leading sample dimension")
    if torch.is_tensor(seed):
        device = seed.device
        seed_dev = seed
    else:
        seed_dev = seed_tensor(seed, device)
    _lib.require_cuda(seed_dev, "philox")
    B = shape[0]
    n = int(np.prod(shape[1:], dtype=np.int64)) if B else 0
    out = torch.empty(shape, dtype=torch.float32 if kind else torch.int32, device=seed_dev.device)
    streams = _per_sample(stream, B, seed_dev.device, True, "stream")
    t = _per_sample(step, B, seed_dev.device, False, "step")
    check(lib().anoddpm_philox_fill(ptr(out), kind, B, n, ptr(seed_dev), ptr(streams), (int(stream) & _U32) if streams is None else 0,
                                    int(domain), ptr(t), (int(step) & _U32) if t is None else 0, int(T), current_stream()), "philox_fill")
    return out


def bits(seed, shape, stream=0, step=0, domain=PHILOX_FILL, device="cuda", T=0):
    """Raw 32-bit words, int32 tensor of `shape` = [B, ...] (read them as uint32): sample b is stream `stream + b` (int) or
    `stream[b]`, at step `step` (int) or `step[b]`.  `seed`: an int, or a device int64[1] tensor holding its bits.
    T > 0: negative steps mean step + T."""
    return _fill(0, seed, shape, stream, step, domain, device, T)


def normal(seed, shape, stream=0, step=0, domain=PHILOX_FILL, device="cuda", T=0):
    """Standard normals, fp32 tensor of `shape` = [B, ...]; arguments as `bits`."""
    return _fill(1, seed, shape, stream, step, domain, device, T)


def host_bits(seed, stream, step, domain, nquads, quad0=0):
    """The words of `nquads` consecutive counters computed on the host (no GPU): uint32 array [4 * nquads]."""
    out = np.empty(4 * int(nquads), dtype=np.uint32)
    check(lib().anoddpm_philox_bits_host(int(seed) & _U64, int(stream) & _U32, int(step) & _U32, int(domain) & _U32,
                                         int(quad0) & _U32, int(nquads), out.ctypes.data_as(ctypes.c_void_p)), "philox_bits_host")
    return out
