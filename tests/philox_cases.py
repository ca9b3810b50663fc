"""The seeded Gaussian stream of DESIGN 9g restated in numpy (uint64 integer arithmetic, fp64 Box-Muller), and the key list the
CPU and GPU tests share.  Independent of the library: nothing here imports anoddpm_amd."""
import itertools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57                  # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                  # Weyl constants of the key schedule
MASK = np.uint64(0xFFFFFFFF)

SEEDS = (0, 1234, 0x0123456789ABCDEF, 2 ** 64 - 1)
STREAMS = (0, 7, 2 ** 32 - 1)
STEPS = (0, 249, 999)
DOMAINS = (0, 1, 2)
KEYS = list(itertools.product(SEEDS, STREAMS, STEPS, DOMAINS))

# Random123's known answers for philox4x32-10: (counter, key, output)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on arrays (or scalars) of counters: -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c0                                      # < 2^64: no wrap
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def bits(seed, stream, step, domain, n, quad0=0):
    """The first n words of one sample (uint32[n]): element i is word i & 3 of counter (quad0 + (i >> 2), stream, step, domain)."""
    nq = (n + 3) // 4
    w = philox4x32_10(np.arange(quad0, quad0 + nq, dtype=np.uint64), stream, step, domain, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=1).reshape(-1)[:n].astype(np.uint32)


def unit(w):
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(seed, stream, step, domain, n):
    """-> (z, r): the n normals of one sample in fp64 and, per element, the radius sqrt(-2 ln u) of its pair."""
    w = bits(seed, stream, step, domain, 4 * ((n + 3) // 4)).reshape(-1, 2, 2)          # [quad][pair][radius word, angle word]
    r = np.sqrt(-2.0 * np.log(unit(w[:, :, 0])))
    ang = 2.0 * np.pi * unit(w[:, :, 1])
    z = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=2).reshape(-1)[:n]
    return z, np.repeat(r.reshape(-1), 2)[:n]
