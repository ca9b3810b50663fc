"""The seeded Gaussian stream without a GPU: the numpy restatement against Random123's known answers, the library's
host routine against the restatement, the distribution of the restatement's normals, and the host-side stream bookkeeping."""
import copy
import pickle

import numpy as np
import pytest

import philox_cases as pc

N = 1 << 20
DIST_KEYS = [(1234, 0, 0, 2), (1234, 1, 0, 2), (1234, 0, 1, 2), (1234, 0, 0, 0), (0x0123456789ABCDEF, 7, 249, 0)]
SIGMA5 = 5.0 / np.sqrt(N)                                        # 5 sigma of a mean of N unit-variance terms: 4.9e-3


def test_restatement_reproduces_random123_known_answers():
    for ctr, key, out in pc.KAT:
        got = tuple(int(w[0]) for w in pc.philox4x32_10(*ctr, *key))
        assert got == out, [hex(g) for g in got]


def test_restatement_reproduces_the_quoted_stream_values():
    b = pc.bits(0x0123456789ABCDEF, 7, 249, 0, 24)
    assert [int(w) for w in b[:4]] == [0xd5aeeaaa, 0xcd7f576e, 0x1dff3d56, 0x219a3bd8]
    assert [int(w) for w in b[20:24]] == [0xa066267b, 0xf4519cdc, 0x9343281f, 0xe9dbd6db]
    z, r = pc.normals(0x0123456789ABCDEF, 7, 249, 0, 4)
    assert np.allclose(z, [0.19551992, -0.56845147, 1.40555979, 1.52071042], rtol=0, atol=5e-9)
    assert r[0] == r[1] and r[2] == r[3] and np.isclose(r[0] ** 2, z[0] ** 2 + z[1] ** 2)
    # a partial tail uses the leading lanes of its quad; quad0 offsets the counter
    assert np.array_equal(pc.bits(1234, 7, 249, 1, 5), pc.bits(1234, 7, 249, 1, 8)[:5])
    assert np.array_equal(pc.bits(1234, 7, 249, 1, 8, quad0=3), pc.bits(1234, 7, 249, 1, 20)[12:])


@pytest.mark.parametrize("nquads", [1, 2, 257])
def test_host_routine_equals_restatement(nquads):
    from anoddpm_amd import philox
    for key in pc.KEYS:
        got = philox.host_bits(*key, nquads)
        assert got.dtype == np.uint32 and np.array_equal(got, pc.bits(*key, 4 * nquads)), key
    assert np.array_equal(philox.host_bits(1234, 7, 249, 0, nquads, quad0=2 ** 32 - 1)[:4], pc.bits(1234, 7, 249, 0, 4, quad0=2 ** 32 - 1))


def test_host_routine_validates():
    from anoddpm_amd import _lib
    L = _lib.lib()
    assert L.anoddpm_philox_bits_host(0, 0, 0, 0, 0, 1, None) == -1 and b"philox_bits_host" in L.anoddpm_last_error()
    assert L.anoddpm_philox_bits_host(0, 0, 0, 0, 0, 0, None) == 0
    # no launch without a seed pointer (checked before anything touches the device)
    assert L.anoddpm_philox_fill(1, 1, 1, 4, None, None, 0, 2, None, 0, 0, None) == -1 and b"null seed" in L.anoddpm_last_error()
    assert L.anoddpm_philox_fill(1, 2, 1, 4, None, None, 0, 2, None, 0, 0, None) == -1 and b"kind" in L.anoddpm_last_error()


@pytest.fixture(scope="module")
def draws():
    return {k: pc.normals(*k, N)[0] for k in DIST_KEYS + [(1235, 0, 0, 2)]}


@pytest.mark.parametrize("key", DIST_KEYS)
def test_moments_and_autocorrelation(draws, key):
    z = draws[key]
    assert z.shape == (N,) and np.isfinite(z).all()
    m, v, k4 = z.mean(), z.var(), (z ** 4).mean()
    lags = {lag: float((z[:-lag] * z[lag:]).mean()) for lag in (1, 2, 4)}
    print(key, "mean %.2e var-1 %.2e m4-3 %.2e" % (m, v - 1, k4 - 3), lags)
    assert abs(m) < SIGMA5
    assert abs(v - 1.0) < 5.0 * np.sqrt(2.0 / N)
    assert abs(k4 - 3.0) < 5.0 * np.sqrt(96.0 / N)
    for lag, c in lags.items():
        assert abs(c) < SIGMA5, (lag, c)


@pytest.mark.parametrize("other", DIST_KEYS[1:] + [(1235, 0, 0, 2)])
def test_streams_steps_domains_and_seeds_are_uncorrelated(draws, other):
    c = float((draws[DIST_KEYS[0]] * draws[other]).mean())
    print(other, "cross-correlation %.2e" % c)
    assert abs(c) < SIGMA5


def test_stream_bookkeeping(monkeypatch):
    import GaussianDiffusion as GD
    monkeypatch.delenv("ANODDPM_GAUSS_SEED", raising=False)
    mk = lambda: GD.GaussianDiffusionModel([32, 32], GD.get_beta_schedule(100, "linear"), noise="gauss")
    d = mk()
    assert d.gauss_seed is None and d.gauss_next_stream == 0
    key = GD.ReverseChain._reuse_key_of
    assert key(d, "gauss") == key(d, "noise_fn") == ("gauss",)
    d.seed_gauss(5)
    assert d.gauss_seed == 5 and d.gauss_next_stream == 0
    assert key(d, "gauss") == key(d, "random") == key(d, "noise_fn") != ("gauss",)      # never the unseeded chain's graph
    assert d._take_streams(9) == 0 and d._take_streams(3) == 9 and d.gauss_next_stream == 12
    d2, d3 = copy.deepcopy(d), pickle.loads(pickle.dumps(d))
    for c in (d2, d3):
        assert (c.gauss_seed, c.gauss_next_stream) == (5, 12)
        assert c.noise_fn.owner is c and c.noise_fn is c._default_noise_fn
        assert c._take_streams(1) == 12
    assert d.gauss_next_stream == 12                             # the copies advance on their own
    d.seed_gauss(6)
    assert d.gauss_seed == 6 and d.gauss_next_stream == 0        # re-seeding rewinds the allocator
    d.seed_gauss(2 ** 64 + 3)
    assert d.gauss_seed == 3
    d.gauss_next_stream = 2 ** 32 - 1
    assert d._take_streams(2) == 2 ** 32 - 1 and d.gauss_next_stream == 1               # ids wrap mod 2^32
    d.seed_gauss(None)
    assert d.gauss_seed is None and key(d, "gauss") == ("gauss",)
    monkeypatch.setenv("ANODDPM_GAUSS_SEED", "0x10")
    assert mk().gauss_seed == 16
    s = GD.GaussianDiffusionModel([32, 32], GD.get_beta_schedule(100, "linear"), noise="simplex")
    s.seed_gauss(5)
    assert key(s, "noise_fn")[0] == "simplex" and key(s, "gauss") == ("gauss", "seeded")
