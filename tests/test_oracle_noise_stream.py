"""CPU: oracle/noise_stream.py -- the NumPy restatement of the device N(0,1) stream (philox_normal) -- against Random123's
Philox4x32-10 known answers, a scalar restatement in Python integers, the float32 rounding of the uniforms at their edges,
and the statistics a Gaussian noise stream must have."""
import math

import numpy as np
import pytest

from oracle import noise_stream as ns

M32 = 0xFFFFFFFF

# Random123 (kat_vectors): philox4x32 with 10 rounds, (counter c0..c3, key k0 k1) -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((M32,) * 4, (M32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def philox_scalar(c, k):
    """Philox4x32-10 on Python integers, one counter at a time (the kernel's round, spelled out)."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform_exact(word):
    """(float32(x) + 0.5f) * 2^-24 with x = word >> 8, as an exact fraction: below 2^23 the sum is exact; from 2^23 on the
    float32 spacing is 1 and the tie x + 0.5 rounds to the even neighbour."""
    x = word >> 8
    return (2 * x + 1) / 2.0 ** 25 if x < 2 ** 23 else (x + (x & 1)) / 2.0 ** 24


def normal_scalar(seed, step, idx, stream):
    w = philox_scalar((idx, stream, step & M32, step >> 32), (seed & M32, seed >> 32))
    u1, u2 = uniform_exact(w[0]), uniform_exact(w[1])
    theta = float(np.float32(np.float32(6.28318530717958647692) * np.float32(u2)))
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(theta)


@pytest.mark.parametrize("c,k,want", KAT)
def test_philox_known_answers(c, k, want):
    got = ns.philox4x32(*c, *k)
    assert tuple(int(x) for x in got) == want
    assert philox_scalar(c, k) == want


def test_vectorised_equals_scalar():
    rs = np.random.RandomState(11)
    c = rs.randint(0, 2 ** 32, size=(4, 500), dtype=np.uint64)
    k = rs.randint(0, 2 ** 32, size=(2, 500), dtype=np.uint64)
    got = np.stack(ns.philox4x32(*c, *k))
    for j in range(500):
        assert tuple(int(x) for x in got[:, j]) == philox_scalar(tuple(int(x) for x in c[:, j]),
                                                                 tuple(int(x) for x in k[:, j]))
    seeds = [0, 5, (1 << 32) | 5, 2 ** 64 - 1, 0x0123456789ABCDEF]
    steps = [0, 1, 2, 3, 2 ** 32 + 3, 2 ** 63 + 7]
    for seed in seeds:
        for step in steps:
            for stream in (0, 1):
                d = ns.draws(seed, step, 5, 16, stream)
                for b in range(5):
                    for a in (0, 7, 15):
                        assert d[b, a] == normal_scalar(seed, step, b * 16 + a, stream), (seed, step, stream, b, a)


def test_uniform_float32_rounding_edges():
    words = np.array([0x00000000, 0x000000FF, 0x7FFFFF00, 0x80000000, 0x80000100, 0x80000200, 0x80000300,
                      0xFFFFFE00, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], np.uint32)
    u = ns.uniform_f32(words)
    assert u.dtype == np.float32
    for w, got in zip(words, u):
        assert float(got) == uniform_exact(int(w)), hex(int(w))
    # the low byte is dropped; the smallest uniform is 2^-25, never 0
    assert u[0] == u[1] == np.float32(2.0 ** -25)
    # below 2^23 the +0.5 is exact: (2^23 - 1 + 0.5) 2^-24
    assert float(u[2]) == (2 ** 23 - 0.5) / 2 ** 24
    # from 2^23 on it is a tie, rounded to even: 2^23 -> 2^23, 2^23 + 1 -> 2^23 + 2, 2^23 + 2 -> 2^23 + 2, 2^23 + 3 -> 2^23 + 4
    assert [float(x) * 2 ** 24 for x in u[3:7]] == [2 ** 23, 2 ** 23 + 2, 2 ** 23 + 2, 2 ** 23 + 4]
    # 2^24 - 2 stays, 2^24 - 1 rounds up to 2^24: u = 1 exactly
    assert float(u[7]) * 2 ** 24 == 2 ** 24 - 2 and float(u[8]) * 2 ** 24 == 2 ** 24 - 2
    assert u[9] == u[10] == np.float32(1.0)


def test_draw_edges():
    # u1 = 1 (first word >> 8 = 2^24 - 1): the draw is exactly 0 whatever the angle
    for w1 in (0, 0x40000000, 0x80000000, M32):
        assert ns.normal_from_words(np.uint32(0xFFFFFF00), np.uint32(w1)) == 0.0
        assert ns.normal_from_words(np.uint32(M32), np.uint32(w1)) == 0.0
    # u1 = 2^-25, the largest radius: sqrt(50 ln 2), times cos of the smallest angle
    r = ns.normal_from_words(np.uint32(0), np.uint32(0))
    theta = float(np.float32(ns.TWO_PI_F32 * np.float32(2.0 ** -25)))
    assert r == math.sqrt(50.0 * math.log(2.0)) * math.cos(theta)
    assert 0 < ns.EPS_MAX - r < 1e-12
    # u2 from the second word, not the first: the same first word with two angles gives two draws
    assert ns.normal_from_words(np.uint32(0x12345678), np.uint32(0)) != ns.normal_from_words(np.uint32(0x12345678),
                                                                                              np.uint32(0x80000000))
    # angle: float32(6.2831855f * u2) -- u2 = 1/2 gives float32 pi, u2 = 1 gives 6.2831855f
    r0 = math.sqrt(50.0 * math.log(2.0))
    half = float(np.float32(ns.TWO_PI_F32 * np.float32((2 ** 23 - 0.5) / 2 ** 24)))
    assert ns.normal_from_words(np.uint32(0), np.uint32(0x7FFFFFFF)) == r0 * math.cos(half)
    assert ns.normal_from_words(np.uint32(0), np.uint32(M32)) == r0 * math.cos(float(ns.TWO_PI_F32))


def _sample():
    """2^20 draws: 8 seeds (two differ only in their high word) x 4 steps (one above 2^32) x 1024 rows x 16 actions x
    2 streams."""
    seeds = [0, 1, 5, (1 << 32) | 5, 77, 123, 2 ** 64 - 1, 0x9E3779B97F4A7C15]
    steps = [0, 1, 1000, 2 ** 32 + 3]
    out = [ns.draws(s, t, 1024, 16, stream) for s in seeds for t in steps for stream in (0, 1)]
    return np.stack(out)


def test_stream_is_standard_normal():
    from scipy import stats
    x = _sample().ravel()
    n = x.size
    assert n == 2 ** 20
    assert np.all(np.isfinite(x)) and np.max(np.abs(x)) <= ns.EPS_MAX
    d, p = stats.kstest(x, "norm")
    # fixed sample; the 1 % critical value of the one-sample KS statistic is 1.628 / sqrt(n)
    assert d <= 1.628 / math.sqrt(n), (d, p)
    assert abs(np.mean(x)) <= 5 / math.sqrt(n) and abs(np.var(x) - 1) <= 5 * math.sqrt(2 / n)


def _corr(a, b):
    a, b = np.ravel(a), np.ravel(b)
    a, b = a - a.mean(), b - b.mean()
    return float(np.dot(a, b) / math.sqrt(np.dot(a, a) * np.dot(b, b)))


def test_neighbouring_counters_are_uncorrelated():
    B, A = 4096, 16
    n = B * A
    bound = 5 / math.sqrt(n)
    for seed, step in ((5, 0), (123, 7), (0xDEADBEEF, 2 ** 32 + 3)):
        s0, s1 = ns.draws(seed, step, B, A, 0), ns.draws(seed, step, B, A, 1)
        assert abs(_corr(s0, s1)) < bound                                     # eps1 vs eps2 of one step
        assert abs(_corr(s0, ns.draws(seed, step + 1, B, A, 0))) < bound      # neighbouring steps
        assert abs(_corr(s0[:-1], s0[1:])) < 5 / math.sqrt(n - A)              # neighbouring rows (idx vs idx + 16)
        assert abs(_corr(s0[:, :-1], s0[:, 1:])) < 5 / math.sqrt(n - B)        # neighbouring actions
        hi = ns.draws(seed ^ (1 << 32), step, B, A, 0)                          # seeds differing in their high word only
        assert abs(_corr(s0, hi)) < bound
        st_hi = ns.draws(seed, step ^ (1 << 32), B, A, 0)                       # steps differing in their high word only
        assert abs(_corr(s0, st_hi)) < bound
        for other in (s1, hi, st_hi):                                          # and none is the same draw
            assert np.mean(s0 == other) < 1e-3
