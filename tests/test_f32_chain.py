"""tests/f32_chain.py (the yardstick of sample_dtype="f32mma") against the C library's fmaf."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from tests.f32_chain import chain, fmaf


@pytest.fixture(scope="module")
def libm_fmaf():
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.fmaf.restype = ctypes.c_float
    lib.fmaf.argtypes = [ctypes.c_float] * 3
    return lambda a, b, c: np.array([lib.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)


def naive(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def test_fmaf_equals_libm_on_random_triples(libm_fmaf):
    """10^5 triples: a, b, c with independent binary exponents; c near a * b in magnitude (cancellation, rounding of the sum);
    c a few binades above (the product only decides the rounding); and results in the subnormal range of float32."""
    rng = np.random.default_rng(5)
    n = 25000
    sets = []
    m = lambda: (rng.uniform(1, 2, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    e = lambda lo, hi: np.exp2(rng.integers(lo, hi + 1, n)).astype(np.float32)
    sets.append((m() * e(-20, 20), m() * e(-20, 20), m() * e(-40, 40)))
    a, b = m() * e(-8, 8), m() * e(-8, 8)
    sets.append((a, b, (-(a * b) * (1 + rng.integers(-4, 5, n) * np.float32(2.0 ** -23))).astype(np.float32)))
    a, b = m(), m()
    sets.append((a, b, (m() * e(20, 26))))
    sets.append((m() * e(-70, -60), m() * e(-70, -60), m() * e(-140, -126)))
    for a, b, c in sets:
        want = libm_fmaf(a, b, c)
        got = fmaf(a, b, c)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)[:5]


def test_fmaf_on_double_rounding_cases(libm_fmaf):
    """a * b + c whose float64 sum is exactly halfway between two floats while the true sum is not: the form that rounds
    twice goes to the even neighbour, fmaf to the side of the true sum.  a = +-(1 + 2^-23), b = 1 - 2^-23 (a * b = +-(1 - 2^-46)),
    c = 2^24 + 2: fmaf gives 16 777 218 both times, the naive form 16 777 220 and 16 777 216.  The family: c = 2^24 + 2 m with m odd
    (c is then the ODD neighbour of the halfway point c +- 1, so ties-to-even always leaves it), m = 1, 3 and more, c negated, and
    the same bits in two other binades."""
    f = np.float32
    a, b, c = [], [], []
    for sa in (1, -1):
        for c0 in [2.0 ** 24 + 2, 2.0 ** 24 + 6] + [2.0 ** 24 + 2 * i for i in range(9, 200, 14)]:
            for sc in (1, -1):
                for scale in (1.0, 2.0 ** -30, 2.0 ** 40):  # (the same bits in other binades: a scaled, c scaled)
                    a.append(sa * (1 + 2.0 ** -23) * scale)
                    b.append(1 - 2.0 ** -23)
                    c.append(sc * c0 * scale)
    a, b, c = np.array(a, dtype=f), np.array(b, dtype=f), np.array(c, dtype=f)
    want = libm_fmaf(a, b, c)
    assert fmaf(f(1 + 2.0 ** -23), f(1 - 2.0 ** -23), f(2.0 ** 24 + 2)) == 16777218.0
    assert fmaf(f(-(1 + 2.0 ** -23)), f(1 - 2.0 ** -23), f(2.0 ** 24 + 2)) == 16777218.0
    assert naive(a[:1], b[:1], c[:1])[0] == 16777220.0
    assert np.array_equal(fmaf(a, b, c).view(np.uint32), want.view(np.uint32))
    # the cases are real: the twice-rounded form misses every one of them
    assert (naive(a, b, c) != want).all()


def test_chain_is_the_ordered_fmaf_chain(libm_fmaf):
    rng = np.random.default_rng(9)
    Z, A = rng.standard_normal((5, 37)), 0.3 * rng.standard_normal((37, 6))
    got = chain(Z, A)
    Zf, Af = Z.astype(np.float32), A.astype(np.float32)
    for s in range(5):
        for j in range(6):
            acc = np.zeros(1, dtype=np.float32)
            for k in range(37):
                acc = libm_fmaf(Zf[s, k:k + 1], Af[k:k + 1, j], acc)
            assert got[s, j] == acc[0]
    assert np.mean(chain(Z, A, order=range(36, -1, -1)) != got) > 0.25
