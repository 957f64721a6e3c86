"""Extended-precision restatement of the reference's curve cost (gpet.py:391-408 with scipy >= 1.11 ``simpson``) in plain
loops, and the curves the scorer tests feed to it (tests/test_curve_cost_exact.py on the host, tests/test_gpu_score_injected.py
on the device).  Nothing here comes from the oracle or from the kernels.

A curve is one row y[0..Lg-1] over the image columns x_st .. x_st + Lg - 1.  The integrals run over the SAMPLES 0 .. Lg-2:

    g[k]    = grad(clamp(y[k], 0, M-1), x_st + k) + 1e-3     linear between the two rows of the float32 image
    ell[k]  = sqrt(1 + (y[k+1] - y[k])^2)                     segment k -> k+1
    arc     = simpson(ell[0..Lg-2], unit spacing)
    line    = simpson(g[0..Lg-2], spacing between samples k and k+1 = ell[k+1])
    cost    = arc / line

The spacing ell[k+1] -- the NEXT segment's length -- is the reference's: it integrates over ``cumsum(ell)``, whose differences
start at the second segment.  The kernels reproduce it.  ``simpson`` is the composite rule with the weights for irregular
spacing; an even number of samples (odd Lg) takes the rule over all but the last sample and adds Cartwright's term for the last
interval, each integral with its own spacings.

The arithmetic is np.longdouble where that has a 64-bit mantissa, else ``decimal`` at 40 digits.  Besides the cost a condition
number is returned: max over the two integrals of sum |term| / |sum term|, the factor by which the roundings of the terms of a
float64 evaluation are amplified in its result."""
import decimal
import functools
import math

import numpy as np

LD = np.longdouble
USE_DECIMAL = float(np.finfo(LD).eps) > 2e-19
_CTX = decimal.Context(prec=40)


def _num(v):
    """An exact copy of the float (or small integer) v in the extended format."""
    return _CTX.create_decimal(float(v)) if USE_DECIMAL else LD(v)


def _sqrt(v):
    return v.sqrt(_CTX) if USE_DECIMAL else np.sqrt(v)


def _simpson(f, h):
    """(integral, sum of the absolute terms) of the n samples f with the n - 1 spacings h."""
    n = len(f)
    m = n if n % 2 == 1 else n - 1
    tot, tabs = _num(0), _num(0)
    for i in range(0, m - 1, 2):
        h0, h1 = h[i], h[i + 1]
        hs = h0 + h1
        w = hs / 6
        t0, t1, t2 = f[i] * (2 - h1 / h0), f[i + 1] * (hs * hs / (h0 * h1)), f[i + 2] * (2 - h0 / h1)
        tot += w * (t0 + t1 + t2)
        tabs += w * (abs(t0) + abs(t1) + abs(t2))
    if n % 2 == 0:  # Cartwright's correction for the last interval
        h0, h1 = h[n - 3], h[n - 2]
        a = (2 * h1 * h1 + 3 * h0 * h1) / (6 * (h1 + h0))
        b = (h1 * h1 + 3 * h0 * h1) / (6 * h0)
        e = h1 * h1 * h1 / (6 * h0 * (h0 + h1))
        tot += a * f[n - 1] + b * f[n - 2] - e * f[n - 3]
        tabs += abs(a * f[n - 1]) + abs(b * f[n - 2]) + abs(e * f[n - 3])
    return tot, tabs


def curve_cost(grad, x_st, y):
    """(cost in the extended format, condition number as a float) of the curve y on the float32 image grad."""
    assert grad.dtype == np.float32 and grad.ndim == 2
    M = grad.shape[0]
    y = [float(v) for v in y]
    Lg = len(y)
    assert Lg >= 4 and M >= 2
    n = Lg - 1
    with decimal.localcontext(_CTX):
        ye = [_num(v) for v in y]
        one = _num(1)
        ell = [_sqrt(one + (ye[k + 1] - ye[k]) * (ye[k + 1] - ye[k])) for k in range(n)]
        g = []
        for k in range(n):
            yc = min(max(y[k], 0.0), float(M - 1))  # (exact in float64; the weights below are not)
            iy = min(int(math.floor(yc)), M - 2)
            yy = _num(yc)
            g.append(_num(grad[iy, x_st + k]) * (_num(iy + 1) - yy) + _num(grad[iy + 1, x_st + k]) * (yy - _num(iy)) + _num(1e-3))
        al, ala = _simpson(ell, [one] * (n - 1))
        li, lia = _simpson(g, ell[1:n])
        return al / li, float(max(ala / abs(al), lia / abs(li)))


def curve_costs(grad, x_st, Y):
    """curve_cost of every row of Y: (list of costs in the extended format, float64 array of condition numbers)."""
    out = [curve_cost(grad, x_st, row) for row in np.asarray(Y)]
    return [c for c, _ in out], np.array([k for _, k in out])


def rel_err(got, want):
    """|got - want| / |want| as a float, the difference taken in the extended format."""
    with decimal.localcontext(_CTX):
        return float(abs((_num(got) - want) / want))


# ---- the scorer tests' inputs --------------------------------------------------------------------------------------------------

FAMILIES = ["smooth", "const_int", "row0", "rowlast", "below", "above", "ramp", "saw", "saw3", "uniform", "ints", "near_int",
            "step_last"]

# (M, N, x_st, Lg): 19, 17, 15, 15, 16 and 16 Simpson pairs -- one pair past a tile of 15, the last pair on the tile boundary
# with and without Cartwright's term --, the shortest edges, and 65 pairs: more than the 64 of a wave's chunk
SHAPES = [(12, 40, 0, 40), (12, 40, 3, 37), (33, 80, 1, 32), (33, 80, 1, 33), (33, 80, 46, 34), (33, 80, 2, 35), (12, 40, 0, 4),
          (12, 40, 35, 5), (7, 140, 0, 133)]

# (shape, S, sample dtype).  S >= 64 takes the tiled scorer (200: two blocks of 128 curves, the second not full; 1100: nine, and
# the rank-counting top-k), S < 64 the wave-per-curve one -- whose lane 63 fetches its successor from the next chunk on the 65
# pairs of Lg = 133.
CASES = ([(sh, S, "f64") for sh in SHAPES[:2] for S in (64, 200, 1100)] + [(sh, 64, "f64") for sh in SHAPES[2:]] +
         [(SHAPES[8], 40, "f64"), (SHAPES[0], 40, "f64"), (SHAPES[3], 40, "f64")] +
         [(SHAPES[0], 200, "f32"), (SHAPES[1], 64, "f32"), (SHAPES[8], 40, "f32"), (SHAPES[0], 40, "f32")])

# one batch of three edges of different widths on one 33 x 80 image: 15, 16 and 39 pairs = 1, 2 and 3 tiles
BATCH_SPANS = [(1, 33), (46, 34), (0, 80)]  # (x_st, Lg)
BATCH_S = 64


def image(M, N, seed):
    """Random float32 in [0, 1) with about 30 % exact zeros (where the 1e-3 floor is all of g) and one 1.0."""
    rng = np.random.default_rng(seed)
    g = rng.random((M, N)).astype(np.float32)
    g[rng.random((M, N)) < 0.3] = 0
    g[M // 2, N // 2] = 1.0
    return g


def _curve(fam, M, Lg, s, rng):
    k = np.arange(Lg)
    if fam == "smooth":
        return M / 2 + 0.3 * M * np.sin(k / 7.0 + rng.uniform(0, 2 * np.pi)) + rng.uniform(-0.5, 0.5)
    if fam == "const_int":
        return np.full(Lg, float(rng.integers(1, M - 1)))
    if fam == "row0":
        return np.zeros(Lg)
    if fam == "rowlast":
        return np.full(Lg, M - 1.0)
    if fam == "below":
        return np.full(Lg, -rng.uniform(0.25, 4.0))
    if fam == "above":
        return np.full(Lg, M - 1 + rng.uniform(0.25, 4.0))
    if fam == "ramp":
        y = np.linspace(-6.0, M + 5.0, Lg)
        return y[::-1].copy() if (s // len(FAMILIES)) % 2 else y
    if fam == "saw":
        return M / 2 + rng.uniform(-0.04, 0.04) * M + np.where((k + s) % 2 == 0, -0.45 * M, 0.45 * M)
    if fam == "saw3":
        return M / 2 + rng.uniform(-0.05, 0.05) * M + np.where((k + s) % 3 == 0, -0.4 * M, 0.1 * M)
    if fam == "uniform":
        return rng.uniform(-5, M + 5, Lg)
    if fam == "ints":
        return rng.integers(0, M, Lg).astype(float)
    if fam == "near_int":
        return np.nextafter(rng.integers(1, M - 1, Lg).astype(float), np.where((k + s) % 2, np.inf, -np.inf))
    assert fam == "step_last"
    return np.r_[np.full(Lg - 1, float(rng.integers(1, M - 2)) + 0.25), M - 1.0]


COND_DRAW = 16.0  # a drawn curve is kept when its condition number on the image is at most this
REDRAWS = {}  # seed of a curves() call -> {family: draws rejected}; tests/test_curve_cost_exact.py holds them to a few


def curves(grad, x_st, Lg, S, seed):
    """S curves of Lg points on the image grad, row s of family s % 13, every row with offsets / phases / draws of its own; with
    their costs and condition numbers.
    A draw whose sums cancel -- a long segment next to a short one gives Simpson weights of both signs, and where the image is 0
    beside 1 the terms then nearly cancel -- is drawn again: the scorer test's tolerance is proportional to the condition
    number, and at a condition number of hundreds it would pin nothing.  The bound of the tests is 32; the margin is for the
    float32 rounding of the samples, which moves the condition number a little.  The rejected draws are counted per family in
    REDRAWS[seed]."""
    M = grad.shape[0]
    rng = np.random.default_rng(seed)
    Y, costs, cond = np.empty((S, Lg)), [], []
    rejected = REDRAWS[seed] = {}
    for s in range(S):
        fam = FAMILIES[s % len(FAMILIES)]
        for _ in range(50):
            Y[s] = _curve(fam, M, Lg, s, rng)
            c, k = curve_cost(grad, x_st, Y[s])
            if k <= COND_DRAW:
                break
            rejected[fam] = rejected.get(fam, 0) + 1
        else:
            raise AssertionError("no well-conditioned draw for row %d" % s)
        costs.append(c)
        cond.append(k)
    return Y, costs, np.array(cond)


@functools.lru_cache(maxsize=None)
def case_reference(shape, S, dt):
    """(image, samples as the device holds them, their costs in the extended format, their condition numbers) of a case, seeded
    by the shape and S alone.  Computed once per process; nobody may write to the arrays."""
    M, N, x_st, Lg = shape
    grad = image(M, N, 1000 * M + Lg)
    Y, costs, cond = curves(grad, x_st, Lg, S, 100000 * x_st + 100 * Lg + S)
    if dt == "f32":
        Y = Y.astype(np.float32).astype(np.float64)
        costs, cond = curve_costs(grad, x_st, Y)
    for a in (grad, Y, cond):
        a.setflags(write=False)
    return grad, Y, costs, cond


@functools.lru_cache(maxsize=None)
def batch_reference():
    """(image, [(samples, costs, condition numbers) of every edge of BATCH_SPANS])."""
    grad = image(33, 80, 7)
    grad.setflags(write=False)
    return grad, [curves(grad, x_st, Lg, BATCH_S, 31 * Lg + x_st) for x_st, Lg in BATCH_SPANS]
