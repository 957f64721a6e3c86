"""The exact general-nu Matern reference (tests/matern_exact.py) against mpmath, and the oracle's correlation against it.
CPU only: these pin the yardstick the GPU tests of test_gpu_matern_nu.py measure the device's quadrature with."""
import math

import mpmath as mp
import numpy as np
import pytest

from oracle import gpet_oracle as orc
from tests import matern_exact as me

NUS = [0.01, 0.03, 0.06, 0.1, 0.3, 0.7, 1.2, 2.0, 3.5, 7.5, 20.0, 50.0, 99.0, 101.0, 170.0, 171.0, 171.5, 172.0, 500.0,
       1000.0]
RS = [me.EPS, 1e-8, 1e-3, 0.05, 0.3, 1.0, 3.0, 10.0, 30.0]


def _mp_rho_here(nu, r, deriv=False):
    """(at the working precision of the caller)"""
    nu, r = mp.mpf(nu), mp.mpf(r)
    x = mp.sqrt(2 * nu) * r
    c = mp.power(2, 1 - nu) / mp.gamma(nu)
    if deriv:
        return c * x ** (nu + 1) * mp.besselk(nu - 1, x)
    return c * x ** nu * mp.besselk(nu, x)


def _mp_rho(nu, r, deriv=False):
    with mp.workdps(30):
        return _mp_rho_here(nu, r, deriv)


def _close(got, want, what):
    want = float(want)
    assert abs(got - want) <= 1e-14 + 1e-12 * abs(want), "%s: %r vs %r" % (what, got, want)


def test_helper_rho_and_derivative_match_mpmath():
    """180 points (nu from 0.01 to 1000, r from eps to where rho underflows): both branches of the helper (closed form
    with scipy's kve; ratio of mixture sums) to 1e-14 absolute + 1e-12 relative of 30-digit values."""
    for nu in NUS:
        got = me.rho(nu, np.array(RS))
        dgot = me.drho_dlogl(nu, np.array(RS))
        for i, r in enumerate(RS):
            _close(got[i], _mp_rho(nu, r), "rho(nu=%g, r=%g)" % (nu, r))
            _close(dgot[i], _mp_rho(nu, r, True), "drho(nu=%g, r=%g)" % (nu, r))
    assert me.rho(3.5, 0.0) == 1.0 and me.drho_dlogl(3.5, 0.0) == 0.0


@pytest.mark.parametrize("nu,r", [(0.06, 0.3), (0.7, 1e-3), (1.2, 1.0), (3.5, 0.3), (20.0, 1.0), (172.0, 0.3),
                                  (1000.0, 0.05)])
def test_helper_derivative_is_the_derivative_of_rho(nu, r):
    """The closed form c x^(nu+1) K_(nu-1)(x) is d rho / d log(l) (r = d / l): against mpmath's numerical derivative."""
    with mp.workdps(30):
        want = mp.diff(lambda t: _mp_rho_here(nu, mp.mpf(r) * mp.exp(-t)), 0)
    _close(float(me.drho_dlogl(nu, r)), want, "d/dlog l at nu=%g r=%g" % (nu, r))


@pytest.mark.parametrize("nu", [0.03, 0.06, 0.3, 0.7, 1.2, 2.0, 3.5, 7.5, 12.0])
def test_oracle_corr_matrix_matches_helper(nu):
    """gpet_oracle.corr_matrix (sklearn's formula: eps added to zero distances) against the helper's sklearn convention,
    cross-kernel with duplicated and shared inputs, to 1e-13 wherever sklearn's formula is finite."""
    rng = np.random.default_rng(int(nu * 100))
    xa = np.concatenate([np.sort(rng.uniform(-2.0, 2.0, 40)), [0.5, 0.5, 0.0]])
    xb = np.concatenate([xa[::3], rng.uniform(-3.0, 3.0, 10)])
    for ell in (0.1, 0.8, 7.0):
        R = orc.corr_matrix("Matern", nu, xa, xb, ell)
        E, _ = me.sklearn_convention(nu, xa, xb, ell, False)
        fin = np.isfinite(R)
        assert fin.mean() > 0.9
        np.testing.assert_allclose(R[fin], E[fin], rtol=0, atol=1e-13)
    # the parity gap the device closes: rho(eps) is visibly below 1 for small nu
    if nu <= 0.3:
        assert orc.corr_matrix("Matern", nu, [1.0], [1.0], 1.0)[0, 0] < 1.0 - 1e-10


@pytest.mark.parametrize("nu", [20.0, 50.0, 100.0, 172.0, 500.0])
def test_oracle_is_not_finite_at_zero_distance_for_large_nu(nu):
    """sklearn's formula overflows at zero distance from nu ~ 20 on (inf, then NaN): the reason whole traces at such nu
    are checked against the helper's posterior instead of the oracle (test_gpu_matern_nu.py)."""
    with np.errstate(all="ignore"):
        R = orc.corr_matrix("Matern", nu, [0.0, 0.0], [0.0], 1.0)
    assert not np.all(np.isfinite(R))
    assert me.rho(nu, me.EPS) == pytest.approx(1.0, abs=1e-14)


@pytest.mark.parametrize("nu", [0.06, 0.7, 5.0, 172.0])
def test_helper_lml_gradient_is_the_gradient_of_its_objective(nu):
    """The helper's log marginal likelihood gradient against a central difference of its own objective (duplicated
    inputs included: their zero distance is evaluated at eps whatever l is, so the convention's zero gradient is exact)."""
    rng = np.random.default_rng(3)
    xs = np.sort(np.concatenate([rng.uniform(-1.5, 1.5, 14), [0.25, 0.25]]))
    ys = np.sin(3 * xs) + 0.1 * rng.normal(size=xs.size)
    w = np.ones_like(xs)
    th = np.log([2.0, 0.7, 0.05])
    f0, g = me.lml_and_grad(th, xs, ys, w, nu)
    assert np.isfinite(f0)
    h = 1e-5
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        fd = (me.lml_and_grad(th + e, xs, ys, w, nu)[0] - me.lml_and_grad(th - e, xs, ys, w, nu)[0]) / (2 * h)
        assert math.isclose(g[k], fd, rel_tol=1e-6, abs_tol=1e-6), (k, g[k], fd)
