"""Float64 reference of the general-nu Matern kernel (sklearn kernels.py Matern, any nu > 0) and of the GP quantities
built from it, for the tests of the device's quadrature (csrc/gpet_k_common.inc, matern_gen).

    rho(r)            = 2^(1-nu) / Gamma(nu) x^nu K_nu(x),          x = sqrt(2 nu) r
    d rho / d log(l)  = 2^(1-nu) / Gamma(nu) x^(nu+1) K_(nu-1)(x)   (closed form; r = d / l)

Where scipy's scaled Bessel function ``kve`` and the prefactor stay well scaled (nu <= 100, x not so small that
x^nu K_nu(x) overflows) the closed forms are evaluated directly.  Elsewhere (large nu, or tiny x at moderate nu) both come from the
Gamma-mixture form  rho = int exp(nu s - e^s - q e^-s) ds / int exp(nu s - e^s) ds,  q = nu r^2 / 2, as a RATIO of two
fine trapezoid sums on the same nodes: the normalisation Gamma(nu) and the shift that keeps the exponents finite cancel,
so nothing overflows and the only rounding is that of the node weights.  mpmath (30 digits) pins both branches in
test_matern_exact.py; it is too slow to be used at test time.

``sklearn_convention`` gives what sklearn (and the oracle, gpet_oracle.corr_matrix) evaluates for a matrix of inputs:
a self-kernel's diagonal is exactly 1, and any other zero distance is evaluated at r = eps with zero gradient.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.linalg
import scipy.special

EPS = float(np.finfo(float).eps)


def _closed_form(nu, r, deriv):
    x = math.sqrt(2.0 * nu) * r
    c = 2.0 ** (1.0 - nu) / scipy.special.gamma(nu)
    with np.errstate(all="ignore"):
        if deriv:
            out = c * x ** (nu + 1.0) * scipy.special.kve(nu - 1.0, x) * np.exp(-x)
        else:
            out = c * x ** nu * scipy.special.kve(nu, x) * np.exp(-x)
    return out


def _mixture(nu, r, deriv):
    """Ratio-of-trapezoid-sums form for the points r (1-D, r > 0)."""
    q = 0.5 * nu * r * r
    h = min(0.1, 0.25 / math.sqrt(nu))
    s_lo = math.log(nu) - 1.0 - 46.0 / nu
    s_hi = math.log(2.0 * nu + 2.0 * math.sqrt(float(q.max(initial=0.0))) + 100.0) + 1.0
    s = np.arange(math.floor(s_lo / h), math.ceil(s_hi / h) + 1) * h
    es = np.exp(s)
    lw = nu * s - es
    w = np.exp(lw - lw.max())
    out = np.empty_like(q)
    for i in range(0, q.size, 2048):
        with np.errstate(over="ignore"):
            e = np.exp(-np.outer(q[i:i + 2048], 1.0 / es))  # [points, nodes]
        out[i:i + 2048] = 2.0 * q[i:i + 2048] * (e @ (w / es)) if deriv else e @ w
    return out / w.sum()


def _eval(nu, r, deriv):
    nu = float(nu)
    r = np.abs(np.asarray(r, dtype=np.float64))
    flat, back = np.unique(r.reshape(-1), return_inverse=True)
    out = np.empty_like(flat)
    zero = flat == 0.0
    out[zero] = 0.0 if deriv else 1.0
    pos = ~zero
    if nu <= 100.0:
        v = _closed_form(nu, flat[pos], deriv)
        # neither kve nor the product overflowed, and the power did not underflow
        with np.errstate(all="ignore"):
            xp = (math.sqrt(2.0 * nu) * flat[pos]) ** nu
        ok = np.isfinite(v) & (xp > 1e-290)
        tmp = out[pos]
        tmp[ok] = v[ok]
        todo = np.flatnonzero(~ok)
        if todo.size:
            tmp[todo] = _mixture(nu, flat[pos][todo], deriv)
        out[pos] = tmp
    elif pos.any():
        out[pos] = _mixture(nu, flat[pos], deriv)
    return out[back].reshape(r.shape)


def rho(nu, r):
    """Matern correlation at scaled distance r (any shape; rho(0) = 1)."""
    return _eval(nu, r, False)


def drho_dlogl(nu, r):
    """d rho / d log(length_scale) at scaled distance r = d / l (closed form, no numerical differentiation)."""
    return _eval(nu, r, True)


def sklearn_convention(nu, xa, xb, length_scale, self_kernel):
    """(rho, d rho / d log l) matrices for 1-D inputs, as sklearn evaluates them: inputs divided by l, distances
    |a_i - b_j|; a self-kernel's diagonal is 1 with zero gradient; any other zero distance is evaluated at eps with
    zero gradient (sklearn adds eps to exact zeros, and its forward difference of two equal values is 0)."""
    a = np.asarray(xa, dtype=np.float64) / length_scale
    b = np.asarray(xb, dtype=np.float64) / length_scale
    d = np.abs(a[:, None] - b[None, :])
    zero = d == 0.0
    R = rho(nu, np.where(zero, EPS, d))
    G = np.where(zero, 0.0, drho_dlogl(nu, np.where(zero, 1.0, d)))
    if self_kernel:
        np.fill_diagonal(R, 1.0)
        np.fill_diagonal(G, 0.0)
    return R, G


def lml_and_grad(theta, xs, ys, w, nu, jitter=1e-6):
    """log marginal likelihood and its gradient wrt theta = log(c, l, noise) (sklearn_gpr.py:512-585, the formulas of
    gpet_oracle.lml_and_grad) with the exact correlation and derivative.  (-inf, 0) when K is not positive definite."""
    c, ell, nl = np.exp(theta)
    R, dR = sklearn_convention(nu, xs, xs, ell, True)
    n = xs.shape[0]
    K = c * R + np.diag(nl * w)
    K[np.diag_indices(n)] += jitter
    try:
        L = scipy.linalg.cholesky(K, lower=True, check_finite=False)
    except np.linalg.LinAlgError:
        return -np.inf, np.zeros(3)
    alpha = scipy.linalg.cho_solve((L, True), ys, check_finite=False)
    lml = -0.5 * ys @ alpha - np.log(np.diag(L)).sum() - n / 2 * np.log(2 * np.pi)
    Kinv = scipy.linalg.cho_solve((L, True), np.eye(n), check_finite=False)
    inner = np.outer(alpha, alpha) - Kinv
    g = np.array([0.5 * np.einsum("ij,ji->", inner, Gk) for Gk in (c * R, c * dR, np.diag(nl * w))])
    return lml, g


def posterior(x, y, noise, amp, length_scale, nu, xq, jitter=1e-6, y_mean=0.0, y_std=1.0):
    """GaussianProcessRegressor.fit + predict (sklearn_gpr.py:221-234, 381-436) for training inputs x, targets y
    (already centred / scaled by the caller's convention), per-point noise variances ``noise`` (added to the
    diagonal with the jitter): K, L, mean, std and covariance at xq, the outputs rescaled by y_std / y_mean."""
    x = np.asarray(x, dtype=np.float64)
    xq = np.asarray(xq, dtype=np.float64)
    K = amp * sklearn_convention(nu, x, x, length_scale, True)[0]
    K[np.diag_indices(x.shape[0])] += np.asarray(noise, dtype=np.float64)
    K[np.diag_indices(x.shape[0])] += jitter
    L = scipy.linalg.cholesky(K, lower=True, check_finite=False)
    alpha = scipy.linalg.cho_solve((L, True), y, check_finite=False)
    Kt = amp * sklearn_convention(nu, xq, x, length_scale, False)[0]
    mean = y_std * (Kt @ alpha) + y_mean
    V = scipy.linalg.solve_triangular(L, Kt.T, lower=True, check_finite=False)
    var = amp - np.einsum("ij,ij->j", V, V)
    var[var < 0] = 0.0
    Kss = amp * sklearn_convention(nu, xq, xq, length_scale, True)[0]
    cov = (Kss - V.T @ V) * y_std ** 2
    return dict(K=K, L=L, alpha=alpha, mean=mean, std=np.sqrt(var * y_std ** 2), cov=cov)
