"""Extended-precision restatement of the posterior of a training set -- K, its Cholesky factor, alpha, mean, variance and
covariance on a grid -- with the componentwise rounding bounds a float64 evaluation of it has to meet, and the table of training
sets the posterior tests use (tests/test_posterior_exact.py on the host, tests/test_gpu_posterior_injected.py on the device).
Nothing here comes from the oracle or from the kernels.

The arithmetic is np.longdouble where that has a 64-bit mantissa, else ``decimal`` at 40 digits (arrays of Decimal objects: slow,
the same statements).

Two forms reach the same core (``posterior``):

* LOOP form (k_fit<., false>, gpet.py:209-231, sklearn_gpr.py:221-227): ``loop_prelude`` is y_s = std(y) + 1, v = y / y_s,
  y_mean = mean(v), y_std = std(v) (1 when 0), y_train = v - y_mean (centred ONLY: y_std still multiplies mean, std and cov),
  amp = sigma_f^2 / y_s^2; the weights are 1e-7 (fix_endpoints) or 0.5 on the init points and 1 elsewhere; the noise is left
  out of K when n == Lg.  The grid is the pixel columns.
* CONVERGED-FIT form (k_fit<., true>, gpet.py:232-266): training values, weights and par[0..8] = (amp, length scale, noise
  level, X_m, X_s, y_m, y_s, y_mean, y_std) are taken as given; the grid is (x - par[3]) / par[4]; the mean leaves as
  par[6] * mean + par[5]; the std is not rescaled (``final_posterior``).

Staging.  The prelude's five results are float64 numbers an implementation holds (the device: GPET_BUF_Y_TRAIN and the
scalars), each with a bound of its own below.  The core is then evaluated on the float64 values the implementation under test
HOLDS -- not on the exact ones -- so that its bounds are those of the core's own arithmetic, as for the converged form whose
inputs are given.  An error cannot hide between the two: the prelude's values are checked first, against the exact prelude.

Bounds.  u = 2^-53; every + - * / sqrt of the implementation is taken as correctly rounded (1 u), ``exp`` as within one ulp
(2 u).  M = |L||L^T|, z_j = K^-1 k_j, E = the rounding of the kernel-function values (below).  With n training points:

  factor (backward)   |L_dev L_dev^T - K|_ij <= (n + 1) u sqrt(K_ii K_jj) + E_ij           (Higham, Accuracy and Stability, Thm 10.3)
  alpha (forward)     |K^-1| (3 n u M + E) |alpha|                                        (Thm 10.4: (K + dK) a = y, |dK| <= 3 n u M)
  mean                y_std (|k_j|^T b_alpha + n u |k_j|^T |alpha| + E_j^T |alpha|) + u (|y_std k_j^T alpha| + |mean_j|)
  var, cov            y_std^2 (3 n u |z_j|^T M |z_j'| + |z_j|^T E_j' + E_j^T |z_j'| + E**_jj' + 4 u amp)
  std                 compared as std^2 against the clamped var, with 3 u std^2 more (product, sqrt); where the exact var is
                      below its own bound, std <= sqrt(2 bound)

Any summation order meets them (a sum of n products errs by at most n u sum |terms|, Higham 3.1), so the 4-wide chunks of the
matrix cores do.  3 n u M carries the forward substitution V = L^-1 k_j (its rows solve (L + dL) v = k with |dL| <= n u |L|,
Thm 8.5, hence v^T v = k^T (K + dK)^-1 k with |dK| <= 3 n u M to first order) and the n-term sum of squares.  E stands beside
3 n u M in alpha's bound because alpha solves the system of the ROUNDED K; it matters for n of a few.  A product with the explicit
inverse of a diagonal block in place of a substitution is NOT covered: its error grows with the block's condition number
(k_vsolve_mfma had that form and missed b_cov by a factor 2.6 on the ill-conditioned sets of ``jitter_only_case``).

The rounding of one kernel-function value, c_k, is not one constant: the argument's rounding is amplified by the argument
(``kernel_ulps``, derived there from the formula the kernels evaluate, corr_fn in csrc/gpet_k_common.inc).  E = c_k u |value|
per entry; on K's diagonal amp + noise * w + jitter is one product and two sums: 3 u.
"""
import decimal
import functools
import math

import numpy as np

LD = np.longdouble
USE_DECIMAL = float(np.finfo(LD).eps) > 2e-19
_CTX = decimal.Context(prec=40)
U = 2.0 ** -53
KERNELS = {"RBF": ("RBF", 2.5), "M25": ("Matern", 2.5), "M15": ("Matern", 1.5), "M05": ("Matern", 0.5)}


# ---- the extended format ---------------------------------------------------------------------------------------------------------

def _in_context(f):
    @functools.wraps(f)
    def g(*a, **k):
        with decimal.localcontext(_CTX):
            return f(*a, **k)
    return g


def ext(a, use_decimal=None):
    """An exact copy of the float64 array (or number) a in the extended format."""
    if USE_DECIMAL if use_decimal is None else use_decimal:
        a = np.asarray(a, dtype=np.float64)
        out = np.empty(a.shape, dtype=object)
        for idx in np.ndindex(a.shape):
            out[idx] = _CTX.create_decimal(float(a[idx]))
        return out if out.ndim else out[()]
    return np.asarray(a, dtype=LD) if np.ndim(a) else LD(a)


def f64(a):
    """The extended array a rounded to float64."""
    return np.asarray(a, dtype=object).astype(np.float64) if np.asarray(a).dtype == object else np.asarray(a, dtype=np.float64)


def _is_dec(a):
    return np.asarray(a).dtype == object


_dexp = np.frompyfunc(lambda v: v.exp(_CTX), 1, 1)
_dsqrt = np.frompyfunc(lambda v: v.sqrt(_CTX), 1, 1)


def _exp(a):
    return _dexp(a) if _is_dec(a) else np.exp(a)


def _sqrt(a):
    return _dsqrt(a) if _is_dec(a) else np.sqrt(a)


def _zeros(shape, like):
    if _is_dec(like):
        out = np.empty(shape, dtype=object)
        out.fill(decimal.Decimal(0))
        return out
    return np.zeros(shape, dtype=LD)


def _dot(a, b):
    """a @ b; a product with an empty inner dimension is the zero of the format."""
    if a.shape[-1] == 0:
        return _zeros(a.shape[:-1] + b.shape[1:], a)
    return a @ b


def chol(K):
    """Lower Cholesky factor, row by row; raises ValueError where a pivot is not positive."""
    n = K.shape[0]
    L = _zeros((n, n), K)
    for j in range(n):
        d = K[j, j] - _dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise ValueError("pivot %d is not positive" % j)
        L[j, j] = _sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - _dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    return L


def fsub(L, B):
    """L^-1 B."""
    X = _zeros(B.shape, B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - _dot(L[i, :i], X[:i])) / L[i, i]
    return X


def bsub(L, B):
    """L^-T B."""
    n = L.shape[0]
    X = _zeros(B.shape, B)
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - _dot(L[i + 1:, i], X[i + 1:])) / L[i, i]
    return X


# ---- the kernel function -----------------------------------------------------------------------------------------------------

def corr(kernel, a, b):
    """rho(|a_i - b_j|) of the pre-scaled inputs a, b (extended vectors): RBF, or Matern nu in {0.5, 1.5, 2.5} in closed form."""
    name, nu = KERNELS[kernel]
    d = a[:, None] - b[None, :]
    if name == "RBF":
        return _exp(-(d * d) / 2)
    r = abs(d)
    if nu == 0.5:
        return _exp(-r)
    k = r * _sqrt(ext(3.0 if nu == 1.5 else 5.0, _is_dec(a)))
    if nu == 1.5:
        return (1 + k) * _exp(-k)
    return (1 + k + k * k / 3) * _exp(-k)


def kernel_ulps(kernel, a, b, ra=1, rb=1):
    """c_k per entry, in units of u: |amp * rho_float64 - amp * rho| <= c_k u amp rho for the float64 evaluation

        d = a_i - b_j;  RBF: exp(-0.5 * (d * d));  Matern: r = sqrt(d * d), k = r * sqrt(nu')  [0.5: exp(-r)],
        1.5: (1 + k) * exp(-k);  2.5: (1 + k + k * k / 3) * exp(-k);  then amp * rho

    of float64 inputs a, b that carry ra, rb roundings themselves (x / l: one division; the converged fit's grid
    ((x - X_m) / X_s) / l: three).  With A = ra |a| + rb |b|, everything in units of u:
      d      absolute error A + |d|                      (the inputs' roundings are NOT relative to d: they cancel)
      RBF    t = 0.5 d^2: |d| (A + |d|) + t  (the square; the half is exact), exp amplifies an absolute error of its argument
             one to one and adds 2, the product with amp 1:                       c = |d| (A + |d|) + t + 3
      r      A + |d| + 1.5 r = A + 2.5 r             (the square's rounding halves under the root, the root adds 1)
      0.5    exp(-r), amp:                                                         c = A + 2.5 r + 3
      k      D = s (A + 2.5 r) + 2 k,  s = sqrt(3) or sqrt(5)  (the rounded constant and the product)
      1.5    1 + k: relative D / (1 + k) + 1; exp: D + 2; two products:            c = D (1 + 1 / (1 + k)) + 5
      2.5    p = 1 + k + k^2 / 3: the derivative 1 + 2 k / 3 carries D, the square, the division and two sums at most 4
             relative (all terms positive); exp: D + 2; two products:              c = D (1 + (1 + 2 k / 3) / p) + 8
    Equal float64 inputs give d = 0 and rho = 1 exactly in float64; the exact rho of their unrounded values is 1 - O(A^2 u^2)."""
    name, nu = KERNELS[kernel]
    a = np.asarray(a, dtype=np.float64)[:, None]
    b = np.asarray(b, dtype=np.float64)[None, :]
    A = ra * np.abs(a) + rb * np.abs(b)
    d = np.abs(a - b)
    if name == "RBF":
        return d * (A + d) + 0.5 * d * d + 3
    if nu == 0.5:
        return A + 2.5 * d + 3
    s = math.sqrt(3.0 if nu == 1.5 else 5.0)
    k = s * d
    D = s * (A + 2.5 * d) + 2 * k
    if nu == 1.5:
        return D * (1 + 1 / (1 + k)) + 5
    return D * (1 + (1 + 2 * k / 3) / (1 + k + k * k / 3)) + 8


# ---- the loop form's prelude -------------------------------------------------------------------------------------------------

@_in_context
def loop_prelude(y, sigma_f, use_decimal=None):
    """(exact, bounds) of the loop form's scalings of the row coordinates y >= 0 (float64): dicts with y_s, amp, y_mean,
    y_std and y_train.  The bounds are for the float64 evaluation with sums of n terms in any order (units of u, n_ = n + 3):
      y_s      the deviations d_i = y_i - m err by u |d_i| + (n + 1) u m; the root of their mean square moves by at most the
               largest of those (it is 1-Lipschitz in the maximum norm) and by (n + 2) u s / 2 for the sum, the division and the
               root: e_ys = n_ u (y_s + m)
      amp      sigma_f^2 / y_s^2: relative 2 e_ys / y_s + 3 u
      v = y / y_s   relative rv = e_ys / y_s + u;   y_mean   (rv + (n + 1) u) mean |v|
      y_train  rv |v_i| + e_mean + u |y_train_i|;   y_std    max e_train + n_ u y_std"""
    ye = ext(np.asarray(y, dtype=np.float64), use_decimal)
    n = ye.shape[0]
    m1 = ye.sum() / n
    s = _sqrt(((ye - m1) * (ye - m1)).sum() / n)
    y_s = s + 1
    v = ye / y_s
    m2 = v.sum() / n
    yt = v - m2
    sd = _sqrt((yt * yt).sum() / n)
    if sd == 0:
        sd = sd + 1
    sf = ext(float(sigma_f), use_decimal)
    amp = sf * sf / (y_s * y_s)
    n_ = n + 3
    e_ys = n_ * U * float(y_s + m1)
    rv = e_ys / float(y_s) + U
    mean_abs_v = float(abs(v).sum() / n)
    e_mean = (rv + (n + 1) * U) * mean_abs_v
    e_train = rv * f64(abs(v)) + e_mean + U * f64(abs(yt))
    exact = dict(y_s=y_s, amp=amp, y_mean=m2, y_std=sd, y_train=yt)
    bounds = dict(y_s=e_ys, amp=(2 * e_ys / float(y_s) + 3 * U) * float(amp), y_mean=e_mean, y_train=e_train,
                  y_std=float(e_train.max()) + n_ * U * float(sd))
    return exact, bounds


def loop_weights(is_init, fix_endpoints):
    """The noise weights of a sorted training set: 1e-7 or 0.5 on the init points (gpet.py:161), 1 on the observations."""
    return np.where(np.asarray(is_init, dtype=bool), 1e-7 if fix_endpoints else 0.5, 1.0)


# ---- the core ----------------------------------------------------------------------------------------------------------------

@_in_context
def posterior(x, y_train, w, amp, length, noise, jitter, kernel, grid, y_mean=0.0, y_std=1.0, zero_noise=False, grid_roundings=1,
              use_decimal=None):
    """The posterior of the training set (x, y_train, w) -- float64, x sorted, y_train as it enters K alpha = y -- under
    K = amp rho(x / l) + diag(noise w) + jitter (the noise left out when zero_noise) on the grid -- an EXTENDED vector of inputs
    on the scale of x (the loop's pixel columns, or the converged fit's standardised columns), of which a float64 evaluation
    holds copies with grid_roundings roundings once divided by l.

    Returns a dict: K, L, alpha, mean, var (not clamped), cov in the extended format; the bounds of the module's docstring as
    float64 arrays b_factor [n, n], b_alpha [n], b_mean [Lg], b_var [Lg], b_cov [Lg, Lg]; ``safety``: the largest row sum of
    |K^-1| b_factor -- far below 1 where the factorisation of a float64 evaluation is certain to find positive pivots."""
    dec = USE_DECIMAL if use_decimal is None else use_decimal
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    l = ext(float(length), dec)
    ampe = ext(float(amp), dec)
    a = ext(x, dec) / l
    g = grid / l
    K = ampe * corr(kernel, a, a)
    noise_w = _zeros((n,), a) if zero_noise else ext(float(noise), dec) * ext(np.asarray(w, dtype=np.float64), dec)
    diag = ampe + noise_w + ext(float(jitter), dec)
    K[np.diag_indices(n)] = diag
    L = chol(K)
    yt = ext(np.asarray(y_train, dtype=np.float64), dec)
    alpha = bsub(L, fsub(L, yt[:, None]))[:, 0]
    Kt = ampe * corr(kernel, a, g)  # [n, Lg]
    V = fsub(L, Kt)
    Z = bsub(L, V)
    ys, ym = ext(float(y_std), dec), ext(float(y_mean), dec)
    lin = ys * _dot(Kt.T, alpha)
    mean = lin + ym
    Kss = ampe * corr(kernel, g, g)
    Kss[np.diag_indices(g.shape[0])] = ampe
    cov = Kss - _dot(V.T, V)
    var = cov.diagonal().copy()
    cov = cov * (ys * ys)
    # the bounds, in the same arithmetic
    a64, g64 = f64(a), f64(g)
    u = ext(U, dec)
    EK = ext(kernel_ulps(kernel, a64, a64), dec) * u * abs(K)
    EK[np.diag_indices(n)] = 3 * u * diag
    Et = ext(kernel_ulps(kernel, a64, g64, 1, grid_roundings), dec) * u * abs(Kt)
    Ess = ext(kernel_ulps(kernel, g64, g64, grid_roundings, grid_roundings), dec) * u * abs(Kss)
    Ess[np.diag_indices(g.shape[0])] = 0
    M = _dot(abs(L), abs(L.T))
    Kinv = bsub(L, fsub(L, ext(np.eye(n), dec)))
    sq = _sqrt(diag)
    b_factor = (n + 1) * u * sq[:, None] * sq[None, :] + EK
    dK = 3 * n * u * M + EK
    b_alpha = _dot(abs(Kinv), _dot(dK, abs(alpha)))
    aKt, aZ = abs(Kt), abs(Z)
    b_mean = ys * (_dot(aKt.T, b_alpha) + n * u * _dot(aKt.T, abs(alpha)) + _dot(Et.T, abs(alpha))) + u * (abs(lin) + abs(mean))
    zE = _dot(aZ.T, Et)
    b_cov = (ys * ys) * (3 * n * u * _dot(aZ.T, _dot(M, aZ)) + zE + zE.T + Ess + 4 * u * ampe)
    return dict(K=K, L=L, alpha=alpha, mean=mean, var=var, cov=cov, amp=float(amp), y_std=float(y_std), n=n,
                b_factor=f64(b_factor), b_alpha=f64(b_alpha), b_mean=f64(b_mean), b_cov=f64(b_cov), b_var=f64(b_cov.diagonal()),
                safety=float(_dot(abs(Kinv), b_factor).sum(axis=1).max()))


@_in_context
def final_posterior(xs, ys, w, par, kernel, grid_px, use_decimal=None):
    """The converged-fit form: the training set and par[0..8] as given, the grid (x - par[3]) / par[4] of the pixel columns
    grid_px.  ``out_mean`` = par[6] * mean + par[5] with b_out_mean = |par[6]| b_mean + u (|par[6] mean| + |out_mean|); the std
    and the covariance are the core's (not rescaled).  jitter = 1e-6."""
    dec = USE_DECIMAL if use_decimal is None else use_decimal
    par = [float(v) for v in par]
    g = (ext(np.asarray(grid_px, dtype=np.float64), dec) - ext(par[3], dec)) / ext(par[4], dec)
    r = posterior(xs, ys, w, par[0], par[1], par[2], 1e-6, kernel, g, y_mean=par[7], y_std=par[8], grid_roundings=3,
                  use_decimal=dec)
    scaled = ext(par[6], dec) * r["mean"]
    r["out_mean"] = scaled + ext(par[5], dec)
    r["b_out_mean"] = abs(par[6]) * r["b_mean"] + U * f64(abs(scaled) + abs(r["out_mean"]))
    return r


# ---- comparisons -------------------------------------------------------------------------------------------------------------

@_in_context
def within(ratios):
    """True when every one of the ratios (a dict's values) is a number of at most 1: a NaN -- an entry that is not a number on
    either side -- is a miss, which ``max(...) <= 1`` would not notice."""
    return all(bool(v <= 1.0) for v in ratios.values())


def ratio(got, want, bound):
    """max |got - want| / bound over the entries, the difference taken in the extended format (0 for no entries).  An entry
    with a zero bound must be met exactly (its ratio is 0 then, else inf).  NaN where an entry of got is not finite."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return float("nan")
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape)
    err = f64(abs(ext(got, _is_dec(want)) - want))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(q.max())


@_in_context
def factor_ratio(L_dev, ref):
    """max |L_dev L_dev^T - K|_ij / b_factor_ij over the lower triangle, the product in the extended format."""
    if not np.all(np.isfinite(L_dev)):
        return float("nan")
    Le = ext(np.tril(np.asarray(L_dev, dtype=np.float64)), _is_dec(ref["K"]))
    res = f64(abs(_dot(Le, Le.T) - ref["K"]))
    return float(np.tril(res / ref["b_factor"]).max())


@_in_context
def std_ratio(std_dev, ref):  # (NaN for a std that is not finite)
    """The std of a float64 evaluation, sqrt(max(var, 0) * y_std^2), against the exact variance: std^2 against the clamped
    variance under b_var + 3 u std^2; where the exact variance is below its bound (the clamp may or may not have acted),
    std <= sqrt(2 b_var) instead.  Returns the largest ratio."""
    std_dev = np.asarray(std_dev, dtype=np.float64)
    if not np.all(np.isfinite(std_dev)):
        return float("nan")
    dec = _is_dec(ref["cov"])
    var = ref["cov"].diagonal()  # (times y_std^2 already)
    s = ext(std_dev, dec)
    v64, b = f64(var), ref["b_var"]
    small = v64 < b
    q = f64(abs(s * s - np.where(small, 0 * var, var))) / (b + 3 * U * std_dev * std_dev)
    q = np.where(small, std_dev * std_dev / (2 * b), q)
    return float(q.max())


# ---- the training sets of the tests --------------------------------------------------------------------------------------------

M_ROWS = 64  # rows of every image of the tests
SIGMA_F, LENGTH = 12, 9  # the kernel of every case but those that say otherwise
SPANS = (63, 64, 65, 130)  # edge lengths: partial, exact and multiple 64-tiles of k_cov_mfma


class Case(object):
    """One training set on one edge.  n_cap, n_init, n: capacity, init points, count (n - n_init observations); Lg, x_st: the
    edge's span in an image of N columns; dup: the last observation repeats the first init point's column."""

    def __init__(self, n_cap, n_init, n, Lg, N, dup=False, seed=0, length=None):
        self.n_cap, self.n_init, self.n, self.Lg, self.N, self.dup, self.seed = n_cap, n_init, n, Lg, N, dup, seed
        self.length = LENGTH if length is None else length
        self.x_st = (N - Lg) // 3
        assert n_init <= n <= n_cap and self.x_st + Lg <= N and n - n_init <= N - n_init

    def key(self):
        return (self.n_cap, self.n_init, self.n, self.Lg, self.N, self.dup, self.seed, self.length)

    def __repr__(self):
        return "cap%d-init%d-n%d-Lg%d%s" % (self.n_cap, self.n_init, self.n, self.Lg, "-dup" if self.dup else "")

    def points(self):
        """(init [n_init, 2], obs [n - n_init, 2]) as int64 (x, y): the init points on the span's ends (and evenly inside it),
        the observations on distinct other columns of the whole image -- inside the span when n == Lg, which then holds every
        column --, the rows a sinusoid with integer scatter."""
        rng = np.random.default_rng(1000 * self.n_cap + 7 * self.n + self.Lg + self.seed)
        xi = np.unique(np.round(np.linspace(self.x_st, self.x_st + self.Lg - 1, max(self.n_init, 2))).astype(np.int64))[:self.n_init]
        assert xi.shape[0] == self.n_init
        n_obs = self.n - self.n_init
        if self.n == self.Lg:
            pool = np.arange(self.x_st, self.x_st + self.Lg)
        else:
            pool = np.arange(self.N)
        pool = np.setdiff1d(pool, xi)
        xo = rng.choice(pool, size=n_obs - (1 if self.dup else 0), replace=False)
        if self.dup:
            xo = np.r_[xo, xi[0]]
        row = lambda x: np.clip(np.round(M_ROWS / 2 + 0.3 * M_ROWS * np.sin(x / 23.0 + 0.1 * self.seed)), 1, M_ROWS - 2)
        yi = row(xi)
        if self.n_init >= 2:
            yi[-1] = min(yi[-1] + 3, M_ROWS - 2)
        yo = np.clip(row(xo) + rng.integers(-3, 4, size=xo.shape[0]), 0, M_ROWS - 1)
        return np.stack([xi, yi], axis=1).astype(np.int64), np.stack([xo, yo], axis=1).astype(np.int64)

    def training(self, fix_endpoints):
        """(x, y, w) sorted by x, stably, init points first (np.argsort of gpet.py:212 on init + obs)."""
        init, obs = self.points()
        pts = np.concatenate([init, obs], axis=0)
        order = np.argsort(pts[:, 0], kind="stable")
        w = loop_weights(np.arange(pts.shape[0]) < self.n_init, fix_endpoints)
        return pts[order, 0].astype(np.float64), pts[order, 1].astype(np.float64), w[order]

    def grid(self):
        return np.arange(self.x_st, self.x_st + self.Lg, dtype=np.float64)


def width_for(n_cap):
    """Image width for a capacity: the widest whose own bin count (delta_x = 2: about N / 2 + 2 whatever the span) stays below
    n_cap - n_init for up to five init points."""
    return 2 * (n_cap - 5) - 8


def spans_for(n_cap):
    """The edge lengths an image of that width holds."""
    return tuple(s for s in SPANS if s + 8 <= width_for(n_cap))


# regime -> capacities, and the counts under each (n_init = 2 unless the entry is (n_init, n)); counts above a
# capacity are left out for that capacity, "cap" and "cap-1" stand for the capacity itself
REGIMES = {
    "lds": ((64, 127, 128), ((1, 1), (2, 2), (5, 5), 3, 63, 64, 65, 127, 128)),
    "blocked": ((129, 200, 285, 286), (2, 63, 64, 65, 128, 129, 191, 192, 193, "cap-1", "cap")),
    "hbm": ((287, 330), (2, 64, 65, 256, 257, 287, "cap")),
}


def regime_of(n_cap):
    return "lds" if n_cap <= 128 else ("blocked" if n_cap <= 286 else "hbm")


@functools.lru_cache(maxsize=None)
def cases_of(n_cap):
    """The edges of one capacity: one Case per count of its regime's row, the spans cycling through SPANS; one of them with a
    duplicate of an init column; and the n == Lg case of the capacity (Lg = 64 up to n_cap = 199, else 130)."""
    caps, counts = REGIMES[regime_of(n_cap)]
    assert n_cap in caps
    N = width_for(n_cap)
    out, seen = [], set()
    for c in counts:
        n_init, n = c if isinstance(c, tuple) else (2, n_cap if c == "cap" else (n_cap - 1 if c == "cap-1" else c))
        if n > n_cap or (n_init, n) in seen:
            continue
        seen.add((n_init, n))
        spans = spans_for(n_cap)
        Lg = spans[len(out) % len(spans)]
        if n == Lg:  # (that is the n == Lg case's; here the noise stays)
            Lg = spans[(len(out) + 1) % len(spans)]
        out.append(Case(n_cap, n_init, n, Lg, N, dup=(n in (65, 129) and n_init == 2)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def full_grid_case(n_cap):
    """n == Lg: a training point on every column of the edge, where the weights vanish (sklearn_gpr.py:673-677) under either
    fix_endpoints setting.  With only the jitter of 1e-6 on its diagonal K is as well conditioned as the correlation matrix of
    adjacent columns alone: at the table's length scale of 9 columns that matrix is singular to working precision for the RBF
    kernel (the mean's bound is then of the size of the mean and pins nothing), so these sets have a length scale of half a
    column -- rho(1) = 0.14 for RBF and Matern-2.5 alike, a condition number of a few -- and meet the sharpness asked of every
    other set (tests/test_posterior_exact.py asserts it for both settings)."""
    Lg = 64 if n_cap < 200 else 130
    return Case(n_cap, 2, Lg, Lg, width_for(n_cap), length=0.5)


JITTER_ONLY_CAPS = (200, 287, 330)


@functools.lru_cache(maxsize=None)
def jitter_only_case(n_cap):
    """n == Lg = 130 once more, at a length scale of 2 columns, for the RBF kernel with fix_endpoints alone: K is then the jitter
    away from a matrix that is singular to working precision (condition number about 1e6).  The bounds on alpha and on the mean
    are of the size of alpha and the mean themselves there and pin NOTHING; the set is kept for the factor's residual, the
    variance and the covariance, whose bounds stay sharp (tests/test_posterior_exact.py asserts 1e-11 amp y_std^2 for them and
    that the mean's bound is indeed vacuous), and which separate a substitution from a product with an explicit inverse:
    k_vsolve_mfma's product with the inverse of a diagonal block missed b_cov by a factor 2.6 on exactly this set."""
    return Case(n_cap, 2, 130, 130, width_for(n_cap), length=2, seed=1)


ALL_CAPS = tuple(c for r in ("lds", "blocked", "hbm") for c in REGIMES[r][0])
# (kernel, fix_endpoints) of the table: RBF and Matern-2.5 under both settings everywhere; Matern-1.5 and -0.5 once per regime
COMBOS = (("RBF", False), ("RBF", True), ("M25", False), ("M25", True))
EXTRA_KERNELS = {64: ("M15", False), 127: ("M05", True), 200: ("M15", True), 285: ("M05", False), 287: ("M15", False),
                 330: ("M05", True)}


def combos_of(n_cap):
    return COMBOS + ((EXTRA_KERNELS[n_cap],) if n_cap in EXTRA_KERNELS else ())


@functools.lru_cache(maxsize=None)
def loop_reference(case_key, kernel, fix_endpoints, held=None, sigma_f=SIGMA_F):
    """(prelude exact, prelude bounds, core) of a Case in the loop form.  held: (y_train bytes, amp, y_mean, y_std) as the
    implementation under test holds them, None for the exact prelude rounded to float64."""
    c = Case(*case_key)
    x, y, w = c.training(fix_endpoints)
    exact, bounds = loop_prelude(y, sigma_f)
    if held is None:
        yt, amp, ym, ysd = f64(exact["y_train"]), float(exact["amp"]), float(exact["y_mean"]), float(exact["y_std"])
    else:
        yt, amp, ym, ysd = np.frombuffer(held[0], dtype=np.float64), held[1], held[2], held[3]
    core = posterior(x, yt, w, amp, c.length, 1.0, 1e-6, kernel, ext(c.grid()), y_mean=ym, y_std=ysd, zero_noise=(c.n == c.Lg))
    return exact, bounds, core


def final_inputs(case, fix_endpoints):
    """The converged form's inputs of a Case, standardised as gpet.py:235-238 and sklearn_gpr.py:229-234 do (in float64: they
    are inputs, taken as given): (xs, ys, w, par[12]) with amplitude, length scale and noise level that differ from edge to
    edge, a scale par[4] != 1 and offsets that are not zero."""
    x, y, w = case.training(fix_endpoints)
    if case.n == case.Lg:
        w = np.zeros_like(w)  # (the host zeroes them in this form)
    X_m, X_s = float(np.mean(x)), float(np.std(x)) if case.n > 1 else 1.0
    y_m, y_s = float(np.mean(y)), float(np.std(y)) if case.n > 1 else 1.0
    X_s, y_s = X_s or 1.0, y_s or 1.0
    if case.n == 1:  # (no spread to standardise by: any scales are legitimate inputs)
        X_s, y_s = 2.0, 3.0
    xs, v = (x - X_m) / X_s, (y - y_m) / y_s
    m2, s2 = float(np.mean(v)) + 0.03125, (float(np.std(v)) or 1.0) * 1.25  # (not the set's own: any values are legitimate)
    k = case.n % 5
    par = np.zeros(12)
    par[:9] = [0.5 + 0.25 * k, case.length * (1 + 0.1 * k) / X_s, 1.0 + 0.25 * k, X_m, X_s, y_m, y_s, m2, s2]
    return xs, (v - m2) / s2, w, par


@functools.lru_cache(maxsize=None)
def final_reference(case_key, kernel, fix_endpoints):
    c = Case(*case_key)
    xs, ys, w, par = final_inputs(c, fix_endpoints)
    return final_posterior(xs, ys, w, par, kernel, c.grid())


# the sharpness the inputs must keep (fix_endpoints = False): bounds that small pin every term of every sum
SHARP_MEAN, SHARP_VAR = 1e-10, 1e-11
SAFETY_MAX = 1e-3  # |K^-1| b_factor: K is this far from the nearest singular matrix in units of its own rounding bound


def sharpness(ref):
    """(largest b_mean / max |mean|, largest b_var / (amp y_std^2)) of a core."""
    return (float(ref["b_mean"].max() / np.abs(f64(ref["mean"])).max()),
            float(ref["b_var"].max() / (ref["amp"] * ref["y_std"] ** 2)))
