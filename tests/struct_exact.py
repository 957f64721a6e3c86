"""Extended-precision restatement of the loop's prior-eigenbasis ("structured") path -- the basis of the grid's correlation matrix,
U = L^-1 (c Q0[obs, :]^T Lam), H = c Lam - U^T U, beta, the mean and the factor rows -- with the bounds a float64 evaluation has
to meet, the on-grid training sets the tests use, a plain float64 restatement of the four stages and the mistakes it must not
survive (tests/test_struct_exact.py on the host, tests/test_gpu_struct_injected.py on the device).  The extended arithmetic, the
posterior it is compared with and the eigen stage's constants are those of tests/posterior_exact.py (px) and
tests/factor_exact.py (fx).  Nothing here comes from the oracle or from the kernels.

The path (csrc/gpet_k_factor.inc).  rho, the unit-amplitude correlation matrix of the edge's Lg pixel columns, is factored once,
at creation: pivoted Cholesky to 1e-14 of the first pivot (r0 rows), eigen-decomposition of its Gram matrix, rows
sqrt(lam_t) q_t; the basis keeps Q0 = (q_t) normalised and lam0.  Every formula below needs only rho~ = Q0^T Lam Q0 = rho - T:
with training columns obs, weights alpha and Cholesky factor L of K = c rho[obs, obs] + noise,

    Bo = c Q0[:, obs]^T Lam   (n x r0)      U = L^-1 Bo      H = c Lam - U^T U      beta = Bo^T alpha
    mean = y_std Q0^T beta + y_mean         Sigma_struct = y_std^2 Q0^T H Q0 = y_std^2 (c rho~ - c^2 rho~_o^T K^-1 rho~_o)

whether or not Q0's rows are orthogonal.  H = R Theta R^T (two-sided Jacobi, warm or cold), G = R sqrt(Theta) y_std, and the
factor rows are A = G^T Q0 with the sign rule sum_j A[k, j] / (j + 1) >= 0; GPET_BUF_EIGVALS holds Theta, unscaled.

Staging, as in px: every stage is judged on the float64 values the implementation under test HOLDS of the stage before -- the
basis bytes, its own L and alpha, its own H -- after those have met their own bounds, so that each bound is that of one stage's
arithmetic; the end-to-end checks then tie the result to px.posterior of the same training set.

Bounds (u = 2^-53; + - * / sqrt correctly rounded; a sum of m products in any order errs by m u sum |terms|, Higham 3.1, so the
4-wide chunks of the matrix cores and the two half sums of the mean are covered).  First order in u throughout: the terms left
out are n u cond(L) times the ones kept, below 1e-9 of them on every set of the table.

  basis, orth     the rows sqrt(lam_t) q_t are an fx factor of rho: |sqrt(lam_s lam_t) q_s.q_t| <= fx.bound_fro(rho, r0) for
                  s != t (the LDS path's ABSOLUTE orthogonality: q_s.q_t itself is not small where lam is 1e-13);
                  |q_t.q_t - 1| <= (Lg + 4) u  (sum of squares, root, division)
  basis, rec      |Q0^T Lam Q0 - rho|_ij <= (fx.C_REC r0 + Lg + 8 + c_k) u + 1e-14: fx's reconstruction bound on a unit diagonal;
                  the normalisation and lam0 = |row|^2 ((Lg + 8) u); the float64 rho the stage factors (px.kernel_ulps); and what
                  the stopping rule leaves: the Schur complement S of a pivoted Cholesky that stops when its largest diagonal entry
                  is <= 1e-14 of the first pivot (= 1) has |S_ij| <= sqrt(S_ii S_jj) <= 1e-14.  ``ext_pchol`` runs the rule in
                  the extended format: it predicts r0 and confirms that remainder, but its S is NOT the bound -- rho is
                  persymmetric, so the exact pivots tie in pairs and the float64 order need not be the extended one
  H               dU = |L^-1| (2 u |Bo| + (n + 1) u |L||U|)  (Bo: two products; the substitution solves (L + dL) U = Bo with
                  |dL| <= n u |L|, Thm 8.5 -- blocked or not: a block's subtraction is part of the same sums);
                  |H_dev - H|_ab <= (dU^T |U| + |U|^T dU)_ab + (n + 2) u (|U|^T |U|)_ab + 2 u c lam_a [a = b] + u |H_ab|
  beta, mean      |beta| : (n + 2) u |Bo|^T |alpha|;   mean: y_std (|Q0|^T b_beta + (r0 + 1) u |Q0|^T |beta|) + u (|lin| + |mean|)
  rows, given H   R Theta R^T - H: a rotation rounds its pair of rows by 6 u (fx), two sides, r0 - 1 rotations a sweep and
                  row, N_SWEEPS = 10: 120 r0 u |H|_F; R from orthogonal by 60 r0 u, twice: 120 r0 u; the warm start's
                  W^T H W: 4 r0 u; sqrt, y_std and the scaling: 6 u; and the off-diagonal part the stopping test
                  off^2 <= 1e-24 diag^2 admits: 1e-12 |H|_F.  jac = (C_JAC r0 u + 1e-12) |H|_F, C_JAC = 250.
                  The product A = G^T Q0 (r0-term sums, |G_tk| <= sqrt(H_tt) = h_t since sum_k G_tk^2 = H_tt):
                  |dA_kj| <= v_j = y_std (r0 + 3) u sum_t h_t |Q0_tj|.  With D = Q0 Q0^T - I, a_j = sum_k |A_kj|, t_k = sum_j v_j |A_kj|:
                    rec      |A^T A - y_std^2 Q0^T H Q0|_F <= y_std^2 (1 + |D|_F) jac + |v a^T + a v^T|_F
                    orth     |A_i.A_k| <= y_std^2 (h^T |D| h + jac) + t_i + t_k                              (i != k)
                    evnorm   |y_std^2 ev_k - |A_k|^2| <= y_std^2 (h^T |D| h + jac) + 2 t_k + (Lg + 2) u |A_k|^2
                    order    ev non-increasing;   sign: sum_j A_kj / (j + 1) >= -Lg u sum_j |A_kj| / (j + 1)  (fx's)
  end to end      A^T A - Sigma = (A^T A - y_std^2 Q0^T H_dev Q0) + y_std^2 Q0^T (H_dev - H(L_dev)) Q0
                                  + (Sigma_struct(L_dev) - Sigma_struct(L)) + (Sigma_struct(L) - Sigma):
                  rec, (1 + |D|_F) y_std^2 |b_H|_F, y_std^2 | |z~|^T b_factor |z~| |_F with z~ = K^-1 c rho~_o (the factor's
                  backward error, px.b_factor, which L_dev has met) and the truncation term, which is no bound but the exact
                  difference, formed in the extended format from the held basis and px's exact L.  px's b_cov is not part of
                  it: it bounds the generic path's sums, and nothing of the eigen stage.
                  mean: b_mean of the stage + y_std |c rho~_o|^T b_alpha + |mean_struct(alpha) - mean|.
  n == Lg         the weights vanish and K is the jitter away from c rho: H is what the jitter leaves, and the bounds are
                  sharp only in absolute terms, SHARP_ABS amp y_std^2 (amp lam for H) -- as px.jitter_only_case.  The mean's
                  bound may be of the size of the mean there (tests/test_struct_exact.py says where), and nowhere else.
"""
import functools

import numpy as np

from tests import factor_exact as fx
from tests import posterior_exact as px

U = px.U
C_JAC = 250
OFF_TOL = 1e-12  # sqrt of the Jacobi's stopping test off^2 <= 1e-24 diag^2
N_IMG = 304      # columns of every image of the tests
SHARP_ABS = 1e-9


# ---- the training sets ---------------------------------------------------------------------------------------------------------

class Case(object):
    """One on-grid training set on one edge: n_init = 2 init points on the span's ends, n - 2 observations on distinct other
    columns OF THE SPAN (px.Case draws from the whole image, which takes a batch off the path); dup: the last observation
    repeats the first init point's column.  fam names the batch (one capacity, one basis); r0: the range the rank must fall in."""

    def __init__(self, fam, Lg, n_cap, n, length, r0, factor_cap=96, dup=False, seed=0, x_st=None):
        self.fam, self.Lg, self.n_cap, self.n, self.length, self.r0, self.factor_cap, self.dup, self.seed = fam, Lg, n_cap, n, length, r0, factor_cap, dup, seed
        self.N, self.n_init, self.kernel = N_IMG, 2, "RBF"
        self.x_st = (N_IMG - Lg) // 3 if x_st is None else int(x_st)
        assert 0 <= self.x_st and self.x_st + Lg <= N_IMG
        assert 2 <= n <= n_cap and n - 2 - (1 if dup else 0) <= Lg - 2

    def key(self):
        return (self.fam, self.Lg, self.n_cap, self.n, self.length, self.r0, self.factor_cap, self.dup, self.seed, self.x_st)

    def __repr__(self):
        return "%s-n%d%s" % (self.fam, self.n, "-dup" if self.dup else "")

    def points(self):
        rng = np.random.default_rng(1000 * self.n_cap + 7 * self.n + self.Lg + self.seed)
        xi = np.array([self.x_st, self.x_st + self.Lg - 1], dtype=np.int64)
        pool = np.arange(self.x_st + 1, self.x_st + self.Lg - 1)
        xo = rng.choice(pool, size=self.n - 2 - (1 if self.dup else 0), replace=False)
        if self.dup:
            xo = np.r_[xo, xi[0]]
        row = lambda x: np.clip(np.round(px.M_ROWS / 2 + 0.3 * px.M_ROWS * np.sin(x / 23.0 + 0.1 * self.seed)), 1, px.M_ROWS - 2)
        yi = row(xi)
        yi[-1] = min(yi[-1] + 3, px.M_ROWS - 2)
        yo = np.clip(row(xo) + rng.integers(-3, 4, size=xo.shape[0]), 0, px.M_ROWS - 1)
        return np.stack([xi, yi], axis=1).astype(np.int64), np.stack([xo, yo], axis=1).astype(np.int64)

    def training(self):
        """(x, y, w) sorted by x, stably, init points first; fix_endpoints is set on every batch of these tests."""
        init, obs = self.points()
        pts = np.concatenate([init, obs], axis=0)
        order = np.argsort(pts[:, 0], kind="stable")
        w = px.loop_weights(np.arange(pts.shape[0]) < 2, True)
        return pts[order, 0].astype(np.float64), pts[order, 1].astype(np.float64), w[order]

    def grid(self):
        return np.arange(self.x_st, self.x_st + self.Lg, dtype=np.float64)


class HeldCase(Case):
    """A Case whose points are given: the span (x_st, Lg), the two init points and an observation set read back from a device."""

    def __init__(self, fam, Lg, x_st, n_cap, length, init, obs, factor_cap=96):
        self._init, self._obs = np.asarray(init, dtype=np.int64).reshape(-1, 2), np.asarray(obs, dtype=np.int64).reshape(-1, 2)
        Case.__init__(self, fam, Lg, n_cap, 2 + self._obs.shape[0], length, (1, 96), factor_cap, dup=True)
        self.x_st = int(x_st)
        assert self._init.shape[0] == 2 and np.all((self._obs[:, 0] >= self.x_st) & (self._obs[:, 0] < self.x_st + Lg))

    def points(self):
        return self._init, self._obs


# family -> (Lg, n_cap, length scale, (r0_lo, r0_hi), factor_cap, counts; a count (n, "dup") repeats an init column).
# The length scales were chosen with fx.greedy_pivots on the float64 rho: the last pivot taken at least 1.8 times the stopping
# tolerance, the largest one left at most 0.6 of it (tests/test_struct_exact.py asserts the margins), so the rank is no matter
# of rounding.  Ranks 83 .. 87 have no such length scale on these widths: the Jacobi switch 82 | 84 is reached by 82 and 88.
FAMILIES = {
    # small form (n_cap <= 128): k_struct_H
    "s100": (130, 100, 11.125, (33, 48), 96, (2, 3, 63, 64, (65, "dup"), 99, 100)),   # L beside U in LDS
    "s128": (300, 128, 9.6375, (84, 88), 96, (2, 3, 63, 64, (65, "dup"), 127, 128)),                  # rows of L streamed
    "s100c40": (130, 100, 14.75, (1, 32), 40, (80, 81, 100)),                        # factor_cap 40: the indices leave LDS above n = 80
    "full64": (64, 64, 9.125, (1, 32), 96, (64,)),                                   # n == Lg
    "e56": (300, 64, 16.25, (49, 64), 96, (2, 40)),
    "e70": (130, 64, 5.375, (65, 72), 96, (2, 40)),
    "e80": (300, 64, 10.7875, (73, 80), 96, (2, 40)),
    "e81": (300, 64, 10.6125, (81, 82), 96, (40,)),
    "e82": (300, 64, 10.45, (81, 82), 96, (40,)),
    "e90": (300, 64, 9.4, (90, 96), 96, (40,)),
    "w63": (63, 64, 8.65, (1, 32), 96, (2, 40)),
    "w64": (64, 64, 9.125, (1, 32), 96, (40,)),
    "w65": (65, 64, 8.4875, (1, 32), 96, (40,)),
    # blocked form (n_cap >= 129): k_structB_build, k_struct_beta, k_struct_trsm, k_struct_Hbig, k_struct_mean
    "b129": (130, 129, 44.375, (15, 15), 96, (2, 63, 64, (65, "dup"), 128, 129)),
    "b192": (200, 192, 61.5, (16, 16), 96, (2, 63, 64, 65, 128, (129, "dup"), 191, 192)),
    "b193": (200, 193, 55.125, (17, 17), 96, (2, 63, 64, 65, 128, 129, 191, 192, 193)),
    "b257": (300, 257, 18.25, (49, 64), 96, (2, 63, 64, 65, 128, (129, "dup"), 191, 192, 193, 256, 257)),
    "b257r": (300, 257, 9.6375, (84, 88), 96, (2, 63, 64, 65, 128, 129, 191, 192, 193, 256, 257)),
    "full130": (130, 130, 11.125, (33, 48), 96, (130,)),                             # n == Lg
}
R0_CLASSES = ((1, 32), (33, 48), (49, 64), (65, 72), (73, 80), (81, 82), (84, 88), (90, 96))  # the six K extents; 80 | 81; 82 | 84; 88 | 90


@functools.lru_cache(maxsize=None)
def cases_of(fam):
    Lg, n_cap, length, r0, fcap, counts = FAMILIES[fam]
    out = []
    for c in counts:
        n, dup = (c[0], True) if isinstance(c, tuple) else (c, False)
        out.append(Case(fam, Lg, n_cap, n, length, r0, fcap, dup))
    return tuple(out)


ALL_CASES = tuple(c for f in FAMILIES for c in cases_of(f))


def is_full(c):
    return c.n == c.Lg


# ---- rho and its basis ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rho_ext(Lg, x_st, length, kernel="RBF"):
    """rho on the span in the extended format (unit diagonal)."""
    a = px.ext(np.arange(x_st, x_st + Lg, dtype=np.float64)) / px.ext(float(length))
    R = px.corr(kernel, a, a)
    R[np.diag_indices(Lg)] = px.ext(1.0)
    return R


def rho_f64(Lg, x_st, length):
    """The float64 rho a factor stage starts from: exp(-0.5 (d * d)) of d = fl(x_i / l) - fl(x_j / l)."""
    a = np.arange(x_st, x_st + Lg, dtype=np.float64) / float(length)
    d = a[:, None] - a[None, :]
    R = np.exp(-0.5 * (d * d))
    R[np.diag_indices(Lg)] = 1.0
    return R


@functools.lru_cache(maxsize=None)
def ext_pchol(Lg, x_st, length, cap=97):
    """Greedy pivoted Cholesky of rho in the extended format under the device's rule (stop when the largest remaining diagonal
    entry is <= 1e-14 of the first pivot): (rank, last pivot / tol, largest remaining diagonal entry / tol)."""
    S = np.array(rho_ext(Lg, x_st, length))
    d = S.diagonal().copy()
    G = []
    used = np.zeros(Lg, dtype=bool)
    tol, last = None, None
    for k in range(min(cap, Lg)):
        p = int(np.argmax(np.where(used, -1.0, px.f64(d))))
        if k == 0:
            tol = d[p] * px.ext(fx.PIVOT_TOL)
        if not d[p] > tol:
            break
        last = d[p]
        row = S[p].copy()
        for g in G:
            row = row - g[p] * g
        row = row / px._sqrt(d[p])
        row[used] = 0
        G.append(row)
        used[p] = True
        d = d - row * row
    rem = px.f64(np.where(used, 0 * d, d)).max() if Lg else 0.0
    return len(G), float(last / tol), float(rem / px.f64(tol))


def basis_margins(c):
    """(rank, last pivot / tol, remainder / tol) of fx.greedy_pivots on the float64 rho."""
    piv, rem, tol = fx.greedy_pivots(rho_f64(c.Lg, c.x_st, c.length), cap=min(c.Lg, 97))
    return piv.size, float(piv[-1] / tol), float(rem / tol)


def basis_ratios(c, Q0, lam0):
    """The two basis bounds on held (Q0, lam0); also returns D = Q0 Q0^T - I as float64."""
    r, Lg = Q0.shape
    Q, lam = px.ext(Q0), px.ext(lam0)
    R = rho_ext(c.Lg, c.x_st, c.length)
    Dx = Q @ Q.T - px.ext(np.eye(r))
    D = px.f64(Dx)
    sl = np.sqrt(np.abs(lam0))
    off = np.abs(D) * np.outer(sl, sl)
    np.fill_diagonal(off, 0.0)
    bf = fx.C_REC * r * U * Lg  # fx.bound_fro of a unit diagonal
    a = np.arange(c.x_st, c.x_st + Lg, dtype=np.float64) / c.length
    ck = px.kernel_ulps("RBF", a, a)
    b_rec = (fx.C_REC * r + Lg + 8 + ck) * U + fx.PIVOT_TOL
    rec = px.f64(abs((Q.T * lam[None, :]) @ Q - R))
    out = dict(q_orth=float(off.max(initial=0.0) / bf), q_norm=float(np.abs(np.diag(D)).max() / ((Lg + 4) * U)),
               q_rec=float((rec / b_rec).max()))
    if not (np.all(np.isfinite(Q0)) and np.all(np.isfinite(lam0))):
        out = {k: float("nan") for k in out}
    return out, D


# ---- the stages on held inputs -------------------------------------------------------------------------------------------------

def _idx(c):
    return (c.training()[0] - c.x_st).astype(np.int64)


def stage_h(c, Q0, lam0, L, alpha, amp, y_mean, y_std):
    """Exact U, H, beta, mean, Sigma_struct of the held basis, factor and weights, and the bounds b_H, b_beta, b_mean."""
    n, r = L.shape[0], Q0.shape[0]
    idx = _idx(c)
    Q, lam, Lx, al = px.ext(Q0), px.ext(lam0), px.ext(np.tril(L)), px.ext(alpha)
    ce, ys, ym = px.ext(float(amp)), px.ext(float(y_std)), px.ext(float(y_mean))
    Bo = ce * lam[None, :] * Q[:, idx].T
    Ux = px.fsub(Lx, Bo)
    H = -(Ux.T @ Ux)
    H[np.diag_indices(r)] = H.diagonal() + ce * lam
    beta = Bo.T @ al
    lin = ys * (Q.T @ beta)
    mean = lin + ym
    aU, aBo, aL = px.f64(abs(Ux)), px.f64(abs(Bo)), np.abs(np.tril(L))
    Linv = px.f64(abs(px.fsub(Lx, px.ext(np.eye(n)))))
    dU = Linv @ (2 * U * aBo + (n + 1) * U * (aL @ aU))
    b_H = dU.T @ aU + aU.T @ dU + (n + 2) * U * (aU.T @ aU) + np.diag(2 * U * float(amp) * np.abs(lam0)) + U * px.f64(abs(H))
    b_beta = (n + 2) * U * (aBo.T @ np.abs(alpha))
    aQ = np.abs(Q0)
    b_mean = abs(float(y_std)) * (aQ.T @ b_beta + (r + 1) * U * (aQ.T @ px.f64(abs(beta)))) + U * px.f64(abs(lin) + abs(mean))
    return dict(U=Ux, H=H, beta=beta, mean=mean, b_H=b_H, b_beta=b_beta, b_mean=b_mean, Bo=Bo)


def rows_ratios(c, Q0, D, H_dev, A, ev, y_std):
    """The factor rows and eigenvalues against the held H (module docstring: rows, given H)."""
    r, Lg = Q0.shape
    if A.shape != (r, Lg) or ev.shape != (r,) or not (np.all(np.isfinite(A)) and np.all(np.isfinite(ev)) and np.all(np.isfinite(H_dev))):
        return dict(rec=float("nan"), orth=float("nan"), evnorm=float("nan"), order=float("nan"), sign=float("nan"))
    ys2 = float(y_std) ** 2
    Hf = float(np.sqrt((H_dev * H_dev).sum()))
    jac = (C_JAC * r * U + OFF_TOL) * Hf
    h = np.sqrt(np.maximum(np.diag(H_dev), 0.0))
    hDh = float(h @ np.abs(D) @ h)
    aQ, aA = np.abs(Q0), np.abs(A)
    v = abs(float(y_std)) * (r + 3) * U * (h @ aQ)
    a = aA.sum(axis=0)
    t = aA @ v
    Ax, Q = px.ext(A), px.ext(Q0)
    S = (px.ext(ys2) * (Q.T @ px.ext(H_dev))) @ Q
    res = px.f64(Ax.T @ Ax - S)
    b_rec = ys2 * (1 + float(np.sqrt((D * D).sum()))) * jac + float(np.sqrt(((np.outer(v, a) + np.outer(a, v)) ** 2).sum()))
    Gm = px.f64(Ax @ Ax.T)
    nrm2 = np.diag(Gm).copy()
    off = np.abs(Gm)
    np.fill_diagonal(off, 0.0)
    b_orth = ys2 * (hDh + jac) + t[:, None] + t[None, :]
    b_ev = ys2 * (hDh + jac) + 2 * t + (Lg + 2) * U * nrm2
    wts = 1.0 / np.arange(1, Lg + 1)
    sg = px.f64((Ax * px.ext(wts)[None, :]).sum(axis=1))
    tol = Lg * U * (aA * wts[None, :]).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sign = float(np.where(sg >= 0, 0.0, np.where(tol > 0, -sg / tol, np.inf)).max())
    return dict(rec=float(np.sqrt((res * res).sum()) / b_rec), orth=float((off / b_orth).max()),
                evnorm=float((np.abs(ys2 * ev - nrm2) / b_ev).max()), order=0.0 if np.all(np.diff(ev) <= 0) else float("inf"), sign=sign,
                _b_rec=b_rec)


@functools.lru_cache(maxsize=None)
def _core(x_bytes, w_bytes, x_st, Lg, length, full, yt_bytes, amp, y_mean, y_std):
    x, w, yt = (np.frombuffer(b, dtype=np.float64) for b in (x_bytes, w_bytes, yt_bytes))
    grid = px.ext(np.arange(x_st, x_st + Lg, dtype=np.float64))
    return px.posterior(x, yt, w, amp, length, 1.0, 1e-6, "RBF", grid, y_mean=y_mean, y_std=y_std, zero_noise=full)


def check_all(c, got):
    """Every bound of the module docstring on what an implementation holds for Case c.  got: dict of float64 values -- Q0, lam0,
    y_s, amp, y_mean, y_std, y_train, L (n x n, lower), alpha, H, mean, A, ev.  Returns {check: error / bound} (NaN: not finite)
    and the pieces the sharpness statements need."""
    x, y, w = c.training()
    n = x.shape[0]
    out = {}
    ex, bd = px.loop_prelude(y, px.SIGMA_F)
    for k in ("y_s", "amp", "y_mean", "y_std"):
        out[k] = px.ratio(got[k], ex[k], bd[k])
    out["y_train"] = px.ratio(got["y_train"], ex["y_train"], bd["y_train"])
    core = _core(x.tobytes(), w.tobytes(), c.x_st, c.Lg, float(c.length), is_full(c), np.ascontiguousarray(got["y_train"], dtype=np.float64).tobytes(),
                 float(got["amp"]), float(got["y_mean"]), float(got["y_std"]))
    out["L"] = px.factor_ratio(got["L"], core)
    out["alpha"] = px.ratio(got["alpha"], core["alpha"], core["b_alpha"])
    Q0, lam0 = np.asarray(got["Q0"]), np.asarray(got["lam0"])
    r = Q0.shape[0]
    br, D = basis_ratios(c, Q0, lam0)
    out.update(br)
    st = stage_h(c, Q0, lam0, np.asarray(got["L"]), np.asarray(got["alpha"]), got["amp"], got["y_mean"], got["y_std"])
    Hd = np.asarray(got["H"])
    out["H"] = px.ratio(Hd, st["H"], st["b_H"]) if Hd.shape == (r, r) else float("nan")
    out["H_sym"] = 0.0 if Hd.shape == (r, r) and np.array_equal(Hd, Hd.T) else float("inf")
    out["mean"] = px.ratio(got["mean"], st["mean"], st["b_mean"])
    rr = rows_ratios(c, Q0, D, Hd if Hd.shape == (r, r) else np.full((r, r), np.nan), np.asarray(got["A"]), np.asarray(got["ev"]), got["y_std"])
    b_rec = rr.pop("_b_rec", float("nan"))
    out.update(rr)
    # end to end: the exact chain on px's exact L and alpha, from the held basis
    Q, lam = px.ext(Q0), px.ext(lam0)
    ce, ys = px.ext(float(got["amp"])), px.ext(float(got["y_std"]))
    Ue = px.fsub(core["L"], st["Bo"])
    He = -(Ue.T @ Ue)
    He[np.diag_indices(r)] = He.diagonal() + ce * lam
    Sig = ((ys * ys) * (Q.T @ He)) @ Q
    trunc = px.f64(abs(Sig - core["cov"]))
    Zt = px.f64(abs(px.bsub(core["L"], Ue) @ Q))  # |K^-1 c rho~_o|  (n x Lg)
    ys2 = float(got["y_std"]) ** 2
    b3 = ys2 * (Zt.T @ core["b_factor"] @ Zt)
    fro = lambda M: float(np.sqrt((np.asarray(M, dtype=np.float64) ** 2).sum()))
    nQ2 = 1 + fro(D)
    b_cov = fro(trunc) + fro(b3) + ys2 * nQ2 * fro(st["b_H"]) + b_rec
    A = np.asarray(got["A"])
    if A.shape == (r, c.Lg) and np.all(np.isfinite(A)):
        Ax = px.ext(A)
        out["e2e_cov"] = fro(px.f64(Ax.T @ Ax - core["cov"])) / b_cov
    else:
        out["e2e_cov"] = float("nan")
    mean_e = ys * (Q.T @ (st["Bo"].T @ core["alpha"])) + px.ext(float(got["y_mean"]))
    b_e2e_mean = st["b_mean"] + abs(float(got["y_std"])) * (px.f64(abs(st["Bo"] @ Q)).T @ core["b_alpha"]) + px.f64(abs(mean_e - core["mean"]))
    out["e2e_mean"] = px.ratio(got["mean"], core["mean"], b_e2e_mean)
    sharp = dict(H=float(st["b_H"].max() / (float(got["amp"]) * np.abs(lam0).max())), cov=b_cov / (float(got["amp"]) * ys2 * c.Lg),
                 mean=float(b_e2e_mean.max() / np.abs(px.f64(core["mean"])).max()), trunc=fro(trunc) / b_cov)
    return out, sharp


# ---- a float64 restatement, and the mistakes it must not survive -----------------------------------------------------------------

MUTATIONS = ("drop_basis", "drop_row", "skip_block", "tile_H", "rows_tile", "sign", "lam_once", "upper_L")


def applies(mut, c):
    """The class of cases a mutation belongs to: a skipped 64-block needs a second block; the two triangles of the factor's buffer
    differ where a third training point couples with the others (the two init points alone stand a whole span apart: their
    off-diagonal entry is exp(-(Lg / l)^2 / 2), as good as zero in K and in L alike)."""
    return c.n > 64 if mut == "skip_block" else (c.n > 2 if mut == "upper_L" else True)


@functools.lru_cache(maxsize=None)
def restated_basis(Lg, x_st, length):
    """(Q0, lam0): pivoted Cholesky of the float64 rho under the device's rule, then the right singular vectors of its rows."""
    R = rho_f64(Lg, x_st, length)
    piv, _, _ = fx.greedy_pivots(R, cap=min(Lg, 97))
    r = piv.size
    d = np.diag(R).copy()
    G = np.zeros((r, Lg))
    used = np.zeros(Lg, dtype=bool)
    for k in range(r):
        p = int(np.argmax(np.where(used, -1.0, d)))
        G[k] = np.where(used, 0.0, (R[p] - G[:k, p] @ G[:k]) / np.sqrt(d[p]))
        used[p] = True
        d = np.maximum(d - G[k] * G[k], 0.0)
    _, s, Vt = np.linalg.svd(G, full_matrices=False)
    return Vt, s * s


def restate(c, mut=None):
    """The four stages in float64 numpy, in the natural order; mut: one of MUTATIONS, a mistake a kernel can make."""
    import scipy.linalg as sl
    x, y, w = c.training()
    n, Lg = x.shape[0], c.Lg
    Q0, lam0 = restated_basis(c.Lg, c.x_st, c.length)
    r = Q0.shape[0]
    y_s = np.std(y) + 1.0
    v = y / y_s
    y_mean = np.mean(v)
    yt = v - y_mean
    y_std = np.std(yt) or 1.0
    amp = px.SIGMA_F ** 2 / y_s ** 2
    a = x / c.length
    d = a[:, None] - a[None, :]
    K = amp * np.exp(-0.5 * (d * d))
    K[np.diag_indices(n)] = amp + (0.0 if is_full(c) else 1.0 * w) + 1e-6
    L = np.linalg.cholesky(K)
    alpha = sl.solve_triangular(L.T, sl.solve_triangular(L, yt, lower=True), lower=False)
    idx = _idx(c)
    Bo = amp * lam0[None, :] * Q0[:, idx].T
    if mut == "lam_once":
        Bo = amp * Q0[:, idx].T
    Ls = L
    if mut == "upper_L":  # (the buffer's upper triangle still holds K)
        Ls = np.tril(K, -1) + np.diag(np.diag(L))
    Um = sl.solve_triangular(Ls, Bo, lower=True)
    if mut == "skip_block":  # block 1 solved against its diagonal block alone
        k1 = min(n, 128)
        Um = Um.copy()
        Um[64:k1] = sl.solve_triangular(L[64:k1, 64:k1], Bo[64:k1], lower=True)
    if mut == "drop_row":
        Um = Um[:n - 1]
    H = np.diag(amp * lam0) - Um.T @ Um
    H = 0.5 * (H + H.T)
    if mut == "tile_H":
        t = min(16, r)
        H[:t, :t] = np.diag(amp * lam0[:t])
    if mut == "drop_basis":
        H[r - 1, :] = 0.0
        H[:, r - 1] = 0.0
    beta = (Bo[:n - 1] if mut == "drop_row" else Bo).T @ (alpha[:n - 1] if mut == "drop_row" else alpha)
    mean = y_std * (Q0.T @ beta) + y_mean
    if not np.all(np.isfinite(H)):  # (a mutation on a jitter-only set can overflow: nothing to decompose)
        nan = np.full((r, Lg), np.nan)
        return dict(Q0=Q0, lam0=lam0, y_s=y_s, amp=amp, y_mean=y_mean, y_std=y_std, y_train=yt, L=L, alpha=alpha, H=H, mean=mean, A=nan, ev=nan[:, 0])
    th, Rm = np.linalg.eigh(H)
    th, Rm = th[::-1], Rm[:, ::-1]
    A = (Rm * (y_std * np.sqrt(np.maximum(th, 0.0)))[None, :]).T @ Q0
    flip = (A / np.arange(1, Lg + 1)[None, :]).sum(axis=1) < 0
    A[flip] = -A[flip]
    if mut == "rows_tile":
        A[:, 64 * ((Lg - 1) // 64):] = 0.0
    if mut == "sign":
        A[0] = -A[0]
    return dict(Q0=Q0, lam0=lam0, y_s=y_s, amp=amp, y_mean=y_mean, y_std=y_std, y_train=yt, L=L, alpha=alpha, H=H, mean=mean, A=A, ev=th)


def worst(ratios):
    """(name, value) of the largest ratio; a NaN wins."""
    bad = [(k, v) for k, v in ratios.items() if not v == v]
    return bad[0] if bad else max(ratios.items(), key=lambda kv: kv[1])
