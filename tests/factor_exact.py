"""Covariances of known spectrum for the eigen-factor stage (GPET_BUF_COV -> GPET_BUF_FACTOR, GPET_BUF_EIGVALS), an
extended-precision reference of their factor, and the bounds a float64 factor has to meet: tests/test_factor_exact.py pins the
reference on the host, tests/test_gpu_factor_injected.py the kernels (csrc/gpet_k_factor.inc, csrc/gpet_eig.hip) against it,
tests/test_gpu_factor_warm_injected.py the any-rank path's warm start ("Warm start" below).
Nothing here comes from the oracle or from the kernels.

Inputs.  Sigma = B^T B with B (r x Lg) a matrix of small integers times powers of two, so that every entry of Sigma is a sum of
at most 136 integers below 10 on a grid of 2^-32 (the warm start's cases: at most 193 on a grid of 2^-18): exact in float64 in any order of summation (``sigma_of`` forms it in the
extended format and asserts that nothing is lost).  The exact rank is r.
* ``graded``: B = diag(2^-e_k) C, C random integers in [-3, 3], e_k integers over ``octaves`` <= 16 (``graded_exponents``; rank-deficient cases with a lead row, see there): a spectrum
  that spans about 4^octaves with no structure the kernels could exploit.
* ``hadamard``: rows of a Sylvester-Hadamard matrix in the first columns, groups of them scaled by the same power of two:
  EXACTLY equal eigenvalues n 4^-e, eigenvectors h_k / sqrt(n) known without a solver; B's rows are the factor's rows.
* ``diagonal``: one entry per row -- a diagonal Sigma, with ties: the pivot rule "smallest index", every rotation trivial.
* ``pair_small`` / ``pair_large``: two nearly equal diagonal entries coupled by 2^-50 / by 1/4 against a difference of 2^-9 /
  2^-19 -- rotation angles of 1e-13 and of pi/4 to 1e-6 --, next to three separated directions.

Reference.  ``ref_factor`` is a one-sided (Hestenes) Jacobi on the rows of B in np.longdouble (``decimal`` at 40 digits where long
double has no 64-bit mantissa: posterior_exact.USE_DECIMAL), vectorised over the disjoint pairs of a round-robin round: rows are
rotated until every pair has |x.y| <= 1e-17 |x||y|; they are then sqrt(s_k) v_k and their squared norms s_k.

Rank test.  The device's pivoted Cholesky stops at 1e-14 of its first pivot.  ``greedy_pivots`` restates it in float64; a case is
SAFE when it takes exactly r pivots, each above 100 tol, and leaves a diagonal below 0.05 tol (``rank_safe``): the rank the
device finds is then no matter of rounding.  tests/test_factor_exact.py asserts it for every case; the GPU test does not discover it.

Bounds (u = 2^-53).  bound_ij = C_REC r u sqrt(Sigma_ii Sigma_jj) for |A^T A - Sigma|_ij, from the roundings of the algorithm --
both paths compute A = Q G with G the pivoted Cholesky factor (r rows) and Q a product of plane rotations:
* G^T G - Sigma: the r-term sums of the factorisation, (r + 1) u sum_t |g_ti||g_tj| <= (r + 1) u sqrt(Sigma_ii Sigma_jj) (Higham,
  Accuracy and Stability, Thm 10.3; Cauchy-Schwarz), and the Schur complement that is left where the factorisation stops, which
  ``rank_safe`` holds below 0.05 tol = 4.5 u max Sigma_ii <= r u sqrt(Sigma_ii Sigma_jj) for r >= 5 where the diagonal is even
  (below r = 5 the factorisation of these inputs is all but exact):                                                       2 r u
* Q^T Q - I.  One application of a rotation, x' = fma(c, x, -(s y)), y' = fma(s, x, c y), rounds twice per entry: at most
  2 u |(x, y)| for the pair.  (c, s) itself: c = rsqrt(1 + t^2) by two Newton steps (2 u), s = t c (u), 1 + t^2 rounded (u):
  |c^2 + s^2 - 1| <= 7 u, the pair's norm moves by 3.5 u.  Together under 6 u per rotation and row of Q; a row meets r - 1
  rotations a sweep (LDS path: one per round; any-rank path: r / 8 products with an accumulated 16 x 16 rotation, each 15
  rotations deep and a 16-term sum: the same count), so |Q^T Q - I|_2 <= 2 * 6 u (r - 1) per sweep to first order, and
  |G^T (Q^T Q - I) G|_ij <= |g_i||g_j| 12 u r per sweep.  Sweeps: the reference needs 7-8 on these inputs, the kernels stop
  earlier (their tests are looser); the bound allows the rounding of N_SWEEPS = 10 (the GPU tests print the count the kernels
  report; more sweeps than that have to fit the same allowance):                                                       120 r u
* the rows' r-term sums A_kj = sum_t q_tk g_tj (k_factor_rows; the any-rank path has none, its rotations act on G's rows): r u
  sum_t |q_tk||g_tj| per entry, in A^T A twice:                                                                            2 r u
C_REC = 2 + 12 * 10 + 2 = 124: 1.3e-12 at r = 96 (the LDS path's tests had 1e-9 s_0), 1.9e-12 at r = 136 (the any-rank path's
tests have 2e-12 max |Sigma|).  ``bound_fro`` = |bound|_F = C_REC r u trace(Sigma) is the Weyl bound of the eigenvalues and the
E of Davis-Kahan: a row of gap g to every other eigenvalue (0 included when r < Lg) is within sqrt(s_k) 2 |bound|_F / g, plus
the difference of the norms, of the reference's; rows where that exceeds sqrt(s_k) / 10 -- gap below ``iso_gap`` = 20 |bound|_F --
are compared as clusters: sum over the group of A_k^T A_k, by the gap to the nearest eigenvalue outside the group.
``isolated_fraction`` (from the reference alone) must be at least 0.9 for every case that has no exact degeneracy: the octaves are
chosen so that it is (``test_isolated_rows_are_not_skipped``).

Warm start (any-rank path, k_ojw_* of csrc/gpet_eig.hip).  From the second factor of a trace on, the Jacobi starts from rows built
out of the previous factor's rows A_0: with s_k = |A_0k|^2, T = A_0 Sigma, M' = T A_0^T, L' = chol(M'), X = (diag(1 / s) L')^T A_0.
* Inputs (``WARM``: widths 97, 128, 129, 130, 161, 193).  "w<Lg>-0": Sigma_0 = B_0^T B_0, B_0 = graded(Lg, Lg, octaves) of full rank.
  "w<Lg>-1": Sigma_1 = (D B_0)^T (D B_0), D = ``warm_scales``: ones, and 2^-1 / 2^-3 alternately on 5 or 40 rows -- Sigma_0 less a
  positive-semidefinite matrix of that rank, what an iteration's new observations do to a posterior covariance; exact in float64.
  Octaves 3 .. 6, chosen per width so that r u s_0 / s_min <= 1e-6 for both matrices (1.2e-8 .. 7.6e-7; a square C of integers
  is ill conditioned before any grading, and D^2 adds up to 64): check_edge's ``relev`` (1e-6 relative) has to FOLLOW from a
  backward error of r u sqrt(Sigma_ii Sigma_jj) (see _octaves_big).
  "w<Lg>-def" (129: rank 100, 161: rank 120) and "w<Lg>-def1" (rank 128 and 159): rank-deficient matrices on the same columns,
  safe for the rank test; after Sigma_0 their M' is exactly singular from column r on.
* ``warm_start`` restates the kernels in float64 (``blocked_cholesky``: 64-column panels -- diagonal block, rows below, trailing
  update --, pivots tested for > 0 as the device does); ``projector`` and ``projected`` form P = A_0^T diag(1 / s) A_0 and P Sigma P
  in the extended format.  X^T X = P Sigma P exactly in exact arithmetic, and a Jacobi preserves X^T X: the warm path factors
  P Sigma P.  Of bound_ij = 124 r u sqrt(Sigma_ii Sigma_jj) the start of the Jacobi has the 2 r u of the first line above
  (``warm_bound``); from A_0 = the reference rows of Sigma_0 rounded to float64 (|P - I|_2 = 1.3e-16 .. 1.4e-16) the restatement
  is at 0.058, 0.036, 0.037, 0.050, 0.036, 0.028 of it at 97, 128, 129, 130, 161, 193 columns.
* Teeth (tests/test_factor_exact.py).  Leaving the terms beyond the last whole chunk of 32 out of T makes M' lose positivity at
  97, 129, 130, 161 and 193 columns (first at columns 39, 52, 48, 79, 89: no warm rows at all, which the GPU test reads off the
  sweeps); leaving a last panel of fewer than 64 columns unfactored puts X^T X at 8e10, 5e5 and 3e11 times the share at 97, 129
  and 161.  At 128 columns neither corruption changes a bit.
* Sigma_def after Sigma_0: the restatement's first pivot that is not positive is at column 102 of 129 and 120 of 161 -- in the
  panel that starts at column 64, after G and Gt were overwritten.  Sigma_def1: its one (129) or two (161) pivots of rounding
  size come out positive in the restatement; on the device that is a matter of its own rounding.
"""
import functools
import math

import numpy as np

from tests.posterior_exact import LD, USE_DECIMAL, ext, f64, _sqrt

U = 2.0 ** -53
N_SWEEPS = 10
C_REC = 2 + 12 * N_SWEEPS + 2
PIVOT_TOL = 1e-14  # of the first pivot: where the device's pivoted Cholesky stops


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def graded(r, Lg, octaves, seed):
    """diag(2^-e_k) C: C integers in [-3, 3] (redrawn until a float64 SVD gives it full row rank), e = graded_exponents.
    Rank-deficient cases of three rows and more get a LEAD row: row 0 is 3 in one column and 0 elsewhere, the others start four
    octaves lower (see graded_exponents)."""
    assert 1 <= r <= Lg and 0 <= octaves <= 16
    rng = np.random.default_rng(1000003 * r + 1009 * Lg + seed)
    lead = 3 <= r < Lg and octaves >= 6
    while True:
        C = rng.integers(-3, 4, size=(r, Lg)).astype(np.float64)
        if lead:
            C[0] = 0.0
            C[0, Lg // 3] = 3.0
        if np.linalg.matrix_rank(C) == r and np.all(np.abs(C).sum(axis=1) > 0):
            break
    return C * (2.0 ** -graded_exponents(r, octaves, lead))[:, None]


def graded_exponents(r, octaves, lead=False):
    """Spread evenly over 0 .. octaves; with a lead row e_0 = 0 and the others over 4 .. octaves.
    Why a lead row.  Where the factorisation of an exactly rank-deficient Sigma stops, the remaining diagonal is rounding: every
    pivot step subtracts products of the size of Sigma's entries from entries of that size, an error of u |Sigma_pi| that the step
    amplifies into 2 u |Sigma_pi| of the diagonal whatever the pivot's own size -- after r steps some sqrt(r) u max |Sigma|,
    0.05 to 0.3 of the stopping tolerance 1e-14 d_0 for dense rows at ANY number of octaves (measured with greedy_pivots).  The
    lead row makes one diagonal entry, the first pivot d_0 = 9 + ..., some thirty times the other entries of Sigma, and what is
    left that much smaller against the tolerance: ``rank_safe`` needs 0.05 of it."""
    if r < 2:
        return np.zeros(r, dtype=np.int64)
    if not lead:
        return np.round(np.arange(r) * (octaves / (r - 1))).astype(np.int64)
    return np.concatenate([[0], 4 + np.round(np.arange(r - 1) * ((octaves - 4) / (r - 2)))]).astype(np.int64)


def hadamard_matrix(n):
    """Sylvester's: n a power of two, entries +-1, H H^T = n I."""
    assert n >= 1 and n & (n - 1) == 0
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def hadamard(n, Lg, exps, first=1, spike=None):
    """Rows first, first + 1, ... of H_n in columns 0 .. n - 1 of Lg, row k scaled by 2^-exps[k]: eigenvalues n 4^-exps[k].
    spike: one more row, 2^spike in column n -- an eigenvalue 4^spike of its own, and the first pivot (the lead row of
    graded_exponents, for rows that stay orthogonal)."""
    exps = np.asarray(exps, dtype=np.int64)
    assert first + exps.size <= n <= Lg and exps.min() >= 0 and exps.max() <= 16
    B = np.zeros((exps.size + (spike is not None), Lg))
    B[:exps.size, :n] = hadamard_matrix(n)[first:first + exps.size] * (2.0 ** -exps)[:, None]
    if spike is not None:
        assert n < Lg and all(4.0 ** spike != n * 4.0 ** -e for e in exps)
        B[-1, n] = 2.0 ** spike
    return B


def diagonal(Lg, cols, exps, mult):
    """Row k: mult[k] 2^-exps[k] in column cols[k]."""
    B = np.zeros((len(cols), Lg))
    for k, (c, e, m) in enumerate(zip(cols, exps, mult)):
        B[k, c] = m * 2.0 ** -e
    return B


def pair(coupling):
    """Two nearly equal diagonal entries and their coupling in columns 0, 1 (and 2), three separated directions in columns 3-7."""
    B = np.zeros((5, 8))
    if coupling == "small":  # Sigma_00 = 1 + 2^-50, Sigma_11 = (1 + 2^-10)^2 + 2^-50, Sigma_01 = 2^-50
        B[0, [0, 2]] = 1.0, 2.0 ** -25
        B[1, [1, 2]] = 1.0 + 2.0 ** -10, 2.0 ** -25
    else:  # Sigma_00 = 1 + 2^-6, Sigma_11 = 2^-6 + (1 + 2^-20)^2, Sigma_01 = 2^-2 + 2^-23
        B[0, [0, 1]] = 1.0, 0.125
        B[1, [0, 1]] = 0.125, 1.0 + 2.0 ** -20
    B[2, 3:8] = [3, -1, 2, 0, 1]
    B[3, 3:8] = np.array([1, 3, 0, -2, 0]) / 8.0
    B[4, 3:8] = np.array([0, 0, 1, 0, -2]) / 64.0
    return B


def _exps_groups():
    """Groups of 2, 3 and 8 equal exponents between separated ones: 17 rows."""
    return [0, 1, 1, 2, 3, 3, 3, 4] + [5] * 8 + [6]


# name -> (builder, kind); kind "graded" cases must have 90 % isolated rows, the others hold exact degeneracies or are tiny
_TABLE = {}


def _case(name, kind, fn):
    assert name not in _TABLE
    _TABLE[name] = (kind, fn)


LDS_CAPS = (40, 42, 44, 82, 84, 88, 90, 96)


def lds_ranks(cap):
    """The exact ranks of the four edges of a capacity's batch: 1, an odd rank, cap - 1, cap."""
    odd = cap // 2 + (1 if (cap // 2) % 2 == 0 else 0)
    return (1, odd, cap - 1, cap)


def _octaves_for(r):
    """Octaves of a graded case of rank r: 16 where the rows stay isolated, fewer as |bound|_F grows with r."""
    return 16 if r <= 48 else 14 if r <= 100 else 12


def _octaves_big(r):
    """Any-rank cases, whose eigenvalues are asserted to 1e-6 RELATIVE: a factorisation of Sigma with a backward error of
    r u sqrt(Sigma_ii Sigma_jj) moves an eigenvalue s_k by about r u s_0 (these diagonals are even), r u 4^octaves relative to the
    smallest: 2e-7 at twelve octaves and r = 100.  At fourteen the claim does not follow (3e-6), whatever the solver."""
    return min(_octaves_for(r), 12)


for _cap in LDS_CAPS:
    for _r in lds_ranks(_cap):
        if "g100-r%d" % _r not in _TABLE:
            _case("g100-r%d" % _r, "graded", functools.partial(graded, _r, 100, _octaves_for(_r), 1))
for _Lg in (4, 7, 33, 64, 65):
    _case("g%d-full" % _Lg, "graded", functools.partial(graded, _Lg, _Lg, min(_octaves_for(_Lg), 8), 2))
_case("g513-r31", "graded", functools.partial(graded, 31, 513, 12, 3))
_case("g1030-r20", "graded", functools.partial(graded, 20, 1030, 16, 4))
_case("g100-r17-oct16", "graded", functools.partial(graded, 17, 100, 16, 5))
_case("had32-equal", "degenerate", functools.partial(hadamard, 32, 32, [0] * 32, 0))
_case("had32-groups", "degenerate", functools.partial(hadamard, 32, 100, _exps_groups(), 1, 3))
_case("diag33", "degenerate", functools.partial(diagonal, 33, [5, 0, 32, 17, 9, 10, 31, 2, 20, 21], [0, 0, 1, 2, 2, 4, 7, 7, 7, 16],
                                                [3, 3, 1, 3, 3, 1, 2, 2, 2, 1]))
_case("pair-small", "small", functools.partial(pair, "small"))
_case("pair-large", "small", functools.partial(pair, "large"))
# mixed batch (Lg, cap, rank)
MIXED = ((7, 7, 7), (97, 90, 41), (64, 40, 1))
_case("g97-r41", "graded", functools.partial(graded, 41, 97, 12, 6))
_case("g64-r1", "graded", functools.partial(graded, 1, 64, 0, 6))
# any-rank path (capacity = Lg > 96)
BIG = ((97, 97), (100, 41), (130, 104), (130, 105), (200, 129), (200, 136))
for _Lg, _r in BIG:
    _case("b%d-r%d" % (_Lg, _r), "graded", functools.partial(graded, _r, _Lg, _octaves_big(_r), 7))
_case("bhad128-r105", "degenerate", functools.partial(hadamard, 128, 130, [0, 1, 1, 2, 2, 2] + [3] * 8 + [4 + (k // 15) for k in range(90)], 1, 4))
# capacity errors: rank cap + 1 with the last eigenvalue near 1e-6 of the largest (4^-10)
CAP_ERR = 40
_case("g100-r41-over", "graded", lambda: np.vstack([graded(40, 100, 4, 8), graded(1, 100, 0, 9) * 2.0 ** -10]))

# warm start of the any-rank path (see "Warm start" in the module docstring): width -> (octaves of B_0, rows D scales down)
WARM = {97: (6, 5), 128: (3, 40), 129: (5, 5), 130: (4, 40), 161: (3, 40), 193: (4, 5)}
WARM_WIDTHS = (97, 128, 129, 161, 193)
WARM_DEF = {129: 100, 161: 120}  # width -> exact rank of Sigma_def: M' loses positivity in the panel at column 64
WARM_DEF1 = {129: 128, 161: 159}  # ... of Sigma_def1: one or two pivots of rounding size, which the float64 restatement ACCEPTS


def warm_scales(Lg):
    """The diagonal of D: ones, and 2^-1 / 2^-3 alternately on WARM[Lg][1] rows drawn without replacement."""
    rng = np.random.default_rng(7919 * Lg + 11)
    d = np.ones(Lg)
    rows = np.sort(rng.choice(Lg, size=WARM[Lg][1], replace=False))
    d[rows[0::2]], d[rows[1::2]] = 0.5, 0.125
    return d


def warm_start_rows(Lg):
    return graded(Lg, Lg, WARM[Lg][0], 10)


for _Lg in WARM:
    _case("w%d-0" % _Lg, "graded", functools.partial(warm_start_rows, _Lg))
    _case("w%d-1" % _Lg, "graded", lambda _Lg=_Lg: warm_scales(_Lg)[:, None] * warm_start_rows(_Lg))
for _Lg, _r in WARM_DEF.items():
    _case("w%d-def" % _Lg, "graded", functools.partial(graded, _r, _Lg, _octaves_big(_r), 11))
for _Lg, _r in WARM_DEF1.items():
    _case("w%d-def1" % _Lg, "graded", functools.partial(graded, _r, _Lg, _octaves_big(_r), 11))

CASES = tuple(_TABLE)


def kind_of(name):
    return _TABLE[name][0]


# ---- extended-precision pieces ---------------------------------------------------------------------------------------------------

def sigma_of(B):
    """B^T B as float64, asserted exact: formed in the extended format, rounded, compared."""
    Bx = ext(B)
    Sx = Bx.T @ Bx
    S = f64(Sx)
    assert np.all(ext(S) == Sx), "Sigma is not exactly representable"
    assert np.array_equal(S, S.T)
    return S


def _rr_pairs(m, rnd):
    """The m / 2 disjoint pairs of round rnd of the circle method among m players (m even)."""
    m1 = m - 1
    k = np.arange(1, m // 2)
    p = np.concatenate([[rnd], (rnd + k) % m1])
    q = np.concatenate([[m1], (rnd - k) % m1])
    return np.minimum(p, q), np.maximum(p, q)


def ref_factor(B, tol=1e-17, max_sweeps=60, use_decimal=None):
    """(F, s, sweeps): rows sqrt(s_k) v_k of B^T B in the extended format, by descending s_k with the sign convention
    sum_j F[k, j] / (j + 1) >= 0, and s_k = |F_k|^2."""
    X = np.array(ext(B, use_decimal))
    r, Lg = X.shape
    dec = X.dtype == object
    one, zero = ext(1.0, dec), ext(0.0, dec)
    tolx = ext(tol, dec)
    m = r + (r & 1)
    sweeps = 0
    for sweep in range(max_sweeps):
        rotated = False
        for rnd in range(m - 1 if m > 1 else 0):
            p, q = _rr_pairs(m, rnd)
            keep = q < r
            p, q = p[keep], q[keep]
            x, y = X[p], X[q]
            a, b, g = (x * x).sum(axis=1), (y * y).sum(axis=1), (x * y).sum(axis=1)
            on = (g * g) > (tolx * tolx) * (a * b)
            if not np.any(on):
                continue
            rotated = True
            p, q, x, y, a, b, g = p[on], q[on], x[on], y[on], a[on], b[on], g[on]
            zeta = (b - a) / (g + g)
            sgn = np.where(zeta >= zero, one, -one)
            t = sgn / (abs(zeta) + _sqrt(one + zeta * zeta))
            c = one / _sqrt(one + t * t)
            s = c * t
            X[p] = c[:, None] * x - s[:, None] * y
            X[q] = s[:, None] * x + c[:, None] * y
        if not rotated:
            break
        sweeps += 1
    else:
        raise RuntimeError("ref_factor: no convergence in %d sweeps" % max_sweeps)
    s = (X * X).sum(axis=1)
    order = np.argsort(-f64(s), kind="stable")
    # (float64 keys order equal values by index; values a rounding apart in the extended format need no finer order)
    X, s = X[order], s[order]
    wts = one / ext(np.arange(1, Lg + 1, dtype=np.float64), dec)
    flip = (X * wts[None, :]).sum(axis=1) < zero
    X[flip] = -X[flip]
    return X, s, sweeps


@functools.lru_cache(maxsize=None)
def sigma(name):
    """(B, Sigma) of a case of the table, without its reference factor; computed once, not to be changed."""
    B = _TABLE[name][1]()
    S = sigma_of(B)
    for a in (B, S):
        a.setflags(write=False)
    return B, S


@functools.lru_cache(maxsize=None)
def case(name):
    """(B, Sigma, F, s) of a case of the table; computed once, not to be changed."""
    B, S = sigma(name)
    F, s, _ = ref_factor(B)
    return B, S, F, s


# ---- the warm start, restated ----------------------------------------------------------------------------------------------------

WARM_PANEL = 64  # columns of a panel of the blocked Cholesky
WARM_CHUNK = 32  # terms of a product that go through LDS together


def blocked_cholesky(M, skip_partial_panel=False):
    """Lower Cholesky factor of M (its lower triangle is read) in float64 by panels of WARM_PANEL columns -- diagonal block, the
    rows below it, the trailing update --, the order of the device's k_ojw_chol_*: (L, k) with k the first column whose pivot is
    not positive (L is then unfinished), or None.  skip_partial_panel: a corruption for the tests -- a last panel of fewer than
    WARM_PANEL columns is left as the trailing updates made it."""
    n = M.shape[0]
    K = np.tril(M).astype(np.float64)
    for k0 in range(0, n, WARM_PANEL):
        nb = min(WARM_PANEL, n - k0)
        if skip_partial_panel and nb < WARM_PANEL:
            break
        D = K[k0:k0 + nb, k0:k0 + nb]
        for c in range(nb):
            piv = D[c, c]
            if not piv > 0.0:
                return K, k0 + c
            f = D[c + 1:, c] / piv
            D[c + 1:, c + 1:] -= np.tril(np.outer(f, D[c + 1:, c]))
        d = np.sqrt(np.diag(D).copy())
        D[:] = np.tril(D / d[None, :])
        np.fill_diagonal(D, d)
        if k0 + nb < n:
            Lkk = D
            X = K[k0 + nb:, k0:k0 + nb]
            for c in range(nb):  # X Lkk^T = A by columns
                X[:, c] /= Lkk[c, c]
                X[:, c + 1:] -= np.outer(X[:, c], Lkk[c + 1:, c])
            K[k0 + nb:, k0 + nb:] -= np.tril(X @ X.T)
    return K, None


def warm_start(A0, S, drop_partial_chunk=False, skip_partial_panel=False):
    """The warm start of the any-rank factor in float64 from the previous rows A0 (Lg x Lg): 1 / s_k from the rows' float64
    squared norms, T = A0 Sigma, M' = T A0^T (lower), L' = chol(M'), X = (diag(1 / s) L')^T A0.  Returns (X, k): k the first
    column of M' whose pivot is not positive (X is then None: the device falls back to the pivoted Cholesky), else None.
    drop_partial_chunk: a corruption for the tests -- the terms of T beyond the last whole chunk of WARM_CHUNK are left out."""
    n = A0.shape[0]
    assert A0.shape == S.shape == (n, n)
    s = (A0 * A0).sum(axis=1)
    inv = np.where(s > 0.0, 1.0 / np.where(s > 0.0, s, 1.0), 0.0)
    kk = (n // WARM_CHUNK) * WARM_CHUNK if drop_partial_chunk else n
    T = A0[:, :kk] @ S[:kk, :]
    M = T @ A0.T
    L, bad = blocked_cholesky(M, skip_partial_panel)
    if bad is not None:
        return None, bad
    return (inv[:, None] * L).T @ A0, None


def projector(A):
    """P = A^T diag(1 / |A_k|^2) A of the float64 rows A, in the extended format: the identity where the rows are orthogonal and
    span everything."""
    Ax = ext(A)
    nrm2 = (Ax * Ax).sum(axis=1)
    return (Ax / nrm2[:, None]).T @ Ax


def projected(P, S):
    """P Sigma P in the extended format."""
    return P @ ext(S) @ P


def projector_defect(P):
    """|P - I|_2 (the difference formed in the extended format)."""
    n = P.shape[0]
    return float(np.linalg.norm(f64(P - ext(np.eye(n))), 2))


def warm_bound(S, r):
    """The share of bound_matrix that belongs to the start of the Jacobi: 2 r u sqrt(Sigma_ii Sigma_jj)."""
    d = np.diag(S)
    return 2 * r * U * np.sqrt(np.outer(d, d))


# ---- the rank test, restated ---------------------------------------------------------------------------------------------------------

def greedy_pivots(S, cap=None, tol_rel=PIVOT_TOL):
    """Greedy pivoted Cholesky in float64 (ties: smallest index) until the largest remaining diagonal entry is at most tol_rel
    of the first pivot or cap pivots are taken: (pivot values, largest remaining diagonal entry, tol)."""
    n = S.shape[0]
    cap = n if cap is None else min(cap, n)
    d = np.diag(S).copy()
    G = np.zeros((cap, n))
    used = np.zeros(n, dtype=bool)
    piv, tol = [], 0.0
    for k in range(cap):
        p = int(np.argmax(np.where(used, -1.0, d)))
        if k == 0:
            tol = d[p] * tol_rel
        if not (d[p] > tol and d[p] > 0.0):
            break
        piv.append(d[p])
        G[k] = np.where(used, 0.0, (S[p] - G[:k, p] @ G[:k]) / math.sqrt(d[p]))
        used[p] = True
        d = np.maximum(d - G[k] * G[k], 0.0)
    rem = float(np.where(used, 0.0, d).max()) if n else 0.0
    return np.array(piv), rem, tol


def rank_safe(S, r):
    """The condition under "Rank test" above."""
    piv, rem, tol = greedy_pivots(S)
    return piv.size == r and bool(np.all(piv > 100.0 * tol)) and rem < 0.05 * tol, (piv.size, piv.min() / tol if piv.size else 0.0, rem / tol if tol else 0.0)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------

def bound_matrix(S, r):
    d = np.diag(S)
    return C_REC * r * U * np.sqrt(np.outer(d, d))


def bound_fro(S, r):
    return C_REC * r * U * float(np.trace(S))


def iso_gap(S, r):
    """Rows whose eigenvalue is at least this far from every other one are compared one by one."""
    return 20.0 * bound_fro(S, r)


def gaps(s, full_rank):
    """Distance of every s_k (descending) to the nearest other eigenvalue; 0 counts as one unless full_rank."""
    s = np.asarray(s, dtype=np.float64)
    lo = np.append(s[:-1] - s[1:], np.inf if full_rank else s[-1])
    hi = np.append(np.inf, s[:-1] - s[1:])
    return np.minimum(lo, hi)


def clusters(s, rel_gap, abs_gap=0.0):
    """Groups [k0, k1) of the descending eigenvalues s: neighbours belong together when they are closer than rel_gap of the
    larger one (or than abs_gap)."""
    s = np.asarray(s, dtype=np.float64)
    out, k0 = [], 0
    for k in range(1, s.size + 1):
        if k == s.size or s[k - 1] - s[k] > max(rel_gap * s[k - 1], abs_gap):
            out.append((k0, k))
            k0 = k
    return out


def groups_of(S, s, r):
    """The clusters the checks use: by iso_gap; a last eigenvalue that close to 0 (r < Lg) stays a group of its own."""
    return clusters(s, 0.0, iso_gap(S, r))


def isolated_fraction(S, s):
    r = len(s)
    g = gaps(f64(s), r == S.shape[0])
    single = [k0 for k0, k1 in groups_of(S, f64(s), r) if k1 - k0 == 1 and g[k0] >= iso_gap(S, r)]
    return len(single) / r
