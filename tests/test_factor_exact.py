"""The reference and the case table of tests/factor_exact.py, on the host: the extended-precision one-sided Jacobi against mpmath
at 40 digits and against LAPACK, the table's conditions -- exact representability, safety for the device's rank test, isolated
rows --, the Hadamard cases' eigenvectors in integer arithmetic, and the float64 restatement of the any-rank path's warm start
(factor_exact.warm_start) against P Sigma P in the extended format, with the two corruptions that only ragged widths catch.
No GPU, no kernel code."""
import functools
import math

import numpy as np
import pytest

from tests import factor_exact as fx

SMALL = ("g4-full", "g7-full", "pair-small", "pair-large")
GRADED = tuple(n for n in fx.CASES if fx.kind_of(n) in ("graded", "small"))
HADAMARD = {"had32-equal": (32, 32, [0] * 32, 0, None), "had32-groups": (32, 100, fx._exps_groups(), 1, 3)}


def _mp(mp, x):
    """The extended number x as an mpf, exactly: a long double is the sum of two float64 numbers."""
    if fx.USE_DECIMAL:
        return mp.mpf(str(x))
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - fx.LD(hi)))


@pytest.mark.parametrize("name", SMALL)
def test_reference_matches_mpmath_at_40_digits(name):
    """Eigenvalues to 16 eps of long double (2^-63) relative to the largest -- and, these matrices being small and graded by
    rows, relative to each one to 1e-15 --, rows to the same against sqrt(s_k) v_k of mpmath's symmetric eigensolver."""
    mp = pytest.importorskip("mpmath")
    B, S, F, s = fx.case(name)
    r, Lg = B.shape
    assert Lg <= 16
    with mp.workdps(40):
        M = mp.matrix(Lg, Lg)
        Bm = [[mp.mpf(float(B[k, j])) for j in range(Lg)] for k in range(r)]
        for i in range(Lg):
            for j in range(Lg):
                M[i, j] = mp.fsum(Bm[k][i] * Bm[k][j] for k in range(r))
                assert M[i, j] == mp.mpf(float(S[i, j]))
        ev, V = mp.eigsy(M)
        order = sorted(range(Lg), key=lambda k: -ev[k])[:r]
        eps = 2.0 ** -63 if not fx.USE_DECIMAL else 1e-38
        for k, o in enumerate(order):
            sk = _mp(mp, s[k])
            assert abs(sk - ev[o]) <= 16 * eps * ev[order[0]], (name, k)
            assert abs(sk - ev[o]) <= 1e-15 * ev[o], (name, k)
            row = [mp.sqrt(ev[o]) * V[j, o] for j in range(Lg)]
            sign = 1 if mp.fsum(row[j] / (j + 1) for j in range(Lg)) >= 0 else -1
            gap = min(abs(ev[o] - ev[q]) for q in range(Lg) if q != o)
            err = max(abs(_mp(mp, F[k, j]) - sign * row[j]) for j in range(Lg))
            assert err <= 64 * eps * mp.sqrt(ev[o]) * ev[order[0]] / gap, (name, k, float(err))


def test_reference_in_decimal_agrees_with_long_double():
    B = fx.case("g4-full")[0]
    F, s, _ = fx.ref_factor(B)
    Fd, sd, _ = fx.ref_factor(B, use_decimal=True)
    np.testing.assert_allclose(fx.f64(sd), fx.f64(s), rtol=4 * fx.U)
    np.testing.assert_allclose(fx.f64(Fd), fx.f64(F), rtol=0, atol=1e-15 * float(np.abs(fx.f64(F)).max()))


@pytest.mark.parametrize("name", fx.CASES)
def test_reference_matches_lapack_and_reconstructs(name):
    """eigvalsh is backward stable: its eigenvalues are within Lg u s_0 of the exact ones.  And F^T F = Sigma, rows orthogonal."""
    B, S, F, s = fx.case(name)
    r, Lg = B.shape
    w = np.linalg.eigvalsh(S)[::-1]
    sf = fx.f64(s)
    assert np.all(np.diff(sf) <= 0) and sf[-1] > 0
    assert np.abs(w[:r] - sf).max() <= Lg * fx.U * sf[0], name
    assert np.abs(w[r:]).max(initial=0.0) <= Lg * fx.U * sf[0], name
    eps = 2.0 ** -63
    R = fx.f64(abs(F.T @ F - fx.ext(S)))
    d = np.sqrt(np.diag(S))
    assert np.all(R <= 8 * Lg * eps * np.outer(d, d) + 0.0), name
    Gm = fx.f64(F @ F.T)
    nrm = np.sqrt(np.diag(Gm))
    off = np.abs(Gm - np.diag(np.diag(Gm)))
    assert np.all(off <= 4e-17 * np.outer(nrm, nrm)), (name, (off / np.outer(nrm, nrm)).max())  # (1e-17 when the pair was last visited)
    assert np.all(fx.f64((F / fx.ext(np.arange(1, Lg + 1.0))[None, :]).sum(axis=1)) >= 0)


@pytest.mark.parametrize("name", fx.CASES)
def test_case_is_exact_and_safe_for_the_rank_test(name):
    B, S, F, s = fx.case(name)  # (sigma_of has asserted that Sigma is exact)
    r, Lg = B.shape
    assert r <= 193 and (fx.kind_of(name) == "small" or np.abs(np.log2(np.abs(B[B != 0]))).max() <= 16 + 4)
    if fx.kind_of(name) == "graded":  # integers in [-3, 3] times one power of two per row
        for row in B:
            assert any(np.all(row * 2.0 ** e == np.round(row * 2.0 ** e)) and np.abs(row * 2.0 ** e).max() <= 3 for e in range(17))
    if name == "g100-r41-over":
        piv, rem, tol = fx.greedy_pivots(S, fx.CAP_ERR)
        assert piv.size == fx.CAP_ERR and rem > 100 * 1e4 * tol  # (the device reports the capacity above 1e4 tol)
        assert 1e-7 < fx.f64(s)[-1] / fx.f64(s)[0] < 1e-4
        return
    ok, info = fx.rank_safe(S, r)
    assert ok, (name, info)


@pytest.mark.parametrize("name", GRADED)
def test_isolated_rows_are_not_skipped(name):
    B, S, F, s = fx.case(name)
    assert fx.isolated_fraction(S, s) >= 0.9, name


def test_degenerate_cases_have_the_groups_they_state():
    for name, sizes in [("had32-equal", [32]), ("had32-groups", [1, 1, 2, 1, 3, 1, 8, 1]), ("diag33", [2, 2, 1, 1, 3, 1]),
                        ("bhad128-r105", [1, 1, 2, 3, 8] + [15] * 6)]:
        B, S, F, s = fx.case(name)
        got = [k1 - k0 for k0, k1 in fx.clusters(fx.f64(s), 1e-12)]
        assert got == sizes, (name, got)
        assert [k1 - k0 for k0, k1 in fx.groups_of(S, fx.f64(s), B.shape[0])] == sizes, name
        # rows of B are mutually orthogonal: the reference has nothing to rotate and returns them, reordered and signed
        assert fx.ref_factor(B)[2] == 0
        assert sorted(map(tuple, np.abs(fx.f64(F)))) == sorted(map(tuple, np.abs(B)))


@pytest.mark.parametrize("name", sorted(HADAMARD))
def test_hadamard_eigenvectors_in_integer_arithmetic(name):
    """Sigma v = s v with v = h_k (integers), Sigma scaled to integers by 4^emax: exact in int64."""
    n, Lg, exps, first, spike = HADAMARD[name]
    B, S, F, s = fx.case(name)
    emax = max(exps)
    Si = S * 4.0 ** emax
    assert np.all(Si == np.round(Si)) and np.abs(Si).max() < 2 ** 40
    Si = Si.astype(np.int64)
    H = fx.hadamard_matrix(n).astype(np.int64)
    seen = []
    for k, e in enumerate(exps):
        v = np.zeros(Lg, dtype=np.int64)
        v[:n] = H[first + k]
        lam = n * 4 ** (emax - e)
        assert np.array_equal(Si @ v, lam * v)
        seen.append(lam / 4.0 ** emax)
    if spike is not None:
        v = np.zeros(Lg, dtype=np.int64)
        v[n] = 1
        assert np.array_equal(Si @ v, 4 ** (spike + emax) * v)
        seen.append(4.0 ** spike)
    assert np.array_equal(np.sort(seen)[::-1], fx.f64(s))


def test_clusters_and_gaps():
    s = np.array([8.0, 4.0, 4.0, 1.0, 1.0 - 1e-9, 0.25])
    assert fx.clusters(s, 1e-12) == [(0, 1), (1, 3), (3, 4), (4, 5), (5, 6)]
    assert fx.clusters(s, 1e-6) == [(0, 1), (1, 3), (3, 5), (5, 6)]
    assert fx.clusters(s, 0.0, 0.8) == [(0, 1), (1, 3), (3, 6)]
    np.testing.assert_allclose(fx.gaps(s, False), [4.0, 0.0, 0.0, 1e-9, 1e-9, 0.25], atol=1e-15)
    assert fx.gaps(s, True)[-1] == 0.75 - 1e-9
    assert fx.C_REC * 96 * fx.U <= 1e-9 / 100 and fx.C_REC * 136 * fx.U <= 2e-12


# ---- the warm start of the any-rank path, restated (factor_exact.warm_start) --------------------------------------------------------

WARM_RAGGED = (97, 129, 161)


@functools.lru_cache(maxsize=None)
def _warm_host(Lg):
    """(A_0, P Sigma_1 P, |P - I|_2): A_0 the reference rows of Sigma_0 rounded to float64, P their projector."""
    A0 = fx.f64(fx.case("w%d-0" % Lg)[2])
    P = fx.projector(A0)
    return A0, fx.projected(P, fx.sigma("w%d-1" % Lg)[1]), fx.projector_defect(P)


def _warm_fraction(Lg, **corruption):
    """max |X^T X - P Sigma_1 P|_ij / (2 r u sqrt(Sigma_ii Sigma_jj)) of the restatement; inf where its Cholesky meets a pivot
    that is not positive -- the device then starts cold, which the GPU tests' sweep counts notice."""
    A0, PSP, _ = _warm_host(Lg)
    S1 = fx.sigma("w%d-1" % Lg)[1]
    X, bad = fx.warm_start(A0, S1, **corruption)
    if X is None:
        return math.inf
    Xx = fx.ext(X)
    return float((fx.f64(abs(Xx.T @ Xx - PSP)) / fx.warm_bound(S1, Lg)).max())


@pytest.mark.parametrize("Lg", sorted(fx.WARM))
def test_warm_step_is_a_downdate_of_known_rank(Lg):
    """Sigma_0 - Sigma_1 = B_0^T (I - D^2) B_0: positive semidefinite of rank = the rows D scales (B_0 has full rank), D's
    entries 1, 2^-1 and 2^-3; and both matrices are conditioned so that an eigenvalue's 1e-6 follows from a backward error of
    r u sqrt(Sigma_ii Sigma_jj) (factor_exact._octaves_big)."""
    B0, S0 = fx.sigma("w%d-0" % Lg)
    B1, S1 = fx.sigma("w%d-1" % Lg)
    d = fx.warm_scales(Lg)
    assert B0.shape == (Lg, Lg) and np.array_equal(B1, d[:, None] * B0) and set(d) == {1.0, 0.5, 0.125}
    assert int((d != 1).sum()) == fx.WARM[Lg][1] and np.linalg.matrix_rank(B0) == Lg
    E = np.sqrt(1 - d * d)[:, None] * B0
    np.testing.assert_allclose(E.T @ E, S0 - S1, rtol=0, atol=8 * Lg * fx.U * np.abs(S0).max())
    for name in ("w%d-0" % Lg, "w%d-1" % Lg):
        s = fx.f64(fx.case(name)[3])
        assert Lg * fx.U * s[0] / s[-1] <= 1e-6, (name, s[0] / s[-1])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 161])
def test_blocked_cholesky_is_a_cholesky(n):
    """Higham, Thm 10.3: |L L^T - M|_ij <= (n + 1) u sqrt(M_ii M_jj); and the first pivot that is not positive is reported."""
    rng = np.random.default_rng(n)
    G = rng.integers(-3, 4, size=(n + 5, n)).astype(np.float64)
    M = G.T @ G
    L, bad = fx.blocked_cholesky(M)
    assert bad is None and np.array_equal(L, np.tril(L))
    d = np.sqrt(np.diag(M))
    assert np.all(np.abs(fx.f64(fx.ext(L) @ fx.ext(L).T - fx.ext(M))) <= (n + 1) * fx.U * np.outer(d, d))
    if n >= 65:
        M2 = M.copy()
        M2[n - 1, n - 1] = -1.0
        assert fx.blocked_cholesky(M2)[1] == n - 1


@pytest.mark.parametrize("Lg", sorted(fx.WARM))
def test_warm_restatement_meets_the_start_share_of_the_bound(Lg):
    """The condition the GPU test puts to the kernels, 124 r u sqrt(Sigma_ii Sigma_jj) against P Sigma_1 P, leaves 2 r u of it
    to the start of the Jacobi: the float64 restatement stays within that (0.03 .. 0.06 of it, printed)."""
    A0, PSP, defect = _warm_host(Lg)
    assert defect <= 8 * fx.U, defect  # (rows orthogonal to 1e-17, rounded to float64)
    frac = _warm_fraction(Lg)
    print("warm restatement %d columns: %.3g of 2 r u sqrt(Sigma_ii Sigma_jj), |P - I|_2 = %.2e" % (Lg, frac, defect))
    assert frac <= 1.0, (Lg, frac)


@pytest.mark.parametrize("Lg", WARM_RAGGED)
def test_warm_condition_catches_a_dropped_partial_chunk_and_an_empty_partial_panel(Lg):
    assert not _warm_fraction(Lg, drop_partial_chunk=True) <= 1.0
    assert not _warm_fraction(Lg, skip_partial_panel=True) <= 1.0


def test_warm_corruptions_pass_unnoticed_at_the_aligned_width():
    """128 columns have no partial chunk of 32 and no partial panel of 64: why aligned widths prove nothing about either."""
    want = _warm_fraction(128)
    assert _warm_fraction(128, drop_partial_chunk=True) == want <= 1.0
    assert _warm_fraction(128, skip_partial_panel=True) == want


@pytest.mark.parametrize("Lg", sorted(fx.WARM_DEF))
def test_rank_deficient_step_loses_positivity_in_a_later_panel(Lg):
    """M' = A_0 Sigma_def A_0^T has exact rank r >= 64: its Schur complement after r pivots is rounding, and the restatement
    meets a pivot that is not positive in the panel that starts at column 64 -- after G and Gt have been overwritten."""
    r = fx.WARM_DEF[Lg]
    assert fx.sigma("w%d-def" % Lg)[0].shape == (r, Lg) and 64 <= r < 128
    X, bad = fx.warm_start(_warm_host(Lg)[0], fx.sigma("w%d-def" % Lg)[1])
    assert X is None and r <= bad < 128, bad


@pytest.mark.parametrize("Lg", sorted(fx.WARM_DEF1))
def test_nearly_full_rank_step_has_its_rounding_pivots_accepted(Lg):
    """Rank Lg - 1 and Lg - 2: the last one or two pivots of M' are rounding, and in the restatement they come out positive --
    the warm start is then accepted with rank Lg and the next one divides by squared norms of rounding size.  (The sign of a
    pivot of rounding size is the device's own; the GPU test's contract covers both outcomes.)"""
    r = fx.WARM_DEF1[Lg]
    assert fx.sigma("w%d-def1" % Lg)[0].shape == (r, Lg) and Lg - 2 <= r < Lg
    X, bad = fx.warm_start(_warm_host(Lg)[0], fx.sigma("w%d-def1" % Lg)[1])
    assert bad is None and np.all(np.isfinite(X))
