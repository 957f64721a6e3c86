"""The any-rank factor's warm start (csrc/gpet_eig.hip: k_ojw_begin, k_ojw_gemm<0|1|2>, k_ojw_chol_diag / _trsm / _syrk,
k_ojw_commit) on injected covariances at the edges of its 64 x 64 tiles, 32-term chunks and 64-column panels.  The inputs, the
float64 restatement of the warm start and the extended-precision projector are tests/factor_exact.py's ("w" cases, warm_start,
projector), pinned on the host by tests/test_factor_exact.py; the conditions are tests/test_gpu_factor_injected.py's check_edge.

How the kernels are reached without a trace.  A batch of capacity = Lg > 96 gets Sigma_0 = B_0^T B_0 (full rank) through
GPET_BUF_COV and gpet_gp_factor at iteration 0: the cold path, whose k_oj_rows leaves the rows A_0 in slot 0 of the ring with
tag 1.  GPET_BUF_FACTOR is read back: the very rows the warm start will read.  The scalars are then written back with iter = 1,
Sigma_1 = (D B_0)^T (D B_0) -- Sigma_0 less a positive-semidefinite matrix of rank 5 or 40 -- goes to GPET_BUF_COV, and the second
gpet_gp_factor runs k_ojw_*: 1 / |A_0k|^2, T = A_0 Sigma_1, M' = T A_0^T, its blocked Cholesky factor L', X = (diag(1 / s) L')^T A_0,
and the one-sided Jacobi on X's rows.  A call at iter = 1 writes slot 1; slot 0 keeps A_0, so several matrices can be factored
from the same rows.  Widths: 97 (panels of 64 + 33, a chunk of one term), 128 (aligned: the control), 129 (a panel of ONE row),
161 (two and a half tiles), 193 (three panels and one row); 130 in the mixed batches.

Paths.  Defaults: k_pcb_init -> k_ojw_* -> k_pcb_block (no-ops) -> k_oj_persist, staged.  Twins: oj_warm = 0 (cold: the same
launches as iteration 0), pcx_one_pivot = 1 (the plan has no warm start: k_pcx_step), oj_persist = 0 (k_oj_round launches),
oj_stage = 0 (operands from global memory).  That the warm kernels ran is read off the sweeps (scalars.lml): Sigma_0 factored
AGAIN at iter = 1 must need strictly fewer than the cold call on the same matrix, and exactly as many where the twin has no
warm start.  For Sigma_1 the count is printed, not asserted.

The one adjusted condition.  X^T X = A_0^T S^-1 (A_0 Sigma A_0^T) S^-1 A_0 = P Sigma P with P = A_0^T diag(1 / |A_0k|^2) A_0, and the
Jacobi that follows preserves X^T X whatever X is: the warm path factors P Sigma P, not Sigma.  P is the identity only as far as
A_0's rows are orthogonal, which the cold call promises to 1e-10 of their norms (check_edge's ``orth``), i.e. |P - I|_2 <= r 1e-10
(r pairs per row at most).  So ``rec`` compares A^T A with P Sigma_1 P -- P formed in the extended format from the rows read
back, the only quantity taken from the device -- under the unchanged bound_matrix of Sigma_1, and two more lines say how far
that is from Sigma_1:  |P - I|_2 <= r 1e-10  and  |P Sigma_1 P - Sigma_1|_ij <= 2 |P - I|_2 |Sigma_1|_2  (both printed).  Every other
condition of check_edge (weyl, evnorm, relev, orth, rows, clusters, sign) stays against Sigma_1's own reference.  Where an edge
starts cold -- a twin without warm start, a rank-deficient predecessor, a fallback -- ``rec`` is against Sigma_1 itself.

Mixed batches (one launch, widths 97, 161 and 130; once more as nine edges, pointers from the edge table): the grids of k_ojw_*
come from the widest edge, n is each edge's own.  Edge 1's Sigma_0 has rank 120 < 161: no rows are kept (tag 0), and it must
come out exactly as on a fresh batch of the same layout.

Three steps on one edge (129 and 161 columns): Sigma_0, then the rank-deficient Sigma_def at iter = 1, then Sigma_1 at iter = 2.
M' = A_0 Sigma_def A_0^T has exact rank r in 64 .. 127: the Cholesky's pivots from column r on are rounding.  Either one of them is
not positive -- the fallback to the pivoted Cholesky from a LATER panel (k0 = 64), after G and Gt were overwritten: rank r, and
the result must equal the cold factor of the same matrix bit for bit (test_natural_fallback_in_a_later_panel; the host
restatement meets its first such pivot at column 102 of 129 and 120 of 161) -- or all are accepted and the factor reports rank
Lg with Lg - r eigenvalues of rounding size, rows that k_oj_rows keeps for step 3.  Step 3 must then still factor Sigma_1.
Sigma_def1 (rank 128 of 129: the one-row panel's only pivot is rounding; rank 159 of 161) is there for that second outcome: the
host restatement accepts its one or two pivots of rounding size.  Which way the device goes is printed; the contract of step 2
is status OK, everything finite, eigenvalues non-increasing, ``rec`` within Sigma_def's bound_matrix (against Sigma_def after a
fallback, against P Sigma_def P else), rank r -- or rank Lg with every eigenvalue beyond the r-th at most |bound|_F.

Scaling: Sigma_0 and Sigma_1 times 4^+-20 must give, on the SECOND call, rows 2^+-20 times the unscaled ones bit for bit
(M' scales by 16^+-20: in range).

Out of scope: the carry across frames (ap_tag[2], GPET_IMAGES_NEXT_FRAME: reachable only through set_frame; the sequence tests
cover it) and widths above 512 columns (half-panel staging).

Measured on an MI355X (largest deviation as a fraction of its bound over all cases of a line; sweeps as the kernels report them):
  warm path (defaults, oj_persist = 0, oj_stage = 0, mixed batches, step 3 from kept rows)
      rec 0.015 (against P Sigma_1 P)  weyl 0.008  evnorm 0.017  relev 0.0005  orth 0.010  rows 0.002
      |P - I|_2 <= 2.0e-12 = 0.00016 of r 1e-10;  |P Sigma_1 P - Sigma_1|_ij <= 0.012 of 2 |P - I|_2 |Sigma_1|_2, i.e. under 5e-14 |Sigma_1|_2
  cold twins and cold edges (oj_warm = 0, pcx_one_pivot = 1, after a rank-deficient matrix or a fallback)
      rec 0.015 (against Sigma_1)      weyl 0.001  evnorm 0.022  relev 0.0005  orth 0.010  rows 0.0005
  sweeps  Sigma_0 cold 7 (97 columns), 8 (128, 129), 9 (161, 193); Sigma_0 again at iter 1: 1 at every width and warm twin, the cold
          count in the cold twins; Sigma_1 warm 6, 7, 6, 7, 5 against 7, 8, 8, 9, 9 cold; mixed batches 6 | 9 (cold edge) | 7
  scaling by 4^+-20 on the second call: rows and eigenvalues equal bit for bit at all five widths
What the first run found: nothing to fix.  Every condition held at every width with a factor 45 to spare; the restatement on
the host (0.03 .. 0.06 of the 2 r u share) and the kernels (0.015 of 124 r u) agree on the size of the start's error.
* Sigma_def (rank 100 of 129, 120 of 161) fell back from the panel at k0 = 64, Sigma_def1 at 161 columns (rank 159) from the one
  at k0 = 128: rank r, for Sigma_def the cold factor's bits, and step 3 then started cold (8 and 9 sweeps, as Sigma_0 cold).
* Sigma_def1 at 129 columns (rank 128) had its one pivot of rounding size ACCEPTED: rank 129 with a last eigenvalue of 1.4e-16
  (2e-6 of |bound|_F) after 8 sweeps, rec 0.013 against P Sigma_def1 P, and k_oj_rows kept the rows.  The chain that was feared -- the
  next warm start divides by that squared norm -- is harmless: the Jacobi orthogonalises rows RELATIVE to their norms, so the
  row of rounding size is a direction like any other, |P - I|_2 = 2.0e-12 for these rows, and step 3 met every condition (rec
  0.015, weyl 0.008, rows 0.002; 9 sweeps against 8 cold: such rows are no better a start than the pivoted Cholesky's).
  Only a row that is EXACTLY zero would lose its direction (k_ojw_begin's 1 / s = 0); no exact input produced one.
"""
import functools

import numpy as np
import pytest

from tests import factor_exact as fx
from tests.test_gpu_factor_injected import _frac, batch_of, check_edge, options

pytestmark = pytest.mark.gpu

TWINS = {"default": {}, "oj_warm0": {"oj_warm": 0}, "pcx_one_pivot": {"pcx_one_pivot": 1}, "oj_persist0": {"oj_persist": 0},
         "oj_stage0": {"oj_stage": 0}}
COLD_TWINS = ("oj_warm0", "pcx_one_pivot")
MIXED = ((97, "w97-0", "w97-1"), (161, "w161-def", "w161-1"), (130, "w130-0", "w130-1"))  # (width, first matrix, second matrix)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@functools.lru_cache(maxsize=64)
def _projection(rows, Lg, name):
    """(P Sigma P, |P - I|_2, max |P Sigma P - Sigma|_ij / (2 |P - I|_2 |Sigma|_2)) for the rows (bytes of an Lg x Lg float64
    array) and the case ``name``."""
    S = fx.sigma(name)[1]
    P = fx.projector(np.frombuffer(rows, dtype=np.float64).reshape(Lg, Lg))
    PSP = fx.projected(P, S)
    defect = fx.projector_defect(P)
    return PSP, defect, _frac(abs(PSP - fx.ext(S)), np.full(S.shape, 2 * defect * np.linalg.norm(S, 2)))


def start(amd, ctx, edges, opts=None, scale=1.0):
    """A batch of the edges [(Lg, case name)] under the process options opts, its first factor made (iteration 0: cold);
    returns (batch, sweeps per edge)."""
    L = amd._lib
    with options(L, opts or {}):
        b = batch_of(amd, ctx, [(fx.sigma(name)[1], Lg, Lg) for Lg, name in edges], scale=scale)
    try:
        b.factor()
        return b, [int(b.scalars(e).lml) for e in range(len(edges))]
    except BaseException:
        b.close()
        raise


def step(L, b, names, it, scale=1.0):
    """Every edge's scalars with iter = it, then Sigma of names[e] into GPET_BUF_COV, then gpet_gp_factor; returns the sweeps."""
    for e in range(len(names)):
        sc = b.scalars(e)
        assert sc.status == L.OK, (e, sc.status)
        sc.iter = it
        b.write_scalars(sc, e)
    for e, name in enumerate(names):
        b.write(L.BUF_COV, fx.sigma(name)[1] * scale, e)
    b.factor()
    return [int(b.scalars(e).lml) for e in range(len(names))]


def full_rows(L, b, e, Lg):
    sc = b.scalars(e)
    assert (sc.rank, sc.status) == (Lg, L.OK), (e, sc.rank, sc.status)
    return np.array(b.read(L.BUF_FACTOR, e))


def check_warm_edge(L, b, e, name, rows, what):
    """check_edge with ``rec`` against P Sigma P, P from ``rows`` (the previous factor as read back), and the two lines that tie
    P Sigma P to Sigma."""
    Lg = rows.shape[1]
    PSP, defect, frac = _projection(rows.tobytes(), Lg, name)
    print("PROJ %s: |P - I|_2 = %.3g (%.3g of r 1e-10)  max |P Sigma P - Sigma|_ij = %.3g of 2 |P - I|_2 |Sigma|_2" % (what, defect, defect / (Lg * 1e-10), frac))
    assert defect <= Lg * 1e-10, (what, defect)
    assert frac <= 1.0, (what, frac)
    return check_edge(L, b, e, name, "any", what, rec_target=PSP)


# ---- one edge per width, every twin ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("twin", sorted(TWINS))
@pytest.mark.parametrize("Lg", fx.WARM_WIDTHS)
def test_warm_start_at_tile_edges(amd, ctx, Lg, twin):
    L = amd._lib
    n0, n1 = "w%d-0" % Lg, "w%d-1" % Lg
    b, (cold,) = start(amd, ctx, [(Lg, n0)], TWINS[twin])
    try:
        A0 = full_rows(L, b, 0, Lg)
        (again,) = step(L, b, [n0], 1)
        full_rows(L, b, 0, Lg)
        (sweeps,) = step(L, b, [n1], 1)  # (the call before wrote slot 1 of the ring: slot 0 still holds A_0)
        what = "%d columns %s" % (Lg, twin)
        print("SWEEPS %s: Sigma_0 cold %d, Sigma_0 again at iter 1: %d, Sigma_1 at iter 1: %d" % (what, cold, again, sweeps))
        if twin in COLD_TWINS:
            assert again == cold, (what, cold, again)
            check_edge(L, b, 0, n1, "any", what)
        else:
            assert again < cold, (what, cold, again)
            check_warm_edge(L, b, 0, n1, A0, what)
    finally:
        b.close()


@pytest.mark.parametrize("Lg", fx.WARM_WIDTHS)
def test_scaling_by_powers_of_four_on_the_second_call(amd, ctx, Lg):
    L = amd._lib
    n0, n1 = "w%d-0" % Lg, "w%d-1" % Lg
    got = {}
    for k in (0, 20, -20):
        b, (cold,) = start(amd, ctx, [(Lg, n0)], scale=4.0 ** k)
        try:
            (sweeps,) = step(L, b, [n1], 1, scale=4.0 ** k)
            sc = b.scalars(0)
            got[k] = (sc.rank, sc.status, sweeps, b.read(L.BUF_FACTOR), b.read(L.BUF_EIGVALS), cold)
        finally:
            b.close()
    for k in (20, -20):
        assert got[k][:3] == got[0][:3] and got[0][:2] == (Lg, L.OK), (k, got[k][:3], got[0][:3])
        dA = np.abs(got[k][3] * 2.0 ** -k - got[0][3]).max() / np.abs(got[0][3]).max()
        dev = np.abs(got[k][4] * 4.0 ** -k - got[0][4]).max() / got[0][4][0]
        print("scaling %d columns 4^%d: rows differ by %.3g of the largest entry, eigenvalues by %.3g of the largest; sweeps %d (cold %d)"
              % (Lg, k, dA, dev, got[k][2], got[k][5]))
        assert np.array_equal(got[k][3] * 2.0 ** -k, got[0][3]), (Lg, k, dA)
        assert np.array_equal(got[k][4] * 4.0 ** -k, got[0][4]), (Lg, k, dev)


# ---- mixed batches -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("copies", [1, 3], ids=["three-edges", "nine-edges"])
def test_mixed_batch(amd, ctx, copies):
    L = amd._lib
    lay = MIXED * copies
    B = len(lay)
    fresh, cold1 = start(amd, ctx, [(Lg, n1) for Lg, _, n1 in lay])  # every edge's second matrix, cold
    try:
        want = [(fresh.scalars(e).rank, np.array(fresh.read(L.BUF_FACTOR, e)), np.array(fresh.read(L.BUF_EIGVALS, e))) for e in range(B)]
    finally:
        fresh.close()
    b, cold0 = start(amd, ctx, [(Lg, n0) for Lg, n0, _ in lay])
    try:
        rows0 = [np.array(b.read(L.BUF_FACTOR, e)) for e in range(B)]
        again = step(L, b, [n0 for _, n0, _ in lay], 1)
        sweeps = step(L, b, [n1 for _, _, n1 in lay], 1)
        print("SWEEPS mixed x%d: first matrices cold %s, again at iter 1 %s; second matrices cold %s, at iter 1 %s" % (copies, cold0, again, cold1, sweeps))
        for e, (Lg, n0, n1) in enumerate(lay):
            what = "mixed x%d edge %d (%d columns)" % (copies, e, Lg)
            if n0.endswith("-def"):  # no rows were kept: cold, exactly
                assert rows0[e].shape == (fx.sigma(n0)[0].shape[0], Lg) and again[e] == cold0[e], what
                sc = b.scalars(e)
                assert (sc.rank, sc.status) == (want[e][0], L.OK) and sweeps[e] == cold1[e], what
                assert np.array_equal(b.read(L.BUF_FACTOR, e), want[e][1]) and np.array_equal(b.read(L.BUF_EIGVALS, e), want[e][2]), what
                check_edge(L, b, e, n1, "any", what)
            else:
                assert rows0[e].shape == (Lg, Lg) and again[e] < cold0[e], (what, cold0[e], again[e])
                check_warm_edge(L, b, e, n1, rows0[e], what)
    finally:
        b.close()


# ---- a singular covariance after a full-rank one ---------------------------------------------------------------------------------

def cold_factor(amd, ctx, Lg, name):
    L = amd._lib
    b, (sweeps,) = start(amd, ctx, [(Lg, name)])
    try:
        sc = b.scalars(0)
        assert sc.status == L.OK
        return sc.rank, np.array(b.read(L.BUF_FACTOR)), np.array(b.read(L.BUF_EIGVALS)), sweeps
    finally:
        b.close()


@pytest.mark.parametrize("deficient", ["def", "def1"])
@pytest.mark.parametrize("Lg", sorted(fx.WARM_DEF))
def test_three_steps_full_rank_singular_full_rank(amd, ctx, Lg, deficient):
    L = amd._lib
    n0, nd, n1 = "w%d-0" % Lg, "w%d-%s" % (Lg, deficient), "w%d-1" % Lg
    Bd, Sd = fx.sigma(nd)
    r = Bd.shape[0]
    b, (cold,) = start(amd, ctx, [(Lg, n0)])
    try:
        A0 = full_rows(L, b, 0, Lg)
        # step 2
        (sw2,) = step(L, b, [nd], 1)
        sc = b.scalars(0)
        A2, ev2 = np.array(b.read(L.BUF_FACTOR)), np.array(b.read(L.BUF_EIGVALS))
        what = "%d columns step 2 (rank %d of %d)" % (Lg, r, Lg)
        assert sc.status == L.OK and sc.rank in (r, Lg), (what, sc.status, sc.rank)
        assert A2.shape == (sc.rank, Lg) and ev2.shape == (sc.rank,) and np.all(np.isfinite(A2)) and np.all(np.isfinite(ev2)), what
        assert np.all(np.diff(ev2) <= 0), what
        A2x = fx.ext(A2)
        bf = fx.bound_fro(Sd, r)
        if sc.rank == r:  # a pivot was not positive: the pivoted Cholesky took over, Sigma_def itself is the target
            target = fx.ext(Sd)
            print("STEP2 %s: fell back to the pivoted Cholesky, rank %d, sweeps %d" % (what, sc.rank, sw2))
        else:  # every pivot accepted: rank Lg, the directions beyond r are rounding
            target = _projection(A0.tobytes(), Lg, nd)[0]
            tail = float(ev2[r:].max())
            print("STEP2 %s: warm start accepted, rank %d, sweeps %d, largest eigenvalue beyond r = %.3g (%.3g of |bound|_F), smallest = %.3g"
                  % (what, sc.rank, sw2, tail, tail / bf, float(ev2[-1])))
            assert tail <= bf, (what, tail, bf)
        rec2 = _frac(abs(A2x.T @ A2x - target), fx.bound_matrix(Sd, r))
        print("STEP2 %s: rec %.3g" % (what, rec2))
        assert rec2 <= 1.0, (what, rec2)
        kept = sc.rank == Lg and sw2 < b.get_option("oj_max_sweeps")  # (k_oj_rows keeps rows of full rank of a converged Jacobi)
        # step 3
        (sw3,) = step(L, b, [n1], 2)
        what = "%d columns step 3 after %s" % (Lg, "kept rows" if kept else "a fallback")
        print("SWEEPS %s: %d (Sigma_0 cold: %d)" % (what, sw3, cold))
        if kept:
            check_warm_edge(L, b, 0, n1, A2, what)
        else:
            check_edge(L, b, 0, n1, "any", what)
    finally:
        b.close()


@pytest.mark.parametrize("Lg", sorted(fx.WARM_DEF))
def test_natural_fallback_in_a_later_panel(amd, ctx, Lg):
    """Sigma_def after Sigma_0: M' is exactly singular from column r >= 64 on, a pivot of the panel at k0 = 64 (or later) is not
    positive, and the factor must be the pivoted Cholesky's, as if the warm start had never touched G and Gt: the property
    test_any_rank_factor_warm_start_falls_back_to_the_pivoted_cholesky asserts for an injected failure at k0 = 0."""
    L = amd._lib
    n0, nd = "w%d-0" % Lg, "w%d-def" % Lg
    rank, A, ev, sweeps = cold_factor(amd, ctx, Lg, nd)
    assert rank == fx.sigma(nd)[0].shape[0]
    b, _ = start(amd, ctx, [(Lg, n0)])
    try:
        (sw,) = step(L, b, [nd], 1)
        sc = b.scalars(0)
        print("FALLBACK %d columns: rank %d (cold %d), sweeps %d (cold %d)" % (Lg, sc.rank, rank, sw, sweeps))
        assert (sc.rank, sc.status, sw) == (rank, L.OK, sweeps)
        assert np.array_equal(b.read(L.BUF_FACTOR), A) and np.array_equal(b.read(L.BUF_EIGVALS), ev)
    finally:
        b.close()
