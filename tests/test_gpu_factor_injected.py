"""The eigen-factor stage on injected covariances of known spectrum: Sigma (tests/factor_exact.py: exact in float64, of exact rank)
written through GPET_BUF_COV, factored by gpet_gp_factor, GPET_BUF_FACTOR / GPET_BUF_EIGVALS compared with the extended-precision
reference of the same matrix (factor_exact.ref_factor, pinned on the host by tests/test_factor_exact.py).  Every residual is
formed in the extended format.

Paths, selected by the batch's capacity and width (the plans of csrc/gpet_factor_plan.h, which tests/test_factor_plan.py holds
against the shapes used here), not by the rank that is found:
* LDS path (capacity <= 96): k_pchol_reg (Lg <= 512), k_pchol (513), the multi-workgroup form (1030, options 1 and 2) -> k_gram ->
  k_jacobi_seat<2|3, log|no log> (option jacobi_variant = 0) or k_jacobi_ahead<2|3, log> / <2, no log, RR 6> / <3, no log>
  (1, the default), the log forms followed by k_jacobi_wpass -> k_factor_rows.  Capacities 40 .. 96 on 100 columns stand on
  both sides of every switch: k_jacobi_ahead's two -> three blocks per thread (82 | 84), k_jacobi_seat's (88 | 90), the register
  rows of k_jacobi_ahead<2, false, 6> (below 42 all of the padded matrix's 42 rows would be register rows); each capacity as
  one batch of four edges of exact rank 1, an odd rank, cap - 1 and cap.  "No log" is option jlog_max_b = 0 when the batch is
  created; jacobi_logw = 0 takes the no-log kernels on a batch that has a log.
* any-rank path (capacity > 96, csrc/gpet_eig.hip): k_pcb_block or k_pcx_step (pcx_one_pivot) -> k_oj_persist or k_oj_round
  (oj_persist = 0), staged or not (oj_stage), pointers in the arguments or the edge table (oj_args; nine edges: above
  OJ_ARGS_MAXB) -> k_oj_norms, k_oj_order, k_oj_rows.  Ranks off the 8-row block (41, 97, 105, 129), an odd (7, 13, 17) and
  an even number of blocks, widths off the 32-column slab, more than PCB_CH = 128 previous rows (129, 136).

What a factor A (rank rows) with eigenvalues ev must satisfy -- bounds and their derivation in tests/factor_exact.py
(bound_ij = C_REC r u sqrt(Sigma_ii Sigma_jj), C_REC = 124 from ten sweeps' rounding; the sweeps the kernels report are printed):
  rank        rank == r, status 0, shapes, everything finite, ev non-increasing
  rec         |A^T A - Sigma|_ij <= bound_ij
  weyl        |ev_k - s_k| <= |bound|_F
  evnorm      |ev_k - |A_k|^2| <= (Lg + 2) u ev_k
  relev       any-rank path: |ev_k - s_k| / s_k < 1e-6 (LAPACK's eigvalsh on the same matrix is printed beside it)
  orth        any-rank path: |A_i.A_k| <= 1e-10 |A_i||A_k|; LDS path (two-sided Jacobi on the Gram matrix: absolute): <= |bound|_F
  rows        isolated eigenvalues: |+-A_k - F_k| <= sqrt(s_k) 2 |bound|_F / gap_k + |sqrt(ev_k) - sqrt(s_k)|
  clusters    groups closer than 20 |bound|_F: |sum A_k^T A_k - sum F_k^T F_k|_F <= s 2 |bound|_F / gap_outside + sum |(|A_k|^2 - s_k)|
              + the group's own spread (0 for the exactly degenerate Hadamard and diagonal cases, whose sum is B's rows')
  sign        sum_j A[k, j] / (j + 1) >= -Lg u sum_j |A[k, j]| / (j + 1)
Each check returns its largest deviation as a fraction of the bound (printed with -s).

Measured on an MI355X (largest deviation as a fraction of its bound, over all cases of a path; sweeps as the kernels report them):
  LDS path, graded and pair cases   rec 0.022  weyl 0.012  evnorm 0.12  orth 0.12  rows 0.012            sweeps <= 7
  LDS path, Hadamard and diagonal   rec 0.006  weyl 0.001  evnorm 0.054 orth 0.81  rows 0.30  clusters 0.32   sweeps <= 7
  any-rank path, graded cases       rec 0.030  weyl 0.003  evnorm 0.019 orth 0.010 rows 0.0005 relev 0.15 (1.5e-7 at rank 97 of
                                    97 over twelve octaves, where eigvalsh has 6e-8; 1e-11 .. 1e-9 elsewhere)      sweeps <= 8
  any-rank path, Hadamard           rec 0.027  weyl 0.002  evnorm 0.017 orth 0.039 rows 0.0005 clusters 0.0008    sweeps 15-18
C_REC stands with a factor 30 to spare: the rotations' errors do not add up in the worst case's way.
What the first run found, with the kernels as they were:
* evnorm on the LDS path was 1.06 .. 1.86 at ranks 33 and 64 .. 96 (under 1 below): GPET_BUF_EIGVALS was the diagonal of the
  rotated Gram matrix, which carries the rounding of every rotation, and agreed with the rows' norms to 2e-14 only.
  k_factor_rows now reports the row's squared norm, as the any-rank path does (gpet_batch_read hands the values out in
  descending order): 0.12 at most.
* orth on the any-rank path with EXACTLY degenerate groups (bhad128-r105: groups of 2, 3, 8 and 15 equal eigenvalues) was 0.53
  with the defaults, 1.48 with oj_stage = 0 and 7.4 with pcx_one_pivot = 1: rows of one group left coupled by up to 7.4e-10 of
  their norms.  The stopping test takes every coupling as a sweep MEETS it, before the sweep rotates it, at 1e-8; "squared"
  holds where the eigenvalues differ (5e-5 met, 8e-12 left); equal eigenvalues whose rows are not neighbours converge linearly, a
  factor 5 to 10 a sweep (left after sweeps 13 .. 16 with pcx_one_pivot: 1.7e-7, 2.1e-8, 6.0e-9, 7.4e-10), and the test stopped
  with whatever the last factor gave.  The verdict (oj_verdict, csrc/gpet_eig.hip) now also asks that what the last two sweeps
  met PREDICTS less than 1e-11 left, c_k^3 / c_(k-1)^2: one or two sweeps more for this case (16 .. 18; the budget
  oj_max_sweeps went from 16 to 20), orth 0.039 at most, and the same sweeps and bits as before on every graded case.

Zero matrix.  Read before it was run: k_pchol_reg / k_pchol take no pivot (the first candidate is 0: not above tol = 0), rank 0;
k_gram and k_factor_rows return on their first row test; the Jacobi kernels run no sweep below rank 2 and their loops over
blocks, pairs and rows are empty (k_jacobi_ahead forms, and never uses, addresses from a block count of 0); k_jacobi_wpass
returns before it reads the log.  The contract: rank 0, status OK, empty factor and eigenvalues.

Scaling.  Sigma 4^+-20 must give the same rank and rows 2^+-20 times the unscaled ones, bit for bit: powers of two commute with
every rounding, so a difference means an absolute constant in the kernels (test_scaling_by_powers_of_four).
"""
import numpy as np
import pytest

from tests import factor_exact as fx
from tests.injected_batch import make_batch

pytestmark = pytest.mark.gpu

U = fx.U


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


class options:
    """Process-wide options for the batches created inside (a batch copies the table when it is created); restored on exit."""

    def __init__(self, L, opts):
        self.L, self.opts, self.old = L, dict(opts), {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.old[k] = self.L.set_option(k, v, live_batches=False)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.L.set_option(k, v, live_batches=False)


def batch_of(amd, ctx, edges, scale=1.0):
    """A batch of the edges [(case name or Sigma, Lg, factor_cap)], Sigma * scale written to GPET_BUF_COV of each."""
    n_cols = max(Lg for _, Lg, _ in edges)
    grad = np.random.default_rng(5).random((8, n_cols)).astype(np.float32)
    grad[0, 0], grad[7, n_cols - 1] = 0.0, 1.0
    b = make_batch(amd, ctx, grad, [(0, Lg) for _, Lg, _ in edges], 16, factor_cap=[cap for _, _, cap in edges])
    try:
        for e, (what, Lg, cap) in enumerate(edges):
            S = fx.case(what)[1] if isinstance(what, str) else what
            assert S.shape == (Lg, Lg) and b.info(e)["Lg"] == Lg
            b.write(amd._lib.BUF_COV, S * scale, e)
    except BaseException:
        b.close()
        raise
    return b


def _frac(dev, bound):
    """max dev / bound; a zero bound admits a zero deviation only."""
    dev, bound = np.asarray(fx.f64(dev), dtype=np.float64), np.asarray(bound, dtype=np.float64)
    zero = bound == 0
    assert np.all(dev[zero] == 0), "a deviation where the bound is zero"
    return float((dev[~zero] / bound[~zero]).max(initial=0.0))


def check_edge(L, b, e, name, path, what, rec_target=None):
    """All of the module docstring's conditions on edge e against the case ``name``; returns {check: fraction of its bound}.
    rec_target: the matrix (extended format) that ``rec`` compares A^T A with where the algorithm does not target Sigma itself
    (tests/test_gpu_factor_warm_injected.py: the warm start's P Sigma P); every bound stays Sigma's."""
    B, S, F, s = fx.case(name)
    r, Lg = B.shape
    sc = b.scalars(e)
    assert (sc.rank, sc.status) == (r, L.OK), (what, sc.rank, sc.status)
    A, ev = b.read(L.BUF_FACTOR, e), b.read(L.BUF_EIGVALS, e)
    assert A.shape == (r, Lg) and ev.shape == (r,) and np.all(np.isfinite(A)) and np.all(np.isfinite(ev)), what
    assert np.all(np.diff(ev) <= 0), what
    sf = fx.f64(s)
    bound, bf = fx.bound_matrix(S, r), fx.bound_fro(S, r)
    Ax = fx.ext(A)
    out = {"rec": _frac(abs(Ax.T @ Ax - (fx.ext(S) if rec_target is None else rec_target)), bound)}
    nrm2 = (Ax * Ax).sum(axis=1)
    out["weyl"] = _frac(abs(fx.ext(ev) - s), np.full(r, bf))
    out["evnorm"] = _frac(abs(fx.ext(ev) - nrm2), (Lg + 2) * U * ev)
    Gm = fx.f64(Ax @ Ax.T)
    nrm = np.sqrt(np.diag(Gm))
    off = np.abs(Gm - np.diag(np.diag(Gm)))
    if path == "any":
        rel = float(np.abs(fx.f64(fx.ext(ev) - s) / sf).max())
        w = np.linalg.eigvalsh(S)[::-1][:r]
        print("%s: max |ev - s| / s = %.2e (eigvalsh on the same matrix: %.2e)" % (what, rel, np.abs(fx.f64(fx.ext(w) - s) / sf).max()))
        out["relev"] = rel / 1e-6
        out["orth"] = _frac(off, 1e-10 * np.outer(nrm, nrm))
    else:
        out["orth"] = _frac(off, np.full((r, r), bf))
    # rows of isolated eigenvalues one by one, the others by groups
    g = fx.gaps(sf, r == Lg)
    iso = fx.iso_gap(S, r)
    rows_checked, worst_row, worst_cl = 0, 0.0, 0.0
    for k0, k1 in fx.groups_of(S, sf, r):
        if k1 - k0 == 1 and g[k0] >= iso:
            k = k0
            d = min(np.sqrt(fx.f64(((Ax[k] - F[k]) ** 2).sum())), np.sqrt(fx.f64(((Ax[k] + F[k]) ** 2).sum())))
            lim = np.sqrt(sf[k]) * 2 * bf / g[k] + abs(np.sqrt(ev[k]) - np.sqrt(sf[k]))
            assert lim <= np.sqrt(sf[k]) * 0.1 * 1.5
            worst_row = max(worst_row, _frac(d, lim))
            rows_checked += 1
            continue
        lo = sf[k1] if k1 < r else (0.0 if r < Lg else -np.inf)
        gap_out = min(sf[k0 - 1] - sf[k0] if k0 > 0 else np.inf, sf[k1 - 1] - lo)
        if not 2 * bf / gap_out <= 0.1:
            continue  # (a last eigenvalue within 20 |bound|_F of 0: nothing to compare it by)
        Pd, Pr = Ax[k0:k1].T @ Ax[k0:k1], F[k0:k1].T @ F[k0:k1]
        d = np.sqrt(fx.f64(((Pd - Pr) ** 2).sum()))
        lim = sf[k0] * 2 * bf / gap_out + float(fx.f64(abs(nrm2[k0:k1] - s[k0:k1]).sum())) + (sf[k0] - sf[k1 - 1])
        worst_cl = max(worst_cl, _frac(d, lim))
        rows_checked += k1 - k0
    assert rows_checked >= 0.9 * r, (what, rows_checked, r)
    out["rows"], out["clusters"] = float(worst_row), float(worst_cl)
    wts = 1.0 / np.arange(1, Lg + 1)
    assert np.all(fx.f64((Ax * fx.ext(wts)[None, :]).sum(axis=1)) >= -Lg * U * (np.abs(A) * wts[None, :]).sum(axis=1)), what
    print("FRAC %s %s: sweeps %d  %s" % (path, what, int(sc.lml), "  ".join("%s %.3g" % kv for kv in out.items())))
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return out


def run_cases(amd, ctx, edges, path, what, opts=None, batch_opts=None):
    """One launch over edges [(case name, Lg, cap)] under the options opts (set while the batch is created) and batch_opts
    (set on the batch afterwards); every edge checked."""
    L = amd._lib
    with options(L, opts or {}):
        b = batch_of(amd, ctx, edges)
    try:
        for k, v in (batch_opts or {}).items():
            b.set_option(k, v)
        b.factor()
        return [check_edge(L, b, e, name, path, "%s edge %d %s cap %d" % (what, e, name, cap)) for e, (name, Lg, cap) in enumerate(edges)]
    finally:
        b.close()


# ---- LDS path ------------------------------------------------------------------------------------------------------------------

LOG_MODES = {"log": ({}, {}), "nolog": ({"jlog_max_b": 0}, {}), "logw0": ({}, {"jacobi_logw": 0})}


@pytest.mark.parametrize("mode", sorted(LOG_MODES))
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("cap", fx.LDS_CAPS)
def test_lds_path_at_the_instantiation_boundaries(amd, ctx, cap, variant, mode):
    opts, batch_opts = LOG_MODES[mode]
    edges = [("g100-r%d" % r, 100, cap) for r in fx.lds_ranks(cap)]
    run_cases(amd, ctx, edges, "lds", "cap %d variant %d %s" % (cap, variant, mode), dict(opts, jacobi_variant=variant), batch_opts)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("Lg", [4, 7, 33, 64, 65])
def test_lds_path_full_rank_widths(amd, ctx, Lg, variant):
    """rank = Lg: no column is left unpivoted; odd widths are padded to even; 4 and 7: fewer columns than a wave."""
    run_cases(amd, ctx, [("g%d-full" % Lg, Lg, min(Lg, 96))], "lds", "width %d variant %d" % (Lg, variant), {"jacobi_variant": variant})


def test_lds_path_513_columns_takes_k_pchol(amd, ctx):
    run_cases(amd, ctx, [("g513-r31", 513, 96)], "lds", "k_pchol")


@pytest.mark.parametrize("pchol_multi", [0, 1, 2])
def test_lds_path_1030_columns_pivoted_cholesky_over_the_gpu(amd, ctx, pchol_multi):
    run_cases(amd, ctx, [("g1030-r20", 1030, 96)], "lds", "pchol_multi %d" % pchol_multi, {"pchol_multi": pchol_multi})


SPECTRA = [("g100-r17-oct16", 100, 40), ("had32-equal", 32, 32), ("had32-groups", 100, 40), ("diag33", 33, 33), ("pair-small", 8, 8),
           ("pair-large", 8, 8)]


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name,Lg,cap", SPECTRA, ids=[c[0] for c in SPECTRA])
def test_lds_path_spectra(amd, ctx, name, Lg, cap, variant):
    """Sixteen octaves; all eigenvalues equal; groups of 2, 3 and 8 equal ones; a diagonal matrix with ties; the two extremes of
    the rotation parameters."""
    run_cases(amd, ctx, [(name, Lg, cap)], "lds", "spectrum variant %d" % variant, {"jacobi_variant": variant})


@pytest.mark.parametrize("variant", [0, 1])
def test_lds_path_mixed_batch(amd, ctx, variant):
    """One launch over edges of different width, capacity and rank: the kernels are shaped by the batch's maximum."""
    names = {(7, 7, 7): "g7-full", (97, 90, 41): "g97-r41", (64, 40, 1): "g64-r1"}
    run_cases(amd, ctx, [(names[m], m[0], m[1]) for m in fx.MIXED], "lds", "mixed variant %d" % variant, {"jacobi_variant": variant})


def test_lds_path_capacity(amd, ctx):
    """Exact rank = capacity: status OK, rank = cap (g100-r40 at capacity 40, also in the boundary batches).  One more direction
    at 1e-6 of the largest: GPET_ERR_RANK_CAP."""
    L = amd._lib
    run_cases(amd, ctx, [("g100-r%d" % fx.CAP_ERR, 100, fx.CAP_ERR)], "lds", "rank = cap")
    b = batch_of(amd, ctx, [("g100-r41-over", 100, fx.CAP_ERR)])  # (a fresh batch: the status sticks)
    try:
        with pytest.raises(L.GpetError) as err:
            b.factor()
        assert err.value.code == L.ERR_RANK_CAP
        assert b.scalars(0).status == L.ERR_RANK_CAP
    finally:
        b.close()


def test_zero_matrix_has_rank_zero(amd, ctx):
    L = amd._lib
    b = batch_of(amd, ctx, [(np.zeros((33, 33)), 33, 33)])
    try:
        b.factor()
        sc = b.scalars(0)
        assert (sc.rank, sc.status) == (0, L.OK) and np.isfinite(sc.lml)
        assert b.read(L.BUF_FACTOR).shape == (0, 33) and b.read(L.BUF_EIGVALS).shape == (0,)
    finally:
        b.close()


# ---- any-rank path ---------------------------------------------------------------------------------------------------------------

BIG_CASES = [("b%d-r%d" % (Lg, r), Lg) for Lg, r in fx.BIG] + [("bhad128-r105", 130)]
BIG_OPTS = [{}, {"pcx_one_pivot": 1}, {"oj_stage": 0}, {"oj_args": 0}, {"oj_persist": 0}]


@pytest.mark.parametrize("opts", BIG_OPTS, ids=["default", "pcx_one_pivot", "oj_stage0", "oj_args0", "oj_persist0"])
@pytest.mark.parametrize("name,Lg", BIG_CASES, ids=[c[0] for c in BIG_CASES])
def test_any_rank_path(amd, ctx, name, Lg, opts):
    run_cases(amd, ctx, [(name, Lg, Lg)], "any", "any-rank %s" % (opts or "default"), opts)


def test_any_rank_path_batch_of_nine(amd, ctx):
    """Above OJ_ARGS_MAXB = 8 edges the per-edge pointers come from the edge table; widths and ranks differ across the batch."""
    edges = [(n, Lg, Lg) for n, Lg in BIG_CASES] + [("b130-r104", 130, 130), ("b97-r97", 97, 97)]
    assert len(edges) == 9
    run_cases(amd, ctx, edges, "any", "nine edges")


# ---- scaling -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,Lg,cap,path", [("g100-r41", 100, 44, "lds"), ("b130-r105", 130, 130, "any")], ids=["lds", "any"])
def test_scaling_by_powers_of_four(amd, ctx, name, Lg, cap, path):
    L = amd._lib
    got = {}
    for k in (0, 20, -20):
        b = batch_of(amd, ctx, [(name, Lg, cap)], scale=4.0 ** k)
        try:
            b.factor()
            sc = b.scalars(0)
            got[k] = (sc.rank, sc.status, b.read(L.BUF_FACTOR), b.read(L.BUF_EIGVALS))
        finally:
            b.close()
    for k in (20, -20):
        assert got[k][:2] == got[0][:2] == (fx.case(name)[0].shape[0], L.OK)
        dA = np.abs(got[k][2] * 2.0 ** -k - got[0][2]).max() / np.abs(got[0][2]).max()
        dev = np.abs(got[k][3] * 4.0 ** -k - got[0][3]).max() / got[0][3][0]
        print("scaling %s 4^%d: rows differ by %.3g of the largest entry, eigenvalues by %.3g of the largest" % (path, k, dA, dev))
        assert np.array_equal(got[k][2] * 2.0 ** -k, got[0][2]), (path, k, dA)
        assert np.array_equal(got[k][3] * 4.0 ** -k, got[0][3]), (path, k, dev)
