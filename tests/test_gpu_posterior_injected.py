"""GPU tests of the posterior of injected training sets -- training-set assembly, K, Cholesky factor, alpha, mean, std and
covariance -- at every size class of the launch rules (csrc/gpet_iter_plan.h), in the loop form (gpet_batch_set_obs +
gpet_gp_fit_predict) and the converged-fit form (gpet_final_set_training_all + gpet_final_predict_all + gpet_final_cov), against
the extended-precision reference of tests/posterior_exact.py under ITS componentwise rounding bounds (derived there; the host
test tests/test_posterior_exact.py holds the float64 oracle and the inputs' sharpness against the same bounds).

Which launch form a row of the table reaches -- every rule decides by the batch's CAPACITY n_cap = max over the edges of
n_init + obs_cap, never by the count n (tests/test_iter_plan.py holds the table's capacities against the header):

  n_cap <= 128 (64, 127, 128)        fit: k_fit<true, .>, K in LDS, 4 x 4 register tiles, the solves by one wave
                                     predict: k_predict<true, .>, a wave's 64 columns of V in LDS
  129 .. 286 (129, 200, 285, 286)    fit: blocked in HBM by CB = 64 -- k_fit_head, k_fit_kbuild, per panel k_chol_diag / k_chol_trsm_sub /
                                     k_chol_syrk (which factors the next diagonal block), k_chol_solve_mw<.> or k_chol_solve -- in
                                     the loop; k_fit<false, true>, left-looking in HBM, for the converged fit
                                     predict: still k_predict<true, .> ((64 n_cap + 3 n_cap) * 8 <= 150 KB of LDS up to 286)
  n_cap >= 287 (287, 330)            fit: as above;  predict, loop: k_kstar_build, k_pred_colsum_big<false>, one k_vsolve_mfma per
                                     64-block of n_cap, k_pred_colsum_big<true> (V through HBM); converged fit: k_predict<false, true>
  covariance, everywhere             k_cov_mfma on 64 x 64 tiles of the grid: Lg = 63, 64, 65 and 130 are a partial, an exact, two
                                     and three tiles (final_mode = 1 after the converged fit)

Under each capacity the counts run from the init points alone to the capacity itself, with the block edges 63 / 64 / 65, 128 /
129, 191 / 192 / 193, 256 / 257 between: the panel kernels are enqueued for every 64-block of n_cap and return past n.  One batch
per capacity holds all its counts as edges on one shared image, so the edges of a batch differ in n, in Lg and -- in the
converged form -- in every parameter.

Each test prints the largest device error / bound it saw (pytest -s); the pass criterion is the derived bound, ratio <= 1."""
import numpy as np
import pytest

from tests import posterior_exact as px
from tests.injected_batch import make_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def image(N):
    return np.random.default_rng(N).random((px.M_ROWS, N)).astype(np.float32)


def kernel_options(kernel, length):
    name, nu = px.KERNELS[kernel]
    d = {'kernel': name, 'sigma_f': px.SIGMA_F, 'length_scale': length}
    if name == "Matern":
        d['nu'] = nu
    return d


def build(amd, ctx, cases, kernel, fixes, n_cap=None, delta_x=2):
    """One batch with the Cases as its edges on one shared image; the capacities come out as the Cases name them, and the batch's
    as n_cap (the largest by default).  delta_x = 2 leaves an edge about N / 2 + 2 bins, below every capacity of the table on
    the table's image widths (px.width_for); a list gives a batch's edges different bin counts on one width."""
    N = cases[0].N
    assert all(c.N == N for c in cases)
    b = make_batch(amd, ctx, image(N), [(c.x_st, c.Lg) for c in cases], 64, delta_x=delta_x, fix_endpoints=list(fixes),
                   kernel=[kernel_options(kernel, c.length) for c in cases], obs_cap=[c.n_cap - c.n_init for c in cases],
                   inits=[c.points()[0] for c in cases])
    for e, c in enumerate(cases):
        inf = b.info(e)
        assert (inf["n_cap"], inf["Lg"], inf["obs_cap"]) == (c.n_cap, c.Lg, c.n_cap - c.n_init), (c, inf)
    assert b._max_info("n_cap") == (max(c.n_cap for c in cases) if n_cap is None else n_cap)
    return b


def inject_loop(b, cases):
    for e, c in enumerate(cases):
        b.set_obs(e, c.points()[1])


def check_core(tag, core, chol, alpha, mean, std, cov, mean_key="mean", b_mean="b_mean"):
    assert np.array_equal(cov, cov.T), tag  # bitwise: k_cov_mfma mirrors the tiles above the diagonal
    r = dict(L=px.factor_ratio(chol, core), alpha=px.ratio(alpha, core["alpha"], core["b_alpha"]),
             mean=px.ratio(mean, core[mean_key], core[b_mean]), var=px.std_ratio(std, core),
             cov=px.ratio(cov, core["cov"], core["b_cov"]), cov_diag=px.ratio(np.diag(cov), core["cov"].diagonal(), core["b_var"]))
    print("%-48s %s" % (tag, "  ".join("%s %.3g" % kv for kv in r.items())))
    assert px.within(r), (tag, r)  # (every ratio a number <= 1: NaN fails)
    return r


def check_loop_edge(L, b, e, c, kernel, fix):
    """Edge e of the batch holds Case c in the loop form: everything the fit and the prediction leave, against the reference."""
    tag = "%s %s fix=%d" % (c, kernel, fix)
    s = b.scalars(e)
    x, y, w = c.training(fix)
    assert s.status == 0 and s.n == c.n, (tag, s.status, s.n)
    assert np.array_equal(b.read(L.BUF_X_TRAIN, e), x), tag      # the stable sort by x, init points first among equals
    assert np.array_equal(b.read(L.BUF_NOISE_W, e), w), tag
    ex, bd, _ = px.loop_reference(c.key(), kernel, fix)
    yt = b.read(L.BUF_Y_TRAIN, e)
    pre = dict(y_s=px.ratio(s.y_s, ex["y_s"], bd["y_s"]), amp=px.ratio(s.amp, ex["amp"], bd["amp"]),
               y_mean=px.ratio(s.y_mean, ex["y_mean"], bd["y_mean"]), y_std=px.ratio(s.y_std, ex["y_std"], bd["y_std"]),
               y_train=px.ratio(yt, ex["y_train"], bd["y_train"]))
    assert px.within(pre), (tag, pre)
    # the core on the float64 values the device holds, which have just passed their own bounds
    _, _, core = px.loop_reference(c.key(), kernel, fix, held=(yt.tobytes(), float(s.amp), float(s.y_mean), float(s.y_std)))
    chol = b.read(L.BUF_CHOL, e)
    if c.n == c.Lg:  # "the weights vanish when there are edge_length training rows": no noise on K's diagonal
        assert abs(chol[0, 0] ** 2 - (s.amp + 1e-6)) <= 1e-12 * s.amp, (tag, chol[0, 0] ** 2, s.amp)
        assert np.all(px.f64(core["K"].diagonal()) < s.amp + 2e-6)
    r = check_core(tag, core, chol, b.read(L.BUF_ALPHA, e), b.read(L.BUF_MEAN, e), b.read(L.BUF_STD, e), b.read(L.BUF_COV, e))
    return dict(r, **pre)


def inject_final(b, cases, fixes):
    ins = [px.final_inputs(c, f) for c, f in zip(cases, fixes)]
    b.final_set_training_all([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins])
    mean, std = b.final_predict_all(np.stack([i[3] for i in ins]))
    b.final_cov()
    return ins, mean, std


def check_final_edge(L, b, e, c, kernel, fix, inputs, mean, std):
    tag = "%s %s fix=%d converged" % (c, kernel, fix)
    xs, ys, w, par = inputs
    s = b.scalars(e)
    assert s.status == 0 and s.n == c.n and s.amp == par[0] and s.y_mean == par[7] and s.y_std == par[8], tag
    assert np.array_equal(b.read(L.BUF_X_TRAIN, e), xs) and np.array_equal(b.read(L.BUF_Y_TRAIN, e), ys), tag
    assert np.array_equal(b.read(L.BUF_NOISE_W, e), w), tag
    out = b.read(L.BUF_FIN_OUT, e)
    assert np.array_equal(out[0], mean[e, :c.Lg]) and np.array_equal(out[1], std[e, :c.Lg]), tag
    core = px.final_reference(c.key(), kernel, fix)
    chol = b.read(L.BUF_CHOL, e)
    if c.n == c.Lg:
        assert np.all(w == 0) and abs(chol[0, 0] ** 2 - (par[0] + 1e-6)) <= 1e-12 * par[0], tag
    return check_core(tag, core, chol, b.read(L.BUF_ALPHA, e), out[0], out[1], b.read(L.BUF_COV, e), "out_mean", "b_out_mean")


def summary(tag, rs):
    worst = {}
    for r in rs:
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("%s: largest device error / bound: %s" % (tag, "  ".join("%s %.3g" % kv for kv in worst.items())))


COMBO_IDS = {c: "%s-fix%d" % c for c in px.COMBOS + tuple(px.EXTRA_KERNELS.values())}
TABLE = [pytest.param(n_cap, combo, id="cap%d-%s" % (n_cap, COMBO_IDS[combo])) for n_cap in px.ALL_CAPS for combo in px.combos_of(n_cap)]


def table_cases(n_cap, fix):
    """The counts of a capacity and its n == Lg case, under either fix_endpoints setting."""
    return list(px.cases_of(n_cap)) + [px.full_grid_case(n_cap)]


@pytest.mark.parametrize("n_cap,combo", TABLE)
def test_loop_posterior_every_count_of_a_capacity(amd, ctx, n_cap, combo):
    L = amd._lib
    kernel, fix = combo
    cases = table_cases(n_cap, fix)
    b = build(amd, ctx, cases, kernel, [fix] * len(cases))
    try:
        inject_loop(b, cases)
        b.fit_predict(want_cov=True)
        summary("loop, n_cap %d, %s, fix_endpoints %d" % (n_cap, kernel, fix),
                [check_loop_edge(L, b, e, c, kernel, fix) for e, c in enumerate(cases)])
    finally:
        b.close()


@pytest.mark.parametrize("n_cap,combo", TABLE)
def test_converged_posterior_every_count_of_a_capacity(amd, ctx, n_cap, combo):
    """gpet_final_predict_all and gpet_final_cov: edges of one batch with different n and different par[0..8] -- amplitude, length
    scale, noise level, grid offset and scale, output offset and scale, y_mean and y_std, none of them trivial."""
    L = amd._lib
    kernel, fix = combo
    cases = table_cases(n_cap, fix)
    b = build(amd, ctx, cases, kernel, [fix] * len(cases))
    try:
        ins, mean, std = inject_final(b, cases, [fix] * len(cases))
        pars = np.stack([i[3] for i in ins])
        assert np.all(pars[:, 4] != 1) and np.all(pars[:, [3, 5, 7]] != 0) and np.all(pars[:, [6, 8]] != 1)
        assert len({tuple(p[:3]) for p in pars}) >= min(5, len({c.n % 5 for c in cases}))
        summary("converged, n_cap %d, %s, fix_endpoints %d" % (n_cap, kernel, fix),
                [check_final_edge(L, b, e, c, kernel, fix, ins[e], mean, std) for e, c in enumerate(cases)])
    finally:
        b.close()


@pytest.mark.parametrize("n_cap", [200, 330])
@pytest.mark.parametrize("solve_mw,diag_in_syrk", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_blocked_fit_variants_under_the_bounds(amd, ctx, n_cap, solve_mw, diag_in_syrk):
    """The four forms of the blocked fit (alpha by one workgroup per 64-row block or by one workgroup; the next diagonal block
    factored inside the trailing update or by a launch of its own), each under the same bounds."""
    L = amd._lib
    cases = table_cases(n_cap, True)
    b = build(amd, ctx, cases, "RBF", [True] * len(cases))
    try:
        b.set_option("solve_mw", solve_mw)
        b.set_option("diag_in_syrk", diag_in_syrk)
        inject_loop(b, cases)
        b.fit_predict(want_cov=True)
        summary("loop, n_cap %d, solve_mw %d, diag_in_syrk %d" % (n_cap, solve_mw, diag_in_syrk),
                [check_loop_edge(L, b, e, c, "RBF", True) for e, c in enumerate(cases)])
    finally:
        b.close()


@pytest.mark.parametrize("n_cap", px.JITTER_ONLY_CAPS)
def test_jitter_only_covariance_blocked_and_through_hbm(amd, ctx, n_cap):
    """px.jitter_only_case: K the jitter away from singular.  Alpha and the mean are inside their bounds too, but those bounds are
    vacuous on this set (the host test says so); what it pins is the factor, the std and the covariance -- in the LDS prediction
    (200) and in k_vsolve_mfma's (287, 330), which missed this covariance bound before its refinement step."""
    L = amd._lib
    cases = [px.jitter_only_case(n_cap)]
    b = build(amd, ctx, cases, "RBF", [True])
    try:
        inject_loop(b, cases)
        b.fit_predict(want_cov=True)
        r = check_loop_edge(L, b, 0, cases[0], "RBF", True)
        summary("loop, jitter-only K, n_cap %d" % n_cap, [r])
    finally:
        b.close()


# ---- mixed batches -------------------------------------------------------------------------------------------------------------

def mixed_cases():
    """Five edges on one image of the widest capacity's width whose own capacities fall in all three regimes (64 and 128: K and V
    in LDS alone; 200 and 286: blocked; 330: V through HBM) with n = 2, 64, 129, 200 and a full 330: bd.n_cap = 330 puts every one
    of them through the blocked fit and the HBM prediction.  (An edge's capacity is at least its bin count, about N / delta_x + 2:
    MIXED_DX gives the small capacities room on the wide image.)"""
    N = px.width_for(330)
    return [px.Case(64, 2, 2, 63, N, seed=1), px.Case(128, 2, 64, 65, N, seed=2), px.Case(200, 2, 129, 64, N, dup=True, seed=3),
            px.Case(286, 2, 200, 130, N, seed=4), px.Case(330, 2, 330, 65, N, seed=5)]


MIXED_FIX = [False, True, False, True, False]
MIXED_DX = [16, 8, 4, 4, 2]


@pytest.mark.parametrize("kernel", ["RBF", "M25"])
def test_mixed_batch_loop_form(amd, ctx, kernel):
    L = amd._lib
    cases = mixed_cases()
    b = build(amd, ctx, cases, kernel, MIXED_FIX, n_cap=330, delta_x=MIXED_DX)
    try:
        inject_loop(b, cases)
        b.fit_predict(want_cov=True)
        summary("loop, mixed batch, %s" % kernel, [check_loop_edge(L, b, e, c, kernel, f) for e, (c, f) in enumerate(zip(cases, MIXED_FIX))])
    finally:
        b.close()


@pytest.mark.parametrize("kernel", ["RBF", "M25"])
def test_mixed_batch_converged_form(amd, ctx, kernel):
    L = amd._lib
    cases = mixed_cases()
    b = build(amd, ctx, cases, kernel, MIXED_FIX, n_cap=330, delta_x=MIXED_DX)
    try:
        ins, mean, std = inject_final(b, cases, MIXED_FIX)
        summary("converged, mixed batch, %s" % kernel,
                [check_final_edge(L, b, e, c, kernel, f, ins[e], mean, std) for e, (c, f) in enumerate(zip(cases, MIXED_FIX))])
    finally:
        b.close()


def test_mixed_batch_done_edges_are_left_alone(amd, ctx):
    """One iteration of the loop on the mixed batch.  gpet_batch_set_obs marks an edge done when its observations reach the
    edge's threshold (Lg // delta_x - 1 here), which the four larger sets do; the stage call above runs them regardless (it forces
    every edge), the loop does not.  Their mean and covariance are filled with a pattern beforehand and every other buffer of
    the posterior is read; one iteration later all of it is there bit for bit, while the edge of the two init points -- fitted
    by the blocked kernels and predicted through HBM under bd.n_cap = 330, now without the force flag -- meets the bounds."""
    L = amd._lib
    cases = mixed_cases()
    b = build(amd, ctx, cases, "RBF", MIXED_FIX, n_cap=330, delta_x=MIXED_DX)
    try:
        inject_loop(b, cases)
        b.fit_predict(want_cov=True)
        sc = b.all_scalars()
        assert [s.done for s in sc] == [0, 1, 1, 1, 1] and all(s.force == 0 for s in sc)
        rng = np.random.default_rng(9)
        before = {}
        for e in range(1, 5):
            Lg = cases[e].Lg
            b.write(L.BUF_MEAN, rng.standard_normal(Lg), e)
            b.write(L.BUF_COV, rng.standard_normal((Lg, Lg)), e)
            before[e] = [b.read(w, e) for w in (L.BUF_X_TRAIN, L.BUF_Y_TRAIN, L.BUF_NOISE_W, L.BUF_CHOL, L.BUF_ALPHA, L.BUF_MEAN,
                                                  L.BUF_STD, L.BUF_COV)]
        # edge 0: its posterior wiped, so that what is read afterwards is the loop's
        b.write(L.BUF_MEAN, np.full(cases[0].Lg, np.nan), 0)
        b.write(L.BUF_COV, np.full((cases[0].Lg, cases[0].Lg), np.nan), 0)
        b.iterate([3, 4, 5, 6, 7], 1)
        for e in range(1, 5):
            s = b.scalars(e)
            assert s.done == 1 and s.iter == 0 and s.n_obs == cases[e].n - 2 and s.status == 0, (e, s.done, s.iter, s.n_obs)
            after = [b.read(w, e) for w in (L.BUF_X_TRAIN, L.BUF_Y_TRAIN, L.BUF_NOISE_W, L.BUF_CHOL, L.BUF_ALPHA, L.BUF_MEAN,
                                            L.BUF_STD, L.BUF_COV)]
            for k, (p, q) in enumerate(zip(before[e], after)):
                assert p.shape == q.shape and np.array_equal(p.view(np.int64), q.view(np.int64)), (e, k)
        assert b.scalars(0).iter == 1
        check_loop_edge(L, b, 0, cases[0], "RBF", MIXED_FIX[0])
    finally:
        b.close()
