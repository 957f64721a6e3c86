"""The loop's prior-eigenbasis ("structured") path on injected on-grid training sets, stage by stage against the extended-precision
reference and the derived bounds of tests/struct_exact.py (pinned on the host by tests/test_struct_exact.py, which also holds the
table's launch classes against csrc/gpet_iter_plan.h): gpet_batch_set_obs, then gpet_profile_stage 120 (fit), 121 (U, H, beta,
mean: GPET_BUF_STRUCT_H, GPET_BUF_ALPHA, GPET_BUF_CHOL, GPET_BUF_MEAN are read here), 122 (Jacobi on H), 123 (factor rows:
GPET_BUF_FACTOR, GPET_BUF_EIGVALS); the basis (GPET_BUF_STRUCT_Q0, GPET_BUF_STRUCT_LAM0) is read as the batch's creation left it.
set_obs marks an edge done when its set reaches the edge's threshold and the stage calls skip done edges, so the tests clear the
flag through GPET_BUF_SCALARS.  Every check is device error / bound; the tests assert <= 1 (NaN fails) and print the ratios
(pytest -s).

Families (sx.FAMILIES): one batch per family, one edge per count.  The rank r0 of a basis follows the length scale; the length
scales were chosen on the host, and every batch asserts that gpet_batch_info's r0 lies in the family's class, so that a miss fails
instead of testing another class.
  small form (n_cap <= 128, k_struct_H)   s100: L beside U in LDS, counts 2 (the init points alone), 3, 63, 64, 65 (one column
                                          twice), 99, 100;  s128: r0 in 84 .. 88, rows of L streamed, the same counts to 127, 128;  s100c40:
                                          factor_cap 40, n = 81 and 100 > 2 r_cap: the training indices leave LDS;  full64: n == Lg
  K extents of k_struct_rows, Jacobi      e56 (49 .. 64), e70 (65 .. 72), e80 (73 .. 80: a warm start is allowed), e81, e82 (cold; two
                                          blocks per thread), s128 / b257r (88: three blocks in k_jacobi_ahead, two in k_jacobi_seat),
                                          e90 (three in both);  w63, w64, w65, Lg 130, 200, 300: partial, exact and several 64-column tiles
  blocked form (n_cap >= 129)             b129, b192, b193 (r0 = 15, 16, 17: the 16-wide column groups and 16 x 16 tiles), b257
                                          (r0 = 50), b257r (88): under EACH capacity the counts 2, 63, 64, 65, 128, 129, 191, 192, 193, cap - 1, cap that
                                          do not exceed it; full130: n == Lg
Not reachable, as read (csrc/gpet_api_batch.hip, setup_struct_basis): a basis of full rank.  A batch whose basis reaches the
factor capacity (rank >= r_cap = min(factor_cap, Lg)) is not structured, and r0 == Lg is such a rank: RBF with a short length
scale and Matern-2.5 at Lg = 64 and 65 are asserted to leave the path at creation.  Ranks 83 .. 87 have no length scale with a
safe margin on these widths; the switch 82 | 84 is reached by 82 and 88.
The warm form of stage 122 cannot be reached by set_obs + stages: set_obs clears wq_tag and the iteration counter, and
jac_warm_source needs iteration >= 1 with the previous iteration's tag.  It is reached through two gpet_trace_iterate(1) calls:
the counter then stands at 2 with iteration 1's eigenvectors tagged, and stages 120 .. 123 run on the observation set the loop
left, read back from the device (test_warm_and_cold_jacobi_after_two_loop_iterations).
Scaling of sigma_f by powers of two is NOT a test here: K = amp rho + noise + jitter is not homogeneous in amp with the noise
fixed, so H and the rows do not scale by powers of two; tests/test_gpu_factor_injected.py holds the scaling of the eigen stage.

Measured on an MI355X (largest device error / bound over all cases of a class):
  small form (s100, s128, s100c40)       L 0.36  alpha 0.19  q_orth 0.054   q_rec 0.015  H 0.54  mean 0.54    rec 0.34    orth 0.035   evnorm 0.034    e2e_cov 0.084  e2e_mean 0.56
  K extents, Jacobi classes (e.., w..)   L 0.29  alpha 0.22  q_orth 0.0014  q_rec 0.022  H 0.58  mean 0.20    rec 0.07    orth 0.0014  evnorm 0.0017   e2e_cov 0.067  e2e_mean 0.54
  blocked form (b129 .. b257r)           L 0.54  alpha 0.29  q_orth 0.0012  q_rec 0.015  H 0.64  mean 0.58    rec 0.12    orth 0.0005  evnorm 0.0018   e2e_cov 0.061  e2e_mean 0.54
  n == Lg (full64, full130)              L 0.12  alpha 0.001 q_orth 0.045   q_rec 0.022  H 0.14  mean 0.0012  rec 0.0015  orth 0.10    evnorm 0.0004   e2e_cov 9e-06  e2e_mean 3e-10
  mixed batch                            L 0.11  alpha 0.017 q_orth 0.054   q_rec 0.014  H 0.39  mean 0.018   rec 0.34    orth 0.025   evnorm 0.025    e2e_cov 0.20   e2e_mean 0.033
  Jacobi forms (s100, e80, e82, e90)     H 0.54  rec 0.004  orth 0.028  evnorm 0.014  e2e_cov 0.006   (log and no-log forms of a variant: the same bits)
  warm | cold after two iterations       rec 0.0059 | 0.0021 on bit-equal H (asserted; the rows differ in bits); 5 sweeps each (8 training points)
  q_norm <= 0.045, the prelude <= 0.02, the sign rule and the order exact everywhere; the Jacobi reports at most 9 sweeps.
What the first run found, with the kernels as they were:
* full130 (n == Lg = 130, the blocked fit, K the jitter away from singular at a length scale of 11 columns): L 1.41 -- the loop's
  blocked Cholesky missed px's backward error bound of the factor; every bound of the structured stages themselves held (H 0.35).
  Read in csrc/gpet_k_fit.inc: the rows below a diagonal block came from k_chol_trsm, a product with the block's explicit inverse,
  the form px's docstring names as not covered by the bound (its error grows with the block's condition number, 1e7 here;
  px's own jitter-only sets, at a length scale of 2 columns, stay inside).  launch_fit_blocked now takes k_chol_trsm_sub, the
  substitution the converged fits' objective already used: L 0.11, and 0.54 at most over the blocked families.  The fit of
  902 training points takes 1.35 ms instead of 1.09 ms for it, that of 1502 points 2.30 instead of 1.86 ms (stage 120, MI355X).
"""
import numpy as np
import pytest

from tests import factor_exact as fx
from tests import posterior_exact as px
from tests import struct_exact as sx
from tests.injected_batch import make_batch
from tests.test_gpu_factor_injected import options

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def image():
    return np.random.default_rng(sx.N_IMG).random((px.M_ROWS, sx.N_IMG)).astype(np.float32)


def kernel_options(c):
    return {'kernel': 'RBF', 'sigma_f': px.SIGMA_F, 'length_scale': c.length}


def build(amd, ctx, cases, opts=None, structured=True, delta_x=16):
    """One batch with the Cases as its edges on one shared image; capacities, spans and -- for a structured batch -- the rank
    class of every edge are asserted."""
    with options(amd._lib, opts or {}):
        b = make_batch(amd, ctx, image(), [(c.x_st, c.Lg) for c in cases], 64, delta_x=delta_x, fix_endpoints=True,
                       kernel=[kernel_options(c) for c in cases], obs_cap=[c.n_cap - 2 for c in cases],
                       factor_cap=[c.factor_cap for c in cases], inits=[c.points()[0] for c in cases])
    try:
        for e, c in enumerate(cases):
            inf = b.info(e)
            assert (inf["n_cap"], inf["Lg"]) == (c.n_cap, c.Lg), (c, inf)
            if structured:
                assert inf["structured"] == 1 and c.r0[0] <= inf["r0"] <= c.r0[1], (c, inf)
    except BaseException:
        b.close()
        raise
    return b


def inject(b, cases):
    for e, c in enumerate(cases):
        b.set_obs(e, c.points()[1])
    undone(b)


def undone(b):
    for e in range(b.B):
        s = b.scalars(e)
        if s.done:
            s.done = 0
            b.write_scalars(s, e)


def run_stages(L, b, cases):
    """Stages 120 .. 123; what every edge holds, as sx.check_all takes it."""
    b.profile_stage(120, 1)
    b.profile_stage(121, 1)
    got = []
    for e, c in enumerate(cases):
        s = b.scalars(e)
        assert (s.status, s.n, s.rank) == (L.OK, c.n, b.info(e)["r0"]), (c, s.status, s.n, s.rank)
        assert np.array_equal(b.read(L.BUF_X_TRAIN, e), c.training()[0]), c
        got.append(dict(Q0=b.read(L.BUF_STRUCT_Q0, e), lam0=b.read(L.BUF_STRUCT_LAM0, e), y_s=s.y_s, amp=s.amp, y_mean=s.y_mean, y_std=s.y_std,
                        y_train=b.read(L.BUF_Y_TRAIN, e), L=b.read(L.BUF_CHOL, e), alpha=b.read(L.BUF_ALPHA, e), H=b.read(L.BUF_STRUCT_H, e),
                        mean=b.read(L.BUF_MEAN, e)))
    b.profile_stage(122, 1)
    b.profile_stage(123, 1)
    for e, g in enumerate(got):
        g["A"], g["ev"], g["sweeps"] = b.read(L.BUF_FACTOR, e), b.read(L.BUF_EIGVALS, e), int(b.scalars(e).lml)
    return got


def check(tag, cases, got):
    worst = {}
    for c, g in zip(cases, got):
        r, _ = sx.check_all(c, g)
        print("%-22s %-16s sweeps %d  %s" % (tag, c, g["sweeps"], "  ".join("%s %.3g" % kv for kv in r.items())))
        assert px.within(r), (tag, c, {k: v for k, v in r.items() if not v <= 1})
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("WORST %-22s %s" % (tag, "  ".join("%s %.3g" % kv for kv in worst.items())))
    return worst


@pytest.mark.parametrize("fam", sorted(sx.FAMILIES))
def test_every_stage_of_a_family_inside_its_bounds(amd, ctx, fam):
    L = amd._lib
    cases = list(sx.cases_of(fam))
    b = build(amd, ctx, cases)
    try:
        inject(b, cases)
        check(fam, cases, run_stages(L, b, cases))
    finally:
        b.close()


# ---- leaving the path ----------------------------------------------------------------------------------------------------------

def _refused(L, b):
    for stage in (120, 121, 122, 123):
        with pytest.raises(L.GpetError) as err:
            b.profile_stage(stage, 1)
        assert err.value.code == L.ERR_BAD_ARG, stage
    for which in (L.BUF_STRUCT_Q0, L.BUF_STRUCT_LAM0, L.BUF_STRUCT_H):
        with pytest.raises(L.GpetError) as err:
            b.read(which, 0)
        assert err.value.code == L.ERR_BAD_ARG, which


@pytest.mark.parametrize("Lg", [64, 65])
@pytest.mark.parametrize("kernel", ["RBF", "M25"])
def test_full_rank_basis_is_not_structured(amd, ctx, Lg, kernel):
    """r0 == Lg reaches the factor capacity: the batch is created off the path (module docstring), the stages and the path's
    buffers are refused, and the generic stages meet px's bounds."""
    L = amd._lib
    from tests.test_gpu_posterior_injected import build as px_build, check_loop_edge, inject_loop
    c = px.Case(64, 2, 40, Lg, px.width_for(64), length=0.5)
    b = px_build(amd, ctx, [c], kernel, [True])
    try:
        assert b.info(0)["structured"] == 0
        _refused(L, b)
        inject_loop(b, [c])
        b.fit_predict(want_cov=True)
        check_loop_edge(L, b, 0, c, kernel, True)
    finally:
        b.close()


def test_an_off_grid_observation_takes_the_batch_off_the_path(amd, ctx):
    """One observation outside [x_st, x_en]: gpet_batch_set_obs clears the batch's flag while the edges keep theirs and their
    basis.  As read (csrc/gpet_api_stages.hip), stages 120 .. 123 launched the structured kernels whatever the batch's flag said,
    and k_struct_H / k_structB_build would then have gathered Q0[a * Lg + (x - x_st)] outside the basis: gpet_profile_stage now
    refuses them before any launch.  The unguarded form was never run.  The generic stages meet px's bounds; the factor
    reconstructs the device's covariance within fx's bound."""
    L = amd._lib
    from tests.test_gpu_posterior_injected import build as px_build, check_loop_edge, inject_loop
    c = px.Case(64, 2, 40, 65, px.width_for(64))
    init, obs = c.points()
    assert np.any((obs[:, 0] < c.x_st) | (obs[:, 0] >= c.x_st + c.Lg))
    b = px_build(amd, ctx, [c], "RBF", [True])
    try:
        assert b.info(0)["structured"] == 1 and b.read(L.BUF_STRUCT_Q0, 0).shape == (b.info(0)["r0"], c.Lg)
        for which in (L.BUF_STRUCT_Q0, L.BUF_STRUCT_LAM0, L.BUF_STRUCT_H):  # read only, on the path too
            with pytest.raises(L.GpetError) as err:
                b.write(which, b.read(which, 0), 0)
            assert err.value.code == L.ERR_BAD_ARG, which
        inject_loop(b, [c])
        assert b.info(0)["structured"] == 0
        _refused(L, b)
        with pytest.raises(L.GpetError) as err:
            b.write(L.BUF_STRUCT_H, np.zeros(4), 0)
        assert err.value.code == L.ERR_BAD_ARG
        b.fit_predict(want_cov=True)
        check_loop_edge(L, b, 0, c, "RBF", True)
        b.factor()
        A, cov, rank = b.read(L.BUF_FACTOR, 0), b.read(L.BUF_COV, 0), b.scalars(0).rank
        res = fx.f64(abs(fx.ext(A).T @ fx.ext(A) - fx.ext(cov)))
        frac = float((res / fx.bound_matrix(cov, rank)).max())
        print("off the path: rank %d, |A^T A - cov| / bound %.3g" % (rank, frac))
        assert frac <= 1.0
    finally:
        b.close()


# ---- batches of mixed edges, shared bases ------------------------------------------------------------------------------------------

def _mixed():
    """Two length scales (r0 = 38 and 30 below the batch's r0_max), two edge lengths, two first columns; one capacity."""
    return [sx.Case("mixed", 130, 100, 40, 11.125, (33, 48), seed=1), sx.Case("mixed", 130, 100, 64, 14.75, (1, 32), seed=2),
            sx.Case("mixed", 200, 100, 41, 61.5, (1, 32), seed=3), sx.Case("mixed", 130, 100, 65, 11.125, (33, 48), seed=4, x_st=100)]


def test_mixed_batch_equals_its_edges_alone(amd, ctx):
    """Edges of smaller rank than the batch's r0_max multiply zero rows in k_struct_rows<MT, KS> and sit in a Jacobi sized for the
    largest: factor, eigenvalues, mean, H and the basis must be, bit for bit, those of the same edge as a batch of one (every
    kernel of the path sizes its arithmetic by the edge's own n and r0; the batch's maxima size only grids and LDS)."""
    L = amd._lib
    cases = _mixed()
    b = build(amd, ctx, cases)
    try:
        inject(b, cases)
        together = run_stages(L, b, cases)
        check("mixed", cases, together)
    finally:
        b.close()
    for e, c in enumerate(cases):
        b = build(amd, ctx, [c])
        try:
            inject(b, [c])
            alone = run_stages(L, b, [c])[0]
        finally:
            b.close()
        for k in ("Q0", "lam0", "L", "alpha", "H", "mean", "A", "ev"):
            assert np.array_equal(together[e][k], alone[k]), (c, k, float(np.abs(together[e][k] - alone[k]).max()))


def test_eleven_basis_classes_with_repeats_share_the_right_bits(amd, ctx):
    """Fifteen edges of eleven (length scale) classes: repeats inside the look-back of eight read the representative's basis,
    the repeat of class 0 after nine others founds a class of its own.  Every edge's Q0 and lam0 are the bits of its own
    single-edge batch."""
    L = amd._lib
    lengths = [8.0 + 0.5 * k for k in range(11)]
    order = list(range(11)) + [0, 5, 10, 2]
    cases = [sx.Case("classes", 64, 64, 2, lengths[k], (1, 32)) for k in order]
    b = build(amd, ctx, cases)
    try:
        Q = [(b.read(L.BUF_STRUCT_Q0, e), b.read(L.BUF_STRUCT_LAM0, e)) for e in range(len(cases))]
    finally:
        b.close()
    alone = {}
    for k in range(11):
        b1 = build(amd, ctx, [cases[k]])
        try:
            alone[k] = (b1.read(L.BUF_STRUCT_Q0, 0), b1.read(L.BUF_STRUCT_LAM0, 0))
        finally:
            b1.close()
    assert len({a[0].shape[0] for a in alone.values()}) >= 2  # (more than one rank among the classes)
    for e, k in enumerate(order):
        assert Q[e][0].shape == alone[k][0].shape and np.array_equal(Q[e][0], alone[k][0]) and np.array_equal(Q[e][1], alone[k][1]), (e, k)


# ---- the forms of the Jacobi on H ------------------------------------------------------------------------------------------------

FORMS = {"default": ({}, {}), "nolog": ({"jlog_max_b": 0}, {}), "logw0": ({}, {"jacobi_logw": 0}), "seat": ({"jacobi_variant": 0}, {}),
         "seat-nolog": ({"jacobi_variant": 0, "jlog_max_b": 0}, {})}


@pytest.mark.parametrize("fam", ["s100", "e80", "e82", "e90"])
def test_jacobi_forms_on_the_same_set(amd, ctx, fam):
    """scaled_out = 1 in its log / no-log forms and both variants, cold (iteration 0), on one injected set per rank class: each
    inside the bounds; the log and no-log forms of one variant apply the same rotations with the same arithmetic
    (tests/test_gpu_stages.py::test_jacobi_rotation_log_form_equals_lds_form) and are compared bit for bit."""
    L = amd._lib
    cases = [sx.cases_of(fam)[-1]]
    out = {}
    for name, (opts, batch_opts) in FORMS.items():
        b = build(amd, ctx, cases, opts)
        try:
            for k, v in batch_opts.items():
                b.set_option(k, v)
            inject(b, cases)
            out[name] = run_stages(L, b, cases)
            check("%s %s" % (fam, name), cases, out[name])
        finally:
            b.close()
    for a, o in (("default", "nolog"), ("default", "logw0"), ("seat", "seat-nolog")):
        for k in ("H", "A", "ev"):
            assert np.array_equal(out[a][0][k], out[o][0][k]), (fam, a, o, k)


def test_warm_and_cold_jacobi_after_two_loop_iterations(amd, ctx):
    """The warm form (module docstring): two loop iterations of one each leave the counter at 2 and iteration 1's eigenvectors
    tagged; stages 120 .. 123 then run on the set the loop left -- larger than the injected one --, warm (jacobi_warm = 1, the
    default: r0 <= 80) and, on a second batch brought to the same state, cold (jacobi_warm = 0).  Both inside the bounds."""
    L = amd._lib
    c0 = sx.cases_of("s100")[1]  # three training points
    sweeps, got = {}, {}
    for warm in (1, 0):
        b = build(amd, ctx, [c0], delta_x=4)  # (32 bins: two iterations do not finish the edge)
        try:
            b.set_option("jacobi_warm", warm)
            b.set_obs(0, c0.points()[1])
            b.iterate([7], 1)
            b.iterate([7], 1)
            assert b.info(0)["structured"] == 1
            s = b.scalars(0)
            obs = b.read(L.BUF_OBS, 0)
            # the precondition of jac_warm_source as far as the interface shows it: iteration 2, and iteration 1 factored at the
            # rank of the basis (its tag is iteration + 65536 * rank)
            assert s.iter == 2 and s.status == L.OK and s.rank == b.info(0)["r0"] <= 80 and obs.shape[0] > c0.n - 2, (s.iter, s.status, s.rank, obs.shape)
            c = sx.HeldCase("loop", c0.Lg, c0.x_st, c0.n_cap, c0.length, c0.points()[0], obs)
            undone(b)
            got[warm] = run_stages(L, b, [c])[0]
            check("after two iterations, jacobi_warm %d" % warm, [c], [got[warm]])
            sweeps[warm] = got[warm]["sweeps"]
        finally:
            b.close()
    print("sweeps warm %d, cold %d" % (sweeps[1], sweeps[0]))
    # the two batches came to the same state by the same loop (the loop's own Jacobi differs, its selected pixels do not): the
    # same H goes into stage 122 -- and only a start from iteration 1's eigenvectors can then leave other bits than the cold
    # start does.  Were the warm source not taken (a wrong tag, a rank outside the warm class), both runs would be cold and equal
    for k in ("Q0", "lam0", "L", "alpha", "H", "mean"):
        assert np.array_equal(got[1][k], got[0][k]), k
    assert not np.array_equal(got[1]["A"], got[0]["A"])
    assert sweeps[1] <= sweeps[0]
