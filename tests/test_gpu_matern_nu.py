"""General-nu Matern on the device (matern_gen's quadrature through every kernel that builds a covariance) against the
exact float64 reference of tests/matern_exact.py: the loop's posterior (lag table), the converged fit's posterior,
objective and gradient of every objective kernel, the converged fit itself, whole traces, and the accepted range of nu."""
import math

import numpy as np
import pytest
import scipy.optimize

from oracle import gpet_oracle as orc
from tests import final_fit_inputs as ff
from tests import matern_exact as me

pytestmark = pytest.mark.gpu

NU_GRID = [0.01, 0.03, 0.06, 0.3, 0.7, 1.0, 1.2, 2.0, 3.0, 3.5, 5.0, 7.5, 12.0, 20.0, 50.0, 170.0, 171.0, 171.5, 172.0,
           500.0]
CONTROLS = [0.5, 1.5, 2.5]


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def _image(N, seed):
    img, truth = orc.synth_sinusoid_image(N, seed)
    return orc.comp_grad_img(img, orc.kernel_builder((11, 5))), truth


def _kw(nu, length_scale=10, delta_x=6):
    return dict(kernel_options={'kernel': 'Matern', 'nu': nu, 'sigma_f': 15, 'length_scale': length_scale}, noise_y=1,
                N_samples=128, score_thresh=1, delta_x=delta_x, keep_ratio=0.1, pixel_thresh=3, seed=5,
                fix_endpoints=True)


@pytest.fixture
def exact_oracle(monkeypatch):
    """The oracle with its general-nu correlation replaced by the exact reference (sklearn's conventions kept)."""
    orig = orc.corr_matrix

    def corr(kernel_type, nu, xa, xb, length_scale):
        if kernel_type == "Matern" and nu not in (0.5, 1.5, 2.5, np.inf):
            return me.sklearn_convention(nu, xa, xb, length_scale, False)[0]
        return orig(kernel_type, nu, xa, xb, length_scale)
    monkeypatch.setattr(orc, "corr_matrix", corr)
    return orc


@pytest.fixture
def sklearn_oracle(monkeypatch):
    """The oracle with sklearn's k(X) convention restored where it calls corr_matrix(x, x) with one array for both sides:
    the diagonal is 1 (kernels.py Matern: squareform, then fill_diagonal), not rho(eps).  The oracle's objective and
    converged fit leave rho(eps) there -- 1.0 to the last bit only for nu >~ 1, 0.9885 at nu = 0.06."""
    orig = orc.corr_matrix

    def corr(kernel_type, nu, xa, xb, length_scale):
        R = orig(kernel_type, nu, xa, xb, length_scale)
        if xa is xb:
            np.fill_diagonal(R, 1.0)
        return R
    monkeypatch.setattr(orc, "corr_matrix", corr)
    return orc


def _obs(truth, N, n_obs, rng, dup=True):
    cols = np.sort(rng.choice(np.arange(1, N - 1), size=n_obs, replace=False))
    if dup:  # duplicate columns: a zero distance off the diagonal of k(X, X), and the endpoint columns again
        cols = np.sort(np.concatenate([cols, cols[:2], [0, N - 1]]))
    return np.stack([cols, np.clip(truth[cols, 0] + rng.integers(-3, 4, size=cols.size), 0, N - 1)], axis=1)


@pytest.mark.parametrize("nu", NU_GRID + CONTROLS)
@pytest.mark.parametrize("N,n_obs", [(96, 12), (500, 40), (500, 200)])
def test_loop_posterior_against_exact(amd, ctx, exact_oracle, nu, N, n_obs):
    """fit_predict(want_cov=True) of the loop (integer lags through the per-edge table rho_tab): K = L L^T to 1e-13 of
    the amplitude, mean to 1e-8, std and covariance to 1e-5 of the exact posterior.  n <= 128 is k_fit; 200 training
    points take the blocked Cholesky, k_kstar_build, k_vsolve_mfma and k_pred_colsum_big."""
    L = amd._lib
    grad, truth = _image(N, 3)
    init = truth[[0, -1], :][:, [1, 0]]
    tr = amd.GP_Edge_Tracing(init, grad, **_kw(nu, delta_x=2 if n_obs > 100 else 6), _ctx=ctx)
    obs = _obs(truth, N, n_obs, np.random.default_rng(N + n_obs))
    b = tr._batch
    b.set_obs(0, obs)
    b.fit_predict(want_cov=True)
    p = orc.resolve_params(init, grad, **_kw(nu, delta_x=2 if n_obs > 100 else 6))
    _, info = exact_oracle.fit_predict_samples(p["init"], obs, p, 11, want_all=True)
    s = b.scalars()
    assert s.n == info["x"].shape[0]
    assert np.array_equal(b.read(L.BUF_X_TRAIN), info["x"])
    Lc = b.read(L.BUF_CHOL)
    amp = s.amp
    assert np.all(np.isfinite(Lc))
    # (above nu = 170, in the log form, the products nu s in the quadrature's exponents carry ~1e-13 of rounding)
    np.testing.assert_allclose(np.tril(Lc) @ np.tril(Lc).T, info["fit"]["K"], rtol=0,
                               atol=(1e-13 if nu <= 170 else 1e-12) * amp)
    pr = info["pred"]
    np.testing.assert_allclose(b.read(L.BUF_MEAN), pr["mean"], rtol=1e-8, atol=1e-8 * np.abs(pr["mean"]).max())
    np.testing.assert_allclose(b.read(L.BUF_STD), pr["std"], rtol=1e-5, atol=1e-8)
    cov = b.read(L.BUF_COV)
    np.testing.assert_allclose(cov, pr["cov"], rtol=1e-5, atol=1e-9 * np.abs(pr["cov"]).max())


def _lml_batch_problems(amd, ctx, nu, specs, N):
    grad, truth = _image(N, 5)
    init = truth[[0, -1], :][:, [1, 0]]
    kw = _kw(nu, delta_x=2)
    del kw["seed"]  # (a batch takes one seed per edge)
    bt = amd.GP_Edge_Tracing_Batch([init] * len(specs), grad.astype(np.float32), list(range(len(specs))), **kw, _ctx=ctx)
    b = bt._batch
    rng = np.random.default_rng(int(1000 * nu) % 9973)
    off = rng.uniform(0.05, 0.45, size=N)  # per-column shift of the off-lattice sets (duplicates stay duplicates)
    prs = []
    for e, (n, lattice) in enumerate(specs):
        k = max(n - 4, 1)
        # (column 1 next to the endpoint at 0: the smallest gap is one pixel, so the pixel columns form a lattice)
        cols = np.sort(np.concatenate([[1], rng.choice(np.arange(2, N - 1), size=k - 1, replace=False)]))
        cols = np.sort(np.concatenate([cols, cols[:n - 2 - k]])) if n - 2 > k else cols[:n - 2]
        x = cols if lattice else cols + off[cols]
        obs = np.stack([x, truth[cols, 0] + rng.integers(-3, 4, size=cols.size)], axis=1).reshape(-1, 2)
        pr = ff.prepare(np.asarray(init)[np.argsort(np.asarray(init)[:, 0])], obs, np.arange(N), True)
        assert pr["xs"].shape[0] == n
        b.final_set_training(e, pr["xs"], pr["yt"], pr["w"])
        # (slot 10 of the edge's parameters: the largest lag of the lattice its training set sits on, -1 for none)
        assert (b.read(amd._lib.BUF_FIN_PAR, e)[10] >= 0) == lattice, (n, lattice)
        prs.append(pr)
    return b, prs


def _thetas(rng, P):
    th = ff.BOUNDS[:, 0] + (ff.BOUNDS[:, 1] - ff.BOUNDS[:, 0]) * rng.uniform(size=(P, 3))
    th[:, 2] = np.log(rng.uniform(1e-2, 1.0, size=P))
    th[0] = np.log([5.0, 5.0, 1.0])
    th[1] = [ff.BOUNDS[0, 1], ff.BOUNDS[1, 0], np.log(0.5)]  # bounds: largest amplitude, shortest length scale
    th[2] = [ff.BOUNDS[0, 0], ff.BOUNDS[1, 1], 0.0]          # smallest amplitude, longest length scale
    return th


def _check_objective(f, gr, th, pr, nu, what):
    wrong = []
    for i in range(th.shape[0]):
        lml, g = me.lml_and_grad(th[i], pr["xs"], pr["yt"], pr["w"], nu)
        if not np.isfinite(lml):
            if not (np.isinf(f[i]) and f[i] > 0):
                wrong.append((what, i, "not PD in the reference", f[i]))
            continue
        if not np.isfinite(f[i]):
            wrong.append((what, i, "not finite", f[i], -lml))
            continue
        if not (abs(f[i] + lml) <= 1e-9 * max(1.0, abs(lml)) and
                np.all(np.abs(gr[i] + g) <= 1e-7 * (1.0 + np.abs(g).max()))):
            wrong.append((what, i, float(f[i]), float(-lml), gr[i].tolist(), (-g).tolist()))
    assert not wrong, wrong


# (n, training set on a lattice): launch_lml sends lattice sets of n <= 108 to k_lml16; other sets of n <= 128 to k_lml,
# or to k_lml2 when the launch has lml_two_tiles_from problems or more; 128 < n <= 250 always to k_lml2; n > 250 to the
# blocked path
LML_SPECS = [(3, True), (17, True), (64, True),
             (3, False), (17, False), (64, False), (128, True),
             (129, True), (250, True),
             (251, True), (400, True)]
LML_GROUPS = (("k_lml16", [0, 1, 2], [None]),
              ("k_lml / k_lml2", [3, 4, 5, 6], [1 << 29, 1]),
              ("k_lml2", [7, 8], [None]),
              ("blocked", [9, 10], [None]))


@pytest.mark.parametrize("nu", [0.01, 0.03, 0.06, 0.3, 0.7, 1.2, 3.5, 7.5, 20.0, 171.0, 171.5, 172.0, 500.0, 2.5])
def test_objective_and_gradient_every_kernel_against_exact(amd, ctx, nu):
    """lml_batch against the exact objective and its exact gradient (sklearn's is a forward difference): k_lml16 for
    lattice sets of n = 3, 17, 64; k_lml and then k_lml2 (option lml_two_tiles_from) for off-lattice sets of n = 3, 17,
    64 and a lattice set of 128; k_lml2 at 129 and 250; the blocked path at 251 and 400.  Duplicate inputs in every set
    of more than 4 points; theta at the bounds."""
    L = amd._lib
    b, prs = _lml_batch_problems(amd, ctx, nu, LML_SPECS, 808)
    rng = np.random.default_rng(11)
    for kernel, group, opts in LML_GROUPS:
        for opt in opts:
            old = L.set_option("lml_two_tiles_from", opt) if opt is not None else None
            try:
                for e in group:
                    th = _thetas(rng, 6)
                    f, gr = b.lml_batch(np.full(th.shape[0], e, dtype=np.int32), th)
                    _check_objective(f, gr, th, prs[e], nu, (kernel, LML_SPECS[e], opt))
            finally:
                if opt is not None:
                    L.set_option("lml_two_tiles_from", old)


@pytest.mark.parametrize("nu", [0.06, 0.7, 5.0, 20.0, 171.0, 172.0])
def test_converged_fit_and_lattice_objective_against_exact(amd, ctx, nu):
    """final_fit_all: the k_lml16 lattice objective (lml_batch after the fit has set the lattice) against the exact
    objective; at nu in {0.7, 5, 20} the fit's theta against scipy L-BFGS-B on the exact objective from the same 13
    start points (log c and log l to 1e-4), its mean / std and final_cov against the exact posterior at that theta (final_cov
    finite and symmetric at every nu)."""
    L = amd._lib
    N = 96
    grad, truth = _image(N, 3)
    init = truth[[0, -1], :][:, [1, 0]]
    tr = amd.GP_Edge_Tracing(init, grad, **_kw(nu), _ctx=ctx)
    obs = _obs(truth, N, 14, np.random.default_rng(2))
    b = tr._batch
    b.set_obs(0, obs)
    seed = 17
    mean, std, theta, fmin, rounds = b.final_fit_all([seed])
    train = b.read(L.BUF_FIN_TRAIN)
    pr = ff.prepare(tr.init, obs, tr.x_grid, tr.fix_endpoints)
    n = pr["xs"].shape[0]
    assert np.array_equal(train[0, :n], pr["xs"]) and np.array_equal(train[2, :n], pr["w"])
    assert np.all(np.isfinite(mean[0])) and np.all(np.isfinite(std[0])) and np.isfinite(fmin[0])
    th = _thetas(np.random.default_rng(4), 8)
    f, gr = b.lml_batch(np.zeros(th.shape[0], dtype=np.int32), th)
    _check_objective(f, gr, th, pr, nu, "lattice")
    b.final_cov()
    cov = b.read(L.BUF_COV)
    assert cov.shape == (N, N) and np.all(np.isfinite(cov)) and np.array_equal(cov, cov.T)
    if nu not in (0.7, 5.0, 20.0):
        return
    starts = b.read(L.BUF_FIN_STARTS)

    def obj(t):
        lml, g = me.lml_and_grad(t, pr["xs"], pr["yt"], pr["w"], nu)
        return -lml, -g
    res = [scipy.optimize.minimize(obj, t0, method="L-BFGS-B", jac=True, bounds=list(map(tuple, ff.BOUNDS)))
           for t0 in starts]
    best = res[int(np.argmin([r.fun for r in res]))]
    np.testing.assert_allclose(theta[0][:2], best.x[:2], rtol=0, atol=1e-4)
    np.testing.assert_allclose(fmin[0], best.fun, rtol=1e-7, atol=1e-7)
    # posterior at the device's theta (sklearn_gpr.py:381-436 on the standardised set), mapped back as the device does
    c, ell, nl = np.exp(theta[0])
    xq = (pr["xg"] - pr["X_m"]) / pr["X_s"]
    post = me.posterior(pr["xs"], pr["yt"], nl * pr["w"], c, ell, nu, xq)
    m_ref = pr["y_s"] * (pr["s2"] * post["mean"] + pr["m2"]) + pr["y_m"]
    np.testing.assert_allclose(mean[0][:N], m_ref, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(std[0][:N], pr["s2"] * post["std"], rtol=1e-5, atol=1e-6)
    # the covariance of the same posterior (sklearn_gpr.py:398-403): in the units of the std, not rescaled either
    np.testing.assert_allclose(cov, pr["s2"] ** 2 * post["cov"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("nu", [0.06, 0.3, 0.7, 1.2, 7.5])
def test_full_trace_vs_oracle_general_nu(amd, ctx, sklearn_oracle, nu):
    """Whole trace against the oracle (sklearn's own formula, finite at these nu; k(X)'s diagonal 1 as sklearn has it):
    observation sets per iteration, iteration count and trace bit-exact, as test_full_trace_vs_oracle."""
    N = 96
    grad, truth = _image(N, 3)
    init = truth[[0, -1], :][:, [1, 0]]
    kw = _kw(nu)
    rec = []
    et_o, _, info = sklearn_oracle.trace(init, grad, record=rec, sign_convention="harmonic", **kw)
    tr = amd.GP_Edge_Tracing(init, grad, **kw, _ctx=ctx)
    et, (_, all_obs, _) = tr(return_lines=True)
    assert tr._n_iter == info["n_iter"]
    for i, r in enumerate(rec):
        assert np.array_equal(all_obs[i + 1], r["obs_out"]), "iteration %d" % i
    assert np.array_equal(et, et_o)


@pytest.mark.parametrize("nu", [20.0, 50.0, 171.0, 171.5, 172.0, 500.0])
def test_full_trace_large_nu_against_exact_posterior(amd, ctx, nu):
    """At nu >= 20 sklearn's formula is not finite at zero distance (test_matern_exact.py), so there is no oracle: the
    trace must converge inside the image with every column traced, and its credible interval must be the exact
    posterior of its own last observation set at its own optimum theta (mean and std as in the converged-fit test)."""
    L = amd._lib
    N = 96
    grad, truth = _image(N, 3)
    init = truth[[0, -1], :][:, [1, 0]]
    tr = amd.GP_Edge_Tracing(init, grad, **dict(_kw(nu), return_std=True), _ctx=ctx)
    et, (lower, upper) = tr()
    assert et.shape == (N, 2)
    assert np.array_equal(et[:, 1], np.arange(N))
    assert np.all((et[:, 0] >= 0) & (et[:, 0] < N))
    assert 1 <= tr._n_iter < 200
    assert np.all(np.isfinite(lower)) and np.all(np.isfinite(upper))
    b = tr._batch
    pr = ff.prepare(tr.init, b.read(L.BUF_OBS), tr.x_grid, tr.fix_endpoints)
    n = pr["xs"].shape[0]
    train = b.read(L.BUF_FIN_TRAIN)
    assert np.array_equal(train[0, :n], pr["xs"]) and np.array_equal(train[2, :n], pr["w"])
    c, ell, nl = np.exp(tr._theta)
    xq = (pr["xg"] - pr["X_m"]) / pr["X_s"]
    post = me.posterior(pr["xs"], pr["yt"], nl * pr["w"], c, ell, nu, xq)
    m_ref = pr["y_s"] * (pr["s2"] * post["mean"] + pr["m2"]) + pr["y_m"]
    np.testing.assert_allclose((lower + upper) / 2, m_ref, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose((upper - lower) / 3.92, pr["s2"] * post["std"], rtol=1e-5, atol=1e-6)


def test_matern_nu_inf_is_rbf_and_out_of_range_nu_is_refused(amd, ctx):
    """{'kernel': 'Matern', 'nu': inf} traces exactly what RBF traces (gpet.py:81-82); nu below 0.01 (the quadrature's node
    count grows as 1 / nu), NaN and nu above 1000 are refused at construction with ERR_UNSUPPORTED; nu = 1000 is accepted."""
    L = amd._lib
    N = 64
    grad, truth = _image(N, 4)
    init = truth[[0, -1], :][:, [1, 0]]
    kw = _kw(np.inf)
    et_inf = amd.GP_Edge_Tracing(init, grad, **kw, _ctx=ctx)()
    kw_rbf = dict(kw, kernel_options={'kernel': 'RBF', 'sigma_f': 15, 'length_scale': 10})
    assert np.array_equal(et_inf, amd.GP_Edge_Tracing(init, grad, **kw_rbf, _ctx=ctx)())
    for bad in (0.0, -1.0, 1e-300, 0.0099, math.nan, 1000.5, 1e6):
        with pytest.raises(L.GpetError) as ei:
            amd.GP_Edge_Tracing(init, grad, **_kw(bad), _ctx=ctx)
        assert ei.value.code == L.ERR_UNSUPPORTED, bad
    tr = amd.GP_Edge_Tracing(init, grad, **_kw(1000.0), _ctx=ctx)
    b = tr._batch
    b.set_obs(0, _obs(truth, N, 8, np.random.default_rng(1)))
    b.fit_predict(want_cov=True)
    assert np.all(np.isfinite(b.read(L.BUF_MEAN))) and np.all(np.isfinite(b.read(L.BUF_COV)))
