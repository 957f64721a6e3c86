"""Host tests of tests/posterior_exact.py, the extended-precision reference of the posterior tests: a 3-point case worked out with
``decimal`` at 60 digits from explicit formulas (no loops shared with the helper), in both of the helper's arithmetics; the
kernel-function rounding c_k against numpy's own float64 evaluation; and, on every training set of the table the device tests run
(tests/test_gpu_posterior_injected.py), the float64 oracle (oracle.gp_fit / gp_predict, LAPACK) inside every bound, the sharpness
the inputs must keep, and the distance of every K from singular.  Each test prints the ratios it measured (pytest -s)."""
import decimal
from decimal import Decimal as D

import numpy as np
import pytest
import scipy.linalg

from oracle import gpet_oracle as orc
from tests import posterior_exact as px

HAND = decimal.Context(prec=60)


def _dec(v):
    """An extended number of either arithmetic as a 60-digit Decimal (exactly: a longdouble is a binary fraction)."""
    if isinstance(v, D):
        return v
    hi = float(v)
    lo = float(v - px.LD(hi))
    return HAND.add(HAND.create_decimal(hi), HAND.create_decimal(lo))


@pytest.mark.parametrize("use_decimal", [False, True], ids=["native", "decimal"])
@pytest.mark.parametrize("kernel", ["RBF", "M05", "M15", "M25"])
def test_three_points_by_hand(kernel, use_decimal):
    """x = (0, 2, 5), y_train = (-1, 0.5, 0.25), w = (0.5, 1, 0.5), amp = 2, l = 2, noise = 0.75, jitter = 1/64 (all exact in
    binary), y_mean = 3, y_std = 1.5, grid (1, 5): the 3 x 3 factor, both substitutions, mean, variance and covariance written out."""
    if not use_decimal and px.USE_DECIMAL:
        use_decimal = True  # (no 64-bit mantissa here: the native arithmetic IS the decimal one)
    x, yt, w = np.array([0.0, 2.0, 5.0]), np.array([-1.0, 0.5, 0.25]), np.array([0.5, 1.0, 0.5])
    grid = np.array([1.0, 5.0])
    r = px.posterior(x, yt, w, 2.0, 2.0, 0.75, 1.0 / 64, kernel, px.ext(grid, use_decimal), y_mean=3.0, y_std=1.5,
                     use_decimal=use_decimal)
    with decimal.localcontext(HAND):
        def rho(a, b):
            d = abs(D(a) - D(b)) / 2
            if kernel == "RBF":
                return (-(d * d) / 2).exp()
            if kernel == "M05":
                return (-d).exp()
            k = d * D(3 if kernel == "M15" else 5).sqrt()
            return ((1 + k) if kernel == "M15" else (1 + k + k * k / 3)) * (-k).exp()
        amp, jit, nz = D(2), D(1) / 64, D("0.75")
        k11, k22, k33 = amp + nz * D("0.5") + jit, amp + nz + jit, amp + nz * D("0.5") + jit
        k21, k31, k32 = amp * rho(2, 0), amp * rho(5, 0), amp * rho(5, 2)
        l11 = k11.sqrt()
        l21, l31 = k21 / l11, k31 / l11
        l22 = (k22 - l21 * l21).sqrt()
        l32 = (k32 - l31 * l21) / l22
        l33 = (k33 - l31 * l31 - l32 * l32).sqrt()
        y1, y2, y3 = D(-1), D("0.5"), D("0.25")
        z1 = y1 / l11
        z2 = (y2 - l21 * z1) / l22
        z3 = (y3 - l31 * z1 - l32 * z2) / l33
        a3 = z3 / l33
        a2 = (z2 - l32 * a3) / l22
        a1 = (z1 - l21 * a2 - l31 * a3) / l11
        want = dict(L=[[l11, 0, 0], [l21, l22, 0], [l31, l32, l33]], alpha=[a1, a2, a3], mean=[], var=[], V=[])
        for g in (1, 5):
            c1, c2, c3 = amp * rho(g, 0), amp * rho(g, 2), amp * rho(g, 5)
            v1 = c1 / l11
            v2 = (c2 - l21 * v1) / l22
            v3 = (c3 - l31 * v1 - l32 * v2) / l33
            want["mean"].append(D("1.5") * (c1 * a1 + c2 * a2 + c3 * a3) + 3)
            want["var"].append(amp - (v1 * v1 + v2 * v2 + v3 * v3))
            want["V"].append((v1, v2, v3))
        cov01 = (amp * rho(1, 5) - sum(p * q for p, q in zip(*want["V"]))) * D("2.25")
        tol = D("1e-36") if use_decimal else D("4e-19")  # (a few roundings of 2^-64; K's entries are of size 1)
        worst = D(0)

        def check(got, exact):
            nonlocal worst
            e = abs(_dec(got) - D(exact)) / max(abs(D(exact)), D(1))
            worst = max(worst, e)
            assert e <= tol, (got, exact, e)
        for i in range(3):
            for j in range(3):
                check(r["L"][i, j], want["L"][i][j])
            check(r["alpha"][i], want["alpha"][i])
        for j in range(2):
            check(r["mean"][j], want["mean"][j])
            check(r["var"][j], want["var"][j])
            check(r["cov"][j, j], want["var"][j] * D("2.25"))
        check(r["cov"][0, 1], cov01)
        check(r["cov"][1, 0], cov01)
        check(r["K"][2, 0], k31)
        check(r["K"][1, 1], k22)
    print("three points, %s, %s: worst relative difference %.2g" % (kernel, "decimal" if use_decimal else "longdouble", worst))
    # the grid point on the third training column, whose weight leaves 0.375 + 1/64 of noise there: a variance far below amp
    assert 0 < float(r["var"][1]) < 0.4 and float(r["var"][0]) > float(r["var"][1])


@pytest.mark.parametrize("use_decimal", [False, True], ids=["native", "decimal"])
def test_loop_prelude_by_hand(use_decimal):
    """y = (3, 5, 10): mean 6, variance 26/3; sigma_f = 12."""
    ex, bd = px.loop_prelude(np.array([3.0, 5.0, 10.0]), 12, use_decimal=use_decimal or px.USE_DECIMAL)
    tol = D("1e-36") if (use_decimal or px.USE_DECIMAL) else D("4e-19")
    with decimal.localcontext(HAND):
        y_s = (D(26) / 3).sqrt() + 1
        v = [D(3) / y_s, D(5) / y_s, D(10) / y_s]
        m = D(6) / y_s
        sd = (D(26) / 3).sqrt() / y_s
        for got, want in [(ex["y_s"], y_s), (ex["amp"], D(144) / (y_s * y_s)), (ex["y_mean"], m), (ex["y_std"], sd)] + \
                [(ex["y_train"][i], v[i] - m) for i in range(3)]:
            assert abs(_dec(got) - want) <= tol * max(abs(want), D(1)), (got, want)
    # float64 numpy inside the prelude's bounds
    y = np.array([3.0, 5.0, 10.0])
    ys = float(np.std(y)) + 1.0
    assert px.ratio(ys, ex["y_s"], bd["y_s"]) <= 1 and px.ratio(144 / ys ** 2, ex["amp"], bd["amp"]) <= 1
    assert px.ratio(y / ys - np.mean(y / ys), ex["y_train"], bd["y_train"]) <= 1
    assert px.ratio(float(np.std(y / ys)), ex["y_std"], bd["y_std"]) <= 1
    # a single point: no spread, y_s = 1 and y_std = 1 (sklearn's zero scale)
    ex1, bd1 = px.loop_prelude(np.array([17.0]), 12, use_decimal=use_decimal or px.USE_DECIMAL)
    assert float(ex1["y_s"]) == 1.0 and float(ex1["y_std"]) == 1.0 and float(ex1["y_train"][0]) == 0.0 and float(ex1["amp"]) == 144.0


@pytest.mark.parametrize("kernel", ["RBF", "M05", "M15", "M25"])
@pytest.mark.parametrize("ra,rb", [(1, 1), (1, 3)])
def test_kernel_rounding_covers_a_float64_evaluation(kernel, ra, rb):
    """numpy's float64 evaluation of the kernels' formula, on inputs x / l and ((x - m) / s) / l rounded as the kernels round
    them, stays inside c_k u of the extended value -- with a margin, and c_k itself stays a few units except where the argument
    amplifies it (distant points, whose correlation is tiny)."""
    rng = np.random.default_rng(5)
    xa, xb = rng.integers(0, 640, 300).astype(np.float64), np.arange(200, 330, dtype=np.float64)
    l, m, s = 9.0, 311.7, 187.3
    if rb == 3:
        a, b = ((xa - m) / s) / (l / s), ((xb - m) / s) / (l / s)
        ae, be = ((px.ext(xa) - px.ext(m)) / px.ext(s)) / px.ext(l / s), ((px.ext(xb) - px.ext(m)) / px.ext(s)) / px.ext(l / s)
        ra = 3
    else:
        a, b = xa / l, xb / l
        ae, be = px.ext(xa) / px.ext(l), px.ext(xb) / px.ext(l)
    name, nu = px.KERNELS[kernel]
    got = orc.corr_matrix(name, nu, a, b, 1.0)
    want = px.corr(kernel, ae, be)
    c = px.kernel_ulps(kernel, a, b, ra, rb)
    err = px.f64(abs(px.ext(got) - want))
    live = px.f64(want) > 1e-300
    q = (err[live] / (c[live] * px.U * px.f64(want)[live])).max()
    print("%s, %d / %d roundings: largest error / (c_k u rho) = %.3f; c_k at rho > 0.01: %.1f .. %.1f" %
          (kernel, ra, rb, q, c[px.f64(want) > 0.01].min(), c[px.f64(want) > 0.01].max()))
    assert q <= 1.0
    assert c[px.f64(want) > 0.01].max() < 3000 and c.min() >= 3


def test_a_nan_is_a_miss():
    """What the bounds are asserted through: a result that is not a number is outside its bound, wherever it stands."""
    ex, bd = px.loop_prelude(np.array([3.0, 5.0, 10.0]), 12)
    assert np.isnan(px.ratio(np.array([np.nan, 0.0, 0.0]), ex["y_train"], bd["y_train"]))
    assert np.isnan(px.ratio(np.array([0.0, np.inf, 0.0]), ex["y_train"], bd["y_train"]))
    assert px.within(dict(a=0.2, b=1.0)) and not px.within(dict(a=0.2, b=float("nan"), c=0.3)) and not px.within(dict(a=1.5))
    assert not px.within(dict(a=float("nan"))) and not px.within(dict(a=0.1, b=float("inf")))
    r = px.posterior(np.array([0.0, 2.0]), np.array([1.0, -1.0]), np.array([1.0, 1.0]), 2.0, 2.0, 1.0, 1e-6, "RBF", px.ext(np.array([1.0])))
    assert np.isnan(px.std_ratio(np.array([np.nan]), r)) and np.isnan(px.factor_ratio(np.full((2, 2), np.nan), r))
    assert px.std_ratio(np.sqrt(px.f64(r["var"])), r) <= 1


def _report(tag, r):
    print("%-44s %s" % (tag, "  ".join("%s %.3g" % kv for kv in r.items())))


def _check_core(tag, core, L, alpha, mean, std, cov, b_mean="b_mean", mean_key="mean"):
    r = dict(L=px.factor_ratio(L, core), alpha=px.ratio(alpha, core["alpha"], core["b_alpha"]),
             mean=px.ratio(mean, core[mean_key], core[b_mean]), var=px.std_ratio(std, core),
             cov=px.ratio(cov, core["cov"], core["b_cov"]))
    _report(tag, r)
    assert px.within(r), (tag, r)
    return r


def _check_inputs(tag, core, must_be_sharp):
    """K far from singular in units of its own bound, on every case; bounds sharp on the reference alone without fix_endpoints --
    and on the n == Lg sets under either setting, where the weights are gone anyway."""
    assert core["safety"] <= px.SAFETY_MAX, (tag, core["safety"])
    sm, sv = px.sharpness(core)
    if must_be_sharp:
        assert sm <= px.SHARP_MEAN and sv <= px.SHARP_VAR, (tag, sm, sv)
    return sm, sv


@pytest.mark.parametrize("n_cap", px.ALL_CAPS)
def test_oracle_inside_every_bound_loop_form(n_cap):
    worst, sharp = {}, [0.0, 0.0]
    for kernel, fix in px.combos_of(n_cap):
        cases = px.cases_of(n_cap) + (px.full_grid_case(n_cap),)
        for c in cases:
            tag = "%s %s fix=%d" % (c, kernel, fix)
            x, y, w = c.training(fix)
            assert x.shape[0] == c.n and np.all(np.diff(x) >= 0) and (np.sum(np.diff(x) == 0) == (1 if c.dup else 0))
            ex, bd, _ = px.loop_reference(c.key(), kernel, fix)
            y_s = float(np.std(y)) + 1.0
            amp = px.SIGMA_F ** 2 / y_s ** 2
            name, nu = px.KERNELS[kernel]
            fit = orc.gp_fit(x, y / y_s, w, amp, c.length, name, nu, 1, c.Lg)
            pred = orc.gp_predict(fit, c.grid())
            yt = y / y_s - fit["y_mean"]
            pre = dict(y_s=px.ratio(y_s, ex["y_s"], bd["y_s"]), amp=px.ratio(amp, ex["amp"], bd["amp"]),
                       y_mean=px.ratio(fit["y_mean"], ex["y_mean"], bd["y_mean"]), y_std=px.ratio(fit["y_std"], ex["y_std"], bd["y_std"]),
                       y_train=px.ratio(yt, ex["y_train"], bd["y_train"]))
            assert px.within(pre), (tag, pre)
            _, _, core = px.loop_reference(c.key(), kernel, fix, held=(yt.tobytes(), float(amp), float(fit["y_mean"]), float(fit["y_std"])))
            if c.n == c.Lg:  # the noise is gone from K's diagonal
                assert np.allclose(px.f64(core["K"].diagonal()), amp + 1e-6, rtol=1e-12)
            r = _check_core(tag, core, fit["L"], fit["alpha"], pred["mean"], pred["std"], pred["cov"])
            s = _check_inputs(tag, core, not fix or c.n == c.Lg)
            for k, v in dict(r, **pre).items():
                worst[k] = max(worst.get(k, 0.0), v)
            if not fix:
                sharp = [max(sharp[0], s[0]), max(sharp[1], s[1])]
    _report("n_cap %d, loop form, oracle / bound:" % n_cap, worst)
    print("    sharpness (fix_endpoints = False): mean bound / max|mean| %.2g, var bound / (amp y_std^2) %.2g" % tuple(sharp))


@pytest.mark.parametrize("n_cap", px.ALL_CAPS)
def test_oracle_inside_every_bound_converged_form(n_cap):
    worst, sharp = {}, [0.0, 0.0]
    for kernel, fix in px.combos_of(n_cap):
        cases = px.cases_of(n_cap) + (px.full_grid_case(n_cap),)
        for c in cases:
            tag = "%s %s fix=%d converged" % (c, kernel, fix)
            xs, ys, w, par = px.final_inputs(c, fix)
            core = px.final_reference(c.key(), kernel, fix)
            name, nu = px.KERNELS[kernel]
            fit = orc.gp_fit(xs, ys, w, par[0], par[1], name, nu, par[2], -1)  # (-1: the weights are already zero where n == Lg)
            fit["alpha"] = scipy.linalg.cho_solve((fit["L"], True), ys, check_finite=False)  # (the values are given: not centred again)
            fit["y_mean"], fit["y_std"] = par[7], par[8]
            pred = orc.gp_predict(fit, (c.grid() - par[3]) / par[4])
            if c.n == c.Lg:
                assert np.all(w == 0) and np.allclose(px.f64(core["K"].diagonal()), par[0] + 1e-6, rtol=1e-12)
            r = _check_core(tag, core, fit["L"], fit["alpha"], par[6] * pred["mean"] + par[5], pred["std"], pred["cov"],
                            b_mean="b_out_mean", mean_key="out_mean")
            s = _check_inputs(tag, core, not fix or c.n == c.Lg)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            if not fix:
                sharp = [max(sharp[0], s[0]), max(sharp[1], s[1])]
    _report("n_cap %d, converged form, oracle / bound:" % n_cap, worst)
    print("    sharpness (fix_endpoints = False): mean bound / max|mean| %.2g, var bound / (amp y_std^2) %.2g" % tuple(sharp))


@pytest.mark.parametrize("n_cap", px.JITTER_ONLY_CAPS)
def test_jitter_only_sets_pin_factor_variance_and_covariance(n_cap):
    """The ill-conditioned n == Lg sets: the oracle inside every bound, K still safely positive definite, variance and covariance
    bounds sharp -- and the mean's bound vacuous, as the helper says: these sets are not what pins alpha and the mean."""
    c = px.jitter_only_case(n_cap)
    x, y, w = c.training(True)
    ex, bd, _ = px.loop_reference(c.key(), "RBF", True)
    y_s = float(np.std(y)) + 1.0
    amp = px.SIGMA_F ** 2 / y_s ** 2
    fit = orc.gp_fit(x, y / y_s, w, amp, c.length, "RBF", 2.5, 1, c.Lg)
    pred = orc.gp_predict(fit, c.grid())
    yt = y / y_s - fit["y_mean"]
    _, _, core = px.loop_reference(c.key(), "RBF", True, held=(yt.tobytes(), float(amp), float(fit["y_mean"]), float(fit["y_std"])))
    _check_core("%s RBF fix=1" % c, core, fit["L"], fit["alpha"], pred["mean"], pred["std"], pred["cov"])
    sm, sv = px.sharpness(core)
    print("    sharpness: mean bound / max|mean| %.2g, var bound / (amp y_std^2) %.2g, safety %.2g" % (sm, sv, core["safety"]))
    assert core["safety"] <= px.SAFETY_MAX and sv <= px.SHARP_VAR and sm > 1e-6
    assert float(np.max(px.f64(core["b_cov"]))) <= px.SHARP_VAR * core["amp"] * core["y_std"] ** 2


def test_table_covers_every_regime():
    """Every (capacity, count) of the table exists, with one duplicate column and one n == Lg case per regime at least."""
    for regime, (caps, counts) in px.REGIMES.items():
        for n_cap in caps:
            got = {(c.n_init, c.n) for c in px.cases_of(n_cap)}
            for c in counts:
                n_init, n = c if isinstance(c, tuple) else (2, n_cap if c == "cap" else (n_cap - 1 if c == "cap-1" else c))
                assert n > n_cap or (n_init, n) in got, (n_cap, c)
            assert any(c.dup for c in px.cases_of(n_cap)) or n_cap == 64
            assert {c.Lg for c in px.cases_of(n_cap)} == set(px.spans_for(n_cap))
            f = px.full_grid_case(n_cap)
            assert f.n == f.Lg and f.n - f.n_init <= n_cap - f.n_init
        assert {k for k, _ in [px.EXTRA_KERNELS[c] for c in caps if c in px.EXTRA_KERNELS]} == {"M15", "M05"}, regime
    assert set(px.spans_for(128)) == {63, 64, 65, 130}
