"""GPU tests of the device L-BFGS-B (gpet_final_optimize: k_lb_init / k_lb_advance / k_lb_pick and the persistent k_lml16_fit)
on bounded problems, read back per problem through gpet_final_problems: against the host build of the same header driven with
the device objective, across problem counts that fill waves unevenly, for the pick of the best restart, and against scipy on
the oracle's objective.  tests/lbfgsb_cases.py has the host build, the box / start generators and the margins."""
import numpy as np
import pytest

from tests import final_fit_inputs as ff
from tests import lbfgsb_cases as lc

pytestmark = pytest.mark.gpu

N = 256
SIZES = (8, 17, 40, 12, 29)  # training points per edge of the 5-edge batch: all within k_lml16_fit (n <= 108)
BIG = 120                    # more than 108 points: the round-based driver whatever fit_persistent says
CENTRE = np.log([1.0, 1.0, 1e-2])


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def host():
    if lc.compiler() is None:
        pytest.skip("no host C++ compiler found")
    import tempfile
    return lc.build_shim(tempfile.mkdtemp())


def _training(n, seed):
    rng = np.random.default_rng(seed)
    cols = np.sort(rng.choice(np.arange(1, N - 1), size=n - 2, replace=False))
    rows = np.rint(30.0 + 12.0 * np.sin(cols / 40.0) + rng.normal(0.0, 1.5, size=n - 2)).astype(np.int64)
    pr = ff.prepare(np.array([[0, 30], [N - 1, 30]]), np.stack([cols, rows], axis=1), np.arange(N), True)
    assert pr["xs"].shape[0] == n
    return pr


def _batch(amd, ctx, sizes):
    """a batch of len(sizes) edges whose converged-fit training sets are set directly (no trace runs)"""
    img = np.random.default_rng(1).uniform(size=(64, N)).astype(np.float32)
    init = np.array([[0, 30], [N - 1, 30]])
    kw = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 40, 'length_scale': 12}, noise_y=1, N_samples=64, score_thresh=1,
              delta_x=2, keep_ratio=0.1, pixel_thresh=20, fix_endpoints=True)
    tr = amd.GP_Edge_Tracing_Batch([init] * len(sizes), img, list(range(len(sizes))), **kw, _ctx=ctx)
    prs = [_training(n, 100 + n) for n in sizes]
    for e, pr in enumerate(prs):
        tr._batch.final_set_training(e, pr["xs"], pr["yt"], pr["w"])
    return tr, prs


@pytest.fixture(scope="module")
def five(amd, ctx):
    return _batch(amd, ctx, SIZES)


@pytest.fixture(scope="module")
def one(amd, ctx):
    return _batch(amd, ctx, SIZES[:1])  # the training set of edge 0 of `five`, alone


@pytest.fixture(scope="module")
def big(amd, ctx):
    return _batch(amd, ctx, (BIG,))


def _boxes():
    """boxes of the corpus' GP family: the optimum cut off in one and in two variables, and a degenerate noise interval"""
    rng = np.random.default_rng(4242)
    out = []
    for n_cut in (1, 2, 0):
        lo, hi = lc._box(rng, CENTRE, n_cut, 3.0)
        out.append([lo, hi])
    out[2][1][2] = out[2][0][2]  # lo == hi
    return [(np.array(lo), np.array(hi)) for lo, hi in out]


def _starts(seed, lo, hi, count):
    rng = np.random.default_rng(seed)
    kinds = ("inside", "corner", "outside", "face")
    return np.array([lc._start(rng, lo, hi, kinds[k % 4]) for k in range(count)])


def _persistent(L, mode):
    class Scope:
        def __enter__(self):
            self.old = L.set_option("fit_persistent", mode)

        def __exit__(self, *exc):
            L.set_option("fit_persistent", -1 if self.old == 2 else self.old)
    return Scope()


def _device_eval(b, edge_of):
    edge_of = np.asarray(edge_of, dtype=np.int32)

    def evaluate(index, x):
        return b.lml_batch(edge_of[index], x)
    return evaluate


@pytest.fixture(scope="module")
def host_runs(five, big, host):
    """the host build on every (batch, box) of the test below, driven with the device objective: computed once"""
    out = {}
    for name, (tr, prs), n_starts in (("five", five, 13), ("big", big, 13)):
        B = len(prs)
        for k, (lo, hi) in enumerate(_boxes()):
            starts = np.stack([_starts(1000 * k + e, lo, hi, n_starts) for e in range(B)])
            rec = lc.run_host_lockstep(host, _device_eval(tr._batch, np.repeat(np.arange(B), n_starts)), starts.reshape(-1, 3), lo, hi)
            out[name, k] = (starts, rec)
    return out


# (more than 108 training points: fit_persistent 1 runs the rounds as well, which mode 0 covers)
@pytest.mark.parametrize("name,box,mode", [("five", k, m) for k in range(3) for m in (0, 1)] + [("big", k, 0) for k in range(3)])
def test_device_problems_equal_the_host_build(amd, five, big, host_runs, name, box, mode):
    """every (edge, start) problem: iterations, evaluations and stop reason of the device equal the host build of the same
    header on the same (device) objective; the rounds (fit_persistent 0) run the very objective kernel that lml_batch runs,
    so the end point agrees to the floor of the host tests' margin.  The persistent kernel compiles the objective into
    another kernel, whose last bits differ: the tolerance of test_final_fit_one_workgroup_per_problem_equals_rounds, and
    evaluation counts within 3 (an iteration more or less is an evaluation more or less: iterations within 3 too)."""
    tr, prs = five if name == "five" else big
    lo, hi = _boxes()[box]
    starts, h = host_runs[name, box]
    with _persistent(amd._lib, mode):
        tr._batch.final_optimize(starts, np.stack([lo, hi], axis=1))
        d = tr._batch.final_problems()
    assert d["x"].shape == h["x"].shape
    assert np.all(d["x"] >= lo) and np.all(d["x"] <= hi)
    print(name, box, mode, "nfev", d["nfev"].min(), d["nfev"].max(), "why", np.bincount(d["why"], minlength=6)[1:],
          "max |dx|", np.abs(d["x"] - h["x"]).max(), "max |dnfev|", np.abs(d["nfev"] - h["nfev"]).max())
    assert np.array_equal(d["why"], h["why"])
    if mode == 0:
        assert np.array_equal(d["iter"], h["iter"])
        assert np.array_equal(d["nfev"], h["nfev"])
        scale = 1.0 + np.abs(h["x"]).max(axis=1, keepdims=True)
        assert np.all(np.abs(d["x"] - h["x"]) <= lc.MARGIN_FLOOR * scale)
        np.testing.assert_allclose(d["f"], h["f"], rtol=lc.MARGIN_FLOOR, atol=lc.MARGIN_FLOOR)
    else:
        assert np.all(np.abs(d["nfev"] - h["nfev"]) <= 3) and np.all(np.abs(d["iter"] - h["iter"]) <= 3)
        np.testing.assert_allclose(d["x"][:, :2], h["x"][:, :2], rtol=0, atol=1e-6)
        np.testing.assert_allclose(np.exp(d["x"][:, 2]), np.exp(h["x"][:, 2]), rtol=1e-3, atol=1e-9)
        np.testing.assert_allclose(d["f"], h["f"], rtol=1e-9, atol=0)


def _stationary_corner(b, e, lo, hi):
    """the corner of a box at which every component of the gradient of edge e's objective pushes outwards"""
    corners = np.array([[(lo, hi)[(k >> c) & 1][c] for c in range(3)] for k in range(8)])
    f, g = b.lml_batch(np.full(8, e, dtype=np.int32), corners)
    for x, gk in zip(corners, g):
        if lc.projected_gradient(x, gk, lo, hi) == 0.0:
            return x
    return None


def test_results_do_not_depend_on_the_problem_count(amd, five, one):
    """P = 1, 63, 64, 65 and 130 problems: sets that mix starts which are done at their first evaluation (stationary on a
    corner) with long ones, so that slots empty unevenly between the host's reads of the running count; a problem's record
    is bit-identical alone, among 63 / 64 / 65, and among 130 (fit_persistent 0: the rounds)."""
    (tr5, _), (tr1, _) = five, one
    b5, b1 = tr5._batch, tr1._batch
    # a box that cuts every edge's optimum off in all three variables (the oracle's objective has a stationary corner in it
    # for each of the five training sets, and interior starts take 2 to 18 evaluations)
    wide_lo, wide_hi = lc._box(np.random.default_rng(505), CENTRE, 3, 3.0)
    rng = np.random.default_rng(99)
    pool = wide_lo + (wide_hi - wide_lo) * rng.uniform(size=(5, 64, 3))
    corner = _stationary_corner(b1, 0, wide_lo, wide_hi)
    for e in range(5):  # every third start sits on the edge's stationary corner
        c = _stationary_corner(b5, e, wide_lo, wide_hi)
        if c is not None:
            pool[e, 1::3] = c
    bounds = np.stack([wide_lo, wide_hi], axis=1)
    recs = {}
    with _persistent(amd._lib, 0):
        for P, b, starts in ((130, b5, pool[:, :26]), (65, b5, pool[:, :13]), (64, b1, pool[:1, :64]), (63, b1, pool[:1, :63]),
                             (1, b1, pool[:1, 7:8]), (1, b1, pool[:1, 1:2]), (1, b1, pool[:1, 25:26])):
            theta, fmin, rounds = b.final_optimize(starts, bounds)
            d = b.final_problems()
            assert d["x"].shape[0] == P == starts.shape[0] * starts.shape[1]
            assert np.all(d["why"] >= 1) and np.all(d["x"] >= wide_lo) and np.all(d["x"] <= wide_hi)
            # k_lb_pick: the first minimum among an edge's restarts
            per_edge = d["f"].reshape(starts.shape[0], -1)
            best = np.argmin(per_edge, axis=1)
            assert np.array_equal(fmin, per_edge[np.arange(len(best)), best])
            assert np.array_equal(theta, d["x"].reshape(starts.shape[0], -1, 3)[np.arange(len(best)), best])
            recs.setdefault(P, []).append((starts, d))
    s130, d130 = recs[130][0]
    n_first = int(np.sum(d130["nfev"] == 1))
    print("130 problems: done at the first evaluation %d, longest %d evaluations" % (n_first, d130["nfev"].max()))
    assert corner is not None and np.array_equal(corner, pool[0, 1]) and n_first >= 9 and d130["nfev"].max() >= 10
    assert np.all(d130["why"][d130["nfev"] == 1] == 1) and np.all(d130["nfev"].reshape(5, 26)[0, 1::3] == 1)

    def same(da, ia, db, ib):
        for key in ("x", "f", "g", "iter", "nfev", "why"):
            assert np.array_equal(da[key][ia], db[key][ib]), key
    idx130 = np.arange(130).reshape(5, 26)
    d65 = recs[65][0][1]
    same(d65, np.arange(65), d130, idx130[:, :13].reshape(-1))          # 65 of the 130
    d64, d63 = recs[64][0][1], recs[63][0][1]
    same(d63, np.arange(63), d64, np.arange(63))                        # 63 of the 64
    same(d64, np.arange(26), d130, idx130[0])                           # edge 0's 26 among 64 and among 130
    for (s1, d1), j in zip(recs[1], (7, 1, 25)):                        # alone
        same(d1, np.arange(1), d130, idx130[0, j:j + 1])


def test_best_restart_is_the_first_minimum_with_ties(amd, one):
    """the same start twice ties exactly; k_lb_pick returns the first minimum (np.argmin) in either order of the starts"""
    tr, _ = one
    b = tr._batch
    lo, hi = CENTRE - 3.0, CENTRE + 3.0
    s = _starts(5, lo, hi, 4)
    with _persistent(amd._lib, 0):
        for order in ([0, 1, 2, 1, 3, 1], [1, 1, 0], [3, 2, 1, 0, 1]):
            starts = s[order][None]
            theta, fmin, _ = b.final_optimize(starts, np.stack([lo, hi], axis=1))
            d = b.final_problems()
            twins = [k for k, o in enumerate(order) if o == 1]
            for k in twins[1:]:
                assert d["f"][k] == d["f"][twins[0]] and np.array_equal(d["x"][k], d["x"][twins[0]])
            best = int(np.argmin(d["f"]))
            assert fmin[0] == d["f"][best] and np.array_equal(theta[0], d["x"][best])


def test_device_against_scipy_on_the_oracle_objective(amd, five, host_runs):
    """scipy's L-BFGS-B on the oracle's objective (float64 Cholesky) with the same box and starts: per problem, the minimum
    and theta within the host tests' margin (ten times scipy's own spread under +-2 ulp, floor 1e-12), the noise level
    compared in linear space.  Problems on which scipy does not reproduce its own path are left out."""
    tr, prs = five
    box = 0
    lo, hi = _boxes()[box]
    starts, _ = host_runs["five", box]
    with _persistent(amd._lib, 0):
        tr._batch.final_optimize(starts, np.stack([lo, hi], axis=1))
        d = tr._batch.final_problems()
    bad, n_cmp = [], 0
    for e in (0, 1):  # 8 and 17 training points
        fun = lc.GpObjective.from_training(prs[e]["xs"], prs[e]["yt"], prs[e]["w"], "RBF")
        for k in range(starts.shape[1]):
            i = e * starts.shape[1] + k
            ref = lc.reference(dict(fun=fun, x0=starts[e, k], lo=lo, hi=hi, seed=i))
            if not ref["stable"]:
                continue
            n_cmp += 1
            r, m = ref["ref"], lc.margin(ref["spread"])
            dx = np.max(np.abs(d["x"][i, :2] - r["x"][:2])) / (1.0 + np.max(np.abs(r["x"])))
            dn = abs(np.exp(d["x"][i, 2]) - np.exp(r["x"][2])) / (1.0 + np.max(np.abs(r["x"])))
            df = abs(d["f"][i] - r["f"]) / (1.0 + abs(r["f"]))
            print("edge %d start %2d: spread %.2e  theta %.2e  noise %.2e  f %.2e  nfev %d / %d" %
                  (e, k, ref["spread"], dx, dn, df, d["nfev"][i], r["nfev"]))
            if max(dx, dn, df) > m:
                bad.append((e, k, ref["spread"], dx, dn, df))
    assert n_cmp >= 20
    assert not bad, bad
