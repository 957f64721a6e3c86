"""The two forms of the fused curve KDE against each other (csrc/gpet_k_kde_pix.inc): the register form k_kde_fused_r (option
kde_variant = 1, the default: a tile's points stay in registers, weights once per edge from k_kde_prep, first chunk cleared under
the loads, fixed point converted by the vertical pass's reads) and the staged form k_kde_fused (kde_variant = 0).  What rounds is
the same in both and the binning sums are 64-bit fixed point, so everything must be equal bit for bit: GPET_BUF_KDE (the loop's
form on a buffer prefilled with 0.75: the raw density of the band rows; the stage form: the normalised image), every tile's band
and the two keys of the raw minimum / maximum (GPET_BUF_KDE_TILES), and what the pixel selection that follows makes of them --
observations, threshold, counters, status.

Injected curves, built with the pieces of tests/kde_pix_cases.py.  The smallest shapes at which the register form can go wrong:
N = 20, 36, 37 (two and three tiles, a ragged last tile, N & 3 != 0: the scalar horizontal pass), M = 24 (one chunk) and 150 (curves
over more than 128 rows: two chunks, the points held in registers are binned twice), n_keep = 1, 3, 128 (one thread with a point,
a few, every thread's six); x_st > 0 and x_en < N - 1 throughout; edges that leave a tile wholly beside them (band == false); points
at y < 0, y > M - 1, on integers, at 0 and M - 1; an edge with every point outside the image (nothing binned); three edges of
different n_keep and width as one batch; 129 kept curves with kde_variant = 1, which the launcher must hand to the staged form."""
import numpy as np
import pytest

from tests import kde_pix_cases as kc

pytestmark = pytest.mark.gpu

GARBAGE = np.float32(0.75)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def spread_curves(rng, n_keep, Lg, M):
    """Curves whose points on adjacent columns cover the rows lo .. M - 1 - lo, lo = min(10, M // 4) (column k of curve b sits at
    the fraction ((7 k + 13 b) mod Lg) / (Lg - 1) of them): bands that start above row 0 and, at M = 150, are taller than a chunk.
    The special points of the module's docstring sit on the first ten columns -- staged by the first tile only, whose band then
    is the whole image -- of the first and the last curve."""
    k, b = np.arange(Lg)[None, :], np.arange(n_keep)[:, None]
    lo = min(10, M // 4)
    y = lo + (M - 1.0 - 2 * lo) * (((7 * k + 13 * b) % Lg) / (Lg - 1.0)) + rng.uniform(-0.4, 0.4, size=(n_keep, Lg))
    for i, v in enumerate([0.0, M - 1.0, -0.5, M - 0.5, 7.0, np.nextafter(M - 1.0, np.inf), -0.0]):
        y[0, i] = v
    for i, v in enumerate([float(M // 2), M + 3.0, -2.0]):
        y[-1, 7 + i] = v
    return y


def finish(name, M, N, x_st, curves, rng, S, delta_x=2):
    """kde_pix_cases._finish with the sample count as a parameter (edges of one batch differ in n_keep, not in S)."""
    n_keep, Lg = curves.shape
    best_idx = kc._pick_rows(rng, S, n_keep)
    Y = rng.uniform(0.0, M - 1.0, size=(S, Lg))
    Y[best_idx] = curves
    costs = rng.uniform(0.5, 4.0, size=n_keep)
    grad_kde = (rng.integers(0, 1025, size=(M, N)) / 1024.0).astype(np.float32)
    w = int(np.argmin(costs))
    on_curve = lambda k: (x_st + k, int(np.clip(np.rint(curves[w, k]), 0, M - 1)))
    obs = [on_curve(Lg // 2), on_curve(0)]
    for x, y in obs:
        grad_kde[y, x] = 1.0
    return kc.Case(name=name, M=M, N=N, x_st=x_st, Lg=Lg, S=S, n_keep=n_keep, Y=Y, best_idx=best_idx, best_costs=costs,
                   obs=np.array(obs, dtype=np.int64).reshape(-1, 2), grad_kde=grad_kde, delta_x=delta_x, pixel_thresh=2, score_thresh=1.0,
                   fix_endpoints=True, sample_dtype=None)


def grid_case(N, M, n_keep, x_st=2, x_en=None, seed=0):
    x_en = N - 3 if x_en is None else x_en
    rng = np.random.default_rng(7000 + 97 * N + 13 * M + n_keep + seed)
    Lg = x_en - x_st + 1
    return finish("N%d-M%d-k%d-[%d,%d]" % (N, M, n_keep, x_st, x_en), M, N, x_st, spread_curves(rng, n_keep, Lg, M), rng, max(64, 2 * n_keep))


# ---- running ---------------------------------------------------------------------------------------------------------------------------
def image(M, N):
    g = np.random.default_rng(7).random((M, N)).astype(np.float32)
    g.flat[0], g.flat[-1] = 0.0, 1.0
    return g


def inject(amd, ctx, cases, prefill=None):
    """tests/test_gpu_kde_pix_injected.py::inject with every edge's own n_keep: the batch of `cases` (edges on one image) with
    every input of the stage written, after one scoring pass."""
    from gaussian_process_edge_trace_amd.gpet import resolve_params, to_abi_params
    from tests.injected_batch import KERNEL
    L, c0 = amd._lib, cases[0]
    grad = image(c0.M, c0.N)
    params, inits = [], []
    for c in cases:
        init = np.array([[c.x_st, 1], [c.x_st + c.Lg - 1, c.M - 2]])
        p = resolve_params(init, grad.shape, KERNEL, noise_y=1, N_samples=max(c.S, 101), score_thresh=c.score_thresh, delta_x=c.delta_x,
                           keep_ratio=0.25, pixel_thresh=c.pixel_thresh, seed=1, fix_endpoints=c.fix_endpoints)
        q = to_abi_params(p, obs_cap=None, factor_cap=0, z_cols=0)
        q.n_samples, q.n_keep = c.S, c.n_keep
        params.append(q)
        inits.append(p["init"])
    b = L.Batch(ctx, [grad], params, inits, share_image=len(cases) > 1)
    try:
        for e, c in enumerate(cases):
            inf = b.info(e)
            assert (inf["Lg"], inf["S"], inf["n_keep"], inf["algo_thresh"]) == (c.Lg, c.S, c.n_keep, kc.pixel_state(c)["algo_thresh"])
            b.write(L.BUF_SAMPLES, c.Y, e)
        b.score()  # (sets the state the stage asks for; what it leaves is overwritten)
        for e, c in enumerate(cases):
            b.write(L.BUF_SAMPLES, c.Y, e)
            b.write(L.BUF_BEST_IDX, c.best_idx, e)
            b.write(L.BUF_BEST_COSTS, c.best_costs, e)
            b.write(L.BUF_GRAD_KDE, c.grad_kde, e)
            b.set_obs(e, c.obs)
            if prefill is not None:
                b.write(L.BUF_KDE, np.full((c.M, c.N), prefill, dtype=np.float32), e)
    except Exception:
        b.close()
        raise
    return b


def snapshot(L, b, err):
    out = []
    for e in range(b.B):
        s = b.scalars(e)
        out.append(dict(kde=b.read(L.BUF_KDE, e).view(np.uint32), tiles=b.read(L.BUF_KDE_TILES, e), obs=b.read(L.BUF_OBS, e),
                        state=(s.score_thresh, s.n_obs, s.n_removed, s.done, s.iter, s.status), error=err))
    return out


def run(amd, ctx, cases, variant):
    """Per edge, the loop's form (raw band, pixel selection) and the stage form (normalised density) under kde_variant = variant."""
    L = amd._lib
    old = L.set_option("kde_variant", variant)
    try:
        b = inject(amd, ctx, cases, prefill=GARBAGE)
        try:
            err = None
            try:
                b.select_pixels_loop()
            except L.GpetError as ex:  # (a density without a candidate: the same error code in both forms)
                err = ex.code
            loop = snapshot(L, b, err)
        finally:
            b.close()
        b = inject(amd, ctx, cases)
        try:
            b.curve_kde()
            stage = snapshot(L, b, None)
        finally:
            b.close()
    finally:
        L.set_option("kde_variant", old)
    return loop, stage


def assert_same(cases, got, want, form):
    for c, g, w in zip(cases, got, want):
        # (the stage form writes no bands -- it writes the rows outside them as zeros --, only the two keys)
        assert np.array_equal(g["tiles"][-1], w["tiles"][-1]) and (form == "stage" or np.array_equal(g["tiles"], w["tiles"])), (c.name, form)
        for k in ("kde", "obs"):
            assert np.array_equal(g[k], w[k]), (c.name, form, k)
        assert g["state"] == w["state"] and g["error"] == w["error"], (c.name, form, g["state"], w["state"], g["error"], w["error"])


def check(amd, ctx, cases, selects=True):
    """Both variants on `cases` as one batch; returns the register form's loop-form results."""
    loop0, stage0 = run(amd, ctx, cases, 0)
    loop1, stage1 = run(amd, ctx, cases, 1)
    assert_same(cases, loop1, loop0, "loop")
    assert_same(cases, stage1, stage0, "stage")
    for c, lp in zip(cases, loop1):
        # the cases are what they are named for: every tile's band is the band of its surviving points, and the band rows hold
        # the density, not the prefill
        bands = kc.tile_bands(c)
        assert [tuple(r) for r in lp["tiles"][:-1].tolist()] == bands, (c.name, lp["tiles"].tolist(), bands)
        kde = lp["kde"].view(np.float32)
        for t, (lo, hi) in enumerate(bands):
            if hi >= lo:
                assert not np.any(kde[lo:hi + 1, t * kc.KDE_TX:(t + 1) * kc.KDE_TX] == GARBAGE), (c.name, t)
        if selects:
            assert lp["error"] is None and lp["state"][4:] == (1, 0) and lp["state"][1] > c.obs.shape[0], (c.name, lp["state"], lp["error"])
    return loop1


@pytest.mark.parametrize("n_keep", [1, 3, 128])
@pytest.mark.parametrize("M", [24, 150])
@pytest.mark.parametrize("N", [20, 36, 37])
def test_register_form_equals_staged_form(amd, ctx, N, M, n_keep):
    c = grid_case(N, M, n_keep)
    lp = check(amd, ctx, [c])[0]
    heights = [hi - lo + 1 for lo, hi in kc.tile_bands(c)]
    assert (max(heights) > kc.KDE_H) == (M == 150), heights  # M = 150: a band of two chunks


@pytest.mark.parametrize("N,x_en", [(20, 11), (36, 25), (37, 27)])
def test_a_tile_wholly_beside_the_edge(amd, ctx, N, x_en):
    """The edge ends more than four columns before the last tile: that tile stages nothing (band == false) and reports (M, -1)."""
    c = grid_case(N, 24, 3, x_st=2, x_en=x_en, seed=1)
    lp = check(amd, ctx, [c])[0]
    assert tuple(lp["tiles"][-2]) == (c.M, -1) and kc.tile_bands(c)[-1] == (c.M, -1)


def test_every_point_outside_the_image(amd, ctx):
    """Nothing is binned in any tile (s_band[1] < 0), W = 0: no band anywhere, both keys the key of 0, and a selection without a
    candidate -- whatever that ends in, it ends the same in both forms."""
    c = grid_case(36, 24, 3, seed=2)
    out = np.where(np.arange(c.Lg)[None, :] % 2 == 0, -3.0, c.M + 2.5) + np.zeros((c.n_keep, 1))
    c.Y[c.best_idx] = out
    lp = check(amd, ctx, [c], selects=False)[0]
    assert all(tuple(r) == (c.M, -1) for r in lp["tiles"][:-1].tolist())
    assert lp["tiles"][-1, 0] == lp["tiles"][-1, 1] and lp["state"][2] == c.n_keep * c.Lg
    assert np.all(lp["kde"].view(np.float32) == GARBAGE)


def test_three_edges_of_different_n_keep_and_width(amd, ctx):
    M, N, S = 150, 37, 256
    cases = []
    for i, (x_st, x_en, n_keep) in enumerate([(2, 25, 1), (5, 34, 3), (1, 35, 128)]):
        rng = np.random.default_rng(7900 + i)
        Lg = x_en - x_st + 1
        cases.append(finish("three[%d]" % i, M, N, x_st, spread_curves(rng, n_keep, Lg, M), rng, S))
    shared = cases[0].grad_kde.copy()  # (edges on one image share its gradient KDE)
    for c in cases:
        shared[c.obs[:, 1], c.obs[:, 0]] = 1.0
    for c in cases:
        c["grad_kde"] = shared
    batch = check(amd, ctx, cases)
    for e, c in enumerate(cases):  # every edge as in its single-edge run
        one = check(amd, ctx, [c])[0]
        for k in ("tiles", "kde", "obs"):
            assert np.array_equal(batch[e][k], one[k]), (c.name, k)
        assert batch[e]["state"] == one["state"]


def test_129_curves_take_the_staged_form_whatever_the_variant(amd, ctx):
    """n_keep = 129 > KDE_NB: kde_variant = 1 must reach the staged form (the register form would bin 128 curves and read
    the 129th's weight from nowhere); the results are those of variant 0."""
    check(amd, ctx, [kc.case("restage_129")])
