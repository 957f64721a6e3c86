"""The curve KDE and the pixel selection (csrc/gpet_k_kde_pix.inc: k_kde_prep, k_kde_fused, k_pix_columns, k_pix_old,
k_pix_argbest, k_pix_select) on injected curves, in both forms: the stage form (gpet_curve_kde / gpet_select_pixels: the
normalised density everywhere) and the form the device loop runs (gpet_select_pixels_loop: the raw density of every tile's band
of rows, normalised on the fly by the pixel kernels).

The cases are those of tests/kde_pix_cases.py (tests/test_kde_pix_cases_host.py checks that each reaches its path): bands of three
and two 128-row chunks with points on the chunk boundaries, with one and with two staging passes of the kept curves (150 and 129
curves), curves that leave the image (removed columns, a tile without a surviving point, -0.0, M - 1 and its neighbours), an image
of five rows, a total weight below 1 and at a power of two with costs over six decades, edges that start and end four and five
columns from a tile boundary as one batch of four, float32 samples.  The inputs go in through GPET_BUF_SAMPLES, _BEST_IDX (not
increasing, with rows beyond n_keep), _BEST_COSTS, _GRAD_KDE and gpet_batch_set_obs after one gpet_score_curves.

(a) density: GPET_BUF_KDE after gpet_curve_kde against the np.longdouble reference's normalised float32 image: every pixel within
    4e-7, at most 1e-3 of the pixels unequal at all; n_removed equal to the count of points outside the image.  The device differs
    from the exact value by f64 rounding and the order of its sums (binning lsb 2^-70 against contributions of ~2^-17), so a pixel's
    float32 rounding flips with a probability of about 1e-7: 1e-3 is a cap with four decades of margin, not a measurement.
(b) selection, stage form: gpet_select_pixels against the oracle's compute_new_obs on the DEVICE's density -- observations, score
    threshold (bit for bit), iteration counter, done flag.
(c) loop form: a twin batch whose GPET_BUF_KDE is filled with 0.75 first; observations, threshold, counters equal to (b) bit for
    bit, and inside every tile's band (taken from the reference: the rows of the tile's surviving points, +-4, clipped) the raw
    density within the bounds of (a) of the reference's raw float32 image.
(d) every edge of the batch of four equal to its single-edge run, in both forms.

Measured on an MI355X, share of pixels unequal to the reference (normalised image of (a) / raw band of (c)):
tall_single 0 / 0, tall_restage 0 / 0, restage_129 0 / 0, leaving 0 / 0, tiny_M 0 / 0, small_W 0 / 0, small_W_pow2 0 / 0,
f32_samples 0 / 0, span_edges (four edges) 0 / 0.

The pixel rules run on injected densities through gpet_select_pixels_only against compute_new_obs, exact: float32 fields of
multiples of 1/8, so that equal scores are real -- within a column across the row lanes and the 64-row stride of k_pix_columns,
across the columns of a bin, between an old observation and a new pixel -- at 140 x 150 with delta_x = 2 (74 bins: several ballots
of k_pix_select, halves that round to even) and 64 x 40 with delta_x = 5; an old observation on density 0 and at x_st with
fix_endpoints both ways; density float32(1e-3) and its predecessor; eighteen decays of the threshold; a trace ended by algo_thresh.
A density of zeros has no candidate at any threshold, where the reference would spin forever: GPET_ERR_ITER_CAP, and the context
goes on working.  (That case found k_pix_select's escape unreachable -- it waited for the threshold to decay to 0, which a
multiplication by 0.95 never produces -- and the kernel now stops when a pass has found every bin that holds a candidate.)"""
import numpy as np
import pytest

from tests import kde_pix_cases as kc
from tests.injected_batch import make_batch

pytestmark = pytest.mark.gpu

ATOL, SHARE = 4e-7, 1e-3
GARBAGE = np.float32(0.75)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def image(M, N):
    g = np.random.default_rng(7).random((M, N)).astype(np.float32)
    g.flat[0], g.flat[-1] = 0.0, 1.0
    return g


def inject(amd, ctx, cases, prefill=None):
    """The batch of `cases` (edges on one image) with every input of the stage written, after one scoring pass."""
    L, c0 = amd._lib, cases[0]
    b = make_batch(amd, ctx, image(c0.M, c0.N), [(c.x_st, c.Lg) for c in cases], c0.S, sample_dtype=c0.sample_dtype,
                   delta_x=c0.delta_x, fix_endpoints=c0.fix_endpoints, pixel_thresh=c0.pixel_thresh, score_thresh=c0.score_thresh,
                   keep_ratio=0.5)
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


def state(b, e):
    s = b.scalars(e)
    return dict(score_thresh=s.score_thresh, n_obs=s.n_obs, n_removed=s.n_removed, done=s.done, iter=s.iter, status=s.status)


def run_both_forms(amd, ctx, cases):
    """Per edge: (normalised density after gpet_curve_kde, state and observations after gpet_select_pixels, density after it) of the
    stage form, and (GPET_BUF_KDE, state, observations) after gpet_select_pixels_loop on the twin batch."""
    L = amd._lib
    stage, loop = [], []
    b = inject(amd, ctx, cases)
    try:
        b.curve_kde()
        dens = [b.read(L.BUF_KDE, e) for e in range(b.B)]
        removed = [b.scalars(e).n_removed for e in range(b.B)]
        b.select_pixels()
        for e in range(b.B):
            stage.append(dict(kde=dens[e], removed=removed[e], kde_after=b.read(L.BUF_KDE, e), obs=b.read(L.BUF_OBS, e), **state(b, e)))
    finally:
        b.close()
    t = inject(amd, ctx, cases, prefill=GARBAGE)
    try:
        t.select_pixels_loop()
        for e in range(t.B):
            loop.append(dict(kde=t.read(L.BUF_KDE, e), obs=t.read(L.BUF_OBS, e), **state(t, e)))
    finally:
        t.close()
    return stage, loop


def band_mask(c):
    m = np.zeros((c.M, c.N), dtype=bool)
    for t, (lo, hi) in enumerate(kc.tile_bands(c)):
        if hi >= lo:
            m[lo:hi + 1, t * kc.KDE_TX:(t + 1) * kc.KDE_TX] = True
    return m


def check_edge(c, st, lp):
    """(a), (b), (c) for one edge; returns the shares of unequal pixels (normalised image, raw band)."""
    raw, norm, removed = kc.reference(c)
    # (a)
    kde = st["kde"]
    assert kde.dtype == np.float32 and kde.shape == norm.shape and np.all(np.isfinite(kde))
    err = np.abs(kde.astype(np.float64) - norm.astype(np.float64))
    share = float(np.mean(kde != norm))
    print("%s: normalised density: %d of %d pixels unequal (share %.2e), max abs %.3g" % (c.name, int((kde != norm).sum()), kde.size,
                                                                                          share, err.max()))
    assert err.max() <= ATOL, (c.name, np.unravel_index(err.argmax(), err.shape), err.max())
    assert share <= SHARE, (c.name, share)
    assert st["removed"] == removed and st["n_removed"] == removed, (c.name, st["removed"], removed)
    # (b)
    assert np.array_equal(st["kde_after"], kde), c.name
    fobs, thresh, done = kc.expected_selection(c, kde)
    assert np.array_equal(st["obs"], fobs), (c.name, st["obs"].tolist(), fobs.tolist())
    assert st["score_thresh"] == thresh and st["n_obs"] == fobs.shape[0], (c.name, st["score_thresh"], thresh)
    assert (st["iter"], st["done"], st["status"]) == (1, done, 0), (c.name, st)
    # (c)
    for k in ("score_thresh", "n_obs", "n_removed", "done", "iter", "status"):
        assert lp[k] == st[k], (c.name, k, lp[k], st[k])
    assert np.array_equal(lp["obs"], st["obs"]), c.name
    m = band_mask(c)
    got, want = lp["kde"][m], raw[m]
    berr = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bshare = float(np.mean(got != want))
    print("%s: raw density in the bands: %d of %d pixels unequal (share %.2e), max abs %.3g, largest density %.3g"
          % (c.name, int((got != want).sum()), got.size, bshare, berr.max(), want.max()))
    assert berr.max() <= ATOL and bshare <= SHARE, (c.name, berr.max(), bshare)
    return share, bshare


@pytest.mark.parametrize("name", kc.NAMES)
def test_density_and_selection_in_both_forms(amd, ctx, name):
    c = kc.case(name)
    stage, loop = run_both_forms(amd, ctx, [c])
    check_edge(c, stage[0], loop[0])


def test_batch_of_four_edges_next_to_tile_boundaries(amd, ctx):
    cases = kc.case("span_edges")
    stage, loop = run_both_forms(amd, ctx, cases)
    for e, c in enumerate(cases):
        check_edge(c, stage[e], loop[e])
        st1, lp1 = run_both_forms(amd, ctx, [c])
        for got, one, form in ((stage[e], st1[0], "stage"), (loop[e], lp1[0], "loop")):
            for k, v in one.items():
                assert np.array_equal(got[k], v), (c.name, form, k)


# ---- pixel rules on injected densities -----------------------------------------------------------------------------------------------
def rule_batch(amd, ctx, c):
    L = amd._lib
    b = make_batch(amd, ctx, image(c.M, c.N), [(c.x_st, c.Lg)], 64, delta_x=c.delta_x, fix_endpoints=c.fix_endpoints,
                   pixel_thresh=c.pixel_thresh, score_thresh=c.score_thresh)
    try:
        assert b.info()["algo_thresh"] == kc.pixel_state(c)["algo_thresh"]
        b.write(L.BUF_GRAD_KDE, c.grad_kde)
        b.write(L.BUF_KDE, c.kde)
        b.set_obs(0, c.obs)
    except Exception:
        b.close()
        raise
    return b


def check_rule(amd, ctx, c):
    L = amd._lib
    fobs, thresh, done = kc.expected_selection(c, c.kde)
    b = rule_batch(amd, ctx, c)
    try:
        b.select_pixels_only()
        got, s = b.read(L.BUF_OBS), b.scalars()
        assert np.array_equal(got, fobs), (c.name, got.tolist(), fobs.tolist())
        assert s.score_thresh == thresh and (s.n_obs, s.iter, s.done, s.status) == (fobs.shape[0], 1, done, 0), (c.name, s.score_thresh, thresh)
    finally:
        b.close()
    return [tuple(v) for v in got.tolist()]


@pytest.mark.parametrize("shape", list(kc.RULE_SHAPES))
@pytest.mark.parametrize("rule", kc.RULES)
def test_pixel_rules_on_injected_densities(amd, ctx, rule, shape):
    c = kc.rule_case(rule, shape)
    got = check_rule(amd, ctx, c)
    m = c.marks
    if "winner" in m:
        assert m["winner"] in got
    if "absent" in m:
        assert m["absent"] not in got
    if "count" in m:
        assert len(got) == m["count"]


def test_density_of_zeros_is_an_error_code_and_the_context_goes_on(amd, ctx):
    """No pixel passes `density > 1e-3`, so no bin holds a candidate at any threshold: the reference's loop would never end.  The
    library reports GPET_ERR_ITER_CAP; the next batch of the context works."""
    L = amd._lib
    c = kc.Case(kc.rule_case("five_decays", "64x40-dx5"))
    c["kde"] = np.zeros_like(c.kde)
    b = rule_batch(amd, ctx, c)
    try:
        with pytest.raises(L.GpetError) as ei:
            b.select_pixels_only()
        assert ei.value.code == L.ERR_ITER_CAP
        s = b.scalars()
        assert (s.status, s.n_obs, s.iter) == (L.ERR_ITER_CAP, 0, 0)
    finally:
        b.close()
    check_rule(amd, ctx, kc.rule_case("five_decays", "64x40-dx5"))
