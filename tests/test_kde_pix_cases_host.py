"""Host checks of tests/kde_pix_cases.py: the extended-precision reference of the curve KDE against the f64 oracle with a direct
convolution (bit for bit -- the proof that the reference alone meets the cap the GPU test sets on unequal pixels; the oracle's
default FFT convolution does not), the count of removed points, and for every case the property it is named for, computed from
the kernels' constants (16-column tiles that stage 24 columns, 128-row chunks, 128 curves per staging pass), so that an edit of
the data cannot quietly stop reaching the path."""
import numpy as np
import pytest

from oracle import gpet_oracle as orc
from tests import kde_pix_cases as kc

TX, H, NB = 16, 128, 128


def all_cases():
    return [kc.case(n) for n in kc.NAMES] + list(kc.case("span_edges"))


ALL_IDS = kc.NAMES + ["span_edges%d" % i for i in range(len(kc.SPANS))]


def chunks(band):
    return 0 if band[1] < band[0] else -(-(band[1] - band[0] + 1) // H)


@pytest.mark.parametrize("i", range(len(ALL_IDS)), ids=ALL_IDS)
def test_reference_equals_the_f64_oracle_and_counts_removed_points(i):
    c = all_cases()[i]
    raw, norm, removed = kc.reference(c)
    got = kc.oracle_kde(c)
    assert got.shape == norm.shape == (c.M, c.N) and norm.dtype == np.float32
    diff = np.abs(got - norm.astype(np.float64))
    print("%s: %d unequal pixels of %d, max abs %.3g" % (c.name, int((diff != 0).sum()), diff.size, diff.max()))
    assert np.array_equal(got, norm.astype(np.float64))
    assert norm.min() == 0.0 and norm.max() == 1.0
    y = kc.kept_curves(c)
    assert removed == int(np.sum((y < 0) | (y > c.M - 1)))
    # the data is what it says: rows of best_idx distinct, not monotone, some beyond n_keep; S, n_keep as make_batch derives them
    assert len(set(c.best_idx.tolist())) == c.n_keep and c.best_idx.max() >= c.n_keep and not np.all(np.diff(c.best_idx) > 0)
    assert c.Y.shape == (c.S, c.Lg) and c.n_keep == max(1, int(0.5 * c.S)) and np.all(c.best_costs > 0)
    assert 0 < c.obs.shape[0] < c.Lg // c.delta_x - (c.pixel_thresh - 1)


def test_default_fft_convolution_is_not_the_reference():
    """Why method="direct": the FFT form leaves rounding noise of ~1e-17 of the peak on pixels whose density is exactly zero, and
    the normalised image then differs from the reference on more than a tenth of the pixels (within the absolute bound)."""
    c = kc.case("leaving")
    y = kc.kept_curves(c)
    x = np.broadcast_to((c.x_st + np.arange(c.Lg)).astype(np.float64)[:, None], y.T.shape)
    fft = orc.kde_of_curves(np.stack([x, y.T], axis=-1), c.best_costs, c.M, c.N, method="fft")
    norm = kc.reference(c)[1]
    assert np.abs(fft - norm).max() < 4e-7 and np.mean(fft != norm) > 0.1


def test_tall_cases_reach_three_chunks_and_their_boundaries():
    for name, passes in (("tall_single", 1), ("tall_restage", 2)):
        c = kc.case(name)
        bands = kc.tile_bands(c)
        assert len(bands) == 3 and all(b == (0, c.M - 1) for b in bands) and all(chunks(b) == 3 for b in bands), (name, bands)
        assert -(-c.n_keep // NB) == passes
        y, x = kc.kept_curves(c), c.x_st + np.arange(c.Lg)
        for x0 in range(0, c.N, TX):  # every tile stages points on the boundary rows of its chunks
            own = y[:, (x >= x0 - 4) & (x <= x0 + TX + 3)]
            for v in (123.0, 123.5, 127.0, 128.5, 131.5, 255.999, 0.0, c.M - 1.0):
                assert np.any(own == v), (name, x0, v)
            # ... among them points that feed two chunks: grid rows floor(y) + 1, floor(y) + 2 inside the rows
            # 128 j - 3 .. 128 j + 132 of chunk j and of chunk j + 1
            rows = np.floor(own).astype(int) + 1
            for j in (0, 1):
                both = (rows + 1 >= H * (j + 1) - 3) & (rows <= H * j + H + 4)
                assert both.any(), (name, x0, j)
    c = kc.case("tall_restage")
    assert (c.N % 16, c.N % 4, c.n_keep - NB) == (5, 1, 22)
    assert kc.case("tall_single").N % 4 == 0  # (the vector form of the horizontal pass; tall_restage takes the scalar one)


def test_restage_129_has_one_curve_in_its_second_pass_and_two_chunks():
    c = kc.case("restage_129")
    assert c.n_keep - NB == 1 and c.N % 4 == 0
    assert all(chunks(b) == 2 for b in kc.tile_bands(c)), kc.tile_bands(c)
    inv = 1.0 / c.best_costs
    assert inv[128] / inv.sum() > 0.1  # (losing that curve moves the density by far more than the bound)


def test_leaving_has_removed_columns_an_empty_tile_and_the_edge_values():
    c = kc.case("leaving")
    ok, y = kc.survives(c), kc.kept_curves(c)
    assert 0.45 < 1.0 - ok.mean() < 0.65
    assert int((~ok.any(axis=0)).sum()) >= 2 + 17 and not ok[:, [4, 12]].any() and ok[:, [3, 5, 11, 13]].any(axis=0).all()
    bands = kc.tile_bands(c)
    assert bands[2] == (c.M, -1) and bands[0][1] >= 0 and bands[1][1] >= 0
    vals = y[ok]
    for v in (0.0, c.M - 1.0, np.nextafter(c.M - 1.0, 0.0), np.nextafter(0.0, 1.0)):
        assert np.any(vals == v)
    assert np.any((vals == 0.0) & np.signbit(vals))  # -0.0 survives
    gone = y[~ok]
    assert np.any(gone == np.nextafter(c.M - 1.0, np.inf)) and np.any(gone == np.nextafter(0.0, -1.0))
    assert (c.N % 16, c.N % 4) == (5, 1)
    # bands clipped at the first and the last rows of the image
    assert bands[0][0] == 0 and bands[0][1] == c.M - 1


def test_tiny_M_is_below_the_tap_count_and_clipped_at_both_ends():
    c = kc.case("tiny_M")
    assert c.M < 9
    assert all(b == (0, c.M - 1) for b in kc.tile_bands(c))
    ok = kc.survives(c)
    assert 0 < (~ok).sum() < ok.size


def test_small_W_cases():
    c = kc.case("small_W")
    assert 1.0 - kc.survives(c).mean() > 0.9 and 0.0 < kc.total_weight(c) < 1.0
    assert all(b[1] >= 0 for b in kc.tile_bands(c))
    assert np.log10(c.best_costs.max() / c.best_costs.min()) > 5.0
    p = kc.case("small_W_pow2")
    assert abs(kc.total_weight(p) - 8.0) < 1e-12
    assert np.log10(p.best_costs.max() / p.best_costs.min()) > 5.0


def test_span_edges_sit_on_either_side_of_the_tile_predicate():
    """band = (x0 + 16 + 4 > x_st) and (x0 - 4 <= x_en): a tile takes part when one of its 24 staged columns is on the edge."""
    def takes_part(x0, x_st, x_en):
        return x0 + TX + 4 > x_st and x0 - 4 <= x_en
    cs = kc.case("span_edges")
    assert [(c.x_st, c.x_st + c.Lg - 1) for c in cs] == [(19, 43), (20, 44), (21, 59), (4, 27)]
    assert takes_part(0, 19, 43) and not takes_part(0, 20, 44) and not takes_part(0, 21, 59)
    assert not takes_part(48, 19, 43) and takes_part(48, 20, 44)
    assert takes_part(32, 4, 27) is False and takes_part(16, 4, 27) and takes_part(0, 4, 27)
    for c in cs:
        for t, b in enumerate(kc.tile_bands(c)):
            assert (b[1] >= 0) == takes_part(t * TX, c.x_st, c.x_st + c.Lg - 1), (c.name, t, b)
        assert (c.M, c.N, c.n_keep) == (64, 64, 30)


def test_f32_samples_are_off_the_f32_grid():
    c = kc.case("f32_samples")
    raw = c.Y[c.best_idx]
    assert c.sample_dtype == "f32" and np.mean(raw != kc.kept_curves(c)) > 0.9
    ok = kc.survives(c)
    assert 0.1 < ok.mean() < 0.9


def selection(c):
    fobs, thresh, done = kc.expected_selection(c, c.kde)
    return [tuple(v) for v in fobs.tolist()], thresh, done


def score(c, xy):
    iv, gv = float(c.kde[xy[1], xy[0]]), float(c.grad_kde[xy[1], xy[0]])
    return 1 / 3 * (iv * gv + iv + gv)


@pytest.mark.parametrize("shape", list(kc.RULE_SHAPES))
@pytest.mark.parametrize("rule", kc.RULES)
def test_pixel_rule_cases_hold_their_situation(rule, shape):
    c = kc.rule_case(rule, shape)
    M, N, x_st, Lg, dx = kc.RULE_SHAPES[shape]
    if rule not in ("kde_threshold", "old_on_low_kde"):  # multiples of 1/8 (1/16 after the halving of five_decays)
        assert np.array_equal(c.kde * 16, np.round(c.kde * 16)) and np.array_equal(c.grad_kde * 16, np.round(c.grad_kde * 16))
    n_bins = len(set(np.round((np.arange(N) - x_st) / dx).astype(int).tolist()))
    assert (n_bins > 64) == (dx == 2)
    fobs, thresh, done = selection(c)
    m = c.marks
    if "tied" in m:
        assert len(set(score(c, xy) for xy in m["tied"])) == 1 and score(c, m["winner"]) == c.kde.max() == 1.0
        assert m["winner"] in fobs and not any(xy in fobs for xy in m["tied"] if xy != m["winner"])
    if rule == "column_ties":
        ys = sorted(xy[1] for xy in m["tied"])
        assert ys[1] % 8 != ys[0] % 8 and ys[2] - ys[0] == 8 and (M < 74 or ys[3] - ys[0] == 64)
    if rule == "bin_ties":
        (xa, ya), (xb, yb) = m["tied"]
        assert xa > xb and ya < yb and np.round((xa - x_st) / dx) == np.round((xb - x_st) / dx)
        assert dx != 2 or (xa - x_st) / dx % 1 == 0.5  # (a half that rounds to the even bin)
    if "absent" in m:
        assert m["absent"] not in fobs
    if "present" in m:
        assert m["present"] in fobs
    if "count" in m:
        assert len(fobs) == m["count"]
    if rule == "kde_threshold":
        assert float(c.kde[m["present"][1], m["present"][0]]) > 1e-3 > float(c.kde[m["absent"][1], m["absent"][0]]) > 0.999e-3
    if rule == "five_decays":
        assert thresh <= 0.95 ** 5 * (1 + 1e-12)
    if rule == "algo_thresh_ends":
        algo = Lg // dx - (c.pixel_thresh - 1)
        assert done == 1 and len(fobs) == algo and len(fobs) - c.obs.shape[0] < c.pixel_thresh and thresh < 1.0
    else:
        assert len(fobs) - c.obs.shape[0] >= c.pixel_thresh or done


def test_a_threshold_decayed_by_095_never_reaches_zero():
    """Why k_pix_select cannot wait for `thresh == 0` to leave the reference's endless loop: in f64 the decay stops at nine units
    of the smallest subnormal, where x * 0.95 rounds back to x."""
    t, n = 1.0, 0
    while t * 0.95 != t:
        t, n = t * 0.95, n + 1
    assert t == 9 * 5e-324 and t > 0.0 and 14000 < n < 15000
