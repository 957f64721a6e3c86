"""CPU tests of tests/label_ref.py, the numpy restatement of the label-map rules (csrc/gpet_label_plan.h) every other label-map test
compares against: Rule 1 against the reference's own mask (gpet_utils.py:303-307) and the package's Dice / Jaccard score, Rule 2 against
exact rational arithmetic and, on convex polygons, against the sign test of the cross products."""
from fractions import Fraction

import numpy as np
import pytest

from tests import label_ref as R


def eighths(rng, lo, hi, size):
    """Coordinates that are multiples of 1/8 in [lo, hi]: with pixel coordinates below 2^20 every difference and product of Rule 2 is
    exact in float64."""
    return rng.integers(int(lo * 8), int(hi * 8) + 1, size=size) / 8.0


@pytest.mark.parametrize("n", [16, 33])
def test_one_edge_is_the_references_mask(n):
    rng = np.random.default_rng(n)
    trace = np.stack([rng.integers(0, n, size=n), np.arange(n)], axis=1)
    mask = np.zeros((n, n), dtype=np.uint8)
    for c in range(n):  # gpet_utils.py:303-307: pred_bin[int(row[c]):, c] = 1
        mask[int(trace[c, 0]):, c] = 1
    got = R.trace_maps([trace], (n, n))
    assert got.shape == (1, n, n) and got.dtype == np.uint8 and np.array_equal(got[0], mask)
    assert np.array_equal(got[0], (np.arange(n)[:, None] >= trace[:, 0][None, :]).astype(np.uint8))


def test_dice_and_jaccard_of_two_maps_are_the_packages_scores():
    from gaussian_process_edge_trace_amd import gpet_utils as U
    n = 48
    rng = np.random.default_rng(7)
    pred = np.stack([np.clip(20 + rng.integers(-6, 7, size=n), 0, n - 1), np.arange(n)], axis=1)
    true = np.stack([np.clip(22 + rng.integers(-3, 4, size=n), 0, n - 1), np.arange(n)], axis=1)
    pb, tb = (R.trace_maps([t], (n, n))[0].astype(float) for t in (pred, true))
    jacc = np.sum(pb * tb) / np.sum(np.clip(pb + tb, 0, 1))
    assert np.round(jacc, 4) == U.trace_dicecoef(pred, true, jaccard=True)
    assert np.round(2 * jacc / (jacc + 1), 4) == U.trace_dicecoef(pred, true)


@pytest.mark.parametrize("extend", [False, True])
def test_thickness_sums_to_the_rows_of_the_frame(extend):
    M, N = 21, 37
    rng = np.random.default_rng(3)
    x_st = [0, 5, 0, 30, 2]
    lens = [37, 20, 10, 7, 35]
    rows = [rng.integers(-4, M + 5, size=n) for n in lens]
    rows[1][3] = R.NO_ROW
    map_of = [0, 1, 0, -1, 0]
    label = R.row_maps((M, N), x_st, rows, map_of, extend=extend)
    L = R.most_edges(map_of, 5)
    thick = R.thick_of(label, L)
    assert L == 3 and thick.shape == (2, 4, N) and thick.dtype == np.int32
    assert np.array_equal(thick.sum(axis=1), np.full((2, N), M))
    assert label.max() <= 3 and np.array_equal(R.row_maps((M, N), x_st, rows, map_of, extend, transposed=True), label.transpose(0, 2, 1))


def exact_inside(px, py, xy):
    """Rule 2 in rational arithmetic."""
    n, odd = len(xy), False
    for j in range(n):
        (xi, yi), (xj, yj) = xy[j], xy[(j + 1) % n]
        if (yi > py) != (yj > py):
            a, b = (px - xi) * (yj - yi), (xj - xi) * (py - yi)
            if (a < b) if yj > yi else (a > b):
                odd = not odd
    return odd


@pytest.mark.parametrize("n", [4, 5, 9, 17])
def test_rule_two_equals_exact_parity_on_every_pixel(n):
    Ms, Ns = 13, 15
    rng = np.random.default_rng(100 + n)
    xy = np.stack([eighths(rng, -2, Ns + 1, n), eighths(rng, -2, Ms + 1, n)], axis=1)
    xy[0] = (3.0, 4.0)  # a vertex on a pixel, a horizontal segment on a pixel row
    xy[1] = (9.0, 4.0)
    got = R.inside((Ms, Ns), xy)
    fx = [(Fraction(float(x)), Fraction(float(y))) for x, y in xy]
    want = np.array([[exact_inside(Fraction(px), Fraction(py), fx) for px in range(Ns)] for py in range(Ms)])
    assert np.array_equal(got, want)
    assert got.any() or n == 4


@pytest.mark.parametrize("n", [4, 7, 12])
def test_rule_two_on_convex_polygons_is_the_sign_test(n):
    Ms, Ns = 24, 26
    # vertices on an ellipse, rounded to eighths: convex as long as the rounding is small against the curvature
    th = 2.0 * np.pi * (np.arange(n) + 0.37) / n
    xy = np.stack([np.rint((12.6 + 10.2 * np.cos(th)) * 8) / 8, np.rint((11.3 + 9.1 * np.sin(th)) * 8) / 8], axis=1)
    got = R.inside((Ms, Ns), xy)
    checked = 0
    for py in range(Ms):
        for px in range(Ns):
            cr = [(xy[(j + 1) % n, 0] - xy[j, 0]) * (py - xy[j, 1]) - (xy[(j + 1) % n, 1] - xy[j, 1]) * (px - xy[j, 0]) for j in range(n)]
            if any(v == 0 for v in cr):
                continue  # on an edge line
            checked += 1
            assert got[py, px] == (all(v > 0 for v in cr) or all(v < 0 for v in cr)), (px, py)
    assert checked > Ms * Ns // 2 and got.sum() > 100


def test_an_outline_with_a_vertex_that_is_not_finite_contributes_nothing():
    sq = np.array([[2.0, 2.0], [8.0, 2.0], [8.0, 8.0], [2.0, 8.0]])
    bad = sq.copy()
    bad[2, 0] = np.nan
    maps = R.outline_maps((10, 10), [sq, bad, sq * 0.5 + 2.5], map_of=[0, 0, 0])
    assert set(np.unique(maps)) == {0, 1, 2} and maps[0, 5, 5] == 2 and maps[0, 2, 2] == 1 and maps[0, 8, 8] == 0
