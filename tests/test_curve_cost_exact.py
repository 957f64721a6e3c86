"""The extended-precision curve cost (tests/curve_cost_exact.py) against the oracle's vectorised float64 one on the inputs of the
injected-scorer test (tests/test_gpu_score_injected.py), and the condition those inputs must meet for that test's tolerance."""
import decimal

import numpy as np
import pytest

from oracle import gpet_oracle as orc
from tests import curve_cost_exact as cx


def _cases():
    seen, out = set(), []
    for shape, S, dt in cx.CASES:
        if (shape, S, dt) not in seen:
            seen.add((shape, S, dt))
            out.append((shape, S, dt))
    return out


@pytest.fixture(scope="module")
def reference():
    """(image, samples, costs, condition numbers) of every case and of every edge of the batch, computed once."""
    out = {(shape, S, dt): cx.case_reference(shape, S, dt) for shape, S, dt in _cases()}
    grad, edges = cx.batch_reference()
    for (x_st, Lg), (Y, costs, cond) in zip(cx.BATCH_SPANS, edges):
        out[(grad.shape + (x_st, Lg), cx.BATCH_S, "batch")] = (grad, Y, costs, cond)
    return out


def test_extended_format_has_at_least_64_mantissa_bits():
    if cx.USE_DECIMAL:
        assert cx._CTX.prec == 40 and isinstance(cx._num(0.1), decimal.Decimal)
        assert cx._num(0.1) == decimal.Decimal(0.1)  # an exact copy of the double, not of its decimal text
    else:
        assert float(np.finfo(np.longdouble).eps) <= 2e-19
    a = cx._num(1.0) + cx._num(2.0 ** -60)
    assert a != cx._num(1.0) and float(a) == 1.0


def test_the_cases_are_the_ones_the_scorer_test_is_to_run():
    assert len(cx.FAMILIES) == 13 and len(_cases()) == len(cx.CASES) == 20
    for (M, N, x_st, Lg), S, dt in cx.CASES:
        assert 0 <= x_st and x_st + Lg <= N and Lg >= 4 and dt in ("f64", "f32")
    ends = [sh for sh in cx.SHAPES if sh[2] + sh[3] == sh[1] and sh[2] > 0]  # end at the image's last column, x_st > 0
    assert ends == [(12, 40, 3, 37), (33, 80, 46, 34), (12, 40, 35, 5)]
    assert sorted({(sh[3] - 2) // 2 for sh in cx.SHAPES}) == [1, 15, 16, 17, 19, 65]
    assert {(sh[3] & 1, S < 64) for sh, S, dt in cx.CASES if dt == "f32"} == {(0, False), (1, False), (0, True), (1, True)}


def test_curves_cover_the_families(reference):
    for (shape, S, dt), (grad, Y, _, _) in reference.items():
        M, Lg = shape[0], shape[3]
        assert Y.shape == (S, Lg) and grad.shape == shape[:2] and grad.dtype == np.float32
        assert 0.2 < np.mean(grad == 0) < 0.4 and grad.min() == 0 and grad.max() == 1
        fam = {n: Y[i::13] for i, n in enumerate(cx.FAMILIES)}
        assert np.all(fam["row0"] == 0) and np.all(fam["rowlast"] == M - 1)
        assert np.all(fam["below"] < 0) and np.all(fam["above"] > M - 1)
        assert np.all(fam["const_int"] == np.floor(fam["const_int"])) and np.all(fam["ints"] == np.floor(fam["ints"]))
        assert fam["ramp"].min() < 0 and fam["ramp"].max() > M - 1 and fam["uniform"].min() < 0 and fam["uniform"].max() > M - 1
        if dt != "f32":
            assert np.all(fam["near_int"] != np.floor(fam["near_int"] + 0.5))
            assert np.all(np.abs(fam["near_int"] - np.floor(fam["near_int"] + 0.5)) < 1e-14)
        assert np.all(fam["step_last"][:, -1] == M - 1) and np.all(fam["step_last"][:, :-1] == fam["step_last"][:, :1])


def test_oracle_agrees_to_1e_13(reference):
    worst = 0.0
    for (shape, S, dt), (grad, Y, costs, _) in reference.items():
        x_st, Lg = shape[2], shape[3]
        oc = orc.costs_batch(grad.astype(np.float64), np.arange(x_st, x_st + Lg), Y.T)
        dev = np.array([cx.rel_err(o, c) for o, c in zip(oc, costs)])
        worst = max(worst, dev.max())
        assert dev.max() <= 1e-13, (shape, S, dt, int(dev.argmax()), dev.max())
    print("oracle against the extended-precision cost: worst relative deviation %.2e" % worst)


def test_every_input_is_well_conditioned(reference):
    """A condition on the INPUTS, not a tolerance on anything: the scorer test's bound is proportional to the condition number."""
    worst = 0.0
    for (shape, S, dt), (_, _, _, cond) in reference.items():
        worst = max(worst, cond.max())
        assert np.all(cond >= 1.0) and cond.max() <= 32.0, (shape, S, dt, int(cond.argmax()), cond.max())
    print("largest condition number %.1f" % worst)


def test_few_draws_are_rejected_for_their_condition_number(reference):
    """curves() draws a row again when its condition number exceeds COND_DRAW.  That filter must stay marginal -- at most two
    draws of a call, of 40 to 1100 rows -- or a change of the image or of a family would quietly narrow the random families to
    their tame draws.  Today: one draw in each of four of the nineteen calls (uniform twice, step_last twice)."""
    assert len(cx.REDRAWS) == len({(sh, S) for sh, S, _ in _cases()}) + len(cx.BATCH_SPANS)
    for seed, rejected in cx.REDRAWS.items():
        assert set(rejected) <= set(cx.FAMILIES)
        assert sum(rejected.values()) <= 2, (seed, rejected)
    print("rejected draws:", {s: r for s, r in cx.REDRAWS.items() if r})


def test_single_curve_hand_values():
    """Lg = 4 on a constant image: three samples, one pair, straight line -> arc = 2 sqrt(2), line = 2 sqrt(2) (c + 1e-3)."""
    grad = np.full((5, 6), 0.5, dtype=np.float32)
    cost, cond = cx.curve_cost(grad, 1, [0.0, 1.0, 2.0, 3.0])
    assert cx.rel_err(1.0 / (0.5 + 1e-3), cost) < 1e-15 and abs(cond - 1.0) < 1e-15
    # Lg = 5, flat: four samples of unit spacing; Simpson over three and Cartwright's 5/12, 8/12, -1/12 add up to 3
    cost, cond = cx.curve_cost(grad, 0, [2.0] * 5)
    assert cx.rel_err(1.0 / (0.5 + 1e-3), cost) < 1e-15
    # the last point is no sample: it only ends the last segment (the arc's last integrand, the line integral's last spacing)
    a, _ = cx.curve_cost(grad, 0, [2.0, 2.0, 2.0, 2.0])
    b, _ = cx.curve_cost(grad, 0, [2.0, 2.0, 2.0, 4.5])
    assert cx.rel_err(float(a), b) > 1e-3
    grad2 = grad.copy()
    grad2[:, 3] = 0.0  # the last point's column is never sampled
    c, _ = cx.curve_cost(grad2, 0, [2.0, 2.0, 2.0, 4.5])
    assert c == b
