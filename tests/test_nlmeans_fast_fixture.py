"""tests/golden/nlmeans_fast.npz (the unmodified reference's gpet_utils.denoise(image, 'nl', {..., fast_mode=True}) under
scikit-image 0.18.3, made by tests/golden/make_nlmeans_fast_fixture.py) against the two restatements the GPU tests use as their
reference (tests/nlmeans_fast_ref.py): the plain loops and the anti-diagonal walk with the per-pixel gather, array_equal for every
pixel type.  Runs without scikit-image."""
import json
import os

import numpy as np
import pytest

from tests import nlmeans_fast_ref as R

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlmeans_fast.npz"))
CASES = json.loads(str(FIX["cases"]))
IDS = [c["name"] for c in CASES]


def _src(c):
    img = FIX["in_" + c["input"]]
    return img.astype(np.float64) if c["promote"] else img


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_plain_loops_equal_the_reference(case):
    exp = FIX["exp_" + case["name"]]
    assert exp.dtype == np.float64 and np.array_equal(R.with_kwargs(R.nlmeans_fast_loops, _src(case), case["kwargs"]), exp)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_diagonal_walk_with_the_gather_equals_the_reference(case):
    assert np.array_equal(R.with_kwargs(R.nlmeans_fast, _src(case), case["kwargs"]), FIX["exp_" + case["name"]])


def test_the_batch_of_shifts_walked_side_by_side_does_not_matter():
    c = [c for c in CASES if c["name"] == "f64_b_s5_d3_sig0.05"][0]
    for batch_bytes in (1, 100000):
        assert np.array_equal(R.with_kwargs(R.nlmeans_fast, _src(c), c["kwargs"], batch_bytes=batch_bytes), FIX["exp_" + c["name"]])


def test_fixture_covers_what_the_gpu_tests_need():
    names = {c["name"] for c in CASES}
    assert {FIX["in_" + c["input"]].dtype.name for c in CASES} == {"uint8", "uint16", "float32", "float64"}
    f64 = [c for c in CASES if c["input"].startswith("f64_") and "patch_size" in c["kwargs"] and c["kwargs"]["h"] == 0.1]
    got = {(FIX["in_" + c["input"]].shape, c["kwargs"]["patch_size"], c["kwargs"]["patch_distance"], c["kwargs"]["sigma"]) for c in f64}
    want = {(shape, s, d, sigma) for shape in ((9, 11), (20, 70), (33, 65)) for s, d in ((3, 2), (4, 2), (5, 3), (7, 11)) for sigma in (0.0, 0.05)
            if (s, d) != (7, 11) or min(shape) >= 16}
    assert got == want and len(want) == 22
    assert "f64_b_small_h" in names and [c for c in CASES if c["name"] == "f64_b_small_h"][0]["cut_share"] > 0.5
    assert [c for c in CASES if c["kwargs"] == {}] and all(min(FIX["in_" + c["input"]].shape) >= 16 for c in CASES if c["kwargs"] == {})
    assert str(FIX["versions"]).startswith("skimage 0.18.3 ")


def test_float_cases_pin_the_order_of_the_sums():
    """Integer frames with sigma 0 sum exactly; a float frame does not: adding one pixel's terms in another order changes bits."""
    c = [c for c in CASES if c["name"] == "f64_b_s5_d3_sig0"][0]
    img, kw = _src(c), dict(R.DEFAULTS, **c["kwargs"])
    exp = FIX["exp_" + c["name"]]
    real = R.terms_in_order
    try:
        R.terms_in_order = lambda t_row, t_col: tuple(reversed(real(t_row, t_col)))
        swapped = R.nlmeans_fast(img, **kw)
    finally:
        R.terms_in_order = real
    assert not np.array_equal(swapped, exp) and np.allclose(swapped, exp, rtol=1e-12, atol=0)


def test_shift_table_and_ranges():
    t = R.shifts(2)
    assert len(t) == 15 and t[0] == (-2, 0, 0.5) and t[1] == (-2, 1, 1.0) and t[6] == (0, 0, 1.0) and t[12] == (2, 0, 0.5) and t[-1] == (2, 2, 1.0)
    assert R.integral_range(50, -3) == (3, 50) and R.integral_range(50, 0) == (1, 50) and R.integral_range(50, 3) == (1, 47)
    assert R.weight_range(50, -3, 2) == (5, 48) and R.weight_range(50, 0, 2) == (2, 48) and R.weight_range(50, 3, 2) == (2, 45)
    assert R.geometry(20, 70, 7, 11) == (7, 3, 11, 15, 50, 100) and R.geometry(9, 11, 4, 2) == (5, 2, 2, 5, 19, 21)
