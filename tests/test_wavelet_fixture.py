"""CPU tests that pin the restatement tests/wavelet_ref.py, and the package's table of filters, to tests/golden/wavelet.npz -- what
the unmodified reference's denoise(image, 'wavelet', kwargs) returned under scikit-image 0.18.3 / PyWavelets 1.1.1
(tests/golden/make_wavelet_fixture.py).  Filters, coefficients, sigma and -- with the fixture's thresholds -- the output are bit
for bit.  The restatement's OWN thresholds rest on a mean of squares summed in the device's order, not numpy's: every such mean
must lie within 2 (n - 1) 2^-53 relative of the fixture's, the distance any two summation orders of n non-negative terms can be
apart to first order (each of the n - 1 additions of either order is off by at most 2^-53 relative of a partial sum that does
not exceed the total)."""
import functools
import json
import os

import numpy as np
import pytest

from tests import wavelet_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "wavelet.npz"))
CASES = json.loads(str(FIX["cases"]))
NAMES = json.loads(str(FIX["names"]))
IDS = [c["name"] for c in CASES]


def case_args(case, **over):
    kw = case["kwargs"]
    args = dict(sigma=kw.get("sigma"), mode=kw.get("mode", "soft"), wavelet_levels=kw.get("wavelet_levels"),
                method=kw.get("method", "BayesShrink"), rescale_sigma=kw.get("rescale_sigma", True), ppf=float(FIX["ppf"]), c=case["c"],
                strict=False)
    args.update(over)
    return args


def case_input(case):
    img = FIX["in_" + case["input"]]
    return img.astype(np.float64) if case["promote"] else img


@functools.lru_cache(maxsize=None)
def restated(name, injected):
    """(output, info) of the restatement on a case, with the fixture's thresholds or its own; computed once."""
    case = [c for c in CASES if c["name"] == name][0]
    dec_lo = FIX["filt_%s_dec_lo" % case["kwargs"]["wavelet"]]
    return R.denoise_wavelet(case_input(case), dec_lo, thresholds=FIX["thr_" + name] if injected else None, return_info=True,
                             **case_args(case))


@pytest.mark.parametrize("name", NAMES)
def test_filters_follow_from_dec_lo_and_the_table_holds_them(name):
    from gaussian_process_edge_trace_amd import _lib
    lo, hi, rlo, rhi = R.filters(FIX["filt_%s_dec_lo" % name])
    for got, key in ((lo, "dec_lo"), (hi, "dec_hi"), (rlo, "rec_lo"), (rhi, "rec_hi")):
        assert np.array_equal(np.array(got), FIX["filt_%s_%s" % (name, key)]), key
    assert np.array_equal(np.array(_lib.wavelet_table()[name]), FIX["filt_%s_dec_lo" % name])
    assert len(lo) % 2 == 0 and 2 <= len(lo) <= 16


def test_the_table_is_the_fixtures_list_of_names():
    from gaussian_process_edge_trace_amd import _lib
    assert list(_lib.wavelet_table()) == NAMES and "bior2.2" not in NAMES and len(NAMES) == 18


def test_max_level_is_pywavelets():
    from gaussian_process_edge_trace_amd import _lib
    seen = 0
    for key in FIX.files:
        if key.startswith("maxlevel_"):
            shape, F = key[len("maxlevel_"):].split("_F")
            M, N = (int(v) for v in shape.split("x"))
            assert R.max_level(min(M, N), int(F)) == int(FIX[key]) == _lib.wavelet_max_level(min(M, N), int(F)), key
            seen += 1
    assert seen >= 10
    for case in CASES:
        assert case["levels"] == R.levels_of(FIX["in_" + case["input"]].shape, len(FIX["filt_%s_dec_lo" % case["kwargs"]["wavelet"]]),
                                             case["kwargs"].get("wavelet_levels"), strict=False)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sigma_and_coefficients_bit_for_bit(case):
    _, info = restated(case["name"], True)
    assert info["sigma"] == case["sigma"] and info["var"] == case["var"] and info["levels"] == case["levels"]
    if case["coeffs"]:
        L = case["levels"]
        assert np.array_equal(info["coeffs"][L - 1]["aa"], FIX["co_%s_aa" % case["name"]])
        for l in range(L):
            for k in R.BANDS:
                assert np.array_equal(info["coeffs"][l][k], FIX["co_%s_%s%d" % (case["name"], k, l + 1)]), (l, k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_output_with_the_fixtures_thresholds_bit_for_bit(case):
    out, _ = restated(case["name"], True)
    exp = FIX["exp_" + case["name"]]
    assert out.dtype == np.float64 and out.shape == exp.shape and np.array_equal(out, exp)
    if FIX["in_" + case["input"]].dtype.kind == "u":
        assert exp.min() >= 0.0 and exp.max() <= 1.0


@pytest.mark.parametrize("case", [c for c in CASES if c["kwargs"].get("method", "BayesShrink") == "BayesShrink"],
                         ids=[c["name"] for c in CASES if c["kwargs"].get("method", "BayesShrink") == "BayesShrink"])
def test_own_means_of_squares_within_the_bound_of_any_order(case):
    _, info = restated(case["name"], False)
    ms = FIX["ms_" + case["name"]]
    assert info["ms"].shape == ms.shape == (case["levels"], 3)
    for l in range(case["levels"]):
        for b, k in enumerate(R.BANDS):
            n = info["coeffs"][l][k].size
            print(case["name"], l, k, n, abs(info["ms"][l, b] - ms[l, b]) / ms[l, b], R.mean_bound(n))
            assert abs(info["ms"][l, b] - ms[l, b]) <= R.mean_bound(n) * ms[l, b], (l, k)
            # and the fixture's threshold is the formula on the fixture's mean
            assert FIX["thr_" + case["name"]][l, b] == R.bayes_thresh(float(ms[l, b]), case["var"])


def test_visushrink_threshold_is_sigma_times_c():
    case = [c for c in CASES if c["kwargs"].get("method") == "VisuShrink"][0]
    _, info = restated(case["name"], False)
    assert np.array_equal(info["thresholds"], FIX["thr_" + case["name"]]) and info["thresholds"][0, 0] == case["sigma"] * case["c"]
    out, _ = restated(case["name"], False)
    assert np.array_equal(out, FIX["exp_" + case["name"]])


def test_the_fixture_covers_what_it_claims():
    assert {c["nonzero"] % 2 for c in CASES if "sigma" not in c["kwargs"]} == {0, 1}  # (both forms of the median)
    sat = [c for c in CASES if c["input"] == "u8_sat_40x44"][0]
    assert sat["nonzero"] < 20 * 22                                                     # (exact zeros in dd1)
    above = [c for c in CASES if c["levels"] > c["max_level"]]
    assert [c["name"] for c in above] == ["f64_48x80_db8_l2"]                            # (the one case the device refuses)
    with pytest.raises(ValueError, match="wavelet_levels"):
        R.denoise_wavelet(case_input(above[0]), FIX["filt_db8_dec_lo"], **case_args(above[0], strict=True))
    assert os.path.getsize(os.path.join(HERE, "golden", "wavelet.npz")) < os.path.getsize(os.path.join(HERE, "golden", "denoise.npz"))


def test_all_zero_finest_band_has_no_sigma():
    assert R.sigma_est(np.zeros((4, 5))) is None
    with pytest.raises(ValueError, match="all zero"):
        R.denoise_wavelet(np.full((8, 8), 0.5), FIX["filt_db1_dec_lo"])


def test_shrink_keeps_the_sign_of_a_zero():
    x = np.array([0.0, -0.0, 0.3, -0.3, 0.05, -0.05])
    s = R.shrink(x, 0.1, "soft")
    assert np.array_equal(np.signbit(s), np.signbit(x)) and s[0] == 0 and s[4] == 0 and s[2] == 0.3 * (1 - 0.1 / 0.3)
    h = R.shrink(x, 0.1, "hard")
    assert list(h) == [0.0, 0.0, 0.3, -0.3, 0.0, 0.0]
