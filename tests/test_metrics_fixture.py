"""The numpy restatement of the denoise quality metrics (tests/metrics_ref.py) against tests/golden/denoise_metrics.npz, what
scikit-image 0.18.3 itself computes (made by tests/golden/make_metrics_fixture.py): the SSIM map bit for bit, the counts exactly, the
four figures -- summed in the device's order -- within the bounds of DESIGN.md section 9.  No GPU."""
import json
import os

import numpy as np
import pytest

from tests import metrics_ref as R

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoise_metrics.npz"))
CASES = json.loads(str(FIX["cases"]))
FIGS = ("psnr", "ssim", "nrmse", "entropy")


def case_bounds(case):
    """The bound of every figure for a case, from the library's own figures and map."""
    name, kw = case["name"], case["kwargs"]
    a, b, lib, S = FIX["a_" + name], FIX["b_" + name], FIX["lib_" + name], FIX["map_" + name]
    pad = (kw.get("win_size", 7) - 1) // 2
    crop = S[pad:S.shape[0] - pad, pad:S.shape[1] - pad]
    return R.bounds(a.size, crop.size, float(np.abs(crop).mean()), np.unique(b).size, lib[0], lib[2], lib[3])


def test_the_fixture_covers_the_cases():
    names = {c["name"] for c in CASES}
    shapes = {FIX["a_" + n].shape for n in names}
    assert {(7, 7), (7, 9), (37, 53), (70, 130)} <= shapes
    pairs = {(FIX["a_" + n].dtype.name, FIX["b_" + n].dtype.name) for n in names}
    assert {("uint8", "uint8"), ("uint16", "uint16"), ("float32", "float32"), ("float64", "float64"), ("uint8", "float64"),
            ("float32", "float64")} <= pairs
    kws = [c["kwargs"] for c in CASES]
    assert {3, 11} <= {k.get("win_size") for k in kws} and any(k.get("use_sample_covariance") is False for k in kws)
    assert any("data_range" in k for k in kws)
    lib = FIX["lib_identical_f64"]
    assert lib[0] == np.inf and lib[2] == 0.0
    b = FIX["b_signed_zeros_f64"]
    assert np.signbit(b[b == 0.0]).any() and not np.signbit(b[b == 0.0]).all()
    assert np.unique(FIX["b_few_values_u8"]).size <= 8 and np.unique(FIX["b_all_distinct_f64"]).size == FIX["b_all_distinct_f64"].size
    a, b = FIX["a_mid_u16"], FIX["b_mid_u16"]
    assert np.mean(R.sq_diffs(a, b)) != np.mean(R.sq_diffs(a.astype(np.float64), b.astype(np.float64)))
    margin = json.loads(str(FIX["margin"]))
    assert set(margin) == set(FIGS) and all(0.0 <= v <= 1.0 for v in margin.values())


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_against_the_library(case):
    name, kw = case["name"], case["kwargs"]
    a, b, lib, S = FIX["a_" + name], FIX["b_" + name], FIX["lib_" + name], FIX["map_" + name]
    m = R.figures(a, b, **kw)
    assert np.array_equal(m["ssim_map"], S)
    assert np.array_equal(np.sort(m["counts"]), np.sort(np.unique(b, return_counts=True)[1]))
    bd = case_bounds(case)
    for j, fig in enumerate(FIGS):
        print(name, fig, m[fig], lib[j], bd[fig])
        assert R.within(m[fig], float(lib[j]), bd[fig]), (fig, m[fig], lib[j], bd[fig])


def test_the_refusals_of_the_restatement():
    a = FIX["a_mid_f64"]
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        R.figures(a[:5], a[:5])
    with pytest.raises(ValueError, match="Window size must be odd"):
        R.figures(a, a, win_size=8)
    with pytest.raises(ValueError, match="outside the range expected"):
        R.figures(a * 3.0, a)
    assert np.isfinite(R.figures(a * 3.0, a, data_range=3.0)["psnr"])
