"""tests/tvb_ref.py, the restatement of scikit-image 0.18.3's denoise_tv_bregman, against tests/golden/tvb.npz (written by the
unmodified reference; tests/golden/make_tvb_fixture.py): both forms -- raster order and a whole anti-diagonal at a time -- give
every stored output bit for bit, the stored sweep counts and every sweep's rmse in both orders of adding; and the margin
condition under which the device's order of adding cannot change a sweep count is recomputed here."""
import json
import os

import numpy as np
import pytest

from tests import tvb_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "tvb.npz"))
CASES = json.loads(str(FIX["cases"]))


def args_of(case):
    kw = case["kwargs"]
    return dict(weight=kw["weight"], max_iter=kw.get("max_iter", 100), eps=kw.get("eps", 1e-3), isotropic=kw.get("isotropic", True))


def source(case):
    img = FIX["in_" + case["input"]]
    return img.astype(np.float64) if case["promote"] else img


@pytest.fixture(scope="module")
def runs():
    """Every case once per form (the reference of the tests below, computed once and left unchanged)."""
    out = {}
    for case in CASES:
        out[case["name"]] = {form: R.denoise_tv_bregman(source(case), form=form, order=order, return_info=True, **args_of(case))
                             for form, order in (("raster", "raster"), ("diagonal", "device"))}
    return out


def test_the_fixture_holds_the_cases_the_stage_is_pinned_on():
    shapes = {c["name"]: FIX["in_" + c["input"]].shape for c in CASES}
    for s in ((2, 2), (2, 9), (9, 2), (9, 13), (12, 7), (17, 17), (65, 70), (70, 65), (33, 65), (21, 19), (26, 30)):
        assert s in shapes.values(), s
    dtypes = {str(FIX["in_" + c["input"]].dtype) for c in CASES}
    assert dtypes == {"uint8", "uint16", "float32", "float64"}
    assert {c["kwargs"]["weight"] for c in CASES} >= {0.5, 5, 10}
    assert {c["stopped_by"] for c in CASES} == {"eps", "max_iter"} and any(c["kwargs"].get("isotropic") is False for c in CASES)
    assert [c for c in CASES if c["name"] == "f64_17x17_7sweeps"][0]["kwargs"] == dict(weight=5, max_iter=7, eps=0)
    assert len({c["n_iter"] for c in CASES if c["name"] in ("f64_9x13", "f64_9x13_b", "f64_9x13_c")}) == 3
    assert os.path.getsize(os.path.join(HERE, "golden", "tvb.npz")) < os.path.getsize(os.path.join(HERE, "golden", "denoise.npz"))
    assert str(FIX["versions"]).startswith("skimage 0.18.3")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
@pytest.mark.parametrize("form", ["raster", "diagonal"])
def test_restatement_equals_the_library(runs, case, form):
    out, info = runs[case["name"]][form]
    assert out.dtype == np.float64 and np.array_equal(out, FIX["exp_" + case["name"]])
    assert info["n_iter"] == case["n_iter"]
    assert np.array_equal(info["rmse_raster"], FIX["rmse_raster_" + case["name"]])
    assert np.array_equal(info["rmse_device"], FIX["rmse_device_" + case["name"]])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_stopping_rule_and_margin(case):
    a = args_of(case)
    n = FIX["in_" + case["input"]].size
    for key in ("rmse_raster_", "rmse_device_"):
        rm = FIX[key + case["name"]]
        assert len(rm) == case["n_iter"] <= a["max_iter"]
        assert all(v > a["eps"] for v in rm[:-1])  # (every sweep but the last asked for another)
        if case["stopped_by"] == "eps":
            assert rm[-1] <= a["eps"]
        else:
            assert len(rm) == a["max_iter"] and rm[-1] > a["eps"]
        # farther from eps than any two orders of adding n non-negative terms can be apart
        assert all(abs(v - a["eps"]) > R.acc_bound(n) * max(v, a["eps"]) for v in rm) and R.margin_ok(rm, a["eps"], n)
    rr, rd = FIX["rmse_raster_" + case["name"]], FIX["rmse_device_" + case["name"]]
    assert np.all(np.abs(rr - rd) <= R.acc_bound(n) * rr)


def test_input_conversion():
    u8 = FIX["in_u8_33x65"]
    assert np.array_equal(R.as_input(u8), u8.astype(np.float64) * (1.0 / 255.0))
    u16 = FIX["in_u16_21x19"]
    assert np.array_equal(R.as_input(u16), u16.astype(np.float64) * (1.0 / 65535.0))
    f32 = FIX["in_f32_26x30"]
    assert R.as_input(f32).dtype == np.float64 and np.array_equal(R.as_input(f32), f32.astype(np.float64))
    with pytest.raises(ValueError):
        R.denoise_tv_bregman(np.zeros((1, 5)), 5.0)
