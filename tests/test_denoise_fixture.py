"""The NumPy restatement of the four denoising techniques (tests/denoise_ref.py) against tests/golden/denoise.npz, which the
UNMODIFIED reference's gpet_utils.denoise wrote under scipy 1.7.1 / scikit-image 0.18.3 (tests/golden/make_denoise_fixture.py).
This is what makes the restatement a stand-in for the reference where the reference cannot run, and the conditions the fixture's
inputs must meet are re-checked here from the stored data.

One operation of the reference is not reproducible from machine to machine: scipy forms the Gaussian taps with numpy.exp, whose
vectorised forms differ from the C library's exp by one unit in the last place for some arguments (which ones depends on numpy's
version and the CPU).  So for float64 frames the fixture also stores the reference's own taps: with THEM the restatement must
give the reference's image bit for bit (every other operation is pinned), and the taps formed with the C library's exp -- the
restatement's and the device library's -- must agree with them to what such a disagreement can cause.  For float32, uint8 and
uint16 frames the result must be the reference's bit for bit with the restatement's own taps."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import denoise_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "denoise.npz"))
CASES = json.loads(str(FIX["cases"]))
BIG = json.loads(str(FIX["big"]))
IDS = [c["name"] for c in CASES]


def source(case):
    img = FIX["in_" + case["input"]]
    return img.astype(np.float64) if case["promote"] else img


def test_fixture_covers_what_the_issue_lists():
    names = set(IDS)
    assert len(names) == len(CASES)
    for tech in ("median", "minimum"):
        for dt in ("u8", "u16", "f32", "f64"):
            for size in ("3x3", "5x5", "4x3", "7x1", "9x9"):
                for mode in R.MODES:
                    assert "%s_%s_%s_%s" % (tech, dt, size, mode) in names
    for dt in ("u8", "u16", "f32", "f64"):
        assert {"gaussian_%s_s0.8" % dt, "gaussian_%s_s1.5" % dt, "gaussian_%s_pair" % dt} <= names
    assert {"tvc_f64_a_w0.05", "tvc_f64_b_w0.1", "tvc_u8", "tvc_u16", "tvc_f32_promoted", "tvc_f64_b_cap5"} <= names
    assert sorted(b["technique"] for b in BIG) == ["gaussian", "median", "minimum", "tvc"]
    assert "scipy 1.7.1" in str(FIX["versions"]) and "skimage 0.18.3" in str(FIX["versions"])
    for k in FIX.files:
        if k.startswith("in_"):
            assert FIX[k].shape[0] <= 128 and FIX[k].shape[1] <= 160
    assert os.path.getsize(os.path.join(HERE, "golden", "denoise.npz")) < 1000000


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_the_reference(case):
    img, exp, kw = source(case), FIX["exp_" + case["name"]], case["kwargs"]
    assert str(exp.dtype) == case["dtype"]
    if case["technique"] == "tvc":
        out, n_iter, margins = R.tvc(img, kw.get("weight", 0.1), kw.get("eps", 2e-4), kw.get("n_iter_max", 200), return_info=True)
        assert out.dtype == exp.dtype == np.float64 and np.array_equal(out, exp)
        assert n_iter == case["n_iter"]
        assert np.array_equal(margins, FIX["margins_" + case["name"]])
        return
    if case["technique"] == "gaussian" and img.dtype == np.float64:
        taps = [FIX["taps%d_%s" % (a, case["name"])] for a in (0, 1)]
        out = R.gaussian(img, kw["sigma"], kw.get("truncate", 4.0), kw.get("mode", "reflect"), taps=taps)
        assert out.dtype == exp.dtype and np.array_equal(out, exp)
        # the taps of the C library's exp: each within 4 units in the last place of the reference's (one from the exponential
        # itself, the rest from the sum it enters), and the image within 16 x what one such unit does to it
        sig = R._pair(kw["sigma"])
        for a in (0, 1):
            mine = R.gaussian_taps(sig[a], kw.get("truncate", 4.0))
            assert mine.shape == taps[a].shape and np.all(np.abs(mine - taps[a]) <= 4 * np.spacing(taps[a]))
        own = R.denoise(img, "gaussian", kw)
        assert case["exp_spread"] > 0 and np.abs(own - exp).max() <= 16 * case["exp_spread"]
        return
    out = R.denoise(img, case["technique"], kw)
    assert out.dtype == exp.dtype and out.shape == exp.shape
    assert np.array_equal(out, exp)


@pytest.mark.parametrize("case", [c for c in CASES if c["technique"] == "tvc"], ids=[c["name"] for c in CASES if c["technique"] == "tvc"])
def test_tvc_stopping_test_is_nowhere_near_a_tie(case):
    margins = FIX["margins_" + case["name"]]
    assert margins.size == case["n_iter"] - 1
    assert np.abs(margins).min() >= 1e-6
    capped = "n_iter_max" in case["kwargs"] and case["n_iter"] == case["kwargs"]["n_iter_max"]
    # every iteration but the last goes on (margin above 0); the last one stops (below 0) unless n_iter_max cut the run short
    assert np.all(margins[:-1] > 0) and (margins[-1] > 0 if capped else margins[-1] < 0)


def test_tvc_cases_stop_at_different_iterations():
    assert len({c["n_iter"] for c in CASES if c["technique"] == "tvc"}) >= 3


@pytest.mark.parametrize("case", [c for c in CASES if c["technique"] == "gaussian" and c["input"].endswith(("u8", "u16"))],
                         ids=lambda c: c["name"])
def test_integer_gaussian_is_nowhere_near_a_rounding_boundary(case):
    kw = case["kwargs"]
    _, accs = R.gaussian(source(case), kw["sigma"], kw.get("truncate", 4.0), kw.get("mode", "reflect"), return_acc=True)
    assert len(accs) == 2
    for acc in accs:  # scipy truncates: the boundaries are the integers
        assert np.abs(acc - np.rint(acc)).min() >= 1e-9


@pytest.mark.parametrize("rec", BIG, ids=[b["technique"] for b in BIG])
def test_500x500_cases(rec):
    dt = dict(u8=np.uint8, u16=np.uint16, f32=np.float32, f64=np.float64)[rec["pix"]]
    img = R.make_frame(rec["seed"], 500, 500, rec["noise"], dt)
    kw = rec["kwargs"]
    if rec["technique"] == "tvc":
        out, n_iter, margins = R.tvc(img, kw["weight"], return_info=True)
        assert n_iter == rec["n_iter"] and np.abs(margins).min() >= 1e-6
    else:
        out = R.denoise(img, rec["technique"], kw)
    if rec["technique"] == "gaussian":
        _, accs = R.gaussian(img, kw["sigma"], return_acc=True)
        assert min(float(np.abs(a - np.rint(a)).min()) for a in accs) >= 1e-9
    assert str(out.dtype) == rec["dtype"]
    assert hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest() == rec["sha256"]
