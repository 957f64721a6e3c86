"""tests/golden/nlmeans.npz (the unmodified reference's gpet_utils.denoise(image, 'nl', {..., fast_mode=False}) under scikit-image
0.18.3, made by tests/golden/make_nlmeans_fixture.py) against the restatement the GPU tests use as their reference
(tests/nlmeans_ref.py): the outputs array_equal for every pixel type, the integer-trick exponential bit for bit, and the
conditions under which parity is claimed."""
import json
import os

import numpy as np
import pytest

from tests import nlmeans_ref as R

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlmeans.npz"))
CASES = json.loads(str(FIX["cases"]))


def _src(c):
    img = FIX["in_" + c["input"]]
    return img.astype(np.float64) if c["promote"] else img


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_the_reference(case):
    out, info = R.nlmeans_kwargs(_src(case), case["kwargs"], w=FIX[case["taps"]], return_info=True)
    exp = FIX["exp_" + case["name"]]
    assert exp.dtype == np.float64 and np.array_equal(out, exp)
    assert info["dmax"] == case["dmax"] and info["fell_back"] == case["fell_back"]


def test_fixture_covers_what_the_gpu_tests_need():
    names = {c["name"] for c in CASES}
    assert {FIX["in_" + c["input"]].dtype.name for c in CASES} == {"uint8", "uint16", "float32", "float64"}
    assert {FIX["in_" + c["input"]].shape for c in CASES} >= {(9, 11), (20, 70), (33, 65)}
    assert max(FIX["in_" + c["input"]].shape[0] for c in CASES) <= 40 and max(FIX["in_" + c["input"]].shape[1] for c in CASES) <= 80
    assert {(R.odd_patch(c["kwargs"].get("patch_size", 7)), c["kwargs"].get("patch_distance", 11)) for c in CASES} >= {(3, 2), (5, 2), (5, 3), (7, 11)}
    assert any(c["kwargs"].get("patch_size") == 4 for c in CASES)  # (an even size: the next odd one)
    assert "f64_spike_falls_back" in names and [c for c in CASES if c["name"] == "f64_spike_falls_back"][0]["fell_back"]
    assert str(FIX["versions"]).startswith("skimage 0.18.3 ")


def test_largest_final_distance_is_inside_the_defined_range():
    assert float(FIX["dmax"]) == max(c["dmax"] for c in CASES) < 708.0


def test_small_h_stops_most_candidates_at_the_cutoff():
    c = [c for c in CASES if c["name"] == "f64_b_small_h"][0]
    img, kw = _src(c), c["kwargs"]
    w = FIX[c["taps"]]
    P, (M, N) = R.pad(img, 2), img.shape
    cut = total = 0
    for row, col in ((0, 0), (10, 35), (19, 69), (7, 3)):
        for i in range(*R.window(row, M, kw["patch_distance"])):
            for j in range(*R.window(col, N, kw["patch_distance"])):
                dist = 0.0
                for a in range(4):  # the distance before the last patch row starts
                    for b in range(5):
                        t = P[row + a, col + b] - P[i + a, j + b]
                        dist = dist + w[a, b] * (t * t)
                cut += dist > R.CUTOFF
                total += 1
    assert cut > total // 2


def test_plain_loop_of_one_pixel_equals_the_spread_out_loops():
    for name in ("f64_a_s7_d11_sig0.05", "f64_spike_falls_back", "u8_b_s3_d2"):
        c = [c for c in CASES if c["name"] == name][0]
        img, kw = _src(c), dict(R.DEFAULTS, **c["kwargs"])
        s = R.odd_patch(kw["patch_size"])
        w = FIX[c["taps"]]
        P, (M, N) = R.pad(img, s // 2), img.shape
        exp = FIX["exp_" + name]
        for row, col in ((0, 0), (M - 1, N - 1), (M // 2, N // 2), (M - 1, 0), (2, N - 3)):
            assert R.pixel(P, w, row, col, M, N, kw["patch_distance"], 2.0 * kw["sigma"] * kw["sigma"]) == exp[row, col], (name, row, col)


def test_fexp_equals_the_librarys_bit_for_bit():
    args, vals = FIX["fexp_args"], FIX["fexp_vals"]
    assert args.size >= 1500 and args.min() == -30.0 and args.max() == 0.0
    assert np.array_equal(R.fexp_array(args).view(np.uint64), vals.view(np.uint64))
    assert all(R.fexp(float(a)) == v for a, v in zip(args[::7], vals[::7]))
    assert R.fexp(0.0) == 0.9710078239440918 and R.fexp(-0.0) == R.fexp(0.0)
    assert R.fexp(-708.0) > 0.0 and R.fexp(np.nextafter(-708.0, -np.inf)) == 0.0 and R.fexp(-1e300) == 0.0
