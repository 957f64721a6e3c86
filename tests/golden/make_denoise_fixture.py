#!/opt/conda/bin/python3.9
"""tests/golden/denoise.npz: what the UNMODIFIED reference's gpet_utils.denoise (gpet_utils.py:122-158) returns for the four
techniques the device runs -- 'median', 'minimum', 'gaussian' (scipy.ndimage 1.7.1) and 'tvc' (scikit-image 0.18.3) -- on
small seeded frames.  Needs the build container's second interpreter, like make_readme_image.py (the reference's package
import pulls in a scikit-learn that interpreter does not have, so its gpet_utils.py is loaded as a file, unmodified):

    /opt/conda/bin/python3.9 tests/golden/make_denoise_fixture.py

Stored per case: the input's key, the keyword arguments, the expected image; for 'tvc' the number of iterations the reference
ran (found from the reference itself: its result with n_iter_max = n equals the unbounded one, with n - 1 it does not) and every
iteration's margin (|E_prev - E| - eps E_0) / (eps E_0) of the stopping test; for float64 'gaussian' the reference's own
taps and the largest change of the result when one exponential of the taps moves by one unit in the last place
(tests/denoise_ref.py: gaussian_exp_spread).  One 500 x 500 case per technique is stored as seed + SHA-256 of the expected bytes.
The conditions tests/test_denoise_fixture.py re-checks are asserted here.
"""
import hashlib
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

warnings.simplefilter("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import denoise_ref as R  # noqa: E402
import ref_harness  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_gpet_utils", os.path.join(ref_harness.REFERENCE_ROOT, "gp_edge_tracing", "gpet_utils.py"))
ref_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_utils)
import scipy  # noqa: E402
import skimage  # noqa: E402
from scipy.ndimage import filters as _nd_filters  # noqa: E402

DT = dict(u8=np.uint8, u16=np.uint16, f32=np.float32, f64=np.float64)
arrays, cases, big = {}, [], []


def frame(key, seed, M, N, noise, dt, levels=None):
    arrays["in_" + key] = R.make_frame(seed, M, N, noise, DT[dt], levels)
    return key


def tvc_iterations(img, kw, ref_out):
    """Iterations the reference ran, from the reference alone."""
    _, n, margins = R.tvc(img, kw.get("weight", 0.1), kw.get("eps", 2.0e-4), kw.get("n_iter_max", 200), return_info=True)
    assert np.array_equal(ref_utils.denoise(img, "tvc", dict(kw, n_iter_max=n)), ref_out)
    assert n == 1 or not np.array_equal(ref_utils.denoise(img, "tvc", dict(kw, n_iter_max=n - 1)), ref_out)
    return n, margins


def add(name, technique, key, kw, promote=False):
    img = arrays["in_" + key]
    src = img.astype(np.float64) if promote else img  # ('tvc' of a float32 frame: the device iterates in float64)
    out = ref_utils.denoise(src, technique, dict(kw))
    case = dict(name=name, technique=technique, input=key, kwargs=kw, promote=promote, dtype=str(out.dtype))
    arrays["exp_" + name] = out
    if technique == "tvc":
        n, margins = tvc_iterations(src, kw, out)
        assert np.abs(margins).min() >= 1e-6, (name, margins)
        case["n_iter"] = int(n)
        arrays["margins_" + name] = margins
    if technique == "gaussian":
        sig = R._pair(kw["sigma"])
        tr = kw.get("truncate", 4.0)
        if img.dtype == np.float64:
            for a in (0, 1):
                arrays["taps%d_%s" % (a, name)] = _nd_filters._gaussian_kernel1d(sig[a], 0, R.gaussian_radius(sig[a], tr))[::-1].copy()
            case["exp_spread"] = R.gaussian_exp_spread(img, kw["sigma"], tr, kw.get("mode", "reflect"))
        if img.dtype.kind == "u":
            _, accs = R.gaussian(img, kw["sigma"], tr, kw.get("mode", "reflect"), return_acc=True)
            gap = min(float(np.abs(a - np.rint(a)).min()) for a in accs)
            assert gap >= 1e-9, (name, gap)
    cases.append(case)


# ---- median / minimum: every pixel type x window x mode ------------------------------------------------------------------------
for dt in DT:
    frame("rank_" + dt, 11, 20, 70, 0.15, dt, levels=None if dt in ("u8", "u16") else 4096)
for dt in DT:
    for size in ((3, 3), (5, 5), (4, 3), (7, 1), (9, 9)):
        for mode in R.MODES:
            for tech in ("median", "minimum"):
                add("%s_%s_%dx%d_%s" % (tech, dt, size[0], size[1], mode), tech, "rank_" + dt, dict(size=list(size), mode=mode))
frame("rank_big_u8", 12, 128, 160, 0.2, "u8")
add("median_u8_big_int3", "median", "rank_big_u8", dict(size=3))
add("minimum_u8_big_int5", "minimum", "rank_big_u8", dict(size=5))

# ---- gaussian ------------------------------------------------------------------------------------------------------------------
for dt in DT:
    frame("gauss_" + dt, 21, 32, 72, 0.1, dt)
for dt in DT:
    add("gaussian_%s_s0.8" % dt, "gaussian", "gauss_" + dt, dict(sigma=0.8))
    add("gaussian_%s_s1.5" % dt, "gaussian", "gauss_" + dt, dict(sigma=1.5))
    add("gaussian_%s_s3.0_t3_nearest" % dt, "gaussian", "gauss_" + dt, dict(sigma=3.0, truncate=3.0, mode="nearest"))
    add("gaussian_%s_pair" % dt, "gaussian", "gauss_" + dt, dict(sigma=[2.0, 0.7]))

# ---- tvc -----------------------------------------------------------------------------------------------------------------------
frame("tvc_a", 31, 64, 64, 0.05, "f64")
frame("tvc_b", 32, 48, 100, 0.3, "f64")
frame("tvc_u8", 33, 40, 72, 0.1, "u8")
frame("tvc_u16", 34, 40, 72, 0.1, "u16")
frame("tvc_f32", 35, 40, 72, 0.1, "f32")
add("tvc_f64_a_w0.05", "tvc", "tvc_a", dict(weight=0.05))
add("tvc_f64_b_w0.1", "tvc", "tvc_b", dict(weight=0.1))
add("tvc_f64_b_w0.3", "tvc", "tvc_b", dict(weight=0.3, eps=1.0e-4))
add("tvc_f64_b_cap5", "tvc", "tvc_b", dict(weight=0.1, n_iter_max=5))
add("tvc_u8", "tvc", "tvc_u8", dict(weight=0.1))
add("tvc_u16", "tvc", "tvc_u16", dict(weight=0.2))
add("tvc_f32_promoted", "tvc", "tvc_f32", dict(weight=0.1), promote=True)
assert len({c["n_iter"] for c in cases if c["technique"] == "tvc"}) >= 3  # (stacks of them stop at different iterations)

# ---- one 500 x 500 frame per technique, as seed + digest ---------------------------------------------------------------------
for tech, dt, noise, kw in [("median", "u8", 0.2, dict(size=5)), ("minimum", "f32", 0.2, dict(size=[3, 4])),
                            ("gaussian", "u16", 0.2, dict(sigma=1.5)), ("tvc", "f64", 0.3, dict(weight=0.1))]:
    seed = 500 + len(big)
    img = R.make_frame(seed, 500, 500, noise, DT[dt])
    out = np.ascontiguousarray(ref_utils.denoise(img, tech, dict(kw)))
    rec = dict(technique=tech, seed=seed, noise=noise, pix=dt, kwargs=kw, dtype=str(out.dtype), sha256=hashlib.sha256(out.tobytes()).hexdigest())
    if tech == "tvc":
        n, margins = tvc_iterations(img, kw, out)
        assert np.abs(margins).min() >= 1e-6
        rec["n_iter"] = int(n)
        rec["margin_min"] = float(np.abs(margins).min())
    if tech == "gaussian":
        _, accs = R.gaussian(img, kw["sigma"], return_acc=True)
        assert min(float(np.abs(a - np.rint(a)).min()) for a in accs) >= 1e-9
    big.append(rec)

arrays["cases"] = np.array(json.dumps(cases))
arrays["big"] = np.array(json.dumps(big))
arrays["versions"] = np.array("skimage %s scipy %s numpy %s" % (skimage.__version__, scipy.__version__, np.__version__))
path = os.path.join(HERE, "denoise.npz")
np.savez_compressed(path, **arrays)
print("denoise.npz: %d cases, %d big, %d bytes, %s" % (len(cases), len(big), os.path.getsize(path), arrays["versions"]))
for c in cases:
    if "n_iter" in c:
        print(" ", c["name"], "n_iter", c["n_iter"], "min |margin| %.3g" % np.abs(arrays["margins_" + c["name"]]).min())
    if "exp_spread" in c:
        print(" ", c["name"], "exp spread %.3g" % c["exp_spread"])
print(" ", [(b["technique"], b.get("n_iter")) for b in big])
assert os.path.getsize(path) < 1000000
