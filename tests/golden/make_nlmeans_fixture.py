#!/opt/conda/bin/python3.9
"""tests/golden/nlmeans.npz: what the UNMODIFIED reference's gpet_utils.denoise(image, 'nl', kwargs) (gpet_utils.py:133-134) =
scikit-image 0.18.3's denoise_nl_means returns with fast_mode=False on small seeded frames.  Needs the build container's second
interpreter, like make_denoise_fixture.py (the reference's gpet_utils.py is loaded as a file, unmodified):

    /opt/conda/bin/python3.9 tests/golden/make_nlmeans_fixture.py

Stored per case: the input's key, the keyword arguments, the expected image, the key of the taps this run's numpy formed for it
(tests/nlmeans_ref.py: taps, evaluated here, under the numpy the library ran with; texp_s<s>: the s * s exponentials they were
made of) and the largest final patch distance any candidate reached.  Stored besides: skimage._shared.fast_exp on a grid of
arguments in [-30, 0] with each grid point's two float neighbours, and the versions line.  Asserted here, for every case: the
restatement with the stored taps equals the library's output (array_equal); no final distance exceeds 708 (beyond, the library's exponential is undefined); for the case built for
it, that a distance above the 5.0 cutoff at a row start ended under it (the weight stays 0).
"""
import importlib.util
import json
import math
import os
import sys
import warnings

# numpy's AVX-512 kernel of exp differs from the C library's exp by one unit in the last place for some arguments (exp(-2) among
# them), and taps made of such exponentials differ by up to four units from taps made of the C library's, because the
# normalising sum moves with them.  The library is therefore run with that kernel switched off (numpy reads the variable when it
# is imported): the exponentials of the stored taps are then the C library's -- asserted below -- which is what numpy gives
# wherever it has no kernel of its own for an argument, whatever its version.  Nothing of the reference or scikit-image changes.
os.environ.setdefault("NPY_DISABLE_CPU_FEATURES", "AVX512F")
import numpy as np  # noqa: E402

warnings.simplefilter("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402
from tests import nlmeans_ref as R  # noqa: E402
from tests.denoise_ref import make_frame  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_gpet_utils", os.path.join(ref_harness.REFERENCE_ROOT, "gp_edge_tracing", "gpet_utils.py"))
ref_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_utils)
import skimage  # noqa: E402
from skimage._shared.fast_exp import fast_exp  # noqa: E402

DT = dict(u8=np.uint8, u16=np.uint16, f32=np.float32, f64=np.float64)
arrays, cases = {}, []


def taps_key(s, h):
    key = "taps_s%d_h%r" % (R.odd_patch(s), float(h))
    if key not in arrays:
        arrays[key] = R.taps(s, h)
        te = arrays["texp_s%d" % R.odd_patch(s)] = np.exp(R.tap_arguments(s))  # (this run's exponentials: numpy builds differ in the last place)
        assert all(float(e) == math.exp(float(a)) for e, a in zip(te.ravel(), R.tap_arguments(s).ravel()))  # (the C library's)
    return key


def add(name, key, kw, promote=False, fell_back=False):
    img = arrays["in_" + key]
    src = img.astype(np.float64) if promote else img  # (a float32 frame: the device widens it and works in float64)
    out = ref_utils.denoise(src, "nl", dict(kw, fast_mode=False))
    assert out.dtype == np.float64 and out.shape == img.shape
    tk = taps_key(kw.get("patch_size", 7), kw.get("h", 0.1))
    mine, info = R.nlmeans_kwargs(src, kw, w=arrays[tk], return_info=True)
    assert np.array_equal(mine, out), name
    assert info["dmax"] <= 708.0, (name, info)
    assert info["fell_back"] or not fell_back, name
    arrays["exp_" + name] = out
    cases.append(dict(name=name, input=key, kwargs=kw, promote=promote, taps=tk, dmax=info["dmax"], fell_back=bool(info["fell_back"])))


# ---- float64: frame sizes x (patch, distance) x sigma -----------------------------------------------------------------------------
SIZES = dict(a=(9, 11), b=(20, 70), c=(33, 65))
for k, (M, N) in SIZES.items():
    arrays["in_f64_" + k] = make_frame(40 + ord(k), M, N, 0.1, np.float64)
for k in SIZES:
    for s, d in ((3, 2), (4, 2), (5, 3), (7, 11)):
        for sigma in (0.0, 0.05):
            add("f64_%s_s%d_d%d_sig%g" % (k, s, d, sigma), "f64_" + k, dict(patch_size=s, patch_distance=d, h=0.1, sigma=sigma))
# h small: most candidates stop at the cutoff
add("f64_b_small_h", "f64_b", dict(patch_size=5, patch_distance=3, h=0.02))
assert cases[-1]["dmax"] <= 5.0 + 1e3
# the defaults, by leaving every key out
add("f64_a_defaults", "f64_a", dict())

# ---- a distance that crosses the cutoff and falls back (var2 > 0) ----------------------------------------------------------------
rs = np.random.RandomState(7)
spike = 0.5 + rs.normal(0.0, 0.01, (20, 40))
spike[10, 20] = 5.5
arrays["in_f64_spike"] = spike
add("f64_spike_falls_back", "f64_spike", dict(patch_size=5, patch_distance=3, h=0.1, sigma=0.2), fell_back=True)

# ---- the other pixel types: integer frames keep their range, so h is in their units ---------------------------------------------
for dt, h in (("u8", 25.0), ("u16", 6500.0), ("f32", 0.1)):
    arrays["in_%s_b" % dt] = make_frame(60 + len(dt), 20, 70, 0.1, DT[dt])
    for s, d in ((3, 2), (7, 11)):
        add("%s_b_s%d_d%d" % (dt, s, d), "%s_b" % dt, dict(patch_size=s, patch_distance=d, h=h, sigma=0.0 if s == 3 else 0.05 * h / 0.1),
            promote=dt == "f32")

# ---- the library's exponential ----------------------------------------------------------------------------------------------------
grid = np.linspace(-30.0, 0.0, 601)
args = np.unique(np.concatenate([grid, np.nextafter(grid, -np.inf), np.nextafter(grid, np.inf)]))
args = args[(args >= -30.0) & (args <= 0.0)]
arrays["fexp_args"] = args
arrays["fexp_vals"] = np.array([fast_exp["float64_t"](float(v)) for v in args])
assert all(R.fexp(float(v)) == e for v, e in zip(args, arrays["fexp_vals"]))
assert np.array_equal(R.fexp_array(args), arrays["fexp_vals"])

arrays["cases"] = np.array(json.dumps(cases))
arrays["dmax"] = np.array(max(c["dmax"] for c in cases))
arrays["versions"] = np.array("skimage %s numpy %s with NPY_DISABLE_CPU_FEATURES=%s (exp of the taps: the C library's)"
                              % (skimage.__version__, np.__version__, os.environ["NPY_DISABLE_CPU_FEATURES"]))
path = os.path.join(HERE, "nlmeans.npz")
np.savez_compressed(path, **arrays)
print("nlmeans.npz: %d cases, %d bytes, %s, largest final distance %.4g, fell back: %s" % (
    len(cases), os.path.getsize(path), arrays["versions"], float(arrays["dmax"]), [c["name"] for c in cases if c["fell_back"]]))
assert os.path.getsize(path) < 1000000
