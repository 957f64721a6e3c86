#!/opt/conda/bin/python3.9
"""tests/golden/wavelet.npz and the package's table of filters (gaussian_process_edge_trace_amd/wavelet_table.json): what the
UNMODIFIED reference's gpet_utils.denoise(image, 'wavelet', kwargs) (gpet_utils.py:137-138) = scikit-image 0.18.3's
denoise_wavelet on PyWavelets 1.1.1 returns on small seeded frames.  Needs the build container's second interpreter, like
make_denoise_fixture.py (the reference's gpet_utils.py is loaded as a file, unmodified):

    /opt/conda/bin/python3.9 tests/golden/make_wavelet_fixture.py [--time]

Stored per case: the input's key, the keyword arguments, the expected image, sigma and var as the library formed them, every
detail band's mean(x * x) and threshold as (levels, 3) arrays (level 1 = finest first; bands ad, da, dd), VisuShrink's
sqrt(2 log(M N)), and for the small cases every coefficient array.  Stored besides: PyWavelets' four filters of every name of the
table, dwtn_max_level of every (case shape, filter length), the ppf constant and the versions line.  Asserted here, for every
case: the restatement (tests/wavelet_ref.py) gives the library's filters, coefficients and sigma bit for bit, and with the
library's thresholds its output; its own mean(x * x) lies within 2 (n - 1) 2^-53 relative of numpy's; no band sits at the
max(., eps) switch; both parities of dd1's non-zero count occur.
``--time``: also prints the library's host time per 500 x 500 frame (what profiles/wavelet_timing.txt quotes)."""
import importlib.util
import json
import os
import sys
import time
import warnings

import numpy as np

warnings.simplefilter("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_harness  # noqa: E402
from tests import wavelet_ref as R  # noqa: E402
from tests.denoise_ref import make_frame  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_gpet_utils", os.path.join(ref_harness.REFERENCE_ROOT, "gp_edge_tracing", "gpet_utils.py"))
ref_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_utils)
import pywt  # noqa: E402
import scipy.stats  # noqa: E402
import skimage  # noqa: E402
from skimage.restoration import _denoise as SK  # noqa: E402

NAMES = ["haar"] + ["db%d" % k for k in range(1, 9)] + ["sym%d" % k for k in range(2, 9)] + ["coif1", "coif2"]
DT = dict(u8=np.uint8, u16=np.uint16, f32=np.float32, f64=np.float64)
arrays, cases = {}, []
PPF = float(scipy.stats.norm.ppf(0.75))
assert PPF == R.PPF75

# ---- the table --------------------------------------------------------------------------------------------------------------------
table = {}
for name in NAMES:
    w = pywt.Wavelet(name)
    assert w.orthogonal and w.dec_len % 2 == 0 and 2 <= w.dec_len <= 16
    for key in ("dec_lo", "dec_hi", "rec_lo", "rec_hi"):
        arrays["filt_%s_%s" % (name, key)] = np.array(getattr(w, key), dtype=np.float64)
    table[name] = ["%.17g" % v for v in w.dec_lo]
    assert [float(s) for s in table[name]] == list(w.dec_lo)
    for got, key in zip(R.filters(w.dec_lo), ("dec_lo", "dec_hi", "rec_lo", "rec_hi")):
        assert got == list(getattr(w, key)), (name, key)
with open(os.path.join(ROOT, "gaussian_process_edge_trace_amd", "wavelet_table.json"), "w") as f:
    f.write("{\n" + ",\n".join('  "%s": [%s]' % (n, ", ".join(table[n])) for n in NAMES) + "\n}\n")


def add(name, key, kw, promote=False, coeffs=False):
    img = arrays["in_" + key]
    src = img.astype(np.float64) if promote else img  # (a float32 frame: the device widens it and works in float64)
    out = ref_utils.denoise(src, "wavelet", dict(kw))
    assert out.dtype == np.float64 and out.shape == img.shape
    # the library's intermediates, by its own functions in its own order (skimage.restoration._denoise)
    w = pywt.Wavelet(kw.get("wavelet", "db1"))
    F = w.dec_len
    x, sigma = SK._scale_sigma_and_image_consistently(src, kw.get("sigma"), False, kw.get("rescale_sigma", True))
    top = pywt.dwtn_max_level(x.shape, w)
    arrays["maxlevel_%dx%d_F%d" % (x.shape[0], x.shape[1], F)] = np.array(top)
    assert top == R.max_level(min(x.shape), F)
    L = kw.get("wavelet_levels") or max(top - 3, 1)
    co = pywt.wavedecn(x, wavelet=w, level=L)
    det = co[1:][::-1]  # level 1 (finest) first
    nz = int(np.count_nonzero(det[0]["dd"]))
    if sigma is None:
        sigma = SK._sigma_est_dwt(det[0]["dd"], distribution="Gaussian")
    var = sigma ** 2
    assert float(var) == float(sigma) * float(sigma)
    method = kw.get("method", "BayesShrink")
    ms = np.array([[np.mean(d[k] * d[k]) for k in R.BANDS] for d in det])
    c = float(np.sqrt(2 * np.log(x.size)))
    if method == "BayesShrink":
        thr = np.array([[SK._bayes_thresh(d[k], var) for k in R.BANDS] for d in det])
        for l, d in enumerate(det):
            for b, k in enumerate(R.BANDS):
                n = d[k].size
                assert abs(ms[l, b] - var) > 2 * (n - 1) * 2.0 ** -53 * ms[l, b], (name, l, k)  # (not at the max(., eps) switch)
    else:
        thr = np.full((L, 3), SK._universal_thresh(x, sigma))
        assert thr[0, 0] == float(sigma) * c
    # the restatement against all of it
    args = dict(sigma=kw.get("sigma"), mode=kw.get("mode", "soft"), wavelet_levels=kw.get("wavelet_levels"), method=method,
                rescale_sigma=kw.get("rescale_sigma", True), ppf=PPF, c=c)
    mine, info = R.denoise_wavelet(src, w.dec_lo, thresholds=thr, return_info=True, strict=False, **args)
    assert info["levels"] == L and info["sigma"] == float(sigma) and info["var"] == float(var), name
    for l, d in enumerate(det):
        for k in R.BANDS:
            assert np.array_equal(info["coeffs"][l][k], d[k]), (name, l, k)
    assert np.array_equal(info["coeffs"][L - 1]["aa"], co[0]), name
    assert np.array_equal(mine, out), name
    if method == "BayesShrink":
        for l, d in enumerate(det):
            for b, k in enumerate(R.BANDS):
                assert abs(info["ms"][l, b] - ms[l, b]) <= R.mean_bound(d[k].size) * ms[l, b], (name, l, k)
    arrays["exp_" + name] = out
    arrays["ms_" + name] = ms
    arrays["thr_" + name] = thr
    if coeffs:
        arrays["co_%s_aa" % name] = co[0]
        for l, d in enumerate(det):
            for k in R.BANDS:
                arrays["co_%s_%s%d" % (name, k, l + 1)] = d[k]
    cases.append(dict(name=name, input=key, kwargs=kw, promote=promote, levels=int(L), sigma=float(sigma), var=float(var), c=c,
                      nonzero=nz, coeffs=bool(coeffs), max_level=int(top)))


def frame(key, seed, M, N, dt, noise=0.1):
    # (values on a grid of 1 / 1024, so that float64 inputs compress; still doubles with full-width products)
    arrays["in_" + key] = make_frame(seed, M, N, noise, DT[dt], levels=1024 if dt in ("f64", "f32") else None)


frame("f64_37x50", 11, 37, 50, "f64")
add("f64_37x50_db2", "f64_37x50", dict(wavelet="db2"), coeffs=True)
frame("f64_64x64", 12, 64, 64, "f64")
add("f64_64x64_db1", "f64_64x64", dict(wavelet="db1"))
frame("u8_33x65", 13, 33, 65, "u8")
add("u8_33x65_db1", "u8_33x65", dict(wavelet="db1"), coeffs=True)
frame("f64_40x72", 14, 40, 72, "f64")
add("f64_40x72_db4_hard_visu", "f64_40x72", dict(wavelet="db4", mode="hard", method="VisuShrink", sigma=0.05, wavelet_levels=2))
frame("u16_21x19", 15, 21, 19, "u16")
add("u16_21x19_sym4_l1", "u16_21x19", dict(wavelet="sym4", wavelet_levels=1), coeffs=True)
frame("f64_48x80", 16, 48, 80, "f64")
# (two levels are above dwtn_max_level = 1 of this frame: PyWavelets warns and computes, the device refuses -- the case pins the
# restatement; its sibling of 64 x 80, where two levels are allowed, is the one the device runs)
add("f64_48x80_db8_l2", "f64_48x80", dict(wavelet="db8", wavelet_levels=2))
assert cases[-1]["max_level"] == 1
frame("f64_64x80", 21, 64, 80, "f64")
add("f64_64x80_db8_l2", "f64_64x80", dict(wavelet="db8", wavelet_levels=2))
assert cases[-1]["max_level"] == 2
# the deepest input just at or above F: 30 x 34 under db8 (F = 16): max_level = 1, out_len = 22 x 24
frame("f64_30x34", 17, 30, 34, "f64")
add("f64_30x34_db8_l1", "f64_30x34", dict(wavelet="db8", wavelet_levels=1), coeffs=True)
# several tiles per axis, odd band extents, default levels (max_level 5 -> 2 levels)
frame("u8_130x150", 18, 130, 150, "u8")
add("u8_130x150_db2", "u8_130x150", dict(wavelet="db2"))
# a float32 frame against the widened input
frame("f32_26x30", 19, 26, 30, "f32")
add("f32_26x30_coif1", "f32_26x30", dict(wavelet="coif1"), promote=True)
# a saturated flat region: dd1 of db1 holds exact zeros there
sat = make_frame(20, 40, 44, 0.1, np.uint8)
sat[5:21, 8:30] = 255
arrays["in_u8_sat_40x44"] = sat
add("u8_sat_40x44_db1", "u8_sat_40x44", dict(wavelet="db1"))
assert cases[-1]["nonzero"] < 20 * 22
# a given sigma on an integer frame, rescaled and not
add("u8_33x65_sym2_sigma_rescaled", "u8_33x65", dict(wavelet="sym2", sigma=12.0, rescale_sigma=True))
add("u8_33x65_sym2_sigma_as_given", "u8_33x65", dict(wavelet="sym2", sigma=0.05, rescale_sigma=False))
assert {c["nonzero"] % 2 for c in cases if "sigma" not in c["kwargs"]} == {0, 1}, [c["nonzero"] for c in cases]

arrays["cases"] = np.array(json.dumps(cases))
arrays["names"] = np.array(json.dumps(NAMES))
arrays["ppf"] = np.array(PPF)
arrays["versions"] = np.array("skimage %s pywt %s numpy %s" % (skimage.__version__, pywt.__version__, np.__version__))
path = os.path.join(HERE, "wavelet.npz")
np.savez_compressed(path, **arrays)
print("wavelet.npz: %d cases, %d bytes, %s, non-zero counts %s" % (len(cases), os.path.getsize(path), arrays["versions"],
                                                                   [c["nonzero"] for c in cases]))
assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "denoise.npz"))

if "--time" in sys.argv:
    img = make_frame(3, 500, 500, 0.1, np.uint8)
    for wname in ("db1", "db4"):
        ref_utils.denoise(img, "wavelet", dict(wavelet=wname))
        t0 = time.perf_counter()
        for _ in range(5):
            ref_utils.denoise(img, "wavelet", dict(wavelet=wname))
        print("host, scikit-image %s / PyWavelets %s: 500 x 500 uint8, %s, default levels: %.2f ms per frame"
              % (skimage.__version__, pywt.__version__, wname, (time.perf_counter() - t0) / 5 * 1e3))
