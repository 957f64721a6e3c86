#!/opt/conda/bin/python3.9
"""tests/golden/denoise_metrics.npz: the four figures the UNMODIFIED reference's denoise(..., verbose=True) prints (gpet_utils.py:151-156)
= scikit-image 0.18.3's peak_signal_noise_ratio, structural_similarity, normalized_root_mse(normalization='min-max') and
shannon_entropy, with the library's full SSIM map, on small seeded pairs.  Needs the build container's second interpreter, like its
siblings:

    /opt/conda/bin/python3.9 tests/golden/make_metrics_fixture.py

Stored per case: the pair (a = the frame as given, b = a denoised frame), the keyword arguments, the library's figures and map.
Asserted here, for every case: the restatement's (tests/metrics_ref.py) SSIM map equals the library's with array_equal; its counts equal
np.unique's; each of its four figures -- summed in the device's order -- lies within the bound of DESIGN.md section 9 of the library's.
The largest observed distance per figure, as a fraction of its bound, goes into the file (``margin``).  One case also holds what the
reference's own denoise(..., verbose=True) prints; its figures are asserted to lie farther from a rounding boundary than their bounds."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import warnings

import numpy as np

warnings.simplefilter("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_harness  # noqa: E402
from tests import metrics_ref as R  # noqa: E402
from tests.denoise_ref import make_frame  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_gpet_utils", os.path.join(ref_harness.REFERENCE_ROOT, "gp_edge_tracing", "gpet_utils.py"))
ref_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_utils)
import skimage  # noqa: E402
from scipy import ndimage  # noqa: E402
from skimage.measure import shannon_entropy  # noqa: E402
from skimage.metrics import mean_squared_error, normalized_root_mse, peak_signal_noise_ratio, structural_similarity  # noqa: E402

assert skimage.__version__ == "0.18.3", skimage.__version__
DT = dict(u8=np.uint8, u16=np.uint16, f32=np.float32, f64=np.float64)
arrays, cases = {}, []
margin = dict(psnr=0.0, ssim=0.0, nrmse=0.0, entropy=0.0)


def smooth(a, dt, levels=1024):
    """A stand-in for a denoised frame: a Gaussian-smoothed copy of a, in the dtype a denoiser would leave (values on a coarse grid)."""
    x = ndimage.gaussian_filter(a.astype(np.float64), 1.0)
    if np.dtype(dt).kind == "u":
        return np.rint(x).astype(dt)
    if a.dtype.kind == "u":  # (an integer frame denoised into floats: 'tvc' and the stages of their own work on x / max)
        x = x / np.iinfo(a.dtype).max
    return (np.rint(x * levels) / levels).astype(dt)


def library(a, b, kw):
    ssim_kw = {k: v for k, v in kw.items() if k != "data_range"}
    dr = kw.get("data_range")
    mssim, S = structural_similarity(a, b, data_range=dr, full=True, **ssim_kw)
    return np.array([peak_signal_noise_ratio(a, b, data_range=dr), mssim, normalized_root_mse(a, b, normalization="min-max"),
                     shannon_entropy(b)], dtype=np.float64), S


def add(name, a, b, **kw):
    with np.errstate(divide="ignore", invalid="ignore"):
        lib, S = library(a, b, kw)
    mine = R.figures(a, b, **kw)
    assert np.array_equal(mine["ssim_map"], S), name
    assert np.array_equal(np.sort(mine["counts"]), np.sort(np.unique(b, return_counts=True)[1])), name
    pad = (kw.get("win_size", 7) - 1) // 2
    crop = S[pad:S.shape[0] - pad, pad:S.shape[1] - pad]
    bd = R.bounds(a.size, crop.size, float(np.abs(crop).mean()), len(mine["counts"]), lib[0], lib[2], lib[3])
    for j, fig in enumerate(("psnr", "ssim", "nrmse", "entropy")):
        assert R.within(mine[fig], float(lib[j]), bd[fig]), (name, fig, mine[fig], lib[j], bd[fig])
        if np.isfinite(lib[j]) and bd[fig] > 0:
            margin[fig] = max(margin[fig], abs(mine[fig] - float(lib[j])) / bd[fig])
    arrays["a_" + name], arrays["b_" + name], arrays["lib_" + name], arrays["map_" + name] = a, b, lib, S
    cases.append(dict(name=name, kwargs=kw))
    return lib, bd


def pair(seed, M, N, da, db, noise=0.1):
    a = make_frame(seed, M, N, noise, DT[da], levels=1024 if da in ("f32", "f64") else None)
    return a, smooth(a, DT[db])


add("one_window_f64", *pair(1, 7, 7, "f64", "f64"))
add("small_u8", *pair(2, 7, 9, "u8", "u8"))
add("mid_u8", *pair(3, 37, 53, "u8", "u8"))
a16, b16 = pair(4, 37, 53, "u16", "u16")
d32 = (a16.astype(np.float32) - b16.astype(np.float32)) ** 2
d64 = (a16.astype(np.float64) - b16.astype(np.float64)) ** 2
assert np.mean(d32, dtype=np.float64) != np.mean(d64), "the u16 case must have squares that round in float32"
assert mean_squared_error(a16, b16) == np.mean(d32, dtype=np.float64)
add("mid_u16", a16, b16)
add("mid_f32", *pair(5, 37, 53, "f32", "f32"))
add("mid_f64", *pair(6, 37, 53, "f64", "f64"))
add("mid_u8_f64", *pair(7, 37, 53, "u8", "f64"))  # (the reference's 'tvc' call: a u8 frame, a float64 result in [0, 1], data_range 255)
add("mid_f32_f64", *pair(8, 37, 53, "f32", "f64"))
add("big_f64", *pair(9, 70, 130, "f64", "f64"))
add("big_u8", *pair(10, 70, 130, "u8", "u8"))
add("win3_f64", *pair(11, 37, 53, "f64", "f64"), win_size=3)
add("win11_u8", *pair(12, 37, 53, "u8", "u8"), win_size=11)
add("popcov_f64", *pair(13, 37, 53, "f64", "f64"), use_sample_covariance=False)
add("range_f32", *pair(14, 37, 53, "f32", "f32"), data_range=1.0)
add("k_f64", *pair(15, 37, 53, "f64", "f64"), K1=0.02, K2=0.05)
a, _ = pair(16, 7, 9, "f64", "f64")
lib, _ = add("identical_f64", a, a.copy())
assert lib[0] == np.inf and lib[2] == 0.0
a, b = pair(17, 37, 53, "f64", "f64")
a = a * 2.0 - 1.0  # (a frame below 0: the PSNR's range becomes 2)
b = b * 2.0 - 1.0
b[np.abs(b) < 0.3] = 0.0
b[::2][b[::2] == 0.0] = -0.0
assert np.signbit(b[b == 0.0]).any() and not np.signbit(b[b == 0.0]).all() and a.min() < 0
add("signed_zeros_f64", a, b)
a = make_frame(18, 37, 53, 0.1, np.uint8)
add("few_values_u8", a, (np.rint(ndimage.gaussian_filter(a.astype(np.float64), 2.0) / 64.0) * 64).clip(0, 255).astype(np.uint8))
a, b = pair(19, 37, 53, "f64", "f64")
b = b + np.arange(b.size, dtype=np.float64).reshape(b.shape) * 2.0 ** -30
assert np.unique(b).size == b.size
add("all_distinct_f64", a, b)

# what the reference itself prints, for one case (the median filter keeps u8: the device's result is the library's bit for bit)
a = arrays["a_mid_u8"]
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    den = ref_utils.denoise(a, "median", dict(size=3), verbose=True)
lib, bd = add("print_u8", a, den)
for v, places, key in zip(lib, (2, 2, 5, 3), ("psnr", "ssim", "nrmse", "entropy")):
    frac = abs(v * 10 ** places - np.floor(v * 10 ** places) - 0.5) / 10 ** places
    assert frac > 4 * bd[key], (key, v, frac, bd[key])
arrays["print_text"] = np.array(buf.getvalue())
arrays["print_kwargs"] = np.array(json.dumps(dict(technique="median", kwargs=dict(size=3))))

arrays["cases"] = np.array(json.dumps(cases))
arrays["margin"] = np.array(json.dumps(margin))
out = os.path.join(HERE, "denoise_metrics.npz")
np.savez_compressed(out, **arrays)
print("wrote", out, os.path.getsize(out), "bytes;", len(cases), "cases; margins", margin)
print(buf.getvalue())
