#!/opt/conda/bin/python3.9
"""tests/golden/tvb.npz: what the UNMODIFIED reference's gpet_utils.denoise(image, 'tvb', kwargs) (gpet_utils.py:139-140) =
scikit-image 0.18.3's denoise_tv_bregman returns on small seeded frames.  Needs the build container's second interpreter, like
make_wavelet_fixture.py (the reference's gpet_utils.py is loaded as a file, unmodified):

    /opt/conda/bin/python3.9 tests/golden/make_tvb_fixture.py [--time]

Stored per case: the input's key, the keyword arguments, the library's output, and from the restatement (tests/tvb_ref.py) every
sweep's rmse with the squared changes added in raster order and in the device's order, and the sweep count.  Asserted here, for
every case: the raster restatement equals the library with array_equal; the diagonal-at-a-time form equals the raster form; both
orders of acc give the same sweep count; every rmse of either order is farther from eps than 2 (n - 1) 2^-53 relative; and over
the cases: one stops by eps, one by max_iter, one is anisotropic.
``--time``: also prints the library's host time per 500 x 500 frame (what profiles/tvb_timing.txt quotes)."""
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
from tests import tvb_ref as R  # noqa: E402
from tests.denoise_ref import make_frame  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_gpet_utils", os.path.join(ref_harness.REFERENCE_ROOT, "gp_edge_tracing", "gpet_utils.py"))
ref_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_utils)
import skimage  # noqa: E402

DT = dict(u8=np.uint8, u16=np.uint16, f32=np.float32, f64=np.float64)
arrays, cases = {}, []


def frame(key, seed, M, N, dt, noise=0.1):
    # (values on a grid of 1 / 1024, so that float64 inputs compress)
    arrays["in_" + key] = make_frame(seed, M, N, noise, DT[dt], levels=1024 if dt in ("f64", "f32") else None)


def add(name, key, kw, promote=False):
    img = arrays["in_" + key]
    src = img.astype(np.float64) if promote else img  # (a float32 frame: the device widens it and works in float64)
    out = ref_utils.denoise(src, "tvb", dict(kw))
    assert out.dtype == np.float64 and out.shape == img.shape, (name, out.dtype)
    args = dict(weight=kw["weight"], max_iter=kw.get("max_iter", 100), eps=kw.get("eps", 1e-3), isotropic=kw.get("isotropic", True))
    mine, info = R.denoise_tv_bregman(src, form="raster", order="raster", return_info=True, **args)
    assert np.array_equal(mine, out), name
    diag, info_d = R.denoise_tv_bregman(src, form="diagonal", order="device", return_info=True, **args)
    assert np.array_equal(diag, mine), name
    assert info_d["n_iter"] == info["n_iter"], name
    assert np.array_equal(info_d["rmse_raster"], info["rmse_raster"]) and np.array_equal(info_d["rmse_device"], info["rmse_device"]), name
    n = img.size
    assert R.margin_ok(info["rmse_raster"], args["eps"], n) and R.margin_ok(info["rmse_device"], args["eps"], n), name
    arrays["exp_" + name] = out
    arrays["rmse_raster_" + name] = info["rmse_raster"]
    arrays["rmse_device_" + name] = info["rmse_device"]
    cases.append(dict(name=name, input=key, kwargs=kw, promote=promote, n_iter=int(info["n_iter"]),
                      stopped_by="max_iter" if info["n_iter"] == args["max_iter"] and info["rmse_raster"][-1] > args["eps"] else "eps"))


# the smallest frames the library takes
frame("f64_2x2", 31, 2, 2, "f64")
add("f64_2x2", "f64_2x2", dict(weight=5))
frame("f64_2x9", 32, 2, 9, "f64")
add("f64_2x9", "f64_2x9", dict(weight=5))
frame("f64_9x2", 33, 9, 2, "f64")
add("f64_9x2", "f64_9x2", dict(weight=5))
# 9 x 13, isotropic, default eps; two more frames of the shape that stop after other sweep counts (one call, three counts)
frame("f64_9x13", 34, 9, 13, "f64")
add("f64_9x13", "f64_9x13", dict(weight=5))
frame("f64_9x13_b", 35, 9, 13, "f64", noise=0.3)
add("f64_9x13_b", "f64_9x13_b", dict(weight=5))
frame("f64_9x13_c", 36, 9, 13, "f64", noise=0.02)
add("f64_9x13_c", "f64_9x13_c", dict(weight=5))
assert len({c["n_iter"] for c in cases[-3:]}) == 3, [c["n_iter"] for c in cases[-3:]]
frame("f64_12x7", 37, 12, 7, "f64")
add("f64_12x7_aniso", "f64_12x7", dict(weight=5, isotropic=False))
frame("f64_17x17", 38, 17, 17, "f64")
add("f64_17x17_7sweeps", "f64_17x17", dict(weight=5, max_iter=7, eps=0))
# a diagonal longer than one 64-lane wave, taller and wider
frame("f64_65x70", 39, 65, 70, "f64")
add("f64_65x70", "f64_65x70", dict(weight=5, max_iter=12))
frame("f64_70x65", 40, 70, 65, "f64")
add("f64_70x65_aniso", "f64_70x65", dict(weight=5, max_iter=12, isotropic=False))
frame("u8_33x65", 13, 33, 65, "u8")
add("u8_33x65", "u8_33x65", dict(weight=5, max_iter=20))
frame("u16_21x19", 15, 21, 19, "u16")
add("u16_21x19", "u16_21x19", dict(weight=5))
# a float32 frame against the widened input
frame("f32_26x30", 19, 26, 30, "f32")
add("f32_26x30", "f32_26x30", dict(weight=5), promote=True)
add("f64_9x13_w05", "f64_9x13", dict(weight=0.5))
add("f64_9x13_w10", "f64_9x13", dict(weight=10, max_iter=30))

assert any(c["stopped_by"] == "eps" for c in cases) and any(c["stopped_by"] == "max_iter" for c in cases)
assert any(c["kwargs"].get("isotropic") is False for c in cases)

arrays["cases"] = np.array(json.dumps(cases))
arrays["versions"] = np.array("skimage %s numpy %s" % (skimage.__version__, np.__version__))
path = os.path.join(HERE, "tvb.npz")
np.savez_compressed(path, **arrays)
print("tvb.npz: %d cases, %d bytes, %s, sweeps %s" % (len(cases), os.path.getsize(path), arrays["versions"],
                                                      [(c["name"], c["n_iter"], c["stopped_by"]) for c in cases]))
assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "denoise.npz"))

if "--time" in sys.argv:
    from tools.time_raw_frames import make_frames  # (frame 0 of the frames tools/time_tvb.py times on the device)
    img = make_frames(1, 500, 1)["u8"][0]
    for kw in (dict(weight=5), dict(weight=5, eps=0, max_iter=100)):
        ref_utils.denoise(img, "tvb", dict(kw))
        t0 = time.perf_counter()
        for _ in range(3):
            ref_utils.denoise(img, "tvb", dict(kw))
        ms = (time.perf_counter() - t0) / 3 * 1e3
        # (the sweeps the library ran: all of them at eps = 0, else what the restatement counts)
        n_sweeps = kw["max_iter"] if kw.get("eps") == 0 else R.denoise_tv_bregman(img, form="diagonal", return_info=True, **kw)[1]["n_iter"]
        print("host, scikit-image %s: 500 x 500 uint8, %r: %.1f ms per frame (%d sweeps)" % (skimage.__version__, kw, ms, n_sweeps))
