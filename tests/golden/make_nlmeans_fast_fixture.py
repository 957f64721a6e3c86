#!/opt/conda/bin/python3.9
"""tests/golden/nlmeans_fast.npz: what the UNMODIFIED reference's gpet_utils.denoise(image, 'nl', kwargs) = scikit-image 0.18.3's
denoise_nl_means returns with fast_mode=True (the library's default) on small seeded frames.  Needs the build container's second
interpreter, like make_nlmeans_fixture.py (the reference's gpet_utils.py is loaded as a file, unmodified):

    /opt/conda/bin/python3.9 tests/golden/make_nlmeans_fast_fixture.py

Stored per case: the input's key, the keyword arguments, the expected image and the share of pairs the 5.0 cutoff skipped.
Asserted here, for every case: BOTH restatements of tests/nlmeans_fast_ref.py -- the plain loops and the anti-diagonal walk with
the per-pixel gather -- equal the library's output (array_equal).  The library's output is the authority, not the restatements.
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

warnings.simplefilter("ignore")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402
from tests import nlmeans_fast_ref as R  # noqa: E402
from tests.denoise_ref import make_frame  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_gpet_utils", os.path.join(ref_harness.REFERENCE_ROOT, "gp_edge_tracing", "gpet_utils.py"))
ref_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_utils)
import skimage  # noqa: E402

DT = dict(u8=np.uint8, u16=np.uint16, f32=np.float32, f64=np.float64)
arrays, cases = {}, []


def cut_share(src, kw):
    """The share of (pixel, shift) pairs of the padded frame whose distance exceeds the cutoff."""
    k = dict(R.DEFAULTS, **kw)
    M, N = src.shape
    s, off, d, pad, nr, nc = R.geometry(M, N, k["patch_size"], k["patch_distance"])
    P = R.pad_reflect(src, pad)
    table = R.shifts(d)
    I = R.integrals(P, table, 2.0 * k["sigma"] * k["sigma"])
    cut = total = 0
    for n, (t_row, t_col, _) in enumerate(table):
        r0, r1 = R.weight_range(nr, t_row, off)
        c0, c1 = R.weight_range(nc, t_col, off)
        J = I[n]
        dd = ((J[r0 + off:r1 + off, c0 + off:c1 + off] + J[r0 - off:r1 - off, c0 - off:c1 - off]) - J[r0 - off:r1 - off, c0 + off:c1 + off]) \
            - J[r0 + off:r1 + off, c0 - off:c1 - off]
        cut += int((np.maximum(dd, 0.0) / R.h2s2_of(k["h"], s) > R.CUTOFF).sum())
        total += dd.size
    return cut / total


def add(name, key, kw, promote=False):
    img = arrays["in_" + key]
    src = img.astype(np.float64) if promote else img  # (a float32 frame: the device widens it and works in float64)
    out = ref_utils.denoise(src, "nl", dict(kw, fast_mode=True))
    assert out.dtype == np.float64 and out.shape == img.shape
    assert np.array_equal(R.with_kwargs(R.nlmeans_fast_loops, src, kw), out), name
    assert np.array_equal(R.with_kwargs(R.nlmeans_fast, src, kw), out), name
    assert np.array_equal(R.with_kwargs(R.nlmeans_fast, src, kw, batch_bytes=1), out), name  # (one shift at a time)
    arrays["exp_" + name] = out
    cases.append(dict(name=name, input=key, kwargs=kw, promote=promote, cut_share=cut_share(src, kw)))


# ---- float64: frame sizes x (patch, distance) x sigma: the cases that pin the ORDER of the sums ---------------------------------
SIZES = dict(a=(9, 11), b=(20, 70), c=(33, 65))
for k, (M, N) in SIZES.items():
    arrays["in_f64_" + k] = make_frame(40 + ord(k), M, N, 0.1, np.float64)
for k, (M, N) in SIZES.items():
    for s, d in ((3, 2), (4, 2), (5, 3), (7, 11)):
        if (s, d) == (7, 11) and min(M, N) < 16:  # (the padding of 15 reflects once)
            continue
        for sigma in (0.0, 0.05):
            add("f64_%s_s%d_d%d_sig%g" % (k, s, d, sigma), "f64_" + k, dict(patch_size=s, patch_distance=d, h=0.1, sigma=sigma))
# h small: most pairs are skipped at the cutoff
add("f64_b_small_h", "f64_b", dict(patch_size=5, patch_distance=3, h=0.004))
assert cases[-1]["cut_share"] > 0.5, cases[-1]
# the defaults, by leaving every key out
add("f64_c_defaults", "f64_c", dict())

# ---- the other pixel types: integer frames keep their range, so h is in their units ---------------------------------------------
for dt, h in (("u8", 25.0), ("u16", 6500.0), ("f32", 0.1)):
    arrays["in_%s_b" % dt] = make_frame(60 + len(dt), 20, 70, 0.1, DT[dt])
    for s, d in ((3, 2), (5, 3)):
        add("%s_b_s%d_d%d" % (dt, s, d), "%s_b" % dt, dict(patch_size=s, patch_distance=d, h=h, sigma=0.0 if s == 3 else 0.05 * h / 0.1),
            promote=dt == "f32")

arrays["cases"] = np.array(json.dumps(cases))
arrays["versions"] = np.array("skimage %s numpy %s" % (skimage.__version__, np.__version__))
path = os.path.join(HERE, "nlmeans_fast.npz")
np.savez_compressed(path, **arrays)
print("nlmeans_fast.npz: %d cases, %d bytes, %s, cut shares %s" % (
    len(cases), os.path.getsize(path), arrays["versions"], {c["name"]: round(c["cut_share"], 3) for c in cases if c["cut_share"] > 0.05}))
assert os.path.getsize(path) < 1000000
