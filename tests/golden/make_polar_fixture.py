"""tests/golden/polar_disc.npz: a closed contour traced by the CPU oracle on a polar frame.

    python tests/golden/make_polar_fixture.py

The frame is tests/polar_ref.py's dark disc (96 x 96 uint8, one outline R(theta) = R0 + a cos 3 theta), unwrapped by the restated rule
(numpy, no device), turned into a gradient image by the oracle's comp_grad_img and traced by the oracle between the two init points
that close the contour.  Stored: the frame, the spec, the init points, the tracer's arguments, the oracle's trace and iteration count,
and its mean absolute radial error against the outline.  Data only; tests/test_gpu_polar.py gates the device trace's error on it."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import gpet_oracle as orc  # noqa: E402
from tests import polar_ref as R  # noqa: E402

SHAPE, CENTRE, OUTER = (96, 96), (47.5, 48.25), (26.0, 4.0)
POLAR = dict(n_r=40, n_theta=90, r0=0.0, dr=1.0, theta0=0.0, pad=1)  # pad: half the (5, 3) kernel's width
KW = dict(kernel_options={"kernel": "RBF", "sigma_f": 10, "length_scale": 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
SEED = 7

frame = R.disc_frame(SHAPE, CENTRE, outlines=(OUTER,), levels=(40.0, 200.0), seed=11)  # (one outline: nothing else to lock on to)
unwrapped = R.unwrap([frame], CENTRE, **POLAR)[0]
R.seam_identities(unwrapped, POLAR["n_theta"], POLAR["pad"])
kernel = orc.kernel_builder((5, 3))
grad = orc.comp_grad_img(unwrapped, kernel)
row = int(round(R.outline(0.0, *OUTER)))
init = np.array([[POLAR["pad"], row], [POLAR["pad"] + POLAR["n_theta"], row]], dtype=np.int64)
trace, _, info = orc.trace(init, grad, seed=SEED, sign_convention="harmonic", **KW)
err = R.radial_error(trace, POLAR, *OUTER)
assert trace[0, 0] == row and trace[-1, 0] == row and trace.shape == (POLAR["n_theta"] + 1, 2)
print("oracle: %d iterations, mean |radial error| = %.4f px" % (info["n_iter"], err))
np.savez_compressed(os.path.join(HERE, "polar_disc.npz"), frame=frame, centre=np.array(CENTRE), outer=np.array(OUTER), init=init,
                    polar=np.array(json.dumps(POLAR)), kw=np.array(json.dumps(KW)), seed=np.int64(SEED), kernel=kernel, trace=trace,
                    n_iter=np.int64(info["n_iter"]), radial_error=np.float64(err))
