"""ms per launch sequence of the factor stage, profile_stage(1, reps): the bench edge after 7 iterations at 1, 32 and 1024 edges
(the shapes of tools/time_jacobi_ahead.py) and one any-rank Matern edge of 1 024 columns: device time plus the host's enqueue, so a
change of the launchers alone shows here.  To compare two builds, run one process per library, alternating, in one session:
  GPET_LIB_PATH=/path/to/other/libgpet_hip.so python tools/time_factor_host.py other; python tools/time_factor_host.py this"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import gaussian_process_edge_trace_amd as amd  # noqa: E402
from bench import synth_image, README_KW  # noqa: E402
from oracle import gpet_oracle as orc  # noqa: E402

tag = sys.argv[1]
L = amd._lib
ctx = L.Context(0)
img, truth = synth_image(500, 3)
init = truth[[0, -1], :][:, [1, 0]]
grad = amd.gpet_utils.comp_grad_img(img, amd.gpet_utils.kernel_builder((11, 5)), ctx=ctx)
for E in (1, 32, 1024):
    seeds = [1 + 997 * k for k in range(E)]
    tr = amd.GP_Edge_Tracing_Batch([init] * E, grad, seeds, **README_KW, _ctx=ctx)
    b = tr._batch
    b.iterate(seeds, 7)
    b.profile_stage(1, 3)
    ms = [b.profile_stage(1, 40) for _ in range(5)]
    print("%s bench edge E=%d: factor stage ms per rep %s (min %.4f)" % (tag, E, " ".join("%.4f" % m for m in ms), min(ms)), flush=True)
    b.close()
N = 1024
img, truth = orc.synth_sinusoid_image(N, 5)
grad = amd.gpet_utils.comp_grad_img(img, amd.gpet_utils.kernel_builder((11, 5)), ctx=ctx)
init = truth[[0, -1], :][:, [1, 0]]
warm = truth[16:-16:16][:, [1, 0]].astype(np.int64)
kw = dict(kernel_options={'kernel': 'Matern', 'nu': 2.5, 'sigma_f': 0.15 * N, 'length_scale': 0.04 * N}, noise_y=1, N_samples=300,
          score_thresh=1, delta_x=8, keep_ratio=0.1, pixel_thresh=5, seed=3, fix_endpoints=True)
tr = amd.GP_Edge_Tracing(init, grad, obs=warm, **kw, _ctx=ctx)
b = tr._batch
b.set_obs(0, warm)
b.fit_predict(want_cov=True)
b.profile_stage(1, 2)
ms = [b.profile_stage(1, 5) for _ in range(5)]
print("%s any-rank edge of 1024 columns: factor stage ms per rep %s (min %.4f)" % (tag, " ".join("%.4f" % m for m in ms), min(ms)), flush=True)
