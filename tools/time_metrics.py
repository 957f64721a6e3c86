#!/usr/bin/env python
"""Device against host time of the denoise quality metrics (gpet_utils.denoise_metrics: PSNR, SSIM, NRMSE, entropy per frame).

  python tools/time_metrics.py [--frames 256] [--size 500] [--reps 2] [--host-frames 4] [--out FILE]
      One process.  Frames: tools/time_raw_frames.py's frames (a step edge plus Gaussian noise of 0.2), the "denoised" side a 3 x 3
      median of them (uint8 pairs) or 'tvb' of them (uint8 against float64, data_range 1 on frames / 255 -- float64 pairs).  Printed per
      setting: the device's wall time for the whole stack from host frames (the best of --reps, after one warm-up call), per frame,
      and -- where scikit-image can be imported -- the host's time per frame for the same four figures over --host-frames frames.  Frames 0
      and --frames - 1 of the stack are also scored alone and compared: a stack goes through the workspace in chunks, and a frame's
      figures must not depend on its chunk.  The output belongs in profiles/metrics_timing.txt."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.time_raw_frames import make_frames  # noqa: E402


def host_figures(a, b, data_range):
    from skimage.measure import shannon_entropy
    from skimage.metrics import normalized_root_mse, peak_signal_noise_ratio, structural_similarity
    return (peak_signal_noise_ratio(a, b, data_range=data_range), structural_similarity(a, b, data_range=data_range),
            normalized_root_mse(a, b, normalization="min-max"), shannon_entropy(b))


def main(args):
    import gaussian_process_edge_trace_amd as pkg
    U = pkg.gpet_utils
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fr = make_frames(args.frames, args.size, 11)
    u8 = fr["u8"]
    f64 = u8.astype(np.float64) / 255.0
    settings = [("u8 / u8 (median 3 x 3)", u8, U.denoise_imgs(u8, "median", dict(size=3)), None),
                ("f64 / f64 (tvb weight 5)", f64, U.denoise_imgs(f64, "tvb", dict(weight=5.0)), 1.0)]
    say("denoise_metrics, %d frames of %d x %d, host frames" % (args.frames, args.size, args.size))
    for name, a, b, dr in settings:
        U.denoise_metrics(a[:2], b[:2], data_range=dr)  # (warm-up: the workspace is allocated)
        U.denoise_metrics(a, b, data_range=dr)
        best = np.inf
        for _ in range(args.reps):
            t0 = time.perf_counter()
            m = U.denoise_metrics(a, b, data_range=dr)
            best = min(best, time.perf_counter() - t0)
        say("%-26s device %9.2f ms for the stack, %7.3f ms per frame" % (name, best * 1e3, best * 1e3 / args.frames))
        for t in (0, args.frames - 1):
            one = U.denoise_metrics(a[t:t + 1], b[t:t + 1], data_range=dr)
            same = all(np.array_equal(one[k][0], m[k][t]) for k in one)
            say("%-26s frame %d alone equals its place in the stack: %s" % ("", t, same))
        try:
            import skimage  # noqa: F401
        except ImportError:
            say("%-26s host: scikit-image is not installed here" % "")
            continue
        n = min(args.host_frames, args.frames)
        t0 = time.perf_counter()
        host = [host_figures(a[t], b[t], dr) for t in range(n)]
        dt = (time.perf_counter() - t0) / n
        say("%-26s host   %9.2f ms per frame (scikit-image %s, %d frames)" % ("", dt * 1e3, skimage.__version__, n))
        say("%-26s largest distance device - host over those frames: %s" % ("", ", ".join(
            "%s %.3g" % (k, max(abs(m[k][t] - host[t][j]) for t in range(n))) for j, k in enumerate(("psnr", "ssim", "nrmse", "entropy")))))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
