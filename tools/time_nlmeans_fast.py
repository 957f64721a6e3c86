"""What fast-mode non-local means ('nl_fast' = scikit-image's default denoise_nl_means) costs on the device, next to the classic
stage ('nl', fast_mode=False) in the same run.

  python tools/time_nlmeans_fast.py [--frames 256] [--size 500] [--reps 5] [--out FILE]
      One process.  Frames: tools/time_raw_frames.py's (a step edge plus Gaussian noise of 0.2, values in [0, 1]; u8: 0..255), u8
      and f64, at skimage's defaults (patch 7, distance 11, h = 0.1 -- 25.5 grey levels for u8 --, sigma 0), ONE frame and --frames
      frames.  Every variant is run once untimed, then the variants are ALTERNATED, --reps rounds, every timing ended by a
      synchronise of the context's stream.  Prints the MEDIAN ms per call (min - max) and per frame:
        F<n>_<t>   Context.nlmeans_fast_images, n frames of pixel type t on the device, results into device memory
        C<n>_<t>   Context.nlmeans_images (the classic stage), the same frames
        HF<n>_<t>  gpet_utils.denoise_imgs(host frames, 'nl_fast', {}): host frames in, float64 frames out
      and the plan of the frames (groups of shifts, strips, workspace bytes, frames per chunk).

  python tools/time_nlmeans_fast.py --library [--size 500]
      Under an interpreter that has scikit-image: the library's denoise_nl_means(fast_mode=True) on one such float64 frame on the
      host, median of three.  The figure belongs in the profile with the name of the machine it was measured on.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def library(size):
    from skimage.restoration import denoise_nl_means
    import skimage
    from tools.time_raw_frames import make_frames
    img = np.ascontiguousarray(make_frames(1, size, 1)["f64"][0])
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        denoise_nl_means(img, patch_size=7, patch_distance=11, h=0.1, fast_mode=True, sigma=0.0)
        ts.append(time.perf_counter() - t0)
    print("scikit-image %s denoise_nl_means(fast_mode=True, patch 7, distance 11) of one %d x %d float64 frame on the host, one thread: "
          "median %.3f s (%.3f - %.3f)" % (skimage.__version__, size, size, statistics.median(ts), min(ts), max(ts)))


def main(args):
    from tools.time_raw_frames import DeviceFrames, make_frames
    import gaussian_process_edge_trace_amd as pkg
    L = pkg._lib
    n, size = args.frames, args.size
    ctx = L.Context(0)
    frames = make_frames(n, size, 1)
    h = {"u8": 0.1 * 255, "f64": 0.1}
    dev = {t: DeviceFrames(ctx, frames[t]) for t in ("u8", "f64")}
    buf = L.PreFrames(ctx)
    out_ptrs = buf.reserve(n, size * size * 8)
    variants = {}
    for t in ("u8", "f64"):
        for cnt in (1, n):
            fast = L.RawFrames(None, device_ptrs=dev[t].ptrs[:cnt], dtype=frames[t].dtype, shape=(size, size), denoise=("nl_fast", dict(h=h[t])))
            slow = L.RawFrames(None, device_ptrs=dev[t].ptrs[:cnt], dtype=frames[t].dtype, shape=(size, size),
                               denoise=("nl", dict(h=h[t], fast_mode=False)))
            variants["F%d_%s" % (cnt, t)] = (cnt, lambda raw=fast, cnt=cnt: ctx.nlmeans_fast_images(raw, out_device_ptrs=out_ptrs[:cnt]))
            variants["C%d_%s" % (cnt, t)] = (cnt, lambda raw=slow, cnt=cnt: ctx.nlmeans_images(raw, out_device_ptrs=out_ptrs[:cnt]))
            variants["HF%d_%s" % (cnt, t)] = (cnt, lambda t=t, cnt=cnt: pkg.gpet_utils.denoise_imgs(frames[t][:cnt], "nl_fast", dict(h=h[t]), ctx=ctx))
    ms = {name: [] for name in variants}
    for rnd in range(args.reps + 1):  # round 0 warms every variant up: every timed call follows an untimed one
        for name, (_, call) in variants.items():
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if rnd:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    plan = L.nlmeans_fast_plan(size, size, 7, 11)
    lines = ["fast-mode non-local means ('nl_fast') and the classic stage ('nl', fast_mode=False) at patch 7, distance 11, h 0.1 on distinct "
             "%d x %d frames; %d alternated rounds after one warm-up round; ms per call: median (min - max), ms per frame from the median"
             % (size, size, args.reps),
             "plan: %d shifts in %d groups of %d rows of 12, %d strips of 64 rows, %d bytes of workspace per frame, %d frame(s) per chunk"
             % (plan["n_shifts"], plan["n_groups"], plan["rows_per_group"], plan["strips"], plan["frame_bytes"], plan["frames_per_chunk"])]
    for name, v in ms.items():
        med = statistics.median(v)
        lines.append("%-12s %10.2f (%10.2f - %10.2f)   %9.3f per frame" % (name, med, min(v), max(v), med / variants[name][0]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for d in dev.values():
        d.free()
    buf.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--library", action="store_true")
    a = ap.parse_args()
    library(a.size) if a.library else main(a)
