"""What the polar unwrap costs on the device, next to the host route it replaces.

  python tools/time_polar.py [--frames 256] [--size 500] [--n_r 256] [--n_theta 720] [--reps 5] [--out FILE]
      One process.  Frames: tools/time_raw_frames.py's u8 frames (a step edge plus noise), unwrapped around the frame's middle to
      n_r x (n_theta + 1 + 2 pad), pad = half the (11, 5) kernel's width.  Every variant is run once untimed, then the variants are
      ALTERNATED, --reps rounds, every timing ended by a synchronise of the context's stream.  Prints the MEDIAN ms per call
      (min - max) and per frame:
        U_host     gpet_utils.unwrap_polar_imgs: host u8 frames in, float64 polar frames out on the host
        U_dev      Context.polar_images: frames on the device, results into device memory (the kernel and its launch alone)
        S_polar    set_frame(raw_imgs=u8 frames, polar=...) of a batch with one edge per frame: upload, unwrap, gradient images, KDE
        S_flat     set_frame(raw_imgs=float64 polar frames) of the same batch built without polar: what is left once the frames are
                   unwrapped
        H_map      scipy.ndimage.map_coordinates(order=1, mode='nearest') per frame on the rule's clamped coordinates, on the host
        H_route    H_map followed by S_flat: the host route polar= replaces
      Nothing is traced: the figures are those of getting frames into a batch.
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

KW = dict(kernel_options={"kernel": "RBF", "sigma_f": 10, "length_scale": 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=20,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)


def main(args):
    from scipy.ndimage import map_coordinates
    from tools.time_raw_frames import DeviceFrames, make_frames
    import gaussian_process_edge_trace_amd as pkg
    L, U = pkg._lib, pkg.gpet_utils
    n, size = args.frames, args.size
    ctx = L.Context(0)
    frames = list(make_frames(n, size, 1)["u8"])
    K = U.kernel_builder((11, 5))
    pol = dict(centre=((size - 1) / 2.0, (size - 1) / 2.0), n_r=args.n_r, n_theta=args.n_theta, pad=K.shape[1] // 2)
    spec = L.polar_spec(pol)
    rows, cols = np.meshgrid(np.arange(spec.n_r), np.arange(spec.width), indexing="ij")
    x, y = U.polar_to_xy(rows, cols, spec, shape=(size, size))
    dev = DeviceFrames(ctx, frames)
    buf = L.PreFrames(ctx)
    out_ptrs = buf.reserve(n, spec.n_r * spec.width * 8)
    raw_dev = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=np.uint8, shape=(size, size), polar=pol)
    init = U.closed_init(spec.n_r // 2, spec)
    polar_batch = pkg.GP_Edge_Tracing_Batch([init] * n, None, list(range(n)), raw_imgs=frames, grad_kernel=K, polar=pol, _ctx=ctx, **KW)
    flat = U.unwrap_polar_imgs(frames, ctx=ctx, **pol)
    flat_batch = pkg.GP_Edge_Tracing_Batch([init] * n, None, list(range(n)), raw_imgs=list(flat), grad_kernel=K, _ctx=ctx, **KW)

    def host_map():
        return [map_coordinates(f.astype(np.float64), [y, x], order=1, mode="nearest") for f in frames]

    def host_route():
        flat_batch.set_frame(raw_imgs=host_map(), next_frame=False)

    variants = {
        "U_host": lambda: U.unwrap_polar_imgs(frames, ctx=ctx, **pol),
        "U_dev": lambda: ctx.polar_images(raw_dev, out_device_ptrs=out_ptrs),
        "S_polar": lambda: polar_batch.set_frame(raw_imgs=frames, next_frame=False),
        "S_flat": lambda: flat_batch.set_frame(raw_imgs=list(flat), next_frame=False),
        "H_map": host_map,
        "H_route": host_route,
    }
    ms = {name: [] for name in variants}
    for rnd in range(args.reps + 1):  # round 0 warms every variant up: every timed call follows an untimed one
        for name, call in variants.items():
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if rnd:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    err = float(np.abs(flat[0] - host_map()[0]).max())
    lines = ["polar unwrap of %d u8 frames of %d x %d to %d x %d (n_theta %d, pad %d); %d alternated rounds after one warm-up round; "
             "ms per call: median (min - max), ms per frame from the median" % (n, size, size, spec.n_r, spec.width, spec.n_theta, spec.pad, args.reps),
             "largest |device - map_coordinates| on frame 0: %.3g grey levels" % err]
    for name, v in ms.items():
        med = statistics.median(v)
        lines.append("%-10s %10.2f (%10.2f - %10.2f)   %9.4f per frame" % (name, med, min(v), max(v), med / n))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    dev.free()
    buf.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--n_r", type=int, default=256)
    ap.add_argument("--n_theta", type=int, default=720)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
