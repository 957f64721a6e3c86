"""What label maps cost on the device, next to the host route they replace.

  python tools/time_label_maps.py [--frames 256] [--size 500] [--n_r 256] [--n_theta 720] [--reps 5] [--out FILE]
      One process.  Two batches are traced once, untimed, and then only read:
        rows    --frames u8 frames of --size x --size with two layers (two edges per frame through an image map): one map per frame,
                labels 0 / 1 / 2, Rule 1
        polar   --frames u8 frames with one closed outline, unwrapped as tools/time_polar.py unwraps (n_r x (n_theta + 1 + 2 pad)),
                one edge per frame: one map per frame on the frame's own shape, Rule 2 (space='frame')
      Every variant is run once untimed, then the variants are ALTERNATED, --reps rounds, every timing ended by a synchronise of the
      context's stream.  Prints the MEDIAN ms per call (min - max) and per frame:
        *_dev    label_maps into device memory (GPET_LABELS_OUT_ON_DEVICE): the kernels and their launches alone
        *_host   label_maps into host memory: the same plus the copy home
        *_route  the host route: results() home, the masks in numpy (rows) or polar_trace_xy and a polygon rasterised with PIL
                 (polar), and the upload of the masks to the device
      The host route's masks are compared with the device's: equal for rows; the polygon rasteriser has its own rule for pixels on
      the outline, so the polar figure is the share of pixels that differ.
"""
import argparse
import ctypes as C
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


def layered_frames(n, size, seed):
    """n u8 frames with two dark-to-bright edges one above the other, a quarter of the frame apart, and the inits (xy) of the 2 n edges."""
    x = np.arange(size)
    rows = np.arange(size)[:, None]
    frames, inits = [], []
    for t in range(n):
        a = np.rint(size * 0.3 + size * 0.04 * np.sin(2 * np.pi * x / (size - 1) + 0.1 * t)).astype(int)
        img = np.zeros((size, size))
        img[rows >= a[None, :]] = 0.4
        img[rows >= (a + size // 4)[None, :]] = 0.8
        img = np.clip(img + np.random.default_rng(seed + t).normal(0.0, 0.05, img.shape), 0.0, 1.0)
        frames.append(np.rint(img * 255.0).astype(np.uint8))
        for gap in (0, size // 4):
            inits.append(np.array([[0, a[0] + gap], [size - 1, a[-1] + gap]], dtype=np.int64))
    return frames, inits


def disc_frames(n, size, seed):
    """n u8 frames with one closed outline R(theta) = 0.3 size + 0.04 size cos 3 theta around the middle, dark inside."""
    c = (size - 1) / 2.0
    yy, xx = np.meshgrid(np.arange(size) - c, np.arange(size) - c, indexing="ij")
    rad, th = np.hypot(xx, yy), np.arctan2(yy, xx)
    inside = rad < 0.3 * size + 0.04 * size * np.cos(3 * th)
    frames = []
    for t in range(n):
        img = np.where(inside, 0.2, 0.8) + np.random.default_rng(seed + t).normal(0.0, 0.05, inside.shape)
        frames.append(np.rint(np.clip(img, 0.0, 1.0) * 255.0).astype(np.uint8))
    return frames, c


class DeviceBytes(object):
    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, int(n)
        d = C.c_void_p()
        ctx.check(ctx.lib.gpet_dev_alloc(ctx.h, self.n, C.byref(d)))
        self.ptr = d.value

    def upload(self, a):
        self.ctx.check(self.ctx.lib.gpet_dev_copy(self.ctx.h, C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 0))

    def free(self):
        self.ctx.lib.gpet_dev_free(self.ctx.h, C.c_void_p(self.ptr))


def main(args):
    from PIL import Image, ImageDraw
    import gaussian_process_edge_trace_amd as pkg
    L, U = pkg._lib, pkg.gpet_utils
    n, size = args.frames, args.size
    ctx = L.Context(0)
    # ---- rows: two edges per frame
    frames, inits = layered_frames(n, size, 1)
    K = U.kernel_builder((11, 5))
    rows_batch = pkg.GP_Edge_Tracing_Batch(inits, None, list(range(2 * n)), raw_imgs=frames, grad_kernel=K,
                                           image_of=[f for f in range(n) for _ in range(2)], _ctx=ctx, **KW)
    rows_batch()
    rows_dev = DeviceBytes(ctx, n * size * size)
    rows_ptrs = [rows_dev.ptr + f * size * size for f in range(n)]
    r = np.arange(size)[:, None]

    def rows_route():
        traces = rows_batch.results()[0]
        masks = np.empty((n, size, size), dtype=np.uint8)
        for f in range(n):
            masks[f] = (r >= traces[2 * f][:, 0][None, :]).astype(np.uint8) + (r >= traces[2 * f + 1][:, 0][None, :]).astype(np.uint8)
        rows_dev.upload(masks)
        return masks

    # ---- polar: one closed outline per frame
    discs, c = disc_frames(n, size, 1001)
    pol = dict(centre=(c, c), n_r=args.n_r, n_theta=args.n_theta, pad=K.shape[1] // 2, dr=(size / 2.0) / args.n_r)
    row0 = int(round((0.34 * size) / pol["dr"]))
    polar_batch = pkg.GP_Edge_Tracing_Batch([U.closed_init(row0, pol)] * n, None, list(range(n)), raw_imgs=discs, grad_kernel=K, polar=pol,
                                            _ctx=ctx, **KW)
    polar_batch()
    polar_dev = DeviceBytes(ctx, n * size * size)
    polar_ptrs = [polar_dev.ptr + f * size * size for f in range(n)]

    def polar_route():
        traces = polar_batch.results()[0]
        masks = np.empty((n, size, size), dtype=np.uint8)
        for f in range(n):
            xy = U.polar_trace_xy(traces[f], polar_batch.polar)[:-1]
            im = Image.new("L", (size, size), 0)
            ImageDraw.Draw(im).polygon([(float(x), float(y)) for x, y in xy], fill=1)
            masks[f] = np.asarray(im, dtype=np.uint8)
        polar_dev.upload(masks)
        return masks

    variants = {
        "rows_dev": lambda: rows_batch.label_maps(out_device_ptrs=rows_ptrs),
        "rows_host": lambda: rows_batch.label_maps(),
        "rows_route": rows_route,
        "polar_dev": lambda: polar_batch.label_maps(space="frame", out_device_ptrs=polar_ptrs),
        "polar_host": lambda: polar_batch.label_maps(space="frame"),
        "polar_route": polar_route,
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
    rows_equal = bool(np.array_equal(rows_batch.label_maps(), rows_route()))
    differ = float(np.mean(polar_batch.label_maps(space="frame") != polar_route()))
    lines = ["label maps of %d frames of %d x %d; rows: 2 edges per frame (Rule 1); polar: one contour of %d vertices per frame, unwrapped to "
             "%d x %d (Rule 2); %d alternated rounds after one warm-up round; ms per call: median (min - max), ms per frame from the median"
             % (n, size, size, args.n_theta, args.n_r, polar_batch.polar.width, args.reps),
             "rows: host route's masks equal the device's: %s; polar: pixels where PIL's polygon differs from Rule 2: %.4f %%" % (rows_equal, 100.0 * differ)]
    for name, v in ms.items():
        med = statistics.median(v)
        lines.append("%-12s %10.2f (%10.2f - %10.2f)   %9.4f per frame" % (name, med, min(v), max(v), med / n))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    rows_dev.free()
    polar_dev.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--n_r", type=int, default=256)
    ap.add_argument("--n_theta", type=int, default=720)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
