"""What new frames cost a batch: set_frame from raw frames against today's two steps (comp_grad_img per frame, then set_frame with
the float32 gradient images).  The shape is the bench's fresh_images_pipelined: a batch of 256 edges with one 500 x 500 image each,
256 distinct frames per call, the README's RBF parameters.

  python tools/time_raw_frames.py [--frames 256] [--size 500] [--reps 3] [--out FILE]
      One process.  Every variant is warmed up once, then the variants are ALTERNATED, --reps rounds, every timing ended by a
      synchronise of the context's stream.  Prints ms per call (mean, min, max) and the bytes moved host -> device per call
      (from the shapes).
        A_<t>   256 x comp_grad_img(frame of pixel type t) + set_frame(list of f32 gradient images)      today's caller
        A'      set_frame alone on precomputed gradient images
        B_<t>   set_frame(raw_imgs=host frames of pixel type t)
        C_<t>   set_frame(raw_device_ptrs=frames already on the device)

  python tools/time_raw_frames.py --count FILE
      For a separate `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_raw_frames.py --count FILE`
      run: one call of B (u8, f64) and C (u8) for 1, 32 and 256 frames, each between two marker launches (gpet_normalise_f32 of 7
      values: k_minmax_f32, which the raw-frame path never launches); FILE gets the order of the phases.
  python tools/time_raw_frames.py --parse DIR --count FILE
      Kernel dispatches per call from the kernel trace of that run: the launches between each pair of markers.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 75, 'length_scale': 20}, noise_y=1, N_samples=1000, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
TYPES = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}


def make_frames(n, size, seed):
    """n distinct frames per pixel type: a step edge along the middle row plus noise (values in [0, 1], or 0..255 for u8)."""
    rng = np.random.default_rng(seed)
    base = np.zeros((size, size))
    base[size // 2:] = 0.3
    f64 = np.clip(base[None] + rng.normal(0.0, 0.2, size=(n, size, size)), 0.0, 1.0)
    return {"f64": f64, "f32": f64.astype(np.float32), "u8": np.rint(f64 * 255.0).astype(np.uint8)}


class DeviceFrames(object):
    """Frames copied to the device once through the library's own allocator (what a decoder or a broadcast would leave there)."""

    def __init__(self, ctx, stack):
        import ctypes as C
        self.ctx, self.ptrs = ctx, []
        for f in stack:
            d = C.c_void_p()
            ctx.check(ctx.lib.gpet_dev_alloc(ctx.h, f.nbytes, C.byref(d)))
            ctx.check(ctx.lib.gpet_dev_copy(ctx.h, d, f.ctypes.data, f.nbytes, 0))
            self.ptrs.append(d.value)

    def free(self):
        import ctypes as C
        for p in self.ptrs:
            self.ctx.lib.gpet_dev_free(self.ctx.h, C.c_void_p(p))
        self.ptrs = []


def build(n, size, frames, ctx):
    import gaussian_process_edge_trace_amd as pkg
    k = pkg.gpet_utils.kernel_builder((11, 5))
    init = np.array([[0, size // 2], [size - 1, size // 2]])
    bt = pkg.GP_Edge_Tracing_Batch([init] * n, None, list(range(1, n + 1)), raw_imgs=list(frames["u8"][:n]), grad_kernel=k, _ctx=ctx, **KW)
    return pkg, k, bt


def timing(args):
    import gaussian_process_edge_trace_amd as pkg
    n, size = args.frames, args.size
    ctx = pkg._lib.Context(0)
    frames = make_frames(n, size, 1)
    pkg, k, bt = build(n, size, frames, ctx)
    grads = [pkg.gpet_utils.comp_grad_img(f, k, ctx=ctx) for f in frames["f64"]]
    dev = {t: DeviceFrames(ctx, frames[t]) for t in TYPES}
    px = size * size
    variants = {}
    for t in TYPES:
        variants["A_" + t] = (lambda t=t: bt.set_frame([pkg.gpet_utils.comp_grad_img(f, k, ctx=ctx) for f in frames[t]], next_frame=False),
                              n * px * (8 + 4))  # every frame goes up as f64, every gradient image as f32
    variants["A'"] = (lambda: bt.set_frame(grads, next_frame=False), n * px * 4)
    for t in TYPES:
        variants["B_" + t] = (lambda t=t: bt.set_frame(raw_imgs=list(frames[t]), next_frame=False), n * px * np.dtype(TYPES[t]).itemsize)
    for t in TYPES:
        variants["C_" + t] = (lambda t=t: bt.set_frame(raw_device_ptrs=dev[t].ptrs, raw_dtype=TYPES[t], next_frame=False), 0)
    ms = {name: [] for name in variants}
    for rnd in range(args.reps + 1):  # round 0 warms every variant up
        for name, (call, _) in variants.items():
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if rnd:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    lines = ["set_frame of %d distinct %d x %d frames on a %d-edge batch; %d alternated rounds after one warm-up round" % (n, size, size, n, args.reps),
             "%-8s %10s %10s %10s %14s" % ("variant", "mean ms", "min ms", "max ms", "H2D MB / call")]
    for name, (_, h2d) in variants.items():
        v = ms[name]
        lines.append("%-8s %10.2f %10.2f %10.2f %14.1f" % (name, float(np.mean(v)), min(v), max(v), h2d / 1e6))
    spread = {t: max(ms["A_" + t]) - min(ms["A_" + t]) for t in TYPES}
    for t in TYPES:
        lines.append("B_%s beats A_%s by %.2f ms (slowest B against fastest A); spread of A_%s's repeats %.2f ms"
                     % (t, t, min(ms["A_" + t]) - max(ms["B_" + t]), t, spread[t]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for d in dev.values():
        d.free()
    bt._batch.close()


def counting(args):
    import gaussian_process_edge_trace_amd as pkg
    ctx = pkg._lib.Context(0)
    frames = make_frames(256, args.size, 1)
    marker = np.arange(7, dtype=np.float32)
    phases = []
    for n in (1, 32, 256):
        sub = {t: frames[t][:n] for t in frames}
        pkg, k, bt = build(n, args.size, sub, ctx)
        dev = DeviceFrames(ctx, sub["u8"])
        calls = {"B_u8": lambda: bt.set_frame(raw_imgs=list(sub["u8"]), next_frame=False),
                 "B_f64": lambda: bt.set_frame(raw_imgs=list(sub["f64"]), next_frame=False),
                 "C_u8": lambda: bt.set_frame(raw_device_ptrs=dev.ptrs, raw_dtype=np.uint8, next_frame=False)}
        for name, call in calls.items():
            call()  # (warm: staging allocated)
            ctx.normalise_f32(marker)
            call()
            ctx.normalise_f32(marker)
            phases.append("%s, %d frames" % (name, n))
        dev.free()
        bt._batch.close()
    with open(args.count, "w") as f:
        json.dump(phases, f)
    print("phases:", phases)


def parsing(args):
    phases = json.load(open(args.count))
    files = glob.glob(os.path.join(args.parse, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    marks = [i for i, nm in enumerate(names) if "k_minmax_f32" in nm]
    assert len(marks) == 2 * len(phases), (len(marks), len(phases))
    print("kernel dispatches per set_frame call (between two marker launches; the marker's own k_normalise_f32 excluded)")
    for p, ph in enumerate(phases):
        between = names[marks[2 * p] + 2:marks[2 * p + 1]]  # (+2: the first marker's k_minmax_f32 and k_normalise_f32)
        conv = sum("k_conv_relu_batch" in nm for nm in between)
        norm = sum("k_normalise_f32_batch" in nm for nm in between)
        print("%-20s %3d dispatches: %d convolution, %d normalisation, %d gradient KDE and others" % (ph, len(between), conv, norm, len(between) - conv - norm))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--count", default=None)
    ap.add_argument("--parse", default=None)
    a = ap.parse_args()
    if a.parse:
        parsing(a)
    elif a.count:
        counting(a)
    else:
        timing(a)
