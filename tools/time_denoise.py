"""What denoising costs in front of new frames: set_frame(raw_imgs, denoise=d) against set_frame(raw_imgs) (what the stage adds
to) and against what a caller did before it existed -- the host's scipy / scikit-image function per frame, then
set_frame(raw_imgs=denoised).  The shape is tools/time_raw_frames.py's: a batch of 256 edges with one 500 x 500 image each, 256
distinct frames per call, the README's RBF parameters.

  python tools/time_denoise.py [--frames 256] [--size 500] [--reps 5] [--host-frames 8] [--out FILE]
      One process.  Every device variant is warmed up once, then the variants are ALTERNATED, --reps rounds, every timing ended by
      a synchronise of the context's stream.  Prints ms per call (min - max) per technique and pixel type:
        P_<t>     set_frame(raw_imgs=host frames of pixel type t), no denoising                                the parent's call
        D_<t>     set_frame(raw_imgs=host frames, denoise=d)
        C_<t>     set_frame(raw_device_ptrs=frames already on the device, denoise=d)
        H_<t>     host: the per-frame function (scipy.ndimage for the filters; scikit-image's denoise_tv_chambolle for 'tvc' where
                  it can be imported, else its NumPy restatement tests/denoise_ref.py, the same array operations) timed on
                  --host-frames frames and scaled to --frames, plus the measured set_frame(raw_imgs=denoised frames)

  python tools/time_denoise.py --count FILE
      For a separate `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_denoise.py --count FILE` run:
      one gpet_denoise_images call per technique for 1, 32 and 128 u8 frames on the device, each between two marker launches
      (gpet_normalise_f32 of 7 values: k_minmax_f32, which the denoising path never launches); FILE gets the order of the phases.
  python tools/time_denoise.py --parse DIR --count FILE
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
from tools.time_raw_frames import KW, TYPES, DeviceFrames, make_frames  # noqa: E402

SPECS = {"median3": ("median", dict(size=3)), "median5": ("median", dict(size=5)), "gauss1.5": ("gaussian", dict(sigma=1.5)),
         "tvc0.1": ("tvc", dict(weight=0.1))}


def host_function(technique):
    """The reference's per-frame host function of a technique, and what it is."""
    from scipy import ndimage
    if technique == "median":
        return (lambda f, **kw: ndimage.median_filter(f, **kw)), "scipy.ndimage.median_filter"
    if technique == "gaussian":
        return (lambda f, **kw: ndimage.gaussian_filter(f, **kw)), "scipy.ndimage.gaussian_filter"
    try:
        from skimage.restoration import denoise_tv_chambolle
        return (lambda f, **kw: denoise_tv_chambolle(f, **kw)), "skimage.restoration.denoise_tv_chambolle"
    except ImportError:
        from tests import denoise_ref
        return (lambda f, **kw: denoise_ref.tvc(f, **kw)), "tests/denoise_ref.tvc (NumPy restatement of denoise_tv_chambolle)"


def timing(args):
    import gaussian_process_edge_trace_amd as pkg
    n, size = args.frames, args.size
    ctx = pkg._lib.Context(0)
    frames = make_frames(n, size, 1)
    k = pkg.gpet_utils.kernel_builder((11, 5))
    init = np.array([[0, size // 2], [size - 1, size // 2]])
    bt = pkg.GP_Edge_Tracing_Batch([init] * n, None, list(range(1, n + 1)), raw_imgs=list(frames["u8"][:n]), grad_kernel=k, _ctx=ctx, **KW)
    dev = {t: DeviceFrames(ctx, frames[t]) for t in TYPES}
    variants, host, denoised = {}, {}, {}
    for t in TYPES:
        variants["P_" + t] = lambda t=t: bt.set_frame(raw_imgs=list(frames[t]), next_frame=False)
    for s, spec in SPECS.items():
        fn, what = host_function(spec[0])
        for t in TYPES:
            variants["D_%s_%s" % (s, t)] = lambda t=t, spec=spec: bt.set_frame(raw_imgs=list(frames[t]), next_frame=False, denoise=spec)
            variants["C_%s_%s" % (s, t)] = lambda t=t, spec=spec: bt.set_frame(raw_device_ptrs=dev[t].ptrs, raw_dtype=TYPES[t],
                                                                             next_frame=False, denoise=spec)
            t0 = time.perf_counter()
            for f in frames[t][:args.host_frames]:
                fn(f, **spec[1])
            host[(s, t)] = (1e3 * (time.perf_counter() - t0) / args.host_frames, what)
            den = pkg.gpet_utils.denoise_imgs(frames[t], spec[0], spec[1], ctx=ctx)
            denoised[(s, t)] = den.dtype
            variants["S_%s_%s" % (s, t)] = lambda den=den: bt.set_frame(raw_imgs=list(den), next_frame=False)
    ms = {name: [] for name in variants}
    for rnd in range(args.reps + 1):  # round 0 warms every variant up
        for name, call in variants.items():
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if rnd:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    rng = lambda v: "%8.2f - %8.2f" % (min(v), max(v))
    lines = ["set_frame of %d distinct %d x %d frames on a %d-edge batch; %d alternated rounds after one warm-up round; ms per call, min - max"
             % (n, size, size, n, args.reps)]
    for t in TYPES:
        lines.append("%-22s %s" % ("P_" + t + " (no denoising)", rng(ms["P_" + t])))
    for s, spec in SPECS.items():
        lines.append("%s = %r; host function: %s, %d frames timed once, scaled to %d" % (s, spec, host[(s, "u8")][1], args.host_frames, n))
        for t in TYPES:
            d, c, sf = ms["D_%s_%s" % (s, t)], ms["C_%s_%s" % (s, t)], ms["S_%s_%s" % (s, t)]
            h = host[(s, t)][0] * n
            lines.append("  %-4s D (host frames) %s   C (device frames) %s   H (host function %9.1f + set_frame of %s frames %s) = %9.1f"
                         "   stage adds %7.2f over P   D ahead of H by %9.1f (spread of D %.2f)"
                         % (t, rng(d), rng(c), h, denoised[(s, t)], rng(sf), h + min(sf), min(d) - min(ms["P_" + t]), h + min(sf) - max(d),
                            max(d) - min(d)))
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
    L = pkg._lib
    ctx = L.Context(0)
    frames = make_frames(128, args.size, 1)["u8"]
    marker = np.arange(7, dtype=np.float32)
    phases = []
    for n in (1, 32, 128):
        dev = DeviceFrames(ctx, frames[:n])
        for s, spec in SPECS.items():
            raw = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=np.uint8, shape=frames.shape[1:], denoise=spec)
            ctx.denoise_images(raw)  # (warm: workspace allocated)
            ctx.normalise_f32(marker)
            _, n_iter = ctx.denoise_images(raw)
            ctx.normalise_f32(marker)
            phases.append("%s, %d frames%s" % (s, n, ", iterations %d..%d" % (n_iter.min(), n_iter.max()) if spec[0] == "tvc" else ""))
        dev.free()
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
    print("kernel dispatches per gpet_denoise_images call (between two marker launches; the marker's own k_normalise_f32 excluded)")
    for p, ph in enumerate(phases):
        between = names[marks[2 * p] + 2:marks[2 * p + 1]]  # (+2: the first marker's k_minmax_f32 and k_normalise_f32)
        kinds = {}
        for nm in between:
            key = nm.split("<")[0].split("(")[0].replace("void ", "").replace("gpet::", "")
            kinds[key] = kinds.get(key, 0) + 1
        print("%-40s %4d dispatches: %s" % (ph, len(between), ", ".join("%d %s" % (v, k) for k, v in sorted(kinds.items()))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=8)
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
