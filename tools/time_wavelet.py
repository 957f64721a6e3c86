"""What wavelet denoising ('wavelet') costs on the device: gpet_utils.denoise_imgs on a stack of frames, the stage alone on frames
that are already on the device, and set_frame(raw_imgs, denoise=('wavelet', kw)) against the same call without denoising.

  python tools/time_wavelet.py [--frames 256] [--size 500] [--reps 3] [--out FILE]
      One process.  Frames: tools/time_raw_frames.py's (a step edge plus Gaussian noise of 0.2, values in [0, 1]; u8: 0..255).
      Wavelets db1 (2 taps) and db4 (8 taps) at default levels, soft BayesShrink, sigma estimated per frame.  Every variant is run
      once untimed, then the variants are ALTERNATED, --reps rounds, every timing ended by a synchronise of the context's stream.
      Prints ms per call (min - max) and per frame:
        W_<w>_<t>   denoise_imgs(frames of pixel type t, 'wavelet', dict(wavelet=w)): host frames in, float64 frames out
        K_<w>_<t>   Context.wavelet_images, frames on the device, results into device memory: the 2 levels + 2 launches per chunk,
                    the table upload and the read-back of the noise levels
        D_<w>_u8    set_frame(raw_imgs=u8 host frames, denoise=('wavelet', dict(wavelet=w))) on a batch of --frames edges
        P_u8        set_frame(raw_imgs=u8 host frames), no denoising: what the stage adds to
      and, from the pyramid's sizes, the bytes a frame's passes must move through device memory at the least (every level's input
      read and its four bands written, dd1 read for the median, the detail bands read for the thresholds, every level's four bands
      read and its reconstruction written) with the time that takes at 8 TB/s.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.time_raw_frames import KW, DeviceFrames, make_frames  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
WAVELETS = ("db1", "db4")


def least_bytes(spec, shape, pix_bytes):
    """Bytes one frame's passes move at the least (module docstring)."""
    levels, _ = spec.pyramid(shape)
    m, n, total = shape[0], shape[1], 0
    for l, (mo, no, _) in enumerate(levels):
        band = 8 * mo * no
        total += (pix_bytes if l == 0 else 8) * m * n + 4 * band  # forward
        total += 3 * band                                          # thresholds
        total += 4 * band + 8 * m * n                              # inverse
        m, n = mo, no
    return total + 8 * levels[0][0] * levels[0][1]                 # the median's first pass over dd1


def main(args):
    import gaussian_process_edge_trace_amd as pkg
    L = pkg._lib
    n, size = args.frames, args.size
    ctx = L.Context(0)
    frames = make_frames(n, size, 1)
    k = pkg.gpet_utils.kernel_builder((11, 5))
    init = np.array([[0, size // 2], [size - 1, size // 2]])
    bt = pkg.GP_Edge_Tracing_Batch([init] * n, None, list(range(1, n + 1)), raw_imgs=list(frames["u8"]), grad_kernel=k, _ctx=ctx, **KW)
    dev = {t: DeviceFrames(ctx, frames[t]) for t in ("u8", "f64")}
    buf = L.PreFrames(ctx)
    out_ptrs = buf.reserve(n, size * size * 8)
    variants = {"P_u8": lambda: bt.set_frame(raw_imgs=list(frames["u8"]), next_frame=False)}
    for w in WAVELETS:
        kw = dict(wavelet=w)
        for t in ("u8", "f64"):
            variants["W_%s_%s" % (w, t)] = lambda t=t, kw=kw: pkg.gpet_utils.denoise_imgs(frames[t], "wavelet", kw, ctx=ctx)
            raw = L.RawFrames(None, device_ptrs=dev[t].ptrs, dtype=frames[t].dtype, shape=(size, size), denoise=("wavelet", kw))
            variants["K_%s_%s" % (w, t)] = lambda raw=raw: ctx.wavelet_images(raw, out_device_ptrs=out_ptrs)
        variants["D_%s_u8" % w] = lambda kw=kw: bt.set_frame(raw_imgs=list(frames["u8"]), next_frame=False, denoise=("wavelet", kw))
    ms = {name: [] for name in variants}
    for rnd in range(args.reps + 1):  # round 0 warms every variant up: every timed call follows an untimed one
        for name, call in variants.items():
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if rnd:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    lines = ["wavelet denoising (default levels, soft BayesShrink, sigma estimated) of %d distinct %d x %d frames; %d alternated rounds "
             "after one warm-up round; ms per call, min - max (ms per frame from the min)" % (n, size, size, args.reps)]
    for name, v in ms.items():
        lines.append("%-12s %9.2f - %9.2f   (%8.4f per frame)" % (name, min(v), max(v), min(v) / n))
    for w in WAVELETS:
        lines.append("set_frame with 'wavelet' (%s) adds %.2f ms to the %.2f ms of set_frame without denoising, %.4f ms per frame"
                     % (w, min(ms["D_%s_u8" % w]) - min(ms["P_u8"]), min(ms["P_u8"]), (min(ms["D_%s_u8" % w]) - min(ms["P_u8"])) / n))
    for w in WAVELETS:
        spec = L.wavelet_spec(dict(wavelet=w))
        for t, pb in (("u8", 1), ("f64", 8)):
            b = least_bytes(spec, (size, size), pb)
            per = min(ms["K_%s_%s" % (w, t)]) / n
            lines.append("K_%s_%s: %d levels, at least %.2f MB per frame = %.4f ms at 8 TB/s; measured %.4f ms per frame: the bound is %.1f %% of it"
                         % (w, t, spec.levels_on((size, size)), b / 1e6, b / HBM_BYTES_PER_S * 1e3, per, 100.0 * b / HBM_BYTES_PER_S * 1e3 / per))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for d in dev.values():
        d.free()
    buf.close()
    bt._batch.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
