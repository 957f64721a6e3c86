"""What split-Bregman TV denoising ('tvb') costs on the device: the stage alone on frames that are already on the device, one frame
alone (the latency chain of its diagonals), and set_frame(raw_imgs, denoise=('tvb', kw)) against the same call without denoising.

  python tools/time_tvb.py [--frames 256] [--size 500] [--reps 2] [--out FILE]
      One process.  Frames: tools/time_raw_frames.py's u8 frames (a step edge plus Gaussian noise of 0.2; 0..255).  Two settings:
      weight=5 with the default eps (1e-3), and weight=5, eps=0, max_iter=100 (100 sweeps).  Every variant is run once untimed,
      then the variants are ALTERNATED, --reps rounds, every timing ended by a synchronise of the context's stream.  Prints ms per
      call (min - max) and per frame:
        K_<s>    Context.tvb_images, u8 frames on the device, results into device memory, sweep counts read back
        ONE_<s>  the same for one frame alone: (M + N - 1) steps per sweep, one after the other
        D_<s>    set_frame(raw_imgs=u8 host frames, denoise=('tvb', kw)) on a batch of --frames edges
        P        set_frame(raw_imgs=u8 host frames), no denoising: what the stage adds to
      and the sweeps the frames ran, the frames of a chunk (the workspace of a frame is six skewed f64 arrays) and the time of one
      diagonal step that follows from ONE_<s>.
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

SETTINGS = {"eps1e-3": dict(weight=5), "100sweeps": dict(weight=5, eps=0, max_iter=100)}


def main(args):
    import gaussian_process_edge_trace_amd as pkg
    L = pkg._lib
    n, size = args.frames, args.size
    ctx = L.Context(0)
    frames = make_frames(n, size, 1)["u8"]
    k = pkg.gpet_utils.kernel_builder((11, 5))
    init = np.array([[0, size // 2], [size - 1, size // 2]])
    bt = pkg.GP_Edge_Tracing_Batch([init] * n, None, list(range(1, n + 1)), raw_imgs=list(frames), grad_kernel=k, _ctx=ctx, **KW)
    dev = DeviceFrames(ctx, frames)
    buf = L.PreFrames(ctx)
    out_ptrs = buf.reserve(n, size * size * 8)
    sweeps = {}

    def stage(name, raw, ptrs):
        sweeps[name] = ctx.tvb_images(raw, out_device_ptrs=ptrs, return_n_iter=True)[1]

    variants = {"P": lambda: bt.set_frame(raw_imgs=list(frames), next_frame=False)}
    for s, kw in SETTINGS.items():
        raw = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=frames.dtype, shape=(size, size), denoise=("tvb", kw))
        one = L.RawFrames(None, device_ptrs=dev.ptrs[:1], dtype=frames.dtype, shape=(size, size), denoise=("tvb", kw))
        variants["K_" + s] = lambda s=s, raw=raw: stage("K_" + s, raw, out_ptrs)
        variants["ONE_" + s] = lambda s=s, one=one: stage("ONE_" + s, one, out_ptrs[:1])
        variants["D_" + s] = lambda kw=kw: bt.set_frame(raw_imgs=list(frames), next_frame=False, denoise=("tvb", kw))
    ms = {name: [] for name in variants}
    for rnd in range(args.reps + 1):  # round 0 warms every variant up: every timed call follows an untimed one
        for name, call in variants.items():
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if rnd:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    frame_bytes = L.tvb_frame_bytes(size, size)
    lines = ["split-Bregman TV denoising (weight 5) of %d distinct %d x %d u8 frames; %d alternated rounds after one warm-up round; ms per "
             "call, min - max (ms per frame from the min)" % (n, size, size, args.reps),
             "a frame's workspace: %d bytes; frames to a chunk on device frames: %d (one workgroup each, the chunks one after the other)"
             % (frame_bytes, min(n, L.TVB_CHUNK_BUDGET // frame_bytes))]
    for name, v in ms.items():
        per = n if name[0] in "KDP" else 1
        lines.append("%-14s %10.2f - %10.2f   (%9.4f per frame)" % (name, min(v), max(v), min(v) / per))
    for s in SETTINGS:
        it = sweeps["K_" + s]
        lines.append("%s: sweeps per frame %d - %d (mean %.1f); one frame alone ran %d sweeps in %.2f ms = %.3f ms per sweep = %.3f us per "
                     "diagonal step (%d steps per sweep)" % (s, it.min(), it.max(), it.mean(), sweeps["ONE_" + s][0], min(ms["ONE_" + s]),
                                                             min(ms["ONE_" + s]) / sweeps["ONE_" + s][0],
                                                             1e3 * min(ms["ONE_" + s]) / sweeps["ONE_" + s][0] / (2 * size - 1), 2 * size - 1))
        lines.append("set_frame with 'tvb' (%s) adds %.2f ms to the %.2f ms of set_frame without denoising, %.4f ms per frame"
                     % (s, min(ms["D_" + s]) - min(ms["P"]), min(ms["P"]), (min(ms["D_" + s]) - min(ms["P"])) / n))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    dev.free()
    buf.close()
    bt._batch.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
