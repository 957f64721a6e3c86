"""What tracking bands cost and save in a sequence: 32 frames of 1024 x 1024 uint8 with 8 layers each (8 edges of 1024 columns on one
shared frame, the (11, 5) kernel), every frame handed to the next on the device (set_frame(raw_imgs=next, warm_every=k)).

  python tools/time_bands.py [--frames 32] [--size 1024] [--edges 8] [--bands 128,256] [--out FILE]
      One process, one batch per variant: the full frame (band_rows=None, the path every sequence took before bands) and every H of
      --bands.  Per variant the first frame is traced cold (not timed), then per frame, wall clock around calls that end with a wait:
        set_frame     the hand-over: readiness, [placement,] upload + gradient image of the frame, [the slots' bands,] gradient KDE,
                      warm start, observation sets read back
        full step     set_frame plus the trace of the frame (device loop, converged fits)
      medians with min - max over the frames, and the iterations per frame.  Then the three per-edge stages whose work is O(M N) per
      edge and iteration, on the state the last trace left (gpet_profile_stage, mean of 20 repetitions between two events): the KDE of
      the best curves (151), the column scan of the pixel selection (160) -- and the gradient KDE with the image step, which runs once
      per frame: set_images alone, timed as above.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 20, 'length_scale': 40}, noise_y=1, N_samples=500, score_thresh=1, delta_x=10,
          keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
WARM = 20  # 2 * delta_x, trace_sequence's default


def layered(M, N, E, T, seed0):
    """T uint8 frames with E dark-to-bright layers, evenly spaced, whose middle drifts by 1 row per frame; the E inits."""
    x = np.arange(N)
    bump = np.sin(np.pi * x / (N - 1))
    gap = M // (E + 1)
    frames = []
    for t in range(T):
        img = np.zeros((M, N))
        rows = np.arange(M)[:, None]
        for k in range(E):
            edge = np.rint(gap * (k + 1) + t * bump + 6.0 * np.sin(6 * np.pi * x / (N - 1))).astype(int)
            img[rows >= edge[None, :]] = (k + 1) / E
        img = np.clip(img + np.random.default_rng(seed0 + t).normal(0.0, 0.03, img.shape), 0.0, 1.0)
        frames.append(np.rint(img * 255.0).astype(np.uint8))
    inits = [np.array([[0, gap * (k + 1)], [N - 1, gap * (k + 1)]], dtype=np.int64) for k in range(E)]
    return frames, inits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--edges", type=int, default=8)
    ap.add_argument("--bands", default="128,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gaussian_process_edge_trace_amd as pkg
    L = pkg._lib
    ctx = L.Context(0)
    M = N = a.size
    k = pkg.gpet_utils.kernel_builder((11, 5))
    frames, inits = layered(M, N, a.edges, a.frames, 7)
    seeds = list(range(3, 3 + a.edges))
    med = lambda v: "%9.3f (%.3f - %.3f)" % (np.median(v), min(v), max(v))
    lines = ["%d frames of %d x %d uint8, %d edges of %d columns on the shared frame, kernel (11, 5), warm_every = %d; ms, median (min - max) "
             "over frames 1 .. %d" % (a.frames, M, N, a.edges, N, WARM, a.frames - 1)]
    for H in [None] + [int(v) for v in a.bands.split(",")]:
        name = "full frame (band_rows=None)" if H is None else "band_rows = %d (M / %d)" % (H, M // H)
        try:
            bt = pkg.GP_Edge_Tracing_Batch(inits, None, seeds, raw_imgs=frames[0], grad_kernel=k, band_rows=H, _ctx=ctx, **KW)
            bt()
            hand, step, iters = [], [], []
            for f in range(1, a.frames):
                ctx.sync()
                t0 = time.perf_counter()
                bt.set_frame(raw_imgs=frames[f], warm_every=WARM)
                t1 = time.perf_counter()
                bt()
                t2 = time.perf_counter()
                hand.append((t1 - t0) * 1e3)
                step.append((t2 - t0) * 1e3)
                iters.append(int(np.max(bt.timings["iters"])))
            swap = []
            raw = L.RawFrames(k, frames=[frames[0]])
            for _ in range(7):
                ctx.sync()
                t0 = time.perf_counter()
                bt._batch.set_images(raw=raw)
                swap.append((time.perf_counter() - t0) * 1e3)
            bt.reset()
            bt()
            kde, pix = bt._batch.profile_stage(151, 20), bt._batch.profile_stage(160, 20)
            lines += ["%s:" % name,
                      "  set_frame   %s" % med(hand),
                      "  full step   %s   (iterations of the slowest edge per frame: median %d, max %d)" % (med(step), np.median(iters), max(iters)),
                      "  O(M N) stages: curve KDE (151) %.3f ms per iteration; pixel column scan (160) %.3f ms per iteration; "
                      "set_images (frame -> gradient image%s -> gradient KDE) %s per frame"
                      % (kde, pix, "" if H is None else " -> bands", med(swap[1:]))]
            if H is not None:
                lines.append("  bands at the end: r0 = %s" % [int(v) for v in bt.band_r0])
            bt._batch.close()
        except L.GpetError as exc:  # (a variant that does not trace is reported, the others still run; a HIP error ends the run)
            if exc.code == L.ERR_HIP:
                raise
            lines.append("%s: FAILED -- %s: %s" % (name, type(exc).__name__, exc))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
