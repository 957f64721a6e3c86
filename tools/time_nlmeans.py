"""What non-local means ('nl', fast_mode=False) costs on the device: gpet_utils.denoise_imgs on a stack of frames, the kernel alone
on frames that are already on the device, and set_frame(raw_imgs, denoise=('nl', kw)) against the same call without denoising.

  python tools/time_nlmeans.py [--frames 32] [--size 500] [--reps 3] [--out FILE]
      One process.  Frames: tools/time_raw_frames.py's (a step edge plus Gaussian noise of 0.2, values in [0, 1]; u8: 0..255).  Two
      parameter sets at skimage's default patch 7 and distance 11: "defaults" (h = 0.1: on these noisy frames most candidates stop
      at the 5.0 cutoff after a patch row or two) and "no cutoff" (h = 10: every candidate adds all 49 terms -- the most work the
      defaults' geometry can ask for, and what the LDS and f64 bounds below are counted for).  Every variant is run once untimed,
      then the variants are ALTERNATED, --reps rounds, every timing ended by a synchronise of the context's stream.  Prints ms per
      call (min - max) and per frame:
        N_<p>_<t>   denoise_imgs(frames of pixel type t, 'nl', p): host frames in, float64 frames out
        K_<p>_<t>   Context.nlmeans_images, frames on the device, results into device memory: the kernel and its table upload
        D_<p>_u8    set_frame(raw_imgs=u8 host frames, denoise=('nl', p)) on a batch of --frames edges
        P_u8        set_frame(raw_imgs=u8 host frames), no denoising: what the stage adds to
      and, from the counts of the algorithm (terms = sum over pixels of clipped window size x 49), the least time the LDS (8 bytes
      read per term with the pixel's own patch in registers, 256 bytes per clock and CU) and the f64 vector units (5 operations per
      term, 64 per clock and CU: 78.6 TFLOP/s of fused multiply-adds) could take on 256 CUs at 2.4 GHz, and the share of each the
      "no cutoff" kernel reaches.
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

CUS, CLOCK = 256, 2.4e9
LDS_BYTES_PER_CLK_CU, F64_OPS_PER_CLK_CU = 256, 64
OPS_PER_TERM, LDS_BYTES_PER_TERM = 5, 8


def terms(M, N, s, d):
    """Weighted squared differences of one frame when no candidate stops early: clipped window sizes times s * s."""
    rows = np.array([min(d, r) + min(d + 1, M - r) for r in range(M)], dtype=np.int64)
    cols = np.array([min(d, c) + min(d + 1, N - c) for c in range(N)], dtype=np.int64)
    return int(rows.sum() * cols.sum()) * s * s


def main(args):
    import gaussian_process_edge_trace_amd as pkg
    L = pkg._lib
    n, size = args.frames, args.size
    ctx = L.Context(0)
    frames = make_frames(n, size, 1)
    params = {"defaults": {"u8": dict(fast_mode=False, h=0.1 * 255), "f64": dict(fast_mode=False)},
              "no cutoff": {"u8": dict(fast_mode=False, h=10.0 * 255), "f64": dict(fast_mode=False, h=10.0)}}
    k = pkg.gpet_utils.kernel_builder((11, 5))
    init = np.array([[0, size // 2], [size - 1, size // 2]])
    bt = pkg.GP_Edge_Tracing_Batch([init] * n, None, list(range(1, n + 1)), raw_imgs=list(frames["u8"]), grad_kernel=k, _ctx=ctx, **KW)
    dev = {t: DeviceFrames(ctx, frames[t]) for t in ("u8", "f64")}
    buf = L.PreFrames(ctx)
    out_ptrs = buf.reserve(n, size * size * 8)
    variants = {"P_u8": lambda: bt.set_frame(raw_imgs=list(frames["u8"]), next_frame=False)}
    for p, by_type in params.items():
        for t, kw in by_type.items():
            variants["N_%s_%s" % (p, t)] = lambda t=t, kw=kw: pkg.gpet_utils.denoise_imgs(frames[t], "nl", kw, ctx=ctx)
            raw = L.RawFrames(None, device_ptrs=dev[t].ptrs, dtype=frames[t].dtype, shape=(size, size), denoise=("nl", kw))
            variants["K_%s_%s" % (p, t)] = lambda raw=raw: ctx.nlmeans_images(raw, out_device_ptrs=out_ptrs)
        variants["D_%s_u8" % p] = lambda kw=by_type["u8"]: bt.set_frame(raw_imgs=list(frames["u8"]), next_frame=False, denoise=("nl", kw))
    ms = {name: [] for name in variants}
    for rnd in range(args.reps + 1):  # round 0 warms every variant up: every timed call follows an untimed one
        for name, call in variants.items():
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            if rnd:
                ms[name].append(1e3 * (time.perf_counter() - t0))
    lines = ["non-local means (patch 7, distance 11, fast_mode=False) of %d distinct %d x %d frames; %d alternated rounds after one warm-up "
             "round; ms per call, min - max (ms per frame from the min)" % (n, size, size, args.reps)]
    for name, v in ms.items():
        lines.append("%-22s %9.2f - %9.2f   (%8.3f per frame)" % (name, min(v), max(v), min(v) / n))
    for p in params:
        lines.append("set_frame with 'nl' (%s) adds %.2f ms to the %.2f ms of set_frame without denoising, %.3f ms per frame"
                     % (p, min(ms["D_%s_u8" % p]) - min(ms["P_u8"]), min(ms["P_u8"]), (min(ms["D_%s_u8" % p]) - min(ms["P_u8"])) / n))
    T = terms(size, size, 7, 11)
    t_lds = T * LDS_BYTES_PER_TERM / (CUS * LDS_BYTES_PER_CLK_CU * CLOCK) * 1e3
    t_f64 = T * OPS_PER_TERM / (CUS * F64_OPS_PER_CLK_CU * CLOCK) * 1e3
    lines.append("counts per frame: %.3f G terms, %.1f k per pixel; least time of the LDS reads %.3f ms, of the f64 operations %.3f ms"
                 % (T / 1e9, T / (size * size) / 1e3, t_lds, t_f64))
    for t in ("u8", "f64"):
        per = min(ms["K_no cutoff_%s" % t]) / n
        lines.append("K_no cutoff_%s: %.3f ms per frame = %.0f %% of the f64 bound, %.0f %% of the LDS bound"
                     % (t, per, 100.0 * t_f64 / per, 100.0 * t_lds / per))
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
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
