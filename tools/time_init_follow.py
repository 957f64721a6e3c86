"""What endpoint tracking costs in a frame change, against the host route it replaces: B edges on one shared 512 x 512 uint8 frame whose
layers sink 2 rows per frame (the (11, 5) kernel), B = 32 / 256 / 1 024.

  python tools/time_init_follow.py [--batches 32,256,1024] [--frames 6] [--size 512] [--out FILE]
      Per B, one batch traces frame 0 (not timed); then per frame, wall clock in ms around calls that end with a wait:
        set_frame keep     set_frame(raw_imgs=next, warm_every=k, init='keep'): upload + gradient image, gradient KDE, warm start
        set_frame follow   the same with init='follow' (window 8, cols 4): k_init_follow between the swap and the warm start, and the
                           moved points read back
        host route         what a caller had to do before: comp_grad_imgs of the frame home, the numpy rule of
                           tests/init_follow_ref.py on it for every init point (vectorised here: one cumulative sum per point), and
                           a REBUILT batch with obs=warm_start_obs(previous trace) -- the previous traces are on the host already
      medians with min - max over the frames.  The trace that follows is not part of any of the three.
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
FOLLOW = dict(window=8, cols=4)


def sinking(M, N, E, T, seed0):
    """T uint8 frames with E dark-to-bright layers, evenly spaced, that sink 2 rows per frame, end points included; the E inits."""
    x = np.linspace(-np.pi, np.pi, N)
    gap = M // (E + 2)
    frames = []
    for t in range(T):
        img = np.zeros((M, N))
        rows = np.arange(M)[:, None]
        for k in range(E):
            edge = np.rint(gap * (k + 1) + 2 * t + 4.0 * np.sin(x)).astype(int)
            img[rows >= edge[None, :]] = (k + 1) / E
        img = np.clip(img + np.random.default_rng(seed0 + t).normal(0.0, 0.03, img.shape), 0.0, 1.0)
        frames.append(np.rint(img * 255.0).astype(np.uint8))
    inits = [np.array([[0, gap * (k + 1)], [N - 1, gap * (k + 1)]], dtype=np.int64) for k in range(E)]
    return frames, inits


def rule(G, init, window, cols):
    """tests/init_follow_ref.follow for one edge, the score of every candidate row from one sequential f64 cumulative sum."""
    out = np.array(init, dtype=np.int64, copy=True)
    M, N = G.shape
    for i, (x, y) in enumerate(out):
        r_lo, r_hi = max(0, y - window), min(M - 1, y + window)
        if r_lo > r_hi:
            continue
        s = np.add.accumulate(G[r_lo:r_hi + 1, max(0, x - cols):min(N - 1, x + cols) + 1].astype(np.float64), axis=1)[:, -1]
        r = np.arange(r_lo, r_hi + 1)
        ok = s > 0.0
        if ok.any():
            s, r = s[ok], r[ok]
            best = np.lexsort((r, np.abs(r - y), -s))[0]
            out[i, 1] = r[best]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,256,1024")
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gaussian_process_edge_trace_amd as pkg
    from gaussian_process_edge_trace_amd.sequence import warm_start_obs
    L = pkg._lib
    ctx = L.Context(0)
    M = N = a.size
    K = pkg.gpet_utils.kernel_builder((11, 5))
    layers = 8
    frames, layer_inits = sinking(M, N, layers, a.frames, 7)
    med = lambda v: "%9.3f (%.3f - %.3f)" % (np.median(v), min(v), max(v))
    lines = ["%d frames of %d x %d uint8 shared by all edges, %d layers, kernel (11, 5), warm_every = %d, init_follow = %s; ms, median "
             "(min - max) over frames 1 .. %d" % (a.frames, M, N, layers, WARM, FOLLOW, a.frames - 1)]
    for B in [int(v) for v in a.batches.split(",")]:
        inits = [layer_inits[e % layers] for e in range(B)]
        seeds = list(range(3, 3 + B))
        try:
            times = {}
            for mode in ("keep", "follow"):
                bt = pkg.GP_Edge_Tracing_Batch(inits, None, seeds, raw_imgs=frames[0], grad_kernel=K, _ctx=ctx, **KW)
                traces = bt()
                t_mode = []
                for f in range(1, a.frames):
                    ctx.sync()
                    t0 = time.perf_counter()
                    bt.set_frame(raw_imgs=frames[f], warm_every=WARM, init=mode, init_follow=FOLLOW if mode == "follow" else None)
                    t_mode.append((time.perf_counter() - t0) * 1e3)
                    traces = bt()
                times[mode] = t_mode
                moved = max(int(np.abs(n[:, 1] - o[:, 1]).max()) for n, o in zip(bt.inits, inits))
                bt._batch.close()
            # the host route: the same frames, the batch rebuilt per frame from points found on the host
            bt = pkg.GP_Edge_Tracing_Batch(inits, None, seeds, raw_imgs=frames[0], grad_kernel=K, _ctx=ctx, **KW)
            traces = bt()
            cur, host = [np.array(i, dtype=np.int64) for i in inits], []
            for f in range(1, a.frames):
                ps = bt._ps
                ctx.sync()
                t0 = time.perf_counter()
                G = pkg.gpet_utils.comp_grad_imgs([frames[f]], K, ctx=ctx)[0]
                cur = [rule(G, c, FOLLOW["window"], FOLLOW["cols"]) for c in cur]
                obs = [warm_start_obs(tr, p["x_st"], p["x_en"], WARM, p["algo_thresh"], p["M"]) for tr, p in zip(traces, ps)]
                bt._batch.close()
                bt = pkg.GP_Edge_Tracing_Batch(cur, G, seeds, obs=obs, _ctx=ctx, **KW)
                ctx.sync()
                host.append((time.perf_counter() - t0) * 1e3)
                traces = bt()
            bt._batch.close()
            lines += ["B = %d:" % B,
                      "  set_frame keep     %s" % med(times["keep"]),
                      "  set_frame follow   %s   (points moved by up to %d rows over the sequence)" % (med(times["follow"]), moved),
                      "  host route         %s" % med(host)]
        except L.GpetError as exc:  # (a size that does not trace is reported, the others still run; a HIP error ends the run)
            if exc.code == L.ERR_HIP:
                raise
            lines.append("B = %d: FAILED -- %s: %s" % (B, type(exc).__name__, exc))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
