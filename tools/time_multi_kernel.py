"""What the slot table saves a job with two edge polarities per frame: 32 uint8 frames of 500 x 500 with a dark lumen each, 8 edges
per frame (4 upper walls through one 11 x 5 kernel, 4 lower walls through the flipped one), the README's RBF parameters -- a batch
of 256 edges on 64 image slots.

  python tools/time_multi_kernel.py [--reps 5] [--out profiles/r11_multi_kernel.txt]
      One process on one MI355X.  Both variants are warmed up once, then ALTERNATED, --reps rounds; every timing is a host clock
      around work that ends in a synchronise of the context's stream (a trace ends with its results on the host); ms per call.
      Every timed call of a batch follows an untimed call of the same batch with the other set of frames (tools/time_image_map.py
      says why).
        table_set_frame / table_step   set_frame(raw_imgs=32 frames) of the batch built with grad_kernel=[K0, K1], kernel_of:
                                       every frame uploaded and staged once, 64 gradient images made on the device; alone, and
                                       followed by the trace (a full step)
        host_set_frame / host_step     what the commit before offers for the same job: comp_grad_imgs(frames, K) once per
                                       kernel -- the gradient images come back through host memory -- then
                                       set_frame(grad_imgs=the 64 slot images) of the batch built with the edge-to-slot image map
      The two batches must trace the same: the script checks it and says so.
"""
import argparse
import gc
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 75, 'length_scale': 20}, noise_y=1, N_samples=1000, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
C_FRAMES, E_EDGES, SIZE = 32, 8, 500
ROWS = [60 + 50 * k for k in range(E_EDGES)]  # walls: even k bright-to-dark (a lumen begins), odd k dark-to-bright (it ends)


def make_frames(n, seed):
    """n distinct uint8 frames: 4 dark lumina between the rows the inits sit on, plus noise."""
    rng = np.random.default_rng(seed)
    base = np.full((SIZE, SIZE), 0.6)
    for k in range(0, E_EDGES, 2):
        base[ROWS[k]:ROWS[k + 1]] = 0.2
    return [np.rint(np.clip(base + rng.normal(0.0, 0.05, size=base.shape), 0.0, 1.0) * 255.0).astype(np.uint8) for _ in range(n)]


def main(args):
    import gaussian_process_edge_trace_amd as pkg
    ctx = pkg._lib.Context(0)
    ka, kb = pkg.gpet_utils.kernel_builder((11, 5)), pkg.gpet_utils.kernel_builder((11, 5), b2d=True)
    sets = [make_frames(C_FRAMES, s) for s in (1, 2)]  # two sets of 32 frames, alternated
    ga = pkg.gpet_utils.comp_grad_img(sets[0][0], ka, ctx=ctx)
    K = [ka, kb] if ga[ROWS[0]].mean() > ga[ROWS[1]].mean() else [kb, ka]  # K[0] answers to the upper walls
    B = C_FRAMES * E_EDGES
    inits = [np.array([[0, r], [SIZE - 1, r]]) for _ in range(C_FRAMES) for r in ROWS]
    frame_of_edge = [c for c in range(C_FRAMES) for _ in range(E_EDGES)]
    kernel_of = [k % 2 for _ in range(C_FRAMES) for k in range(E_EDGES)]
    frame_of, kernel_of_slot, edge_slot = pkg._lib.derive_slots(frame_of_edge, kernel_of)
    seeds = list(range(1, B + 1))

    def slot_images(fs):  # the host path: one pass per kernel, the images back on the host, picked per slot
        per_k = [pkg.gpet_utils.comp_grad_imgs(fs, k, ctx=ctx) for k in K]
        return [per_k[kernel_of_slot[g]][frame_of[g]] for g in range(len(frame_of))]
    bt = pkg.GP_Edge_Tracing_Batch(inits, None, seeds, raw_imgs=sets[0], grad_kernel=K, kernel_of=kernel_of, image_of=frame_of_edge,
                                   _ctx=ctx, **KW)
    bh = pkg.GP_Edge_Tracing_Batch(inits, slot_images(sets[0]), seeds, image_of=edge_slot, _ctx=ctx, **KW)
    assert bt._batch.n_img == bh._batch.n_img == 2 * C_FRAMES

    def timed(fn):
        gc.collect()
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3
    set_t = lambda fs: lambda: bt.set_frame(None, None, seeds, raw_imgs=fs, next_frame=False)
    set_h = lambda fs: lambda: bh.set_frame(slot_images(fs), None, seeds, next_frame=False)
    step = lambda setter, b: lambda fs: lambda: (setter(fs)(), b())
    settled = lambda setter, fs_before, fn: (setter(fs_before)(), timed(fn))[1]
    variants = {
        "table_set_frame": lambda r: settled(set_t, sets[~r & 1], set_t(sets[r & 1])),
        "table_step": lambda r: settled(set_t, sets[~r & 1], step(set_t, bt)(sets[r & 1])),
        "host_set_frame": lambda r: settled(set_h, sets[~r & 1], set_h(sets[r & 1])),
        "host_step": lambda r: settled(set_h, sets[~r & 1], step(set_h, bh)(sets[r & 1])),
    }
    for fn in variants.values():  # warm-up
        fn(0)
    ms = {name: [] for name in variants}
    for r in range(args.reps):
        for name, fn in variants.items():
            ms[name].append(fn(r))
    set_t(sets[0])()
    out_t = bt()
    set_h(sets[0])()
    out_h = bh()
    same = bool(all(np.array_equal(a, b) for a, b in zip(out_t, out_h)) and bt.timings["iters"] == bh.timings["iters"])
    lines = ["Two kernels on shared raw frames: 256 edges as 32 frames x 8 edges, 64 image slots (tools/time_multi_kernel.py)",
             "=" * 110,
             "One MI355X, one process, 500 x 500 uint8 raw frames, two 11 x 5 kernels of opposite polarity, README RBF parameters,",
             "N_samples = 1000.  The variants alternate, %d rounds after one warm-up round; wall-clock ms per call, every timing ended by" % args.reps,
             "a synchronise; every timed call follows an untimed call of the same batch with the other set of frames.",
             "  table_*   set_frame(raw_imgs=32 frames) with the slot table: frames up once, 64 gradient images made on the device",
             "  host_*    comp_grad_imgs per kernel (gradient images back through the host), then set_frame(grad_imgs=64 images)",
             "  *_set_frame  set_frame alone     *_step  set_frame + trace", "",
             "%-16s %10s %10s %10s %10s %10s" % ("variant", "mean ms", "median ms", "min ms", "max ms", "range ms")]
    for name, v in ms.items():
        lines.append("%-16s %10.2f %10.2f %10.2f %10.2f %10.2f" % (name, np.mean(v), np.median(v), min(v), max(v), max(v) - min(v)))
    lines += ["", "table batch traces what the host-path batch traces (traces, iterations): %s; iterations per edge %d .. %d"
              % (same, min(bt.timings["iters"]), max(bt.timings["iters"]))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r11_multi_kernel.txt"))
    main(ap.parse_args())
