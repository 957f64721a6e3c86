"""What an image map and the device warm start save a job of several edges per frame: 256 edges as 32 frames x 8 edges of
500 x 500 uint8 raw frames with the 11 x 5 kernel, the README's RBF parameters.  The same script times this commit and the commit
before it (which has neither): it measures what the tree it is pointed at can do.

  python tools/time_image_map.py --root TREE --label NAME --out FILE.json [--reps 5]
      One process on one MI355X, the package imported from TREE.  Every variant is warmed up once, then the variants are
      ALTERNATED, --reps rounds; every timing is a host clock around work that ends in a synchronise of the context's stream (a
      trace ends with its results on the host).  ms per call.  Every timed call of a batch follows an untimed call of the same
      batch (a set_frame with the other set of frames; a reset + trace for the shared batch): the first upload after ANOTHER
      large batch was created and freed costs 16 ms more than the next (256 edges, either commit), and which batch the variant
      before it frees differs between the commits (trace_sequence: 256 edges here, 32 there).
        dup_set_frame / dup_step        256 frames (every frame 8 times) into a batch with one image per edge: set_frame alone, and
                                        set_frame + trace (a full step)                                  -- the only form before
        map_set_frame / map_step        32 frames into the batch with the image map [c for c in range(32) for _ in range(8)]
        shared_step                     reset + trace of 256 edges on one shared image                   -- the gate's second leg
        seq_first / seq_next            trace_sequence at 32 chains x 8 edges: with a list of 8 inits (one batch of 256 edges per
                                        step, device warm start) where the tree has it, else 8 runs of 32 chains, one per init
                                        (a batch of 32 edges per step and init, warm start through the host).  seq_first: a
                                        sequence of ONE step (32 frames) -- batch construction (arena, basis setup: 1 batch here,
                                        8 there) and a cold trace.  seq_next: per step after the first -- (a sequence of 3 steps
                                        minus seq_first of the same round) / 2: set_frame, warm start, trace
  python tools/time_image_map.py --report A.json B.json ... --txt FILE
      The table of every run, the spread of each figure, and the gate: dup_step and shared_step of the runs labelled "this" against
      the runs labelled "parent", with the parent's own range over its repeats as the yardstick.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 75, 'length_scale': 20}, noise_y=1, N_samples=1000, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
C_FRAMES, E_EDGES, SIZE = 32, 8, 500


def make_frames(n, seed):
    """n distinct uint8 frames: 8 step edges at the rows the inits sit on, plus noise."""
    rng = np.random.default_rng(seed)
    base = np.zeros((SIZE, SIZE))
    for k in range(E_EDGES):
        base[60 + 50 * k:] += 0.1
    return [np.rint(np.clip(base + rng.normal(0.0, 0.05, size=base.shape), 0.0, 1.0) * 255.0).astype(np.uint8) for _ in range(n)]


def inits():
    return [np.array([[0, 60 + 50 * k], [SIZE - 1, 60 + 50 * k]]) for k in range(E_EDGES)]


def measure(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import inspect
    import gaussian_process_edge_trace_amd as pkg
    assert os.path.abspath(pkg.__file__).startswith(os.path.abspath(args.root)), pkg.__file__
    has_map = "image_of" in inspect.signature(pkg.GP_Edge_Tracing_Batch.__init__).parameters
    ctx = pkg._lib.Context(0)
    k = pkg.gpet_utils.kernel_builder((11, 5))
    B = C_FRAMES * E_EDGES
    sets = [make_frames(C_FRAMES, s) for s in (1, 2)]  # two sets of 32 frames, alternated
    image_of = [c for c in range(C_FRAMES) for _ in range(E_EDGES)]
    edge_inits = [i for _ in range(C_FRAMES) for i in inits()]
    seeds = list(range(1, B + 1))
    dup = lambda fs: [fs[c] for c in image_of]
    variants = {}
    bd = pkg.GP_Edge_Tracing_Batch(edge_inits, None, seeds, raw_imgs=dup(sets[0]), grad_kernel=k, _ctx=ctx, **KW)

    def timed(fn):
        gc.collect()  # (a batch the variant before left to the collector -- trace_sequence's last one -- is freed here, not inside fn)
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    def set_only(b, fs):
        return lambda: b.set_frame(None, None, seeds, raw_imgs=fs, next_frame=False)

    def step(b, fs):
        def run():
            b.set_frame(None, None, seeds, raw_imgs=fs, next_frame=False)
            b()
        return run
    def settled(b, fs, fn):  # the timed call follows an untimed set_frame of the same batch (see the docstring)
        set_only(b, fs)()
        return timed(fn)
    variants["dup_set_frame"] = lambda r: settled(bd, dup(sets[~r & 1]), set_only(bd, dup(sets[r & 1])))
    variants["dup_step"] = lambda r: settled(bd, dup(sets[~r & 1]), step(bd, dup(sets[r & 1])))
    if has_map:
        bm = pkg.GP_Edge_Tracing_Batch(edge_inits, None, seeds, raw_imgs=sets[0], grad_kernel=k, image_of=image_of, _ctx=ctx, **KW)
        variants["map_set_frame"] = lambda r: settled(bm, sets[~r & 1], set_only(bm, sets[r & 1]))
        variants["map_step"] = lambda r: settled(bm, sets[~r & 1], step(bm, sets[r & 1]))
    grad0 = pkg.gpet_utils.comp_grad_img(sets[0][0], k, ctx=ctx)
    bs = pkg.GP_Edge_Tracing_Batch(edge_inits, grad0, seeds, _ctx=ctx, **KW)

    def shared():
        bs.reset()
        bs()
    variants["shared_step"] = lambda r: (shared(), timed(shared))[1]
    n_steps = 3
    seq_frames = make_frames(C_FRAMES * n_steps, 3)

    def seq(frames):
        def run():
            if has_map:
                pkg.trace_sequence(frames, inits(), n_chains=C_FRAMES, warm_every=10, seed=3, grad_kernel=k, _ctx=ctx, **KW)
            else:
                for i in inits():
                    pkg.trace_sequence(frames, i, n_chains=C_FRAMES, warm_every=10, seed=3, grad_kernel=k, _ctx=ctx, **KW)
        return run
    first = {}

    def seq_first(r):
        first[r] = timed(seq(seq_frames[:C_FRAMES]))
        return first[r]
    variants["seq_first"] = seq_first
    variants["seq_next"] = lambda r: (timed(seq(seq_frames)) - first[r]) / (n_steps - 1)  # (after seq_first of the same round)
    for name, fn in variants.items():  # warm-up
        fn(0)
    ms = {name: [] for name in variants}
    for r in range(args.reps):
        for name, fn in variants.items():
            ms[name].append(fn(r))
    # the outputs the variants must share: the mapped batch traces what the duplicated one traces
    same = None
    if has_map:
        step(bd, dup(sets[0]))()
        out_d = bd()
        step(bm, sets[0])()
        out_m = bm()
        same = bool(all(np.array_equal(a, b) for a, b in zip(out_d, out_m)) and bd.timings["iters"] == bm.timings["iters"])
    res = dict(label=args.label, has_map=has_map, reps=args.reps, ms=ms, mapped_equals_duplicated=same,
               iters_dup=[int(min(bd.timings["iters"])), int(max(bd.timings["iters"]))])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for name, v in ms.items():
        print("%-14s %-8s mean %9.2f  min %9.2f  max %9.2f ms" % (name, args.label, np.mean(v), min(v), max(v)))
    print("mapped == duplicated:", same)


def report(args):
    runs = [json.load(open(p)) for p in args.report]
    lines = ["Image map and device warm start: 256 edges as 32 frames x 8 edges (tools/time_image_map.py)",
             "=" * 110,
             "One MI355X, one process per run, 500 x 500 uint8 raw frames, 11 x 5 kernel, README RBF parameters, N_samples = 1000.",
             "Runs of this commit ('this') and of the commit before it ('parent') alternate on the same machine in one visit; inside a run",
             "the variants alternate, %d rounds after one warm-up round; wall-clock ms per call, every timing ended by a synchronise." % runs[0]["reps"],
             "Every timed call follows an untimed call of the same batch, so that none pays for the memory the variant before it freed.",
             "  dup_*     256 frames (each frame 8 times) into a batch with one image per edge     map_*    32 frames, image map",
             "  *_set_frame  set_frame alone     *_step  set_frame + trace     shared_step  reset + trace, one shared image",
             "  seq_*     trace_sequence, 32 chains x 8 edges: this = one batch of 256 edges per step, device warm start;",
             "            parent = 8 runs, one per init, batches of 32 edges, warm start through the host",
             "            seq_first = a sequence of one step: batch construction (1 batch / 8 batches) and a cold trace",
             "            seq_next  = per step after the first: (a sequence of 3 steps - seq_first of the same round) / 2", "",
             "%-6s %-8s %-14s %10s %10s %10s %10s" % ("run", "commit", "variant", "mean ms", "min ms", "max ms", "range ms")]
    by = {}
    for i, r in enumerate(runs):
        for name, v in r["ms"].items():
            lines.append("%-6d %-8s %-14s %10.2f %10.2f %10.2f %10.2f" % (i, r["label"], name, np.mean(v), min(v), max(v), max(v) - min(v)))
            by.setdefault((r["label"], name), []).extend(v)
        if r["mapped_equals_duplicated"] is not None:
            lines.append("%-6d %-8s mapped batch traces what the duplicated batch traces (traces, iterations): %s; iterations per edge %s"
                         % (i, r["label"], r["mapped_equals_duplicated"], r["iters_dup"]))
    lines += ["", "All repeats of all runs of a commit pooled:"]
    for (label, name), v in sorted(by.items()):
        lines.append("  %-8s %-14s mean %9.2f  median %9.2f  min %9.2f  max %9.2f  (n = %d)" % (label, name, np.mean(v), np.median(v), min(v), max(v), len(v)))
    if ("this", "map_step") in by:
        B = C_FRAMES * E_EDGES
        d, m, sh = (float(np.median(by["this", n])) for n in ("dup_step", "map_step", "shared_step"))
        lines += ["", "Shared against distinct images on this commit (medians; dup_step and map_step include their set_frame, shared_step a reset):",
                  "  256 distinct images %.2f ms (%.0f traces/s), 32 images x 8 edges %.2f ms (%.0f traces/s), one shared image %.2f ms (%.0f traces/s)"
                  % (d, 1e3 * B / d, m, 1e3 * B / m, sh, 1e3 * B / sh),
                  "  grouping closes %.0f %% of the gap between 256 distinct images and one shared image" % (100.0 * (d - m) / (d - sh) if d != sh else 0.0)]
    lines += ["", "Gate: a batch with one image per edge (dup_step) and a shared batch (shared_step) are not slower on this commit than on the",
              "parent by more than the parent's own run-to-run spread: the range over the five repeats of the parent run next to it",
              "(runs are paired in the order they were made: first parent with first this, ...)."]
    ok = True
    parents, these = [r for r in runs if r["label"] == "parent"], [r for r in runs if r["label"] == "this"]
    if not parents or len(parents) != len(these):
        lines.append("  not measured on both commits in pairs")
        ok = False
    for i, (rp, rt) in enumerate(zip(parents, these)):
        for name in ("dup_step", "shared_step"):
            p, t = rp["ms"][name], rt["ms"][name]
            spread = max(p) - min(p)
            diff = float(np.mean(t) - np.mean(p))
            good = diff <= spread
            ok = ok and good
            lines.append("  pair %d %-12s parent mean %.2f ms, range %.2f ms; this mean %.2f ms; this - parent = %+.2f ms -> %s"
                         % (i, name, np.mean(p), spread, np.mean(t), diff, "within the spread" if good else "SLOWER than the spread allows"))
    lines.append("  gate: %s" % ("met" if ok else "NOT met"))
    text = "\n".join(lines) + "\n"
    with open(args.txt, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default="time_image_map.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--report", nargs="+")
    ap.add_argument("--txt", default="r09_image_map.txt")
    a = ap.parse_args()
    report(a) if a.report else measure(a)
