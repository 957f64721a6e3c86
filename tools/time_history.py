"""What the iteration history costs a batch: the bench's edge (500 x 500 sinusoidal image, README RBF parameters, N_samples = 1000)
as batches of 32 and of 1024 edges on one shared image, with the history off and at its three levels.

  python tools/time_history.py --edges 32 --out FILE.json [--reps 5] [--cap 64] [--step-limit 120]
      One process on one MI355X, ONE batch: its history is switched (untimed) between off, 'obs', 'curves' and 'full' before every
      step, so that the levels share the batch's buffers, streams and hardware queues -- separate batch objects differed by up
      to 6 % among themselves at 32 edges whatever their level.  Every level is warmed up once, then the levels are ALTERNATED,
      --reps rounds; a timed step is reset + trace (loop and converged fits), a host clock around work that ends in a
      synchronise of the context's stream.  The loop's share (until every edge is done) is taken from
      the batch's own timings.  Every timed step runs under an alarm of --step-limit seconds that ends the process.  The traces of
      the four levels are compared: the level must not change them.  One read of the history (copy + decode) is timed per level.
  python tools/time_history.py --report A.json B.json ... --txt FILE
      The table: min / median / max per level, and the overhead of each level over 'off' (medians)."""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 75, 'length_scale': 20}, noise_y=1, N_samples=1000, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
LEVELS = ["off", "obs", "curves", "full"]
SIZE = 500


def measure(args):
    sys.path.insert(0, ROOT)
    import gaussian_process_edge_trace_amd as pkg
    from oracle import gpet_oracle as orc
    ctx = pkg._lib.Context(0)
    img, edge = orc.synth_sinusoid_image(SIZE, 3)
    grad = pkg.gpet_utils.comp_grad_img(img, pkg.gpet_utils.kernel_builder((11, 5)), ctx=ctx)
    init = edge[[0, -1], :][:, [1, 0]]
    E = args.edges
    seeds = list(range(1, E + 1))
    b = pkg.GP_Edge_Tracing_Batch([init] * E, grad, seeds, _ctx=ctx, **KW)
    outs, read_ms, hist_mib, dropped = {}, {}, {}, {}

    def step(lv):
        b._batch.set_history(None if lv == "off" else lv, args.cap)
        signal.alarm(args.step_limit)  # (a step that hangs ends the process: nothing more is started on the GPU)
        ctx.sync()
        t0 = time.perf_counter()
        b.reset()
        outs[lv] = b()
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        signal.alarm(0)
        return ms, b.timings["loop_s"] * 1e3

    for lv in LEVELS:  # warm-up
        step(lv)
    ms = {lv: [] for lv in LEVELS}
    loop_ms = {lv: [] for lv in LEVELS}
    for _ in range(args.reps):
        for lv in LEVELS:
            a, l = step(lv)
            ms[lv].append(a)
            loop_ms[lv].append(l)
    same = bool(all(all(np.array_equal(x, y) for x, y in zip(outs["off"], outs[lv])) for lv in LEVELS[1:]))
    iters = b.timings["iters"]
    for lv in LEVELS[1:]:
        step(lv)
        signal.alarm(args.step_limit)
        t0 = time.perf_counter()
        h = b.history()
        read_ms[lv] = (time.perf_counter() - t0) * 1e3
        signal.alarm(0)
        assert [x["n_iter"] + x["dropped"] for x in h] == list(iters)
        dropped[lv] = int(sum(x["dropped"] for x in h))
        hist_mib[lv] = b._batch.history_layout().edge_bytes * E / 2.0 ** 20
    res = dict(edges=E, reps=args.reps, cap=args.cap, ms=ms, loop_ms=loop_ms, traces_equal=same, iters=[int(min(iters)), int(max(iters))],
               iters_total=int(sum(iters)), read_ms=read_ms, hist_mib=hist_mib, dropped=dropped)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for lv in LEVELS:
        print("%5d edges %-7s trace min %9.2f median %9.2f max %9.2f ms   loop median %9.2f ms"
              % (E, lv, min(ms[lv]), np.median(ms[lv]), max(ms[lv]), np.median(loop_ms[lv])))
    print("traces equal at every level:", same)


def report(args):
    runs = [json.load(open(p)) for p in args.report]
    lines = ["Iteration history kept on the device: cost per level (tools/time_history.py)", "=" * 110,
             "One MI355X, one process per batch size; the bench's edge (500 x 500 sinusoidal image, RBF sigma_f=75 l=20, N_samples=1000,",
             "delta_x=5, pixel_thresh=5) as a batch on one shared image, seeds 1..E.  ONE batch, its history switched between off / 'obs' / 'curves' /",
             "'full' before every step (untimed); the levels alternate, %d rounds after one warm-up round; a step is reset + trace (loop + converged fits), wall-clock ms ended by a" % runs[0]["reps"],
             "synchronise; 'loop' is the share until every edge is done.  Overheads compare medians with 'off' of the same run.", "",
             "%-6s %-7s %10s %10s %10s %12s %12s %12s %10s %10s" % ("edges", "level", "min ms", "median ms", "max ms", "loop median", "trace vs off", "loop vs off",
                                                                "MiB", "read ms")]
    for r in runs:
        off, off_l = np.median(r["ms"]["off"]), np.median(r["loop_ms"]["off"])
        for lv in LEVELS:
            v, l = r["ms"][lv], r["loop_ms"][lv]
            lines.append("%-6d %-7s %10.2f %10.2f %10.2f %12.2f %+11.1f%% %+11.1f%% %10s %10s"
                         % (r["edges"], lv, min(v), np.median(v), max(v), np.median(l), 100 * (np.median(v) / off - 1), 100 * (np.median(l) / off_l - 1),
                            "%.1f" % r["hist_mib"][lv] if lv in r["hist_mib"] else "-", "%.1f" % r["read_ms"][lv] if lv in r["read_ms"] else "-"))
        lines.append("%-6d iterations per edge %d..%d (%d in all), history_cap %d, records dropped %s; traces equal at every level: %s"
                     % (r["edges"], r["iters"][0], r["iters"][1], r["iters_total"], r["cap"], r["dropped"], r["traces_equal"]))
        lines.append("%-6d run-to-run range of 'off' itself: %.1f %% of its median" % (r["edges"], 100 * (max(r["ms"]["off"]) - min(r["ms"]["off"])) / off))
        lines.append("")
    lines.append("'read ms' is one history() call: one device-to-host copy of the whole storage and its decoding into numpy arrays per edge.")
    text = "\n".join(lines) + "\n"
    with open(args.txt, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=32)
    ap.add_argument("--out", default="time_history.json")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--report", nargs="+")
    ap.add_argument("--txt", default="r10_history.txt")
    a = ap.parse_args()
    report(a) if a.report else measure(a)
