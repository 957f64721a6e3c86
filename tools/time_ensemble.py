"""What the seed-ensemble calls cost beside the route they replace and beside the trace itself: one edge of the bench's shape (500
columns on a shared 500 x 500 image, the README's RBF parameters) traced with B seeds in one batch.

  python tools/time_ensemble.py [--edges 32,256,1024] [--reps 7] [--host-edges 4] [--out FILE]
      One process.  Per batch size, after one full trace (which is also timed: "step" = reset, device loop, converged fits, one at a
      time), every variant is warmed up once and then timed --reps times between two events on the context's stream
      (gpet_timer_start / gpet_timer_stop_ms around the call, which ends with the copy home); medians, with min - max:
        final_costs        GP_Edge_Tracing_Batch.final_costs()
        ensemble 1 group   GP_Edge_Tracing_Batch.ensemble(tol=2), all B edges one group (final costs included)
        ensemble 8 groups  the same with edge e in group e % 8
      and the host route (wall clock, it is host work):
        results + numpy    results() home, then np.sort along the member axis of the traces' rows (all order statistics), np.rint
                           and the two counts
        B x cost_funct     the injection route of GP_Edge_Tracing.cost_funct per edge (read the edge's samples, put the mean in row 0,
                           score, read the costs, restore): timed on --host-edges edges and scaled to B
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 75, 'length_scale': 20}, noise_y=1, N_samples=1000, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)


def host_reduction(means, tol):
    s = np.sort(means, axis=0, kind="stable")
    n = s.shape[0]
    median = (s[(n - 1) // 2] + s[n // 2]) * 0.5
    c = np.rint(median)
    d = np.abs(np.rint(means) - c[None, :])
    return s[0], s[-1], s[(n - 1) // 4], s[n - 1 - (n - 1) // 4], median, (d <= tol).sum(axis=0), (d > tol).sum(axis=1)


def injection_cost(L, b, e, mean):
    Y = b.read(L.BUF_SAMPLES, e)
    saved = (Y[0].copy(), b.read(L.BUF_COSTS, e), b.read(L.BUF_BEST_IDX, e), b.read(L.BUF_BEST_COSTS, e))
    Y[0] = mean
    b.write(L.BUF_SAMPLES, Y, e)
    b.score()
    cost = float(b.read(L.BUF_COSTS, e)[0])
    Y[0] = saved[0]
    b.write(L.BUF_SAMPLES, Y, e)
    b.write(L.BUF_COSTS, saved[1], e)
    b.write(L.BUF_BEST_IDX, saved[2], e)
    b.write(L.BUF_BEST_COSTS, saved[3], e)
    return cost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", default="32,256,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-edges", type=int, default=4)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gaussian_process_edge_trace_amd as pkg
    from oracle import gpet_oracle as orc
    L = pkg._lib
    ctx = L.Context(0)
    N = a.size
    img, truth = orc.synth_sinusoid_image(N, 3)
    grad = pkg.gpet_utils.comp_grad_img(img, pkg.gpet_utils.kernel_builder((11, 5)), ctx=ctx)
    init = truth[[0, -1], :][:, [1, 0]]
    med = lambda v: "%9.3f (%.3f - %.3f)" % (np.median(v), min(v), max(v))
    lines = ["one edge of %d columns on a shared %d x %d image, B seeds in one batch; ms, median (min - max) of %d calls after a warm-up"
             % (N, N, N, a.reps)]
    for B in [int(v) for v in a.edges.split(",")]:
        bt = pkg.GP_Edge_Tracing_Batch([init] * B, grad, [1000 + 997 * k for k in range(B)], **KW, _ctx=ctx)
        bt()  # (warm: arena, streams, the optimiser's workspace)
        steps = []
        for _ in range(3):
            ctx.sync()
            t0 = time.perf_counter()
            bt.reset()
            bt()
            ctx.sync()
            steps.append(1e3 * (time.perf_counter() - t0))
        g8 = np.arange(B, dtype=np.int32) % 8
        device = {"final_costs": bt.final_costs, "ensemble 1 group": lambda: bt.ensemble(tol=2), "ensemble 8 groups": lambda: bt.ensemble(g8, tol=2)}
        ms = {k: [] for k in device}
        for rnd in range(a.reps + 1):
            for k, call in device.items():
                ctx.sync()
                ctx.timer_start()
                call()
                t = ctx.timer_stop_ms()
                if rnd:
                    ms[k].append(t)
        host = []
        for rnd in range(a.reps + 1):
            ctx.sync()
            t0 = time.perf_counter()
            res, _ = bt.results()
            rows = np.stack(res)[:, :, 0].astype(np.float64)  # (the records hold the ROUNDED means: the cheapest the host route gets)
            host_reduction(rows, 2)
            if rnd:
                host.append(1e3 * (time.perf_counter() - t0))
        costs = bt.final_costs()
        inj = []
        for e in range(min(a.host_edges, B)):
            mean = bt._batch.read(L.BUF_FIN_OUT, e)[0]
            ctx.sync()
            t0 = time.perf_counter()
            c = injection_cost(L, bt._batch, e, mean)
            inj.append(1e3 * (time.perf_counter() - t0))
            assert c == costs[e], (e, c, costs[e])
        ens = bt.ensemble(tol=2)[0]
        lines.append("B = %d: step (reset, loop, converged fits) %s; members agreeing per column: median %d of %d; medoid edge %d, "
                     "best-cost edge %d" % (B, med(steps), int(np.median(ens["agree"])), B, ens["medoid"], ens["best_cost"]))
        for k in device:
            lines.append("  %-18s %s" % (k, med(ms[k])))
        lines.append("  %-18s %s" % ("results + numpy", med(host)))
        lines.append("  %-18s %9.1f  (%.2f per edge, median of %d edges, x %d; every cost equal to final_costs' bit for bit)"
                     % ("B x cost_funct", np.median(inj) * B, np.median(inj), len(inj), B))
        bt._batch.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
