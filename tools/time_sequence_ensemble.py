"""What a frame-to-frame step of a sequence of seed ensembles costs on the device route and on the host route it replaces: one edge
of the bench's shape (500 columns on a shared 500 x 500 image, the README's RBF parameters) traced with B seeds in 8 groups (edge e in
group e % 8), then handed to the next frame.

  python tools/time_sequence_ensemble.py [--edges 32,256,1024] [--reps 7] [--out FILE]
      One process.  Per batch size, after one full trace, every variant is warmed up once and then timed --reps times between two
      events on the context's stream (gpet_timer_start / gpet_timer_stop_ms around the calls; every variant ends with a wait); medians,
      with min - max.  Before every timed call the batch is put back on the first frame and traced again (not timed):
        set_frame medoid    set_frame(next, warm_every=k, warm_from='medoid', group_of=g): readiness, the kept reduction read home as
                            last_ensemble, the image swap, the warm start, the observation sets read back once
        ... of which        the same four calls through _lib.Batch one by one: ensemble_keep, ensemble_kept (home), set_images,
                            warm_start_groups
        set_frame own fit   set_frame(next, warm_every=k): what a sequence of single seeds does today (gpet_batch_warm_start)
        host route          ensemble(g) home, warm_start_obs per group on the medoid's trace, set_frame(next, obs=[...]): B calls of
                            gpet_batch_set_obs, one wait each
      and a full step both ways (wall clock): the hand-over above plus the trace of the next frame (device loop, converged fits).
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
WARM = 10  # 2 * delta_x, trace_sequence's default


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", default="32,256,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gaussian_process_edge_trace_amd as pkg
    from gaussian_process_edge_trace_amd.sequence import warm_start_obs
    from oracle import gpet_oracle as orc
    L = pkg._lib
    ctx = L.Context(0)
    N = a.size
    k = pkg.gpet_utils.kernel_builder((11, 5))
    img, truth = orc.synth_sinusoid_image(N, 3, amplitude=int(0.4 * N))
    img2, _ = orc.synth_sinusoid_image(N, 4, amplitude=int(0.4 * N * 1.02))
    first, nxt = (pkg.gpet_utils.comp_grad_img(i, k, ctx=ctx) for i in (img, img2))
    init = truth[[0, -1], :][:, [1, 0]]
    med = lambda v: "%9.3f (%.3f - %.3f)" % (np.median(v), min(v), max(v))
    lines = ["one edge of %d columns on a shared %d x %d image, B seeds in 8 groups, warm_every = %d; ms, median (min - max) of %d calls "
             "after a warm-up" % (N, N, N, WARM, a.reps)]
    for B in [int(v) for v in a.edges.split(",")]:
        seeds = [1000 + 997 * s for s in range(B)]
        bt = pkg.GP_Edge_Tracing_Batch([init] * B, first, seeds, **KW, _ctx=ctx)
        g = (np.arange(B) % 8).astype(np.int32)
        p = bt._ps[0]

        def back():  # on the first frame, traced (not timed)
            bt.set_frame(first, None, seeds, next_frame=False)
            return bt()

        def device():
            bt.set_frame(nxt, None, seeds, warm_every=WARM, warm_from="medoid", group_of=g, tol=2)

        parts = {}

        def device_parts():
            lb = bt._batch
            for name, call in (("ensemble_keep", lambda: lb.ensemble_keep(g, 2.0)), ("ensemble_kept", lb.ensemble_kept),
                               ("set_images", lambda: lb.set_images([nxt], next_frame=True)),
                               ("warm_start_groups", lambda: lb.warm_start_groups("medoid", WARM))):
                ctx.sync()
                ctx.timer_start()
                call()
                parts.setdefault(name, []).append(ctx.timer_stop_ms())

        def own():
            bt.set_frame(nxt, None, seeds, warm_every=WARM)

        def host():
            traces = host.traces
            ens = bt.ensemble(g, 2)
            obs = [warm_start_obs(traces[d["medoid"]], p["x_st"], p["x_en"], WARM, p["algo_thresh"], p["M"]) for d in ens]
            bt.set_frame(nxt, [obs[e % 8] for e in range(B)], seeds)

        variants = {"set_frame medoid": device, "(its four calls)": device_parts, "set_frame own fit": own, "host route": host}
        ms = {name: [] for name in variants}
        step = {"device": [], "host": []}
        obs_dev = obs_host = None
        for rnd in range(a.reps + 1):
            for name, call in variants.items():
                host.traces = back()
                ctx.sync()
                ctx.timer_start()
                call()
                t = ctx.timer_stop_ms()
                if rnd:
                    ms[name].append(t)
                if name == "set_frame medoid":
                    obs_dev = bt._batch.read_obs_all()
                if name == "host route":
                    obs_host = bt._batch.read_obs_all()
            for name, call in (("device", device), ("host", host)):
                host.traces = back()
                ctx.sync()
                t0 = time.perf_counter()
                call()
                bt()
                ctx.sync()
                if rnd:
                    step[name].append(1e3 * (time.perf_counter() - t0))
        assert all(np.array_equal(x, y) for x, y in zip(obs_dev, obs_host)), "the two routes left different observation sets"
        lines.append("B = %d (%d observations per edge, equal on both routes):" % (B, len(obs_dev[0])))
        for name in variants:
            if name == "(its four calls)":
                lines.append("  %-18s %s" % (name, "; ".join("%s %.3f" % (n, np.median(v[1:])) for n, v in parts.items())))
            else:
                lines.append("  %-18s %s" % (name, med(ms[name])))
        lines.append("  %-18s device route %s; host route %s" % ("full step", med(step["device"]), med(step["host"])))
        bt._batch.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
