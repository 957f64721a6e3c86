"""How often a chain of single seeds and a chain of seed ensembles stay on the true edge: T drifting frames of the bench's scene (500
columns, the README's RBF parameters; the first frame is image seed 1, on which the tracer is bistable), one chain.

  python tools/sequence_ensemble_quality.py [--frames 6] [--seeds 8] [--out FILE]
      Per seed, trace_sequence(frames, init, seed=s): frames whose trace has MSE < 2000 against the true edge (the good branch of
      tests/test_gpu_sequence.py).  Then trace_sequence(frames, init, ensemble_seeds=all of them, warm_from=w) for every w: the same
      count for the medoid's result and for the consensus trace.  An observation, not a test.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 75, 'length_scale': 20}, noise_y=1, N_samples=1000, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
GOOD = 2000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gaussian_process_edge_trace_amd as pkg
    from oracle import gpet_oracle as orc
    ctx = pkg._lib.Context(0)
    N, T = a.size, a.frames
    k = pkg.gpet_utils.kernel_builder((11, 5))
    frames, truths = [], []
    for t in range(T):
        img, truth = orc.synth_sinusoid_image(N, 1 + t, amplitude=int(0.4 * N * (1.0 + 0.02 * t)))
        frames.append(pkg.gpet_utils.comp_grad_img(img, k, ctx=ctx))
        truths.append(truth)
    init = truths[0][[0, -1], :][:, [1, 0]]
    seeds = [1000 + 997 * s for s in range(a.seeds)]
    mse = lambda trace, t: float(pkg.gpet_utils.trace_MSE(trace, truths[t]))
    lines = ["%d drifting frames of %d x %d (first frame: image seed 1), one chain; frames with MSE < %.0f against the true edge" % (T, N, N, GOOD)]
    single = []
    for s in seeds:
        out = pkg.trace_sequence(frames, init, n_chains=1, seed=s, _ctx=ctx, **KW)
        m = [mse(out[t], t) for t in range(T)]
        single.append(sum(v < GOOD for v in m))
        lines.append("  single seed %5d: %d of %d   MSE %s" % (s, single[-1], T, np.round(m).astype(int).tolist()))
    lines.append("  single seeds: mean %.2f of %d frames, worst %d, best %d" % (np.mean(single), T, min(single), max(single)))
    for w in ("medoid", "best_cost", "consensus"):
        out = pkg.trace_sequence(frames, init, n_chains=1, ensemble_seeds=seeds, warm_from=w, _ctx=ctx, **KW)
        m_med = [mse(out[t]["result"], t) for t in range(T)]
        m_con = [mse(out[t]["trace"], t) for t in range(T)]
        lines.append("  ensemble of %d, warm_from=%-9s: medoid %d of %d, consensus %d of %d   medoid MSE %s"
                     % (len(seeds), w, sum(v < GOOD for v in m_med), T, sum(v < GOOD for v in m_con), T, np.round(m_med).astype(int).tolist()))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
