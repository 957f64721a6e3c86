"""GPU tests of seed ensembles inside sequences (trace_sequence / SequenceTracer with ensemble_seeds=): every frame is traced with K
seeds per init, and all K members of the next frame start from their group's medoid, best member or consensus -- reduced and
warm-started on the device while the batch lives, from the host when the shorter chains run out and the batch is rebuilt.  The oracle
is a host-driven loop: a FRESH GP_Edge_Tracing_Batch per step, laid out the same way, with ``obs`` from warm_start_obs of the previous
source, and ``.ensemble()``.  64 x 64 uint8 raw frames of one drifting edge, as the sequence tests use."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd.sequence import chain_slices, warm_start_obs
from tests.test_gpu_raw_frames import drifting_frames

pytestmark = pytest.mark.gpu

N, T, SEEDS, TOL, WARM = 64, 5, [3, 4, 5, 6], 2, 4
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
KEYS = ("trace", "median", "q_lo", "q_hi", "min", "max", "agree", "members", "off", "cost", "medoid", "best_cost")


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def seq(amd):
    frames, init = drifting_frames(N, T, 11, "uint8")
    inner = np.array([[N // 4, init[0, 1]], [3 * N // 4, init[1, 1]]])
    kernels = [amd.gpet_utils.kernel_builder((11, 5)), amd.gpet_utils.kernel_builder((7, 3))]
    return dict(frames=frames, inits=[init, inner], kernels=kernels)


def host_loop(amd, ctx, frames, inits, kernels, n_chains, warm_from, return_std):
    """Step by step, a fresh batch per step: chain-major, init-major, member-minor; one raw frame per active chain; the K members of
    (chain, init) start from warm_start_obs of the source of that chain's previous frame."""
    E, K = len(inits), len(SEEDS)
    chains = chain_slices(len(frames), n_chains)
    results, iterations, prev = [None] * len(frames), [None] * len(frames), {}
    for s in range(max(hi - lo for lo, hi in chains)):
        active = [(c, lo + s) for c, (lo, hi) in enumerate(chains) if lo + s < hi]
        edge_inits, seeds, image_of, kernel_of, obs, group_of = [], [], [], [], [], []
        for ci, (c, f) in enumerate(active):
            for k in range(E):
                for j in range(K):
                    edge_inits.append(inits[k])
                    seeds.append(SEEDS[j])
                    image_of.append(ci)
                    kernel_of.append(k)
                    group_of.append(ci * E + k)
                    obs.append(prev.get((c, k), np.zeros((0, 2), dtype=np.int64)))
        kw = dict(grad_kernel=kernels, kernel_of=kernel_of) if len(kernels) > 1 else dict(grad_kernel=kernels[0])
        b = amd.GP_Edge_Tracing_Batch(edge_inits, None, seeds, raw_imgs=[frames[f] for _, f in active], image_of=image_of, obs=obs,
                                      return_std=return_std, _ctx=ctx, **kw, **KW)
        out = b()
        ens = b.ensemble(np.array(group_of, dtype=np.int32), TOL)
        for ci, (c, f) in enumerate(active):
            dicts, its = [], []
            for k in range(E):
                d = dict(ens[ci * E + k])
                src = {"medoid": d["medoid"], "best_cost": d["best_cost"]}.get(warm_from)
                trace = d["trace"] if src is None else (out[src][0] if return_std else out[src])
                p = b._ps[(ci * E + k) * K]
                prev[c, k] = warm_start_obs(trace, p["x_st"], p["x_en"], WARM, p["algo_thresh"], p["M"])
                d["result"] = out[d["medoid"]]
                dicts.append(d)
                its.append(list(b.timings["iters"][(ci * E + k) * K:(ci * E + k + 1) * K]))
            results[f], iterations[f] = dicts, its
        b._batch.close()
    return results, iterations


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("warm_from", ["medoid", "best_cost", "consensus"])
@pytest.mark.parametrize("n_chains,n_inits", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_sequence_of_ensembles_equals_the_host_driven_loop(amd, ctx, seq, n_chains, n_inits, warm_from):
    E, K = n_inits, len(SEEDS)
    inits, kernels = seq["inits"][:E], seq["kernels"][:E]
    return_std = warm_from == "best_cost"  # (results as (trace, interval) once per layout)
    st = amd.SequenceTracer(seq["frames"], inits if E > 1 else inits[0], n_chains=n_chains, warm_every=WARM, ensemble_seeds=SEEDS,
                            ensemble_tol=TOL, warm_from=warm_from, grad_kernel=kernels if E > 1 else kernels[0], return_std=return_std,
                            _ctx=ctx, **KW)
    got = st()
    want, want_iters = host_loop(amd, ctx, seq["frames"], inits, kernels, n_chains, warm_from, return_std)
    assert len(got) == T
    # with two chains of 3 + 2 frames the batch shrinks after step 1: steps 1 (device) and 2 (rebuilt, from the host) are both warm
    assert st._tracer.B == E * K
    for t in range(T):
        dicts = got[t] if E > 1 else [got[t]]
        its = st.iterations[t] if E > 1 else [st.iterations[t]]
        assert len(dicts) == E and [list(i) for i in its] == want_iters[t], (t, its, want_iters[t])
        for k, (d, w) in enumerate(zip(dicts, want[t])):
            for key in KEYS:
                assert same(d[key], w[key]), (t, k, key, d[key], w[key])
            assert d["seeds"] == [SEEDS[e % K] for e in d["members"]] and len(d["members"]) == K
            assert d["medoid_seed"] == SEEDS[d["medoid"] % K]
            assert same(d["result"], w["result"]), (t, k, "result")
    assert min(i for t in range(T) for its in want_iters[t] for i in its) >= 1
    st._tracer._batch.close()


def test_set_frame_device_route_equals_host_route_per_policy(amd, ctx, seq):
    """One step, both routes on live batches: set_frame(warm_from=w) against set_frame(obs=warm_start_obs(source)) -- the state after
    it and the trace that follows."""
    K = len(SEEDS)
    init, k0 = seq["inits"][0], seq["kernels"][0]
    g = np.zeros(K, dtype=np.int32)
    for w in ("medoid", "best_cost", "consensus"):
        dev = amd.GP_Edge_Tracing_Batch([init] * K, None, SEEDS, raw_imgs=seq["frames"][0], grad_kernel=k0, _ctx=ctx, **KW)
        host = amd.GP_Edge_Tracing_Batch([init] * K, None, SEEDS, raw_imgs=seq["frames"][0], grad_kernel=k0, _ctx=ctx, **KW)
        out, out_h = dev(), host()
        assert same(out, out_h)
        d = host.ensemble(g, TOL)[0]
        trace = d["trace"] if w == "consensus" else out_h[d[w]]
        p = host._ps[0]
        obs = warm_start_obs(trace, p["x_st"], p["x_en"], WARM, p["algo_thresh"], p["M"])
        dev.set_frame(None, None, SEEDS, raw_imgs=seq["frames"][1], warm_every=WARM, warm_from=w, group_of=g, tol=TOL)
        host.set_frame(None, [obs] * K, SEEDS, raw_imgs=seq["frames"][1])
        assert same(dev.last_ensemble[0]["trace"], d["trace"]) and dev.last_ensemble[0]["medoid"] == d["medoid"]
        assert all(np.array_equal(o, obs) for o in dev._batch.read_obs_all()) and len(obs) >= 1
        assert [bytes(s) for s in dev._batch.all_scalars()] == [bytes(s) for s in host._batch.all_scalars()]
        assert same(dev(), host()) and list(dev.timings["iters"]) == list(host.timings["iters"])
        dev._batch.close()
        host._batch.close()
