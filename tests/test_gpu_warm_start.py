"""GPU tests of the warm start on the device (gpet_batch_warm_start, k_warm_start; set_frame(..., warm_every=k)): the next frame's
observation sets come from the converged fits the last trace left on the device, by the rule of sequence.warm_start_obs.  The
oracle is the host path: a twin batch given obs=[warm_start_obs(trace, ...)] must be in the same state and trace the same."""
import numpy as np
import pytest

from oracle import gpet_oracle as orc

pytestmark = pytest.mark.gpu

N = 256
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 40, 'length_scale': 12}, noise_y=1, N_samples=300, score_thresh=1, delta_x=6,
          keep_ratio=0.1, pixel_thresh=4, fix_endpoints=True)
SEEDS0, SEEDS1 = [3, 4, 5, 6], [7, 8, 9, 10]


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def scene(amd, ctx):
    """Two sets of 4 gradient images (a frame and the next) of a drifting sinusoidal edge; edges 0, 1 span the image
    (Lg = 256, algo_thresh = 39), edges 2, 3 its inner half (Lg = 129, algo_thresh = 18)."""
    k = amd.gpet_utils.kernel_builder((11, 5))
    grads, truths = [], []
    for t in range(8):
        img, truth = orc.synth_sinusoid_image(N, 51 + t, amplitude=int(0.4 * N * (1.0 + 0.02 * t)))
        grads.append(amd.gpet_utils.comp_grad_img(img, k, ctx=ctx))
        truths.append(truth)
    ends = [(0, N - 1), (0, N - 1), (N // 4, 3 * N // 4), (N // 4, 3 * N // 4)]
    inits = [truths[e][[a, b], :][:, [1, 0]] for e, (a, b) in enumerate(ends)]
    return dict(first=grads[:4], second=grads[4:], inits=inits)


@pytest.fixture(scope="module")
def traced(amd, ctx, scene):
    """The first frame's traces, computed once (every test starts from a batch that has traced the first frame)."""
    b = amd.GP_Edge_Tracing_Batch(scene["inits"], scene["first"], SEEDS0, _ctx=ctx, **KW)
    out = b()
    iters = list(b.timings["iters"])
    b._batch.close()
    return out, iters


def traced_batch(amd, ctx, scene, traced):
    b = amd.GP_Edge_Tracing_Batch(scene["inits"], scene["first"], SEEDS0, _ctx=ctx, **KW)
    out = b()
    assert all(np.array_equal(a, w) for a, w in zip(out, traced[0])) and list(b.timings["iters"]) == traced[1]
    return b


def state(b):
    sc = b._batch.all_scalars()
    return b._batch.read_obs_all(), [(s.n_obs, s.done, s.iter, s.status) for s in sc]


@pytest.mark.parametrize("warm_every", [1, 3, 12, N])
def test_device_warm_start_equals_host_warm_start(amd, ctx, scene, traced, warm_every):
    from gaussian_process_edge_trace_amd.sequence import warm_start_obs
    dev, twin = traced_batch(amd, ctx, scene, traced), traced_batch(amd, ctx, scene, traced)
    ps = dev._ps
    assert [p["algo_thresh"] for p in ps] == [39, 39, 18, 18] and [p["edge_length"] for p in ps] == [256, 256, 129, 129]
    want = [warm_start_obs(traced[0][e], p["x_st"], p["x_en"], warm_every, p["algo_thresh"], p["M"]) for e, p in enumerate(ps)]
    dev.set_frame(scene["second"], None, SEEDS1, warm_every=warm_every)
    twin.set_frame(scene["second"], want, SEEDS1)
    (obs_d, sc_d), (obs_t, sc_t) = state(dev), state(twin)
    assert sc_d == sc_t, (sc_d, sc_t)
    assert [s[0] for s in sc_d] == [len(o) for o in want] and all(s[1:] == (0, 0, 0) for s in sc_d)  # not done, iter 0, status OK
    for e in range(4):
        assert obs_d[e].dtype == np.int64 and np.array_equal(obs_d[e], want[e]) and np.array_equal(obs_t[e], want[e]), e
        assert np.array_equal(dev._ps[e]["obs"], want[e]), e  # (read back once: what reset() sets again)
        assert len(want[e]) < ps[e]["algo_thresh"]
    if warm_every == 1:  # several doublings: 254 candidates, then 127, 63 -- all at or above the threshold of 39 -- then 31
        assert [len(o) for o in want[:2]] == [31, 31] and all(np.all(np.diff(o[:, 0]) == 8) for o in want[:2])
        assert all(np.all(np.diff(o[:, 0]) == 8) for o in want[2:])  # (127 inner candidates, 63, 31, then 15 below 18)
    if warm_every == N:
        assert all(len(o) == 0 for o in want)
    out_d, out_t = dev(), twin()
    assert list(dev.timings["iters"]) == list(twin.timings["iters"]) and min(dev.timings["iters"]) >= 1
    for e in range(4):
        assert np.array_equal(out_d[e], out_t[e]), e
    # reset() after a device warm start restores the same warm start: the same trace
    dev.reset()
    assert state(dev)[1] == sc_d and all(np.array_equal(a, w) for a, w in zip(state(dev)[0], want))
    again = dev()
    assert list(dev.timings["iters"]) == list(twin.timings["iters"])
    for e in range(4):
        assert np.array_equal(again[e], out_d[e]), e
    dev._batch.close()
    twin._batch.close()


def test_warm_start_needs_the_last_traces_converged_fits(amd, ctx, scene, traced):
    L = amd._lib
    fresh = amd.GP_Edge_Tracing_Batch(scene["inits"], scene["first"], SEEDS0, _ctx=ctx, **KW)
    with pytest.raises(L.GpetError) as ei:
        fresh.set_frame(scene["second"], None, SEEDS1, warm_every=12)
    assert ei.value.code == L.ERR_BAD_ARG and "converged fits" in str(ei.value)
    # refused before the images were swapped: the batch still traces its first frame, with its first seeds
    out = fresh()
    assert all(np.array_equal(a, w) for a, w in zip(out, traced[0])) and list(fresh.timings["iters"]) == traced[1]
    with pytest.raises(ValueError):
        fresh.set_frame(scene["second"], [np.zeros((0, 2))] * 4, SEEDS1, warm_every=12)  # obs and warm_every are alternatives
    fresh._batch.close()
    b = traced_batch(amd, ctx, scene, traced)
    cnt = b._batch.warm_start(12)
    assert cnt.dtype == np.int32 and cnt.tolist() == [len(o) for o in b._batch.read_obs_all()] and cnt.min() >= 1
    with pytest.raises(L.GpetError):  # a warm start without a trace in between
        b._batch.warm_start(12)
    b()
    b._batch.set_obs(0, np.array([[10, 20]], dtype=np.int64))
    with pytest.raises(L.GpetError):  # gpet_batch_set_obs has started another trace
        b._batch.warm_start(12)
    b()
    assert b._batch.warm_start(N).tolist() == [0, 0, 0, 0]  # (and a trace makes it possible again)
    b._batch.close()
