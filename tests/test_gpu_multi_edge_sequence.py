"""GPU tests of sequences with several edges per frame (SequenceTracer / trace_sequence with a list of inits): step s of C chains
is one batch of C x E edges on C images (an image map), warm-started on the device.  The oracle is the single-edge run: edge k of
the multi-edge result equals trace_sequence(frames, init_k, ...) bit for bit."""
import numpy as np
import pytest

from tests.test_gpu_sequence import make_sequence

pytestmark = pytest.mark.gpu

RBF = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 40, 'length_scale': 12}, noise_y=1, N_samples=300, score_thresh=1, delta_x=6,
           keep_ratio=0.1, pixel_thresh=4, fix_endpoints=True)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def two_inits(truths, N):
    """The full span, and the inner half [N/4, 3N/4] of the first frame's edge."""
    return truths[0][[0, -1], :][:, [1, 0]], truths[0][[N // 4, 3 * N // 4], :][:, [1, 0]]


def assert_edges_equal_single_runs(amd, ctx, frames, inits, n_chains, warm_every, seeds, kw):
    multi = amd.SequenceTracer(frames, list(inits), n_chains=n_chains, warm_every=warm_every, seeds=seeds, _ctx=ctx, **kw)
    got = multi()
    T, E = len(frames), len(inits)
    assert len(got) == T and all(isinstance(r, list) and len(r) == E for r in got)
    assert all(isinstance(it, list) and len(it) == E for it in multi.iterations)
    for k, init in enumerate(inits):
        single = amd.SequenceTracer(frames, init, n_chains=n_chains, warm_every=warm_every, seeds=seeds, _ctx=ctx, **kw)
        want = single()
        for t in range(T):
            assert multi.iterations[t][k] == single.iterations[t], (k, t, multi.iterations[t], single.iterations[t])
            assert got[t][k].shape == (len(range(int(init[0, 0]), int(init[-1, 0]) + 1)), 2)
            assert np.array_equal(got[t][k], want[t]), (k, t)
    return multi


def test_rbf_two_edges_two_chains_equal_the_single_edge_runs(amd, ctx):
    N, T = 256, 4
    frames, truths, _ = make_sequence(amd, ctx, N, T)
    multi = assert_edges_equal_single_runs(amd, ctx, frames, two_inits(truths, N), 2, 12, [5 + t for t in range(T)], RBF)
    assert multi._tracer.B == 4 and multi._tracer._batch.n_img == 2 and multi._tracer._batch.image_of == [0, 0, 1, 1]
    assert min(it for its in multi.iterations for it in its) >= 1  # warm frames do iterate
    # a 3-D array of inits is the list
    a, b = two_inits(truths, N)
    stacked = amd.trace_sequence(frames, np.stack([a, a]), n_chains=2, warm_every=12, seeds=[5 + t for t in range(T)], _ctx=ctx, **RBF)
    listed = amd.trace_sequence(frames, [a, a], n_chains=2, warm_every=12, seeds=[5 + t for t in range(T)], _ctx=ctx, **RBF)
    assert all(np.array_equal(s[k], l[k]) for s, l in zip(stacked, listed) for k in range(2))


def test_matern_two_edges_one_chain_equal_the_single_edge_runs(amd, ctx):
    """Matern-5/2: the any-rank factor, whose rows the next frame's first iteration starts from (GPET_IMAGES_NEXT_FRAME) -- an
    iterative solve to a tolerance, but a deterministic one per edge: an edge's rows, tags and observations are the same in the
    batch of two as in the batch of one, so the equality with the single-edge runs holds bit for bit."""
    N, T = 512, 3
    frames, truths, _ = make_sequence(amd, ctx, N, T)
    kw = dict(kernel_options={'kernel': 'Matern', 'nu': 2.5, 'sigma_f': 0.15 * N, 'length_scale': 0.04 * N}, noise_y=1,
              N_samples=300, score_thresh=1, delta_x=8, keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
    multi = assert_edges_equal_single_runs(amd, ctx, frames, two_inits(truths, N), 1, 16, [3 + t for t in range(T)], kw)
    assert multi._tracer._batch.info(0)["factor_cap"] > 96 and multi._tracer._batch.n_img == 1
    assert min(multi.iterations[t][k] for t in (1, 2) for k in (0, 1)) >= 1


def test_a_single_init_returns_what_it_always_returned(amd, ctx):
    N, T = 256, 3
    frames, truths, init = make_sequence(amd, ctx, N, T)
    st = amd.SequenceTracer(frames, init, n_chains=2, warm_every=12, seed=5, _ctx=ctx, **RBF)
    out = st()
    assert len(out) == T and all(isinstance(r, np.ndarray) and r.shape == (N, 2) for r in out)
    assert all(isinstance(it, (int, np.integer)) for it in st.iterations) and st._tracer._batch.image_of is None
    ci = amd.trace_sequence(frames, init, n_chains=1, warm_every=12, seed=5, return_std=True, _ctx=ctx, **RBF)
    assert all(isinstance(r, tuple) and r[0].shape == (N, 2) and len(r[1]) == 2 and r[1][0].shape == (N,) for r in ci)
    one = amd.trace_sequence(frames, [init], n_chains=1, warm_every=12, seed=5, _ctx=ctx, **RBF)  # (a list of one: lists of one)
    plain = amd.trace_sequence(frames, init, n_chains=1, warm_every=12, seed=5, _ctx=ctx, **RBF)
    assert all(isinstance(r, list) and len(r) == 1 and np.array_equal(r[0], p) for r, p in zip(one, plain))
