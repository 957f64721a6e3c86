"""Result records on the GPU (include/gpet_hip.h, "Result records"): k_finish_results packs what
GP_Edge_Tracing_Batch.finish computes on the host -- trace, credible interval -- plus the statistics of each trace, and the
sharded C-ABI path gathers them (gpet_gather_results) for edges of different widths."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 20, 'length_scale': 10}, noise_y=1, N_samples=256,
          score_thresh=1, delta_x=5, keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
MKW = dict(kernel_options={'kernel': 'Matern', 'nu': 2.5, 'sigma_f': 20, 'length_scale': 6}, noise_y=1, N_samples=200,
           score_thresh=1, delta_x=6, keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
# seven edges of four widths (128, 120, 112, 99 points) on one 128 x 128 image
SPANS = [(0, -1), (8, -1), (0, -17), (20, -10), (8, -1), (0, -1), (20, -10)]
WIDTHS = [128, 120, 112, 99, 120, 128, 99]


def _problem(amd, ctx, N=128):
    img, edge = amd.gpet_utils.construct_test_img((N, N), int(0.4 * N), 4, 0.05, 'sinusoidal', 0.3, gaps=True, seed=3)
    inits = [edge[[a, b], :][:, [1, 0]] for a, b in SPANS]
    grad = amd.gpet_utils.comp_grad_img(img, amd.gpet_utils.kernel_builder((11, 5)), ctx=ctx)
    return grad, inits


def _equal_ci(got, want):
    assert len(got) == len(want)
    for (t, (lo, up)), (tw, (low, upw)) in zip(got, want):
        assert t.shape == tw.shape and lo.shape == low.shape
        assert np.array_equal(t, tw) and np.array_equal(lo, low) and np.array_equal(up, upw)


@pytest.mark.gpu
@pytest.mark.parametrize("through_rccl", [0, 1])
def test_world_of_one_cabi_returns_intervals_and_stats(through_rccl):
    """trace_sharded_cabi(..., return_std=True, with_stats=True) over edges of four widths equals the single-process batch
    edge by edge: traces and both interval arrays array_equal, n_iter = the loop's iterations, theta = final_fits'."""
    import gaussian_process_edge_trace_amd as amd
    from gaussian_process_edge_trace_amd.sharding import trace_sharded_cabi
    L = amd._lib
    ctx = L.Context(0)
    grad, inits = _problem(amd, ctx)
    old = L.set_option("comm_force_rccl", through_rccl)
    try:
        comm = L.Comm(ctx, None, 1, 0)
    finally:
        L.set_option("comm_force_rccl", old)
    try:  # (the communicator is closed whatever happens: not left to interpreter shutdown)
        seeds = list(range(1, 8))
        got, stats = trace_sharded_cabi(grad, grad.shape, inits, seeds, comm, return_std=True, with_stats=True, **KW)
        b = amd.GP_Edge_Tracing_Batch(inits, grad, seeds, return_std=True, **KW, _ctx=ctx)
        want = b()
        assert [len(t) for t, _ in got] == WIDTHS
        _equal_ci(got, want)
        assert stats["n_iter"].tolist() == list(b.timings["iters"])
        fits = b.final_fits(b.timings["iters"])
        assert np.array_equal(stats["theta"], np.stack([f[2] for f in fits]))
        assert np.all(np.isfinite(stats["nlml"])) and np.all(stats["n_obs"] > 0)
        # bare traces of different widths: a list of (L_e, 2) traces
        bare = trace_sharded_cabi(grad, grad.shape, inits, seeds, comm, **KW)
        assert isinstance(bare, list) and all(np.array_equal(t, w[0]) for t, w in zip(bare, want))
    finally:
        comm.close()
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw,return_std", [(MKW, True), (KW, False)], ids=["matern52_ci", "rbf_bare"])
def test_batch_results_equal_finish_bit_for_bit(kw, return_std):
    """GP_Edge_Tracing_Batch.results() -- the records k_finish_results packs on the device -- equals what __call__ (the host's
    finish) returned, bit for bit, for a Matern-5/2 and an RBF batch."""
    import gaussian_process_edge_trace_amd as amd
    L = amd._lib
    ctx = L.Context(0)
    grad, inits = _problem(amd, ctx)
    inits = inits[:4]
    b = amd.GP_Edge_Tracing_Batch(inits, grad, [11, 12, 13, 14], return_std=return_std, **kw, _ctx=ctx)
    want = b()
    got, stats = b.results()
    if return_std:
        _equal_ci(got, want)
    else:
        assert all(t.shape == w.shape and np.array_equal(t, w) for t, w in zip(got, want))
    assert stats["n_iter"].tolist() == list(b.timings["iters"])
    # a wider record: the points past each edge are zero
    rec = b._batch.results(160)
    assert rec["trace"].shape == (4, 160, 2) and rec["edge_len"].tolist() == WIDTHS[:4]
    for e, w in enumerate(WIDTHS[:4]):
        assert rec["trace"][e, w - 1, 1] == inits[e][-1][0]
        assert not rec["trace"][e, w:].any() and not rec["lower"][e, w:].any() and not rec["upper"][e, w:].any()


@pytest.mark.gpu
def test_batch_results_refuse_without_a_converged_fit():
    """Before any converged fit, after reset() and after a new frame, gpet_batch_results raises instead of handing back the
    records of an earlier trace."""
    import gaussian_process_edge_trace_amd as amd
    L = amd._lib
    ctx = L.Context(0)
    grad, inits = _problem(amd, ctx)
    b = amd.GP_Edge_Tracing_Batch(inits[:2], grad, [1, 2], return_std=True, **KW, _ctx=ctx)
    with pytest.raises(L.GpetError) as ei:
        b.results()
    assert ei.value.code == L.ERR_BAD_ARG and "final_fit_all" in str(ei.value)
    b()
    b.results()
    with pytest.raises(L.GpetError):
        b._batch.results(64)  # (narrower than the widest edge)
    b.reset()
    with pytest.raises(L.GpetError):
        b.results()
    b()
    b.set_frame(grad)
    with pytest.raises(L.GpetError):
        b.results()


WORKER = r'''
import os, sys, time, pickle
import numpy as np
sys.path.insert(0, %(root)r)
import gaussian_process_edge_trace_amd as amd
from gaussian_process_edge_trace_amd.sharding import trace_sharded_cabi
rank, world, tmp = int(sys.argv[1]), 2, %(tmp)r
L = amd._lib
ctx = L.Context(rank)                      # one process per GPU
idf = os.path.join(tmp, "rccl_id.bin")
if rank == 0:
    uid = L.comm_unique_id()
    open(idf + ".tmp", "wb").write(uid)
    os.replace(idf + ".tmp", idf)
else:
    t0 = time.time()
    while not os.path.exists(idf):
        assert time.time() - t0 < 120
        time.sleep(0.05)
    uid = open(idf, "rb").read()
comm = L.Comm(ctx, uid, world, rank)
try:
    N = 128
    KW = %(kw)r
    SPANS = %(spans)r
    img, edge = amd.gpet_utils.construct_test_img((N, N), int(0.4 * N), 4, 0.05, 'sinusoidal', 0.3, gaps=True, seed=3)
    inits = [edge[[a, b], :][:, [1, 0]] for a, b in SPANS]
    grad = amd.gpet_utils.comp_grad_img(img, amd.gpet_utils.kernel_builder((11, 5)), ctx=ctx) if rank == 0 else None
    out = trace_sharded_cabi(grad, (N, N), inits, list(range(1, 8)), comm, return_std=True, with_stats=True, **KW)
    pickle.dump(out, open(os.path.join(tmp, "res_rank%%d.pkl" %% rank), "wb"))
finally:
    comm.close()
    ctx.close()
'''


@pytest.mark.gpu
def test_two_ranks_gather_results_over_rccl(tmp_path):
    """Two processes, one GPU each: the gathered result records (edges of four widths, intervals, stats) are the same on
    both ranks and equal the single-process batch."""
    import gaussian_process_edge_trace_amd as amd
    L = amd._lib
    try:
        L.Context(1).close()
    except L.GpetError:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    script = tmp_path / "results_worker.py"
    script.write_text(WORKER % dict(root=ROOT, tmp=str(tmp_path), kw=KW, spans=SPANS))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], env=env) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    (a, sa), (b, sb) = [pickle.load(open(tmp_path / ("res_rank%d.pkl" % r), "rb")) for r in range(2)]
    _equal_ci(a, b)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    ctx = L.Context(0)
    grad, inits = _problem(amd, ctx)
    tr = amd.GP_Edge_Tracing_Batch(inits, grad, list(range(1, 8)), return_std=True, **KW, _ctx=ctx)
    _equal_ci(a, tr())
    assert sa["n_iter"].tolist() == list(tr.timings["iters"])
