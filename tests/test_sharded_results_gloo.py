"""Sharded tracing returns what the single-GPU objects return (gloo on CPU, the CPU oracle as the tracer): tracers that
give ``(trace, (lower, upper))`` tuples (``return_std=True``) and edges of different widths on one image, at world 1, 2 and
8 (some ranks idle), for independent edges and for an image sequence.  Every rank's list equals the single-process result
edge by edge; uniform bare traces still come back as one ndarray."""
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from oracle import gpet_oracle as orc
from gaussian_process_edge_trace_amd.sequence import chain_slices, warm_start_obs

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 8, 'length_scale': 8}, noise_y=1, N_samples=128,
          score_thresh=1, delta_x=6, keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
N = 48
img, edge = orc.synth_sinusoid_image(N, 3)
# seven edges of four widths (48, 44, 40, 33 points) on one image
SPANS = [(0, -1), (4, -1), (0, -9), (10, -6), (0, -1), (4, -1), (10, -6)]
INITS = [edge[[a, b], :][:, [1, 0]] for a, b in SPANS]
SEEDS = [3 + 997 * e for e in range(len(INITS))]
T, C = 5, 3

def frame(t):
    return orc.comp_grad_img(orc.synth_sinusoid_image(N, 20 + t, amplitude=int(0.4 * N * (1 + 0.02 * t)))[0],
                             orc.kernel_builder((11, 5)))

def tracer_ci(grad, inits, seeds):       # what GP_Edge_Tracing_Batch(..., return_std=True) returns
    out = []
    for i, s in zip(inits, seeds):
        r = orc.trace(i, grad, seed=s, **KW)
        out.append((r[0], r[1]))
    return out

def tracer_bare(grad, inits, seeds):
    return [orc.trace(i, grad, seed=s, **KW)[0] for i, s in zip(inits, seeds)]

def seq_tracer_ci(block, first_frame, n_chains):   # SequenceTracer(..., return_std=True)
    init = INITS[0]
    out = []
    for lo, hi in chain_slices(len(block), n_chains):
        obs = np.zeros((0, 2), dtype=np.int64)
        for t in range(lo, hi):
            p = orc.resolve_params(init, np.asarray(block[t]), **KW)
            r = orc.trace(init, np.asarray(block[t]), obs=obs, seed=5 + first_frame + t, **KW)
            out.append((r[0], r[1]))
            obs = warm_start_obs(r[0], p["x_st"], p["x_en"], 8, p["algo_thresh"], p["M"])
    return out
'''
WORKER = COMMON + r'''
import pickle
import torch.distributed as dist
from gaussian_process_edge_trace_amd.sharding import trace_sharded, trace_sequence_sharded

W = %(world)d
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=W)
rank = dist.get_rank()
grad = orc.comp_grad_img(img, orc.kernel_builder((11, 5))) if rank == 0 else None   # rank 0 owns the image
res = dict(
    ci=trace_sharded(grad, (N, N), INITS, SEEDS, tracer_ci, dist),
    bare=trace_sharded(grad, (N, N), INITS, SEEDS, tracer_bare, dist),
    uniform=trace_sharded(grad, (N, N), [INITS[0]] * 3, SEEDS[:3], tracer_bare, dist),
    seq=trace_sequence_sharded(np.stack([frame(t) for t in range(T)]) if rank == 0 else None, (N, N), T, INITS[0], C,
                               seq_tracer_ci, dist))
pickle.dump(res, open(os.path.join(%(tmp)r, "res_rank%%d.pkl" %% rank), "wb"))
dist.barrier()
dist.destroy_process_group()
'''


def _single_process():
    """The single-process results, with the workers' BLAS thread count."""
    from threadpoolctl import threadpool_limits
    g = {}
    exec(COMMON % dict(root=ROOT), g)
    grad = g["orc"].comp_grad_img(g["img"], g["orc"].kernel_builder((11, 5)))
    with threadpool_limits(limits=1):
        ci = g["tracer_ci"](grad, g["INITS"], g["SEEDS"])
        seq = g["seq_tracer_ci"](np.stack([g["frame"](t) for t in range(g["T"])]), 0, g["C"])
    return g, grad, ci, seq


@pytest.fixture(scope="module")
def single():
    return _single_process()


def _equal_ci(got, want):
    assert len(got) == len(want)
    for (t, (lo, up)), (tw, (low, upw)) in zip(got, want):
        assert isinstance(lo, np.ndarray) and t.shape == tw.shape
        assert np.array_equal(t, tw) and np.array_equal(lo, low) and np.array_equal(up, upw)


def _equal_bare(got, want):
    assert isinstance(got, list) and len(got) == len(want)
    for t, tw in zip(got, want):
        assert np.array_equal(t, tw)


def test_world_of_one_takes_intervals_and_mixed_widths(single):
    """The two ValueErrors of np.stack: tuples from the tracer, and edges of different lengths."""
    from gaussian_process_edge_trace_amd.sharding import trace_sharded, trace_sequence_sharded
    from threadpoolctl import threadpool_limits
    g, grad, ci, seq = single
    with threadpool_limits(limits=1):
        _equal_ci(trace_sharded(grad, grad.shape, g["INITS"], g["SEEDS"], g["tracer_ci"]), ci)
        bare = trace_sharded(grad, grad.shape, g["INITS"], g["SEEDS"], g["tracer_bare"])
        uni = trace_sharded(grad, grad.shape, [g["INITS"][0]] * 3, g["SEEDS"][:3], g["tracer_bare"])
        frames = np.stack([g["frame"](t) for t in range(g["T"])])
        got_seq = trace_sequence_sharded(frames, frames.shape[1:], g["T"], g["INITS"][0], g["C"], g["seq_tracer_ci"])
    _equal_bare(bare, [c[0] for c in ci])
    assert [len(t) for t in bare] == [48, 44, 40, 33, 48, 44, 33]
    assert isinstance(uni, np.ndarray) and uni.shape == (3, 48, 2)
    assert np.array_equal(uni[0], ci[0][0])  # (edge 0 is the same init and seed)
    _equal_ci(got_seq, seq)


@pytest.mark.parametrize("world", [2, 8])
def test_gloo_world_gathers_intervals_and_mixed_widths(tmp_path, single, world):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    script = tmp_path / "worker.py"
    script.write_text(WORKER % dict(root=ROOT, port=port, tmp=str(tmp_path), world=world))
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], env=env) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    g, grad, ci, seq = single
    uniform_want = None
    for r in range(world):
        res = pickle.load(open(tmp_path / ("res_rank%d.pkl" % r), "rb"))
        _equal_ci(res["ci"], ci)
        _equal_bare(res["bare"], [c[0] for c in ci])
        _equal_ci(res["seq"], seq)
        assert isinstance(res["uniform"], np.ndarray) and res["uniform"].shape == (3, 48, 2)
        assert res["uniform"].dtype == np.int64
        if uniform_want is None:
            from threadpoolctl import threadpool_limits
            with threadpool_limits(limits=1):
                uniform_want = np.stack(g["tracer_bare"](grad, [g["INITS"][0]] * 3, g["SEEDS"][:3]))
        assert np.array_equal(res["uniform"], uniform_want)
