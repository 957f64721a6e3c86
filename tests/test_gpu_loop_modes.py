"""The device loop (gpet_trace_iterate) under every value of the options that only move WHERE and WHEN its work is enqueued
(csrc/gpet_loop_plan.h): each is documented as giving the same bits, so whole traces are compared exactly with the default run."""
import numpy as np
import pytest

from tests.test_oracle_vs_golden import CTOR

pytestmark = pytest.mark.gpu

# one edge and 8 edges (side stream, deep look-ahead; the chunked head needs 2..32 edges), 72 edges (above 64: one launch per group)
BATCHES = [1, 8, 72]
MODES = ([dict(rng_inline=v) for v in (0, 1, 2)] + [dict(rng_inline=0, rng_lookahead=v) for v in (0, 1, 4, 8)]
         + [dict(rng_head=v) for v in (0, 4, 8)] + [dict(rng_refill_at=v) for v in (0, 4, 6)]
         + [dict(loop_fused_tail=v) for v in (0, 1)])


@pytest.fixture(scope="module")
def run_trace(golden):
    import gaussian_process_edge_trace_amd as amd
    g = golden("stage_rbf500")  # (the 500-column image of test_full_trace_vs_oracle[trace_rbf500])
    kw = dict(CTOR["stage_rbf500"])
    kw.pop("seed")
    ctx = amd._lib.Context(0)
    defaults = {}

    def run(B, options):
        """Whole loop + converged fits of a FRESH batch of B edges (distinct seeds) with `options` set on that batch only."""
        if not options and B in defaults:
            return defaults[B]
        tr = amd.GP_Edge_Tracing_Batch([g["in_init"]] * B, g["ref_grad"], seeds=[3 + 7 * e for e in range(B)], **kw, _ctx=ctx)
        try:
            for name, value in options.items():
                assert tr._batch.set_option(name, value) == -1, "%s is not at its automatic default" % name
            traces = [np.asarray(t) for t in tr()]
            out = (list(tr.timings["iters"]), tr._batch.read_obs_all(), traces)
        finally:
            tr._batch.close()
        if not options:
            defaults[B] = out
        return out

    return run


@pytest.mark.parametrize("options", MODES, ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("B", BATCHES)
def test_loop_modes_give_the_default_bits(run_trace, B, options):
    iters0, obs0, traces0 = run_trace(B, {})
    assert min(iters0) >= 2 and len(obs0) == len(traces0) == B
    iters, obs, traces = run_trace(B, options)
    assert iters == iters0
    for e in range(B):
        assert np.array_equal(obs[e], obs0[e]), "observations of edge %d" % e
        assert np.array_equal(traces[e], traces0[e]), "trace of edge %d" % e


def test_fused_tail_gives_the_three_kernels_bits(golden):
    """k_score_tail against k_score_combine + k_topk_sort + k_kde_prep to the last bit of what they compute: two edges, every
    history record of the loop (the cases above compare the integer observations and the traces only)."""
    import gaussian_process_edge_trace_amd as amd
    g = golden("stage_rbf500")
    kw = dict(CTOR["stage_rbf500"])
    kw.pop("seed")
    ctx = amd._lib.Context(0)
    runs = []
    for fused in (0, 1):
        tr = amd.GP_Edge_Tracing_Batch([g["in_init"]] * 2, g["ref_grad"], seeds=[3, 10], **kw, history="curves", _ctx=ctx)
        try:
            assert tr._batch.set_option("loop_fused_tail", fused) == -1
            traces = [np.asarray(t) for t in tr()]
            runs.append((list(tr.timings["iters"]), traces, tr.history()))
        finally:
            tr._batch.close()
    (iters0, traces0, hist0), (iters1, traces1, hist1) = runs
    assert iters0 == iters1 and min(iters0) >= 2
    for e in range(2):
        h0, h1 = hist0[e], hist1[e]
        assert h0["n_iter"] == h1["n_iter"] == iters0[e] and h0["dropped"] == h1["dropped"] == 0
        for k in ("optimal_cost", "best_idx", "n_removed", "score_thresh", "n_obs"):
            assert h0[k].tobytes() == h1[k].tobytes() and len(h0[k]) == iters0[e], (e, k)
        for i in range(iters0[e]):
            assert h0["optimal_curves"][i].tobytes() == h1["optimal_curves"][i].tobytes(), (e, i)
        assert traces0[e].tobytes() == traces1[e].tobytes(), e
