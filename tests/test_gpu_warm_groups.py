"""GPU tests of the warm start from a group's medoid, best member or consensus and from another edge (gpet_batch_ensemble_keep,
gpet_batch_ensemble_kept, gpet_batch_warm_start_groups, gpet_batch_warm_start_from; k_warm_start_src).  The oracle is the host: the
definition in numpy (tests/warm_groups_ref.py, on tests/ensemble_ref.py and sequence.warm_start_obs) gives every edge's observation
set, and a twin batch with the same injected fits is given them through gpet_batch_set_obs, edge by edge -- observations, scalars and
the trace that follows must be equal, bit for bit.

The scene is the 72-column one of tests/test_gpu_ensemble.py: edges of 70 points (68 candidates at stride 1: past one wave's 64 lanes,
with a remainder; algo_thresh 4) and of 40 points (inside one wave; algo_thresh 1, so the rule thins them down to nothing) in one call,
with fits INJECTED into fin_out after one real converged trace."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_ensemble import KW, N40, N70, TIE_A, TIE_B, injected_means, scene, table
from tests.warm_groups_ref import FROM, first_pass_count, trace_of_mean, warm_groups_ref

pytestmark = pytest.mark.gpu

B = N70 + N40
EXCLUDED = (3, 60, 77, 78)   # device status set non-OK before the converged fit: never members, still destinations
ODD = (20, 50, 52)           # means that leave the image both ways; edge 20's is NaN in places as well
TOL = 2.0
# g0, g1: the medoid ties of tests/test_gpu_ensemble.py (cost, then index); g2: 11 members of 12 assigned (edge 3 stopped);
# g3: one member with an odd mean; g4: an odd member and a stopped edge that receives it; g5: both edges stopped -- emptied;
# g6: the 40-point edges; g7: two curves 8 px off the true edge and one on it (the cheapest is not the medoid).  Every other edge,
# odd edge 20 among them: in no group
GROUPS = table(g0=TIE_A, g1=TIE_B, g2=range(0, 12), g3=[50], g4=[52, 60], g5=[77, 78], g6=range(71, 77), g7=[61, 62, 63])


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def world(amd, ctx):
    """The two gradient images (the frame the fits belong to and the next one), the inits and the injected means."""
    grad, truth = scene(amd, ctx, 72, 3)
    nxt, _ = scene(amd, ctx, 72, 4)
    means = injected_means(truth)
    for e in ODD:
        m = means[e]
        # at the indices the strides 16, 20, 24 and 32 visit, and around them: below 0, above M - 1 = 71, and the last rows inside
        m[16], m[20], m[40], m[48], m[64] = -3.2, 75.7, 71.6, 71.4, -0.4
        m[10], m[11] = -1.0, 72.0
    # NaN (no order: the reduction's definition leaves it out, so in no group -- the edge's own fit, and the explicit form)
    means[20][24], means[20][32], means[20][12] = np.nan, np.nan, np.nan
    curve = truth[1:71, 0].astype(np.float64)
    means[61], means[62], means[63] = curve + 8.0, curve + 8.4, curve.copy()
    inits = [truth[[1, 70], :][:, [1, 0]]] * N70 + [truth[[5, 44], :][:, [1, 0]]] * N40
    return dict(grad=grad, nxt=nxt, means=means, inits=inits, truth=truth)


def injected(amd, ctx, world, excluded=EXCLUDED):
    """A batch of the 79 edges after one real trace with a converged fit, the stopped edges' statuses set before the fit (as
    tests/test_gpu_ensemble.py::inj does), and the means written into fin_out."""
    L = amd._lib
    b = amd.GP_Edge_Tracing_Batch(world["inits"], world["grad"], list(range(1, B + 1)), **KW, _ctx=ctx)
    iters = b.run_loop()
    for e in excluded:
        s = b._batch.scalars(e)
        s.status = L.ERR_STATE
        b._batch.write_scalars(s, e)
    if excluded:
        with pytest.raises(L.GpetError) as ei:
            b.finish(iters)
        assert ei.value.code == L.ERR_STATE
    else:
        b.finish(iters)
    for e, m in enumerate(world["means"]):
        b._batch.write(L.BUF_FIN_OUT, np.stack([m, np.ones_like(m)]), e)
    return b


def state(b):
    return b._batch.read_obs_all(), [bytes(s) for s in b._batch.all_scalars()]


def assert_same_state_and_trace(dev, twin, what):
    (obs_d, sc_d), (obs_t, sc_t) = state(dev), state(twin)
    for e in range(dev.B):
        assert obs_d[e].dtype == np.int64 and np.array_equal(obs_d[e], obs_t[e]), (what, "obs", e, obs_d[e], obs_t[e])
        assert sc_d[e] == sc_t[e], (what, "scalars", e)
    ra, rb = dev(), twin()
    assert list(dev.timings["iters"]) == list(twin.timings["iters"]) and min(dev.timings["iters"]) >= 1, what
    for e, (ta, tb) in enumerate(zip(ra, rb)):
        assert np.array_equal(ta, tb), (what, "trace", e)


def test_the_scenario_holds_the_cases_it_is_meant_to(amd, ctx, world):
    """Statements about the definition's answer on the injected fits (not about the code under test): every case of the issue is in."""
    b = injected(amd, ctx, world)
    costs = b.final_costs()
    ps = b._ps
    assert [ps[0][k] for k in ("x_st", "x_en", "algo_thresh", "M")] == [1, 70, 4, 72]
    assert [ps[71][k] for k in ("x_st", "x_en", "algo_thresh", "M")] == [5, 44, 1, 72]
    _, src_m, groups = warm_groups_ref(world["means"], ps, GROUPS, TOL, costs, EXCLUDED, "medoid", 5)
    _, src_b, _ = warm_groups_ref(world["means"], ps, GROUPS, TOL, costs, EXCLUDED, "best_cost", 5)
    # a medoid that is not its group's first edge: by cost in one tie group, then by index
    firsts = [int(np.flatnonzero(GROUPS == g)[0]) for g in range(8)]
    assert (groups[0]["medoid"], groups[1]["medoid"]) in ((30, 42), (31, 40))
    assert groups[0]["off"].tolist() == [0, 0, 0] and groups[1]["off"].tolist() == [0, 0, 0]
    assert any(groups[g]["medoid"] != firsts[g] for g in (0, 1))
    assert costs[31] == costs[32] and groups[0]["medoid"] != 32  # (equal off and cost: the smaller index)
    # best cost that is not the medoid
    assert groups[7]["best_cost"] == 63 and groups[7]["medoid"] in (61, 62)
    # a consensus that equals no member's trace
    assert all(not np.array_equal(trace_of_mean(world["means"][e], 1)[:, 0], groups[2]["trace"][:, 0]) for e in groups[2]["members"])
    # stopped edges: no members, but destinations; a group emptied that way
    assert 3 not in groups[2]["members"] and src_m[3] == groups[2]["medoid"] >= 0
    assert groups[4]["members"].tolist() == [52] and src_m[60] == 52 and src_b[60] == 52
    assert groups[5]["members"].tolist() == [] and src_m[77] == src_m[78] == -1
    # outside any group
    assert src_m[20] == 20 and src_m[45] == 45
    # the stride: 1 and 5 are doubled, 24 is not (70-point edges; any stride is too dense for algo_thresh 1)
    t0 = trace_of_mean(world["means"][0], 1)
    assert first_pass_count(t0, ps[0], 1) == 68 and first_pass_count(t0, ps[0], 5) == 13 and first_pass_count(t0, ps[0], 24) == 2
    assert first_pass_count(trace_of_mean(world["means"][52], 1), ps[52], 1) == 63  # (rows outside the image are no candidates)
    assert first_pass_count(trace_of_mean(world["means"][20], 1), ps[20], 1) == 60  # (nor are NaN)
    b._batch.close()


@pytest.mark.parametrize("warm_every", [1, 5, 24])
@pytest.mark.parametrize("frm", FROM)
def test_group_warm_start_equals_the_definition_through_set_obs(amd, ctx, world, frm, warm_every):
    dev, twin = injected(amd, ctx, world), injected(amd, ctx, world)
    ps = dev._ps
    costs = dev.final_costs()  # (on the frame the fits belong to: what breaks the medoid's ties and defines best_cost)
    want, src, groups = warm_groups_ref(world["means"], ps, GROUPS, TOL, costs, EXCLUDED, frm, warm_every)
    if warm_every in (1, 5):  # the host rule doubled the stride at least once
        assert first_pass_count(trace_of_mean(world["means"][45], 1), ps[45], warm_every) >= ps[45]["algo_thresh"]
        assert len(want[45]) < first_pass_count(trace_of_mean(world["means"][45], 1), ps[45], warm_every)
    # device: keep, swap, warm start
    dev._batch.ensemble_keep(GROUPS, TOL)
    dev._batch.set_images([world["nxt"]], next_frame=True)
    cnt, src_out = dev._batch.warm_start_groups(frm, warm_every)
    # twin: swap, then one gpet_batch_set_obs per edge
    twin._batch.set_images([world["nxt"]], next_frame=True)
    for e in range(B):
        twin._batch.set_obs(e, want[e])
    assert src_out.dtype == np.int32 and np.array_equal(src_out, src), (src_out, src)
    assert np.array_equal(src_out, amd._lib.warm_sources(GROUPS, groups, frm))
    assert cnt.dtype == np.int32 and cnt.tolist() == [len(o) for o in want]
    assert all(len(o) == 0 for o in want[N70:]) and max(len(o) for o in want[:N70]) >= 1
    got = dev._batch.read_obs_all()
    for e in range(B):
        assert np.array_equal(got[e], want[e]), (e, got[e], want[e])
    assert_same_state_and_trace(dev, twin, (frm, warm_every))
    dev._batch.close()
    twin._batch.close()


def test_refused_images_touch_neither_the_ensemble_nor_the_batch(amd, ctx, world):
    """Two gradient images for the batch of one shared image: refused before the ensemble is kept, so ``last_ensemble`` stays and the
    next accepted call leaves what it leaves on a twin that never saw the refused one."""
    dev, twin = injected(amd, ctx, world), injected(amd, ctx, world)
    dev.last_ensemble = before = ["the ensemble of the frame before"]
    with pytest.raises(ValueError) as err:
        dev.set_frame([world["nxt"], world["nxt"]], warm_every=5, warm_from="medoid", group_of=GROUPS, tol=TOL)
    assert str(err.value) == "the new images do not fit the batch: 2 given (one shared image, 72 x 72)"
    assert dev.last_ensemble is before
    for b in (dev, twin):
        b.set_frame(world["nxt"], warm_every=5, warm_from="medoid", group_of=GROUPS, tol=TOL)
    assert len(dev.last_ensemble) == 8
    assert_same_state_and_trace(dev, twin, "after a refused call")
    dev._batch.close()
    twin._batch.close()


# ---- identity, the kept ensemble's life, refusals --------------------------------------------------------------------------------
SMALL = [0, 1, 2, 71, 72]  # three 70-point edges and two 40-point edges of the scene, traced as they are


def small_batch(amd, ctx, world, seeds=(3, 4, 5, 6, 7)):
    return amd.GP_Edge_Tracing_Batch([world["inits"][e] for e in SMALL], world["grad"], list(seeds), **KW, _ctx=ctx)


@pytest.fixture(scope="module")
def small_first(amd, ctx, world):
    b = small_batch(amd, ctx, world)
    out = b()
    iters = list(b.timings["iters"])
    b._batch.close()
    return out, iters


def assert_traces_old_frames(b, small_first):
    out = b()
    assert list(b.timings["iters"]) == small_first[1] and all(np.array_equal(a, w) for a, w in zip(out, small_first[0]))


@pytest.mark.parametrize("warm_every", [1, 24])
def test_identity_table_equals_the_edges_own_warm_start(amd, ctx, world, warm_every):
    a, b = injected(amd, ctx, world, ()), injected(amd, ctx, world, ())
    for x in (a, b):
        x._batch.set_images([world["nxt"]], next_frame=True)
    cnt_a = a._batch.warm_start(warm_every)
    cnt_b = b.warm_start_from(np.arange(B), warm_every)
    assert np.array_equal(cnt_a, cnt_b) and cnt_b.dtype == np.int32
    assert all(np.array_equal(p["obs"], o) for p, o in zip(b._ps, b._batch.read_obs_all()))  # (read back for reset())
    assert_same_state_and_trace(b, a, ("identity", warm_every))
    a._batch.close()
    b._batch.close()


def test_explicit_sources_and_none(amd, ctx, world):
    """Every edge from another edge of its grid (a rotation inside the 70-point and inside the 40-point edges), some from nothing."""
    from gaussian_process_edge_trace_amd.sequence import warm_start_obs
    dev, twin = injected(amd, ctx, world, ()), injected(amd, ctx, world, ())
    src = np.concatenate([np.roll(np.arange(N70), 7), N70 + np.roll(np.arange(N40), 3)]).astype(np.int32)
    src[[4, 20, 75]] = -1
    assert src[27] == 20 and src[57] == 50 and src[10] == 3  # (odd means go to other edges)
    for x in (dev, twin):
        x._batch.set_images([world["nxt"]], next_frame=True)
    cnt = dev.warm_start_from(src, 5)
    for e, p in enumerate(twin._ps):
        o = (np.zeros((0, 2), dtype=np.int64) if src[e] < 0 else
             warm_start_obs(trace_of_mean(world["means"][src[e]], p["x_st"]), p["x_st"], p["x_en"], 5, p["algo_thresh"], p["M"]))
        twin._batch.set_obs(e, o)
        assert cnt[e] == len(o), e
    assert cnt[4] == 0 and cnt[20] == 0 and cnt[10] >= 1
    assert_same_state_and_trace(dev, twin, "explicit")
    dev._batch.close()
    twin._batch.close()


def raw_ensemble(amd, b, group_of, tol, len_cap):
    L = amd._lib
    g, n_groups = L.check_group_table(group_of, b.B)
    raw = np.full(L.ensemble_layout(n_groups, b.B, len_cap)["total_bytes"], 0xA5, dtype=np.uint8)
    b.ctx.check(b.lib.gpet_batch_ensemble(b.h, n_groups, g.ctypes.data_as(C.POINTER(C.c_int32)), float(tol), len_cap, raw.ctypes.data, 0))
    return raw


def test_kept_ensemble_is_the_ensembles_bytes_and_lives_as_documented(amd, ctx, world):
    L = amd._lib
    b = injected(amd, ctx, world)
    lb = b._batch
    with pytest.raises(L.GpetError, match="no ensemble is kept") as ei:
        lb.ensemble_kept()
    assert ei.value.code == L.ERR_BAD_ARG
    want70, want96 = raw_ensemble(amd, lb, GROUPS, TOL, 70), raw_ensemble(amd, lb, GROUPS, TOL, 96)
    lb.ensemble_keep(GROUPS, TOL)
    got70, got96 = lb.ensemble_kept(raw=True), lb.ensemble_kept(len_cap=96, raw=True)
    assert got70.tobytes() == want70.tobytes() and got96.tobytes() == want96.tobytes()
    with pytest.raises(L.GpetError, match="len_cap"):
        lb.ensemble_kept(len_cap=69)
    # into device memory, both layouts
    for len_cap, want in ((70, want70), (96, want96)):
        d = C.c_void_p()
        ctx.check(ctx.lib.gpet_dev_alloc(ctx.h, want.nbytes, C.byref(d)))
        try:
            assert lb.ensemble_kept(len_cap=len_cap, device_ptr=d.value) is None
            raw = np.empty(want.nbytes, dtype=np.uint8)
            ctx.check(ctx.lib.gpet_dev_copy(ctx.h, raw.ctypes.data, d, want.nbytes, 1))
        finally:
            ctx.lib.gpet_dev_free(ctx.h, d)
        assert raw.tobytes() == want.tobytes(), len_cap
    # the decoded form is ensemble()'s
    dec, dec_want = lb.ensemble_kept(), lb.ensemble(GROUPS, TOL)
    for dg, dw in zip(dec[0], dec_want[0]):
        assert dg.keys() == dw.keys() and all(np.array_equal(np.asarray(dg[k]), np.asarray(dw[k])) for k in dg)
    assert dec[1].tobytes() == dec_want[1].tobytes() and np.array_equal(dec[2], dec_want[2])  # (edge 20's cost is NaN: bytes)
    # survives the swap of the images (the costs in it stay those of the old frame)
    lb.set_images([world["nxt"]], next_frame=True)
    assert lb.ensemble_kept(raw=True).tobytes() == want70.tobytes()
    # gone after a warm start of any kind
    lb.warm_start_groups("medoid", 5)
    with pytest.raises(L.GpetError, match="no ensemble is kept"):
        lb.ensemble_kept()
    b._batch.close()


def test_what_drops_the_kept_ensemble(amd, ctx, world, small_first):
    L = amd._lib
    b = small_batch(amd, ctx, world)
    g = np.array([0, 0, 0, 1, 1], dtype=np.int32)
    gone = lambda: pytest.raises(L.GpetError, match="no ensemble is kept")
    with pytest.raises(L.GpetError, match="no converged fit"):
        b._batch.ensemble_keep(g, TOL)  # (valid when gpet_batch_ensemble is)
    for drop in ("warm_start", "warm_start_from", "set_obs", "reset", "final_fit"):
        b.reset()
        assert_traces_old_frames(b, small_first)
        b._batch.ensemble_keep(g, TOL)
        assert len(b._batch.ensemble_kept()[0]) == 2
        if drop == "warm_start":
            b._batch.warm_start(5)
        elif drop == "warm_start_from":
            b._batch.warm_start_from([0, 1, 2, 3, 4], 5)
        elif drop == "set_obs":
            b._batch.set_obs(0, np.array([[10, 20]], dtype=np.int64))
        elif drop == "reset":
            b._batch.reset()
        else:
            b.finish(small_first[1])
        with gone():
            b._batch.ensemble_kept()
        if drop == "final_fit":
            b._batch.warm_start_ready()  # (the fits are there, the ensemble is not: only the group form refuses)
            with gone():
                b._batch.warm_start_groups("medoid", 5)
            assert b._batch.warm_start(5).shape == (5,)
    b._batch.close()


def test_refusals_leave_the_batch_on_its_old_frames(amd, ctx, world, small_first):
    L = amd._lib
    nxt = world["nxt"]
    g = np.array([0, 0, 0, 1, 1], dtype=np.int32)
    fresh = small_batch(amd, ctx, world)
    # no last trace: the readiness check refuses before the images are swapped
    with pytest.raises(L.GpetError, match="converged fits") as ei:
        fresh.set_frame(nxt, None, None, warm_every=5, warm_from="medoid", group_of=g)
    assert ei.value.code == L.ERR_BAD_ARG
    for call in (lambda: fresh._batch.warm_start_groups("medoid", 5), lambda: fresh._batch.warm_start_from([0, 1, 2, 3, 4], 5)):
        with pytest.raises(L.GpetError, match="converged fits"):
            call()
    assert_traces_old_frames(fresh, small_first)
    # the keywords
    with pytest.raises(ValueError, match="warm_every"):
        fresh.set_frame(nxt, None, None, warm_from="medoid", group_of=g)
    with pytest.raises(ValueError, match="alternatives"):
        fresh.set_frame(nxt, [np.zeros((0, 2))] * 5, None, warm_from="medoid", group_of=g)
    with pytest.raises(ValueError, match="warm_from"):
        fresh.set_frame(nxt, None, None, warm_every=5, warm_from="mean", group_of=g)
    with pytest.raises(ValueError, match="x-grids"):
        fresh.set_frame(nxt, None, None, warm_every=5, warm_from="medoid")  # (group_of=None: one group of all edges)
    # a table the reduction refuses: edges of different grids in one group -- refused by the keep, before the swap
    with pytest.raises(L.GpetError, match="different x-grids"):
        fresh.set_frame(nxt, None, None, warm_every=5, warm_from="medoid", group_of=np.array([0, 0, 0, 0, 1], dtype=np.int32))
    # the fits are there but no ensemble is kept; a bad policy; bad explicit tables, naming the edge
    with pytest.raises(L.GpetError, match="no ensemble is kept") as ei:
        fresh._batch.warm_start_groups("medoid", 5)
    assert ei.value.code == L.ERR_BAD_ARG
    fresh._batch.ensemble_keep(g, TOL)
    with pytest.raises(L.GpetError, match="from=7"):
        fresh._batch.ctx.check(fresh._batch.lib.gpet_batch_warm_start_groups(fresh._batch.h, 7, 5, None, None))
    with pytest.raises(L.GpetError, match=r"edge 2: src_of=5 is outside \[0, 5\)") as ei:
        fresh._batch.warm_start_from([0, 1, 5, 3, 4], 5)
    assert ei.value.code == L.ERR_BAD_ARG
    with pytest.raises(L.GpetError, match=r"edge 3 spans columns 5\.\.44, its source edge 1 spans 1\.\.70"):
        fresh._batch.warm_start_from([0, 1, 2, 1, 4], 5)
    with pytest.raises(ValueError):
        fresh._batch.warm_start_from([0, 1, 2], 5)
    # wrong images after a good keep: refused with the batch still on its old frames
    with pytest.raises(ValueError, match="do not fit"):
        fresh.set_frame([nxt, nxt], None, None, warm_every=5, warm_from="medoid", group_of=g)
    fresh.reset()
    assert_traces_old_frames(fresh, small_first)
    # and a call that is not refused: last_ensemble is what ensemble() returned for the frame left
    want = fresh.ensemble(g, TOL)
    assert fresh.last_ensemble is None  # (no refused call, the one for its images included, has kept an ensemble)
    fresh.set_frame(nxt, None, [3, 4, 5, 6, 7], warm_every=5, warm_from="best_cost", group_of=g, tol=TOL)
    assert len(fresh.last_ensemble) == 2
    for dg, dw in zip(fresh.last_ensemble, want):
        assert dg.keys() == dw.keys() and all(np.array_equal(np.asarray(dg[k]), np.asarray(dw[k])) for k in dg)
    assert all(np.array_equal(p["obs"], o) for p, o in zip(fresh._ps, fresh._batch.read_obs_all()))
    first = fresh()
    fresh.reset()  # (restores the same warm start)
    again = fresh()
    assert all(np.array_equal(a, w) for a, w in zip(first, again))
    fresh._batch.close()
