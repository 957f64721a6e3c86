"""GPU tests of the iteration history kept on the device (include/gpet_hip.h, "iteration history"; csrc/gpet_k_history.inc):
a four-edge batch against single stepwise traces and the CPU oracle's own per-iteration record, the column statistics against
extended precision inside a derived bound, injected inputs whose statistics are exact, and the lifetime / cap / opt-in rules.

Scene: a 96 x 96 synthetic sinusoid edge, S = 130 samples (no power-of-two chunk of rows divides it), four edges on the true
edge's rows with grid lengths 88, 96, 23 and 37 -- odd and sub-wave lengths, lengths above 64 that are no multiple of 16 or 64 --
of which two finish inside the loop's first group of eight iterations and two run on into the compacted groups after it."""
import numpy as np
import pytest

from oracle import gpet_oracle as orc

pytestmark = pytest.mark.gpu

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 15, 'length_scale': 12}, noise_y=1, N_samples=130, score_thresh=1, delta_x=2,
          keep_ratio=0.1, pixel_thresh=2)
EDGES = [(3, 90, 2), (0, 95, 1), (30, 52, 6), (20, 56, 3)]  # (x_st, x_en, seed)
S = 130
U = 2.0 ** -53


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def scene():
    img, edge = orc.synth_sinusoid_image(96, seed=1)
    grad = orc.comp_grad_img(img, orc.kernel_builder((5, 3)))
    inits = [edge[[a, b]][:, [1, 0]] for a, b, _ in EDGES]
    return dict(grad=grad, inits=inits, seeds=[s for _, _, s in EDGES])


@pytest.fixture(scope="module")
def oracle_recs(scene):
    """The oracle's per-iteration record of every edge (library sign convention), f64 samples and -- first and last edge -- f32."""
    out = {}
    for e, init in enumerate(scene["inits"]):
        for sd in ((None, "f32") if e in (0, 3) else (None,)):
            rec = []
            _, _, info = orc.trace(init, scene["grad"], record=rec, sign_convention="harmonic", sample_dtype=sd, seed=scene["seeds"][e], **KW)
            assert info["n_iter"] == len(rec)
            out[(e, sd)] = rec
    n = [len(out[(e, None)]) for e in range(4)]
    # the precondition the shapes were chosen for, from the oracle's own record: edges that finish inside the first group of eight
    # iterations beside edges that run into the compacted groups after it
    assert min(n) < 8 < max(n), n
    return out


@pytest.fixture(scope="module")
def singles(amd, ctx, scene):
    """Every edge alone through the stepwise path of __call__(return_lines=True): trace, samples, observation sets, curves, costs."""
    out = []
    for e, init in enumerate(scene["inits"]):
        tr = amd.GP_Edge_Tracing(init, scene["grad"], **KW, seed=scene["seeds"][e], _ctx=ctx)
        et, (all_samples, all_obs, curves) = tr(return_lines=True)
        out.append(dict(et=et, samples=all_samples[:-1], obs=all_obs, curves=curves[:-1], costs=list(tr.iter_optimal_costs),
                        n_iter=tr._n_iter, x_grid=tr.x_grid))
    return out


def _batch(amd, ctx, scene, **kw):
    return amd.GP_Edge_Tracing_Batch(scene["inits"], scene["grad"], scene["seeds"], **KW, return_std=True, _ctx=ctx, **kw)


def _run(batch):
    out = batch()
    return dict(out=out, iters=list(batch.timings["iters"]), obs=batch._batch.read_obs_all())


@pytest.fixture(scope="module")
def full(amd, ctx, scene):
    b = _batch(amd, ctx, scene, history="full")
    r = _run(b)
    r["hist"] = b.history()
    return r


def test_batch_history_equals_single_traces_and_the_oracle(full, singles, oracle_recs, scene):
    grad64 = orc.normalise(scene["grad"], (0, 1), np.float64)
    for e in range(4):
        h, one, rec = full["hist"][e], singles[e], oracle_recs[(e, None)]
        assert h["n_iter"] == one["n_iter"] == full["iters"][e] == len(rec) and h["dropped"] == 0
        assert len(h["obs"]) == len(h["optimal_curves"]) == h["n_iter"]
        for i, r in enumerate(rec):
            assert np.array_equal(h["obs"][i], r["obs_out"]) and h["obs"][i].dtype == np.int64, (e, i)
            assert h["score_thresh"][i] == r["score_thresh"], (e, i)
            assert h["best_idx"][i] == r["best_idxs"][0], (e, i)
            assert h["n_obs"][i] == r["obs_out"].shape[0]
            # against the oracle's own trace: the tolerance tests/test_gpu_trace.py compares the device's floats of a whole trace
            # with (the samples behind the cost are the device's, equal to the oracle's to rounding only) ...
            want = r["costs"][r["best_idxs"][0]]
            print("edge %d iteration %d: optimal cost %.17g, oracle %.17g, rel %.2e" % (e, i, h["optimal_cost"][i], want, abs(h["optimal_cost"][i] / want - 1)))
            np.testing.assert_allclose(h["optimal_cost"][i], want, rtol=1e-6, atol=1e-6)
            # ... and the oracle's scorer on the RECORDED curve, to the suite's tolerance for costs of equal samples
            oc = orc.costs_batch(grad64, one["x_grid"], h["optimal_curves"][i][:, 1:2])
            np.testing.assert_allclose(h["optimal_cost"][i], oc[0], rtol=1e-9)
            # the stepwise single trace: bit for bit
            assert np.array_equal(h["obs"][i], one["obs"][i + 1]), (e, i)
            assert np.array_equal(h["optimal_curves"][i], one["curves"][i]), (e, i)
            assert h["optimal_cost"][i] == one["costs"][i], (e, i)
        assert np.array_equal(full["out"][e][0], one["et"])


def test_column_statistics_inside_the_summation_bound(full, singles):
    """mean / std of all S samples per column against extended precision.  The bound is the worst case of recursive summation
    (any order): |mean - ref| <= 2 S u max|y|, |std - ref| <= 2 S u max(1, max|y|), u = 2^-53, max over the column."""
    worst = [0.0, 0.0]
    for e in range(4):
        h = full["hist"][e]
        assert h["mean"].shape == h["std"].shape == (h["n_iter"], len(singles[e]["x_grid"]))
        for i, Y in enumerate(singles[e]["samples"]):  # (Lg, S)
            assert Y.shape[1] == S
            yl = Y.astype(np.longdouble)
            m_ref, s_ref = np.mean(yl, axis=1), np.std(yl, axis=1)
            amax = np.abs(Y).max(axis=1)
            b_mean, b_std = 2 * S * U * amax, 2 * S * U * np.maximum(1.0, amax)
            d_mean, d_std = np.abs(h["mean"][i] - m_ref), np.abs(h["std"][i] - s_ref)
            worst = [max(worst[0], float((d_mean / b_mean).max())), max(worst[1], float((d_std / b_std).max()))]
            assert (d_mean <= b_mean).all() and (d_std <= b_std).all(), (e, i, float((d_mean / b_mean).max()), float((d_std / b_std).max()))
            # the reference alone is inside it: float64 numpy meets the same bound
            assert (np.abs(np.mean(Y, axis=1) - m_ref) <= b_mean).all() and (np.abs(np.std(Y, axis=1) - s_ref) <= b_std).all()
    print("largest excess over the bound: mean %.3f, std %.3f of it" % tuple(worst))


@pytest.mark.parametrize("sample_dtype", [None, "f32"])
def test_injected_inputs_are_recorded_exactly(amd, ctx, scene, sample_dtype):
    """gpet_history_record on a sample matrix whose rows alternate m_j + v_j and m_j - v_j (small integers, v_j = 0 in some
    columns): mean m_j and std |v_j| exactly, the curve = the last row, observations, cost and scalars as written."""
    L = amd._lib
    tr = amd.GP_Edge_Tracing(scene["inits"][2], scene["grad"], **KW, seed=6, history="full", history_cap=4, sample_dtype=sample_dtype, _ctx=ctx)
    b = tr._batch
    inf = b.info()
    Lg, cap = inf["Lg"], inf["obs_cap"]
    assert (Lg, inf["S"]) == (23, S)
    j = np.arange(Lg)
    m = (j * 7) % 41 + 3.0
    v = np.where(j % 3 == 0, 0.0, (j % 5) - 2.0)  # zeros, and both signs
    v[1] = 6.0
    assert (v == 0).sum() >= 5 and (v < 0).any()
    Y = m[None, :] + np.where(np.arange(S)[:, None] % 2 == 0, 1.0, -1.0) * v[None, :]
    obs = np.stack((np.arange(cap) % 96, (np.arange(cap) * 5 + 1) % 96), -1).astype(np.int64)
    b.set_obs(0, obs)  # obs_cap entries (and an empty history)
    b.write(L.BUF_SAMPLES, Y)
    idx = np.arange(inf["n_keep"], dtype=np.int32)
    idx[0] = S - 1  # the last row
    b.write(L.BUF_BEST_IDX, idx)
    costs = np.linspace(0.8125, 2.0, inf["n_keep"])
    b.write(L.BUF_BEST_COSTS, costs)
    assert tr.history()["n_iter"] == 0
    for it, thresh in ((1, 0.7), (3, 0.5)):
        sc = b.scalars()
        sc.iter, sc.score_thresh, sc.rank, sc.n_removed, sc.y_s = it, thresh, 5 + it, 2, 3.5
        b.write_scalars(sc)
        b.history_record()
    h = tr.history()
    assert (h["n_iter"], h["dropped"]) == (3, 0)
    for i, thresh in ((0, 0.7), (2, 0.5)):
        assert np.array_equal(h["mean"][i], m) and np.array_equal(h["std"][i], np.abs(v))
        assert np.array_equal(h["optimal_curves"][i][:, 1], Y[S - 1]) and np.array_equal(h["optimal_curves"][i][:, 0], tr.x_grid)
        assert np.array_equal(h["obs"][i], obs) and h["optimal_cost"][i] == costs[0] and h["best_idx"][i] == S - 1
        assert (h["score_thresh"][i], h["rank"][i], h["n_removed"][i], h["y_s"][i], h["n_obs"][i]) == (thresh, 6 + i, 2, 3.5, cap)
    # the slot nobody recorded is untouched: zero
    assert h["n_obs"][1] == 0 and not h["mean"][1].any() and not h["optimal_curves"][1][:, 1].any() and h["obs"][1].shape == (0, 2)
    # past the cap: dropped and counted, the records stay
    sc = b.scalars()
    sc.iter = 6
    b.write_scalars(sc)
    b.history_record()
    h2 = tr.history()
    assert (h2["n_iter"], h2["dropped"]) == (3, 2) and np.array_equal(h2["mean"], h["mean"]) and np.array_equal(h2["std"], h["std"])


def test_history_changes_nothing(amd, ctx, scene, full):
    plain = _run(_batch(amd, ctx, scene))
    assert plain["iters"] == full["iters"]
    for e in range(4):
        assert np.array_equal(plain["out"][e][0], full["out"][e][0])
        assert np.array_equal(plain["out"][e][1][0], full["out"][e][1][0]) and np.array_equal(plain["out"][e][1][1], full["out"][e][1][1])
        assert np.array_equal(plain["obs"][e], full["obs"][e])


def test_records_past_the_cap_are_dropped_and_counted(amd, ctx, scene, full):
    b = _batch(amd, ctx, scene, history="full", history_cap=3)
    r = _run(b)
    hist = b.history()
    for e in range(4):
        h, f = hist[e], full["hist"][e]
        assert h["n_iter"] == 3 and h["dropped"] == full["iters"][e] - 3
        for k in ("score_thresh", "optimal_cost", "best_idx", "rank", "n_obs", "mean", "std"):
            assert np.array_equal(h[k], f[k][:3]), (e, k)
        for i in range(3):
            assert np.array_equal(h["obs"][i], f["obs"][i]) and np.array_equal(h["optimal_curves"][i], f["optimal_curves"][i])
        assert np.array_equal(r["out"][e][0], full["out"][e][0]) and np.array_equal(r["obs"][e], full["obs"][e])
    assert r["iters"] == full["iters"]


def _same_history(a, b):
    assert [h["n_iter"] for h in a] == [h["n_iter"] for h in b] and [h["dropped"] for h in a] == [h["dropped"] for h in b]
    for ha, hb in zip(a, b):
        assert set(ha) == set(hb)
        for i in range(ha["n_iter"]):
            assert np.array_equal(ha["obs"][i], hb["obs"][i])
            if "optimal_curves" in ha:
                assert np.array_equal(ha["optimal_curves"][i], hb["optimal_curves"][i])
        assert np.array_equal(ha["score_thresh"], hb["score_thresh"]) and np.array_equal(ha["optimal_cost"], hb["optimal_cost"])


def test_lifetime_and_levels(amd, ctx, scene, full):
    b = _batch(amd, ctx, scene, history="curves")
    b()
    once = b.history()
    assert [h["n_iter"] for h in once] == full["iters"]
    for h, f in zip(once, full["hist"]):  # 'curves' records what 'full' records, without the statistics
        assert "mean" not in h and "std" not in h and len(h["optimal_curves"]) == h["n_iter"]
        for i in range(h["n_iter"]):
            assert np.array_equal(h["optimal_curves"][i], f["optimal_curves"][i]) and np.array_equal(h["obs"][i], f["obs"][i])
    b.reset()
    assert [h["n_iter"] for h in b.history()] == [0, 0, 0, 0]
    b()
    _same_history(b.history(), once)  # the same history, not a doubled one
    b.set_frame(scene["grad"])
    empty = b.history()
    assert [(h["n_iter"], h["dropped"], len(h["obs"])) for h in empty] == [(0, 0, 0)] * 4
    o = _batch(amd, ctx, scene, history="obs")
    o.run_loop()
    for h, f in zip(o.history(), full["hist"]):
        assert "optimal_curves" not in h and "mean" not in h and "std" not in h
        assert h["n_iter"] == f["n_iter"] and all(np.array_equal(x, y) for x, y in zip(h["obs"], f["obs"]))
        assert np.array_equal(h["optimal_cost"], f["optimal_cost"])
    off = _batch(amd, ctx, scene)
    with pytest.raises(amd._lib.GpetError) as ei:
        off.history()
    assert ei.value.code == amd._lib.ERR_STATE
    with pytest.raises(amd._lib.GpetError) as ei:
        off._batch.history_record()
    assert ei.value.code == amd._lib.ERR_STATE
    with pytest.raises(amd._lib.GpetError) as ei:
        off._batch.set_history("obs", 0)
    assert ei.value.code == amd._lib.ERR_BAD_ARG
    assert off._batch.lib.gpet_batch_set_history(off._batch.h, 4, 8) == amd._lib.ERR_BAD_ARG
    # switched on later, and off again
    off._batch.set_history("obs", 8)
    assert off.history()[0]["n_iter"] == 0
    off._batch.set_history(None)
    with pytest.raises(amd._lib.GpetError):
        off.history()


def test_single_tracer_history_without_a_wait_per_iteration(amd, ctx, scene, full):
    """GP_Edge_Tracing(history=...) runs its loop in whole groups and returns the history of its one edge."""
    e = 3
    tr = amd.GP_Edge_Tracing(scene["inits"][e], scene["grad"], **KW, seed=scene["seeds"][e], history="full", _ctx=ctx)
    et = tr()
    assert np.array_equal(et, full["out"][e][0])
    _same_history([tr.history()], [full["hist"][e]])
    assert np.array_equal(tr.history()["mean"], full["hist"][e]["mean"]) and np.array_equal(tr.history()["std"], full["hist"][e]["std"])
    plain = amd.GP_Edge_Tracing(scene["inits"][e], scene["grad"], **KW, seed=scene["seeds"][e], _ctx=ctx)
    with pytest.raises(amd._lib.GpetError):
        plain.history()


def test_f32_samples_mode(amd, ctx, scene, oracle_recs):
    """sample_dtype="f32": the history of the first and last edge against the oracle's f32 record; the curve is the f32 sample
    row widened."""
    sel = [0, 3]
    b = amd.GP_Edge_Tracing_Batch([scene["inits"][e] for e in sel], scene["grad"], [scene["seeds"][e] for e in sel], **KW,
                                  sample_dtype="f32", history="curves", _ctx=ctx)
    b.run_loop()
    hist = b.history()
    for k, e in enumerate(sel):
        h, rec = hist[k], oracle_recs[(e, "f32")]
        assert h["n_iter"] == len(rec) and h["dropped"] == 0
        one = amd.GP_Edge_Tracing(scene["inits"][e], scene["grad"], **KW, seed=scene["seeds"][e], sample_dtype="f32", _ctx=ctx)
        _, (all_samples, all_obs, curves) = one(return_lines=True)
        for i, r in enumerate(rec):
            assert np.array_equal(h["obs"][i], r["obs_out"]) and h["score_thresh"][i] == r["score_thresh"]
            assert h["best_idx"][i] == r["best_idxs"][0]
            y = h["optimal_curves"][i][:, 1]
            assert np.array_equal(y, y.astype(np.float32).astype(np.float64))
            assert np.array_equal(y, all_samples[i][:, h["best_idx"][i]]) and np.array_equal(h["optimal_curves"][i], curves[i])
