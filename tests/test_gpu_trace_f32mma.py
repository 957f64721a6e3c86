"""sample_dtype="f32mma" (the sample GEMM on the f32 matrix cores, gpet_batch_set_sample_arith) on real data and whole traces:
the golden scenes trace_rbf64 (rank <= 96: the register form k_sample_f32_r) and trace_mat128 (full rank: the generic form
k_sample_f32).

The oracle has no such mode.  What is checked instead: the device's samples against the mode's definition (tests/f32_chain.py)
evaluated on the device's OWN factor, normals and mean, bit for bit; the rest of an iteration -- the existing scorer, KDE and
pixel selection on f32 samples -- against the oracle's public functions applied to the device's own sample matrix; and the
plumbing: device loop, batch, history and trace_sequence against the stepwise single-edge run."""
import numpy as np
import pytest

from oracle import gpet_oracle as orc
from tests.f32_chain import chain

pytestmark = pytest.mark.gpu

# (the constructor arguments of tests/test_gpu_trace.py for these two scenes, restated)
SCENES = {
    "trace_rbf64": ("stage_rbf64", dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128,
                                        score_thresh=1, delta_x=5, keep_ratio=0.1, pixel_thresh=3, seed=1, fix_endpoints=True)),
    "trace_mat128": ("stage_mat128", dict(kernel_options=(1, 3, 3), noise_y=0.5, N_samples=256, score_thresh=0.9, delta_x=8,
                                          keep_ratio=0.125, pixel_thresh=4, seed=7, fix_endpoints=False)),
}
NAMES = list(SCENES)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def stepwise(amd, ctx, golden):
    """name, seed -> the stepwise run (one device iteration per call, everything read back): computed once, shared."""
    cache = {}

    def run(name, seed=None):
        stage, kw = SCENES[name]
        kw = dict(kw, seed=kw["seed"] if seed is None else seed)
        if (name, kw["seed"]) not in cache:
            init, grad = golden(name)["in_init"], golden(stage)["ref_grad"]
            tr = amd.GP_Edge_Tracing(init, grad, **kw, sample_dtype="f32mma", _ctx=ctx)
            et, (all_samples, all_obs, curves) = tr(return_lines=True)
            cache[name, kw["seed"]] = dict(tr=tr, et=et, samples=all_samples, obs=all_obs, n_iter=tr._n_iter, init=init, grad=grad, kw=kw)
        return cache[name, kw["seed"]]
    return run


def stage_samples(L, b, obs, seed):
    """One iteration through the stage API; the sample matrix and the GEMM's inputs as the device holds them."""
    b.set_obs(0, obs)
    b.fit_predict(want_cov=True)
    b.factor()
    b.normals([seed])
    b.sample()
    s = b.scalars()
    return dict(Y=b.read(L.BUF_SAMPLES), A=b.read(L.BUF_FACTOR), Z=b.read(L.BUF_NORMALS), mean=b.read(L.BUF_MEAN), rank=int(s.rank),
                y_s=float(s.y_s))


@pytest.mark.parametrize("name", NAMES)
def test_device_samples_equal_the_chain_on_the_device_s_own_inputs(amd, ctx, stepwise, name):
    """First and last iteration of the trace: set_obs with that iteration's input set, fit_predict, factor, normals, sample;
    BUF_SAMPLES equals float32((float64(chain(Z[:, :rank], factor)) + mean) * y_s) bit for bit.  The device's own Jacobi factor
    is the input, so LAPACK's differences do not enter.  The samples are f32-representable."""
    L = amd._lib
    run = stepwise(name)
    assert run["n_iter"] >= 2
    seen = set()
    for i in (0, run["n_iter"] - 1):
        d = stage_samples(L, run["tr"]._batch, run["obs"][i], run["kw"]["seed"] + i + 1)
        r = d["rank"]
        assert d["A"].shape == (r, d["mean"].shape[0]) and d["Z"].shape[1] >= r >= 1
        exp = ((chain(d["Z"][:, :r], d["A"]).astype(np.float64) + d["mean"]) * d["y_s"]).astype(np.float32).astype(np.float64)
        Y = d["Y"]
        assert Y.dtype == np.float64 and Y.shape == exp.shape and np.array_equal(Y, Y.astype(np.float32).astype(np.float64))
        bad = np.argwhere(Y != exp)
        assert bad.size == 0, (name, i, r, len(bad), [(int(a), int(c), Y[a, c], exp[a, c]) for a, c in bad[:8]])
        seen.add(r)
    info = run["tr"]._batch.info()
    print("%s: ranks %s, capacities %d / %d" % (name, sorted(seen), info["factor_cap"], info["factor_rows_cap"]))
    # (launch_sample_f32: capacities of at most 96 take the register form, larger ones the generic form)
    assert (max(info["factor_cap"], info["factor_rows_cap"]) <= 96) == (name == "trace_rbf64")


@pytest.mark.parametrize("name", NAMES)
def test_rest_of_the_iteration_is_the_existing_code(amd, ctx, stepwise, name):
    """For every iteration of the stepwise run: the oracle's get_best_curves and get_best_pixels (with kde_of_gradient, and the
    state dict as oracle.trace builds it) applied to the device's OWN returned sample matrix reproduce the device's next
    observation set."""
    run = stepwise(name)
    p = orc.resolve_params(run["init"], run["grad"], **run["kw"])
    grad64 = orc.normalise(run["grad"], (0, 1), np.float64)
    grad_kde = orc.kde_of_gradient(grad64)
    state = dict(score_thresh=p["score_thresh"], pixel_thresh=p["pixel_thresh"], algo_thresh=p["algo_thresh"], x_st=p["x_st"],
                 delta_x=p["delta_x"])
    assert len(run["samples"]) == run["n_iter"] + 1 and len(run["obs"]) == run["n_iter"] + 2
    for i in range(run["n_iter"]):
        pre = p["obs"] if i == 0 else run["obs"][i]
        bc, bcost, bidx, costs = orc.get_best_curves(grad64, p["x_grid"], run["samples"][i], p["N_keep"])
        new, _ = orc.get_best_pixels(bc, bcost, pre[:, [1, 0]], grad_kde, p["M"], p["N"], state, p["fix_endpoints"], p["x_st"], p["x_en"])
        assert np.array_equal(new, run["obs"][i + 1]), (name, "iteration %d" % i)


@pytest.mark.parametrize("name", NAMES)
def test_device_loop_and_batch_equal_the_stepwise_run(amd, ctx, stepwise, name):
    run = stepwise(name)
    loop = amd.GP_Edge_Tracing(run["init"], run["grad"], **run["kw"], sample_dtype="f32mma", _ctx=ctx)
    assert np.array_equal(loop(), run["et"]) and loop._n_iter == run["n_iter"]
    seeds = [run["kw"]["seed"] + k for k in range(3)]
    kw = {k: v for k, v in run["kw"].items() if k != "seed"}
    batch = amd.GP_Edge_Tracing_Batch([run["init"]] * 3, run["grad"], seeds, **kw, sample_dtype="f32mma", _ctx=ctx)
    out = batch()
    for k, seed in enumerate(seeds):
        one = stepwise(name, seed)
        assert np.array_equal(out[k], one["et"]), (name, seed)
        assert batch.timings["iters"][k] == one["n_iter"], (name, seed)
    batch._batch.close()


@pytest.mark.parametrize("name", NAMES)
def test_history_curve_is_the_best_row_of_the_sample_matrix(amd, ctx, stepwise, name):
    run = stepwise(name)
    tr = amd.GP_Edge_Tracing(run["init"], run["grad"], **run["kw"], sample_dtype="f32mma", history="curves", _ctx=ctx)
    assert np.array_equal(tr(), run["et"])
    h = tr.history()
    assert h["n_iter"] == run["n_iter"] and h["dropped"] == 0
    for i in range(run["n_iter"]):
        assert np.array_equal(h["obs"][i], run["obs"][i + 1])
        assert np.array_equal(h["optimal_curves"][i][:, 1], run["samples"][i][:, h["best_idx"][i]]), (name, i)


def test_trace_sequence_forwards_the_mode(amd, ctx):
    """trace_sequence(..., sample_dtype="f32mma") on four 64-wide frames in two chains equals four chained single-edge runs
    in the same mode (and is not the f32-storage sequence, if the two modes part anywhere on these frames: printed)."""
    from gaussian_process_edge_trace_amd.gpet import resolve_params
    from gaussian_process_edge_trace_amd.sequence import chain_slices, warm_start_obs
    N, T = 64, 4
    frames, init = [], None
    for t in range(T):
        img, truth = orc.synth_sinusoid_image(N, 11 + t, amplitude=int(0.4 * N * (1.0 + 0.02 * t)))
        frames.append(amd.gpet_utils.comp_grad_img(img, amd.gpet_utils.kernel_builder((11, 5)), ctx=ctx))
        init = truth[[0, -1], :][:, [1, 0]] if init is None else init
    kw = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
              keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
    got = amd.trace_sequence(frames, init, n_chains=2, warm_every=10, seed=5, sample_dtype="f32mma", _ctx=ctx, **kw)
    p = resolve_params(init, frames[0].shape, **kw)
    for lo, hi in chain_slices(T, 2):
        prev = None
        for t in range(lo, hi):
            obs = np.array([]) if prev is None else warm_start_obs(prev, p["x_st"], p["x_en"], 10, p["algo_thresh"], p["M"])
            tr = amd.GP_Edge_Tracing(init, frames[t], obs=obs, seed=5, **kw, sample_dtype="f32mma", _ctx=ctx)
            prev = tr()
            assert tr._n_iter >= 1
            assert np.array_equal(got[t], prev), "frame %d" % t
    other = amd.trace_sequence(frames, init, n_chains=2, warm_every=10, seed=5, sample_dtype="f32", _ctx=ctx, **kw)
    print("f32mma sequence %s the f32 sequence" % ("equals" if all(np.array_equal(a, b) for a, b in zip(got, other)) else "differs from"))


def test_a_different_name_alone_is_not_a_mode(amd, ctx, stepwise):
    """trace_rbf64, first iteration: the "f32mma" sample matrix differs from the "f32" one (same observations, same normals)."""
    L = amd._lib
    run = stepwise("trace_rbf64")
    seed = run["kw"]["seed"] + 1
    mma = stage_samples(L, run["tr"]._batch, run["obs"][0], seed)
    tr32 = amd.GP_Edge_Tracing(run["init"], run["grad"], **run["kw"], sample_dtype="f32", _ctx=ctx)
    f32 = stage_samples(L, tr32._batch, run["obs"][0], seed)
    assert np.array_equal(mma["Z"], f32["Z"])
    exp32 = ((f32["Z"][:, :f32["rank"]] @ f32["A"] + f32["mean"]) * f32["y_s"]).astype(np.float32)
    share = float(np.mean(mma["Y"] != f32["Y"]))
    print("trace_rbf64, iteration 0: %.3f of the f32mma samples differ from the f32 ones (numpy's f32 value differs from the "
          "device's f32 in %.4f: summation order in f64)" % (share, float(np.mean(exp32 != f32["Y"]))))
    assert share > 0
