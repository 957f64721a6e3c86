"""GPU characterisation of the state rules of a batch (csrc/gpet_state_plan.h) as the C ABI shows them: which call is refused when,
with which code and message, what lifts the refusal and what brings it back.  Only refusals the library returns by design are provoked;
after each of them the batch goes on working, and at the end it traces, bit for bit, what a fresh batch traces.

One tiny batch: the 64 x 64 image and the RBF parameters of tests/test_gpu_edge_cases.py::test_error_codes_rank_cap_unsupported_nu_bad_state,
two edges, 128 samples."""
import numpy as np
import pytest

from oracle import gpet_oracle as orc

pytestmark = pytest.mark.gpu

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
SEEDS = [1, 2]
NOT_CONVERGED = "no converged fit of the current trace (run gpet_final_fit_all first)"
NO_LAST_FIT = "gpet_batch_warm_start: no converged fits of a last trace on the device"
NOT_KEPT = "gpet_batch_ensemble_kept: no ensemble is kept"


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def scene():
    img, truth = orc.synth_sinusoid_image(64, 4)
    grad = orc.comp_grad_img(img, orc.kernel_builder((11, 5)))
    return grad, truth[[0, -1], :][:, [1, 0]]


def tracer(amd, ctx, scene):
    grad, init = scene
    return amd.GP_Edge_Tracing_Batch([init, init], grad, SEEDS, **KW, _ctx=ctx)


@pytest.fixture(scope="module")
def fresh_trace(amd, ctx, scene):
    """What a batch that nothing else has happened to traces (computed once, left unchanged)."""
    t = tracer(amd, ctx, scene)
    out = [np.array(et) for et in t()]
    t._batch.close()
    return out


def refused(amd, call, code, text):
    with pytest.raises(amd._lib.GpetError) as ei:
        call()
    assert ei.value.code == code and text in str(ei.value), (ei.value.code, str(ei.value))


def assert_traces_like_a_fresh_batch(t, fresh_trace):
    t.reset()
    out = t()
    assert len(out) == len(fresh_trace)
    for et, want in zip(out, fresh_trace):
        assert np.array_equal(et, want)


def test_stage_order_settings_and_injections(amd, ctx, scene, fresh_trace):
    L = amd._lib
    t = tracer(amd, ctx, scene)
    b = t._batch
    no = lambda call, text: refused(amd, call, L.ERR_STATE, text)
    sample_needs = "gpet_gp_sample needs fit, factor and normals first"
    # a fresh batch: every stage that reads another stage's output refuses
    no(b.factor, "gpet_gp_factor before gpet_gp_fit_predict")
    no(b.sample, sample_needs)
    no(b.score, "gpet_score_curves before samples exist")
    no(b.curve_kde, "gpet_curve_kde before gpet_score_curves")
    no(b.select_pixels, "gpet_select_pixels before gpet_score_curves")
    no(b.select_pixels_loop, "gpet_select_pixels_loop before gpet_score_curves")
    # the stages; the sampler with the factor alone missing (the normals alone, the fit alone: below)
    b.fit_predict(True)
    b.normals([11, 12])
    no(b.sample, sample_needs)
    b.factor()
    b.sample()
    cov = [b.read(L.BUF_COV, e) for e in range(2)]
    factor = [b.read(L.BUF_FACTOR, e) for e in range(2)]
    normals = b.read(L.BUF_NORMALS, 0)
    # the generator changes (to what it was): the normals are gone until new ones exist -- here injected ones
    b.set_rng("mt19937")
    no(b.sample, sample_needs)
    b.write(L.BUF_NORMALS, normals, 0)
    b.sample()
    samples = b.read(L.BUF_SAMPLES, 0)
    b.score()
    best = b.read(L.BUF_BEST_IDX, 0)
    # the sample type changes (to what it was): the samples are gone until new ones exist -- here injected ones
    b.set_sample_dtype("f64")
    no(b.score, "gpet_score_curves before samples exist")
    b.write(L.BUF_SAMPLES, samples, 0)
    b.score()
    b.curve_kde()
    b.select_pixels_loop()
    # one iteration has run: the init points stay where they are
    moved = "iterations have run since the batch was created, reset or given new images"
    no(lambda: b.init_follow(2, 1), "gpet_batch_init_follow: 1 " + moved)
    no(lambda: b.set_init(t.inits), "gpet_batch_set_init: 1 " + moved)
    # new images: the outputs of all five stages are gone; injected ones stand in for them
    b.set_images([scene[0]])
    b.set_init(t.inits)
    no(b.factor, "gpet_gp_factor before gpet_gp_fit_predict")
    no(b.score, "gpet_score_curves before samples exist")
    no(b.curve_kde, "gpet_curve_kde before gpet_score_curves")
    b.normals([11, 12])
    for e in range(2):
        b.write(L.BUF_FACTOR, factor[e], e, rows=factor[e].shape[0])
    no(b.sample, sample_needs)  # (the fit alone is missing)
    for e in range(2):
        b.write(L.BUF_COV, cov[e], e)
    b.sample()
    b.factor()
    b.write(L.BUF_BEST_IDX, best, 0)
    b.curve_kde()
    for e in range(2):
        b.clear_injected_factor(e)
    assert_traces_like_a_fresh_batch(t, fresh_trace)
    b.close()


def test_converged_fit_warm_start_ensemble_and_init(amd, ctx, scene, fresh_trace):
    L = amd._lib
    t = tracer(amd, ctx, scene)
    b = t._batch
    bad = lambda call, text: refused(amd, call, L.ERR_BAD_ARG, text)
    bad(b.results, NOT_CONVERGED)
    bad(b.warm_start_ready, NO_LAST_FIT)
    bad(b.ensemble_kept, NOT_KEPT)
    bad(lambda: b.ensemble_keep([0, 0]), NOT_CONVERGED)
    for et, want in zip(t(), fresh_trace):
        assert np.array_equal(et, want)
    b.results()
    b.warm_start_ready()
    refused(amd, lambda: b.init_follow(2, 1), L.ERR_STATE, "gpet_batch_init_follow: ")
    refused(amd, lambda: b.set_init(t.inits), L.ERR_STATE, "gpet_batch_set_init: ")
    # another optimum in the optimiser's output: no result record, but the converged fits of the trace are still there
    centre = np.log([1.0, 1.0, 1e-2])
    b.final_optimize(np.tile(centre, (2, 1, 1)), np.stack([centre - 3.0, centre + 3.0], axis=1))
    bad(b.results, NOT_CONVERGED)
    b.warm_start_ready()
    # a traced and fitted batch with a kept ensemble, then the next frame's images: the fits and the ensemble outlive the swap
    t.reset()
    t()
    b.ensemble_keep([0, 0])
    b.ensemble_kept()
    b.set_images([scene[0]], next_frame=True)
    b.warm_start_ready()
    b.ensemble_kept()
    bad(b.results, NOT_CONVERGED)
    # a reset drops the ensemble, not the fits; and the init points may move again
    b.reset()
    bad(b.ensemble_kept, NOT_KEPT)
    b.warm_start_ready()
    b.init_follow(2, 1)
    b.set_init(t.inits)
    # a caller's observation set: another trace, whose fits those are not
    t()
    b.results()
    b.set_obs(0, np.array([[20, 40]], dtype=np.int64))
    bad(b.results, NOT_CONVERGED)
    bad(b.warm_start_ready, NO_LAST_FIT)
    assert_traces_like_a_fresh_batch(t, fresh_trace)
    b.close()
