"""GPU tests of the denoising stage in front of the gradient-image convolution: gpet_utils.denoise / denoise_imgs
(gpet_denoise_images), comp_grad_imgs(denoise=) (gpet_grad_images_dn), GP_Edge_Tracing_Batch(raw_imgs=, denoise=) and
set_frame(denoise=) (gpet_batch_create_raw_dn, gpet_batch_set_raw_images_dn), SequenceTracer(grad_kernel=, denoise=).

The reference is tests/golden/denoise.npz, written by the unmodified reference under scipy 1.7.1 / scikit-image 0.18.3; where an
input is not in it (seeded stacks), tests/denoise_ref.py stands in, which tests/test_denoise_fixture.py pins to the fixture bit for
bit.  Everything is np.array_equal with one documented exception: 'gaussian' of float64 frames.  scipy forms the Gaussian taps with
numpy.exp, whose vectorised forms differ from the C library's exp (which the device library's host code calls) by one unit in the
last place for some arguments, depending on numpy's version and the CPU.  There the device result must equal the
restatement with the C library's exponential bit for bit, and lie within 16 x the fixture's `exp_spread` of the reference's
image -- the largest change the restatement shows on the same input when one exponential of the taps moves by one unit in the
last place, computed by the fixture's generator.  Compositions (denoise inside a larger device pass against denoise_imgs first) are
exact by construction."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import gpet_oracle as orc
from tests import denoise_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "denoise.npz"))
CASES = json.loads(str(FIX["cases"]))
BIG = json.loads(str(FIX["big"]))
DT = dict(u8=np.uint8, u16=np.uint16, f32=np.float32, f64=np.float64)
SPECS = [("median", dict(size=3)), ("median", dict(size=5)), ("median", dict(size=[4, 3], mode="nearest")), ("minimum", dict(size=[7, 1])),
         ("median", dict(size=9)), ("gaussian", dict(sigma=1.5)), ("gaussian", dict(sigma=[2.0, 0.7], mode="nearest")),
         ("tvc", dict(weight=0.1))]
SPEC_IDS = ["median3", "median5", "median4x3", "minimum7x1", "median9", "gauss1.5", "gauss_pair", "tvc"]


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def by_technique(*techniques):
    sel = [c for c in CASES if c["technique"] in techniques]
    return dict(argvalues=sel, ids=[c["name"] for c in sel])


class DeviceFrames(object):
    """Frames copied into device memory of the context (gpet_dev_alloc / gpet_dev_copy); ``ptrs`` are their addresses."""

    def __init__(self, ctx, frames):
        self.ctx, self.frames, self.ptrs = ctx, [np.ascontiguousarray(f) for f in frames], []
        for f in self.frames:
            d = C.c_void_p()
            ctx.check(ctx.lib.gpet_dev_alloc(ctx.h, f.nbytes, C.byref(d)))
            ctx.check(ctx.lib.gpet_dev_copy(ctx.h, d, f.ctypes.data, f.nbytes, 0))
            self.ptrs.append(d.value)

    def download(self, i):
        out = np.empty_like(self.frames[i])
        self.ctx.check(self.ctx.lib.gpet_dev_copy(self.ctx.h, out.ctypes.data, C.c_void_p(self.ptrs[i]), out.nbytes, 1))
        return out

    def free(self):
        for p in self.ptrs:
            self.ctx.lib.gpet_dev_free(self.ctx.h, C.c_void_p(p))
        self.ptrs = []


# ---- against the fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", **by_technique("median", "minimum"))
def test_rank_filters_equal_the_reference(amd, ctx, case):
    img, exp = FIX["in_" + case["input"]], FIX["exp_" + case["name"]]
    out = amd.gpet_utils.denoise(img, case["technique"], case["kwargs"], ctx=ctx)
    assert out.dtype == exp.dtype == img.dtype and out.shape == exp.shape
    assert np.array_equal(out, exp)


@pytest.mark.parametrize("case", **by_technique("gaussian"))
def test_gaussian_equals_the_reference(amd, ctx, case):
    img, exp, kw = FIX["in_" + case["input"]], FIX["exp_" + case["name"]], case["kwargs"]
    out = amd.gpet_utils.denoise(img, "gaussian", kw, ctx=ctx)
    assert out.dtype == exp.dtype == img.dtype and out.shape == exp.shape
    if img.dtype != np.float64:
        assert np.array_equal(out, exp)
        return
    own = R.denoise(img, "gaussian", kw)  # every operation the reference's, the exponential the C library's
    diff = float(np.abs(out - exp).max())
    print("%s: max |device - reference| = %.3g, 16 x exp_spread = %.3g, device == restatement: %s"
          % (case["name"], diff, 16 * case["exp_spread"], np.array_equal(out, own)))
    assert np.array_equal(out, own)
    assert case["exp_spread"] > 0 and diff <= 16 * case["exp_spread"]


@pytest.mark.parametrize("case", **by_technique("tvc"))
def test_tvc_equals_the_reference_with_its_iteration_count(amd, ctx, case):
    """(for the float32 frame the expected image is the reference's on frame.astype(float64): the device iterates in float64)"""
    img, exp = FIX["in_" + case["input"]], FIX["exp_" + case["name"]]
    out, n_iter = amd.gpet_utils.denoise_imgs([img], "tvc", case["kwargs"], ctx=ctx, return_n_iter=True)
    assert out.dtype == np.float64 and out.shape == (1,) + exp.shape
    assert int(n_iter[0]) == case["n_iter"]
    assert np.array_equal(out[0], exp)
    assert np.array_equal(amd.gpet_utils.denoise(img, "tvc", case["kwargs"], ctx=ctx), exp)


@pytest.mark.parametrize("rec", BIG, ids=[b["technique"] for b in BIG])
def test_500x500_cases(amd, ctx, rec):
    img = R.make_frame(rec["seed"], 500, 500, rec["noise"], DT[rec["pix"]])
    out, n_iter = amd.gpet_utils.denoise_imgs([img], rec["technique"], rec["kwargs"], ctx=ctx, return_n_iter=True)
    assert str(out.dtype) == rec["dtype"] and int(n_iter[0]) == rec.get("n_iter", 0)
    assert hashlib.sha256(np.ascontiguousarray(out[0]).tobytes()).hexdigest() == rec["sha256"]


def test_plot_and_verbose_are_ignored_with_a_warning(amd, ctx):
    img = FIX["in_rank_u8"]
    with pytest.warns(UserWarning, match="ignored"):
        out = amd.gpet_utils.denoise(img, "median", dict(size=3), plot=True, verbose=True, ctx=ctx)
    assert np.array_equal(out, FIX["exp_median_u8_3x3_reflect"])
    # any other dtype means its float64 values
    assert np.array_equal(amd.gpet_utils.denoise(img.astype(np.int32), "median", dict(size=3), ctx=ctx), FIX["exp_median_u8_3x3_reflect"].astype(np.float64))


# ---- stacks ------------------------------------------------------------------------------------------------------------------------
def seeded_stack(dt, T, M, N, seed, noise=0.15):
    return np.stack([R.make_frame(seed + t, M, N, noise * (1 + t % 3), DT[dt]) for t in range(T)])


@pytest.mark.parametrize("spec", SPECS, ids=SPEC_IDS)
@pytest.mark.parametrize("dt", ["u8", "u16", "f32", "f64"])
def test_stack_of_8_equals_single_frame_calls_and_the_restatement(amd, ctx, dt, spec):
    tech, kw = spec
    stack = seeded_stack(dt, 8, 37, 131, seed=100 + len(tech))
    got, n_iter = amd.gpet_utils.denoise_imgs(stack, tech, kw, ctx=ctx, return_n_iter=True)
    for t in range(8):
        one, n1 = amd.gpet_utils.denoise_imgs([stack[t]], tech, kw, ctx=ctx, return_n_iter=True)
        assert np.array_equal(got[t], one[0]) and n_iter[t] == n1[0], (dt, tech, t)
    # a frame's neighbours in a stack do not matter
    other = amd.gpet_utils.denoise_imgs([stack[5], stack[2], stack[7]], tech, kw, ctx=ctx)
    assert np.array_equal(other[1], got[2]) and np.array_equal(other[0], got[5])
    # and the values are the restatement's ('tvc' of a float32 frame: on the promoted frame)
    for t in (0, 3):
        src = stack[t].astype(np.float64) if (tech == "tvc" and dt == "f32") else stack[t]
        want = R.denoise(src, tech, kw)
        assert got[t].dtype == want.dtype and np.array_equal(got[t], want), (dt, tech, t)
    if tech == "tvc":
        assert [int(v) for v in n_iter[:4]] == [R.tvc(stack[t].astype(np.float64) if dt == "f32" else stack[t], kw["weight"], return_info=True)[1]
                                               for t in range(4)]
    else:
        assert not n_iter.any()


@pytest.mark.parametrize("spec", [SPECS[0], SPECS[5], SPECS[7]], ids=["median3", "gauss1.5", "tvc"])
def test_a_stack_of_more_than_one_chunk(amd, ctx, spec):
    """float64 frames of 500 x 500 go up 16 ('median'), 11 ('gaussian') and 5 ('tvc') to a chunk (tests/test_denoise_plan.py pins
    that plan): later chunks reuse the staging slot and the workspace of the earlier ones."""
    tech, kw = spec
    T = {"median": 18, "gaussian": 13, "tvc": 7}[tech]
    stack = seeded_stack("f64", T, 500, 500, seed=7, noise=0.2)
    got, n_iter = amd.gpet_utils.denoise_imgs(stack, tech, kw, ctx=ctx, return_n_iter=True)
    for t in (0, T // 2, T - 2, T - 1):
        one, n1 = amd.gpet_utils.denoise_imgs([stack[t]], tech, kw, ctx=ctx, return_n_iter=True)
        assert np.array_equal(got[t], one[0]) and n_iter[t] == n1[0], (tech, t)
    assert np.array_equal(got[T - 1], R.denoise(stack[T - 1], tech, kw))
    # and the context's staging serves a smaller call afterwards
    assert np.array_equal(amd.gpet_utils.denoise_imgs(stack[T - 2:], tech, kw, ctx=ctx), got[T - 2:])


@pytest.mark.parametrize("spec", SPECS, ids=SPEC_IDS)
def test_device_frames_equal_host_frames_and_are_not_written(amd, ctx, spec):
    L = amd._lib
    tech, kw = spec
    k = amd.gpet_utils.kernel_builder((11, 5))
    for dt in ("u8", "f32"):
        stack = seeded_stack(dt, 3, 37, 131, seed=40)
        dev = DeviceFrames(ctx, stack)
        try:
            raw = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=stack.dtype, shape=stack.shape[1:], denoise=spec)
            out, n_iter = ctx.denoise_images(raw)
            want, n_want = amd.gpet_utils.denoise_imgs(stack, tech, kw, ctx=ctx, return_n_iter=True)
            assert np.array_equal(out, want) and np.array_equal(n_iter, n_want)
            g_dev = ctx.grad_images(L.RawFrames(k, device_ptrs=dev.ptrs, dtype=stack.dtype, shape=stack.shape[1:], denoise=spec))
            assert np.array_equal(g_dev, amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx, denoise=spec))
            for i in range(3):
                assert np.array_equal(dev.download(i), stack[i])
        finally:
            dev.free()


# ---- composition: exact by construction --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", SPECS, ids=SPEC_IDS)
@pytest.mark.parametrize("dt", ["u8", "u16", "f32", "f64"])
def test_gradient_images_of_denoised_frames(amd, ctx, dt, spec):
    stack = seeded_stack(dt, 5, 53, 70, seed=60)
    rng = np.random.default_rng(0)
    for k in (amd.gpet_utils.kernel_builder((11, 5)), rng.normal(size=(4, 3))):
        one_pass = amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx, denoise=spec)
        two_step = amd.gpet_utils.comp_grad_imgs(amd.gpet_utils.denoise_imgs(stack, spec[0], spec[1], ctx=ctx), k, ctx=ctx)
        assert one_pass.dtype == np.float32 and np.array_equal(one_pass, two_step)
        assert not np.array_equal(one_pass, amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx))  # (denoising does something)


def test_denoise_none_is_the_parents_path(amd, ctx):
    k = amd.gpet_utils.kernel_builder((11, 5))
    for dt in ("u8", "f64"):
        stack = seeded_stack(dt, 4, 64, 64, seed=9)
        want = np.stack([amd.gpet_utils.comp_grad_img(f, k, ctx=ctx) for f in stack])
        assert np.array_equal(amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx, denoise=None), want)
        assert np.array_equal(amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx), want)
        none = amd._lib.GpetDenoise(technique=amd._lib.DN_NONE)  # technique NONE through the new entry point
        assert np.array_equal(ctx.grad_images(amd._lib.RawFrames(k, frames=stack, denoise=none)), want)


def drifting_frames(N, T, seed0, dtype, noise_seed=0):
    """T frames of one drifting sinusoidal edge (tests/test_gpu_raw_frames.py) with speckle on top, as raw frames of ``dtype``."""
    frames, init = [], None
    rs = np.random.RandomState(noise_seed)
    for t in range(T):
        img, truth = orc.synth_sinusoid_image(N, seed0 + t, amplitude=int(0.4 * N * (1.0 + 0.02 * t)))
        if init is None:
            init = truth[[0, -1], :][:, [1, 0]]
        img = np.clip(img + rs.normal(0.0, 0.05, img.shape), 0.0, 1.0)
        frames.append(np.rint(img * 255.0).astype(np.uint8) if dtype == "uint8" else img.astype(dtype))
    return frames, init


KW_RBF = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 20, 'length_scale': 8}, noise_y=1, N_samples=300, score_thresh=1, delta_x=8,
              keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)


def assert_same_batch(amd, a, b, what):
    """Images, gradient KDEs, then (run both) traces, credible intervals and iteration counts of two batch objects."""
    L = amd._lib
    n_img = 1 if a._batch.share_image else a.B
    for e in range(n_img):
        assert np.array_equal(a._batch.read(L.BUF_GRAD, e), b._batch.read(L.BUF_GRAD, e)), (what, "grad", e)
        assert np.array_equal(a._batch.read(L.BUF_GRAD_KDE, e), b._batch.read(L.BUF_GRAD_KDE, e)), (what, "grad kde", e)
    ra, rb = a(), b()
    assert a.timings["iters"] == b.timings["iters"] and min(a.timings["iters"]) >= 1, (what, a.timings["iters"], b.timings["iters"])
    for e, ((ta, (la, ua)), (tb, (lb, ub))) in enumerate(zip(ra, rb)):
        assert np.array_equal(ta, tb), (what, "trace", e)
        assert np.array_equal(la, lb) and np.array_equal(ua, ub), (what, "interval", e)


def test_technique_none_and_denoise_false_through_the_batch_calls(amd, ctx):
    """gpet_batch_create_raw_dn / gpet_batch_set_raw_images_dn with a technique-NONE struct, and set_frame(denoise=False) on a batch
    built WITH a spec, give what the calls without the argument give: images, gradient KDE, traces, intervals, iterations."""
    L = amd._lib
    N, B = 128, 2
    k = amd.gpet_utils.kernel_builder((11, 5))
    for dtype in ("uint8", "float32"):
        frames, init = drifting_frames(N, 2 * B, 41, dtype)
        plain = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=frames[:B], grad_kernel=k, return_std=True, _ctx=ctx, **KW_RBF)
        none = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=frames[:B], grad_kernel=k, return_std=True, _ctx=ctx,
                                         denoise=L.GpetDenoise(technique=L.DN_NONE), **KW_RBF)
        assert none._batch._keep[0].dn is not None  # (the struct went through gpet_batch_create_raw_dn)
        assert_same_batch(amd, none, plain, "technique NONE, construction")
        none.set_frame(raw_imgs=frames[B:], seeds=[6, 7], next_frame=False)  # (the constructor's struct: gpet_batch_set_raw_images_dn)
        plain.set_frame(raw_imgs=frames[B:], seeds=[6, 7], next_frame=False)
        assert_same_batch(amd, none, plain, "technique NONE, set_frame")
        spec = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=frames[:B], grad_kernel=k, return_std=True, _ctx=ctx,
                                         denoise=("median", dict(size=3)), **KW_RBF)
        spec.set_frame(raw_imgs=frames[B:], seeds=[6, 7], next_frame=False, denoise=False)
        plain.set_frame(raw_imgs=frames[B:], seeds=[6, 7], next_frame=False)
        assert_same_batch(amd, spec, plain, "denoise=False")
        spec.set_frame(raw_imgs=frames[B:], seeds=[6, 7], next_frame=False)  # (and the constructor's spec is still remembered)
        assert not np.array_equal(spec._batch.read(L.BUF_GRAD, 0), plain._batch.read(L.BUF_GRAD, 0))
        for bt in (plain, none, spec):
            bt._batch.close()


@pytest.mark.parametrize("share", [True, False], ids=["shared", "per_edge"])
@pytest.mark.parametrize("spec", [SPECS[0], SPECS[2], SPECS[5], SPECS[7]], ids=["median3", "median4x3", "gauss1.5", "tvc"])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_batch_with_denoise_equals_batch_from_denoised_frames(amd, ctx, dtype, spec, share):
    """Creation, then set_frame with the remembered spec, then set_frame overriding it; host frames."""
    N, B = 128, 3
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, 3 if share else 3 * B, 21, dtype)
    sets = [frames[0], frames[1], frames[2]] if share else [frames[0:B], frames[B:2 * B], frames[2 * B:3 * B]]

    def dn(s, d):
        out = amd.gpet_utils.denoise_imgs([s] if share else s, d[0], d[1], ctx=ctx)
        return out[0] if share else list(out)

    seeds = [3, 4, 5]
    one = amd.GP_Edge_Tracing_Batch([init] * B, None, seeds, raw_imgs=sets[0], grad_kernel=k, denoise=spec, return_std=True, _ctx=ctx, **KW_RBF)
    two = amd.GP_Edge_Tracing_Batch([init] * B, None, seeds, raw_imgs=dn(sets[0], spec), grad_kernel=k, return_std=True, _ctx=ctx, **KW_RBF)
    assert one._batch.share_image == two._batch.share_image == share
    assert_same_batch(amd, one, two, "construction")
    one.set_frame(raw_imgs=sets[1], seeds=[6, 7, 8], next_frame=False)  # (the constructor's spec)
    two.set_frame(raw_imgs=dn(sets[1], spec), seeds=[6, 7, 8], next_frame=False)
    assert_same_batch(amd, one, two, "set_frame")
    other = ("gaussian", dict(sigma=0.8)) if spec[0] != "gaussian" else ("minimum", dict(size=3))
    one.set_frame(raw_imgs=sets[2], seeds=[9, 10, 11], next_frame=True, denoise=other)
    two.set_frame(raw_imgs=dn(sets[2], other), seeds=[9, 10, 11], next_frame=True)
    assert_same_batch(amd, one, two, "set_frame(denoise=other)")
    one._batch.close()
    two._batch.close()


@pytest.mark.parametrize("spec", [SPECS[1], SPECS[7]], ids=["median5", "tvc"])
def test_batch_with_denoise_on_device_frames(amd, ctx, spec):
    N, B = 128, 2
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, 2 * B + 1, 5, "uint8")
    dev = DeviceFrames(ctx, frames)
    try:
        for share in (True, False):
            first, nxt = ([0], [1]) if share else ([0, 1], [2, 3])
            one = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_device_ptrs=[dev.ptrs[i] for i in first], raw_dtype=np.uint8,
                                            grad_shape=(N, N), grad_kernel=k, denoise=spec, return_std=True, _ctx=ctx, **KW_RBF)
            den = amd.gpet_utils.denoise_imgs([frames[i] for i in first], spec[0], spec[1], ctx=ctx)
            two = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=den[0] if share else list(den), grad_kernel=k,
                                            return_std=True, _ctx=ctx, **KW_RBF)
            assert one._batch.share_image == two._batch.share_image == share
            assert_same_batch(amd, one, two, "device frames, construction")
            one.set_frame(raw_device_ptrs=[dev.ptrs[i] for i in nxt], seeds=[6, 7])
            den = amd.gpet_utils.denoise_imgs([frames[i] for i in nxt], spec[0], spec[1], ctx=ctx)
            two.set_frame(raw_imgs=den[0] if share else list(den), seeds=[6, 7])
            assert_same_batch(amd, one, two, "device frames, set_frame")
            one._batch.close()
            two._batch.close()
        for i in range(len(frames)):
            assert np.array_equal(dev.download(i), frames[i])
    finally:
        dev.free()


@pytest.mark.parametrize("spec", [SPECS[0], SPECS[7]], ids=["median3", "tvc"])
def test_sequence_with_denoise_equals_sequence_of_denoised_frames(amd, ctx, spec):
    N, T = 128, 6
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, T, 11, "uint8")
    seeds = [3 + t for t in range(T)]
    a = amd.SequenceTracer(frames, init, n_chains=2, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, denoise=spec, **KW_RBF)
    den = list(amd.gpet_utils.denoise_imgs(frames, spec[0], spec[1], ctx=ctx))
    b = amd.SequenceTracer(den, init, n_chains=2, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, **KW_RBF)
    ra, rb = a(), b()
    assert a.iterations == b.iterations and min(a.iterations) >= 1
    for t in range(T):
        assert np.array_equal(ra[t], rb[t]), t
    rc = amd.trace_sequence(frames, init, n_chains=2, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, denoise=spec, **KW_RBF)
    assert all(np.array_equal(x, y) for x, y in zip(rc, rb))


# ---- 'tvc': images that stop at different iterations --------------------------------------------------------------------------------
def test_tvc_images_of_one_chunk_stop_at_different_iterations(amd, ctx):
    frames = [R.make_frame(70 + t, 48, 100, noise, np.float64) for t, noise in enumerate((0.02, 0.3, 0.1, 0.3, 0.05, 0.2))]
    want = [R.tvc(f, 0.1, return_info=True) for f in frames]
    counts = [w[1] for w in want]
    assert len(set(counts)) >= 3 and max(counts) > 8 + min(counts)  # (more than one group of iterations apart)
    got, n_iter = amd.gpet_utils.denoise_imgs(frames, "tvc", dict(weight=0.1), ctx=ctx, return_n_iter=True)
    assert [int(v) for v in n_iter] == counts
    for t, f in enumerate(frames):
        one, n1 = amd.gpet_utils.denoise_imgs([f], "tvc", dict(weight=0.1), ctx=ctx, return_n_iter=True)
        assert np.array_equal(got[t], one[0]) and int(n1[0]) == counts[t], t
        assert np.array_equal(got[t], want[t][0]), t
    # n_iter_max below the natural counts stops every image there, as the reference does; exactly at a count changes nothing
    for cap in (1, 3, 9, min(counts), max(counts)):
        got_c, n_c = amd.gpet_utils.denoise_imgs(frames, "tvc", dict(weight=0.1, n_iter_max=cap), ctx=ctx, return_n_iter=True)
        assert [int(v) for v in n_c] == [min(cap, c) for c in counts], cap
        for t in (0, 1, 4):
            assert np.array_equal(got_c[t], R.tvc(frames[t], 0.1, n_iter_max=cap)), (cap, t)


def test_tvc_runs_are_identical(amd, ctx):
    stack = seeded_stack("f64", 6, 200, 300, seed=90, noise=0.1)
    a, na = amd.gpet_utils.denoise_imgs(stack, "tvc", dict(weight=0.15), ctx=ctx, return_n_iter=True)
    b, nb = amd.gpet_utils.denoise_imgs(stack, "tvc", dict(weight=0.15), ctx=ctx, return_n_iter=True)
    assert np.array_equal(na, nb) and na.min() >= 2 and np.array_equal(a, b)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_bad_specs_are_refused_and_the_batch_traces_on(amd, ctx):
    L = amd._lib
    N = 128
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, 2, 2, "uint8")
    good = dict(technique=L.DN_MEDIAN, size_y=3, size_x=3, mode=0, sigma_y=1.0, sigma_x=1.0, truncate=4.0, weight=0.1, eps=2e-4, n_iter_max=200)
    bad = {"technique 9": (dict(technique=9), "unknown denoising technique"),
           "technique -1": (dict(technique=-1), "unknown denoising technique"),
           "window 10 x 9": (dict(size_y=10, size_x=9), "81 pixels"),
           "window 0": (dict(technique=L.DN_MINIMUM, size_y=0), "at least 1"),
           "sigma 0": (dict(technique=L.DN_GAUSSIAN, sigma_x=0.0), "sigma"),
           "sigma < 0": (dict(technique=L.DN_GAUSSIAN, sigma_y=-1.0), "sigma"),
           "weight 0": (dict(technique=L.DN_TVC, weight=0.0), "weight"),
           "n_iter_max 0": (dict(technique=L.DN_TVC, n_iter_max=0), "n_iter_max"),
           "mode 5": (dict(mode=5), "boundary mode"),
           "gaussian mode 2": (dict(technique=L.DN_GAUSSIAN, mode=2), "boundary mode")}

    def refused(call, text):
        with pytest.raises(L.GpetError) as ei:
            call()
        assert ei.value.code == L.ERR_BAD_ARG and text in str(ei.value), str(ei.value)

    def raw_with(fields, kernel=k):
        return L.RawFrames(kernel, frames=frames, denoise=L.GpetDenoise(**dict(good, **fields)))

    spec = ("median", dict(size=3))
    want = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames, grad_kernel=k, denoise=spec, _ctx=ctx, **KW_RBF)
    want_grad = want._batch.read(L.BUF_GRAD, 1)
    want_traces = want()
    from gaussian_process_edge_trace_amd.gpet import to_abi_params
    params = [to_abi_params(p) for p in want._ps]
    bt = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames, grad_kernel=k, denoise=spec, _ctx=ctx, **KW_RBF)
    for name, (fields, text) in bad.items():
        refused(lambda: ctx.denoise_images(raw_with(fields, kernel=None)), text)
        refused(lambda: ctx.grad_images(raw_with(fields)), text)
        refused(lambda: L.Batch(ctx, None, params, [init, init], raw=raw_with(fields)), text)
        refused(lambda: bt._batch.set_images(raw=raw_with(fields)), text)
    refused(lambda: ctx.denoise_images(raw_with(dict(technique=L.DN_NONE), kernel=None)), "no technique")
    assert np.array_equal(bt._batch.read(L.BUF_GRAD, 1), want_grad)
    got = bt()  # the batch is as it was: it traces, and to the same result
    assert bt.timings["iters"] == want.timings["iters"]
    assert all(np.array_equal(x, y) for x, y in zip(got, want_traces))
    # and so does the context
    assert np.array_equal(amd.gpet_utils.denoise_imgs(frames, *spec, ctx=ctx), np.stack([R.median(f, 3) for f in frames]))
    bt._batch.close()
    want._batch.close()
