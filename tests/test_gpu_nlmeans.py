"""GPU tests of the non-local means stage: gpet_utils.denoise / denoise_imgs with 'nl' (gpet_nlmeans_images), comp_grad_imgs(denoise=),
GP_Edge_Tracing_Batch(raw_imgs=, denoise=) / set_frame and trace_sequence with ``denoise=('nl', kwargs)``.

The reference is tests/golden/nlmeans.npz, written by the unmodified reference under scikit-image 0.18.3 (fast_mode=False); where an
input is not in it, tests/nlmeans_ref.py stands in, which tests/test_nlmeans_fixture.py pins to the fixture bit for bit.  Everything
is np.array_equal.  Parity tests inject the fixture's patch weights (a numpy whose exp differs in the last place derives weights a
few units apart: DESIGN.md 9); compositions use the derived ones on both sides and are exact by construction."""
import json
import os

import numpy as np
import pytest

from tests import nlmeans_ref as R
from tests.test_gpu_denoise import KW_RBF, DeviceFrames, assert_same_batch, drifting_frames

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "nlmeans.npz"))
CASES = json.loads(str(FIX["cases"]))
NL = dict(patch_size=5, patch_distance=4, h=0.15, sigma=0.02, fast_mode=False)  # (the compositions: small, so that tests stay quick)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def run(amd, ctx, frames, kw, taps=None, device_in=False, device_out=False):
    """gpet_nlmeans_images of a list of frames -> (T, M, N) float64, through host or device memory on either side."""
    L = amd._lib
    spec = kw if isinstance(kw, L.NlmeansSpec) else L.nlmeans_spec(dict(kw, fast_mode=False), taps=taps)
    dev = DeviceFrames(ctx, frames) if device_in else None
    buf = L.PreFrames(ctx) if device_out else None
    try:
        if device_in:
            raw = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=frames[0].dtype, shape=frames[0].shape, denoise=spec)
        else:
            raw = L.RawFrames(None, frames=frames, denoise=spec)
        if not device_out:
            out = ctx.nlmeans_images(raw)
        else:
            M, N = frames[0].shape
            ptrs = buf.reserve(len(frames), M * N * 8)
            assert ctx.nlmeans_images(raw, out_device_ptrs=ptrs) is None
            out = np.empty((len(frames), M, N))
            for g, p in enumerate(ptrs):  # (gpet_dev_copy is on the context's stream and waits: stream order alone makes the frames ready)
                ctx.check(ctx.lib.gpet_dev_copy(ctx.h, out[g].ctypes.data, L._P(p), out[g].nbytes, 1))
        if device_in:
            for i, f in enumerate(frames):
                assert np.array_equal(dev.download(i), f)  # (read where they lie, not written)
        return out
    finally:
        if dev is not None:
            dev.free()
        if buf is not None:
            buf.close()


# ---- against the fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_equals_the_reference(amd, ctx, case):
    """Every case of the fixture: frames of 9 x 11 (the window clipped on every side at once; with (7, 11) wider than the frame),
    20 x 70 and 33 x 65 (past one tile each way); (s, d) = (3, 2), (4 -> 5, 2), (5, 3), (7, 11); sigma 0 and 0.05; an h that stops
    most candidates at the cutoff; a distance that crosses the cutoff and falls back; u8, u16, f64, and f32 against the reference
    on the widened frame."""
    img, exp = FIX["in_" + case["input"]], FIX["exp_" + case["name"]]
    out = run(amd, ctx, [img], case["kwargs"], taps=FIX[case["taps"]])
    assert out.dtype == np.float64 and out.shape == (1,) + exp.shape
    assert np.array_equal(out[0], exp)


def test_through_gpet_utils_with_the_restatement_on_the_derived_taps(amd, ctx):
    img = FIX["in_f64_b"]
    kw = dict(patch_size=5, patch_distance=3, h=0.1, sigma=0.05, fast_mode=False)
    w = amd._lib.nlmeans_taps(5, 0.1)
    exp = R.nlmeans(img, 5, 3, 0.1, 0.05, w=w)
    out = amd.gpet_utils.denoise(img, "nl", kw, ctx=ctx)
    assert out.dtype == np.float64 and np.array_equal(out, exp)
    u8 = FIX["in_u8_b"]
    stack = amd.gpet_utils.denoise_imgs([u8, u8[::-1].copy()], "nl", dict(patch_size=3, patch_distance=2, h=25.0, fast_mode=False), ctx=ctx)
    w = amd._lib.nlmeans_taps(3, 25.0)
    assert np.array_equal(stack[0], R.nlmeans(u8, 3, 2, 25.0, w=w)) and np.array_equal(stack[1], R.nlmeans(u8[::-1], 3, 2, 25.0, w=w))


# ---- launch shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("device_in", [False, True], ids=["host_in", "device_in"])
def test_three_frames_in_one_call(amd, ctx, device_in, device_out):
    """Different content per frame; the result of a frame does not depend on how many frames the call holds or where it stands."""
    frames = [FIX["in_f64_c"], FIX["in_f64_c"][::-1].copy(), np.ascontiguousarray(FIX["in_f64_c"][:, ::-1])]
    kw = dict(patch_size=7, patch_distance=11, h=0.1, sigma=0.05)
    taps = FIX["taps_s7_h0.1"]
    exp0 = FIX["exp_f64_c_s7_d11_sig0.05"]
    out = run(amd, ctx, frames, kw, taps=taps, device_in=device_in, device_out=device_out)
    assert np.array_equal(out[0], exp0)
    singles = [run(amd, ctx, [f], kw, taps=taps, device_in=device_in, device_out=device_out)[0] for f in frames]
    for g in range(3):
        assert np.array_equal(out[g], singles[g]), g
    back = run(amd, ctx, frames[::-1], kw, taps=taps, device_in=device_in, device_out=device_out)
    for g in range(3):
        assert np.array_equal(back[2 - g], singles[g]), g
    assert not np.array_equal(singles[0], singles[1]) and not np.array_equal(singles[0], singles[2])


def test_a_stack_of_two_chunks_with_a_short_last_one(amd, ctx):
    """Host in, host out: a float64 frame of 1024 x 1024 stages 8388608 bytes and its result as many, so 4 frames fill the 64 MiB
    of a chunk and 5 frames are 4 + 1 (tests/test_raw_frames_host.py asserts the split).  The first frame of the first chunk, its
    last frame and the one frame of the last chunk differ; every frame's result is that of its one-frame call, bit for bit.
    (Frames and results on the device take one launch and no chunk.)"""
    a = np.random.RandomState(3).rand(1024, 1024)
    frames = dict(a=a, b=a[::-1].copy(), c=np.ascontiguousarray(a[:, ::-1]), filler=np.ascontiguousarray(a.T))
    kw = dict(patch_size=3, patch_distance=1, h=0.1, sigma=0.0)
    singles = {k: run(amd, ctx, [f], kw)[0] for k, f in frames.items()}
    assert not np.array_equal(singles["a"], singles["b"]) and not np.array_equal(singles["a"], singles["c"])
    names = ["a", "filler", "filler", "b", "c"]
    out = run(amd, ctx, [frames[k] for k in names], kw)
    for g, k in enumerate(names):
        assert np.array_equal(out[g], singles[k]), (g, k)


def test_u8_device_frames_into_device_memory(amd, ctx):
    img = FIX["in_u8_b"]
    out = run(amd, ctx, [img, img], dict(patch_size=7, patch_distance=11, h=25.0, sigma=12.5), taps=FIX["taps_s7_h25.0"], device_in=True, device_out=True)
    assert np.array_equal(out[0], FIX["exp_u8_b_s7_d11"]) and np.array_equal(out[1], out[0])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_bad_arg_with_the_reason(amd, ctx):
    L = amd._lib
    frame = FIX["in_f64_a"]

    def refused(spec, frames, reason):
        with pytest.raises(L.GpetError) as e:
            ctx.nlmeans_images(L.RawFrames(None, frames=frames, denoise=spec))
        assert e.value.code == L.ERR_BAD_ARG and reason in str(e.value), str(e.value)

    refused(L.NlmeansSpec(1, 2, 0.1, 0.0, np.ones((1, 1))), [frame], "patch_size")                        # a patch of one pixel
    refused(L.nlmeans_spec(dict(patch_size=7, fast_mode=False)), [np.zeros((3, 20))], "smaller extent")  # off = 3 >= min(M, N)
    refused(L.nlmeans_spec(dict(patch_size=7, fast_mode=False)), [np.zeros((20, 2))], "smaller extent")
    bad = L.nlmeans_taps(5, 0.1)
    bad[4, 4] = np.nan
    refused(L.nlmeans_spec(dict(patch_size=5, fast_mode=False), taps=bad), [frame], "finite")
    refused(L.NlmeansSpec(7, 32, 0.1, 0.0, L.nlmeans_taps(7, 0.1)), [frame], "above 31")                 # d above the bound
    refused(L.NlmeansSpec(5, 31, 0.1, 0.0, L.nlmeans_taps(5, 0.1)), [frame], "73472")                    # the LDS bound, with the byte counts
    refused(L.NlmeansSpec(5, 3, 0.0, 0.0, L.nlmeans_taps(5, 0.1)), [frame], "h must")
    # and the context works on
    assert np.array_equal(run(amd, ctx, [frame], dict(patch_size=3, patch_distance=2, h=0.1, sigma=0.0), taps=FIX["taps_s3_h0.1"])[0],
                          FIX["exp_f64_a_s3_d2_sig0"])


def test_a_refused_spec_leaves_a_batch_on_its_old_frames(amd, ctx):
    L = amd._lib
    N = 64
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, 4, 31, "uint8")
    nl = ("nl", dict(NL, h=40.0, sigma=5.0))
    want = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames[:2], grad_kernel=k, denoise=nl, _ctx=ctx, **KW_RBF)
    want_grad = want._batch.read(L.BUF_GRAD, 1)
    want_traces = want()
    bt = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames[:2], grad_kernel=k, denoise=nl, _ctx=ctx, **KW_RBF)
    bad = L.nlmeans_taps(5, 40.0)
    bad[0, 0] = np.inf
    with pytest.raises(L.GpetError) as e:
        bt.set_frame(raw_imgs=frames[2:], denoise=L.nlmeans_spec(nl[1], taps=bad))
    assert e.value.code == L.ERR_BAD_ARG and "finite" in str(e.value)
    with pytest.raises(NotImplementedError, match="fast_mode"):
        bt.set_frame(raw_imgs=frames[2:], denoise=("nl", dict(patch_size=5)))
    assert np.array_equal(bt._batch.read(L.BUF_GRAD, 1), want_grad)
    for a, b in zip(bt(), want_traces):
        assert np.array_equal(a, b)
    bt._batch.close()
    want._batch.close()


# ---- compositions ------------------------------------------------------------------------------------------------------------------
def test_gradient_images_of_denoised_frames(amd, ctx):
    k = amd.gpet_utils.kernel_builder((11, 5))
    for dtype, kw in (("uint8", dict(NL, h=40.0, sigma=5.0)), ("float64", NL)):
        frames, _ = drifting_frames(64, 3, 7, dtype)
        one_pass = amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx, denoise=("nl", kw))
        den = amd.gpet_utils.denoise_imgs(frames, "nl", kw, ctx=ctx)
        assert den.dtype == np.float64 and one_pass.dtype == np.float32
        assert np.array_equal(one_pass, amd.gpet_utils.comp_grad_imgs(den, k, ctx=ctx))
        assert not np.array_equal(one_pass, amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx))  # (denoising does something)
        two = amd.gpet_utils.comp_grad_imgs(frames, [k, -k], ctx=ctx, denoise=("nl", kw))
        assert np.array_equal(two[:, 0], one_pass) and np.array_equal(two[:, 1], amd.gpet_utils.comp_grad_imgs(den, -k, ctx=ctx))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_batch_with_nlmeans_equals_batch_from_denoised_frames(amd, ctx, dtype):
    """Creation, then set_frame with the remembered spec, host frames first and device frames after."""
    N, B = 64, 2
    k = amd.gpet_utils.kernel_builder((11, 5))
    kw = dict(NL, h=40.0, sigma=5.0) if dtype == "uint8" else NL
    frames, init = drifting_frames(N, 3 * B, 21, dtype)
    sets = [frames[0:B], frames[B:2 * B], frames[2 * B:3 * B]]
    dn = lambda s: list(amd.gpet_utils.denoise_imgs(s, "nl", kw, ctx=ctx))  # noqa: E731
    one = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=sets[0], grad_kernel=k, denoise=("nl", kw), return_std=True, _ctx=ctx, **KW_RBF)
    two = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=dn(sets[0]), grad_kernel=k, return_std=True, _ctx=ctx, **KW_RBF)
    assert_same_batch(amd, one, two, "construction")
    one.set_frame(raw_imgs=sets[1], seeds=[6, 7], next_frame=False)  # (the constructor's spec)
    two.set_frame(raw_imgs=dn(sets[1]), seeds=[6, 7], next_frame=False)
    assert_same_batch(amd, one, two, "set_frame")
    dev = DeviceFrames(ctx, sets[2])
    try:
        one.set_frame(raw_device_ptrs=dev.ptrs, raw_dtype=frames[0].dtype, seeds=[8, 9], next_frame=True)
        two.set_frame(raw_imgs=dn(sets[2]), seeds=[8, 9], next_frame=True)
        assert_same_batch(amd, one, two, "set_frame, device frames")
    finally:
        dev.free()
    one._batch.close()
    two._batch.close()


def test_image_map_and_two_kernels(amd, ctx):
    """Two frames, two kernels, four edges: every frame is denoised once, then read through both kernels."""
    N = 64
    k0 = amd.gpet_utils.kernel_builder((11, 5))
    k1 = amd.gpet_utils.kernel_builder((7, 3))
    kw = dict(NL, h=40.0, sigma=5.0)
    frames, init = drifting_frames(N, 4, 51, "uint8")
    dn = lambda s: list(amd.gpet_utils.denoise_imgs(s, "nl", kw, ctx=ctx))  # noqa: E731
    common = dict(grad_kernel=[k0, k1], kernel_of=[0, 1, 0, 1], image_of=[0, 0, 1, 1], return_std=True, _ctx=ctx)
    one = amd.GP_Edge_Tracing_Batch([init] * 4, None, [3, 4, 5, 6], raw_imgs=frames[:2], denoise=("nl", kw), **common, **KW_RBF)
    two = amd.GP_Edge_Tracing_Batch([init] * 4, None, [3, 4, 5, 6], raw_imgs=dn(frames[:2]), **common, **KW_RBF)
    assert one._batch.n_img == two._batch.n_img == 4
    assert_same_batch(amd, one, two, "image map, construction")
    one.set_frame(raw_imgs=frames[2:], seeds=[7, 8, 9, 10], next_frame=False)
    two.set_frame(raw_imgs=dn(frames[2:]), seeds=[7, 8, 9, 10], next_frame=False)
    assert_same_batch(amd, one, two, "image map, set_frame")
    one._batch.close()
    two._batch.close()


def test_sequence_of_three_frames(amd, ctx):
    N, T = 64, 3
    k = amd.gpet_utils.kernel_builder((11, 5))
    kw = dict(NL, h=40.0, sigma=5.0)
    frames, init = drifting_frames(N, T, 11, "uint8")
    seeds = [3 + t for t in range(T)]
    ra = amd.trace_sequence(frames, init, n_chains=1, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, denoise=("nl", kw), **KW_RBF)
    den = list(amd.gpet_utils.denoise_imgs(frames, "nl", kw, ctx=ctx))
    rb = amd.trace_sequence(den, init, n_chains=1, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, **KW_RBF)
    assert len(ra) == len(rb) == T and all(np.array_equal(x, y) for x, y in zip(ra, rb))


# ---- the weight below -708 ---------------------------------------------------------------------------------------------------------
def test_final_distance_above_708_has_weight_zero(amd, ctx):
    """A flat frame with one pixel of 10: where that pixel sits in the LAST patch row of one of the two patches, the distance is 0
    at every row start and 8.38 * 100 = 838 or more at the end -- beyond the range in which the reference's exponential is defined.
    The device's weight there is +0.0, as the restatement's is: a defined result, finite and not negative."""
    img = np.zeros((12, 14))
    img[6, 7] = 10.0
    w = amd._lib.nlmeans_taps(3, 0.1)
    exp, info = R.nlmeans(img, 3, 2, 0.1, 0.0, w=w, return_info=True)
    assert info["dmax"] > 708.0
    out = run(amd, ctx, [img], dict(patch_size=3, patch_distance=2, h=0.1, sigma=0.0), taps=w)[0]
    assert np.isfinite(out).all() and (out >= 0.0).all()
    assert np.array_equal(out, exp)
    assert out[5, 7] == 0.0  # (the spike in the last row of the pixel's own patch: every candidate but the pixel itself weighs 0)
