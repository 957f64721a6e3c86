"""GPU tests of the fast-mode non-local means stage: gpet_utils.denoise / denoise_imgs with 'nl_fast' (gpet_nlmeans_fast_images),
comp_grad_imgs(denoise=), GP_Edge_Tracing_Batch(raw_imgs=, denoise=) / set_frame, trace_sequence and a vertical batch with
``denoise=('nl_fast', kwargs)``.

The reference is tests/golden/nlmeans_fast.npz, written by the unmodified reference under scikit-image 0.18.3 with fast_mode=True;
where an input is not in it, tests/nlmeans_fast_ref.py stands in, which tests/test_nlmeans_fast_fixture.py pins to the fixture bit
for bit.  Everything is np.array_equal: the stage claims the library's result bit for bit, with no deviation of its own."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import nlmeans_fast_ref as R
from tests.test_gpu_denoise import KW_RBF, DeviceFrames, assert_same_batch, drifting_frames

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "nlmeans_fast.npz"))
CASES = json.loads(str(FIX["cases"]))
BY_NAME = {c["name"]: c for c in CASES}
NLF = dict(patch_size=5, patch_distance=3, h=0.1, sigma=0.0)  # (the compositions, float frames)
NLF_U8 = dict(NLF, h=40.0, sigma=5.0)                          # (uint8 frames keep their range)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def case_input(case):
    return FIX["in_" + case["input"]]


def run(amd, ctx, frames, kw, device_in=False, device_out=False):
    """gpet_nlmeans_fast_images of a list of frames -> (T, M, N) float64, through host or device memory on either side."""
    L = amd._lib
    dev = DeviceFrames(ctx, frames) if device_in else None
    buf = L.PreFrames(ctx) if device_out else None
    try:
        if device_in:
            raw = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=frames[0].dtype, shape=frames[0].shape, denoise=("nl_fast", kw))
        else:
            raw = L.RawFrames(None, frames=frames, denoise=("nl_fast", kw))
        if not device_out:
            out = ctx.nlmeans_fast_images(raw)
        else:
            M, N = frames[0].shape
            ptrs = buf.reserve(len(frames), M * N * 8)
            assert ctx.nlmeans_fast_images(raw, out_device_ptrs=ptrs) is None
            out = np.empty((len(frames), M, N))
            for g, p in enumerate(ptrs):
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
    """Every case of the fixture: 9 x 11, 20 x 70 and 33 x 65 float64 frames at (s, d) = (3, 2), (4, 2), (5, 3) and the defaults'
    (7, 11), sigma 0 and 0.05 -- the float cases pin the order of every sum --, a small h that skips 96 % of the pairs, the
    defaults by omission, u8, u16 and f32 (against the reference on the widened frame)."""
    img, exp = case_input(case), FIX["exp_" + case["name"]]
    out = run(amd, ctx, [img], case["kwargs"])
    assert out.dtype == np.float64 and out.shape == (1,) + exp.shape
    assert np.array_equal(out[0], exp)


@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("device_in", [False, True], ids=["host_in", "device_in"])
@pytest.mark.parametrize("name", ["f64_c_s7_d11_sig0.05", "u8_b_s5_d3", "f32_b_s5_d3", "u16_b_s3_d2"])
def test_three_frames_from_and_to_either_memory(amd, ctx, name, device_in, device_out):
    case = BY_NAME[name]
    img = case_input(case)
    flipped = np.ascontiguousarray(img[::-1])
    out = run(amd, ctx, [img, flipped, img], case["kwargs"], device_in=device_in, device_out=device_out)
    exp = FIX["exp_" + name]
    assert np.array_equal(out[0], exp) and np.array_equal(out[2], exp)
    assert np.array_equal(out[1], run(amd, ctx, [flipped], case["kwargs"])[0]) and not np.array_equal(out[1], exp)


def test_a_frame_upside_down_against_the_restatement(amd, ctx):
    case = BY_NAME["f64_b_s5_d3_sig0.05"]
    img = np.ascontiguousarray(case_input(case)[::-1])
    assert np.array_equal(run(amd, ctx, [img], case["kwargs"])[0], R.with_kwargs(R.nlmeans_fast, img, case["kwargs"]))


def test_the_defaults_span_one_group_on_the_fixtures_frames_and_a_wide_search_spans_two(amd, ctx):
    """20 x 70 at the defaults keeps all 276 integral images at once (11 MB).  100 x 100 at d = 31, s = 3: 2016 shifts of 166 x 166
    cells are 444 MB, more than the 256 MiB a frame may keep: 37 rows of shifts, then 26 -- W and R go through the workspace."""
    L = amd._lib
    assert L.nlmeans_fast_plan(20, 70, 7, 11)["n_groups"] == 1
    plan = L.nlmeans_fast_plan(100, 100, 3, 31)
    assert plan["n_groups"] == 2 and plan["rows_per_group"] == 37 and plan["strips"] == 3 and plan["nr"] == 166
    img = np.random.RandomState(61).rand(100, 100)
    kw = dict(patch_size=3, patch_distance=31, h=0.3, sigma=0.02)
    want = R.with_kwargs(R.nlmeans_fast, img, kw)
    assert np.array_equal(run(amd, ctx, [img], kw)[0], want)


@pytest.fixture(scope="module")
def strips_case():
    """70 x 75 at s = 3, d = 1: six shifts, padded to 76 x 81 -- two strips of 64 rows, the second of 12."""
    img = np.random.RandomState(62).rand(70, 75)
    kw = dict(patch_size=3, patch_distance=1, h=0.2, sigma=0.01)
    return img, kw, R.with_kwargs(R.nlmeans_fast, img, kw)


def test_more_rows_than_a_strip_and_not_a_multiple_of_it(amd, ctx, strips_case):
    L = amd._lib
    img, kw, want = strips_case
    plan = L.nlmeans_fast_plan(70, 75, 3, 1)
    assert plan["n_shifts"] == 6 and plan["strips"] == 2 and plan["nr"] % L.NLF_STRIP != 0 and plan["nc"] % L.NLF_STRIP != 0
    assert np.array_equal(run(amd, ctx, [img], kw)[0], want)
    # the transposed frame: 81 x 76 padded, columns short of the rows
    assert np.array_equal(run(amd, ctx, [np.ascontiguousarray(img.T)], kw)[0], R.with_kwargs(R.nlmeans_fast, np.ascontiguousarray(img.T), kw))


@pytest.mark.parametrize("device", [False, True], ids=["host_in_host_out", "device_in_device_out"])
def test_a_stack_of_three_chunks(amd, ctx, device):
    """A 100 x 100 frame at d = 31 takes the chunk budget alone (tests/test_nlmeans_fast_plan.py: one frame per chunk): three
    frames are three chunks of two groups each, and every frame's result is that of its one-frame call."""
    L = amd._lib
    assert L.nlmeans_fast_plan(100, 100, 3, 31)["frames_per_chunk"] == 1
    rs = np.random.RandomState(63)
    frames = [rs.rand(100, 100) for _ in range(3)]
    kw = dict(patch_size=3, patch_distance=31, h=0.3, sigma=0.0)
    singles = [run(amd, ctx, [f], kw)[0] for f in frames]
    out = run(amd, ctx, frames, kw, device_in=device, device_out=device)
    for g in range(3):
        assert np.array_equal(out[g], singles[g]), g
    assert not np.array_equal(singles[0], singles[1])


def test_a_stack_of_two_chunks_of_small_frames(amd, ctx):
    """20 x 70 at the defaults: 24 frames to a chunk, so 25 frames are 24 + 1."""
    L = amd._lib
    assert L.nlmeans_fast_plan(20, 70, 7, 11)["frames_per_chunk"] == 24
    case = BY_NAME["f64_b_s7_d11_sig0.05"]
    img, exp = case_input(case), FIX["exp_f64_b_s7_d11_sig0.05"]
    flipped = np.ascontiguousarray(img[:, ::-1])
    frames = [img] * 23 + [flipped, img]
    out = run(amd, ctx, frames, case["kwargs"], device_in=True, device_out=True)
    assert all(np.array_equal(out[g], exp) for g in (0, 22, 24))
    assert np.array_equal(out[23], run(amd, ctx, [flipped], case["kwargs"])[0])


def test_through_gpet_utils(amd, ctx):
    case = BY_NAME["f64_c_defaults"]
    img, want = case_input(case), FIX["exp_f64_c_defaults"]
    out = amd.gpet_utils.denoise(img, "nl_fast", {}, ctx=ctx)
    assert out.dtype == np.float64 and np.array_equal(out, want)
    assert np.array_equal(amd.gpet_utils.denoise(img, "nl_fast", dict(fast_mode=True, multichannel=False), ctx=ctx), want)
    u8 = BY_NAME["u8_b_s5_d3"]
    stack, n_iter = amd.gpet_utils.denoise_imgs([case_input(u8)] * 2, "nl_fast", u8["kwargs"], ctx=ctx, return_n_iter=True)
    assert np.array_equal(stack[0], FIX["exp_u8_b_s5_d3"]) and np.array_equal(stack[1], stack[0]) and list(n_iter) == [0, 0]
    with pytest.raises(NotImplementedError, match="fast_mode=False"):  # ('nl' itself means what it meant)
        amd.gpet_utils.denoise(img, "nl", {}, ctx=ctx)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_bad_arg_with_the_reason(amd, ctx):
    """Argument checks only: nothing is launched."""
    L = amd._lib

    def refused(spec, M, N, reason, pix=L.PIX_F64, null_out=False, null_frame=False):
        buf = np.zeros(max(M * N, 1) if M * N < (1 << 22) else 1)  # (a refused call reads no pixel)
        out = np.empty(buf.size)
        rp = (L._P * 1)(None if null_frame else buf.ctypes.data)
        op = (L._P * 1)(None if null_out else out.ctypes.data)
        with pytest.raises(L.GpetError) as e:
            ctx.check(ctx.lib.gpet_nlmeans_fast_images(ctx.h, rp, 1, pix, M, N, C.byref(spec), 0, op))
        assert e.value.code == L.ERR_BAD_ARG and reason in str(e.value), str(e.value)

    good = dict(patch_size=7, patch_distance=11, h=0.1, sigma=0.0)
    F = L.GpetNlmeansFast
    refused(F(**dict(good, patch_size=1)), 40, 60, "patch_size")
    refused(F(**dict(good, patch_size=16)), 40, 60, "15 x 15")
    refused(F(**dict(good, patch_distance=-1)), 40, 60, "negative")
    refused(F(**dict(good, patch_distance=32)), 80, 80, "above 31")
    refused(F(**dict(good, h=0.0)), 40, 60, "h must")
    refused(F(**dict(good, h=float("inf"))), 40, 60, "h must")
    refused(F(**dict(good, sigma=-0.5)), 40, 60, "sigma")
    refused(F(**dict(good, sigma=float("nan"))), 40, 60, "sigma")
    refused(F(**good), 15, 60, "reflects once")   # pad = 15 needs min(M, N) >= 16
    refused(F(**good), 40, 15, "reflects once")
    refused(F(**good), 40, 60, "pixel type", pix=7)
    refused(F(**good), 40, 60, "null pointer", null_out=True)
    refused(F(**good), 40, 60, "null pointer", null_frame=True)
    # the workspace bound, with the byte counts: 1000 x 1000 at s = 15, d = 31 needs 322790400 bytes for one row of 32 shifts
    refused(F(patch_size=15, patch_distance=31, h=0.1, sigma=0.0), 1000, 1000, "322790400")
    refused(F(patch_size=15, patch_distance=31, h=0.1, sigma=0.0), 1000, 1000, "268435456")
    # through the Python layer the device's refusal comes back as it is
    with pytest.raises(L.GpetError) as e:
        run(amd, ctx, [np.zeros((15, 60))], good)
    assert e.value.code == L.ERR_BAD_ARG and "reflects once" in str(e.value)
    case = BY_NAME["f64_a_s3_d2_sig0"]  # (the context works on)
    assert np.array_equal(run(amd, ctx, [case_input(case)], case["kwargs"])[0], FIX["exp_f64_a_s3_d2_sig0"])


def test_a_refused_set_frame_leaves_a_batch_on_its_old_frames(amd, ctx):
    L = amd._lib
    N = 64
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, 4, 31, "uint8")
    nlf = ("nl_fast", NLF_U8)
    want = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames[:2], grad_kernel=k, denoise=nlf, _ctx=ctx, **KW_RBF)
    want_grad = want._batch.read(L.BUF_GRAD, 1)
    want_traces = want()
    bt = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames[:2], grad_kernel=k, denoise=nlf, _ctx=ctx, **KW_RBF)
    with pytest.raises(L.GpetError) as e:  # (the device refuses: specs made past nlmeans_fast_spec)
        bt.set_frame(raw_imgs=frames[2:], denoise=L.NlmeansFastSpec(5, 3, 0.0, 0.0))
    assert e.value.code == L.ERR_BAD_ARG and "h must" in str(e.value)
    with pytest.raises(L.GpetError) as e:
        bt.set_frame(raw_imgs=frames[2:], denoise=L.NlmeansFastSpec(17, 3, 40.0, 0.0))
    assert e.value.code == L.ERR_BAD_ARG and "15 x 15" in str(e.value)
    with pytest.raises(ValueError, match="fast_mode"):  # (the Python layer)
        bt.set_frame(raw_imgs=frames[2:], denoise=("nl_fast", dict(fast_mode=False)))
    assert np.array_equal(bt._batch.read(L.BUF_GRAD, 1), want_grad)
    for a, b in zip(bt(), want_traces):
        assert np.array_equal(a, b)
    bt._batch.close()
    want._batch.close()


# ---- compositions ------------------------------------------------------------------------------------------------------------------
def test_gradient_images_of_denoised_frames(amd, ctx):
    k = amd.gpet_utils.kernel_builder((11, 5))
    for dtype, kw in (("uint8", NLF_U8), ("float64", NLF)):
        frames, _ = drifting_frames(64, 3, 7, dtype)
        one_pass = amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx, denoise=("nl_fast", kw))
        den = amd.gpet_utils.denoise_imgs(frames, "nl_fast", kw, ctx=ctx)
        assert den.dtype == np.float64 and one_pass.dtype == np.float32
        assert np.array_equal(den[0], R.with_kwargs(R.nlmeans_fast, frames[0], kw))
        assert np.array_equal(one_pass, amd.gpet_utils.comp_grad_imgs(den, k, ctx=ctx))
        assert not np.array_equal(one_pass, amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx))  # (denoising does something)
        two = amd.gpet_utils.comp_grad_imgs(frames, [k, -k], ctx=ctx, denoise=("nl_fast", kw))
        assert np.array_equal(two[:, 0], one_pass) and np.array_equal(two[:, 1], amd.gpet_utils.comp_grad_imgs(den, -k, ctx=ctx))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_batch_with_the_stage_equals_batch_from_denoised_frames(amd, ctx, dtype):
    """Creation, then set_frame with the remembered spec, host frames first and device frames after."""
    N, B = 64, 2
    k = amd.gpet_utils.kernel_builder((11, 5))
    kw = NLF_U8 if dtype == "uint8" else NLF
    frames, init = drifting_frames(N, 3 * B, 21, dtype)
    sets = [frames[0:B], frames[B:2 * B], frames[2 * B:3 * B]]
    dn = lambda s: list(amd.gpet_utils.denoise_imgs(s, "nl_fast", kw, ctx=ctx))  # noqa: E731
    one = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=sets[0], grad_kernel=k, denoise=("nl_fast", kw), return_std=True, _ctx=ctx, **KW_RBF)
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
    frames, init = drifting_frames(N, 4, 51, "uint8")
    dn = lambda s: list(amd.gpet_utils.denoise_imgs(s, "nl_fast", NLF_U8, ctx=ctx))  # noqa: E731
    common = dict(grad_kernel=[k0, k1], kernel_of=[0, 1, 0, 1], image_of=[0, 0, 1, 1], return_std=True, _ctx=ctx)
    one = amd.GP_Edge_Tracing_Batch([init] * 4, None, [3, 4, 5, 6], raw_imgs=frames[:2], denoise=("nl_fast", NLF_U8), **common, **KW_RBF)
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
    frames, init = drifting_frames(N, T, 11, "uint8")
    seeds = [3 + t for t in range(T)]
    ra = amd.trace_sequence(frames, init, n_chains=1, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, denoise=("nl_fast", NLF_U8), **KW_RBF)
    den = list(amd.gpet_utils.denoise_imgs(frames, "nl_fast", NLF_U8, ctx=ctx))
    rb = amd.trace_sequence(den, init, n_chains=1, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, **KW_RBF)
    assert len(ra) == len(rb) == T and all(np.array_equal(x, y) for x, y in zip(ra, rb))


def test_vertical_batch(amd, ctx):
    """orientation='vertical': the frame is denoised as it lies, then the transposed gradient image is made of the result."""
    N, B = 64, 2
    k = amd.gpet_utils.kernel_builder((11, 5), vertical_edges=True)
    frames, init = drifting_frames(N, B, 31, "uint8")
    frames = [np.ascontiguousarray(f.T) for f in frames]
    init = np.ascontiguousarray(init[:, ::-1])
    den = list(amd.gpet_utils.denoise_imgs(frames, "nl_fast", NLF_U8, ctx=ctx))
    one = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=frames, grad_kernel=k, denoise=("nl_fast", NLF_U8), orientation='vertical',
                                    return_std=True, _ctx=ctx, **KW_RBF)
    two = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=den, grad_kernel=k, orientation='vertical', return_std=True, _ctx=ctx,
                                    **KW_RBF)
    assert_same_batch(amd, one, two, "vertical")
    one._batch.close()
    two._batch.close()
