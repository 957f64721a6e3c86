"""GPU tests of the split-Bregman stage: gpet_utils.denoise / denoise_imgs with 'tvb' (gpet_tvb_images), comp_grad_imgs(denoise=),
GP_Edge_Tracing_Batch(raw_imgs=, denoise=) / set_frame, trace_sequence and a vertical batch with ``denoise=('tvb', kwargs)``.

The reference is tests/golden/tvb.npz, written by the unmodified reference under scikit-image 0.18.3; where an input is not in it,
tests/tvb_ref.py stands in, which tests/test_tvb_fixture.py pins to the fixture bit for bit.  Everything is np.array_equal: the
one deviation of the stage, the order in which the squared changes under the stopping rule are added, can only change a sweep
count, and only where a sweep's rmse lies within 2 (n - 1) 2^-53 relative of eps -- the fixture's maker asserts that no case is
that close, and the sweep counts are compared as well."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import tvb_ref as R
from tests.test_gpu_denoise import KW_RBF, DeviceFrames, assert_same_batch, drifting_frames

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "tvb.npz"))
CASES = json.loads(str(FIX["cases"]))
BY_NAME = {c["name"]: c for c in CASES}
TVB = dict(weight=5, max_iter=8)  # (the compositions)


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
    """gpet_tvb_images of a list of frames -> ((T, M, N) float64, sweeps per frame), through host or device memory on either side."""
    L = amd._lib
    dev = DeviceFrames(ctx, frames) if device_in else None
    buf = L.PreFrames(ctx) if device_out else None
    try:
        if device_in:
            raw = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=frames[0].dtype, shape=frames[0].shape, denoise=("tvb", kw))
        else:
            raw = L.RawFrames(None, frames=frames, denoise=("tvb", kw))
        if not device_out:
            out, n_iter = ctx.tvb_images(raw, return_n_iter=True)
        else:
            M, N = frames[0].shape
            ptrs = buf.reserve(len(frames), M * N * 8)
            none, n_iter = ctx.tvb_images(raw, out_device_ptrs=ptrs, return_n_iter=True)
            assert none is None
            out = np.empty((len(frames), M, N))
            for g, p in enumerate(ptrs):
                ctx.check(ctx.lib.gpet_dev_copy(ctx.h, out[g].ctypes.data, L._P(p), out[g].nbytes, 1))
        if device_in:
            for i, f in enumerate(frames):
                assert np.array_equal(dev.download(i), f)  # (read where they lie, not written)
        return out, n_iter
    finally:
        if dev is not None:
            dev.free()
        if buf is not None:
            buf.close()


# ---- against the fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_equals_the_reference(amd, ctx, case):
    """Every case of the fixture: 2 x 2, 2 x 9 and 9 x 2 (the smallest frames the library takes); isotropic and anisotropic; stops
    by eps and by max_iter; 65 x 70 and 70 x 65 (a diagonal longer than one wave, taller and wider); u8, u16, f64, and f32 against
    the reference on the widened frame; weights 0.5, 5 and 10."""
    img, exp = case_input(case), FIX["exp_" + case["name"]]
    out, n_iter = run(amd, ctx, [img], case["kwargs"])
    assert out.dtype == np.float64 and out.shape == (1,) + exp.shape and n_iter.dtype == np.int32
    assert list(n_iter) == [case["n_iter"]]
    assert np.array_equal(out[0], exp)


def test_a_lane_owns_several_cells(amd, ctx):
    """(threads + 5) x (threads + 9): the longest diagonals have more cells than the workgroup has lanes."""
    T = R.THREADS
    rs = np.random.RandomState(41)
    img = np.rint(rs.rand(T + 5, T + 9) * 1024) / 1024
    want, info = R.denoise_tv_bregman(img, 5.0, max_iter=2, eps=0, form="diagonal", order="device", return_info=True)
    out, n_iter = run(amd, ctx, [img], dict(weight=5, max_iter=2, eps=0))
    assert list(n_iter) == [2] == [info["n_iter"]]
    assert np.array_equal(out[0], want)


def test_the_largest_smaller_extent(amd, ctx):
    """768 x 770, min(M, N) at the plan's bound: the hand-over and the lanes' sums fill the 64 KB of LDS exactly.  One sweep, which
    does not depend on the order of acc."""
    M, N = R.DIAG_MAX, R.DIAG_MAX + 2
    img = np.random.RandomState(42).randint(0, 256, (M, N)).astype(np.uint8)
    x, u, dx, dy, bx, by = R._start(img)
    R.sweep_diagonal(x, u, dx, dy, bx, by, 5.0, True)
    out, n_iter = run(amd, ctx, [img], dict(weight=5, max_iter=1))
    assert list(n_iter) == [1] and np.array_equal(out[0], u[1:M + 1, 1:N + 1])


@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("device_in", [False, True], ids=["host_in", "device_in"])
def test_three_frames_that_stop_after_different_sweeps(amd, ctx, device_in, device_out):
    """The sweep counts are per frame: a finished frame's workgroup exits while the others go on."""
    names = ["f64_9x13", "f64_9x13_b", "f64_9x13_c"]
    counts = [BY_NAME[n]["n_iter"] for n in names]
    assert len(set(counts)) == 3
    out, n_iter = run(amd, ctx, [FIX["in_" + n] for n in names], dict(weight=5), device_in=device_in, device_out=device_out)
    assert list(n_iter) == counts
    for g, n in enumerate(names):
        assert np.array_equal(out[g], FIX["exp_" + n]), n


def test_state_is_carried_across_launches(amd, ctx):
    """max_iter = 5 with four sweeps to a launch, and the 17 x 17 case of seven sweeps: two launches each."""
    assert R.SWEEPS_PER_LAUNCH < 5
    img = FIX["in_f64_17x17"]
    want, info = R.denoise_tv_bregman(img, 5.0, max_iter=5, eps=0, form="diagonal", order="device", return_info=True)
    out, n_iter = run(amd, ctx, [img], dict(weight=5, max_iter=5, eps=0))
    assert list(n_iter) == [5] and np.array_equal(out[0], want)
    assert not np.array_equal(want, FIX["exp_f64_17x17_7sweeps"])


def test_u8_device_frames_into_device_memory_without_a_wait(amd, ctx):
    """Frames and outputs on the device, no sweep counts asked for: the call enqueues; the copy that follows on the stream reads it."""
    L = amd._lib
    img = FIX["in_u8_33x65"]
    dev, buf = DeviceFrames(ctx, [img, img]), L.PreFrames(ctx)
    try:
        raw = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=img.dtype, shape=img.shape, denoise=("tvb", BY_NAME["u8_33x65"]["kwargs"]))
        ptrs = buf.reserve(2, img.size * 8)
        assert ctx.tvb_images(raw, out_device_ptrs=ptrs) is None
        for p in ptrs:
            out = np.empty(img.shape)
            ctx.check(ctx.lib.gpet_dev_copy(ctx.h, out.ctypes.data, L._P(p), out.nbytes, 1))
            assert np.array_equal(out, FIX["exp_u8_33x65"])
    finally:
        dev.free()
        buf.close()


# ---- more than one chunk -----------------------------------------------------------------------------------------------------------
CHUNK_KW = dict(weight=5, max_iter=3, eps=1e-3)


@pytest.fixture(scope="module")
def chunk_singles(amd, ctx):
    """Four float64 frames of 500 x 500 with their one-frame results, computed once: a flat frame (no change in its first sweep:
    one sweep), a smooth one (rmse 1.4e-3, 8.6e-4: two), a noisy one and the filler between them (rmse above 1e-2 throughout: all
    three) -- every rmse is far from eps = 1e-3."""
    M = N = 500
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:M, 0:N]
    smooth = 0.5 + 0.25 * np.sin(xx / 40.0) * np.cos(yy / 55.0)
    frames = dict(flat=np.full((M, N), 0.5), smooth=smooth, noisy=np.clip(smooth + rs.normal(0.0, 0.1, (M, N)), 0.0, 1.0), filler=rs.rand(M, N))
    singles = {k: run(amd, ctx, [f], CHUNK_KW) for k, f in frames.items()}
    assert [int(singles[k][1][0]) for k in ("flat", "smooth", "noisy", "filler")] == [1, 2, 3, 3]
    return frames, singles


@pytest.mark.parametrize("device,per_chunk", [(False, 16), (True, 22)], ids=["host_in_host_out", "device_in_device_out"])
def test_a_stack_of_two_chunks_with_a_short_last_one(amd, ctx, chunk_singles, device, per_chunk):
    """float64 frames of 500 x 500 keep 12096256 bytes of workspace each.  Host in, host out: with 2000128 staged bytes either way
    16 frames fill the 256 MiB of a chunk, so 17 frames are 16 + 1; device in, device out: 22 to a chunk, 23 frames are 22 + 1
    (tests/test_tvb_plan.py asserts both splits).  The first frame of the first chunk, its last frame and the one frame of the last
    chunk stop after 1, 2 and 3 sweeps; every frame's result and sweep count are those of its one-frame call, bit for bit."""
    frames, singles = chunk_singles
    names = ["flat"] + ["filler"] * (per_chunk - 2) + ["smooth", "noisy"]
    out, n_iter = run(amd, ctx, [frames[k] for k in names], CHUNK_KW, device_in=device, device_out=device)
    assert list(n_iter) == [int(singles[k][1][0]) for k in names]
    assert (n_iter[0], n_iter[per_chunk - 1], n_iter[per_chunk]) == (1, 2, 3)
    for g, k in enumerate(names):
        assert np.array_equal(out[g], singles[k][0][0]), (g, k)


def test_through_gpet_utils(amd, ctx):
    case = BY_NAME["u8_33x65"]
    img, want = case_input(case), FIX["exp_u8_33x65"]
    out = amd.gpet_utils.denoise(img, "tvb", case["kwargs"], ctx=ctx)
    assert out.dtype == np.float64 and np.array_equal(out, want)
    flipped = img[::-1].copy()
    stack, n_iter = amd.gpet_utils.denoise_imgs([img, flipped], "tvb", case["kwargs"], ctx=ctx, return_n_iter=True)
    want1, info = R.denoise_tv_bregman(flipped, form="diagonal", order="device", return_info=True, **case["kwargs"])
    assert np.array_equal(stack[0], want) and np.array_equal(stack[1], want1) and list(n_iter) == [case["n_iter"], info["n_iter"]]
    assert np.array_equal(amd.gpet_utils.denoise_imgs([img], "tvb", case["kwargs"], ctx=ctx)[0], want)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_bad_arg_with_the_reason(amd, ctx):
    """Argument checks only: nothing is launched."""
    L = amd._lib
    frame = FIX["in_f64_9x13"]

    def refused(spec, M, N, reason, null_out=False):
        buf = np.zeros(max(M * N, 1))
        out = np.empty(max(M * N, 1))
        rp = (L._P * 1)(buf.ctypes.data)
        op = None if null_out else (L._P * 1)(out.ctypes.data)
        with pytest.raises(L.GpetError) as e:
            ctx.check(ctx.lib.gpet_tvb_images(ctx.h, rp, 1, L.PIX_F64, M, N, C.byref(spec), 0, op, None))
        assert e.value.code == L.ERR_BAD_ARG and reason in str(e.value), str(e.value)

    good = dict(weight=5.0, eps=1e-3, max_iter=100, isotropic=1)
    refused(L.GpetTvb(**good), 1, 13, "2 x 2")
    refused(L.GpetTvb(**good), 9, 1, "2 x 2")
    refused(L.GpetTvb(**dict(good, weight=0.0)), 9, 13, "weight")
    refused(L.GpetTvb(**dict(good, max_iter=0)), 9, 13, "max_iter")
    refused(L.GpetTvb(**dict(good, eps=-1.0)), 9, 13, "eps")
    refused(L.GpetTvb(**good), 9, 13, "out is a null pointer", null_out=True)
    with pytest.raises(ValueError, match="2 x 2"):  # (the Python layer, before the device)
        L.RawFrames(None, frames=[np.zeros((1, 9))], denoise=("tvb", dict(weight=5)))
    out, n_iter = run(amd, ctx, [frame], dict(weight=5))  # (the context works on)
    assert np.array_equal(out[0], FIX["exp_f64_9x13"])


# ---- compositions ------------------------------------------------------------------------------------------------------------------
def test_gradient_images_of_denoised_frames(amd, ctx):
    k = amd.gpet_utils.kernel_builder((11, 5))
    for dtype in ("uint8", "float64"):
        frames, _ = drifting_frames(64, 3, 7, dtype)
        one_pass = amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx, denoise=("tvb", TVB))
        den = amd.gpet_utils.denoise_imgs(frames, "tvb", TVB, ctx=ctx)
        assert den.dtype == np.float64 and one_pass.dtype == np.float32
        assert np.array_equal(den[0], R.denoise_tv_bregman(frames[0], form="diagonal", order="device", **TVB))
        assert np.array_equal(one_pass, amd.gpet_utils.comp_grad_imgs(den, k, ctx=ctx))
        assert not np.array_equal(one_pass, amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx))  # (denoising does something)


def test_two_edges_then_set_frame_with_a_warm_start(amd, ctx):
    N = 64
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, 4, 51, "uint8")
    dn = lambda s: list(amd.gpet_utils.denoise_imgs(s, "tvb", TVB, ctx=ctx))  # noqa: E731
    common = dict(grad_kernel=k, return_std=True, _ctx=ctx)
    one = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames[:2], denoise=("tvb", TVB), **common, **KW_RBF)
    two = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=dn(frames[:2]), **common, **KW_RBF)
    assert_same_batch(amd, one, two, "construction")
    one.set_frame(raw_imgs=frames[2:], seeds=[7, 8], warm_every=16)
    two.set_frame(raw_imgs=dn(frames[2:]), seeds=[7, 8], warm_every=16)
    assert_same_batch(amd, one, two, "set_frame with a warm start")
    one._batch.close()
    two._batch.close()


def test_sequence_of_three_frames(amd, ctx):
    N, T = 64, 3
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, T, 11, "uint8")
    seeds = [3 + t for t in range(T)]
    ra = amd.trace_sequence(frames, init, n_chains=1, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, denoise=("tvb", TVB), **KW_RBF)
    den = list(amd.gpet_utils.denoise_imgs(frames, "tvb", TVB, ctx=ctx))
    rb = amd.trace_sequence(den, init, n_chains=1, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, **KW_RBF)
    assert len(ra) == len(rb) == T and all(np.array_equal(x, y) for x, y in zip(ra, rb))


def test_vertical_batch(amd, ctx):
    """orientation='vertical': the frame is denoised as it lies, then the transposed gradient image is made of the result."""
    N, B = 64, 2
    k = amd.gpet_utils.kernel_builder((11, 5), vertical_edges=True)
    frames, init = drifting_frames(N, B, 31, "uint8")
    frames = [np.ascontiguousarray(f.T) for f in frames]
    init = np.ascontiguousarray(init[:, ::-1])
    den = list(amd.gpet_utils.denoise_imgs(frames, "tvb", TVB, ctx=ctx))
    one = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=frames, grad_kernel=k, denoise=("tvb", TVB), orientation='vertical',
                                    return_std=True, _ctx=ctx, **KW_RBF)
    two = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=den, grad_kernel=k, orientation='vertical', return_std=True, _ctx=ctx,
                                    **KW_RBF)
    assert_same_batch(amd, one, two, "vertical")
    one._batch.close()
    two._batch.close()
