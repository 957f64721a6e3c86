"""GPU tests of the wavelet stage: gpet_utils.denoise / denoise_imgs with 'wavelet' (gpet_wavelet_images), comp_grad_imgs(denoise=),
GP_Edge_Tracing_Batch(raw_imgs=, denoise=) / set_frame, trace_sequence and a vertical batch with ``denoise=('wavelet', kwargs)``.

The reference is tests/golden/wavelet.npz, written by the unmodified reference under scikit-image 0.18.3 / PyWavelets 1.1.1; where
an input or a quantity is not in it, tests/wavelet_ref.py stands in, which tests/test_wavelet_fixture.py pins to the fixture bit
for bit.  Everything is np.array_equal but one quantity: the mean of squares under a BayesShrink threshold is summed in the
device's order (csrc/gpet_wavelet_plan.h), not numpy's, so against the FIXTURE it is held to 2 (n - 1) 2^-53 relative, the
distance any two summation orders of n non-negative terms can be apart (against the restatement, which follows the device's
order, it is equal).  Parity tests therefore inject the fixture's thresholds; compositions use the derived ones on both sides and
are exact by construction."""
import json
import os

import numpy as np
import pytest

from tests import wavelet_ref as R
from tests.test_gpu_denoise import KW_RBF, DeviceFrames, assert_same_batch, drifting_frames

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, "golden", "wavelet.npz"))
CASES = json.loads(str(FIX["cases"]))
RUNS = [c for c in CASES if c["levels"] <= c["max_level"]]  # (the device refuses levels above max_level: one case, tested below)
WV = dict(wavelet="db2", wavelet_levels=2)  # (the compositions)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def case_input(case):
    return FIX["in_" + case["input"]]


def ref_args(case):
    """The restatement's arguments of a case; VisuShrink's constant as THIS process's numpy forms it, which is what the package
    passes to the device (the fixture's, from another numpy, is used where the fixture's thresholds are injected)."""
    kw = case["kwargs"]
    c = float(np.sqrt(2 * np.log(case_input(case).size)))
    return dict(sigma=kw.get("sigma"), mode=kw.get("mode", "soft"), wavelet_levels=kw.get("wavelet_levels"), method=kw.get("method", "BayesShrink"),
                rescale_sigma=kw.get("rescale_sigma", True), ppf=float(FIX["ppf"]), c=c)


def run(amd, ctx, frames, kw, thresholds=None, device_in=False, device_out=False, report=False):
    """gpet_wavelet_images of a list of frames -> (T, M, N) float64, through host or device memory on either side."""
    L = amd._lib
    spec = kw if isinstance(kw, L.WaveletSpec) else L.wavelet_spec(kw, thresholds=thresholds)
    dev = DeviceFrames(ctx, frames) if device_in else None
    buf = L.PreFrames(ctx) if device_out else None
    try:
        if device_in:
            raw = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=frames[0].dtype, shape=frames[0].shape, denoise=spec)
        else:
            raw = L.RawFrames(None, frames=frames, denoise=spec)
        rep = None
        if not device_out:
            out = ctx.wavelet_images(raw, report=report)
            if report:
                out, rep = out
        else:
            M, N = frames[0].shape
            ptrs = buf.reserve(len(frames), M * N * 8)
            if report:
                none, rep = ctx.wavelet_images(raw, out_device_ptrs=ptrs, report=True)
                assert none is None
            else:
                assert ctx.wavelet_images(raw, out_device_ptrs=ptrs) is None
            out = np.empty((len(frames), M, N))
            for g, p in enumerate(ptrs):
                ctx.check(ctx.lib.gpet_dev_copy(ctx.h, out[g].ctypes.data, L._P(p), out[g].nbytes, 1))
        if device_in:
            for i, f in enumerate(frames):
                assert np.array_equal(dev.download(i), f)  # (read where they lie, not written)
        return (out, rep) if report else out
    finally:
        if dev is not None:
            dev.free()
        if buf is not None:
            buf.close()


# ---- against the fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RUNS, ids=[c["name"] for c in RUNS])
def test_equals_the_reference_with_the_fixtures_thresholds(amd, ctx, case):
    """Every case of the fixture the level rule allows: db1 / db2 / db4 / db8 / sym2 / sym4 / coif1; frames from 21 x 19 to
    130 x 150 (several tiles each way, odd band extents); one and two levels; soft / BayesShrink and hard / VisuShrink; u8, u16,
    f64, and f32 against the reference on the widened frame; a saturated region (exact zeros in dd1); a given sigma rescaled
    and as given; 30 x 34 under 16 taps, the deepest input just above the filter."""
    img, exp = case_input(case), FIX["exp_" + case["name"]]
    out = run(amd, ctx, [img], case["kwargs"], thresholds=FIX["thr_" + case["name"]])
    assert out.dtype == np.float64 and out.shape == (1,) + exp.shape
    assert np.array_equal(out[0], exp)


@pytest.mark.parametrize("case", RUNS, ids=[c["name"] for c in RUNS])
def test_own_thresholds_coefficients_and_sigma(amd, ctx, case):
    """The device's own thresholds: coefficients, sigma, thresholds and the output equal the restatement's; the means of squares
    lie within the bound of any two summation orders of the fixture's (numpy's); the thresholds the fixture stores follow from its
    means by the same formula (tests/test_wavelet_fixture.py)."""
    img = case_input(case)
    src = img.astype(np.float64) if case["promote"] else img
    want, info = R.denoise_wavelet(src, FIX["filt_%s_dec_lo" % case["kwargs"]["wavelet"]], return_info=True, **ref_args(case))
    (out, rep) = run(amd, ctx, [img], case["kwargs"], report=True)
    L = case["levels"]
    assert rep["sigma"][0] == info["sigma"] == case["sigma"]
    co = rep["coeffs"][0]
    assert len(co) == L and np.array_equal(co[L - 1]["aa"], info["coeffs"][L - 1]["aa"])
    for l in range(L):
        for k in R.BANDS:
            assert np.array_equal(co[l][k], info["coeffs"][l][k]), (l, k)
            if case["coeffs"]:
                assert np.array_equal(co[l][k], FIX["co_%s_%s%d" % (case["name"], k, l + 1)]), (l, k)
    assert np.array_equal(rep["thresholds"][0], info["thresholds"])
    if case["kwargs"].get("method", "BayesShrink") == "BayesShrink":
        assert np.array_equal(rep["mean_sq"][0], info["ms"])
        ms = FIX["ms_" + case["name"]]
        for l in range(L):
            for b, k in enumerate(R.BANDS):
                n = co[l][k].size
                print(case["name"], l, k, n, abs(rep["mean_sq"][0, l, b] - ms[l, b]) / ms[l, b], R.mean_bound(n))
                assert abs(rep["mean_sq"][0, l, b] - ms[l, b]) <= R.mean_bound(n) * ms[l, b], (l, k)
    else:
        assert rep["mean_sq"] is None and (rep["thresholds"][0] == case["sigma"] * ref_args(case)["c"]).all()
        assert abs(ref_args(case)["c"] - case["c"]) <= 2.0 ** -51 * case["c"]  # (two numpys' log and sqrt: a unit or two in the last place)
    assert np.array_equal(out[0], want)


def test_through_gpet_utils(amd, ctx):
    case = [c for c in CASES if c["name"] == "u8_33x65_db1"][0]
    img = case_input(case)
    want = R.denoise_wavelet(img, FIX["filt_db1_dec_lo"], **ref_args(case))
    out = amd.gpet_utils.denoise(img, "wavelet", dict(wavelet="db1"), ctx=ctx)
    assert out.dtype == np.float64 and np.array_equal(out, want) and out.min() >= 0.0 and out.max() <= 1.0
    stack = amd.gpet_utils.denoise_imgs([img, img[::-1].copy()], "wavelet", dict(wavelet="haar"), ctx=ctx)
    assert np.array_equal(stack[0], want) and np.array_equal(stack[1], R.denoise_wavelet(img[::-1], FIX["filt_db1_dec_lo"], **ref_args(case)))
    out, n_iter = amd.gpet_utils.denoise_imgs([img], "wavelet", dict(wavelet="db1"), ctx=ctx, return_n_iter=True)
    assert np.array_equal(out[0], want) and list(n_iter) == [0]


# ---- launch shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_out", [False, True], ids=["host_out", "device_out"])
@pytest.mark.parametrize("device_in", [False, True], ids=["host_in", "device_in"])
def test_three_frames_in_one_call(amd, ctx, device_in, device_out):
    """Different content per frame; the result of a frame does not depend on how many frames the call holds or where it stands."""
    base = FIX["in_f64_37x50"]
    frames = [base, base[::-1].copy(), np.ascontiguousarray(base[:, ::-1])]
    kw = dict(wavelet="db2")
    out = run(amd, ctx, frames, kw, device_in=device_in, device_out=device_out)
    assert np.array_equal(run(amd, ctx, frames[:1], kw, thresholds=FIX["thr_f64_37x50_db2"], device_in=device_in, device_out=device_out)[0],
                          FIX["exp_f64_37x50_db2"])
    singles = [run(amd, ctx, [f], kw, device_in=device_in, device_out=device_out)[0] for f in frames]
    for g in range(3):
        assert np.array_equal(out[g], singles[g]), g
    back = run(amd, ctx, frames[::-1], kw, device_in=device_in, device_out=device_out)
    for g in range(3):
        assert np.array_equal(back[2 - g], singles[g]), g
    assert not np.array_equal(singles[0], singles[1]) and not np.array_equal(singles[0], singles[2])
    # thresholds per frame: frame 0 with the fixture's, the others with their own
    _, rep = run(amd, ctx, frames, kw, report=True)
    thr = rep["thresholds"].copy()
    thr[0] = FIX["thr_f64_37x50_db2"]
    mixed = run(amd, ctx, frames, kw, thresholds=thr, device_in=device_in, device_out=device_out)
    assert np.array_equal(mixed[0], FIX["exp_f64_37x50_db2"]) and np.array_equal(mixed[1], singles[1]) and np.array_equal(mixed[2], singles[2])


CHUNK_KW = dict(wavelet="db1", wavelet_levels=1)


@pytest.fixture(scope="module")
def chunk_singles(amd, ctx):
    """Four float64 frames of 1024 x 1024 with their one-frame results and reports, computed once."""
    a = np.random.RandomState(3).rand(1024, 1024)
    frames = dict(a=a, b=a[::-1].copy(), c=np.ascontiguousarray(a[:, ::-1]), filler=np.ascontiguousarray(a.T))
    singles = {k: run(amd, ctx, [f], CHUNK_KW, report=True) for k, f in frames.items()}
    assert not np.array_equal(singles["a"][0], singles["b"][0]) and not np.array_equal(singles["a"][0], singles["c"][0])
    return frames, singles


@pytest.mark.parametrize("device,per_chunk", [(False, 10), (True, 32)], ids=["host_in_host_out", "device_in_device_out"])
def test_a_stack_of_two_chunks_with_a_short_last_one(amd, ctx, chunk_singles, device, per_chunk):
    """float64 frames of 1024 x 1024 under db1, one level, keep a pyramid of 8388608 bytes each.  Host in, host out: with 8388608
    staged bytes either way 10 frames fill the 256 MiB of a chunk, so 11 frames are 10 + 1; device in, device out: 32 to a chunk,
    33 frames are 32 + 1 (tests/test_wavelet_plan.py asserts both splits).  The first frame of the first chunk, its last frame and
    the one frame of the last chunk differ; every frame's result, noise level, thresholds, means of squares and coefficients --
    indexed by the frame's number in the whole stack -- are those of its one-frame call, bit for bit."""
    frames, singles = chunk_singles
    names = ["a"] + ["filler"] * (per_chunk - 2) + ["b", "c"]
    out, rep = run(amd, ctx, [frames[k] for k in names], CHUNK_KW, device_in=device, device_out=device, report=True)
    for g, k in enumerate(names):
        want, one = singles[k]
        assert np.array_equal(out[g], want[0]), (g, k)
        assert rep["sigma"][g] == one["sigma"][0], (g, k)
        assert np.array_equal(rep["thresholds"][g], one["thresholds"][0]) and np.array_equal(rep["mean_sq"][g], one["mean_sq"][0]), (g, k)
        assert same(rep["coeffs"][g], one["coeffs"][0]), (g, k)


def test_u8_device_frames_into_device_memory(amd, ctx):
    img = FIX["in_u8_130x150"]
    out = run(amd, ctx, [img, img], dict(wavelet="db2"), thresholds=FIX["thr_u8_130x150_db2"], device_in=True, device_out=True)
    assert np.array_equal(out[0], FIX["exp_u8_130x150_db2"]) and np.array_equal(out[1], out[0])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_all_zero_finest_band_is_an_error_naming_the_frame(amd, ctx):
    L = amd._lib
    good = FIX["in_u8_33x65"]
    flat = np.full_like(good, 128)
    with pytest.raises(L.GpetError) as e:
        ctx.wavelet_images(L.RawFrames(None, frames=[good, flat, good], denoise=("wavelet", dict(wavelet="db1"))))
    assert e.value.code == L.ERR_BAD_ARG and "frame 1" in str(e.value) and "all zero" in str(e.value), str(e.value)
    with pytest.raises(L.GpetError) as e:  # a flat integer frame under a given, rescaled sigma: (max - min) / (max - min)
        ctx.wavelet_images(L.RawFrames(None, frames=[flat], denoise=("wavelet", dict(wavelet="db1", sigma=10.0))))
    assert e.value.code == L.ERR_BAD_ARG and "frame 0" in str(e.value) and "flat" in str(e.value), str(e.value)
    # ... and with sigma as given the flat frame comes back as it is (every detail coefficient is zero), the context works on
    out = ctx.wavelet_images(L.RawFrames(None, frames=[flat], denoise=("wavelet", dict(wavelet="db1", sigma=0.05, rescale_sigma=False))))
    assert np.allclose(out[0], 128 / 255.0, rtol=0, atol=1e-14)
    assert np.array_equal(run(amd, ctx, [good], dict(wavelet="db1"), thresholds=FIX["thr_u8_33x65_db1"])[0], FIX["exp_u8_33x65_db1"])


def test_refusals_return_bad_arg_with_the_reason(amd, ctx):
    L = amd._lib
    above = [c for c in CASES if c["levels"] > c["max_level"]][0]
    with pytest.raises(ValueError, match="above max_level 1"):  # (the Python layer, before the device)
        run(amd, ctx, [case_input(above)], above["kwargs"])
    frame = FIX["in_f64_37x50"]

    def refused(spec, frames, reason):  # (the library itself, past the checks of the Python layer)
        raw = L.RawFrames(np.ones((1, 1)), frames=frames)
        M, N = raw.shape
        out = np.empty((len(frames), M, N))
        op = (L._P * len(frames))(*[out[g].ctypes.data for g in range(len(frames))])
        import ctypes as C
        with pytest.raises(L.GpetError) as e:
            ctx.check(ctx.lib.gpet_wavelet_images(ctx.h, raw.pointer_array(), len(frames), raw.pix, M, N, C.byref(spec.c), raw.flags, op))
        assert e.value.code == L.ERR_BAD_ARG and reason in str(e.value), str(e.value)

    lo = L.wavelet_table()["db8"]
    refused(L.WaveletSpec("db8", lo, 2, 0, 0, float("nan"), True), [FIX["in_f64_48x80"]], "max_level")
    refused(L.WaveletSpec("odd", lo[:3], 0, 0, 0, float("nan"), True), [frame], "taps")
    refused(L.WaveletSpec("db2", L.wavelet_table()["db2"], 0, 2, 0, float("nan"), True), [frame], "mode")
    refused(L.WaveletSpec("db2", L.wavelet_table()["db2"], 0, 0, 0, -1.0, True), [frame], "sigma")
    assert np.array_equal(run(amd, ctx, [frame], dict(wavelet="db2"), thresholds=FIX["thr_f64_37x50_db2"])[0], FIX["exp_f64_37x50_db2"])


# ---- compositions ------------------------------------------------------------------------------------------------------------------
def test_gradient_images_of_denoised_frames(amd, ctx):
    k = amd.gpet_utils.kernel_builder((11, 5))
    for dtype in ("uint8", "float64"):
        frames, _ = drifting_frames(64, 3, 7, dtype)
        one_pass = amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx, denoise=("wavelet", WV))
        den = amd.gpet_utils.denoise_imgs(frames, "wavelet", WV, ctx=ctx)
        assert den.dtype == np.float64 and one_pass.dtype == np.float32
        assert np.array_equal(one_pass, amd.gpet_utils.comp_grad_imgs(den, k, ctx=ctx))
        assert not np.array_equal(one_pass, amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx))  # (denoising does something)
        two = amd.gpet_utils.comp_grad_imgs(frames, [k, -k], ctx=ctx, denoise=("wavelet", WV))
        assert np.array_equal(two[:, 0], one_pass) and np.array_equal(two[:, 1], amd.gpet_utils.comp_grad_imgs(den, -k, ctx=ctx))


def test_image_map_and_two_kernels_then_set_frame_with_a_warm_start(amd, ctx):
    """Two frames, two kernels, four edges: every frame is denoised once, then read through both kernels; set_frame(warm_every=)
    carries the constructor's spec and starts from the device's own traces."""
    N = 64
    k0 = amd.gpet_utils.kernel_builder((11, 5))
    k1 = amd.gpet_utils.kernel_builder((7, 3))
    frames, init = drifting_frames(N, 4, 51, "uint8")
    dn = lambda s: list(amd.gpet_utils.denoise_imgs(s, "wavelet", WV, ctx=ctx))  # noqa: E731
    common = dict(grad_kernel=[k0, k1], kernel_of=[0, 1, 0, 1], image_of=[0, 0, 1, 1], return_std=True, _ctx=ctx)
    one = amd.GP_Edge_Tracing_Batch([init] * 4, None, [3, 4, 5, 6], raw_imgs=frames[:2], denoise=("wavelet", WV), **common, **KW_RBF)
    two = amd.GP_Edge_Tracing_Batch([init] * 4, None, [3, 4, 5, 6], raw_imgs=dn(frames[:2]), **common, **KW_RBF)
    assert one._batch.n_img == two._batch.n_img == 4
    assert_same_batch(amd, one, two, "image map, construction")
    one.set_frame(raw_imgs=frames[2:], seeds=[7, 8, 9, 10], warm_every=16)
    two.set_frame(raw_imgs=dn(frames[2:]), seeds=[7, 8, 9, 10], warm_every=16)
    assert_same_batch(amd, one, two, "image map, set_frame with a warm start")
    one._batch.close()
    two._batch.close()


def test_sequence_of_three_frames(amd, ctx):
    N, T = 64, 3
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, T, 11, "uint8")
    seeds = [3 + t for t in range(T)]
    ra = amd.trace_sequence(frames, init, n_chains=1, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, denoise=("wavelet", WV), **KW_RBF)
    den = list(amd.gpet_utils.denoise_imgs(frames, "wavelet", WV, ctx=ctx))
    rb = amd.trace_sequence(den, init, n_chains=1, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, **KW_RBF)
    assert len(ra) == len(rb) == T and all(np.array_equal(x, y) for x, y in zip(ra, rb))


def test_vertical_batch(amd, ctx):
    """orientation='vertical': the frame is denoised as it lies, then the transposed gradient image is made of the result."""
    N, B = 64, 2
    k = amd.gpet_utils.kernel_builder((11, 5), vertical_edges=True)
    frames, init = drifting_frames(N, B, 31, "uint8")
    frames = [np.ascontiguousarray(f.T) for f in frames]
    init = np.ascontiguousarray(init[:, ::-1])
    den = list(amd.gpet_utils.denoise_imgs(frames, "wavelet", WV, ctx=ctx))
    one = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=frames, grad_kernel=k, denoise=("wavelet", WV), orientation='vertical',
                                    return_std=True, _ctx=ctx, **KW_RBF)
    two = amd.GP_Edge_Tracing_Batch([init] * B, None, [3, 4], raw_imgs=den, grad_kernel=k, orientation='vertical', return_std=True, _ctx=ctx,
                                    **KW_RBF)
    assert_same_batch(amd, one, two, "vertical")
    one._batch.close()
    two._batch.close()


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_trace_ensemble(amd, ctx):
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(64, 1, 71, "uint8")
    den = amd.gpet_utils.denoise_imgs(frames, "wavelet", WV, ctx=ctx)[0]
    kw = dict(KW_RBF, return_std=True, _ctx=ctx, grad_kernel=k)
    got = amd.trace_ensemble(init, None, [1, 2, 3], raw_imgs=frames[0], denoise=("wavelet", WV), **kw)
    want = amd.trace_ensemble(init, None, [1, 2, 3], raw_imgs=den, **kw)
    assert got["medoid"] >= 0 and len(got["members"]) == 3 and same(got, want)
