"""GPU tests of the polar unwrap (gpet_polar_images, csrc/gpet_k_polar.inc) and of ``polar=`` on everything that takes raw frames.

The unwrap itself is pinned to the bit against tests/polar_ref.py, the rule restated with numpy float64.  Everything behind it is
pinned by the definition: ``polar=P`` together with anything else equals the same call on ``unwrap_polar_imgs(frames, **P)`` given
as float64 frames, bit for bit.  The closed contour's quality is gated on the CPU oracle's trace of the same unwrapped frame
(tests/golden/polar_disc.npz, written by tests/golden/make_polar_fixture.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import polar_ref as R
from tests.test_gpu_denoise import DeviceFrames, assert_same_batch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
SHAPE = (37, 53)
CORNER = (46.3, 4.6)  # a non-integer centre near the upper right corner: rays leave over the right and the upper border
# (frame shape, centres, n_r, n_theta, r0, dr, theta0, pad, number of frames)
UNWRAP_CASES = {
    "inside_one_wave": (SHAPE, CORNER, 40, 48, 0.0, 0.75, 0.0, 5, 1),            # W = 59
    "crosses_a_wave": (SHAPE, CORNER, 40, 70, 0.0, 0.75, 0.4, 3, 1),             # W = 77
    "one_row": (SHAPE, (20.25, 17.5), 1, 48, 6.5, 1.0, 0.0, 5, 1),               # n_r = 1
    "pad_is_n_theta": (SHAPE, (20.25, 17.5), 9, 12, 1.0, 1.5, 0.0, 12, 1),       # W = 37
    "frame_2x2": ((2, 2), (0.4, 0.7), 5, 8, 0.0, 0.3, 0.0, 1, 1),
    "three_centres": (SHAPE, [(46.3, 4.6), (20.25, 17.5), (3.0, 30.0)], 40, 48, 0.0, 0.75, 0.0, 5, 3),
}


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def spec_kw(case):
    shape, centre, n_r, n_theta, r0, dr, theta0, pad, T = case
    return dict(centre=centre, n_r=n_r, n_theta=n_theta, r0=r0, dr=dr, theta0=theta0, pad=pad)


# ---- 1. the unwrap against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", list(UNWRAP_CASES))
def test_unwrap_equals_the_restated_rule(amd, ctx, name, dtype):
    case = UNWRAP_CASES[name]
    shape, T, kw = case[0], case[8], spec_kw(case)
    frames = [R.frame_of(dtype, shape, 100 + t) for t in range(T)]
    ref = R.unwrap(frames, **kw)
    got = amd.gpet_utils.unwrap_polar_imgs(frames, ctx=ctx, **kw)
    assert got.dtype == np.float64 and got.shape == (T, kw["n_r"], kw["n_theta"] + 1 + 2 * kw["pad"])
    assert np.array_equal(got, ref)
    R.seam_identities(got, kw["n_theta"], kw["pad"])
    # frames already on the device, results into device memory: nothing passes through the host
    L = amd._lib
    dev = DeviceFrames(ctx, frames)
    out = DeviceFrames(ctx, [np.zeros(ref.shape[1:]) for _ in range(T)])
    try:
        raw = L.RawFrames(None, device_ptrs=dev.ptrs, dtype=dtype, shape=shape, polar=kw)
        assert ctx.polar_images(raw, out_device_ptrs=out.ptrs) is None
        assert np.array_equal(np.stack([out.download(t) for t in range(T)]), ref)
        assert np.array_equal(ctx.polar_images(raw), ref)  # (device frames, host results)
    finally:
        dev.free()
        out.free()


def test_integer_centre_reads_the_frames_own_pixels(amd, ctx):
    for dtype in DTYPES:
        frame = R.frame_of(dtype, (21, 30), 5)
        got = amd.gpet_utils.unwrap_polar_imgs([frame], (11, 6), 9, 8, ctx=ctx)[0]
        assert np.array_equal(got[:, 0], frame[6, 11:20].astype(np.float64))  # angle 0: frame[cy, cx + i]
        assert np.array_equal(got[:, 8], got[:, 0])


# ---- 2. composition ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def comp(amd, ctx):
    """Three uint8 frames, three centres, the spec without pad (it follows the kernel), and the reference unwraps by pad."""
    frames = [R.frame_of(np.uint8, SHAPE, 200 + t) for t in range(3)]
    pol = dict(centre=[(46.3, 4.6), (20.25, 17.5), (30.0, 20.0)], n_r=24, n_theta=40, r0=0.0, dr=0.75, theta0=0.1)
    return frames, pol, lambda pad: R.unwrap(frames, pad=pad, **pol)


def test_comp_grad_imgs_on_polar_frames(amd, ctx, comp):
    U = amd.gpet_utils
    frames, pol, flat = comp
    K = U.kernel_builder((5, 3))
    got = U.comp_grad_imgs(frames, K, ctx=ctx, polar=pol)  # (pad = 3 // 2)
    assert got.shape == (3, 24, 40 + 1 + 2) and np.array_equal(got, U.comp_grad_imgs(flat(1), K, ctx=ctx))
    assert np.array_equal(got, U.comp_grad_imgs(U.unwrap_polar_imgs(frames, ctx=ctx, pad=1, **pol), K, ctx=ctx))
    # the pad gives the convolution periodic data: the seam columns of the gradient images agree
    assert np.array_equal(got[..., 1], got[..., 41])
    # two kernels (the wider decides the pad), an in-pass technique
    Ks = [K, U.kernel_builder((3, 7))]
    dn = ("median", dict(size=3))
    got = U.comp_grad_imgs(frames, Ks, ctx=ctx, denoise=dn, polar=pol)
    assert got.shape == (3, 2, 24, 40 + 1 + 6) and np.array_equal(got, U.comp_grad_imgs(flat(3), Ks, ctx=ctx, denoise=dn))
    # an explicit pad is kept
    got = U.comp_grad_imgs(frames, K, ctx=ctx, polar=dict(pol, pad=6))
    assert np.array_equal(got, U.comp_grad_imgs(flat(6), K, ctx=ctx))


def test_a_stage_of_its_own_runs_on_the_unwrapped_frames(amd, ctx, comp):
    U = amd.gpet_utils
    frames, pol, flat = comp
    K = U.kernel_builder((5, 3))
    # a small frame: the fewest angles there are, and six rows -- the stage itself takes two (its patch radius is 1), but the (5, 3)
    # kernel's gradient image of two rows is all zero, and its min-max normalisation then NaN on both sides
    small = dict(pol, n_r=6, n_theta=4, pad=1)
    nl = ("nl", dict(patch_size=3, patch_distance=2, h=25.0, fast_mode=False))
    want = U.comp_grad_imgs(R.unwrap(frames, **small), K, ctx=ctx, denoise=nl)
    assert want.shape == (3, 6, 7) and np.isfinite(want).all() and want.max() == 1.0 and np.array_equal(U.comp_grad_imgs(frames, K, ctx=ctx, denoise=nl, polar=small), want)
    got = U.denoise_imgs(frames, *nl, ctx=ctx, polar=dict(pol, pad=2))
    assert got.dtype == np.float64 and np.array_equal(got, U.denoise_imgs(flat(2), *nl, ctx=ctx))
    # an in-pass technique alone: pad defaults to 0 without a kernel
    got = U.denoise_imgs(frames, "gaussian", dict(sigma=1.0), ctx=ctx, polar=pol)
    assert np.array_equal(got, U.denoise_imgs(flat(0), "gaussian", dict(sigma=1.0), ctx=ctx))


STAGES = {"nl": ("nlmeans_images", dict(patch_size=3, patch_distance=2, h=25.0, fast_mode=False)),
          "nl_fast": ("nlmeans_fast_images", dict(patch_size=3, patch_distance=1, h=25.0)),
          "wavelet": ("wavelet_images", dict(wavelet="db1")),
          "tvb": ("tvb_images", dict(weight=5, max_iter=7))}


@pytest.mark.parametrize("technique", list(STAGES))
def test_every_stage_of_its_own_is_reached_through_the_registry(amd, ctx, comp, technique):
    """The two routes to a stage that no other test takes for all four: the registry's (denoise_images and the raw-frame path, the
    polar unwrap first) against the stage's own public method on the unwrapped frames.  Both sides run the same kernels: equality
    says the dispatch reaches the right call with the right arguments, not that the stage is right (its fixture tests say that).
    6 x 7 frames: the smallest all four stages take ('nl_fast' needs more than 1 + 1 + 1 rows)."""
    U, L = amd.gpet_utils, amd._lib
    frames, pol, flat = comp
    method, kw = STAGES[technique]
    small = dict(pol, n_r=6, n_theta=4, pad=1)
    unwrapped = U.unwrap_polar_imgs(frames, ctx=ctx, **small)
    assert unwrapped.shape == (3, 6, 7)
    got, n_iter = U.denoise_imgs(frames, technique, kw, ctx=ctx, polar=small, return_n_iter=True)
    raw = L.RawFrames(None, frames=unwrapped, denoise=(technique, kw))
    if technique == "tvb":
        want, sweeps = ctx.tvb_images(raw, return_n_iter=True)
        assert sweeps.dtype == np.int32 and sweeps.shape == (3,) and sweeps.any()  # (max_iter is 7)
    else:
        want, sweeps = getattr(ctx, method)(raw), np.zeros(3, dtype=np.int32)
    assert want.dtype == np.float64 and want.shape == (3, 6, 7) and np.isfinite(want).all() and not np.array_equal(want, unwrapped)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert n_iter.dtype == np.int32 and np.array_equal(n_iter, sweeps)
    K = U.kernel_builder((5, 3))
    grad = U.comp_grad_imgs(unwrapped, K, ctx=ctx, denoise=(technique, kw))
    assert np.isfinite(grad).all() and np.array_equal(U.comp_grad_imgs(frames, K, ctx=ctx, denoise=(technique, kw), polar=small), grad)


# ---- 3. the batch --------------------------------------------------------------------------------------------------------------------
KW = dict(kernel_options={"kernel": "RBF", "sigma_f": 10, "length_scale": 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
INNER, OUTER = (14.0, 2.0), (26.0, 4.0)


def test_batch_on_polar_frames_equals_the_batch_on_unwrapped_frames(amd, ctx):
    """Two frames, two edges each (the two outlines of a nested lumen) through an image map: construction, the next frames with a
    device warm start, and moved centres."""
    U, L = amd.gpet_utils, amd._lib
    K = U.kernel_builder((5, 3))
    c0, c1, c2 = [(47.5, 48.25), (49.0, 46.5)], [(47.0, 48.0), (49.5, 47.0)], [(48.5, 47.75), (48.0, 47.5)]
    f0 = [R.disc_frame((96, 96), c, seed=31 + i) for i, c in enumerate(c0)]
    f1 = [R.disc_frame((96, 96), c, seed=41 + i) for i, c in enumerate(c1)]
    f2 = [R.disc_frame((96, 96), c, seed=51 + i) for i, c in enumerate(c2)]
    pol = dict(centre=c0, n_r=40, n_theta=90)
    flat = lambda fr, c: R.unwrap(fr, c, 40, 90, pad=1)  # noqa: E731 (pad: half the kernel's width)
    inits = [U.closed_init(int(round(R.outline(0.0, *o))), dict(pol, pad=1)) for _ in range(2) for o in (INNER, OUTER)]
    args = dict(seeds=[3, 4, 5, 6], grad_kernel=K, image_of=[0, 0, 1, 1], return_std=True, _ctx=ctx, **KW)
    a = amd.GP_Edge_Tracing_Batch(inits, None, raw_imgs=f0, polar=pol, **args)
    b = amd.GP_Edge_Tracing_Batch(inits, None, raw_imgs=list(flat(f0, c0)), **args)
    assert a.polar.pad == 1 and a._batch.frame_shape == (40, 93) == b._batch.frame_shape
    assert_same_batch(amd, a, b, "construction")
    a.set_frame(raw_imgs=f1, warm_every=10, polar=dict(centre=c1))
    b.set_frame(raw_imgs=list(flat(f1, c1)), warm_every=10)
    assert_same_batch(amd, a, b, "next frames, device warm start, centres replaced")
    a.set_frame(raw_imgs=f2, warm_every=10)  # (the spec is kept: the centres of the last call)
    b.set_frame(raw_imgs=list(flat(f2, c1)), warm_every=10)
    assert_same_batch(amd, a, b, "next frames, spec kept")
    a.set_frame(raw_imgs=f2, warm_every=10, polar=dict(centre=c2))
    b.set_frame(raw_imgs=list(flat(f2, c2)), warm_every=10)
    assert_same_batch(amd, a, b, "centres moved")
    # device frames: grad_shape is the frames' own shape
    dev = DeviceFrames(ctx, f0)
    try:
        a.set_frame(raw_device_ptrs=dev.ptrs, raw_dtype=np.uint8, next_frame=False, polar=dict(centre=c0))
        b.set_frame(raw_imgs=list(flat(f0, c0)), next_frame=False)
        assert_same_batch(amd, a, b, "device frames")
    finally:
        dev.free()
    # refusals leave the batch as it was
    for change in (dict(n_r=41), dict(n_theta=91), dict(pad=2)):
        with pytest.raises(ValueError, match="cannot change the shape"):
            a.set_frame(raw_imgs=f1, polar=dict(centre=c1, **change))
    with pytest.raises(ValueError, match="replaces the centres only"):
        a.set_frame(raw_imgs=f1, polar=dict(centre=c1, dr=0.5))
    with pytest.raises(ValueError, match="polar needs raw frames"):
        amd.GP_Edge_Tracing_Batch(inits, [np.zeros((40, 93), dtype=np.float32)] * 2, polar=pol, **dict(args, grad_kernel=None))
    with pytest.raises(ValueError, match="orientation='vertical'"):
        amd.GP_Edge_Tracing_Batch(inits, None, raw_imgs=f0, polar=pol, orientation="vertical", **args)
    with pytest.raises(ValueError, match="not built on polar frames"):
        b.set_frame(raw_imgs=list(flat(f1, c1)), polar=dict(centre=c1))
    a.set_frame(raw_imgs=f0, next_frame=False, polar=dict(centre=c0))
    b.set_frame(raw_imgs=list(flat(f0, c0)), next_frame=False)
    assert_same_batch(amd, a, b, "after the refusals")


def test_sequence_with_a_centre_per_frame(amd, ctx):
    U = amd.gpet_utils
    from gaussian_process_edge_trace_amd.sequence import trace_sequence
    K = U.kernel_builder((5, 3))
    centres = [(47.5, 48.25), (48.0, 47.5), (48.5, 47.0)]
    frames = [R.disc_frame((96, 96), c, outlines=(OUTER,), levels=(40.0, 200.0), seed=61 + i) for i, c in enumerate(centres)]
    pol = dict(centre=centres, n_r=40, n_theta=90)
    init = U.closed_init(30, dict(pol, pad=1))
    got = trace_sequence(frames, init, seed=9, grad_kernel=K, polar=pol, _ctx=ctx, **KW)
    want = trace_sequence(list(R.unwrap(frames, centres, 40, 90, pad=1)), init, seed=9, grad_kernel=K, _ctx=ctx, **KW)
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want))


# ---- 4. the closed contour -----------------------------------------------------------------------------------------------------------
def test_closed_contour_against_the_oracle(amd, ctx):
    """The device trace's mean absolute radial error may exceed the oracle's by at most one pixel: traces are integer rows and a
    near-tie settles one row either way.  Measured on an MI355X when the test was written: the two traces are EQUAL (5 iterations
    each, 0.7742 px both), so equality is asserted as well."""
    U = amd.gpet_utils
    g = np.load(os.path.join(GOLDEN, "polar_disc.npz"))
    pol, kw = json.loads(str(g["polar"])), json.loads(str(g["kw"]))
    centre, outer, init = tuple(g["centre"]), tuple(g["outer"]), g["init"]
    given = dict(pol, centre=centre, pad=None)  # (the pad is left to the kernel: (5, 3) gives the fixture's 1)
    bt = amd.GP_Edge_Tracing_Batch([init], None, [int(g["seed"])], raw_imgs=g["frame"], grad_kernel=g["kernel"], polar=given, return_std=True,
                                   _ctx=ctx, **kw)
    assert bt.polar.pad == pol["pad"] and np.array_equal(U.closed_init(init[0, 1], bt.polar), init)
    trace, (lower, upper) = bt()[0]
    assert trace.shape == (pol["n_theta"] + 1, 2) and trace[0, 1] == pol["pad"] and trace[-1, 1] == pol["pad"] + pol["n_theta"]
    assert trace[0, 0] == init[0, 1] and trace[-1, 0] == init[1, 1]  # closed: both ends on the init row
    xy, (xy_lo, xy_hi) = U.polar_trace_xy((trace, (lower, upper)), bt.polar)
    assert np.array_equal(xy[0], xy[-1])  # one point, to the bit
    assert xy.shape == (pol["n_theta"] + 1, 2) and xy_lo.shape == xy.shape == xy_hi.shape
    err, err_oracle = R.radial_error(trace, pol, *outer), float(g["radial_error"])
    same = np.array_equal(trace, g["trace"])
    print("closed contour: device %.4f px, oracle %.4f px, traces equal: %s, iterations %s against %d"
          % (err, err_oracle, same, bt.timings["iters"], int(g["n_iter"])))
    assert err <= err_oracle + 1.0
    assert same and bt.timings["iters"] == [int(g["n_iter"])]
    # the points lie around the centre at the traced radii
    assert np.allclose(np.hypot(xy[:, 0] - centre[0], xy[:, 1] - centre[1]), trace[:, 0] * pol["dr"] + pol["r0"], atol=1e-9)


# ---- 5. the error path ----------------------------------------------------------------------------------------------------------------
def test_a_bad_spec_through_the_c_abi(amd, ctx):
    L = amd._lib
    frame = np.ascontiguousarray(R.frame_of(np.uint8, (9, 11), 1))
    cos_t, sin_t = R.tables(8)
    cx, cy = np.array([4.0]), np.array([5.0])
    dp = C.POINTER(C.c_double)

    def call(M=9, N=11, pix=0, n_img=1, tables=True, **change):
        f = dict(cx=cx.ctypes.data_as(dp), cy=cy.ctypes.data_as(dp), n_centres=1, n_r=5, n_theta=8, pad=1, r0=0.0, dr=1.0,
                 cos_t=cos_t.ctypes.data_as(dp) if tables else None, sin_t=sin_t.ctypes.data_as(dp))
        f.update(change)
        out = np.full((5, 11), -7.0)
        rp, op = (L._P * n_img)(*[frame.ctypes.data] * n_img), (L._P * n_img)(*[out.ctypes.data] * n_img)
        rc = ctx.lib.gpet_polar_images(ctx.h, rp, n_img, pix, M, N, C.byref(L.GpetPolar(**f)), 0, op)
        return rc, (ctx.lib.gpet_last_error(ctx.h) or b"").decode(), out

    rc, _, out = call()
    assert rc == L.OK and np.array_equal(out, R.unwrap([frame], (4.0, 5.0), 5, 8, pad=1)[0])
    bad = [(dict(n_r=0), L.polar_refusal(0, 8, 1, 0.0, 1.0)), (dict(n_theta=3), L.polar_refusal(5, 3, 1, 0.0, 1.0)),
           (dict(pad=9), L.polar_refusal(5, 8, 9, 0.0, 1.0)), (dict(r0=-1.0), L.polar_refusal(5, 8, 1, -1.0, 1.0)),
           (dict(dr=0.0), L.polar_refusal(5, 8, 1, 0.0, 0.0)), (dict(pix=7), "polar: unknown pixel type"),
           (dict(M=1), "polar: frames must be at least 2 x 2 pixels"), (dict(n_centres=2, n_img=3), "polar: one centre for all frames or one per frame"),
           (dict(cx=None), "polar: the centres are a null pointer"), (dict(tables=False), "polar: the trig tables are a null pointer"),
           (dict(n_r=1 << 20, n_theta=1 << 20), L.polar_refusal(1 << 20, 1 << 20, 1, 0.0, 1.0))]
    for change, words in bad:
        assert words is not None
        rc, msg, out = call(**change)
        assert rc == L.ERR_BAD_ARG and msg.startswith(words), (change, rc, msg)
        assert np.all(out == -7.0)  # nothing was launched, nothing copied
    cx[0] = np.inf
    rc, msg, _ = call()
    assert rc == L.ERR_BAD_ARG and msg.startswith("polar: a centre is not finite")
    cx[0] = 4.0
    assert call()[0] == L.OK  # the context is as good as before
