"""GPU tests of the multi-kernel raw-frame path (gpet_grad_images_multi, gpet_batch_create_raw_multi,
gpet_batch_set_raw_images_multi; comp_grad_imgs with a list of kernels, GP_Edge_Tracing_Batch / SequenceTracer with kernel_of):
image slot g is raw frame frame_of[g] convolved with kernel kernel_of[g], every frame uploaded, denoised and staged once.  The
oracle is inside the project: the single-kernel path, once per kernel.  Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 64
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
MATERN = dict(KW, kernel_options={'kernel': 'Matern', 'nu': 2.5, 'sigma_f': 10, 'length_scale': 8})
DTYPES = ["uint8", "uint16", "float32", "float64"]
SHAPES = [(16, 64), (17, 65), (33, 130), (5, 7)]  # exactly one tile; one more row and column; several tiles; smaller than the halo


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def kernel_sets(amd):
    k = amd.gpet_utils.kernel_builder((11, 5))
    rng = np.random.default_rng(7)

    def r(*s):  # small integers, some of them zero (the skipped taps), of a sum above 0: the clamp leaves a span to normalise by
        k = np.rint(rng.normal(size=s) * 4.0)
        return k if k.sum() > 0 else (-k if k.sum() < 0 else k + 1.0)
    return {"11x5 and its negation": [k, -k], "4x6, 11x5": [r(4, 6), k], "1x1, 3x7, 2x5": [np.array([[2.0]]), r(3, 7), r(2, 5)]}


def frames_of(dtype, shape, T=3, seed=0):
    rng = np.random.default_rng(seed + shape[0] * 131 + shape[1])
    a = rng.integers(0, 65536 if dtype == "uint16" else 256, size=(T,) + shape)
    if dtype in ("float32", "float64"):
        a = a / 255.0 + rng.normal(size=a.shape) * 0.01
    return np.ascontiguousarray(a.astype(dtype))


class DeviceFrames(object):
    """Frames in device memory of the library's own allocator (no second HIP runtime in the test process)."""

    def __init__(self, ctx, frames):
        self.ctx, self.ptrs = ctx, []
        for f in frames:
            a = np.ascontiguousarray(f)
            d = C.c_void_p()
            ctx.check(ctx.lib.gpet_dev_alloc(ctx.h, a.nbytes, C.byref(d)))
            ctx.check(ctx.lib.gpet_dev_copy(ctx.h, d, a.ctypes.data, a.nbytes, 0))
            self.ptrs.append(d.value)

    def close(self):
        for p in self.ptrs:
            self.ctx.lib.gpet_dev_free(self.ctx.h, C.c_void_p(p))
        self.ptrs = []


def per_kernel(amd, ctx, frames, kernels, denoise=None):
    """The oracle: the single-kernel path, once per kernel -> [k][t]."""
    return [amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx, denoise=denoise) for k in kernels]


def slot_images(amd, ctx, frames, kernels, frame_of, kernel_of, denoise=None, device=False):
    L = amd._lib
    if not device:
        return ctx.grad_images(L.RawFrames(kernels, frames=frames, denoise=denoise, slots=(frame_of, kernel_of)))
    dev = DeviceFrames(ctx, frames)
    try:
        raw = L.RawFrames(kernels, device_ptrs=dev.ptrs, dtype=frames[0].dtype, shape=frames[0].shape, denoise=denoise,
                          slots=(frame_of, kernel_of))
        return ctx.grad_images(raw)
    finally:
        dev.close()


# ---- 1. gradient images --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_kernel_of_a_list_equals_its_own_pass(amd, ctx, dtype):
    for name, kernels in kernel_sets(amd).items():
        for shape in SHAPES:
            frames = frames_of(dtype, shape)
            got = amd.gpet_utils.comp_grad_imgs(frames, kernels, ctx=ctx)
            assert got.shape == (3, len(kernels)) + shape and got.dtype == np.float32
            want = per_kernel(amd, ctx, frames, kernels)
            for k in range(len(kernels)):
                for t in range(3):
                    assert np.array_equal(got[t, k], want[k][t]), (dtype, name, shape, t, k)
            assert np.isfinite(got).all() and got.max() == 1.0 and got.min() == 0.0
    # a 3-D array of kernels is the list; a list of one kernel is one kernel with an axis for it
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames = frames_of(dtype, (17, 65))
    assert np.array_equal(amd.gpet_utils.comp_grad_imgs(frames, np.stack([k, -k]), ctx=ctx), amd.gpet_utils.comp_grad_imgs(frames, [k, -k], ctx=ctx))
    one = amd.gpet_utils.comp_grad_imgs(frames, [k], ctx=ctx)
    assert one.shape == (3, 1, 17, 65) and np.array_equal(one[:, 0], amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx))


TABLES = {"uneven": ([0, 0, 0, 1, 2, 2], [0, 1, 2, 1, 0, 2]),       # frame 0: kernels {0, 1, 2}, frame 1: {1}, frame 2: {0, 2}
          "interleaved": ([2, 0, 1, 0, 2, 1], [1, 0, 2, 2, 0, 0])}   # the slot order interleaves the frames


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_slot_tables(amd, ctx, table, device):
    kernels = kernel_sets(amd)["1x1, 3x7, 2x5"]
    frame_of, kernel_of = TABLES[table]
    for dtype in DTYPES:
        for shape in [(17, 65), (33, 130)]:
            frames = frames_of(dtype, shape)
            want = per_kernel(amd, ctx, frames, kernels)
            got = slot_images(amd, ctx, list(frames), kernels, frame_of, kernel_of, device=device)
            assert got.shape == (6,) + shape
            for g in range(6):
                assert np.array_equal(got[g], want[kernel_of[g]][frame_of[g]]), (table, dtype, shape, g)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("spec", [("median", dict(size=3)), ("tvc", dict(weight=0.1, n_iter_max=30))], ids=["median", "tvc"])
def test_denoised_frames(amd, ctx, spec, device):
    """'tvc' leaves float64 frames behind whatever went in: the convolution reads another pixel type than was uploaded."""
    kernels = kernel_sets(amd)["4x6, 11x5"]
    frame_of, kernel_of = [0, 1, 1, 2, 0], [0, 1, 0, 1, 1]
    for dtype in ("uint8", "float32"):
        frames = frames_of(dtype, (33, 130))
        want = per_kernel(amd, ctx, frames, kernels, denoise=spec)
        got = slot_images(amd, ctx, list(frames), kernels, frame_of, kernel_of, denoise=spec, device=device)
        for g in range(5):
            assert np.array_equal(got[g], want[kernel_of[g]][frame_of[g]]), (spec[0], dtype, g)
        if not device:
            full = amd.gpet_utils.comp_grad_imgs(frames, kernels, ctx=ctx, denoise=spec)
            assert all(np.array_equal(full[t, k], want[k][t]) for t in range(3) for k in range(2)), (spec[0], dtype)
        assert not np.array_equal(want[0], per_kernel(amd, ctx, frames, kernels[:1])[0])  # (the denoising does something)


def test_a_constant_frame_is_nan_in_both_paths(amd, ctx):
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames = frames_of("uint8", (17, 65))
    frames[1] = 9  # no gradient at all: span 0
    got = amd.gpet_utils.comp_grad_imgs(frames, [k, -k], ctx=ctx)
    want = per_kernel(amd, ctx, frames, [k, -k])
    assert np.isnan(got[1]).all() and np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    for kk in range(2):
        assert np.array_equal(got[:, kk], want[kk], equal_nan=True), kk


def test_more_than_one_staging_chunk(amd, ctx):
    """9 float64 frames of 1024 x 1024 are 72 MiB: chunks of 8 and 1 through the 64 MiB slot.  Frame 8, of the second chunk, has
    two slots; so has frame 0."""
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames = np.random.default_rng(3).random((9, 1024, 1024))
    frame_of, kernel_of = list(range(9)) + [8, 0], [0] * 9 + [1, 1]
    got = slot_images(amd, ctx, list(frames), [k, -k], frame_of, kernel_of)
    want0 = amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx)
    want1 = amd.gpet_utils.comp_grad_imgs(frames[[8, 0]], -k, ctx=ctx)
    assert np.array_equal(got[:9], want0)
    assert np.array_equal(got[9], want1[0]) and np.array_equal(got[10], want1[1])


# ---- 2. batches ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vessel(amd, ctx):
    """6 uint8 frames of 64 x 64 with a dark lumen between two drifting walls (two sets of 3: construction and set_frame): the
    upper wall is bright-to-dark, the lower one dark-to-bright.  ``K[0]`` is the kernel that answers to the upper wall, ``K[1]``
    to the lower one (told apart by their mean response along the walls); inits of the upper and the lower wall, full span and the
    inner half."""
    x = np.arange(N)
    rng = np.random.default_rng(11)
    raw, tops, bots = [], [], []
    for t in range(6):
        top = np.rint(18 + 4 * np.sin(2 * np.pi * x / N + 0.2 * t)).astype(int)
        bot = np.rint(45 + 4 * np.cos(2 * np.pi * x / N + 0.2 * t)).astype(int)
        rows = np.arange(N)[:, None]
        img = np.where((rows >= top[None, :]) & (rows < bot[None, :]), 0.1, 0.7) + rng.normal(0.0, 0.03, (N, N))
        raw.append(np.rint(np.clip(img, 0, 1) * 255).astype(np.uint8))
        tops.append(top)
        bots.append(bot)
    ka, kb = amd.gpet_utils.kernel_builder((11, 5)), amd.gpet_utils.kernel_builder((11, 5), b2d=True)
    ga = amd.gpet_utils.comp_grad_img(raw[0], ka, ctx=ctx)
    K = [ka, kb] if ga[tops[0], x].mean() > ga[bots[0], x].mean() else [kb, ka]
    ends = lambda wall, lo, hi: np.array([[lo, wall[lo]], [hi, wall[hi]]])
    return dict(raw=raw, K=K, top=ends(tops[0], 0, N - 1), bot=ends(bots[0], 0, N - 1), top_half=ends(tops[0], N // 4, 3 * N // 4),
                bot_half=ends(bots[0], N // 4, 3 * N // 4))


def images(amd, b):
    L = amd._lib
    return [(b._batch.read(L.BUF_GRAD, e), b._batch.read(L.BUF_GRAD_KDE, e)) for e in range(b.B)]


def run(b):
    out = b()
    return out, list(b.timings["iters"])


def assert_same_batch(amd, got, want, what):
    for e, ((ga, ka), (gb, kb)) in enumerate(zip(images(amd, got), images(amd, want))):
        assert np.array_equal(ga, gb), (what, "grad", e)
        assert np.array_equal(ka, kb), (what, "grad kde", e)
    (ra, ia), (rb, ib) = run(got), run(want)
    assert ia == ib and min(ia) >= 1, (what, ia, ib)
    for e, ((ta, (la, ua)), (tb, (lb, ub))) in enumerate(zip(ra, rb)):
        assert np.array_equal(ta, tb), (what, "trace", e)
        assert np.array_equal(la, lb) and np.array_equal(ua, ub), (what, "interval", e)


def check_batch_against_slot_images(amd, ctx, vessel, inits, kernel_of, edge_frames, frames, nxt, image_of=None, denoise=None):
    """The multi-kernel raw batch against the batch of the slot images computed per kernel, with the edge-to-slot map; then the
    next frames through set_frame(warm_every=) on both."""
    K, seeds = vessel["K"], list(range(3, 3 + len(inits)))
    frame_of, kernel_of_slot, edge_slot = amd._lib.derive_slots(edge_frames, kernel_of)
    stack = lambda fr: [fr] if np.ndim(fr) == 2 else list(fr)
    per_k = lambda fr: [amd.gpet_utils.comp_grad_imgs(stack(fr), k, ctx=ctx, denoise=denoise) for k in K]
    slot_imgs = lambda fr: [per_k(fr)[kernel_of_slot[g]][frame_of[g]] for g in range(len(frame_of))]
    m = amd.GP_Edge_Tracing_Batch(inits, None, seeds, return_std=True, _ctx=ctx, raw_imgs=frames, grad_kernel=K, kernel_of=kernel_of,
                                  image_of=image_of, denoise=denoise, **KW)
    d = amd.GP_Edge_Tracing_Batch(inits, slot_imgs(frames), seeds, return_std=True, _ctx=ctx, image_of=edge_slot, **KW)
    assert m._batch.n_img == len(frame_of) == d._batch.n_img and m._batch.image_of == edge_slot
    assert_same_batch(amd, m, d, "construction")
    m.set_frame(None, None, seeds, raw_imgs=nxt, warm_every=10)
    d.set_frame(slot_imgs(nxt), None, seeds, warm_every=10)
    assert_same_batch(amd, m, d, "set_frame")
    m._batch.close()
    d._batch.close()


def test_six_edges_on_three_frames_with_two_kernels(amd, ctx, vessel):
    v = vessel
    check_batch_against_slot_images(amd, ctx, v, [v["top"], v["bot"]] * 3, [0, 1] * 3, [0, 0, 1, 1, 2, 2], v["raw"][:3], v["raw"][3:],
                                    image_of=[0, 0, 1, 1, 2, 2])


def test_shared_frame_with_two_kernels(amd, ctx, vessel):
    v = vessel
    check_batch_against_slot_images(amd, ctx, v, [v["top"], v["bot"], v["top"]], [0, 1, 0], [0, 0, 0], v["raw"][0], v["raw"][3])


def test_one_frame_per_edge_with_per_edge_kernels_and_mixed_widths(amd, ctx, vessel):
    v = vessel
    check_batch_against_slot_images(amd, ctx, v, [v["bot"], v["top_half"], v["bot_half"]], [1, 0, 1], [0, 1, 2], v["raw"][:3], v["raw"][3:])


def test_interleaved_edges_with_median_denoising(amd, ctx, vessel):
    """The edge order interleaves (frame, kernel) pairs, two edges share a slot, and the slots' representatives are not the first
    edges; the frames are denoised first."""
    v = vessel
    check_batch_against_slot_images(amd, ctx, v, [v["bot"], v["top"], v["bot_half"], v["top_half"], v["top"]], [1, 0, 1, 0, 0],
                                    [1, 0, 1, 1, 1], v["raw"][:2], v["raw"][3:5], image_of=[1, 0, 1, 1, 1], denoise=("median", dict(size=3)))


def test_set_frame_refuses_another_count_of_frames(amd, ctx, vessel):
    v = vessel
    m = amd.GP_Edge_Tracing_Batch([v["top"], v["bot"]] * 2, None, [3, 4, 5, 6], return_std=True, _ctx=ctx, raw_imgs=v["raw"][:2],
                                  grad_kernel=v["K"], kernel_of=[0, 1, 0, 1], image_of=[0, 0, 1, 1], **KW)
    first = run(m)
    with pytest.raises(ValueError, match="2 raw frames"):
        m.set_frame(None, None, [3, 4, 5, 6], raw_imgs=v["raw"][:3])
    m.reset()
    again = run(m)
    assert first[1] == again[1] and all(np.array_equal(a[0], b[0]) for a, b in zip(first[0], again[0]))
    m._batch.close()


# ---- 3. sequences --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [KW, MATERN], ids=["rbf", "matern"])
def test_sequence_of_two_walls_equals_the_single_edge_runs(amd, ctx, vessel, kw):
    v = vessel
    frames, seeds = v["raw"][:4], [5, 6, 7, 8]
    multi = amd.SequenceTracer(frames, [v["top"], v["bot"]], n_chains=2, warm_every=10, seeds=seeds, _ctx=ctx, grad_kernel=v["K"], **kw)
    got = multi()
    assert multi._tracer.B == 4 and multi._tracer._batch.n_img == 4 and multi._tracer._batch.image_of == [0, 1, 2, 3]
    for k, init in enumerate([v["top"], v["bot"]]):
        single = amd.SequenceTracer(frames, init, n_chains=2, warm_every=10, seeds=seeds, _ctx=ctx, grad_kernel=v["K"][k], **kw)
        want = single()
        for t in range(4):
            assert multi.iterations[t][k] == single.iterations[t] >= 1, (k, t)
            assert np.array_equal(got[t][k], want[t]), (k, t)
    if kw is KW:  # fewer kernels than inits with kernel_of; trace_sequence is the same call
        three = amd.trace_sequence(frames, [v["top"], v["bot"], v["top_half"]], n_chains=2, warm_every=10, seeds=seeds, _ctx=ctx,
                                   grad_kernel=v["K"], kernel_of=[0, 1, 0], **kw)
        assert all(np.array_equal(three[t][0], got[t][0]) and np.array_equal(three[t][1], got[t][1]) for t in range(4))


# ---- 4. the degenerate table ---------------------------------------------------------------------------------------------------
def test_one_kernel_with_the_identity_table_is_the_mapped_raw_batch(amd, ctx, vessel):
    v = vessel
    inits, seeds, io = [v["top"], v["top_half"], v["top"], v["top_half"]], [3, 4, 5, 6], [0, 0, 1, 1]
    m = amd.GP_Edge_Tracing_Batch(inits, None, seeds, return_std=True, _ctx=ctx, raw_imgs=v["raw"][:2], grad_kernel=[v["K"][0]],
                                  kernel_of=[0, 0, 0, 0], image_of=io, **KW)
    d = amd.GP_Edge_Tracing_Batch(inits, None, seeds, return_std=True, _ctx=ctx, raw_imgs=v["raw"][:2], grad_kernel=v["K"][0], image_of=io, **KW)
    assert m._batch.n_img == 2 and m._batch.image_of == io and m._batch.info(0)["arena_mib"] == d._batch.info(0)["arena_mib"]
    assert_same_batch(amd, m, d, "construction")
    m.set_frame(None, None, seeds, raw_imgs=v["raw"][3:5], warm_every=10)
    d.set_frame(None, None, seeds, raw_imgs=v["raw"][3:5], warm_every=10)
    assert_same_batch(amd, m, d, "set_frame")
    m._batch.close()
    d._batch.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def i32(v):
    return (C.c_int32 * max(1, len(v)))(*v)


BAD_TABLES = [  # (n_frames, kernels used, frame_of, kernel_of, part of the message) for 4 slots
    (2, 2, [0, 0, 1, 2], [0, 1, 0, 1], "frame index out of range"),
    (2, 2, [0, 0, 1, 1], [0, 1, 0, 2], "kernel index out of range"),
    (3, 2, [0, 0, 1, 1], [0, 1, 0, 1], "a frame no slot reads"),
    (2, 3, [0, 0, 1, 1], [0, 1, 0, 1], "a kernel no slot reads"),
    (2, 2, [0, 0, 1, 0], [0, 1, 0, 1], "pair twice"),
    (2, 9, [0, 0, 1, 1], [0, 1, 0, 1], "more than 8 kernels"),
]


def test_c_abi_refuses_bad_tables_and_leaves_the_batch_alone(amd, ctx, vessel):
    v, L, lib = vessel, amd._lib, ctx.lib
    inits, seeds = [v["top"], v["bot"]] * 2, [3, 4, 5, 6]
    mk = lambda: amd.GP_Edge_Tracing_Batch(inits, None, seeds, return_std=True, _ctx=ctx, raw_imgs=v["raw"][:2], grad_kernel=v["K"],
                                           kernel_of=[0, 1, 0, 1], image_of=[0, 0, 1, 1], **KW)
    m, twin = mk(), mk()
    kern = [np.ascontiguousarray(k, dtype=np.float64) for k in v["K"]] + [np.ones((3, 3))] * 7
    big = [np.ones((60, 1)), np.ones((1, 300))]  # each fits the LDS alone, the union does not
    raw = [np.ascontiguousarray(f) for f in v["raw"][3:6]]
    out = np.empty((4, N, N), np.float32)
    op = (C.c_void_p * 4)(*[out[g].ctypes.data for g in range(4)])
    pa = (L.GpetParams * 4)(*[amd.gpet.to_abi_params(p) for p in m._ps])
    ini = [np.ascontiguousarray(p["init"], dtype=np.int64) for p in m._ps]
    ip = (C.c_void_p * 4)(*[i.ctypes.data for i in ini])

    def calls(n_frames, ks, frame_of, kernel_of, frames=raw, dn=None):
        rp = (C.c_void_p * 3)(*[None if f is None else f.ctypes.data for f in frames])
        kp = (C.c_void_p * len(ks))(*[k.ctypes.data for k in ks])
        kh, kw = i32([k.shape[0] for k in ks]), i32([k.shape[1] for k in ks])
        fo, ko = i32(frame_of), i32(kernel_of)
        res = []
        rc = lib.gpet_grad_images_multi(ctx.h, rp, n_frames, L.PIX_U8, N, N, len(ks), kp, kh, kw, dn, 4, fo, ko, 0, op)
        res.append((rc, lib.gpet_last_error(ctx.h).decode()))
        h = C.c_void_p()
        rc = lib.gpet_batch_create_raw_multi(ctx.h, 4, N, N, 4, i32([0, 1, 2, 3]), n_frames, rp, L.PIX_U8, len(ks), kp, kh, kw, fo, ko, dn,
                                             pa, ip, 0, C.byref(h))
        res.append((rc, lib.gpet_last_error(ctx.h).decode()))
        assert bool(h.value) == (rc == L.OK)
        if h.value:
            lib.gpet_batch_destroy(h)
        rc = lib.gpet_batch_set_raw_images_multi(m._batch.h, n_frames, rp, L.PIX_U8, len(ks), kp, kh, kw, fo, ko, dn, 0)
        res.append((rc, lib.gpet_last_error(ctx.h).decode()))
        return res

    for n_frames, n_kern, frame_of, kernel_of, part in BAD_TABLES:
        for rc, msg in calls(n_frames, kern[:n_kern], frame_of, kernel_of):
            assert rc == L.ERR_BAD_ARG and part in msg, (part, rc, msg)
    good = (2, [0, 0, 1, 1], [0, 1, 0, 1])
    for rc, msg in calls(good[0], big, *good[1:]):
        assert rc == L.ERR_BAD_ARG and "220680" in msg and "65536" in msg, msg  # (the byte counts: tests/test_multi_kernel_host.py)
    for rc, msg in calls(good[0], kern[:2], *good[1:], frames=[raw[0], None, raw[2]]):
        assert rc == L.ERR_BAD_ARG and "frame 1" in msg and "null" in msg, msg
    bad_dn = L.GpetDenoise(technique=L.DN_MEDIAN, size_y=11, size_x=11)  # a window above 81 pixels
    for rc, msg in calls(good[0], kern[:2], *good[1:], dn=C.byref(bad_dn)):
        assert rc == L.ERR_BAD_ARG and "denoise" in msg, msg
    # after all the refused calls the batch is what its untouched twin is: images, gradient KDE, and the trace that follows
    assert_same_batch(amd, m, twin, "after refused calls")
    # and the same calls with a good table do go through
    assert [rc for rc, _ in calls(good[0], kern[:2], *good[1:])] == [L.OK, L.OK, L.OK]
    m._batch.close()
    twin._batch.close()
