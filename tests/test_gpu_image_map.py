"""GPU tests of batches with an image map (gpet_batch_create_mapped, gpet_batch_create_raw_mapped, gpet_batch_image_count;
GP_Edge_Tracing_Batch(image_of=...)): several edges read one image, which is uploaded, turned into a gradient image, denoised and
run through the gradient KDE once.  The oracle is inside the project: a mapped batch equals, bit for bit, the batch built from the
duplicated images."""
import ctypes as C

import numpy as np
import pytest

from oracle import gpet_oracle as orc

pytestmark = pytest.mark.gpu

N = 256
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 40, 'length_scale': 12}, noise_y=1, N_samples=300, score_thresh=1, delta_x=6,
          keep_ratio=0.1, pixel_thresh=4, fix_endpoints=True)
MAP = [0, 1, 2, 0, 1, 2]
SEEDS = [3, 4, 5, 6, 7, 8]


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def scene(amd, ctx):
    """6 raw uint8 frames of one drifting sinusoidal edge (two sets of 3: construction and set_frame), their gradient images, and
    per image a full-span init and an init on the inner half [N/4, 3N/4]: a batch of 6 edges with mixed widths."""
    k = amd.gpet_utils.kernel_builder((11, 5))
    raw, truths = [], []
    for t in range(6):
        img, truth = orc.synth_sinusoid_image(N, 31 + t, amplitude=int(0.4 * N * (1.0 + 0.02 * t)))
        raw.append(np.rint(img * 255.0).astype(np.uint8))
        truths.append(truth)
    grads = [amd.gpet_utils.comp_grad_img(f, k, ctx=ctx) for f in raw]
    full = lambda g: truths[g][[0, -1], :][:, [1, 0]]
    half = lambda g: truths[g][[N // 4, 3 * N // 4], :][:, [1, 0]]
    inits = [full(0), full(1), full(2), half(0), half(1), half(2)]  # edge e reads image MAP[e]
    return dict(kernel=k, raw=raw, grads=grads, inits=inits)


def batch(amd, ctx, scene, **kw):
    return amd.GP_Edge_Tracing_Batch(scene["inits"], kw.pop("grad_imgs", None), SEEDS, return_std=True, _ctx=ctx, **kw, **KW)


def dup(imgs):
    return [imgs[g] for g in MAP]


def run(b):
    out = b()
    return out, list(b.timings["iters"])


def assert_same_results(got, want, what):
    (ra, ia), (rb, ib) = got, want
    assert ia == ib and min(ia) >= 1, (what, ia, ib)
    for e, ((ta, (la, ua)), (tb, (lb, ub))) in enumerate(zip(ra, rb)):
        assert np.array_equal(ta, tb), (what, "trace", e)
        assert np.array_equal(la, lb) and np.array_equal(ua, ub), (what, "interval", e)


@pytest.fixture(scope="module")
def duplicated(amd, ctx, scene):
    """The oracle, computed once: the batch of the 6 duplicated gradient images -- its images, traces, intervals, iterations."""
    b = batch(amd, ctx, scene, grad_imgs=dup(scene["grads"][:3]))
    L = amd._lib
    assert b._batch.n_img == 6 and not b._batch.share_image
    images = [(b._batch.read(L.BUF_GRAD, e), b._batch.read(L.BUF_GRAD_KDE, e)) for e in range(6)]
    res = run(b)
    widths = [b._batch.info(e)["Lg"] for e in range(6)]
    assert widths == [N] * 3 + [N // 2 + 1] * 3  # mixed widths
    b._batch.close()
    return dict(images=images, results=res)


class DeviceImages(object):
    """f32 images in device memory of the library's own allocator (no second HIP runtime in the test process)."""

    def __init__(self, ctx, imgs):
        self.ctx, self.ptrs = ctx, []
        for g in imgs:
            a = np.ascontiguousarray(g, dtype=np.float32)
            d = C.c_void_p()
            ctx.check(ctx.lib.gpet_dev_alloc(ctx.h, a.nbytes, C.byref(d)))
            ctx.check(ctx.lib.gpet_dev_copy(ctx.h, d, a.ctypes.data, a.nbytes, 0))
            self.ptrs.append(d.value)

    def close(self):
        for p in self.ptrs:
            self.ctx.lib.gpet_dev_free(self.ctx.h, C.c_void_p(p))
        self.ptrs = []


@pytest.mark.parametrize("source", ["host_grad", "device_grad", "raw_u8", "raw_u8_median"])
def test_mapped_batch_equals_duplicated_batch(amd, ctx, scene, duplicated, source):
    L = amd._lib
    dev = None
    if source == "host_grad":
        b = batch(amd, ctx, scene, grad_imgs=scene["grads"][:3], image_of=MAP)
        want = duplicated
    elif source == "device_grad":
        dev = DeviceImages(ctx, scene["grads"][:3])
        b = batch(amd, ctx, scene, grad_device_ptrs=dev.ptrs, grad_shape=(N, N), image_of=MAP)
        want = duplicated
    elif source == "raw_u8":
        b = batch(amd, ctx, scene, raw_imgs=scene["raw"][:3], grad_kernel=scene["kernel"], image_of=MAP)
        want = duplicated  # (a batch from raw frames equals the one from comp_grad_img's outputs: tests/test_gpu_raw_frames.py)
    else:
        spec = ("median", dict(size=3))
        b = batch(amd, ctx, scene, raw_imgs=scene["raw"][:3], grad_kernel=scene["kernel"], denoise=spec, image_of=MAP)
        d = batch(amd, ctx, scene, raw_imgs=dup(scene["raw"][:3]), grad_kernel=scene["kernel"], denoise=spec)
        want = dict(images=[(d._batch.read(L.BUF_GRAD, e), d._batch.read(L.BUF_GRAD_KDE, e)) for e in range(6)], results=run(d))
        d._batch.close()
    assert b._batch.n_img == 3 and not b._batch.share_image and b._batch.image_of == MAP
    for e in range(6):  # every edge sees the image of its slot, and that slot's gradient KDE
        assert np.array_equal(b._batch.read(L.BUF_GRAD, e), want["images"][e][0]), (source, "grad", e)
        assert np.array_equal(b._batch.read(L.BUF_GRAD_KDE, e), want["images"][e][1]), (source, "grad kde", e)
    assert_same_results(run(b), want["results"], source)
    b._batch.close()
    if dev is not None:
        dev.close()


def test_map_whose_first_edges_are_not_its_slots_representatives(amd, ctx, scene):
    """[1, 1, 0, 2, 0, 2]: the slots' representatives are edges 2, 0, 3 -- not the first n_img edges, so the images are written and
    the gradient KDE runs through the device copy of the representatives' EdgeDev (image_kde), at construction and in set_frame.
    Every edge must see the gradient image and the gradient KDE the duplicated batch gives it, and trace the same."""
    L = amd._lib
    map2 = [1, 1, 0, 2, 0, 2]
    I = scene["inits"]  # I[g] spans image g, I[3 + g] its inner half
    inits = [I[1], I[4], I[0], I[2], I[3], I[5]]
    mk = lambda imgs, **kw: amd.GP_Edge_Tracing_Batch(inits, imgs, SEEDS, return_std=True, _ctx=ctx, **kw, **KW)
    images = lambda b: [(b._batch.read(L.BUF_GRAD, e), b._batch.read(L.BUF_GRAD_KDE, e)) for e in range(6)]

    def assert_same_images(m, d, what):
        for e, ((ga, ka), (gb, kb)) in enumerate(zip(images(m), images(d))):
            assert np.array_equal(ga, gb), (what, "grad", e)
            assert np.array_equal(ka, kb), (what, "grad kde", e)
    m = mk(scene["grads"][:3], image_of=map2)
    d = mk([scene["grads"][g] for g in map2])
    assert m._batch.n_img == 3 and m._batch.image_of == map2 and d._batch.n_img == 6
    g0 = images(d)
    assert not np.array_equal(g0[0][1], g0[2][1]) and not np.array_equal(g0[2][1], g0[3][1])  # (the slots' KDEs do differ)
    assert_same_images(m, d, "construction")
    assert_same_results(run(m), run(d), "construction")
    m.set_frame(scene["grads"][3:], None, SEEDS)
    d.set_frame([scene["grads"][3 + g] for g in map2], None, SEEDS)
    assert_same_images(m, d, "set_frame")
    assert_same_results(run(m), run(d), "set_frame")
    m.set_frame(None, None, SEEDS, raw_imgs=scene["raw"][:3], grad_kernel=scene["kernel"])  # (convolve_images' slots)
    d.set_frame([scene["grads"][g] for g in map2], None, SEEDS)
    assert_same_images(m, d, "set_frame(raw_imgs=)")
    m._batch.close()
    d._batch.close()


def test_single_slot_map_equals_shared_batch(amd, ctx, scene):
    L = amd._lib
    inits = [scene["inits"][0], scene["inits"][3], scene["inits"][0]]
    mk = lambda g, **kw: amd.GP_Edge_Tracing_Batch(inits, g, [3, 4, 5], return_std=True, _ctx=ctx, **kw, **KW)
    shared = mk(scene["grads"][0])
    mapped = mk([scene["grads"][0]], image_of=[0, 0, 0])
    assert shared._batch.share_image and shared._batch.n_img == 1 and mapped._batch.n_img == 1
    assert shared._batch.info(0)["arena_mib"] == mapped._batch.info(0)["arena_mib"]
    for e in range(3):
        assert np.array_equal(shared._batch.read(L.BUF_GRAD_KDE, e), mapped._batch.read(L.BUF_GRAD_KDE, e))
    assert_same_results(run(mapped), run(shared), "n_img = 1")
    shared._batch.close()
    mapped._batch.close()


def test_set_frame_of_a_mapped_batch(amd, ctx, scene, duplicated):
    k = scene["kernel"]
    new_seeds = [11, 12, 13, 14, 15, 16]
    m = batch(amd, ctx, scene, grad_imgs=scene["grads"][:3], image_of=MAP)
    d = batch(amd, ctx, scene, grad_imgs=dup(scene["grads"][:3]))
    first = run(m)
    assert_same_results(first, duplicated["results"], "construction")
    run(d)
    # a wrong count raises before anything is touched: the batch still traces its old frames to the old result
    for bad in (dict(grad_imgs=dup(scene["grads"][3:])), dict(grad_imgs=scene["grads"][3:5]), dict(raw_imgs=scene["raw"][:2], grad_kernel=k)):
        with pytest.raises(ValueError, match="n_img = 3"):
            m.set_frame(seeds=new_seeds, **bad)
    # the C entry points refuse a null image and an unknown pixel type the same way
    lib, L = ctx.lib, amd._lib
    g32 = [np.ascontiguousarray(g, dtype=np.float32) for g in scene["grads"][3:]]
    assert lib.gpet_batch_set_images(m._batch.h, (C.c_void_p * 3)(g32[0].ctypes.data, None, g32[2].ctypes.data), 0) == L.ERR_BAD_ARG
    assert "image 1" in lib.gpet_last_error(ctx.h).decode()
    raw8 = [np.ascontiguousarray(f) for f in scene["raw"][3:]]
    kern = np.ascontiguousarray(k, dtype=np.float64)
    rp = (C.c_void_p * 3)(*[f.ctypes.data for f in raw8])
    assert lib.gpet_batch_set_raw_images(m._batch.h, rp, 9, kern.ctypes.data, kern.shape[0], kern.shape[1], 0) == L.ERR_BAD_ARG
    assert "pixel type" in lib.gpet_last_error(ctx.h).decode()
    m.reset()
    assert_same_results(run(m), first, "after refused set_frame calls")
    # 3 new images for the mapped batch, the same 6 for the duplicated one
    m.set_frame(scene["grads"][3:], None, new_seeds)
    d.set_frame(dup(scene["grads"][3:]), None, new_seeds)
    for e in range(6):
        assert np.array_equal(m._batch.read(L.BUF_GRAD_KDE, e), d._batch.read(L.BUF_GRAD_KDE, e)), e
    second = run(m)
    assert_same_results(second, run(d), "set_frame")
    assert not all(np.array_equal(a[0], b[0]) for a, b in zip(first[0], second[0]))  # (another frame: another trace)
    # and raw frames through set_frame, for a batch built from gradient images
    m.set_frame(None, None, SEEDS, raw_imgs=scene["raw"][:3], grad_kernel=k)
    assert_same_results(run(m), first, "set_frame(raw_imgs=)")
    m._batch.close()
    d._batch.close()


def test_c_abi_refuses_bad_maps_and_counts_images(amd, ctx, scene):
    L = amd._lib
    lib = ctx.lib
    ps = batch(amd, ctx, scene, grad_imgs=scene["grads"][:3], image_of=MAP)
    abi = [amd.gpet.to_abi_params(p) for p in ps._ps]
    assert lib.gpet_batch_image_count(ps._batch.h) == 3
    ps._batch.close()
    own = batch(amd, ctx, scene, grad_imgs=dup(scene["grads"][:3]))
    assert lib.gpet_batch_image_count(own._batch.h) == 6
    own._batch.close()
    sh = amd.GP_Edge_Tracing_Batch(scene["inits"], scene["grads"][0], SEEDS, _ctx=ctx, **KW)
    assert lib.gpet_batch_image_count(sh._batch.h) == 1
    sh._batch.close()
    assert lib.gpet_batch_image_count(None) == 0

    inits = [np.ascontiguousarray(p["init"], dtype=np.int64) for p in ps._ps]
    ip = (C.c_void_p * 6)(*[i.ctypes.data for i in inits])
    pa = (L.GpetParams * 6)(*abi)
    g32 = [np.ascontiguousarray(g, dtype=np.float32) for g in scene["grads"][:3]]

    def create(n_img, image_of, imgs=g32, raw_pix=None):
        gp = (C.c_void_p * max(1, len(imgs)))(*[None if g is None else g.ctypes.data for g in imgs])
        io = (C.c_int32 * 6)(*image_of) if image_of is not None else None
        h = C.c_void_p()
        if raw_pix is not None:
            kern = np.ascontiguousarray(scene["kernel"], dtype=np.float64)
            rc = lib.gpet_batch_create_raw_mapped(ctx.h, 6, N, N, n_img, io, gp, raw_pix, kern.ctypes.data, kern.shape[0], kern.shape[1], None,
                                                  pa, ip, 0, C.byref(h))
        else:
            rc = lib.gpet_batch_create_mapped(ctx.h, 6, N, N, n_img, io, gp, pa, ip, 0, C.byref(h))
        msg = (lib.gpet_last_error(ctx.h) or b"").decode()
        if h.value:
            lib.gpet_batch_destroy(h)
        return rc, msg, bool(h.value)

    msgs = []
    for n_img, image_of, part in [(0, MAP, "at least 1"), (7, MAP, "more image slots than edges"), (3, [0, 1, 3, 0, 1, 2], "outside"),
                                  (3, [0, 1, -1, 0, 1, 2], "outside"), (3, [0, 1, 0, 0, 1, 1], "no edge"), (3, None, "null")]:
        rc, msg, made = create(n_img, image_of)
        assert rc == L.ERR_BAD_ARG and not made and part in msg, (n_img, image_of, rc, msg)
        msgs.append(msg)
    assert len(set(msgs)) == 5  # (the two out-of-range cases share a message)
    rc, msg, made = create(3, MAP, imgs=[g32[0], None, g32[2]])
    assert rc == L.ERR_BAD_ARG and not made and "image 1" in msg and "null" in msg, msg
    raw8 = [np.ascontiguousarray(f) for f in scene["raw"][:3]]
    rc, msg, made = create(3, MAP, imgs=raw8, raw_pix=9)  # (no such pixel type)
    assert rc == L.ERR_BAD_ARG and not made and "pixel type" in msg, msg
    rc, msg, made = create(3, MAP, imgs=raw8, raw_pix=L.PIX_U8)
    assert rc == L.OK and made, msg
    rc, msg, made = create(3, MAP, imgs=[raw8[0], raw8[1], None], raw_pix=L.PIX_U8)
    assert rc == L.ERR_BAD_ARG and not made and "frame 2" in msg, msg
    rc, msg, made = create(0, MAP, imgs=raw8, raw_pix=L.PIX_U8)
    assert rc == L.ERR_BAD_ARG and not made and "at least 1" in msg, msg
    rc, msg, made = create(3, MAP)
    assert rc == L.OK and made, msg
