"""What every raw-frame entry point of the C ABI refuses, and in which order: the return code and the FULL text of gpet_last_error,
for single defects and for pairs of them (which of two defects is named).  Everything here is refused before anything is enqueued:
no invalid non-null pointer, nothing a kernel would have to find.  The context calls see two uint8 frames of 32 x 48, the batch
calls two edges on 128 x 128 frames; after all refused set calls the live batch traces as its untouched twin does, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from oracle import gpet_oracle as orc

pytestmark = pytest.mark.gpu

_P = C.c_void_p
M, N = 32, 48  # frames of the context calls
NB = 128       # frames of the batch calls
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 20, 'length_scale': 8}, noise_y=1, N_samples=300, score_thresh=1,
          delta_x=8, keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)

# ---- the messages, from the library's format strings --------------------------------------------------------------------------
PIX7 = "unknown pixel type 7 (GPET_PIX_U8 = 0 .. GPET_PIX_F64 = 3)"
NULL1 = "raw frame 1 is a null pointer"
RAW_BAD = "raw frames: bad argument"
GRAD_BAD = "gpet_grad_images: bad argument"
# a 45 x 45 kernel: 2025 taps + a patch of (16 + 44) x (64 + 44) doubles; transposed store: (16 + 44) columns of pitch (64 + 44) | 1
K45 = "a 45 x 45 kernel needs 68040 bytes of LDS for its patch, more than 65536"
K45_T = "a 45 x 45 kernel needs 68520 bytes of LDS for its patch, more than 65536"
T45 = "the 1 kernels need 68040 bytes of LDS for their taps and their union patch of 60 x 108, more than 65536"
T45_T = "the 1 kernels need 68520 bytes of LDS for their taps and their union patch of 108 x 60, more than 65536"
DN_BAD = "denoise: windows of more than 81 pixels (9 x 9) are not built"
T_EMPTY = "slot table: kernel 0 is empty or a null pointer"
T_RANGE = "slot table: frame index out of range (n_frames = 2, n_kern = 1, n_img = 2)"
ORIENT = ("GPET_FRAMES_TRANSPOSED on a batch that was created without it: the orientation of a batch is decided at its "
          "creation")

# defects: pix (pixel type 7), null (frame 1 a null pointer), k45 (a 45 x 45 kernel), tr (GPET_FRAMES_TRANSPOSED), kh0 (kh = 0),
# dn (a median window of 11 x 11), frame_of (slot 1 reads frame 2 of 2)
# the entry points with one kernel; `bad`: what the entry point itself says to kh = 0
SINGLE = [(("pix",), PIX7), (("null",), NULL1), (("k45",), K45), (("k45", "tr"), K45_T), (("kh0",), "bad"),
          (("pix", "null"), PIX7), (("pix", "k45"), PIX7), (("kh0", "pix"), "bad")]
SINGLE_DN = SINGLE + [(("dn",), DN_BAD), (("k45", "dn"), K45), (("dn", "null"), DN_BAD)]
# the entry points with a slot table (here: one kernel, slot g = frame g).  The batch calls name the pixel type before the table,
# gpet_grad_images_multi checks the table before it sizes its scratch and so names it first: `pix_first`
TABLE = [(("pix",), PIX7), (("null",), NULL1), (("k45",), T45), (("k45", "tr"), T45_T), (("kh0",), T_EMPTY), (("dn",), DN_BAD),
         (("frame_of",), T_RANGE), (("pix", "null"), PIX7), (("k45", "dn"), T45), (("frame_of", "null"), T_RANGE),
         (("kh0", "null"), T_EMPTY)]
TABLE_PAIRS = [(("pix", "k45"), PIX7, T45), (("kh0", "pix"), PIX7, T_EMPTY), (("pix", "frame_of"), PIX7, T_RANGE)]  # (batch, context)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


class Source(object):
    """Raw uint8 frames and one kernel as the C entry points take them, in both forms (one kernel; a table of one kernel with
    slot g = frame g), with the given defects."""

    def __init__(self, L, frames, kernel, defects=()):
        d, n = set(defects), len(frames)
        assert d <= {"pix", "null", "k45", "tr", "kh0", "dn", "frame_of"}
        self.n, self.frames = n, frames
        self.rp = (_P * n)(*[None if ("null" in d and i == 1) else f.ctypes.data for i, f in enumerate(frames)])
        self.pix = 7 if "pix" in d else L.PIX_U8
        self.k = np.ones((45, 45)) if "k45" in d else kernel
        self.kp, self.kh, self.kw = self.k.ctypes.data, (0 if "kh0" in d else self.k.shape[0]), self.k.shape[1]
        self.spec = L.GpetDenoise(technique=L.DN_MEDIAN, size_y=11, size_x=11) if "dn" in d else None
        self.dn = C.byref(self.spec) if "dn" in d else None
        self.flags = L.FRAMES_TRANSPOSED if "tr" in d else 0
        self.kps, self.khs, self.kws = (_P * 1)(self.kp), (C.c_int32 * 1)(self.kh), (C.c_int32 * 1)(self.kw)
        self.fo, self.ko = (C.c_int32 * n)(*range(n)), (C.c_int32 * n)()
        if "frame_of" in d:
            self.fo[1] = n


def refused(L, lib, ctx, rc, want, what):
    msg = lib.gpet_last_error(ctx.h).decode()
    assert rc == L.ERR_BAD_ARG and msg == want, (what, rc, msg, want)


# ---- the context calls -----------------------------------------------------------------------------------------------------------
def test_context_calls(amd, ctx):
    L, lib = amd._lib, ctx.lib
    rng = np.random.default_rng(5)
    frames = [np.ascontiguousarray(rng.integers(0, 256, size=(M, N), dtype=np.uint8)) for _ in range(2)]
    k = np.ascontiguousarray(amd.gpet_utils.kernel_builder((11, 5)), dtype=np.float64)
    out = np.empty((2, M * N), np.float64)  # (wide enough for every entry point's output type)
    op = (_P * 2)(*[out[g].ctypes.data for g in range(2)])
    src = lambda d: Source(L, frames, k, d)

    for d, want in SINGLE_DN:
        s = src(d)
        want = GRAD_BAD if want == "bad" else want
        if "dn" not in d:
            refused(L, lib, ctx, lib.gpet_grad_images(ctx.h, s.rp, 2, s.pix, M, N, s.kp, s.kh, s.kw, s.flags, op), want, ("grad_images", d))
        refused(L, lib, ctx, lib.gpet_grad_images_dn(ctx.h, s.rp, 2, s.pix, M, N, s.kp, s.kh, s.kw, s.dn, s.flags, op), want,
                ("grad_images_dn", d))
    for d, want in TABLE + [(d, w) for d, _, w in TABLE_PAIRS]:
        s = src(d)
        refused(L, lib, ctx, lib.gpet_grad_images_multi(ctx.h, s.rp, 2, s.pix, M, N, 1, s.kps, s.khs, s.kws, s.dn, 2, s.fo, s.ko, s.flags,
                                                        op), want, ("grad_images_multi", d))
    # the calls' own arguments come before everything about the frames
    s = src(("pix", "null"))
    refused(L, lib, ctx, lib.gpet_grad_images(ctx.h, s.rp, 0, s.pix, M, N, s.kp, s.kh, s.kw, 0, op), GRAD_BAD, "no images")
    refused(L, lib, ctx, lib.gpet_grad_images(ctx.h, s.rp, 2, s.pix, M, N, s.kp, s.kh, s.kw, 0, (_P * 2)(out[0].ctypes.data, None)),
            "gpet_grad_images: output image 1 is a null pointer", "null output")
    s = src(("frame_of", "pix"))  # (with a table: the table, then the outputs, then the frames)
    refused(L, lib, ctx, lib.gpet_grad_images_multi(ctx.h, s.rp, 2, s.pix, M, N, 1, s.kps, s.khs, s.kws, None, 2, s.fo, s.ko, 0,
                                                    (_P * 2)(out[0].ctypes.data, None)), T_RANGE, "table before outputs")

    # gpet_denoise_images: no kernel; a median window of 3 x 3 where the spec is not the defect
    good = L.GpetDenoise(technique=L.DN_MEDIAN, size_y=3, size_x=3)
    n_it = (C.c_int32 * 2)()
    for d, want in [(("pix",), PIX7), (("null",), NULL1), (("dn",), DN_BAD), (("pix", "null"), PIX7), (("pix", "dn"), PIX7),
                    (("dn", "null"), DN_BAD)]:
        s = src(d)
        refused(L, lib, ctx, lib.gpet_denoise_images(ctx.h, s.rp, 2, s.pix, M, N, s.dn or C.byref(good), 0, op, n_it), want,
                ("denoise_images", d))
    s = src(("pix", "null"))
    refused(L, lib, ctx, lib.gpet_denoise_images(ctx.h, s.rp, 2, s.pix, M, N, None, 0, op, n_it), "gpet_denoise_images: bad argument", "no spec")
    refused(L, lib, ctx, lib.gpet_denoise_images(ctx.h, s.rp, 2, s.pix, M, N, C.byref(L.GpetDenoise(technique=L.DN_NONE)), 0, op, n_it),
            "gpet_denoise_images: no technique", "no technique")
    refused(L, lib, ctx, lib.gpet_denoise_images(ctx.h, s.rp, 2, s.pix, M, N, C.byref(good), 0, (_P * 2)(out[0].ctypes.data, None), n_it),
            "gpet_denoise_images: output image 1 is a null pointer", "null output")

    # the two stages of their own: bad arguments, and null frames and outputs (one message for both)
    nlm = L.nlmeans_spec(dict(patch_size=3, patch_distance=2, fast_mode=False))
    wv, keep = L.wavelet_spec(dict(wavelet="db1")).for_frames(2, (M, N))
    for name, fn, spec in (("gpet_nlmeans_images", lib.gpet_nlmeans_images, nlm.arg()), ("gpet_wavelet_images", lib.gpet_wavelet_images, C.byref(wv))):
        bad, null1 = name + ": bad argument", name + ": frame or output 1 is a null pointer"
        s, g = src(("null",)), src(())
        refused(L, lib, ctx, fn(ctx.h, s.rp, 2, s.pix, M, N, spec, 0, op), null1, (name, "null frame"))
        refused(L, lib, ctx, fn(ctx.h, g.rp, 2, g.pix, M, N, spec, 0, (_P * 2)(out[0].ctypes.data, None)), null1, (name, "null output"))
        refused(L, lib, ctx, fn(ctx.h, None, 2, g.pix, M, N, spec, 0, op), bad, (name, "no frames"))
        refused(L, lib, ctx, fn(ctx.h, g.rp, 2, g.pix, M, N, spec, 0, None), bad, (name, "no outputs"))
        refused(L, lib, ctx, fn(ctx.h, g.rp, 2, g.pix, M, N, None, 0, op), bad, (name, "no spec"))
        refused(L, lib, ctx, fn(ctx.h, s.rp, 0, s.pix, M, N, spec, 0, op), bad, (name, "no images, null frame"))
        refused(L, lib, ctx, fn(ctx.h, s.rp, 2, s.pix, 0, N, spec, 0, op), bad, (name, "no rows, null frame"))
    del keep
    # and the context still makes gradient images
    s = src(())
    assert lib.gpet_grad_images(ctx.h, s.rp, 2, s.pix, M, N, s.kp, s.kh, s.kw, 0, op) == L.OK


# ---- batch creation and the set calls --------------------------------------------------------------------------------------------
def test_batch_calls_and_the_batch_traces_on(amd, ctx):
    L, lib = amd._lib, ctx.lib
    frames, init = [], None
    for t in range(2):
        img, truth = orc.synth_sinusoid_image(NB, 2 + t, amplitude=int(0.4 * NB * (1.0 + 0.02 * t)))
        init = truth[[0, -1], :][:, [1, 0]] if init is None else init
        frames.append(np.ascontiguousarray(np.rint(img * 255.0).astype(np.uint8)))
    k = np.ascontiguousarray(amd.gpet_utils.kernel_builder((11, 5)), dtype=np.float64)
    mk = lambda: amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames, grad_kernel=k, _ctx=ctx, **KW)
    bt, twin = mk(), mk()
    pa = (L.GpetParams * 2)(*[amd.gpet.to_abi_params(p) for p in bt._ps])
    ini = [np.ascontiguousarray(p["init"], dtype=np.int64) for p in bt._ps]
    ip = (_P * 2)(*[i.ctypes.data for i in ini])
    io = (C.c_int32 * 2)(0, 1)
    src = lambda d: Source(L, frames, k, d)

    def created(rc, h, want, what):
        refused(L, lib, ctx, rc, want, what)
        assert not h.value, what

    for d, want in SINGLE_DN:
        s, h = src(d), _P()
        want = RAW_BAD if want == "bad" else want
        if "dn" not in d:
            created(lib.gpet_batch_create_raw(ctx.h, 2, NB, NB, s.rp, s.pix, s.kp, s.kh, s.kw, 0, pa, ip, s.flags, C.byref(h)), h, want,
                    ("create_raw", d))
        created(lib.gpet_batch_create_raw_dn(ctx.h, 2, NB, NB, s.rp, s.pix, s.kp, s.kh, s.kw, s.dn, 0, pa, ip, s.flags, C.byref(h)), h, want,
                ("create_raw_dn", d))
        created(lib.gpet_batch_create_raw_mapped(ctx.h, 2, NB, NB, 2, io, s.rp, s.pix, s.kp, s.kh, s.kw, s.dn, pa, ip, s.flags, C.byref(h)), h,
                want, ("create_raw_mapped", d))
    band = L.GpetBand(NB, 2, None, io)  # (bands of the frame's own height hold any init rows; placed from the inits)
    for d, want in TABLE + [(d, w) for d, w, _ in TABLE_PAIRS]:
        s, h = src(d), _P()
        created(lib.gpet_batch_create_raw_multi(ctx.h, 2, NB, NB, 2, io, 2, s.rp, s.pix, 1, s.kps, s.khs, s.kws, s.fo, s.ko, s.dn, pa, ip,
                                                s.flags, C.byref(h)), h, want, ("create_raw_multi", d))
        im = L.GpetBandImages()
        im.raw, im.pix, im.n_frames, im.n_kern = C.cast(s.rp, C.POINTER(_P)), s.pix, 2, 1
        im.kern, im.kh, im.kw, im.frame_of, im.kernel_of = C.cast(s.kps, C.POINTER(_P)), s.khs, s.kws, s.fo, s.ko
        if s.spec is not None:
            im.dn = C.pointer(s.spec)
        im.flags = s.flags
        created(lib.gpet_batch_create_banded(ctx.h, 2, NB, NB, C.byref(band), C.byref(im), pa, ip, C.byref(h)), h, want, ("create_banded", d))
    # a table whose slot count is not the batch's: the count IS the batch's image count at creation, so the image map names it --
    # three slots for two edges -- ahead of everything about the frames
    s, h = src(("pix", "null")), _P()
    created(lib.gpet_batch_create_raw_multi(ctx.h, 2, NB, NB, 3, io, 2, s.rp, s.pix, 1, s.kps, s.khs, s.kws, s.fo, s.ko, None, pa, ip, 0,
                                            C.byref(h)), h, "image map: more image slots than edges (B = 2, n_img = 3)", "three slots")
    created(lib.gpet_batch_create_raw_multi(ctx.h, 2, NB, NB, 1, io, 2, s.rp, s.pix, 1, s.kps, s.khs, s.kws, s.fo, s.ko, None, pa, ip, 0,
                                            C.byref(h)), h, "image map: image_of holds an index outside [0, n_img) (B = 2, n_img = 1)", "one slot")
    # one slot that both edges read, of two frames: the table is checked against the slot count it was given
    s, h = src(()), _P()
    created(lib.gpet_batch_create_raw_multi(ctx.h, 2, NB, NB, 1, (C.c_int32 * 2)(0, 0), 2, s.rp, s.pix, 1, s.kps, s.khs, s.kws, s.fo, s.ko,
                                            None, pa, ip, 0, C.byref(h)), h,
            "slot table: a frame no slot reads (n_frames = 2, n_kern = 1, n_img = 1)", "one slot of two frames")

    # the set calls on the live batch (created without GPET_FRAMES_TRANSPOSED: the flag alone is refused, before the kernel)
    for d, want in SINGLE_DN:
        s = src(d)
        want = RAW_BAD if want == "bad" else ORIENT if "tr" in d else want
        if "dn" not in d:
            refused(L, lib, ctx, lib.gpet_batch_set_raw_images(bt._batch.h, s.rp, s.pix, s.kp, s.kh, s.kw, s.flags), want, ("set_raw", d))
        refused(L, lib, ctx, lib.gpet_batch_set_raw_images_dn(bt._batch.h, s.rp, s.pix, s.kp, s.kh, s.kw, s.dn, s.flags), want, ("set_raw_dn", d))
    for d, want in TABLE + [(d, w) for d, w, _ in TABLE_PAIRS]:
        s = src(d)
        refused(L, lib, ctx, lib.gpet_batch_set_raw_images_multi(bt._batch.h, 2, s.rp, s.pix, 1, s.kps, s.khs, s.kws, s.fo, s.ko, s.dn, s.flags),
                ORIENT if "tr" in d else want, ("set_raw_multi", d))
    s = src(())  # (three frames announced for the batch's two slots: the table of the batch's slot count does not reach frame 2)
    refused(L, lib, ctx, lib.gpet_batch_set_raw_images_multi(bt._batch.h, 3, s.rp, s.pix, 1, s.kps, s.khs, s.kws, s.fo, s.ko, None, 0),
            "slot table: a frame no slot reads (n_frames = 3, n_kern = 1, n_img = 2)", "three frames")
    # after all the refused calls the batch is what its untouched twin is
    got, want = bt(), twin()
    assert bt.timings["iters"] == twin.timings["iters"]
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    bt._batch.close()
    twin._batch.close()
