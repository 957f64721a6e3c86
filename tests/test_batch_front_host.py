"""CPU tests of the batch's Python front end one level above the library: ``_lib.Batch`` is replaced by a recording stand-in, so the
constructor and ``set_frame`` of ``GP_Edge_Tracing_Batch`` run without a device.  Pinned: what ``_lib.Batch`` is created with for
every form the images come in, the sequence of device calls ``set_frame`` makes (as its docstring states it), that the next frames
inherit kernels, slot table, dtype and denoising from the constructor, and that images which are refused are refused before the
first device call."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib, gpet

M = N = 64
H = 32
K = np.ones((11, 5))
K2 = -np.ones((11, 5))
FRAME = (np.arange(M * N) % 251).astype(np.uint8).reshape(M, N)
GRAD = np.zeros((M, N), dtype=np.float32)
INITS = [np.array([[0, 20], [N - 1, 22]]), np.array([[0, 40], [N - 1, 38]])]
V_INITS = [np.array([[20, 0], [22, M - 1]]), np.array([[40, 0], [38, M - 1]])]  # (x, y) of the frame: vertical edges
ENSEMBLE_KEYS = ("trace", "median", "q_lo", "q_hi", "min", "max", "agree", "members", "off", "cost", "medoid", "best_cost")
SENTINEL = ["the ensemble of the frame before"]


class RecordingBatch(object):
    """Stands in for ``_lib.Batch``: keeps the arguments it was created with, derives what the front end reads from them by the
    library's rules -- one shared image: 1; an image map (a slot table's included): its count; else one per edge -- and records
    every other call."""
    RETURNS = dict(init_follow=lambda b, *a: b.inits, read_obs_all=lambda b: [np.zeros((0, 2), dtype=np.int64)] * b.B,
                   ensemble_kept=lambda b: ([{k: np.zeros((4, 2), dtype=np.int64) if k == "trace" else np.zeros(4) for k in ENSEMBLE_KEYS}], None, None),
                   band_r0=lambda b: list(b.r0))

    def __init__(self, ctx, grads, params, inits, share_image=False, device_ptrs=None, shape=None, raw=None, image_of=None, band=None,
                 transposed=False):
        self.made = dict(grads=grads, share_image=share_image, device_ptrs=device_ptrs, shape=shape, raw=raw, image_of=image_of, band=band,
                         transposed=transposed)
        self.B, self.inits, self.calls = len(params), [np.array(i, dtype=np.int64) for i in inits], []
        self.share_image, self.image_of, self.transposed = share_image, image_of, transposed
        self.n_img = 1 if share_image else (max(image_of) + 1 if image_of is not None else self.B)
        self.frame_shape = tuple(raw.shape) if raw is not None else (tuple(shape) if device_ptrs is not None else tuple(grads[0].shape))
        self.frame_M = self.frame_shape[1] if transposed else self.frame_shape[0]
        if band is not None:  # (placed from the init rows where no table is given)
            spans = [gpet.init_row_span(i) for i in self.inits]
            self.r0 = list(band[1]) if band[1] is not None else [_lib.band_place(self.frame_M, band[0], lo, hi, lo, hi) for lo, hi in spans]

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **kw):
            self.calls.append((name, a, kw))
            if name == "band_set":
                self.r0 = list(a[0])
            return self.RETURNS.get(name, lambda b, *a, **kw: None)(self, *a)
        return call


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    monkeypatch.setattr(gpet._lib, "Batch", RecordingBatch)


def make(inits=INITS, grad_imgs=None, **kw):
    """(the batch, what its _lib.Batch was created with); the calls of the constructor are dropped from the record."""
    b = gpet.GP_Edge_Tracing_Batch(inits, grad_imgs, list(range(len(inits))), _ctx=object(), **kw)
    b._batch.calls.clear()
    return b, b._batch.made


def names(b):
    return [c[0] for c in b._batch.calls]


def the_call(b, name):
    got = [c for c in b._batch.calls if c[0] == name]
    assert len(got) == 1
    return got[0]


# ---- creation ---------------------------------------------------------------------------------------------------------------------

def test_gradient_images_shared_per_edge_and_on_the_device():
    _, made = make(grad_imgs=GRAD)
    assert made["share_image"] and made["image_of"] is None and made["raw"] is None and made["band"] is None and not made["transposed"]
    assert len(made["grads"]) == 1 and made["grads"][0].dtype == np.float32 and made["grads"][0].shape == (M, N)
    _, made = make(grad_imgs=[GRAD, GRAD + 1])
    assert not made["share_image"] and made["image_of"] is None and len(made["grads"]) == 2
    _, made = make(grad_device_ptrs=[4096, 8192], grad_shape=(M, N))
    assert made["grads"] is None and made["device_ptrs"] == [4096, 8192] and tuple(made["shape"]) == (M, N) and not made["share_image"]
    _, made = make(grad_device_ptrs=4096, grad_shape=(M, N))
    assert made["device_ptrs"] == [4096] and made["share_image"]


def test_raw_frames_shared_per_edge_stacked_and_on_the_device():
    for frames, share, n in ((FRAME, True, 1), ([FRAME, FRAME], False, 2), (np.stack([FRAME, FRAME]), False, 2)):
        _, made = make(raw_imgs=frames, grad_kernel=K)
        raw = made["raw"]
        assert made["grads"] is None and made["share_image"] == share and made["image_of"] is None
        assert (len(raw), raw.n_slots, raw.slots, tuple(raw.shape), raw.src_shape) == (n, n, None, (M, N), (M, N))
        assert raw.dn is None and raw.pre is None and raw.polar is None and np.array_equal(raw.kernel, K)
    _, made = make(raw_device_ptrs=[4096, 8192], raw_dtype=np.uint16, grad_shape=(M, N), grad_kernel=K)
    raw = made["raw"]
    assert raw.frames is None and raw.ptrs == [4096, 8192] and raw.pix == _lib.pix_code(np.uint16) and tuple(raw.shape) == (M, N)
    assert not made["share_image"]


def test_image_map():
    inits = INITS + INITS
    _, made = make(inits, raw_imgs=[FRAME, FRAME], grad_kernel=K, image_of=[0, 0, 1, 1])
    assert not made["share_image"] and made["image_of"] == [0, 0, 1, 1] and len(made["raw"]) == 2 and made["raw"].slots is None
    _, made = make(inits, grad_imgs=[GRAD], image_of=[0, 0, 0, 0])  # (a map of one image: the library decides that it is shared)
    assert not made["share_image"] and made["image_of"] == [0, 0, 0, 0] and len(made["grads"]) == 1
    with pytest.raises(ValueError, match="3 images for an image map of n_img = 2"):
        make(inits, raw_imgs=[FRAME] * 3, grad_kernel=K, image_of=[0, 0, 1, 1])
    with pytest.raises(ValueError, match="image_of has 3 entries for 4 edges"):
        make(inits, raw_imgs=[FRAME] * 2, grad_kernel=K, image_of=[0, 0, 1])


def test_kernel_list_with_and_without_an_image_map():
    b, made = make(raw_imgs=FRAME, grad_kernel=[K, K2], kernel_of=[0, 1])
    raw = made["raw"]
    assert not made["share_image"] and made["image_of"] == [0, 1]  # (the edge-to-slot map)
    assert (len(raw), raw.n_slots, raw.slots) == (1, 2, ([0, 0], [0, 1])) and [k.tolist() for k in raw.kernels] == [K.tolist(), K2.tolist()]
    assert b.default_map_of() == [0, 0]
    inits = INITS + INITS
    b, made = make(inits, raw_imgs=[FRAME, FRAME], grad_kernel=[K, K2], kernel_of=[0, 1, 1, 1], image_of=[0, 0, 1, 1])
    raw = made["raw"]
    assert made["image_of"] == [0, 1, 2, 2] and (len(raw), raw.n_slots, raw.slots) == (2, 3, ([0, 0, 1], [0, 1, 1]))
    assert b.default_map_of() == [0, 0, 1, 1]
    with pytest.raises(ValueError, match="kernel_of has 1 entries for 2 edges"):
        make(raw_imgs=FRAME, grad_kernel=[K, K2], kernel_of=[0])


def test_bands_placed_and_given():
    b, made = make(raw_imgs=FRAME, grad_kernel=K, band_rows=H)
    assert made["band"] == (H, None) and tuple(made["raw"].shape) == (M, N) and made["share_image"]
    assert b.band_rows == H and list(b.band_r0) == [5, 23] and b._ps[0]["M"] == H  # (placed by the stand-in from rows 20 .. 22, 38 .. 40)
    b, made = make(grad_imgs=[GRAD, GRAD], band_rows=H, band_r0=[10, 30])
    assert made["band"] == (H, [10, 30]) and list(b.band_r0) == [10, 30] and not made["share_image"]


def test_vertical_and_vertical_with_bands():
    b, made = make(V_INITS, raw_imgs=np.zeros((48, N), dtype=np.uint8), grad_kernel=K, orientation="vertical")
    assert made["transposed"] and tuple(made["raw"].shape) == (48, N) and made["band"] is None
    assert (b._ps[0]["M"], b._ps[0]["N"]) == (N, 48) and b.orientation == "vertical"
    assert [i.tolist() for i in b.inits] == [[[20, 0], [22, M - 1]], [[40, 0], [38, M - 1]]]
    b, made = make(V_INITS, raw_imgs=FRAME, grad_kernel=K, orientation="vertical", band_rows=H, band_r0=[10, 30])
    assert made["transposed"] and made["band"] == (H, [10, 30]) and (b._ps[0]["M"], b._ps[0]["N"]) == (H, M)


def test_polar():
    spec = dict(centre=(32.0, 31.0), n_r=24, n_theta=48)
    inits = [np.array([[2, 10], [50, 10]])]
    b, made = make(inits, raw_imgs=FRAME, grad_kernel=K, polar=spec)
    raw = made["raw"]
    assert raw.polar.pad == 2 and tuple(raw.shape) == (24, 48 + 1 + 2 * 2) and raw.src_shape == (M, N) and made["share_image"]
    assert b.polar is raw.polar and (b._ps[0]["M"], b._ps[0]["N"]) == (24, 53)
    with pytest.raises(ValueError, match="polar and orientation='vertical' are alternatives"):
        make(inits, raw_imgs=FRAME, grad_kernel=K, polar=spec, orientation="vertical")
    with pytest.raises(ValueError, match="polar needs raw frames"):
        make(inits, grad_imgs=GRAD, polar=spec)


def test_denoise_in_the_pass_and_as_a_stage_of_its_own():
    _, made = make(raw_imgs=FRAME, grad_kernel=K, denoise=("median", dict(size=3)))
    assert made["raw"].dn is not None and made["raw"].dn.technique == _lib.DN_MEDIAN and made["raw"].pre is None
    _, made = make(raw_imgs=FRAME, grad_kernel=K, denoise=("tvb", dict(weight=2.0)))
    assert made["raw"].dn is None and isinstance(made["raw"].pre, _lib.TvbSpec)
    with pytest.raises(ValueError, match="denoise needs raw frames"):
        make(grad_imgs=GRAD, denoise=("median", dict(size=3)))


# ---- the device calls of set_frame, in order ---------------------------------------------------------------------------------------

def test_set_frame_with_obs():
    b, _ = make(grad_imgs=GRAD)
    obs = [np.array([[10, 21], [30, 22]]), np.zeros((0, 2))]
    b.set_frame(GRAD + 1, obs=obs, seeds=[7, 8])
    assert names(b) == ["set_images", "set_obs"]
    kw = the_call(b, "set_images")[2]
    assert kw["next_frame"] is True and len(kw["grads"]) == 1 and kw["grads"][0][0, 0] == 1.0
    e, o = the_call(b, "set_obs")[1]
    assert e == 0 and o.tolist() == [[10, 21], [30, 22]] and b.seeds == [7, 8] and [p["seed"] for p in b._ps] == [7, 8]


def test_set_frame_with_warm_every():
    b, _ = make(grad_imgs=GRAD)
    b.set_frame(GRAD, warm_every=5, next_frame=False)
    assert names(b) == ["warm_start_ready", "set_images", "warm_start", "read_obs_all"]
    assert the_call(b, "warm_start")[1] == (5,) and the_call(b, "set_images")[2]["next_frame"] is False


def test_set_frame_with_warm_every_and_warm_from():
    b, _ = make(grad_imgs=GRAD)
    b.set_frame(GRAD, warm_every=5, warm_from="medoid", group_of=[0, 0], tol=3)
    assert names(b) == ["warm_start_ready", "ensemble_keep", "ensemble_kept", "set_images", "warm_start_groups", "read_obs_all"]
    groups, tol = the_call(b, "ensemble_keep")[1]
    assert groups.tolist() == [0, 0] and tol == 3 and the_call(b, "warm_start_groups")[1] == ("medoid", 5)
    assert len(b.last_ensemble) == 1 and set(b.last_ensemble[0]) == set(ENSEMBLE_KEYS)


def test_set_frame_with_bands_that_follow():
    b, _ = make(raw_imgs=FRAME, grad_kernel=K, band_rows=H)
    b.set_frame(raw_imgs=FRAME, band="follow")
    assert names(b) == ["warm_start_ready", "band_place", "set_images", "band_r0"]
    assert the_call(b, "band_place")[2] == dict(frm=None)
    b._batch.calls.clear()
    b.set_frame(raw_imgs=FRAME, warm_every=4)  # ('follow' is the default with warm_every)
    assert names(b) == ["warm_start_ready", "band_place", "set_images", "warm_start", "read_obs_all", "band_r0"]


def test_set_frame_with_bands_and_init_points_given():
    b, _ = make(raw_imgs=FRAME, grad_kernel=K, band_rows=H)
    new = [INITS[0] + [0, 2], INITS[1] - [0, 2]]
    b.set_frame(raw_imgs=FRAME, band=[8, 20], init=new)
    assert names(b) == ["band_set", "set_images", "set_init", "band_r0"]
    assert the_call(b, "band_set")[1] == ([8, 20],) and list(b.band_r0) == [8, 20]
    assert [i.tolist() for i in the_call(b, "set_init")[1][0]] == [n.tolist() for n in new] == [i.tolist() for i in b.inits]
    with pytest.raises(ValueError, match="band of edge 0"):  # (rows 22 .. 24 are not in rows 30 .. 61)
        b.set_frame(raw_imgs=FRAME, band=[30, 20])


def test_set_frame_with_init_follow():
    b, _ = make(raw_imgs=FRAME, grad_kernel=K)
    b.set_frame(raw_imgs=FRAME, init="follow", init_follow=dict(window=4, cols=2))
    assert names(b) == ["set_images", "init_follow"] and the_call(b, "init_follow")[1] == (4, 2)


def test_set_frame_with_denoise_false():
    b, _ = make(raw_imgs=FRAME, grad_kernel=K, denoise=("median", dict(size=3)))
    b.set_frame(raw_imgs=FRAME)
    assert names(b) == ["set_images"] and the_call(b, "set_images")[2]["raw"].dn.technique == _lib.DN_MEDIAN
    b._batch.calls.clear()
    b.set_frame(raw_imgs=FRAME, denoise=False)
    raw = the_call(b, "set_images")[2]["raw"]
    assert names(b) == ["set_images"] and raw.dn is None and raw.pre is None


def test_set_frame_with_new_centres():
    spec = dict(centre=(32.0, 31.0), n_r=24, n_theta=48)
    b, made = make([np.array([[2, 10], [50, 10]])], raw_imgs=FRAME, grad_kernel=K, polar=spec)
    b.set_frame(raw_imgs=FRAME)
    assert names(b) == ["set_images"] and the_call(b, "set_images")[2]["raw"].polar is made["raw"].polar
    b._batch.calls.clear()
    b.set_frame(raw_imgs=FRAME, polar=dict(centre=(30.0, 33.0)))
    raw = the_call(b, "set_images")[2]["raw"]
    assert names(b) == ["set_images"] and raw.polar.centre.tolist() == [[30.0, 33.0]] and b.polar is raw.polar
    assert (raw.polar.n_r, raw.polar.n_theta, raw.polar.pad) == (24, 48, 2) and tuple(raw.shape) == (24, 53) and raw.src_shape == (M, N)
    with pytest.raises(ValueError, match="cannot change the shape of the polar frames"):
        b.set_frame(raw_imgs=FRAME, polar=dict(n_r=25))
    assert b.polar is raw.polar


# ---- what the next frames inherit --------------------------------------------------------------------------------------------------

def test_next_frames_take_kernels_table_dtype_and_denoise_from_the_constructor():
    inits = INITS + INITS
    b, made = make(inits, raw_device_ptrs=[4096, 8192], raw_dtype=np.uint16, grad_shape=(M, N), grad_kernel=[K, K2],
                   kernel_of=[0, 1, 1, 1], image_of=[0, 0, 1, 1], denoise=("gaussian", dict(sigma=1.5)))
    b.set_frame(raw_device_ptrs=[12288, 16384])
    first, raw = made["raw"], the_call(b, "set_images")[2]["raw"]
    assert raw.ptrs == [12288, 16384] and raw.frames is None and raw.pix == first.pix == _lib.pix_code(np.uint16)
    assert raw.slots == first.slots == ([0, 0, 1], [0, 1, 1]) and [k.tolist() for k in raw.kernels] == [K.tolist(), K2.tolist()]
    assert bytes(raw.dn) == bytes(first.dn) and raw.dn.technique == _lib.DN_GAUSSIAN and tuple(raw.shape) == (M, N)
    b._batch.calls.clear()
    b.set_frame(raw_imgs=[FRAME, FRAME], grad_kernel=[K2, K], denoise=("median", dict(size=3)))  # (what the call gives wins)
    raw = the_call(b, "set_images")[2]["raw"]
    assert raw.pix == _lib.pix_code(np.uint8) and raw.dn.technique == _lib.DN_MEDIAN and raw.slots == first.slots
    assert [k.tolist() for k in raw.kernels] == [K2.tolist(), K.tolist()]
    # a single kernel on per-edge frames
    b, made = make(raw_imgs=[FRAME, FRAME], grad_kernel=K)
    b.set_frame(raw_imgs=np.stack([FRAME, FRAME]).astype(np.float32))
    raw = the_call(b, "set_images")[2]["raw"]
    assert np.array_equal(raw.kernel, K) and raw.slots is None and len(raw) == 2 and raw.pix == _lib.pix_code(np.float32)


# ---- refused images are refused before the first device call -----------------------------------------------------------------------

REFUSED = [
    (dict(raw_imgs=[FRAME, FRAME], grad_kernel=K), dict(raw_imgs=[FRAME] * 3),
     "the new frames do not fit the batch: 3 given (one image per edge, 2, 64 x 64)"),
    (dict(grad_device_ptrs=4096, grad_shape=(M, N)), dict(grad_device_ptrs=[4096, 8192]),
     "the new images do not fit the batch: 2 given (one shared image)"),
    (dict(grad_imgs=GRAD), dict(grad_imgs=[GRAD, GRAD]),
     "the new images do not fit the batch: 2 given (one shared image, 64 x 64)"),
    (dict(grad_imgs=GRAD), dict(grad_imgs=GRAD, denoise=("median", dict(size=3))),
     "denoise needs raw frames (raw_imgs / raw_device_ptrs)"),
]


@pytest.mark.parametrize("ctor,call,text", REFUSED, ids=["raw-frames", "device-gradients", "host-gradients", "denoise-without-raw"])
def test_refused_images_leave_the_ensemble_alone(ctor, call, text):
    b, _ = make(**ctor)
    b.last_ensemble = SENTINEL
    with pytest.raises(ValueError) as err:
        b.set_frame(warm_every=5, warm_from="medoid", group_of=[0, 0], **call)
    assert str(err.value) == text
    assert b._batch.calls == [] and b.last_ensemble is SENTINEL
