"""GPU tests of vertical edges: ``orientation='vertical'`` on GP_Edge_Tracing_Batch, trace_sequence and trace_ensemble,
``comp_grad_imgs(transpose=True)``, GPET_FRAMES_TRANSPOSED in the C ABI; k_conv_tr_batch, k_conv_tr_multi and k_transpose_f32.

A vertical batch is DEFINED as the horizontal batch on the transposed gradient image of every frame with the two coordinates of
every point swapped, so everything below is np.array_equal -- equal_nan only for the all-NaN gradient image of a flat frame, as in
tests/test_gpu_raw_frames.py.  The batch tests trace a 160 x 96 frame with one edge running down it (a 96 x 160 test image,
transposed); the stage tests use stacks at the edges of the 64 x 16 convolution tile, of its 16 x 64 transposed form and of the
64 x 64 transpose tile."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_denoise import DeviceFrames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 64), (17, 65), (37, 53), (130, 33), (33, 130)]
KERNELS = [(4, 4), (3, 6), (2, 5), (1, 1), (7, 1)]  # the even and odd extents of tests/test_gpu_raw_frames.py
DTYPES = ["uint8", "uint16", "float32", "float64"]
# the RBF options of the small batch tests (tests/test_gpu_bands.py, tests/test_gpu_init_follow.py)
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
FM, FN = 160, 96  # the frame: 160 rows of 96 pixels


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def kernels(amd):
    return [amd.gpet_utils.kernel_builder((11, 5), vertical_edges=True), amd.gpet_utils.kernel_builder((7, 3), vertical_edges=True)]


def seeded_stack(dtype, T, M, N, seed):
    rng = np.random.default_rng(seed)
    if dtype == "uint8":
        return rng.integers(0, 256, size=(T, M, N), dtype=np.uint8)
    if dtype == "uint16":
        return rng.integers(0, 65536, size=(T, M, N), dtype=np.uint16)
    if dtype == "float32":
        return rng.random(size=(T, M, N), dtype=np.float32)
    return rng.random(size=(T, M, N))


def vertical_frame(amd, seed, dtype, amplitude=38):
    """(frame, init): ``construct_test_img((96, 160), ...)[0].T`` -- one edge running down a 160 x 96 frame -- as ``dtype``, and
    the edge's two end points as (x, y) of the frame."""
    img, edge = amd.gpet_utils.construct_test_img((FN, FM), amplitude, 2, 0.05, 'sinusoidal', 0.3, gaps=False, seed=seed)
    frame = np.ascontiguousarray(img.T)
    frame = np.rint(frame * 255.0).astype(np.uint8) if dtype == "uint8" else frame.astype(dtype)
    assert frame.shape == (FM, FN)
    return frame, np.ascontiguousarray(edge[[0, -1]])  # edge rows are (row, column) of the 96 x 160 image = (x, y) of the frame


@pytest.fixture(scope="module")
def scene(amd, ctx, kernels):
    """Per dtype: 6 frames of the drifting edge, the init, and the TRANSPOSED gradient images of every frame for both kernels, made on
    the host from the horizontal stage -- computed once, read by every batch test."""
    out = {}
    for dtype in ("uint8", "float64"):
        made = [vertical_frame(amd, 40 + t, dtype, amplitude=38 + t) for t in range(6)]
        frames, init = [m[0] for m in made], made[0][1]
        GT = [[np.ascontiguousarray(g.T) for g in amd.gpet_utils.comp_grad_imgs(frames, k, ctx=ctx)] for k in kernels]
        for per_kernel in GT:
            for g in per_kernel:
                g.setflags(write=False)
        out[dtype] = dict(frames=frames, init=init, GT=GT)
    return out


def same(a, b):
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def sw(a):
    """The swap a reference user makes by hand (not the package's helper): the two columns of an (..., 2) array exchanged."""
    if isinstance(a, (tuple, list)):
        return [sw(x) for x in a]
    return np.ascontiguousarray(np.asarray(a)[..., ::-1])


def result_h_to_v(res, return_std):
    """What the horizontal batch returned for an edge, in the frame's coordinates."""
    return (sw(res[0]), res[1]) if return_std else sw(res)


def has_history(amd, batch):
    try:
        return bool(batch._batch.history_layout().level)
    except amd._lib.GpetError:  # (the batch keeps no iteration history)
        return False


def assert_vertical_equals_horizontal(amd, v, h, what, group_of=None):
    """Slot images, then (run both) traces, intervals, iteration counts, final observation sets, init points, every field of
    history(), results(), final_costs() and ensemble(): the vertical batch against the horizontal one on the transposed images."""
    L = amd._lib
    assert v._batch.transposed and not h._batch.transposed
    assert (v._batch.M, v._batch.N) == (h._batch.M, h._batch.N)   # (the image slots may differ: two kernels on one frame are 2, not B)
    for e in range(v.B):
        assert np.array_equal(v._batch.read(L.BUF_GRAD, e), h._batch.read(L.BUF_GRAD, e)), (what, "grad", e)
        assert np.array_equal(v._batch.read(L.BUF_GRAD_KDE, e), h._batch.read(L.BUF_GRAD_KDE, e)), (what, "grad kde", e)
    assert same(v.inits, sw(h.inits)), (what, "inits")
    got, want = v(), h()
    assert v.timings["iters"] == h.timings["iters"] and min(h.timings["iters"]) >= 1, (what, v.timings, h.timings)
    for e, (g, w) in enumerate(zip(got, want)):
        assert same(g, result_h_to_v(w, v.return_std)), (what, "result", e)
        tr = g[0] if v.return_std else g
        assert np.array_equal(tr[:, 0], np.arange(tr[0, 0], tr[0, 0] + len(tr))), (what, "one entry per traced frame row", e)
    assert same(v._batch.read_obs_all(), h._batch.read_obs_all()), (what, "final observations")
    assert np.array_equal(v.final_costs(), h.final_costs()), (what, "final costs")
    (rv, sv), (rh, sh) = v.results(), h.results()
    assert same(rv, [result_h_to_v(r, v.return_std) for r in rh]), (what, "results()")
    assert same(rv, got), (what, "results() against finish")
    assert sorted(sv) == sorted(sh) and all(same(sv[k], sh[k]) for k in sv), (what, "statistics")
    if has_history(amd, v):
        hv, hh = v.history(), h.history()
        for e in range(v.B):
            assert sorted(hv[e]) == sorted(hh[e]) and hv[e]["n_iter"] == hh[e]["n_iter"] >= 1, (what, "history", e)
            for k in hv[e]:
                w = sw(hh[e][k]) if k in ("obs", "optimal_curves") else hh[e][k]
                assert same(hv[e][k], w), (what, "history", e, k)
    ev, eh = v.ensemble(group_of), h.ensemble(group_of)
    assert len(ev) == len(eh)
    for g, (dv, dh) in enumerate(zip(ev, eh)):
        assert sorted(dv) == sorted(dh)
        for k in dv:
            assert same(dv[k], sw(dh[k]) if k == "trace" else dh[k]), (what, "ensemble", g, k)
    return got


# ---- 1. the stage ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stage_equals_the_transposed_horizontal_stage(amd, ctx, dtype, shape):
    """comp_grad_imgs(stack, K, transpose=True) == comp_grad_imgs(stack, K).transpose(0, 2, 1): 3 frames of every pixel type at
    every shape, with the vertical reference kernel and with even and odd extents."""
    stack = seeded_stack(dtype, 3, shape[0], shape[1], seed=shape[0] * 7 + len(dtype))
    rng = np.random.default_rng(0)  # (the draws of tests/test_gpu_raw_frames.py: the 1 x 1 kernel is positive, no image is flat)
    for k in [amd.gpet_utils.kernel_builder((11, 5), vertical_edges=True)] + [rng.normal(size=ks) for ks in KERNELS]:
        want = amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx)
        got = amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx, transpose=True)
        assert got.dtype == np.float32 and got.shape == (3, shape[1], shape[0]) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, want.transpose(0, 2, 1)), (dtype, shape, k.shape)
        assert np.isfinite(want).all() and want.max() == 1.0 and want.min() == 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_stage_with_a_gaussian_that_is_not_symmetric(amd, ctx, shape):
    """sigma=(1, 2) blurs the frame's rows with 1 and its columns with 2, as it lies: the transposed stage is the transpose of the
    horizontal stage with the SAME spec."""
    dn = ('gaussian', dict(sigma=(1.0, 2.0)))
    k = amd.gpet_utils.kernel_builder((11, 5), vertical_edges=True)
    for dtype in ("uint8", "float64"):
        stack = seeded_stack(dtype, 3, shape[0], shape[1], seed=shape[1])
        want = amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx, denoise=dn)
        got = amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx, denoise=dn, transpose=True)
        assert np.array_equal(got, want.transpose(0, 2, 1)), (dtype, shape)
        swapped = amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx, denoise=('gaussian', dict(sigma=(2.0, 1.0))))
        assert not np.array_equal(swapped, want)  # (the spec does tell the axes apart)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stage_with_two_kernels(amd, ctx, kernels, dtype, shape):
    """A list of kernels: (T, 2, N, M), every frame read by both kernels (k_conv_tr_multi); and a slot table in which frame 1 is read
    by both kernels, frame 0 and 2 by one each."""
    stack = seeded_stack(dtype, 3, shape[0], shape[1], seed=shape[0] + 3 * len(dtype))
    ks = [kernels[0], np.random.default_rng(2).normal(size=(4, 6))]
    want = amd.gpet_utils.comp_grad_imgs(stack, ks, ctx=ctx)
    got = amd.gpet_utils.comp_grad_imgs(stack, ks, ctx=ctx, transpose=True)
    assert got.shape == (3, 2, shape[1], shape[0]) and np.array_equal(got, want.transpose(0, 1, 3, 2))
    for j in range(2):
        assert np.array_equal(want[:, j], amd.gpet_utils.comp_grad_imgs(stack, ks[j], ctx=ctx))
    L = amd._lib
    raw = L.RawFrames(ks, frames=stack, slots=([0, 1, 1, 2], [1, 0, 1, 0]))
    slots = ctx.grad_images(raw, transpose=True)
    assert slots.shape == (4, shape[1], shape[0])
    for g, (f, k) in enumerate(zip(*raw.slots)):
        assert np.array_equal(slots[g], want[f, k].T), (g, f, k)


def test_stage_of_a_flat_frame_is_all_nan(amd, ctx, kernels):
    flat = np.zeros((37, 53), dtype=np.uint8)
    live = seeded_stack("uint8", 1, 37, 53, seed=3)[0]
    want = amd.gpet_utils.comp_grad_imgs([live, flat, live], kernels[0], ctx=ctx)
    got = amd.gpet_utils.comp_grad_imgs([live, flat, live], kernels[0], ctx=ctx, transpose=True)
    assert np.all(np.isnan(got[1])) and got[1].shape == (53, 37)
    assert np.array_equal(got, want.transpose(0, 2, 1), equal_nan=True)
    assert np.array_equal(got[0], want[0].T) and np.array_equal(got[2], got[0])  # (each image has its own (min, max))


# ---- 2. batches from raw frames ----------------------------------------------------------------------------------------------------
def build_pair(amd, ctx, kernels, sc, layout, frame0=0, **extra):
    """(vertical batch on raw frames, horizontal batch on the transposed gradient images, group table) for a layout of 4 edges."""
    fr, GT, init = sc["frames"], sc["GT"], sc["init"]
    B, seeds = 4, [3, 4, 5, 6]
    kw = dict(KW, return_std=True, history='full', _ctx=ctx)
    kw.update(extra)
    f = frame0
    if layout == "shared":
        v = dict(raw_imgs=fr[f], grad_kernel=kernels[0])
        h = GT[0][f]
    elif layout == "per_edge":
        v = dict(raw_imgs=fr[f:f + B], grad_kernel=kernels[0])
        h = GT[0][f:f + B]
    elif layout == "mapped":
        v = dict(raw_imgs=fr[f:f + 2], grad_kernel=kernels[0], image_of=[0, 0, 1, 1])
        h = GT[0][f:f + 2]
        kw["image_of"] = [0, 0, 1, 1]
    else:  # two kernels on one shared frame: edges 0, 2 through the first, 1, 3 through the second
        v = dict(raw_imgs=fr[f], grad_kernel=kernels, kernel_of=[0, 1, 0, 1])
        h = [GT[k][f] for k in (0, 1, 0, 1)]
    vkw = {k: w for k, w in kw.items() if k != "image_of"}
    vb = amd.GP_Edge_Tracing_Batch([init] * B, None, seeds, orientation='vertical', **v, **vkw)
    hb = amd.GP_Edge_Tracing_Batch([sw(init)] * B, h, seeds, **kw)
    return vb, hb


@pytest.mark.parametrize("layout", ["shared", "per_edge", "mapped", "two_kernels"])
@pytest.mark.parametrize("dtype", ["uint8", "float64"])
def test_batch_from_raw_frames(amd, ctx, kernels, scene, dtype, layout):
    vb, hb = build_pair(amd, ctx, kernels, scene[dtype], layout)
    assert (vb._batch.M, vb._batch.N) == (FN, FM) and vb._batch.frame_shape == (FM, FN)
    group_of = None if layout in ("shared",) else [0, 0, 1, 1]
    got = assert_vertical_equals_horizontal(amd, vb, hb, (dtype, layout), group_of)
    tr, (lo, hi) = got[0]
    assert tr.shape == (FM, 2) and lo.shape == hi.shape == (FM,)              # one entry per frame row, columns in the interval
    assert np.array_equal(tr[:, 0], np.arange(FM)) and tr[:, 1].min() >= 0 and tr[:, 1].max() < FN
    vb._batch.close()
    hb._batch.close()


def test_batch_from_gradient_images_of_the_caller(amd, ctx, kernels, scene):
    """grad_imgs and grad_device_ptrs with orientation='vertical' are gradient images in the FRAME's layout: normalised and
    transposed on the device (k_transpose_f32), equal to the same images transposed on the host."""
    sc = scene["uint8"]
    B, seeds, init = 4, [3, 4, 5, 6], sc["init"]
    G = [np.ascontiguousarray(g.T) for g in sc["GT"][0][:B]]  # frame layout, 160 x 96
    # (scaled and shifted: the batch re-normalises what it is given)
    G = [(g * np.float32(3.5) + np.float32(0.25)).astype(np.float32) for g in G]
    kw = dict(KW, return_std=True, history='full', _ctx=ctx)
    for share in (True, False):
        given = G[0] if share else G
        vb = amd.GP_Edge_Tracing_Batch([init] * B, given, seeds, orientation='vertical', **kw)
        hb = amd.GP_Edge_Tracing_Batch([sw(init)] * B, np.ascontiguousarray(G[0].T) if share else [np.ascontiguousarray(g.T) for g in G],
                                       seeds, **kw)
        first = assert_vertical_equals_horizontal(amd, vb, hb, ("grad_imgs", share), None if share else [0, 0, 1, 1])
        dev = DeviceFrames(ctx, [G[0]] if share else G)
        try:
            db = amd.GP_Edge_Tracing_Batch([init] * B, None, seeds, grad_device_ptrs=dev.ptrs, grad_shape=(FM, FN),
                                           orientation='vertical', **kw)
            for e in range(B):
                assert np.array_equal(db._batch.read(amd._lib.BUF_GRAD, e), hb._batch.read(amd._lib.BUF_GRAD, e)), (share, e)
            assert same(db(), first)
            assert all(np.array_equal(dev.download(i), g) for i, g in enumerate([G[0]] if share else G))  # (read, never written)
            # the next frame as device pointers and as host images, in frame layout
            nxt = [np.ascontiguousarray(g.T) for g in sc["GT"][0][1:1 + (1 if share else B)]]
            dev2 = DeviceFrames(ctx, nxt)
            try:
                db.set_frame(grad_device_ptrs=dev2.ptrs, next_frame=False)
                vb.set_frame(nxt[0] if share else nxt, next_frame=False)
                hb.set_frame(sc["GT"][0][1] if share else sc["GT"][0][1:1 + B], next_frame=False)
                for e in range(B):
                    assert np.array_equal(db._batch.read(amd._lib.BUF_GRAD, e), hb._batch.read(amd._lib.BUF_GRAD, e)), (share, e)
                    assert np.array_equal(vb._batch.read(amd._lib.BUF_GRAD, e), hb._batch.read(amd._lib.BUF_GRAD, e)), (share, e)
                assert same(db(), vb())
            finally:
                db._batch.close()
                dev2.free()
        finally:
            dev.free()
        vb._batch.close()
        hb._batch.close()


TORCH_WORKER = r'''
import sys
import torch  # FIRST (INTEGRATION.md section 4)
sys.path.insert(0, %(root)r)
import numpy as np
import gaussian_process_edge_trace_amd as amd
L = amd._lib
ctx = L.Context(0)
K = amd.gpet_utils.kernel_builder((11, 5), vertical_edges=True)
kw = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True, return_std=True, _ctx=ctx)
frames, init = [], None
for t in range(4):
    img, edge = amd.gpet_utils.construct_test_img((96, 160), 38 + t, 2, 0.05, 'sinusoidal', 0.3, gaps=False, seed=40 + t)
    frames.append(np.ascontiguousarray(img.T))
    init = np.ascontiguousarray(edge[[0, -1]]) if init is None else init
for dtype, tdt in (("uint8", torch.uint8), ("float64", torch.float64)):
    host = [np.rint(f * 255.0).astype(np.uint8) if dtype == "uint8" else f for f in frames]
    dev = [torch.from_numpy(h).to("cuda") for h in host]
    assert all(d.is_cuda and d.is_contiguous() and d.dtype == tdt and tuple(d.shape) == (160, 96) for d in dev)
    torch.cuda.synchronize()
    ptrs = [d.data_ptr() for d in dev]
    GT = [np.ascontiguousarray(g.T) for g in amd.gpet_utils.comp_grad_imgs(host, K, ctx=ctx)]
    g_dev = ctx.grad_images(L.RawFrames(K, device_ptrs=ptrs, dtype=dtype, shape=(160, 96)), transpose=True)
    assert all(np.array_equal(a, b) for a, b in zip(g_dev, GT))
    v = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_device_ptrs=ptrs[0:2], raw_dtype=dtype, grad_shape=(160, 96),
                                  grad_kernel=K, orientation='vertical', **kw)
    h = amd.GP_Edge_Tracing_Batch([init[:, ::-1]] * 2, GT[0:2], [3, 4], **kw)
    for step in range(2):
        for e in range(2):
            assert np.array_equal(v._batch.read(L.BUF_GRAD, e), h._batch.read(L.BUF_GRAD, e))
        rv, rh = v(), h()
        assert v.timings["iters"] == h.timings["iters"] and min(h.timings["iters"]) >= 1
        for (tv, (lv, uv)), (th, (lh, uh)) in zip(rv, rh):
            assert np.array_equal(tv, th[:, ::-1]) and np.array_equal(lv, lh) and np.array_equal(uv, uh)
        if step == 0:
            v.set_frame(raw_device_ptrs=ptrs[2:4], warm_every=10)   # (the dtype is remembered from construction)
            h.set_frame(GT[2:4], warm_every=10)
    # a shared gradient image as a torch tensor, in frame layout
    gt = torch.from_numpy(np.ascontiguousarray(GT[0].T)).to("cuda")
    torch.cuda.synchronize()
    vg = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], grad_device_ptrs=[gt.data_ptr()], grad_shape=(160, 96),
                                   orientation='vertical', **kw)
    hg = amd.GP_Edge_Tracing_Batch([init[:, ::-1]] * 2, GT[0], [3, 4], **kw)
    assert np.array_equal(vg._batch.read(L.BUF_GRAD), hg._batch.read(L.BUF_GRAD))
    for (tv, _), (th, _) in zip(vg(), hg()):
        assert np.array_equal(tv, th[:, ::-1])
    for hh, d in zip(host, dev):   # the device frames are read, never written
        assert np.array_equal(d.cpu().numpy(), hh)
print("vertical device pointers ok")
'''


def test_device_resident_frames_from_a_torch_tensor(tmp_path):
    """raw_device_ptrs / grad_device_ptrs taken from torch CUDA tensors with orientation='vertical'.  One fresh child process that
    imports torch FIRST, as tests/test_gpu_raw_frames.py does: a process must hold only one HIP runtime."""
    script = tmp_path / "vertical_worker.py"
    script.write_text(TORCH_WORKER % dict(root=ROOT))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "vertical device pointers ok" in r.stdout


# ---- 3. frame change -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["shared", "per_edge", "two_kernels"])
def test_frame_change_with_the_device_warm_start(amd, ctx, kernels, scene, layout):
    sc = scene["uint8"]
    vb, hb = build_pair(amd, ctx, kernels, sc, layout)
    vb(), hb()
    fr, GT = sc["frames"], sc["GT"]
    n = 1 if layout != "per_edge" else 4
    nxt_v = fr[1] if n == 1 else fr[1:5]
    nxt_h = GT[0][1] if layout == "shared" else (GT[0][1:5] if layout == "per_edge" else [GT[k][1] for k in (0, 1, 0, 1)])
    vb.set_frame(raw_imgs=nxt_v, warm_every=10, seeds=[7, 8, 9, 10])
    hb.set_frame(nxt_h, warm_every=10, seeds=[7, 8, 9, 10])
    warm_v, warm_h = vb._batch.read_obs_all(), hb._batch.read_obs_all()
    assert same(warm_v, warm_h) and min(len(o) for o in warm_h) >= 1           # (batch coordinates on the device, both)
    assert same([p["obs"] for p in vb._ps], [p["obs"] for p in hb._ps])
    assert_vertical_equals_horizontal(amd, vb, hb, (layout, "after set_frame"), [0, 0, 1, 1])
    # caller's observations, in frame coordinates: the warm start above handed in by hand
    vb.set_frame(raw_imgs=nxt_v, obs=sw(warm_h), next_frame=False)
    hb.set_frame(nxt_h, obs=warm_h, next_frame=False)
    assert same(vb._batch.read_obs_all(), hb._batch.read_obs_all())
    assert_vertical_equals_horizontal(amd, vb, hb, (layout, "obs by hand"), [0, 0, 1, 1])
    vb._batch.close()
    hb._batch.close()


def test_frame_change_matern(amd, ctx, kernels, scene):
    """The any-rank factor (Matern): bits are compared with next_frame=False, as tests/test_gpu_sequence.py does."""
    sc = scene["float64"]
    kw = dict(kernel_options={'kernel': 'Matern', 'nu': 2.5, 'sigma_f': 0.15 * FN, 'length_scale': 0.04 * FM}, noise_y=1, N_samples=128,
              score_thresh=1, delta_x=8, keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True, history=None)
    vb, hb = build_pair(amd, ctx, kernels, sc, "shared", **kw)
    assert vb._batch.info(0)["factor_cap"] > 96
    assert_vertical_equals_horizontal(amd, vb, hb, "matern")
    vb.set_frame(raw_imgs=sc["frames"][1], warm_every=16, next_frame=False)
    hb.set_frame(sc["GT"][0][1], warm_every=16, next_frame=False)
    assert_vertical_equals_horizontal(amd, vb, hb, "matern after set_frame")
    vb._batch.close()
    hb._batch.close()


# ---- 4. bands and endpoint tracking ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["raw", "two_kernels", "grad"])
def test_bands_and_endpoint_tracking(amd, ctx, kernels, scene, source):
    """band_rows=48 is a band of 48 frame COLUMNS, init_follow searches columns: equal to the horizontal banded batch on the
    full-frame transposed gradient images, through two frame changes."""
    sc = scene["uint8"]
    fr, GT, init = sc["frames"], sc["GT"], sc["init"]
    B, seeds = 2, [3, 4]
    rough = init + np.array([[3, 0], [-2, 0]])            # clicks 3 and 2 columns off the edge: x moves, y never does
    kw = dict(KW, return_std=True, history='full', _ctx=ctx, band_rows=48, init_follow=dict(window=6, cols=3))
    multi = source == "two_kernels"
    ko = [0, 1]

    def v_images(t):
        if source == "grad":
            return dict(grad_imgs=[np.ascontiguousarray(GT[0][t].T), np.ascontiguousarray(GT[0][t + 1].T)])
        if multi:
            return dict(raw_imgs=fr[t])
        return dict(raw_imgs=fr[t:t + 2])

    def h_images(t):
        return [GT[k][t] for k in ko] if multi else [GT[0][t], GT[0][t + 1]]

    ctor = dict(grad_kernel=kernels, kernel_of=ko) if multi else (dict(grad_kernel=kernels[0]) if source == "raw" else {})
    first = v_images(0)
    vb = amd.GP_Edge_Tracing_Batch([rough] * B, first.pop("grad_imgs", None), seeds, orientation='vertical', **first, **ctor, **kw)
    hb = amd.GP_Edge_Tracing_Batch([sw(rough)] * B, h_images(0), seeds, **kw)
    assert (vb._batch.M, vb._batch.N, vb._batch.frame_M, vb._batch.frame_shape) == (48, FM, FN, (FM, FN))
    for step in (1, 2, 3):
        assert [int(r) for r in vb.band_r0] == [int(r) for r in hb.band_r0], step
        assert all(0 <= int(r) <= FN - 48 for r in vb.band_r0)
        assert same(vb.inits, sw(hb.inits)), step
        assert all(np.array_equal(i[:, 1], rough[:, 1]) for i in vb.inits)     # y never moves
        assert_vertical_equals_horizontal(amd, vb, hb, (source, "step", step), [0, 1])
        if step == 3:
            break
        vb.set_frame(warm_every=10, **v_images(step))
        hb.set_frame(h_images(step), warm_every=10)
    assert any(not np.array_equal(i, rough) for i in vb.inits)                 # (the search did move a point)
    vb._batch.close()
    hb._batch.close()


def test_a_band_that_cannot_hold_the_init_points_is_refused(amd, ctx, kernels, scene):
    sc = scene["uint8"]
    wide = np.array([[10, 0], [80, FM - 1]])              # init columns 10 and 80: 71 columns do not fit 48
    with pytest.raises(ValueError, match="band of edge 0"):
        amd.GP_Edge_Tracing_Batch([wide], None, [1], raw_imgs=sc["frames"][0], grad_kernel=kernels[0], band_rows=48,
                                  orientation='vertical', _ctx=ctx, **KW)
    with pytest.raises(ValueError, match="band of edge 0"):  # more band columns than the frame has
        amd.GP_Edge_Tracing_Batch([sc["init"]], None, [1], raw_imgs=sc["frames"][0], grad_kernel=kernels[0], band_rows=FN + 1,
                                  orientation='vertical', _ctx=ctx, **KW)
    vb = amd.GP_Edge_Tracing_Batch([sc["init"]], None, [1], raw_imgs=sc["frames"][0], grad_kernel=kernels[0], band_rows=48,
                                   orientation='vertical', _ctx=ctx, **KW)
    want = vb()
    r0 = [int(r) for r in vb.band_r0]
    with pytest.raises(ValueError, match="band of edge 0"):  # a table that leaves the init columns outside
        vb.set_frame(raw_imgs=sc["frames"][1], band=[0 if int(sc["init"][0, 0]) >= 48 else FN - 48], next_frame=False)
    assert [int(r) for r in vb.band_r0] == r0
    vb.reset()
    assert same(vb(), want)                                  # the batch is as it was
    vb._batch.close()


# ---- 5. sequence and ensemble ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ens", [False, True], ids=["plain", "ensemble"])
@pytest.mark.parametrize("n_chains", [1, 2])
def test_trace_sequence(amd, ctx, kernels, scene, n_chains, ens):
    """3 raw frames, 2 edges (both kernels on every frame), against trace_sequence on the transposed gradient images."""
    sc = scene["uint8"]
    frames, init = sc["frames"][:3], sc["init"]
    inits = [init, init + np.array([[1, 0], [0, 0]])]
    kw = dict(KW, return_std=True, _ctx=ctx)
    if ens:
        kw["ensemble_seeds"] = range(3)
    else:
        kw["seeds"] = [5, 6, 7]
    va = amd.SequenceTracer(frames, inits, n_chains=n_chains, warm_every=10, grad_kernel=kernels, orientation='vertical', **kw)
    got = va()
    # the horizontal sequence reads ONE image per frame: run it per edge on that edge's kernel, as the multi-edge docstring defines
    want, iters, hinits = [], [], []
    for k in range(2):
        G = np.ascontiguousarray(amd.gpet_utils.comp_grad_imgs(frames, kernels[k], ctx=ctx).transpose(0, 2, 1))
        hs = amd.SequenceTracer(list(G), sw(inits[k]), n_chains=n_chains, warm_every=10, **kw)
        want.append(hs())
        iters.append(hs.iterations)
        hinits.append(hs.inits)
    for t in range(3):
        for k in range(2):
            assert va.iterations[t][k] == iters[k][t] and np.min(iters[k][t]) >= 1, (t, k)
            assert same(va.inits[t][k], sw(hinits[k][t])), (t, k)
            g, w = got[t][k], want[k][t]
            if not ens:
                assert same(g, result_h_to_v(w, True)), (t, k)
                continue
            assert sorted(g) == sorted(w)
            for key in g:
                if key == "trace":
                    assert same(g[key], sw(w[key])), (t, k, key)
                elif key == "result":
                    assert same(g[key], result_h_to_v(w[key], True)), (t, k, key)
                elif key == "members":  # (edge indices of the step's batch: 2 edges per frame here, 1 there)
                    assert len(g[key]) == len(w[key])
                elif key in ("medoid", "best_cost"):
                    assert (g[key] >= 0) == (w[key] >= 0)
                else:
                    assert same(g[key], w[key]), (t, k, key)
    if n_chains == 1 and not ens:  # (the wrapper)
        again = amd.trace_sequence(frames, inits, n_chains=1, warm_every=10, grad_kernel=kernels, orientation='vertical', **kw)
        assert all(same(a[k], b[k]) for a, b in zip(again, got) for k in range(2))


def test_trace_sequence_with_bands_and_endpoint_tracking(amd, ctx, kernels, scene):
    sc = scene["uint8"]
    frames, init = sc["frames"][:3], sc["init"]
    kw = dict(KW, return_std=True, _ctx=ctx, seeds=[5, 6, 7], band_rows=48, init_follow=dict(window=6, cols=3))
    va = amd.SequenceTracer(frames, init, n_chains=1, warm_every=10, grad_kernel=kernels[0], orientation='vertical', **kw)
    got = va()
    hs = amd.SequenceTracer(sc["GT"][0][:3], sw(init), n_chains=1, warm_every=10, **kw)
    want = hs()
    assert va.iterations == hs.iterations and min(hs.iterations) >= 1
    for t in range(3):
        assert same(got[t], result_h_to_v(want[t], True)), t
        assert same(va.inits[t], sw(hs.inits[t])), t


def test_trace_ensemble(amd, ctx, kernels, scene):
    sc = scene["float64"]
    init = sc["init"]
    kw = dict(KW, return_std=True, _ctx=ctx)
    got = amd.trace_ensemble([init, init + np.array([[1, 0], [0, 0]])], None, [1, 2, 3], raw_imgs=sc["frames"][0], grad_kernel=kernels[0],
                             orientation='vertical', **kw)
    want = amd.trace_ensemble([sw(init), sw(init + np.array([[1, 0], [0, 0]]))], sc["GT"][0][0], [1, 2, 3], **kw)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert sorted(g) == sorted(w) and g["medoid"] >= 0
        for key in g:
            if key == "trace":
                assert same(g[key], sw(w[key])), key
            elif key == "result":
                assert same(g[key], result_h_to_v(w[key], True)), key
            else:
                assert same(g[key], w[key]), key
    # from a gradient image in the frame's layout
    one = amd.trace_ensemble(init, np.ascontiguousarray(sc["GT"][0][0].T), [1, 2, 3], orientation='vertical', **kw)
    assert same(one["trace"], got[0]["trace"]) and same(one["median"], got[0]["median"])


# ---- 6. non-local means in front of a vertical batch -----------------------------------------------------------------------------
def test_nl_means_in_front_of_a_vertical_batch(amd, ctx):
    """'nl' is a stage of its own that hands device frames on: it works unchanged in front of the transposed-store convolution."""
    dn = ('nl', dict(patch_size=3, patch_distance=2, h=0.1, fast_mode=False))
    M, N = 37, 53
    img, edge = amd.gpet_utils.construct_test_img((N, M), 12, 2, 0.02, 'sinusoidal', 0.5, gaps=False, seed=5)
    frame = np.ascontiguousarray(img.T)                      # 37 x 53 float64, one edge running down it
    nxt = np.ascontiguousarray(amd.gpet_utils.construct_test_img((N, M), 13, 2, 0.02, 'sinusoidal', 0.5, gaps=False, seed=6)[0].T)
    init = np.ascontiguousarray(edge[[0, -1]])
    K = amd.gpet_utils.kernel_builder((5, 3), vertical_edges=True)
    kw = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 6, 'length_scale': 5}, noise_y=1, N_samples=128, score_thresh=1, delta_x=4,
              keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True, return_std=True, history='full', _ctx=ctx)
    G = amd.gpet_utils.comp_grad_imgs([frame, nxt], K, ctx=ctx, denoise=dn)
    assert np.array_equal(amd.gpet_utils.comp_grad_imgs([frame, nxt], K, ctx=ctx, denoise=dn, transpose=True), G.transpose(0, 2, 1))
    vb = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frame, grad_kernel=K, denoise=dn, orientation='vertical', **kw)
    hb = amd.GP_Edge_Tracing_Batch([sw(init)] * 2, np.ascontiguousarray(G[0].T), [3, 4], **kw)
    assert_vertical_equals_horizontal(amd, vb, hb, "nl")
    vb.set_frame(raw_imgs=nxt, warm_every=8)                 # (the denoising spec is remembered)
    hb.set_frame(np.ascontiguousarray(G[1].T), warm_every=8)
    assert_vertical_equals_horizontal(amd, vb, hb, "nl after set_frame")
    vb._batch.close()
    hb._batch.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_the_flag_on_a_horizontal_batch_is_refused_and_the_batch_traces_on(amd, ctx, kernels, scene):
    L = amd._lib
    sc = scene["uint8"]
    made = [amd.gpet_utils.construct_test_img((FN, FN), 38, 2, 0.05, 'sinusoidal', 0.3, gaps=False, seed=60 + t) for t in range(2)]
    square = [np.rint(m[0] * 255.0).astype(np.uint8) for m in made]          # 96 x 96: no shape could tell the orientations apart
    init = sw(made[0][1][[0, -1]])
    K = amd.gpet_utils.kernel_builder((11, 5))
    kw = dict(KW, _ctx=ctx)
    bt = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=square, grad_kernel=K, **kw)
    want = bt()
    before = [bt._batch.read(L.BUF_GRAD, e) for e in range(2)]
    raw = L.RawFrames(K, frames=square[::-1])
    kp, kh, kw_ = raw.kernel_args()
    rc = L.load().gpet_batch_set_raw_images(bt._batch.h, raw.pointer_array(), raw.pix, kp, kh, kw_, raw.flags | L.FRAMES_TRANSPOSED)
    assert rc == L.ERR_BAD_ARG
    with pytest.raises(L.GpetError) as ei:
        ctx.check(rc)
    assert "GPET_FRAMES_TRANSPOSED" in str(ei.value)
    g32 = [np.ascontiguousarray(b) for b in before]
    gp = (C.c_void_p * 2)(*[g.ctypes.data for g in g32])
    assert L.load().gpet_batch_set_images(bt._batch.h, gp, L.FRAMES_TRANSPOSED) == L.ERR_BAD_ARG
    assert all(np.array_equal(bt._batch.read(L.BUF_GRAD, e), before[e]) for e in range(2))   # nothing was touched
    bt.reset()
    assert same(bt(), want)
    bt._batch.close()
    # a vertical batch takes the next frames without the bit, and with it
    vb = amd.GP_Edge_Tracing_Batch([sc["init"]] * 2, None, [3, 4], raw_imgs=sc["frames"][:2], grad_kernel=kernels[0],
                                   orientation='vertical', **kw)
    raw = L.RawFrames(kernels[0], frames=sc["frames"][2:4])
    kp, kh, kw_ = raw.kernel_args()
    for flags in (raw.flags, raw.flags | L.FRAMES_TRANSPOSED):
        assert L.load().gpet_batch_set_raw_images(vb._batch.h, raw.pointer_array(), raw.pix, kp, kh, kw_, flags) == 0
        assert all(np.array_equal(vb._batch.read(L.BUF_GRAD, e), sc["GT"][0][2 + e]) for e in range(2))
    vb._batch.close()


def test_frames_of_the_transposed_shape_are_refused_by_python(amd, ctx, kernels, scene):
    sc = scene["uint8"]
    kw = dict(KW, _ctx=ctx)
    vb = amd.GP_Edge_Tracing_Batch([sc["init"]] * 2, None, [3, 4], raw_imgs=sc["frames"][:2], grad_kernel=kernels[0],
                                   orientation='vertical', **kw)
    want = vb()
    turned = [np.ascontiguousarray(f.T) for f in sc["frames"][2:4]]          # 96 x 160: the batch's own shape, not the frame's
    with pytest.raises(ValueError, match="do not fit the batch"):
        vb.set_frame(raw_imgs=turned, next_frame=False)
    with pytest.raises(ValueError, match="do not fit the batch"):
        vb.set_frame([g for g in sc["GT"][0][2:4]], next_frame=False)         # transposed gradient images: the horizontal batch's
    with pytest.raises(ValueError, match="same row"):
        vb.set_frame(raw_imgs=sc["frames"][2:4], init=[np.array([[40, 7], [42, 7]])] * 2, next_frame=False)
    vb.reset()
    assert same(vb(), want)
    # and the horizontal batch refuses frames in a vertical batch's layout, as ever
    hb = amd.GP_Edge_Tracing_Batch([sw(sc["init"])] * 2, sc["GT"][0][:2], [3, 4], **kw)
    with pytest.raises(ValueError, match="do not fit the batch"):
        hb.set_frame([np.ascontiguousarray(g.T) for g in sc["GT"][0][2:4]], next_frame=False)
    vb._batch.close()
    hb._batch.close()
