"""GPU tests of the raw-frame path: gpet_grad_images (gpet_utils.comp_grad_imgs), gpet_batch_create_raw and
gpet_batch_set_raw_images (GP_Edge_Tracing_Batch(raw_imgs=...), set_frame(raw_imgs=...), SequenceTracer(grad_kernel=...)).

Every result is DEFINED as equal, bit for bit, to what the two-step path gives -- comp_grad_img per frame, then a batch on the
float32 gradient images -- so everything below is np.array_equal, except the all-NaN gradient image of a flat frame (equal_nan)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gpet_oracle as orc

pytestmark = pytest.mark.gpu

KERNELS = [(4, 4), (3, 6), (2, 5), (1, 1), (7, 1)]  # the even and odd extents of test_grad_image_500_and_even_kernels


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def seeded_stack(dtype, T, M, N, seed):
    rng = np.random.default_rng(seed)
    if dtype == "uint8":
        return rng.integers(0, 256, size=(T, M, N), dtype=np.uint8)
    if dtype == "uint16":
        return rng.integers(0, 65536, size=(T, M, N), dtype=np.uint16)
    if dtype == "float32":
        return rng.random(size=(T, M, N), dtype=np.float32)
    return rng.random(size=(T, M, N))


def per_frame(amd, ctx, stack, k):
    return np.stack([amd.gpet_utils.comp_grad_img(f, k, ctx=ctx) for f in stack])


# ---- gpet_grad_images ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stage_rbf64", "stage_rbf65", "stage_mat128", "stage_mat15_96", "stage_mat35_96"])
def test_f64_frames_equal_the_reference_gradient_images(amd, ctx, golden, name):
    g = golden(name)
    out = amd.gpet_utils.comp_grad_imgs([g["in_img"]], g["in_kernel"], ctx=ctx)
    assert out.dtype == np.float32 and out.shape == (1,) + g["in_img"].shape
    assert np.array_equal(out[0], g["ref_grad"])
    assert np.array_equal(out[0], amd.gpet_utils.comp_grad_img(g["in_img"], g["in_kernel"], ctx=ctx))


def test_f64_500_equals_the_reference_gradient_image(amd, ctx, golden):
    img, _ = orc.synth_sinusoid_image(500, 1)
    other, _ = orc.synth_sinusoid_image(500, 2)
    k = amd.gpet_utils.kernel_builder((11, 5))
    out = amd.gpet_utils.comp_grad_imgs(np.stack([other, img, other]), k, ctx=ctx)  # (its neighbours in the stack do not matter)
    assert np.array_equal(out[1], golden("stage_rbf500")["ref_grad"])
    assert np.array_equal(out[0], out[2]) and not np.array_equal(out[0], out[1])


@pytest.mark.parametrize("shape", [(500, 500), (37, 53)])
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32"])
def test_stacks_equal_per_frame_calls(amd, ctx, dtype, shape):
    """8 seeded frames of every narrow pixel type at both sizes, with the reference's kernel and with even and odd extents."""
    stack = seeded_stack(dtype, 8, shape[0], shape[1], seed=shape[0] + len(dtype))
    rng = np.random.default_rng(0)
    for k in [amd.gpet_utils.kernel_builder((11, 5))] + [rng.normal(size=ks) for ks in KERNELS]:
        got = amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx)
        assert got.dtype == np.float32 and got.shape == stack.shape
        assert np.array_equal(got, per_frame(amd, ctx, stack, k)), (dtype, shape, k.shape)
    # a list of frames is the same as the stack; another dtype means its float64 values
    k = amd.gpet_utils.kernel_builder((11, 5))
    assert np.array_equal(amd.gpet_utils.comp_grad_imgs(list(stack), k, ctx=ctx), amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx))
    if dtype == "uint8":
        assert np.array_equal(amd.gpet_utils.comp_grad_imgs(stack.astype(np.int32), k, ctx=ctx),
                              amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx))


def test_f64_even_and_odd_kernels_equal_the_cpu_implementation(amd, ctx):
    rng = np.random.default_rng(0)
    small = rng.normal(size=(3, 37, 53))
    for ks in KERNELS:
        kk = rng.normal(size=ks)
        got = amd.gpet_utils.comp_grad_imgs(small, kk, ctx=ctx)
        for t in range(3):
            assert np.array_equal(got[t], orc.comp_grad_img(small[t], kk)), (ks, t)


def test_a_stack_larger_than_the_staging_ring(amd, ctx):
    """70 float64 frames of 500 x 500 are three chunks of 33 + 33 + 4 (tests/test_raw_frames_host.py pins that plan): later
    chunks reuse the staging slot the earlier ones went through."""
    stack = seeded_stack("float64", 70, 500, 500, seed=7)
    k = amd.gpet_utils.kernel_builder((11, 5))
    got = amd.gpet_utils.comp_grad_imgs(stack, k, ctx=ctx)
    for t in range(70):
        assert np.array_equal(got[t], amd.gpet_utils.comp_grad_img(stack[t], k, ctx=ctx)), t
    # and the context's staging serves a smaller call afterwards
    assert np.array_equal(amd.gpet_utils.comp_grad_imgs(stack[68:], k, ctx=ctx), got[68:])


# ---- batches from raw frames ---------------------------------------------------------------------------------------------------------
def drifting_frames(N, T, seed0, dtype):
    """T frames of one drifting sinusoidal edge (tests/test_gpu_sequence.py::make_sequence), as raw frames of ``dtype``."""
    frames, init = [], None
    for t in range(T):
        img, truth = orc.synth_sinusoid_image(N, seed0 + t, amplitude=int(0.4 * N * (1.0 + 0.02 * t)))
        if init is None:
            init = truth[[0, -1], :][:, [1, 0]]
        if dtype == "uint8":
            frames.append(np.rint(img * 255.0).astype(np.uint8))
        elif dtype == "uint16":
            frames.append(np.rint(img * 65535.0).astype(np.uint16))
        else:
            frames.append(img.astype(dtype))
    return frames, init


CONFIGS = {
    # RBF, every training point on the grid: the structured loop path
    "rbf256": (256, "uint8", dict(kernel_options={'kernel': 'RBF', 'sigma_f': 40, 'length_scale': 12}, noise_y=1, N_samples=300,
                                  score_thresh=1, delta_x=6, keep_ratio=0.1, pixel_thresh=4, fix_endpoints=True)),
    # Matern-5/2: full-rank posterior, the any-rank factor
    "matern512": (512, "float32", dict(kernel_options={'kernel': 'Matern', 'nu': 2.5, 'sigma_f': 0.15 * 512, 'length_scale': 0.04 * 512},
                                       noise_y=1, N_samples=300, score_thresh=1, delta_x=8, keep_ratio=0.1, pixel_thresh=5,
                                       fix_endpoints=True)),
}


def assert_same_batch(amd, a, b, what):
    """Images, gradient KDEs, then (run both) traces, credible intervals and iteration counts of two batch objects."""
    L = amd._lib
    n_img = 1 if a._batch.share_image else a.B
    for e in range(n_img):
        assert np.array_equal(a._batch.read(L.BUF_GRAD, e), b._batch.read(L.BUF_GRAD, e)), (what, "grad", e)
        assert np.array_equal(a._batch.read(L.BUF_GRAD_KDE, e), b._batch.read(L.BUF_GRAD_KDE, e)), (what, "grad kde", e)
    ra, rb = a(), b()
    assert a.timings["iters"] == b.timings["iters"] and min(a.timings["iters"]) >= 1, (what, a.timings["iters"], b.timings["iters"])
    for e, ((ta, (la, ua)), (tb, (lb, ub))) in enumerate(zip(ra, rb)):
        assert np.array_equal(ta, tb), (what, "trace", e)
        assert np.array_equal(la, lb) and np.array_equal(ua, ub), (what, "interval", e)


@pytest.mark.parametrize("share", [True, False], ids=["shared", "per_edge"])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_batch_from_raw_frames_equals_batch_from_gradient_images(amd, ctx, cfg, share):
    N, dtype, kw = CONFIGS[cfg]
    B = 3
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, 3 if share else 3 * B, 21, dtype)
    sets = [frames[0], frames[1], frames[2]] if share else [frames[0:B], frames[B:2 * B], frames[2 * B:3 * B]]
    grad = lambda s: (amd.gpet_utils.comp_grad_img(s, k, ctx=ctx) if share else [amd.gpet_utils.comp_grad_img(f, k, ctx=ctx) for f in s])
    seeds = [3, 4, 5]
    raw = amd.GP_Edge_Tracing_Batch([init] * B, None, seeds, raw_imgs=sets[0], grad_kernel=k, return_std=True, _ctx=ctx, **kw)
    two = amd.GP_Edge_Tracing_Batch([init] * B, grad(sets[0]), seeds, return_std=True, _ctx=ctx, **kw)
    assert raw._batch.share_image == two._batch.share_image == share
    info = raw._batch.info(0)
    assert info["structured"] == (1 if cfg == "rbf256" else 0) and (info["factor_cap"] > 96) == (cfg != "rbf256")
    assert_same_batch(amd, raw, two, "construction")
    raw.set_frame(raw_imgs=sets[1], seeds=[6, 7, 8], next_frame=False)
    two.set_frame(grad(sets[1]), seeds=[6, 7, 8], next_frame=False)
    assert_same_batch(amd, raw, two, "set_frame(next_frame=False)")
    raw.set_frame(raw_imgs=sets[2], seeds=[9, 10, 11], next_frame=True)
    two.set_frame(grad(sets[2]), seeds=[9, 10, 11], next_frame=True)
    assert_same_batch(amd, raw, two, "set_frame(next_frame=True)")
    raw._batch.close()
    two._batch.close()


def test_one_image_batches_take_the_frame_bare_or_in_a_list(amd, ctx):
    """Whether one image is shared is decided at construction; set_frame then takes that one frame as an (M, N) array or as a list
    of one, for a batch of one edge (one image per edge) and for a batch sharing its image alike."""
    N, dtype, kw = CONFIGS["rbf256"]
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, 2, 31, dtype)
    for B, first in ((1, [frames[0]]), (1, frames[0]), (3, frames[0])):
        bt = amd.GP_Edge_Tracing_Batch([init] * B, None, list(range(3, 3 + B)), raw_imgs=first, grad_kernel=k, _ctx=ctx, **kw)
        got = []
        for nxt in (frames[1], [frames[1]]):
            bt.set_frame(raw_imgs=nxt, next_frame=False)
            got.append((bt._batch.read(amd._lib.BUF_GRAD, 0), bt()))
        assert np.array_equal(got[0][0], amd.gpet_utils.comp_grad_img(frames[1], k, ctx=ctx)) and np.array_equal(got[0][0], got[1][0])
        assert all(np.array_equal(x, y) for x, y in zip(got[0][1], got[1][1]))
        with pytest.raises(ValueError):
            bt.set_frame(raw_imgs=[frames[0], frames[1]], next_frame=False)
        bt._batch.close()


def test_sequence_tracer_on_raw_frames(amd, ctx):
    """SequenceTracer(raw, grad_kernel=K) == SequenceTracer([comp_grad_img(f, K) ...]): 6 frames in 2 chains (construction,
    then set_frame with warm-start observations), Matern-5/2 at 512 as tests/test_gpu_sequence.py traces it."""
    N, T = 512, 6
    kw = CONFIGS["matern512"][2]
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, T, 11, "uint8")
    seeds = [3 + t for t in range(T)]
    a = amd.SequenceTracer(frames, init, n_chains=2, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, **kw)
    b = amd.SequenceTracer([amd.gpet_utils.comp_grad_img(f, k, ctx=ctx) for f in frames], init, n_chains=2, warm_every=16,
                           seeds=seeds, _ctx=ctx, **kw)
    ra, rb = a(), b()
    assert a.iterations == b.iterations and min(a.iterations) >= 1
    for t in range(T):
        assert np.array_equal(ra[t], rb[t]), t
    rc = amd.trace_sequence(frames, init, n_chains=2, warm_every=16, seeds=seeds, _ctx=ctx, grad_kernel=k, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(rc, ra))


def test_history_free_after_set_frame_with_raw_frames(amd, ctx):
    """A batch that traced frames A and is then given frames B (set_frame(raw_imgs=B, next_frame=False)) gives exactly what a
    fresh raw-frame batch on B gives -- Matern, where the any-rank factor could carry rows over."""
    N = 128
    kw = dict(kernel_options={'kernel': 'Matern', 'nu': 2.5, 'sigma_f': 0.15 * N, 'length_scale': 0.04 * N}, noise_y=1,
              N_samples=200, score_thresh=1, delta_x=8, keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
    k = amd.gpet_utils.kernel_builder((11, 5))
    fa, init = drifting_frames(N, 2, 5, "uint16")
    fb, _ = drifting_frames(N, 2, 9, "uint16")
    seeds = [3, 4]

    def run(bt):
        traces = bt()
        return [np.array(t) for t in traces], list(bt.timings["iters"]), [np.array(o) for o in bt._batch.read_obs_all()]

    fresh = amd.GP_Edge_Tracing_Batch([init] * 2, None, seeds, raw_imgs=fb, grad_kernel=k, _ctx=ctx, **kw)
    want = run(fresh)
    fresh._batch.close()
    used = amd.GP_Edge_Tracing_Batch([init] * 2, None, [11, 12], raw_imgs=fa, grad_kernel=k, _ctx=ctx, **kw)
    run(used)
    used.set_frame(raw_imgs=fb, seeds=seeds, next_frame=False)
    got = run(used)
    used._batch.close()
    assert got[1] == want[1] and min(want[1]) >= 1
    assert all(np.array_equal(x, y) for x, y in zip(got[0], want[0]))
    assert all(np.array_equal(x, y) for x, y in zip(got[2], want[2]))


# ---- flat frames, errors ---------------------------------------------------------------------------------------------------------------
def test_flat_frame_gives_an_all_nan_gradient_image_on_both_paths(amd, ctx):
    L = amd._lib
    k = amd.gpet_utils.kernel_builder((11, 5))
    flat = np.zeros((64, 64), dtype=np.uint8)
    one = amd.gpet_utils.comp_grad_img(flat, k, ctx=ctx)          # status OK: a failing call raises GpetError
    many = amd.gpet_utils.comp_grad_imgs([flat, flat], k, ctx=ctx)
    assert np.all(np.isnan(one)) and np.all(np.isnan(many))
    assert np.array_equal(many[0], one, equal_nan=True) and np.array_equal(many[1], one, equal_nan=True)
    # a flat frame beside a live one: each image has its own (min, max)
    live = seeded_stack("uint8", 1, 64, 64, seed=3)[0]
    mixed = amd.gpet_utils.comp_grad_imgs([live, flat, live], k, ctx=ctx)
    assert np.all(np.isnan(mixed[1])) and np.array_equal(mixed[0], amd.gpet_utils.comp_grad_img(live, k, ctx=ctx))
    assert np.array_equal(mixed[2], mixed[0])
    init = np.array([[0, 32], [63, 32]])
    kw = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1,
              delta_x=5, keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
    raw = amd.GP_Edge_Tracing_Batch([init], None, [1], raw_imgs=flat, grad_kernel=k, _ctx=ctx, **kw)  # (constructed, not traced)
    two = amd.GP_Edge_Tracing_Batch([init], one, [1], _ctx=ctx, **kw)
    ga, gb = raw._batch.read(L.BUF_GRAD, 0), two._batch.read(L.BUF_GRAD, 0)
    assert np.all(np.isnan(ga)) and np.array_equal(ga, gb, equal_nan=True)
    raw._batch.close()
    two._batch.close()


def test_bad_arguments_are_refused_and_the_batch_traces_on(amd, ctx):
    L = amd._lib
    N = 128
    kw = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 20, 'length_scale': 8}, noise_y=1, N_samples=300, score_thresh=1,
              delta_x=8, keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
    k = amd.gpet_utils.kernel_builder((11, 5))
    frames, init = drifting_frames(N, 2, 2, "uint8")

    def broken(which):
        raw = L.RawFrames(np.ones((45, 45)) if which == "kernel" else k, frames=frames)
        if which == "pix":
            raw.pix = 7
        if which == "null":
            raw.ptrs[1] = 0
        return raw

    def refused(call, text):
        with pytest.raises(L.GpetError) as ei:
            call()
        assert ei.value.code == L.ERR_BAD_ARG and text in str(ei.value), str(ei.value)

    texts = dict(pix="pixel type 7", null="frame 1 is a null pointer", kernel="45 x 45 kernel")
    for which, text in texts.items():
        refused(lambda: ctx.grad_images(broken(which)), text)
    want = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames, grad_kernel=k, _ctx=ctx, **kw)
    want_traces = want()
    from gaussian_process_edge_trace_amd.gpet import to_abi_params
    params = [to_abi_params(p) for p in want._ps]
    for which, text in texts.items():
        refused(lambda: L.Batch(ctx, None, params, [init, init], raw=broken(which)), text)
    bt = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=frames, grad_kernel=k, _ctx=ctx, **kw)
    for which, text in texts.items():
        refused(lambda: bt._batch.set_images(raw=broken(which)), text)
    got = bt()  # the batch is as it was: it traces, and to the same result
    assert bt.timings["iters"] == want.timings["iters"]
    assert all(np.array_equal(x, y) for x, y in zip(got, want_traces))
    assert np.array_equal(ctx.grad_images(L.RawFrames(k, frames=frames)), per_frame(amd, ctx, frames, k))  # and so does the context
    bt._batch.close()
    want._batch.close()


# ---- frames that already live on the GPU ---------------------------------------------------------------------------------------------
RAWPTR_WORKER = r'''
import sys
import torch  # FIRST (INTEGRATION.md section 4)
sys.path.insert(0, %(root)r)
import numpy as np
import gaussian_process_edge_trace_amd as amd
from oracle import gpet_oracle as orc  # (synthetic images only)
L = amd._lib
N = 128
ctx = amd._lib.Context(0)
k = amd.gpet_utils.kernel_builder((11, 5))
kw = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 20, 'length_scale': 8}, noise_y=1, N_samples=300, score_thresh=1,
          delta_x=8, keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)
imgs, init = [], None
for s in (2, 3, 4, 5):
    img, truth = orc.synth_sinusoid_image(N, s)
    imgs.append(img)
    init = truth[[0, -1], :][:, [1, 0]]
for dtype, tdt in (("uint8", torch.uint8), ("float32", torch.float32)):
    host = [np.rint(i * 255.0).astype(np.uint8) if dtype == "uint8" else i.astype(np.float32) for i in imgs]
    dev = [torch.from_numpy(h).to("cuda") for h in host]
    assert all(d.is_cuda and d.is_contiguous() and d.dtype == tdt for d in dev)
    torch.cuda.synchronize()
    ptrs = [d.data_ptr() for d in dev]
    # gpet_grad_images on device frames
    g_host = ctx.grad_images(L.RawFrames(k, frames=host))
    g_dev = ctx.grad_images(L.RawFrames(k, device_ptrs=ptrs, dtype=dtype, shape=(N, N)))
    assert np.array_equal(g_host, g_dev)
    # one shared frame
    a = amd.GP_Edge_Tracing_Batch([init] * 3, None, [3, 4, 5], raw_imgs=host[0], grad_kernel=k, _ctx=ctx, **kw)
    b = amd.GP_Edge_Tracing_Batch([init] * 3, None, [3, 4, 5], raw_device_ptrs=[ptrs[0]], raw_dtype=dtype, grad_shape=(N, N),
                                  grad_kernel=k, _ctx=ctx, **kw)
    assert b._batch.share_image
    assert np.array_equal(a._batch.read(L.BUF_GRAD), b._batch.read(L.BUF_GRAD))
    assert np.array_equal(a._batch.read(L.BUF_GRAD_KDE), b._batch.read(L.BUF_GRAD_KDE))
    for x, y in zip(a(), b()):
        assert np.array_equal(x, y)
    # one frame per edge, then set_frame
    a2 = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_imgs=host[0:2], grad_kernel=k, _ctx=ctx, **kw)
    b2 = amd.GP_Edge_Tracing_Batch([init] * 2, None, [3, 4], raw_device_ptrs=ptrs[0:2], raw_dtype=dtype, grad_shape=(N, N),
                                   grad_kernel=k, _ctx=ctx, **kw)
    for e in range(2):
        assert np.array_equal(a2._batch.read(L.BUF_GRAD, e), b2._batch.read(L.BUF_GRAD, e))
    for x, y in zip(a2(), b2()):
        assert np.array_equal(x, y)
    a2.set_frame(raw_imgs=host[2:4], seeds=[6, 7])
    b2.set_frame(raw_device_ptrs=ptrs[2:4], seeds=[6, 7])  # (the dtype is remembered from construction)
    assert np.array_equal(a2._batch.read(L.BUF_GRAD_KDE, 1), b2._batch.read(L.BUF_GRAD_KDE, 1))
    for x, y in zip(a2(), b2()):
        assert np.array_equal(x, y)
    # the device frames are read, never written
    for h, d in zip(host, dev):
        assert np.array_equal(d.cpu().numpy(), h)
print("raw device pointers ok")
'''


def test_device_resident_raw_frames_equal_host_frames(tmp_path):
    """GPET_RAW_ON_DEVICE: uint8 and float32 torch CUDA tensors, handed over by data_ptr(), give what the same frames on the host
    give.  One fresh child process that imports torch FIRST (as test_device_pointer_images_equal_host_images does): torch ships
    its own HIP runtime and a process must hold only one."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rawptr_worker.py"
    script.write_text(RAWPTR_WORKER % dict(root=root))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "raw device pointers ok" in r.stdout
