"""CPU tests of the raw-frame path (gpet_grad_images, gpet_batch_create_raw, gpet_batch_set_raw_images): the ABI surface, what
csrc/gpet_conv_plan.h decides (the header needs no HIP: a small extern "C" shim around it is compiled with the host C++ compiler,
as tests/test_batch_plan.py does), how the Python layer routes dtypes and refuses contradictory arguments, and the machine code of
the batched convolution kernels (no fused multiply-add, no scratch).

Every expected figure of the plan tests is a literal worked out by hand from the rules the issue states (flip both axes; origin
k / 2 - (k even); tiles of 64 x 16 outputs; taps + patch as f64 in LDS, at most 64 KB; chunks of whole images within a 64 MiB slot,
slots used in turn) -- none was produced by the header under test.  The origin rule is checked against scipy.ndimage.convolve itself."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
NEW = ["gpet_grad_images", "gpet_batch_create_raw", "gpet_batch_set_raw_images"]
KERNELS = [(11, 5), (4, 4), (3, 6), (2, 5), (1, 1), (7, 1)]


def _header_text():
    return open(os.path.join(ROOT, "include", "gpet_hip.h")).read()


def _declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text)))


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_raw_frame_calls_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS["gpet_grad_images"][1]) == 11
    assert len(_lib.SYMBOLS["gpet_batch_create_raw"][1]) == 14
    assert len(_lib.SYMBOLS["gpet_batch_set_raw_images"][1]) == 7
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()


def test_pixel_codes_and_flag_agree_between_header_and_python():
    from gaussian_process_edge_trace_amd import _lib
    defs = dict(re.findall(r"#define\s+(GPET_(?:PIX_[A-Z0-9]+|RAW_ON_DEVICE|GRAD_ON_DEVICE|IMAGES_NEXT_FRAME))\s+(\d+)u?\b", _header_text()))
    assert {k: int(v) for k, v in defs.items()} == dict(GPET_PIX_U8=0, GPET_PIX_U16=1, GPET_PIX_F32=2, GPET_PIX_F64=3,
                                                       GPET_RAW_ON_DEVICE=4, GPET_GRAD_ON_DEVICE=1, GPET_IMAGES_NEXT_FRAME=2)
    assert (_lib.PIX_U8, _lib.PIX_U16, _lib.PIX_F32, _lib.PIX_F64) == (0, 1, 2, 3)
    assert _lib.RAW_ON_DEVICE == 4 and _lib.RAW_ON_DEVICE not in (_lib.GRAD_ON_DEVICE, _lib.IMAGES_NEXT_FRAME)
    assert _lib.PIX_OF_DTYPE == {np.dtype("uint8"): 0, np.dtype("uint16"): 1, np.dtype("float32"): 2, np.dtype("float64"): 3}


# ---- csrc/gpet_conv_plan.h through a host-compiled shim --------------------------------------------------------------------------
SHIM = r"""
#include "gpet_conv_plan.h"
using namespace gpet;
extern "C" {
int shim_pix_bytes(int pix) { return pix_bytes(pix); }
void shim_flip(const double* kern, int kh, int kw, double* wf) { conv_flip_taps(kern, kh, kw, wf); }
int shim_origin(int k) { return conv_origin(k); }
long long shim_lds_bytes(int kh, int kw) { return (long long)conv_lds_bytes(kh, kw); }
int shim_fits(int kh, int kw) { return conv_fits_lds(kh, kw) ? 1 : 0; }
void shim_grid(int M, int N, int* out) { const ConvGrid g = conv_grid(M, N); out[0] = g.gx; out[1] = g.gy; out[2] = CONV_TILE_X; out[3] = CONV_TILE_Y; }
// out: per_chunk, n_chunks, slots, slot_bytes; per chunk k: slot, first, count (3 x n_chunks values in `chunks`, room for `room`)
// (ring <= 0: the library's own depth)
int shim_stage(int n_img, long long img_bytes, int ring, long long* out, int* chunks, int room) {
  const StagePlan p = ring > 0 ? stage_plan(n_img, (size_t)img_bytes, STAGE_SLOT_BUDGET, ring) : stage_plan(n_img, (size_t)img_bytes);
  out[0] = p.per_chunk; out[1] = p.n_chunks; out[2] = p.slots; out[3] = (long long)p.slot_bytes;
  out[4] = (long long)STAGE_SLOT_BUDGET; out[5] = STAGE_RING;
  if (p.n_chunks > room) return -1;
  for (int k = 0; k < p.n_chunks; ++k) { *chunks++ = stage_slot(p, k); *chunks++ = stage_first(p, k); *chunks++ = stage_count(p, k, n_img); }
  return 0;
}
}
"""


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = cxx and shutil.which(cxx)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("conv_plan")
    src, so = d / "shim.cpp", d / "libconv_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_lds_bytes.restype = C.c_longlong
    return lib


def _flip(shim, k):
    k = np.ascontiguousarray(k, dtype=np.float64)
    wf = np.empty_like(k)
    shim.shim_flip(k.ctypes.data_as(C.c_void_p), k.shape[0], k.shape[1], wf.ctypes.data_as(C.c_void_p))
    return wf


def test_pixel_sizes(shim):
    assert [shim.shim_pix_bytes(p) for p in (0, 1, 2, 3)] == [1, 2, 4, 8]
    assert [shim.shim_pix_bytes(p) for p in (-1, 4, 7, 1 << 20)] == [0, 0, 0, 0]


ORIGINS = {(11, 5): (5, 2), (4, 4): (1, 1), (3, 6): (1, 2), (2, 5): (0, 2), (1, 1): (0, 0), (7, 1): (3, 0)}


@pytest.mark.parametrize("ks", KERNELS)
def test_flipped_taps_and_origin(shim, ks):
    kh, kw = ks
    k = np.arange(kh * kw, dtype=np.float64).reshape(kh, kw)
    # flipping both axes of a row-major table reverses it end to end
    assert _flip(shim, k).reshape(-1).tolist() == [float(kh * kw - 1 - i) for i in range(kh * kw)]
    assert (shim.shim_origin(kh), shim.shim_origin(kw)) == ORIGINS[ks]


@pytest.mark.parametrize("ks", KERNELS)
def test_taps_and_origin_reproduce_scipy_convolve_on_a_delta_image(shim, ks):
    """out[y, x] = sum_ab wf[a, b] * img[clamp(y + a - oy), clamp(x + b - ox)] -- what the kernels compute from the plan's taps and
    origin -- against scipy.ndimage.convolve(mode='nearest') on delta images (one inside, one in a corner: the edge replication)."""
    ndimage = pytest.importorskip("scipy.ndimage")
    kh, kw = ks
    k = np.random.default_rng(kh * 16 + kw).normal(size=ks)
    wf = _flip(shim, k)
    oy, ox = shim.shim_origin(kh), shim.shim_origin(kw)
    for at in [(9, 7), (0, 0), (16, 12)]:
        img = np.zeros((17, 13))
        img[at] = 1.0
        want = ndimage.convolve(img, k, mode="nearest")
        ys = np.clip(np.arange(17)[:, None] + np.arange(kh)[None, :] - oy, 0, 16)  # [y, a]
        xs = np.clip(np.arange(13)[:, None] + np.arange(kw)[None, :] - ox, 0, 12)  # [x, b]
        got = np.einsum("ab,yaxb->yx", wf, img[ys[:, :, None, None], xs[None, None, :, :]])
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)


def test_grid_and_lds_bytes(shim):
    g = (C.c_int * 4)()
    shim.shim_grid(500, 500, g)
    assert list(g) == [8, 32, 64, 16]
    shim.shim_grid(37, 53, g)  # M = 37 rows, N = 53 columns
    assert list(g) == [1, 3, 64, 16]
    shim.shim_grid(64, 128, g)
    assert list(g)[:2] == [2, 4]
    # (kh kw taps + (16 + kh - 1) x (64 + kw - 1) patch) doubles
    assert shim.shim_lds_bytes(11, 5) == (55 + 26 * 68) * 8 == 14584
    assert shim.shim_lds_bytes(4, 4) == (16 + 19 * 67) * 8 == 10312
    assert shim.shim_lds_bytes(1, 1) == (1 + 16 * 64) * 8 == 8200
    for ks in KERNELS:
        assert shim.shim_fits(*ks) == 1


def test_64k_lds_refusal(shim):
    assert shim.shim_lds_bytes(41, 41) == 60040 and shim.shim_fits(41, 41) == 1
    assert shim.shim_lds_bytes(45, 45) == 68040 and shim.shim_fits(45, 45) == 0
    assert shim.shim_fits(64, 64) == 0 and shim.shim_fits(1, 8000) == 0 and shim.shim_fits(500, 1) == 0
    assert shim.shim_fits(0, 3) == 0 and shim.shim_fits(3, -1) == 0
    # the largest square patch below the line, the smallest above it: (k^2 + (k + 15)(k + 63)) * 8 <= 65536 <=> k <= 43
    assert shim.shim_fits(43, 43) == 1 and shim.shim_fits(44, 44) == 0


def _stage(shim, n_img, img_bytes, ring=0):
    out, chunks = (C.c_longlong * 6)(), (C.c_int * (3 * 4096))()
    assert shim.shim_stage(n_img, C.c_longlong(img_bytes), ring, out, chunks, 4096) == 0
    n = int(out[1])
    return dict(per_chunk=int(out[0]), n_chunks=n, slots=int(out[2]), slot_bytes=int(out[3]), budget=int(out[4]), ring=int(out[5]),
                chunks=[tuple(chunks[3 * k:3 * k + 3]) for k in range(n)])


# 256 frames of 500 x 500 within a 64 MiB slot: (pixel bytes, frames per chunk, chunks, bytes between slots rounded up to 256)
PLANS_256 = {1: (256, 1, 64000000), 2: (134, 2, 67000064), 4: (67, 4, 67000064), 8: (33, 8, 66000128)}


@pytest.mark.parametrize("ring", [0, 1, 2, 3])
@pytest.mark.parametrize("esz", [1, 2, 4, 8])
def test_chunk_plan_256_frames(shim, esz, ring):
    """ring 0: the library's own depth, one slot (a second one was measured and bought nothing); the plan itself cycles through
    any depth it is given."""
    per, n_chunks, slot_bytes = PLANS_256[esz]
    p = _stage(shim, 256, 500 * 500 * esz, ring)
    assert (p["budget"], p["ring"]) == (64 << 20, 1)
    assert (p["per_chunk"], p["n_chunks"], p["slots"], p["slot_bytes"]) == (per, n_chunks, min(n_chunks, max(ring, 1)), slot_bytes)
    assert p["per_chunk"] * 500 * 500 * esz <= p["slot_bytes"] <= (64 << 20) + 255 and p["slot_bytes"] % 256 == 0
    # every frame in exactly one chunk, in order; slots cycle
    seen = []
    for k, (slot, first, count) in enumerate(p["chunks"]):
        assert slot == k % p["slots"] and 1 <= count <= per
        seen += list(range(first, first + count))
    assert seen == list(range(256))
    assert [c[2] for c in p["chunks"]] == [per] * (n_chunks - 1) + [256 - per * (n_chunks - 1)]


@pytest.mark.parametrize("esz,slot_bytes", [(1, 250112), (2, 500224), (4, 1000192), (8, 2000128)])
def test_chunk_plan_one_frame(shim, esz, slot_bytes):
    p = _stage(shim, 1, 500 * 500 * esz)
    assert (p["per_chunk"], p["n_chunks"], p["slots"], p["slot_bytes"]) == (1, 1, 1, slot_bytes)
    assert p["chunks"] == [(0, 0, 1)]


def test_chunk_plan_odd_cases(shim):
    p = _stage(shim, 5, 100 << 20, ring=2)  # an image larger than the budget still goes up, alone
    assert (p["per_chunk"], p["n_chunks"], p["slots"]) == (1, 5, 2)
    assert [c[0] for c in p["chunks"]] == [0, 1, 0, 1, 0] and [c[1] for c in p["chunks"]] == [0, 1, 2, 3, 4]
    assert [c[0] for c in _stage(shim, 5, 100 << 20, ring=3)["chunks"]] == [0, 1, 2, 0, 1]
    p = _stage(shim, 70, 500 * 500 * 8)  # the stack tests/test_gpu_raw_frames.py reuses the staging slot with
    assert (p["per_chunk"], p["n_chunks"], p["slots"]) == (33, 3, 1) and [c for c in p["chunks"]] == [(0, 0, 33), (0, 33, 33), (0, 66, 4)]
    p = _stage(shim, 5, 2 * 1024 * 1024 * 8)  # the stack of tests/test_gpu_nlmeans.py: an f64 frame of 1024 x 1024 and its f64 result
    assert (p["per_chunk"], p["n_chunks"], p["slots"]) == (4, 2, 1) and [c for c in p["chunks"]] == [(0, 0, 4), (0, 4, 1)]
    assert _stage(shim, 0, 1000)["n_chunks"] == 0


# ---- dtype routing and argument checks of the Python layer (no device) ---------------------------------------------------------
K = np.arange(15, dtype=np.float64).reshape(5, 3)


@pytest.mark.parametrize("dtype,pix", [("uint8", 0), ("uint16", 1), ("float32", 2), ("float64", 3)])
def test_native_dtypes_go_up_as_they_are(dtype, pix):
    from gaussian_process_edge_trace_amd import _lib
    stack = (np.arange(3 * 6 * 7).reshape(3, 6, 7) % 251).astype(dtype)
    frames, got = _lib.native_frames(stack)
    assert got == pix and len(frames) == 3
    assert all(f.dtype == np.dtype(dtype) and f.flags.c_contiguous and np.shares_memory(f, stack) for f in frames)  # no copy
    raw = _lib.RawFrames(K, frames=list(stack))
    assert raw.pix == pix and raw.flags == 0 and raw.shape == (6, 7) and len(raw) == 3
    assert raw.ptrs == [stack[t].ctypes.data for t in range(3)]
    assert raw.kernel.dtype == np.float64 and raw.kernel_args()[1:] == (5, 3)


@pytest.mark.parametrize("dtype", ["int8", "int16", "int32", "int64", "uint32", "uint64", "float16", "bool", ">f4", ">u2"])
def test_other_dtypes_are_converted_to_float64(dtype):
    from gaussian_process_edge_trace_amd import _lib
    stack = (np.arange(2 * 4 * 5).reshape(2, 4, 5) % 2).astype(dtype)
    frames, pix = _lib.native_frames(stack)
    assert pix == _lib.PIX_F64 and all(f.dtype == np.float64 and f.dtype.isnative for f in frames)
    assert np.array_equal(np.stack(frames), np.asarray(stack, dtype=np.float64))


def test_mixed_and_strided_frames():
    from gaussian_process_edge_trace_amd import _lib
    frames, pix = _lib.native_frames([np.zeros((4, 5), np.uint8), np.ones((4, 5), np.float32)])
    assert pix == _lib.PIX_F64 and [f.dtype for f in frames] == [np.float64] * 2 and frames[1][0, 0] == 1.0
    big = np.arange(8 * 10, dtype=np.uint16).reshape(8, 10)
    frames, pix = _lib.native_frames([big[::2, ::2]])  # a strided view is made contiguous, in its own dtype
    assert pix == _lib.PIX_U16 and frames[0].flags.c_contiguous and np.array_equal(frames[0], big[::2, ::2])
    with pytest.raises(ValueError):
        _lib.native_frames([np.zeros((4, 5)), np.zeros((5, 4))])
    with pytest.raises(ValueError):
        _lib.native_frames([])
    with pytest.raises(ValueError):
        _lib.native_frames(np.zeros((2, 3, 4, 5)))


def test_device_frames_need_dtype_and_shape():
    from gaussian_process_edge_trace_amd import _lib
    raw = _lib.RawFrames(K, device_ptrs=[4096, 8192], dtype="uint8", shape=(6, 7))
    assert (raw.pix, raw.flags, raw.shape, raw.ptrs, raw.frames) == (0, _lib.RAW_ON_DEVICE, (6, 7), [4096, 8192], None)
    assert _lib.RawFrames(K, device_ptrs=[4096], dtype=np.float32, shape=(6, 7)).pix == 2
    for bad in (dict(dtype=None, shape=(6, 7)), dict(dtype="uint8", shape=None), dict(dtype="int32", shape=(6, 7)),
                dict(dtype="float16", shape=(6, 7))):
        with pytest.raises(ValueError):
            _lib.RawFrames(K, device_ptrs=[4096], **bad)
    with pytest.raises(ValueError):
        _lib.RawFrames(K)
    with pytest.raises(ValueError):
        _lib.RawFrames(K, frames=[np.zeros((4, 4))], device_ptrs=[4096], dtype="uint8", shape=(4, 4))
    with pytest.raises(ValueError):
        _lib.RawFrames(np.zeros(3), frames=[np.zeros((4, 4))])


def test_batch_image_source_routing():
    from gaussian_process_edge_trace_amd import _lib
    from gaussian_process_edge_trace_amd.gpet import resolve_image_source as src
    u8 = np.zeros((3, 6, 7), np.uint8)
    r = src(3, raw_imgs=u8, grad_kernel=K)
    assert (r["kind"], r["share"], r["shape"], r["pix"], r["on_device"]) == ("raw", False, (6, 7), _lib.PIX_U8, False)
    assert isinstance(r["batch"]["raw"], _lib.RawFrames) and r["batch"]["grads"] is None
    r = src(3, raw_imgs=u8[0], grad_kernel=K)  # one 2-D frame: shared by all edges
    assert (r["share"], len(r["batch"]["raw"])) == (True, 1)
    r = src(3, raw_imgs=[f for f in u8.astype(np.float32)], grad_kernel=K)
    assert (r["share"], r["pix"]) == (False, _lib.PIX_F32)
    r = src(3, raw_imgs=u8.astype(np.int32), grad_kernel=K)
    assert r["pix"] == _lib.PIX_F64
    r = src(2, raw_device_ptrs=[4096, 8192], raw_dtype="uint16", grad_shape=(6, 7), grad_kernel=K)
    assert (r["kind"], r["share"], r["shape"], r["pix"], r["on_device"]) == ("raw", False, (6, 7), _lib.PIX_U16, True)
    assert src(2, raw_device_ptrs=4096, raw_dtype="float64", grad_shape=(6, 7), grad_kernel=K)["share"] is True
    # the existing ways in are unchanged
    g = np.ones((6, 7))
    r = src(2, grad_imgs=g)
    assert (r["kind"], r["share"], r["shape"]) == ("grad", True, (6, 7)) and r["batch"]["grads"][0].dtype == np.float32
    r = src(2, grad_imgs=[g, g])
    assert (r["kind"], r["share"], len(r["batch"]["grads"])) == ("grad", False, 2)
    r = src(2, grad_device_ptrs=[4096], grad_shape=(6, 7))
    assert (r["kind"], r["share"], r["batch"]["device_ptrs"]) == ("grad", True, [4096])


def test_batch_image_source_value_errors():
    from gaussian_process_edge_trace_amd.gpet import resolve_image_source as src
    g, u8 = np.ones((6, 7), np.float32), np.zeros((6, 7), np.uint8)
    for bad in (dict(grad_imgs=g, raw_imgs=u8, grad_kernel=K),                                      # both kinds
                dict(grad_device_ptrs=[4096], grad_shape=(6, 7), raw_imgs=u8, grad_kernel=K),
                dict(grad_imgs=g, raw_device_ptrs=[4096], raw_dtype="uint8", grad_shape=(6, 7), grad_kernel=K),
                dict(),                                                                             # none
                dict(raw_imgs=u8),                                                                  # no kernel
                dict(raw_imgs=u8, raw_device_ptrs=[4096], raw_dtype="uint8", grad_shape=(6, 7), grad_kernel=K),
                dict(raw_device_ptrs=[4096], grad_shape=(6, 7), grad_kernel=K),                    # no dtype
                dict(raw_device_ptrs=[4096], raw_dtype="uint8", grad_kernel=K),                    # no shape
                dict(raw_device_ptrs=[4096], raw_dtype="int16", grad_shape=(6, 7), grad_kernel=K),  # not a device pixel type
                dict(raw_imgs=[u8, u8, u8], grad_kernel=K),                                         # 3 frames, 2 edges
                dict(raw_imgs=np.zeros((2, 2, 6, 7)), grad_kernel=K)):
        with pytest.raises(ValueError):
            src(2, **bad)


def test_constructor_refuses_both_kinds_before_it_needs_a_device():
    import gaussian_process_edge_trace_amd as pkg
    init = np.array([[0, 3], [6, 3]])
    with pytest.raises(ValueError):
        pkg.GP_Edge_Tracing_Batch([init], np.ones((6, 7), np.float32), [1], raw_imgs=np.zeros((6, 7), np.uint8), grad_kernel=K)
    with pytest.raises(ValueError):
        pkg.GP_Edge_Tracing_Batch([init], None, [1], raw_imgs=np.zeros((6, 7), np.uint8))
    assert hasattr(pkg.gpet_utils, "comp_grad_imgs")
    import inspect
    assert "grad_kernel" in inspect.signature(pkg.SequenceTracer.__init__).parameters
    assert {"raw_imgs", "raw_device_ptrs"} <= set(inspect.signature(pkg.GP_Edge_Tracing_Batch.set_frame).parameters)


def test_package_does_not_import_torch():
    import sys
    code = ("import sys; sys.path.insert(0, %r); import gaussian_process_edge_trace_amd as p; "
            "from gaussian_process_edge_trace_amd import gpet, sequence, gpet_utils, _lib; print('torch' in sys.modules)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip() == "False"


# ---- machine code of the batched convolution ------------------------------------------------------------------------------------
def _code_objects(tmp_path):
    """The gfx950 code objects of the shipped library, unbundled (as tests/test_results_abi.py::_device_disassembly does)."""
    import __graft_entry__ as ge
    ge.build()
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump")
    so = tmp_path / "lib.so"
    shutil.copy(ge.LIB, so)
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    return objdump, [str(tmp_path / f) for f in sorted(os.listdir(tmp_path)) if "amdgcn" in f]


INSTANCES = {"Ih": "uint8_t", "It": "uint16_t", "If": "float", "Id": "double"}  # Itanium mangling of the template argument


def test_batched_conv_has_no_fused_multiply_add(tmp_path):
    """Bit-exactness with scipy's tap-by-tap sum needs the product rounded before it is added: no v_fma_f64 / v_fmac_f64 in any
    instantiation of k_conv_relu_batch (and, as the yardstick, none in k_conv_relu either)."""
    objdump, objs = _code_objects(tmp_path)
    bodies = {}
    for f in objs:
        text = subprocess.run([objdump, "-d", f], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\S*k_conv_relu\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, flags=re.S | re.M):
            bodies[m.group(1)] = m.group(2)
    batch = {n: b for n, b in bodies.items() if "k_conv_relu_batch" in n}
    for tag, ctype in INSTANCES.items():
        assert any("k_conv_relu_batch" + tag in n for n in batch), "no instantiation for " + ctype
    assert len(batch) == 4 and any("k_conv_relu" in n and "batch" not in n for n in bodies)
    for name, body in bodies.items():
        assert "v_mul_f64" in body and "v_add_f64" in body, name
        assert not re.search(r"v_fmac?_f64", body), name
        assert "scratch_" not in body, name


def test_batched_kernels_use_no_scratch(tmp_path):
    """Resource usage from the code object's metadata: no private segment (scratch), no spilled registers."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("no llvm-readelf")
    _, objs = _code_objects(tmp_path)
    found = {}
    for f in objs:
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:  # one block per kernel; .agpr_count is its first key
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and ("k_conv_relu_batch" in name.group(1) or "k_normalise_f32_batch" in name.group(1)):
                found[name.group(1)] = {k: int(v) for k, v in re.findall(
                    r"\.(private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count|vgpr_count):\s+(\d+)", block)}
    assert len(found) == 5, sorted(found)
    for name, use in found.items():
        assert use["private_segment_fixed_size"] == 0 and use["sgpr_spill_count"] == 0 and use["vgpr_spill_count"] == 0, (name, use)
        assert 0 < use["vgpr_count"] <= 128, (name, use)
