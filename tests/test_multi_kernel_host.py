"""CPU tests of the multi-kernel raw-frame path (gpet_grad_images_multi, gpet_batch_create_raw_multi,
gpet_batch_set_raw_images_multi): what csrc/gpet_conv_multi_plan.h decides (plain data, compiled with the host C++ compiler through
a small extern "C" shim, as tests/test_raw_frames_host.py does for gpet_conv_plan.h), the ABI surface, the Python slot derivation
and the argument errors of the Python layer.

Every expected figure of the plan tests is a literal worked out by hand from the rules: origin k / 2 - (k even); the union halo is
the largest origin (top, left) and the largest kh - 1 - origin (bottom, right) over the kernels; LDS bytes = (sum of kh kw +
(16 + top + bottom) (64 + left + right)) * 8, at most 64 KB; the slots of a frame in ascending slot order."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
NEW = {"gpet_grad_images_multi": 16, "gpet_batch_create_raw_multi": 20, "gpet_batch_set_raw_images_multi": 12}

SHIM = r"""
#include <string.h>
#include "gpet_conv_multi_plan.h"
using namespace gpet;
extern "C" {
// 0 and an empty reason, or 1 and the reason
int shim_check(int n_frames, int n_kern, int n_img, const int32_t* frame_of, const int32_t* kernel_of, char* why, int room) {
  const char* w = slot_table_check(n_frames, n_kern, n_img, frame_of, kernel_of);
  why[0] = 0;
  if (w) strncat(why, w, (size_t)room - 1);
  return w ? 1 : 0;
}
int shim_identity(int n_frames, int n_kern, int n_img, const int32_t* frame_of, const int32_t* kernel_of) {
  return slot_table_is_identity(n_frames, n_kern, n_img, frame_of, kernel_of) ? 1 : 0;
}
// out: top, bottom, left, right, taps, rows, cols, LDS bytes, fits, the cap on kernels, the LDS bound
void shim_union(int n_kern, const int32_t* kh, const int32_t* kw, long long* out) {
  const ConvUnion u = conv_union(n_kern, kh, kw);
  out[0] = u.top; out[1] = u.bottom; out[2] = u.left; out[3] = u.right; out[4] = (long long)u.taps;
  out[5] = conv_union_rows(u); out[6] = conv_union_cols(u); out[7] = (long long)conv_union_lds_bytes(u);
  out[8] = conv_union_fits_lds(n_kern, kh, kw) ? 1 : 0; out[9] = CONV_MULTI_MAX_KERN; out[10] = (long long)CONV_LDS_MAX;
}
// per kernel: kh, kw, dy, dx, w0
void shim_descs(int n_kern, const int32_t* kh, const int32_t* kw, int32_t* out) {
  ConvKernDesc kd[CONV_MULTI_MAX_KERN];
  conv_kern_descs(n_kern, kh, kw, kd);
  for (int k = 0; k < n_kern; ++k) { *out++ = kd[k].kh; *out++ = kd[k].kw; *out++ = kd[k].dy; *out++ = kd[k].dx; *out++ = kd[k].w0; }
}
void shim_frame_slots(int n_frames, int n_img, const int32_t* frame_of, int32_t* off, int32_t* list) {
  frame_slots(n_frames, n_img, frame_of, off, list);
}
long long shim_single_lds(int kh, int kw) { return (long long)conv_lds_bytes(kh, kw); }
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
    d = tmp_path_factory.mktemp("conv_multi_plan")
    src, so = d / "shim.cpp", d / "libconv_multi_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_single_lds.restype = C.c_longlong
    return lib


def i32(v):
    return (C.c_int32 * max(1, len(v)))(*v)


def check(shim, n_frames, n_kern, frame_of, kernel_of):
    why = C.create_string_buffer(256)
    rc = shim.shim_check(n_frames, n_kern, len(frame_of), i32(frame_of), i32(kernel_of), why, 256)
    return rc, why.value.decode()


def union(shim, sizes):
    out = (C.c_longlong * 11)()
    shim.shim_union(len(sizes), i32([s[0] for s in sizes]), i32([s[1] for s in sizes]), out)
    keys = ["top", "bottom", "left", "right", "taps", "rows", "cols", "lds", "fits", "cap", "lds_max"]
    return dict(zip(keys, [int(v) for v in out]))


# ---- the slot table ------------------------------------------------------------------------------------------------------------
def test_valid_tables_pass(shim):
    assert check(shim, 2, 2, [0, 0, 1, 1], [0, 1, 0, 1]) == (0, "")
    assert check(shim, 3, 3, [0, 0, 0, 1, 2, 2], [0, 1, 2, 1, 0, 2]) == (0, "")   # an uneven table
    assert check(shim, 3, 2, [2, 0, 1, 0], [1, 0, 0, 1]) == (0, "")              # slot order interleaves frames
    assert check(shim, 3, 1, [0, 1, 2], [0, 0, 0]) == (0, "")
    assert check(shim, 1, 8, [0] * 8, list(range(8))) == (0, "")                # 8 kernels: the cap itself


@pytest.mark.parametrize("n_frames,n_kern,frame_of,kernel_of,part", [
    (2, 2, [0, 2, 1], [0, 1, 0], "frame index out of range"),
    (2, 2, [0, -1, 1], [0, 1, 0], "frame index out of range"),
    (2, 2, [0, 1, 1], [0, 2, 0], "kernel index out of range"),
    (2, 2, [0, 1, 1], [0, -1, 1], "kernel index out of range"),
    (3, 2, [0, 0, 2], [0, 1, 0], "a frame no slot reads"),
    (2, 3, [0, 0, 1], [0, 2, 0], "a kernel no slot reads"),
    (2, 2, [0, 1, 0, 1, 0], [0, 0, 1, 1, 0], "(frame, kernel) pair twice"),
    (1, 9, [0] * 9, list(range(9)), "more than 8 kernels"),
])
def test_refused_tables_say_why(shim, n_frames, n_kern, frame_of, kernel_of, part):
    rc, why = check(shim, n_frames, n_kern, frame_of, kernel_of)
    assert rc == 1 and part in why, why


def test_refusals_have_distinct_reasons(shim):
    reasons = {check(shim, *t)[1] for t in [(2, 2, [0, 2, 1], [0, 1, 0]), (2, 2, [0, 1, 1], [0, 2, 0]), (3, 2, [0, 0, 2], [0, 1, 0]),
                                             (2, 3, [0, 0, 1], [0, 2, 0]), (1, 1, [0, 0], [0, 0]), (1, 9, [0] * 9, list(range(9)))]}
    assert len(reasons) == 6 and "" not in reasons


def test_identity_table_is_recognised(shim):
    ident = lambda nf, nk, fo, ko: shim.shim_identity(nf, nk, len(fo), i32(fo), i32(ko))
    assert ident(3, 1, [0, 1, 2], [0, 0, 0]) == 1 and ident(1, 1, [0], [0]) == 1
    assert ident(3, 1, [0, 2, 1], [0, 0, 0]) == 0      # another slot order: another arena layout
    assert ident(2, 2, [0, 1], [0, 1]) == 0 and ident(1, 2, [0, 0], [0, 1]) == 0


# ---- the union patch -----------------------------------------------------------------------------------------------------------
def test_union_of_one_kernel_is_the_single_kernel_patch(shim):
    u = union(shim, [(11, 5)])
    assert (u["top"], u["bottom"], u["left"], u["right"]) == (5, 5, 2, 2)
    assert (u["taps"], u["rows"], u["cols"]) == (55, 26, 68)
    assert u["lds"] == (55 + 26 * 68) * 8 == 14584 == shim.shim_single_lds(11, 5) and u["fits"] == 1
    assert (u["cap"], u["lds_max"]) == (8, 65536)


def test_union_of_an_odd_and_an_even_kernel(shim):
    # 11 x 5: origins (5, 2), 5 rows below, 2 columns right;  4 x 6: origins (1, 2), 2 rows below, 3 columns right
    u = union(shim, [(11, 5), (4, 6)])
    assert (u["top"], u["bottom"], u["left"], u["right"]) == (5, 5, 2, 3)
    assert (u["taps"], u["rows"], u["cols"]) == (79, 26, 69)
    assert u["lds"] == (79 + 26 * 69) * 8 == 14984 and u["fits"] == 1
    assert union(shim, [(4, 6), (11, 5)])["lds"] == 14984  # (the order of the kernels does not matter)


def test_union_of_three_small_kernels(shim):
    # 1 x 1: (0, 0 | 0, 0);  3 x 7: origins (1, 3), 1 below, 3 right;  2 x 5: origins (0, 2), 1 below, 2 right
    u = union(shim, [(1, 1), (3, 7), (2, 5)])
    assert (u["top"], u["bottom"], u["left"], u["right"]) == (1, 1, 3, 3)
    assert (u["taps"], u["rows"], u["cols"]) == (32, 18, 70)
    assert u["lds"] == (32 + 18 * 70) * 8 == 10336 and u["fits"] == 1


def test_two_kernels_that_fit_alone_but_not_together(shim):
    # 60 x 1: (60 + 75 * 64) * 8 = 38 880;  1 x 300: (300 + 16 * 363) * 8 = 48 864;  together 75 x 363 + 360 doubles
    assert shim.shim_single_lds(60, 1) == 38880 and union(shim, [(60, 1)])["fits"] == 1
    assert shim.shim_single_lds(1, 300) == 48864 and union(shim, [(1, 300)])["fits"] == 1
    u = union(shim, [(60, 1), (1, 300)])
    assert (u["top"], u["bottom"], u["left"], u["right"]) == (29, 30, 149, 150)
    assert u["lds"] == (360 + 75 * 363) * 8 == 220680 and u["fits"] == 0
    assert union(shim, [(3, 3), (0, 3)])["fits"] == 0 and union(shim, [(3, -1)])["fits"] == 0


def test_kernel_descriptors(shim):
    def descs(sizes):
        out = (C.c_int32 * (5 * len(sizes)))()
        shim.shim_descs(len(sizes), i32([s[0] for s in sizes]), i32([s[1] for s in sizes]), out)
        return [tuple(out[5 * k:5 * k + 5]) for k in range(len(sizes))]
    # (kh, kw, dy = top - origin(kh), dx = left - origin(kw), first tap)
    assert descs([(11, 5)]) == [(11, 5, 0, 0, 0)]
    assert descs([(11, 5), (4, 6)]) == [(11, 5, 0, 0, 0), (4, 6, 4, 0, 55)]
    assert descs([(1, 1), (3, 7), (2, 5)]) == [(1, 1, 1, 3, 0), (3, 7, 0, 0, 1), (2, 5, 1, 1, 22)]


def test_slots_of_each_frame(shim):
    def slots(n_frames, frame_of):
        off, lst = (C.c_int32 * (n_frames + 1))(), (C.c_int32 * len(frame_of))()
        shim.shim_frame_slots(n_frames, len(frame_of), i32(frame_of), off, lst)
        return list(off), list(lst)
    assert slots(3, [0, 1, 0, 2, 1, 0]) == ([0, 3, 5, 6], [0, 2, 5, 1, 4, 3])
    assert slots(3, [0, 1, 2]) == ([0, 1, 2, 3], [0, 1, 2])
    assert slots(2, [1, 1, 0, 1]) == ([0, 1, 4], [2, 0, 1, 3])
    assert slots(1, [0, 0]) == ([0, 2], [0, 1])


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def _header_text():
    return open(os.path.join(ROOT, "include", "gpet_hip.h")).read()


def test_multi_kernel_calls_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name + " is not declared"
        assert len(m.group(1).split(",")) == n_args, name
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n_args, name
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()
    assert C.sizeof(_lib.GpetDenoise) == 64


# ---- the Python slot derivation ------------------------------------------------------------------------------------------------
def test_derive_slots_worked_examples():
    from gaussian_process_edge_trace_amd._lib import derive_slots
    # a shared frame, two kernels
    assert derive_slots([0, 0], [0, 1]) == ([0, 0], [0, 1], [0, 1])
    # two frames with both walls on each
    assert derive_slots([0, 0, 1, 1], [0, 1, 0, 1]) == ([0, 0, 1, 1], [0, 1, 0, 1], [0, 1, 2, 3])
    # one kernel only: the identity table, the edges map to their frames
    assert derive_slots([0, 0, 1, 1], [0, 0, 0, 0]) == ([0, 1], [0, 0], [0, 0, 1, 1])
    assert derive_slots([0, 1, 2], [0, 0, 0]) == ([0, 1, 2], [0, 0, 0], [0, 1, 2])
    # an edge order that interleaves the pairs: slots in order of first occurrence, repeated pairs share a slot
    assert derive_slots([1, 0, 1, 0, 1, 0], [1, 0, 0, 0, 1, 1]) == ([1, 0, 1, 0], [1, 0, 0, 1], [0, 1, 2, 1, 0, 3])
    with pytest.raises(ValueError, match="kernel_of"):
        derive_slots([0, 1, 2], [0, 1])


def test_split_kernels():
    from gaussian_process_edge_trace_amd._lib import split_kernels
    K = np.arange(15.0).reshape(5, 3)
    ks, multi = split_kernels(K)
    assert not multi and len(ks) == 1 and np.array_equal(ks[0], K)
    ks, multi = split_kernels(K.tolist())  # a nested list of numbers is ONE kernel
    assert not multi and len(ks) == 1 and ks[0].shape == (5, 3)
    for many in ([K, -K], (K, np.ones((2, 4))), np.stack([K, -K, K])):
        ks, multi = split_kernels(many)
        assert multi and len(ks) == len(many) and all(k.dtype == np.float64 and k.flags.c_contiguous for k in ks)
    assert split_kernels([K])[1] is True and len(split_kernels([K])[0]) == 1
    for bad in (np.zeros(3), [np.zeros((2, 2)), np.zeros((0, 3))]):
        with pytest.raises(ValueError, match="grad_kernel"):
            split_kernels(bad)


# ---- routing and argument errors (no device) -----------------------------------------------------------------------------------
K = np.arange(15, dtype=np.float64).reshape(5, 3)
U8 = np.zeros((6, 7), np.uint8)


def test_slot_table_routing():
    from gaussian_process_edge_trace_amd import _lib
    from gaussian_process_edge_trace_amd.gpet import resolve_image_source as src
    # a shared frame, two kernels
    r = src(2, raw_imgs=U8, grad_kernel=[K, -K], kernel_of=[1, 0])
    raw = r["batch"]["raw"]
    assert (r["kind"], r["share"], r["shape"], r["pix"]) == ("raw", False, (6, 7), _lib.PIX_U8)
    assert (len(raw), raw.n_slots, raw.slots, r["image_of"], r["edge_frames"]) == (1, 2, ([0, 0], [1, 0]), [0, 1], [0, 0])
    assert len(raw.kernels) == 2 and np.array_equal(raw.kernels[1], -K)
    nk, kp, kh, kw, fo, ko = raw.multi_args()
    assert (nk, list(kh), list(kw), list(fo), list(ko)) == (2, [5, 5], [3, 3], [0, 0], [1, 0])
    # one frame per edge with per-edge kernels
    r = src(3, raw_imgs=[U8, U8, U8], grad_kernel=[K, -K], kernel_of=[0, 1, 0])
    assert (r["batch"]["raw"].slots, r["image_of"]) == (([0, 1, 2], [0, 1, 0]), [0, 1, 2])
    # an image map keeps meaning "edge e reads frame image_of[e]"; n_edges counts the frames
    r = src(2, raw_imgs=[U8, U8], grad_kernel=[K, -K], kernel_of=[0, 1, 0, 1], image_of=[0, 0, 1, 1])
    assert (len(r["batch"]["raw"]), r["batch"]["raw"].slots, r["image_of"]) == (2, ([0, 0, 1, 1], [0, 1, 0, 1]), [0, 1, 2, 3])
    # device frames
    r = src(2, raw_device_ptrs=[4096, 8192], raw_dtype="uint16", grad_shape=(6, 7), grad_kernel=[K, -K], kernel_of=[0, 1])
    assert (r["on_device"], r["pix"], r["batch"]["raw"].slots) == (True, _lib.PIX_U16, ([0, 1], [0, 1]))


def test_single_kernel_resolution_is_what_it_was():
    from gaussian_process_edge_trace_amd import _lib
    from gaussian_process_edge_trace_amd.gpet import resolve_image_source as src
    r = src(3, raw_imgs=np.zeros((3, 6, 7), np.uint8), grad_kernel=K)
    assert sorted(r) == ["batch", "kind", "on_device", "pix", "shape", "share"]
    assert (r["kind"], r["share"], r["shape"], r["pix"], r["on_device"]) == ("raw", False, (6, 7), _lib.PIX_U8, False)
    assert r["batch"]["raw"].slots is None and r["batch"]["raw"].n_slots == 3 and np.array_equal(r["batch"]["raw"].kernel, K)
    r = src(3, raw_imgs=U8, grad_kernel=K.tolist())  # (a nested list is one kernel)
    assert (r["share"], len(r["batch"]["raw"])) == (True, 1) and r["batch"]["raw"].slots is None
    r = src(2, grad_imgs=np.ones((6, 7)))
    assert sorted(r) == ["batch", "kind", "on_device", "shape", "share"] and r["share"] is True


def test_argument_errors_name_their_keyword():
    import gaussian_process_edge_trace_amd as pkg
    from gaussian_process_edge_trace_amd.gpet import resolve_image_source as src
    with pytest.raises(ValueError, match="kernel_of"):  # a list of kernels without kernel_of
        src(2, raw_imgs=U8, grad_kernel=[K, -K])
    with pytest.raises(ValueError, match="kernel_of"):  # kernel_of with gradient images
        src(2, grad_imgs=np.ones((6, 7), np.float32), kernel_of=[0, 1])
    with pytest.raises(ValueError, match="kernel_of"):  # an index outside the kernels
        src(2, raw_imgs=U8, grad_kernel=[K, -K], kernel_of=[0, 2])
    with pytest.raises(ValueError, match="kernel_of"):  # a kernel no edge uses
        src(2, raw_imgs=U8, grad_kernel=[K, -K], kernel_of=[0, 0])
    with pytest.raises(ValueError, match="kernel_of"):  # one frame per edge, but another count of indices
        src(3, raw_imgs=[U8, U8, U8], grad_kernel=[K, -K], kernel_of=[0, 1])
    with pytest.raises(ValueError, match="kernel_of"):
        src(2, raw_imgs=[U8, U8], grad_kernel=[K, -K], kernel_of=[0, 1, 0], image_of=[0, 0, 1, 1])
    with pytest.raises(ValueError, match="grad_kernel"):
        src(2, raw_imgs=U8, grad_kernel=[K, np.zeros((0, 3))], kernel_of=[0, 1])
    init = np.array([[0, 3], [6, 3]])
    with pytest.raises(ValueError, match="kernel_of"):  # (before a device is needed)
        pkg.GP_Edge_Tracing_Batch([init, init], None, [1, 2], raw_imgs=U8, grad_kernel=[K, -K])
    with pytest.raises(ValueError, match="kernel_of"):
        pkg.GP_Edge_Tracing_Batch([init, init], None, [1, 2], raw_imgs=U8, grad_kernel=[K, -K], kernel_of=[0, 1, 0])
    with pytest.raises(ValueError, match="kernel_of"):
        pkg.GP_Edge_Tracing_Batch([init, init], np.ones((6, 7), np.float32), [1, 2], kernel_of=[0, 1])
    frames = [U8, U8]
    with pytest.raises(ValueError, match="kernel_of"):  # 3 kernels for 2 inits
        pkg.SequenceTracer(frames, [init, init], grad_kernel=[K, -K, K])
    with pytest.raises(ValueError, match="kernel_of"):
        pkg.SequenceTracer(frames, [init, init], grad_kernel=[K, -K], kernel_of=[0, 1, 1])
    with pytest.raises(ValueError, match="kernel_of"):
        pkg.SequenceTracer(frames, [init, init], grad_kernel=[K, -K], kernel_of=[0, 2])
    with pytest.raises(ValueError, match="grad_kernel"):
        pkg.SequenceTracer(frames, [init, init], kernel_of=[0, 1])
    t = pkg.SequenceTracer(frames, [init, init], grad_kernel=[K, -K, 2 * K], kernel_of=[2, 0])  # (unused kernels are dropped)
    assert t.kernel_of == [1, 0] and len(t.grad_kernel) == 2 and np.array_equal(t.grad_kernel[1], 2 * K)
    assert pkg.SequenceTracer(frames, [init, init], grad_kernel=[K, -K]).kernel_of == [0, 1]
    assert pkg.SequenceTracer(frames, [init, init], grad_kernel=K).kernel_of is None
    assert "kernel_of" in inspect.signature(pkg.GP_Edge_Tracing_Batch.__init__).parameters


# ---- machine code of the multi-kernel convolution ------------------------------------------------------------------------------
def _code_objects(tmp_path):
    """The gfx950 code objects of the shipped library, unbundled (as tests/test_raw_frames_host.py does)."""
    import __graft_entry__ as ge
    ge.build()
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump")
    so = tmp_path / "lib.so"
    shutil.copy(ge.LIB, so)
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    return objdump, [str(tmp_path / f) for f in sorted(os.listdir(tmp_path)) if "amdgcn" in f]


def test_multi_kernel_conv_rounds_every_product_and_keeps_its_registers(tmp_path):
    """Bit-exactness with the single-kernel path needs the product rounded before it is added (no v_fma_f64 / v_fmac_f64 in any
    of the four instantiations); the code object's metadata shows no private segment and no spilled registers."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("no llvm-readelf")
    objdump, objs = _code_objects(tmp_path)
    bodies, use = {}, {}
    for f in objs:
        text = subprocess.run([objdump, "-d", f], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\S*k_conv_relu_multi\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, flags=re.S | re.M):
            bodies[m.group(1)] = m.group(2)
        notes = subprocess.run([readelf, "--notes", f], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:  # one block per kernel; .agpr_count is its first key
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "k_conv_relu_multi" in name.group(1):
                use[name.group(1)] = {k: int(v) for k, v in re.findall(
                    r"\.(private_segment_fixed_size|sgpr_spill_count|vgpr_spill_count|vgpr_count):\s+(\d+)", block)}
    for tag in ("Ih", "It", "If", "Id"):  # uint8_t, uint16_t, float, double
        assert any("k_conv_relu_multi" + tag in n for n in bodies), tag
    assert len(bodies) == 4 and len(use) == 4, (sorted(bodies), sorted(use))
    for name, body in bodies.items():
        assert "v_mul_f64" in body and "v_add_f64" in body, name
        assert not re.search(r"v_fmac?_f64", body), name
    for name, u in use.items():
        assert u["private_segment_fixed_size"] == 0 and u["sgpr_spill_count"] == 0 and u["vgpr_spill_count"] == 0, (name, u)
        assert 0 < u["vgpr_count"] <= 64, (name, u)
