"""CPU tests of what csrc/gpet_denoise_plan.h decides before the denoising kernels are launched (the header needs no HIP: a small
extern "C" shim around it is compiled with the host C++ compiler, as tests/test_raw_frames_host.py does for gpet_conv_plan.h), and of
the ABI surface of the denoising calls.

Every expected figure is a literal worked out by hand from the rules the issue states: a window of extent k starts k // 2 before
the pixel; median is element n // 2 of the sorted window, minimum element 0; the Gaussian radius is int(truncate * sigma + 0.5);
tiles of 64 x 16 pixels with the patch in LDS in the frame's own type; windows of at most 81 pixels; per image the workspace holds
the denoised frame (plus the frame between the Gaussian passes; plus four f64 p planes and 32 bytes of state and two partial sums
per workgroup for 'tvc'), every part rounded up to 256 bytes; a chunk holds as many images as fit 64 MiB with their workspace and,
for host frames, their staged bytes (rounded up to 256).  None was produced by the header under test."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
NEW = dict(gpet_denoise_images=10, gpet_grad_images_dn=12, gpet_batch_create_raw_dn=15, gpet_batch_set_raw_images_dn=8)
NONE, MEDIAN, MINIMUM, GAUSSIAN, TVC = range(5)
U8, U16, F32, F64 = range(4)


def _header_text():
    return open(os.path.join(ROOT, "include", "gpet_hip.h")).read()


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_denoise_calls_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    declared = set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW.items():
        assert name in declared, name
        assert hasattr(lib, name), name
        assert len(_lib.SYMBOLS[name][1]) == n_args, name
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()


def test_struct_and_codes_agree_between_header_and_python():
    from gaussian_process_edge_trace_amd import _lib
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPET_DN_[A-Z_]+)\s+(\d+)\b", _header_text())}
    assert defs == dict(GPET_DN_NONE=0, GPET_DN_MEDIAN=1, GPET_DN_MINIMUM=2, GPET_DN_GAUSSIAN=3, GPET_DN_TVC=4,
                        GPET_DN_MODE_REFLECT=0, GPET_DN_MODE_NEAREST=1)
    assert _lib.DN_OF_TECHNIQUE == dict(median=1, minimum=2, gaussian=3, tvc=4) and _lib.DN_MODE_OF_NAME == dict(reflect=0, nearest=1)
    body = re.search(r"typedef struct gpet_denoise \{(.*?)\} gpet_denoise;", re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    assert fields == [(n, "int32_t" if t is C.c_int32 else "double") for n, t in _lib.GpetDenoise._fields_]
    # int32 x 4 | double x 5 | int32 (+ 4 bytes of tail padding)
    assert C.sizeof(_lib.GpetDenoise) == 64 and _lib.GpetDenoise.sigma_y.offset == 16 and _lib.GpetDenoise.n_iter_max.offset == 56


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_denoise_plan.h"
using namespace gpet;
extern "C" {
int shim_extend(int i, int n, int mode) { return dn_extend(i, n, mode); }
int shim_origin(int k) { return dn_origin(k); }
int shim_rank(int technique, int sy, int sx) { return dn_rank(technique, sy, sx); }
int shim_radius(double sigma, double truncate) { return dn_gauss_radius(sigma, truncate); }
void shim_taps(double sigma, int r, double* w) { dn_gauss_taps(sigma, r, w); }
long long shim_rank_lds(int sy, int sx, int pix) { return (long long)dn_rank_lds_bytes(sy, sx, pix); }
int shim_out_pix(int technique, int pix) { return dn_out_pix(technique, pix); }
// 0: the spec can run
int shim_check(int technique, int sy, int sx, int mode, double sig_y, double sig_x, double truncate, double weight, double eps, int n_iter_max, int pix) {
  DenoiseSpec s;
  s.technique = technique; s.size_y = sy; s.size_x = sx; s.mode = mode; s.sigma_y = sig_y; s.sigma_x = sig_x; s.truncate = truncate;
  s.weight = weight; s.eps = eps; s.n_iter_max = n_iter_max;
  return dn_check(s, pix) ? 1 : 0;
}
// out: off_out, off_tmp, off_p, off_part, plane_bytes, n_wg, img_bytes, per_chunk, n_chunks, slots, slot_bytes
void shim_plan(int technique, int pix, int M, int N, int n_img, int on_dev, long long* out) {
  const DenoiseLayout L = dn_layout(technique, pix, M, N);
  const StagePlan p = dn_stage_plan(n_img, (size_t)M * N * pix_bytes(pix), on_dev != 0, L);
  out[0] = L.off_out; out[1] = L.off_tmp; out[2] = L.off_p; out[3] = L.off_part; out[4] = L.plane_bytes; out[5] = L.n_wg; out[6] = L.img_bytes;
  out[7] = p.per_chunk; out[8] = p.n_chunks; out[9] = p.slots; out[10] = (long long)p.slot_bytes;
}
int shim_consts(int which) { return which == 0 ? DN_WINDOW_MAX : which == 1 ? DN_TVC_GROUP : which == 2 ? (int)DN_TVC_LDS_BYTES : (int)DN_TVC_STATE_BYTES; }
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
    d = tmp_path_factory.mktemp("denoise_plan")
    src, so = d / "shim.cpp", d / "libdenoise_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_rank_lds.restype = C.c_longlong
    lib.shim_radius.argtypes = [C.c_double, C.c_double]
    lib.shim_taps.argtypes = [C.c_double, C.c_int, C.c_void_p]
    lib.shim_check.argtypes = [C.c_int] * 4 + [C.c_double] * 5 + [C.c_int] * 2
    return lib


def test_boundary_modes(shim):
    # d c b a | a b c d | d c b a, continued periodically; n = 4
    assert [shim.shim_extend(i, 4, 0) for i in range(-9, 13)] == [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3]
    assert [shim.shim_extend(i, 4, 1) for i in range(-3, 8)] == [0, 0, 0, 0, 1, 2, 3, 3, 3, 3, 3]
    assert [shim.shim_extend(i, 1, 0) for i in range(-3, 4)] == [0] * 7
    for n in (1, 2, 5, 16):  # and the restatement the fixture tests use agrees
        for mode, name in enumerate(R.MODES):
            assert [shim.shim_extend(i, n, mode) for i in range(-40, 41)] == R.extend_index(np.arange(-40, 41), n, name).tolist()


def test_window_origin_and_rank(shim):
    assert [shim.shim_origin(k) for k in (1, 2, 3, 4, 5, 7, 8, 9)] == [0, 1, 1, 2, 2, 3, 4, 4]
    assert [shim.shim_rank(MEDIAN, sy, sx) for sy, sx in ((3, 3), (5, 5), (4, 3), (7, 1), (9, 9), (1, 1), (2, 2))] == [4, 12, 6, 3, 40, 0, 2]
    assert [shim.shim_rank(MINIMUM, sy, sx) for sy, sx in ((3, 3), (9, 9), (4, 3))] == [0, 0, 0]


def test_origin_rule_is_scipys():
    """The restatement (which uses the same origin rule) against scipy itself on a ramp, even and odd windows."""
    ndimage = pytest.importorskip("scipy.ndimage")
    a = np.random.default_rng(3).integers(0, 1000, (13, 17)).astype(np.float64)
    for size in ((3, 3), (4, 3), (2, 5), (7, 1), (6, 6)):
        for mode in R.MODES:
            assert np.array_equal(ndimage.median_filter(a, size=size, mode=mode), R.median(a, size, mode)), (size, mode)
            assert np.array_equal(ndimage.minimum_filter(a, size=size, mode=mode), R.minimum(a, size, mode)), (size, mode)


def test_gaussian_radius_and_taps(shim):
    cases = [(0.8, 4.0, 3), (1.5, 4.0, 6), (3.0, 4.0, 12), (3.0, 3.0, 9), (0.7, 4.0, 3), (2.0, 4.0, 8), (0.1, 4.0, 0), (2.5, 2.5, 6), (0.125, 4.0, 1)]
    assert [shim.shim_radius(s, t) for s, t, _ in cases] == [r for _, _, r in cases]
    for s, t, r in cases:
        w = np.empty(2 * r + 1)
        shim.shim_taps(s, r, w.ctypes.data)
        assert np.array_equal(w, R.gaussian_taps(s, t)), (s, t)  # the restatement's taps, bit for bit
        assert np.array_equal(w, w[::-1]) and abs(w.sum() - 1.0) < 1e-15
        assert abs(w[r] * sum(math.exp(-0.5 * x * x / (s * s)) for x in range(-r, r + 1)) - 1.0) < 1e-14


def test_lds_bytes_and_refusals(shim):
    assert shim.shim_rank_lds(3, 3, U8) == 18 * 66 * 1 == 1188
    assert shim.shim_rank_lds(5, 5, F32) == 20 * 68 * 4 == 5440
    assert shim.shim_rank_lds(7, 1, U16) == 22 * 64 * 2 == 2816
    assert shim.shim_rank_lds(9, 9, F64) == 24 * 72 * 8 == 13824
    assert shim.shim_rank_lds(81, 1, F64) == 96 * 64 * 8 == 49152  # the largest patch of an allowed window: inside the 64 KB bound
    assert [shim.shim_consts(i) for i in range(4)] == [81, 8, 2 * 17 * 65 * 8, 32]

    def check(technique, sy=3, sx=3, mode=0, sig=(1.0, 1.0), truncate=4.0, weight=0.1, eps=2e-4, n_iter_max=200, pix=F64):
        return shim.shim_check(technique, sy, sx, mode, sig[0], sig[1], truncate, weight, eps, n_iter_max, pix)

    for t in (MEDIAN, MINIMUM, GAUSSIAN, TVC):
        for pix in (U8, U16, F32, F64):
            assert check(t, pix=pix) == 0
    assert check(NONE) == 0 and check(NONE, sy=0, sx=0, sig=(0.0, 0.0), weight=0.0, n_iter_max=0) == 0
    assert check(5) == 1 and check(-1) == 1                                    # unknown technique
    assert check(MEDIAN, pix=4) == 1 and check(TVC, pix=-1) == 1               # unknown pixel type
    for t in (MEDIAN, MINIMUM):
        assert [check(t, sy, sx) for sy, sx in ((9, 9), (81, 1), (1, 81), (4, 3), (1, 1))] == [0] * 5
        assert [check(t, sy, sx) for sy, sx in ((10, 9), (9, 10), (82, 1), (0, 3), (3, 0), (-1, 3), (100000, 100000))] == [1] * 7
        assert check(t, mode=2) == 1 and check(t, mode=-1) == 1 and check(t, mode=1) == 0
    assert check(GAUSSIAN, sig=(0.0, 1.0)) == 1 and check(GAUSSIAN, sig=(1.0, 0.0)) == 1 and check(GAUSSIAN, sig=(-1.0, 1.0)) == 1
    assert check(GAUSSIAN, sig=(float("nan"), 1.0)) == 1 and check(GAUSSIAN, truncate=0.0) == 1 and check(GAUSSIAN, mode=2) == 1
    assert check(GAUSSIAN, sig=(64.0, 1.0)) == 1 and check(GAUSSIAN, sig=(60.0, 1.0)) == 0  # radius 256 / 240
    assert check(TVC, weight=0.0) == 1 and check(TVC, weight=-0.1) == 1 and check(TVC, n_iter_max=0) == 1 and check(TVC, eps=-1.0) == 1
    assert check(TVC, mode=7) == 0  # ('tvc' has no boundary mode)


def test_intermediate_pixel_type(shim):
    for pix in (U8, U16, F32, F64):
        assert [shim.shim_out_pix(t, pix) for t in (MEDIAN, MINIMUM, GAUSSIAN, TVC)] == [pix, pix, pix, F64]


def _plan(shim, technique, pix, M=500, N=500, n_img=256, on_dev=False):
    out = (C.c_longlong * 11)()
    shim.shim_plan(technique, pix, M, N, n_img, 1 if on_dev else 0, out)
    keys = ["off_out", "off_tmp", "off_p", "off_part", "plane_bytes", "n_wg", "img_bytes", "per_chunk", "n_chunks", "slots", "slot_bytes"]
    return dict(zip(keys, list(out)))


# 500 x 500: a frame of u8 / u16 / f32 / f64 is 250 000 / 500 000 / 1 000 000 / 2 000 000 bytes, 250 112 / 500 224 / 1 000 192 /
# 2 000 128 rounded up to 256; 8 x 32 = 256 workgroups -> partials 32 + 2 * 256 * 8 = 4 128 -> 4 352
FRAME = {U8: 250112, U16: 500224, F32: 1000192, F64: 2000128}
TVC_WS = 5 * 2000128 + 4352


def test_workspace_layout_500(shim):
    for pix in (U8, U16, F32, F64):
        for t in (MEDIAN, MINIMUM):
            p = _plan(shim, t, pix)
            assert (p["off_out"], p["img_bytes"]) == (0, FRAME[pix])
        p = _plan(shim, GAUSSIAN, pix)
        assert (p["off_out"], p["off_tmp"], p["img_bytes"]) == (0, FRAME[pix], 2 * FRAME[pix])
        p = _plan(shim, TVC, pix)
        assert (p["off_out"], p["off_p"], p["plane_bytes"], p["off_part"], p["n_wg"], p["img_bytes"]) == \
            (0, 2000128, 2000128, 5 * 2000128, 256, TVC_WS == 10004992 and TVC_WS)
        assert _plan(shim, NONE, pix)["img_bytes"] == 0
    p = _plan(shim, TVC, F64, M=17, N=65)  # 2 x 2 workgroups, frame 8 840 -> 8 960, partials 32 + 32 -> 256
    assert (p["n_wg"], p["plane_bytes"], p["off_part"], p["img_bytes"]) == (4, 8960, 5 * 8960, 5 * 8960 + 256)


# 256 frames of 500 x 500, 64 MiB = 67 108 864 bytes: images per chunk = budget // (staged frame + workspace), chunks = ceil(256 / that)
CHUNKS_HOST = {(MEDIAN, U8): (134, 2), (MEDIAN, U16): (67, 4), (MEDIAN, F32): (33, 8), (MEDIAN, F64): (16, 16),
               (MINIMUM, U8): (134, 2), (MINIMUM, F64): (16, 16),
               (GAUSSIAN, U8): (89, 3), (GAUSSIAN, U16): (44, 6), (GAUSSIAN, F32): (22, 12), (GAUSSIAN, F64): (11, 24),
               (TVC, U8): (6, 43), (TVC, U16): (6, 43), (TVC, F32): (6, 43), (TVC, F64): (5, 52)}
CHUNKS_DEV = {(MEDIAN, U8): (256, 1), (MEDIAN, U16): (134, 2), (MEDIAN, F32): (67, 4), (MEDIAN, F64): (33, 8),
              (GAUSSIAN, U8): (134, 2), (GAUSSIAN, U16): (67, 4), (GAUSSIAN, F32): (33, 8), (GAUSSIAN, F64): (16, 16),
              (TVC, U8): (6, 43), (TVC, U16): (6, 43), (TVC, F32): (6, 43), (TVC, F64): (6, 43)}


@pytest.mark.parametrize("key", sorted(CHUNKS_HOST))
def test_chunks_of_256_host_frames(shim, key):
    p = _plan(shim, key[0], key[1])
    assert (p["per_chunk"], p["n_chunks"], p["slots"]) == CHUNKS_HOST[key] + (1,)
    assert p["slot_bytes"] == p["per_chunk"] * (FRAME[key[1]] + p["img_bytes"]) <= 64 << 20
    assert (p["per_chunk"] + 1) * (FRAME[key[1]] + p["img_bytes"]) > 64 << 20


@pytest.mark.parametrize("key", sorted(CHUNKS_DEV))
def test_chunks_of_256_device_frames(shim, key):
    p = _plan(shim, key[0], key[1], on_dev=True)  # (device frames are read where they lie: only the workspace counts)
    assert (p["per_chunk"], p["n_chunks"]) == CHUNKS_DEV[key]
    assert p["slot_bytes"] == p["per_chunk"] * p["img_bytes"] <= 64 << 20


def test_without_a_technique_the_chunks_are_the_parents(shim):
    for pix, per, n in ((U8, 256, 1), (F32, 67, 4), (F64, 33, 8)):  # 64 MiB // 250 000 = 268, // 1 000 000 = 67, // 2 000 000 = 33
        p = _plan(shim, NONE, pix)
        assert (p["per_chunk"], p["n_chunks"]) == (per, n)
    p = _plan(shim, MEDIAN, U8, n_img=1)
    assert (p["per_chunk"], p["n_chunks"], p["slot_bytes"]) == (1, 1, 2 * 250112)


# ---- machine code of the denoising kernels ----------------------------------------------------------------------------------------
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


def test_gaussian_pass_has_no_fused_multiply_add_and_every_kernel_is_instantiated(tmp_path):
    """scipy's (x[l] + x[-l]) * w, then += : the product must be rounded before it is added -- no v_fma_f64 / v_fmac_f64 in any
    instantiation of k_dn_gauss_pass.  ('tvc' divides and takes a square root, whose correctly rounded expansions use FMAs.)"""
    objdump, objs = _code_objects(tmp_path)
    bodies = {}
    for f in objs:
        text = subprocess.run([objdump, "-d", f], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\S*k_dn_\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, flags=re.S | re.M):
            bodies[m.group(1)] = m.group(2)
    for tag in ("Ih", "It", "If", "Id"):  # Itanium mangling of uint8_t, uint16_t, float, double
        assert any("k_dn_gauss_pass" + tag in n for n in bodies), tag
        assert any("k_dn_tvc_iter" + tag in n for n in bodies), tag
        for window in ("Li3ELi3E", "Li5ELi5E", "Li0ELi0E"):
            assert any("k_dn_rank" + tag + window in n for n in bodies), (tag, window)
    assert any("k_dn_tvc_check" in n for n in bodies) and len(bodies) == 4 + 4 + 12 + 1
    for name, body in bodies.items():
        assert "scratch_" not in body, name
        if "k_dn_gauss_pass" in name:
            assert "v_mul_f64" in body and "v_add_f64" in body and not re.search(r"v_fmac?_f64", body), name
        if "k_dn_tvc" in name:
            assert "atomic_add_f64" not in body and "atomic_add_f32" not in body, name  # (sums in a fixed order: no float atomics)
