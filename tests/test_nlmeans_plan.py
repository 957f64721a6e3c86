"""CPU tests of what csrc/gpet_nlmeans_plan.h decides before the non-local means kernel is launched (the header needs no HIP: a
small extern "C" shim around it is compiled with the host C++ compiler, as tests/test_denoise_plan.py does), and of the ABI
surface of gpet_nlmeans_images.

Every expected figure is a literal worked out by hand from the rules the header states: an even patch size means the next odd
one; a workgroup owns 16 x 16 pixels and keeps 16 + 2 d + 2 (s // 2) pixels each way in LDS as f64, rows at the smallest pitch
at or above that extent that is 16 mod 32 doubles; at most 64 KB of it; patches of 3 to 15, distances of 0 to 31.  None was
produced by the header under test."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import nlmeans_ref as R
from tests.test_denoise_plan import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
FIX = np.load(os.path.join(ROOT, "tests", "golden", "nlmeans.npz"))
U8, U16, F32, F64 = range(4)


def _header_text():
    return open(os.path.join(ROOT, "include", "gpet_hip.h")).read()


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    assert "gpet_nlmeans_images" in set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    assert hasattr(C.CDLL(_lib.LIB_PATH), "gpet_nlmeans_images")
    assert len(_lib.SYMBOLS["gpet_nlmeans_images"][1]) == 9
    assert hasattr(_lib.Context, "nlmeans_images")
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()


def test_struct_and_flag_agree_between_header_and_python():
    from gaussian_process_edge_trace_amd import _lib
    defs = dict(re.findall(r"#define\s+(GPET_NLM_[A-Z_]+)\s+(\d+)u?\b", _header_text()))
    assert defs == dict(GPET_NLM_OUT_ON_DEVICE="8") and _lib.NLM_OUT_ON_DEVICE == 8
    assert _lib.NLM_OUT_ON_DEVICE not in (_lib.GRAD_ON_DEVICE, _lib.IMAGES_NEXT_FRAME, _lib.RAW_ON_DEVICE)
    body = re.search(r"typedef struct gpet_nlmeans \{(.*?)\} gpet_nlmeans;", re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, name = decl.rsplit(None, 1)
            fields.append((name, ctype))
    names = {C.c_int32: "int32_t", C.c_double: "double", C.c_void_p: "const double*"}
    assert fields == [(n, names[t]) for n, t in _lib.GpetNlmeans._fields_]
    # int32 x 2 | double x 2 | pointer
    assert C.sizeof(_lib.GpetNlmeans) == 32 and _lib.GpetNlmeans.h.offset == 8 and _lib.GpetNlmeans.taps.offset == 24
    # the technique tables of gpet_denoise stay as they were
    assert _lib.DN_OF_TECHNIQUE == dict(median=1, minimum=2, gaussian=3, tvc=4)


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_nlmeans_plan.h"
using namespace gpet;
extern "C" {
double shim_fexp(double y) { return nlm_fexp(y); }
int shim_patch(int ps) { return nlm_patch(ps); }
int shim_extent(int s, int d) { return nlm_extent(s, d); }
int shim_stride(int e) { return nlm_lds_stride(e); }
long long shim_lds(int s, int d) { return (long long)nlm_lds_bytes(s, d); }
void shim_grid(int M, int N, int* g) { const NlmGrid q = nlm_grid(M, N); g[0] = q.gx; g[1] = q.gy; }
int shim_mirror(int q, int n) { return nlm_mirror(q, n); }
void shim_taps(int s, double h, double* out) { nlm_taps_c(s, h, out); }
const char* shim_check(int ps, int d, double h, double sigma, const double* taps, int pix, int M, int N) {
  NlmSpec sp;
  sp.patch_size = ps; sp.patch_distance = d; sp.h = h; sp.sigma = sigma; sp.taps = taps;
  return nlm_check(sp, pix, M, N);
}
int shim_consts(int which) { return which == 0 ? NLM_TILE : which == 1 ? NLM_PATCH_MAX : which == 2 ? NLM_DIST_MAX : (int)NLM_LDS_MAX; }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("nlmeans_plan")
    src, so = d / "shim.cpp", d / "libnlmeans_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_fexp.restype = C.c_double
    lib.shim_fexp.argtypes = [C.c_double]
    lib.shim_lds.restype = C.c_longlong
    lib.shim_taps.argtypes = [C.c_int, C.c_double, C.c_void_p]
    lib.shim_check.restype = C.c_char_p
    lib.shim_check.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_int]
    return lib


def test_fexp_on_the_fixtures_grid_bit_for_bit(shim):
    args, vals = FIX["fexp_args"], FIX["fexp_vals"]
    got = np.array([shim.shim_fexp(float(a)) for a in args])
    assert np.array_equal(got.view(np.uint64), vals.view(np.uint64))
    assert shim.shim_fexp(0.0) == 0.9710078239440918


def test_the_weight_is_zero_below_minus_708(shim):
    below = float(np.nextafter(-708.0, -np.inf))
    for y in (below, -709.0, -800.0, -1e6, -1e300, -math.inf):
        got = shim.shim_fexp(y)
        assert got == 0.0 and math.copysign(1.0, got) == 1.0, y
    # at -708 itself the high word is (int)(C * -708) + 1072632447 = -1071044979 + 1072632447 = 1587468 > 0: a small positive double
    assert shim.shim_fexp(-708.0) == R.fexp(-708.0) == float(np.array([1587468 << 32], dtype=np.int64).view(np.float64)[0]) > 0.0
    assert [shim.shim_fexp(y) for y in (-5.0, -100.0, -700.0)] == [R.fexp(y) for y in (-5.0, -100.0, -700.0)]


def test_patch_extent_pitch_lds_bytes_and_grid(shim):
    assert [shim.shim_patch(p) for p in (2, 3, 4, 5, 6, 7, 8, 9, 14, 15)] == [3, 3, 5, 5, 7, 7, 9, 9, 15, 15]
    assert [shim.shim_consts(i) for i in range(4)] == [16, 15, 31, 65536]
    # extent = 16 + 2 d + 2 (s // 2)
    assert [shim.shim_extent(s, d) for s, d in ((7, 11), (9, 15), (3, 2), (5, 3), (3, 31), (15, 25))] == [44, 54, 22, 26, 80, 80]
    # the pitch: 16, 48, 80, 112 doubles
    assert [shim.shim_stride(e) for e in (16, 17, 22, 28, 44, 48, 49, 54, 80, 81, 82)] == [16, 48, 48, 48, 48, 48, 80, 80, 80, 112, 112]
    assert shim.shim_lds(7, 11) == 44 * 48 * 8 == 16896   # the defaults
    assert shim.shim_lds(9, 15) == 54 * 80 * 8 == 34560
    assert shim.shim_lds(3, 2) == 22 * 48 * 8 == 8448
    assert shim.shim_lds(3, 31) == 80 * 80 * 8 == 51200   # the largest distance
    assert shim.shim_lds(15, 25) == 80 * 80 * 8 == 51200
    assert shim.shim_lds(5, 31) == 82 * 112 * 8 == 73472  # beyond the 64 KB bound
    g = (C.c_int * 2)()
    for (M, N), exp in (((500, 500), (32, 32)), ((9, 11), (1, 1)), ((20, 70), (5, 2)), ((33, 65), (5, 3)), ((16, 16), (1, 1)), ((17, 16), (1, 2))):
        shim.shim_grid(M, N, g)
        assert (g[0], g[1]) == exp, (M, N)
    # c b | a b c | b a
    assert [shim.shim_mirror(q, 3) for q in range(-2, 5)] == [2, 1, 0, 1, 2, 1, 0]
    assert [shim.shim_mirror(q, 5) for q in range(-3, 8)] == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]


def test_refusals_and_their_reasons(shim):
    taps = np.full(225, 0.01)

    def check(ps=7, d=11, h=0.1, sigma=0.0, t=taps, pix=F64, M=40, N=60):
        r = shim.shim_check(ps, d, h, sigma, t.ctypes.data if t is not None else None, pix, M, N)
        return None if r is None else r.decode()

    assert check() is None                                    # the defaults
    assert check(ps=9, d=15) is None
    for pix in (U8, U16, F32, F64):
        assert check(pix=pix) is None
    assert check(ps=2) is None and check(ps=15, d=25) is None and check(ps=3, d=31) is None and check(d=0) is None
    assert "pixel type" in check(pix=4) and "pixel type" in check(pix=-1)
    assert "patch_size" in check(ps=1) and "patch_size" in check(ps=0) and "patch_size" in check(ps=-3)
    assert "15 x 15" in check(ps=16) and "15 x 15" in check(ps=17)
    # off = s // 2 must be below min(M, N): s = 7 -> off 3
    assert "smaller extent" in check(M=3) and "smaller extent" in check(N=3) and check(M=4, N=4) is None
    assert "smaller extent" in check(ps=3, M=1) and check(ps=3, M=2, N=2) is None
    assert "negative" in check(d=-1) and "above 31" in check(d=32)
    assert "h must" in check(h=0.0) and "h must" in check(h=-1.0) and "h must" in check(h=math.nan) and "h must" in check(h=math.inf)
    assert "sigma" in check(sigma=-0.1) and "sigma" in check(sigma=math.nan) and check(sigma=0.3) is None
    assert "LDS" in check(ps=5, d=31) and "LDS" in check(ps=15, d=26) and "LDS" in check(ps=9, d=30)
    assert "null" in check(t=None)
    for bad in (math.nan, math.inf, -math.inf):
        t = taps.copy()
        t[48] = bad
        assert "finite" in check(t=t)
        assert check(ps=3, t=t) is None  # (a 3 x 3 patch reads nine taps)


def test_taps_through_the_c_librarys_exp(shim):
    for s, h in ((3, 0.1), (5, 0.1), (7, 0.1), (9, 0.25), (15, 25.0)):
        w = np.empty((s, s))
        shim.shim_taps(s, h, w.ctypes.data)
        assert np.array_equal(w, R.taps(s, h, exp=math.exp)), (s, h)  # the restatement with the same exponential, bit for bit
        assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1, ::-1]) and abs(w.sum() * h * h - 1.0) < 1e-14
