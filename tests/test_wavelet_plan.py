"""CPU tests of what csrc/gpet_wavelet_plan.h decides before the wavelet kernels are launched (the header needs no HIP: a small
extern "C" shim around it is compiled with the host C++ compiler, as tests/test_nlmeans_plan.py does), and of the ABI surface of
gpet_wavelet_images.

Every expected figure is a literal worked out by hand from the rules the header states: max_level is the largest L with
(F - 1) 2^L <= n; a level of input extent n gives (n + F - 1) // 2 coefficients per axis; a frame's pyramid is its levels' four
bands one after the other; a forward workgroup owns 16 x 16 coefficients and keeps 2 * 16 + F - 2 pixels each way, the axis-0
pass and 32 filter taps in LDS as f64; an inverse workgroup owns 32 x 32 pixels and keeps 16 + F / 2 - 1 coefficients each way of
four bands, the axis-1 pass and 32 taps.  None was produced by the header under test; the summation order is checked against
its restatement in tests/wavelet_ref.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import wavelet_ref as R
from tests.test_denoise_plan import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
U8, U16, F32, F64 = range(4)


def _header_text():
    return open(os.path.join(ROOT, "include", "gpet_hip.h")).read()


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    assert "gpet_wavelet_images" in set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    assert hasattr(C.CDLL(_lib.LIB_PATH), "gpet_wavelet_images")
    assert len(_lib.SYMBOLS["gpet_wavelet_images"][1]) == 9
    assert hasattr(_lib.Context, "wavelet_images")
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()


def test_struct_and_flags_agree_between_header_and_python():
    from gaussian_process_edge_trace_amd import _lib
    defs = dict(re.findall(r"#define\s+(GPET_WV_[A-Z_]+)\s+(\d+)u?\b", _header_text()))
    assert defs == dict(GPET_WV_TAPS_MAX="16", GPET_WV_SOFT="0", GPET_WV_HARD="1", GPET_WV_BAYES="0", GPET_WV_VISU="1", GPET_WV_OUT_ON_DEVICE="8")
    assert _lib.WV_OUT_ON_DEVICE == 8 and _lib.WV_MODES == dict(soft=0, hard=1) and _lib.WV_METHODS == dict(BayesShrink=0, VisuShrink=1)
    assert _lib.WV_OUT_ON_DEVICE not in (_lib.GRAD_ON_DEVICE, _lib.IMAGES_NEXT_FRAME, _lib.RAW_ON_DEVICE, _lib.FRAMES_TRANSPOSED)
    body = re.search(r"typedef struct gpet_wavelet \{(.*?)\} gpet_wavelet;", re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S), re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, name = decl.rsplit(None, 1)
            fields.append((name, ctype))
    names = {C.c_int32: "int32_t", C.c_double: "double", C.c_double * 16: "double"}
    want = []
    for n, t in _lib.GpetWavelet._fields_:
        if t is C.c_void_p:
            want.append((n, "const double*" if n == "thresholds" else "double*"))
        elif t is C.c_int32 or t is C.c_double:
            want.append((n, names[t]))
        else:
            want.append((n + "[16]", "double"))
    assert fields == want
    # int32 x 4 | double x 16 | double | int32 x 2 | double x 2 | pointer x 5
    W = _lib.GpetWavelet
    assert C.sizeof(W) == 216 and W.dec_lo.offset == 16 and W.sigma.offset == 144 and W.ppf.offset == 160 and W.thresholds.offset == 176
    # the technique tables of gpet_denoise stay as they were
    assert _lib.DN_OF_TECHNIQUE == dict(median=1, minimum=2, gaussian=3, tvc=4)


def test_struct_layout_is_what_a_c_compiler_makes_of_the_header(tmp_path):
    from gaussian_process_edge_trace_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpet_hip.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(gpet_wavelet), offsetof(gpet_wavelet, dec_lo), '
                    'offsetof(gpet_wavelet, sigma), offsetof(gpet_wavelet, n_thresholds), offsetof(gpet_wavelet, c), '
                    'offsetof(gpet_wavelet, coeffs_out));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    W = _lib.GpetWavelet
    assert got == [C.sizeof(W), W.dec_lo.offset, W.sigma.offset, W.n_thresholds.offset, W.c.offset, W.coeffs_out.offset] == [216, 16, 144, 156, 168, 208]


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_wavelet_plan.h"
using namespace gpet;
extern "C" {
int shim_max_level(int n, int F) { return wv_max_level(n, F); }
int shim_default_levels(int top) { return wv_default_levels(top); }
int shim_out_len(int n, int F) { return wv_out_len(n, F); }
int shim_sym(int k, int n) { return wv_sym(k, n); }
int shim_tap(int t, int i, int n) { return wv_fwd_tap(t, i, n); }
void shim_filters(const double* lo, int F, double* out) {
  const WvFilters f = wv_filters(lo, F);
  for (int k = 0; k < 16; ++k) { out[k] = f.dec_lo[k]; out[16 + k] = f.dec_hi[k]; out[32 + k] = f.rec_lo[k]; out[48 + k] = f.rec_hi[k]; }
}
// out: levels, frame_doubles, then per level m, n, mo, no, off, fwd gx, gy, inv gx, gy
void shim_plan(int M, int N, int F, int levels, long long* out) {
  const WvPlan p = wv_plan(M, N, F, levels);
  out[0] = p.levels; out[1] = (long long)p.frame_doubles;
  for (int l = 0; l < p.levels; ++l) {
    const WvLevel& v = p.lv[l];
    const WvGrid f = wv_fwd_grid(v), i = wv_inv_grid(v);
    long long* o = out + 2 + 9 * l;
    o[0] = v.m; o[1] = v.n; o[2] = v.mo; o[3] = v.no; o[4] = (long long)v.off; o[5] = f.gx; o[6] = f.gy; o[7] = i.gx; o[8] = i.gy;
  }
}
long long shim_lds(int F, int inverse) { return (long long)(inverse ? wv_inv_lds_bytes(F) : wv_fwd_lds_bytes(F)); }
int shim_patch(int F, int inverse) { return inverse ? wv_inv_patch(F) : wv_fwd_patch(F); }
void shim_chunks(int n_img, long long staged, long long frame_doubles, int* out) {
  const StagePlan p = wv_chunks(n_img, (size_t)staged, (size_t)frame_doubles);
  out[0] = p.per_chunk; out[1] = p.n_chunks;
}
double shim_mean_squares(const double* x, int R, int C) { return wv_mean_squares(x, R, C, (size_t)C); }
double shim_bayes(double ms, double var) { return wv_bayes_thresh(ms, var); }
double shim_shrink(double x, double t, int mode) { return wv_shrink(x, t, mode); }
int shim_consts(int which) {
  const int v[] = {WV_TAPS_MAX, WV_LEVELS_MAX, WV_TILE, WV_THREADS, WV_THRESH_THREADS, WV_SIGMA_THREADS, (int)WV_LDS_MAX, WV_CHUNK_MAX, (int)(WV_CHUNK_BUDGET >> 20)};
  return v[which];
}
const char* shim_check(int F, const double* lo, int levels, int mode, int method, double sigma, double ppf, double c, const double* thr,
                       int n_thr, int pix, int M, int N, int n_img) {
  WvSpec sp;
  sp.n_taps = F;
  for (int k = 0; k < 16 && k < F; ++k) sp.dec_lo[k] = lo[k];
  sp.levels = levels; sp.mode = mode; sp.method = method; sp.sigma = sigma; sp.ppf = ppf; sp.c = c; sp.thresholds = thr; sp.n_thresholds = n_thr;
  return wv_check(sp, pix, M, N, n_img);
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("wavelet_plan")
    src, so = d / "shim.cpp", d / "libwavelet_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_lds.restype = C.c_longlong
    lib.shim_filters.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.shim_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.shim_chunks.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_void_p]
    lib.shim_mean_squares.restype = C.c_double
    lib.shim_mean_squares.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.shim_bayes.restype = C.c_double
    lib.shim_bayes.argtypes = [C.c_double, C.c_double]
    lib.shim_shrink.restype = C.c_double
    lib.shim_shrink.argtypes = [C.c_double, C.c_double, C.c_int]
    lib.shim_check.restype = C.c_char_p
    lib.shim_check.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int,
                               C.c_int, C.c_int, C.c_int]
    return lib


def plan(shim, M, N, F, levels):
    out = (C.c_longlong * (2 + 9 * 16))()
    shim.shim_plan(M, N, F, levels, out)
    return int(out[0]), int(out[1]), [tuple(int(v) for v in out[2 + 9 * l: 11 + 9 * l]) for l in range(int(out[0]))]


def test_constants(shim):
    assert [shim.shim_consts(i) for i in range(9)] == [16, 16, 16, 256, 256, 1024, 65536, 65535, 256]
    assert R.THRESH_GROUP == 256


def test_level_rule(shim):
    # (F - 1) 2^L <= n: 3 * 8 <= 37 < 3 * 16; 1 * 64 <= 64; 7 * 4 <= 40 < 7 * 8; 15 * 2 <= 30; 15 * 2 > 29; 3 * 32 <= 130 < 3 * 64
    got = [shim.shim_max_level(n, F) for n, F in ((37, 4), (64, 2), (33, 2), (40, 8), (19, 8), (48, 16), (30, 16), (29, 16), (130, 4), (500, 2), (500, 8), (1, 2), (2, 2))]
    assert got == [3, 6, 5, 2, 1, 1, 1, 0, 5, 8, 6, 0, 1]
    assert [shim.shim_default_levels(t) for t in (8, 6, 5, 4, 3, 1)] == [5, 3, 2, 1, 1, 1]
    assert [shim.shim_out_len(n, F) for n, F in ((37, 4), (50, 4), (20, 4), (30, 16), (34, 16), (64, 2), (33, 2))] == [20, 26, 11, 22, 24, 32, 17]
    for n, F in ((37, 4), (500, 2), (500, 8), (30, 16), (29, 16), (64, 2)):
        assert shim.shim_max_level(n, F) == R.max_level(n, F)


def test_shapes_offsets_and_grids(shim):
    # 37 x 50 under 4 taps, one level: bands of 20 x 26; forward 2 x 2 workgroups; inverse writes 37 x 50 = 19 x 25 pairs: 2 x 2
    assert plan(shim, 37, 50, 4, 1) == (1, 2080, [(37, 50, 20, 26, 0, 2, 2, 2, 2)])
    # 130 x 150 under 4 taps, two levels: 66 x 76 (4 * 5016 = 20064 doubles), then 34 x 39 (4 * 1326 = 5304)
    assert plan(shim, 130, 150, 4, 2) == (2, 25368, [(130, 150, 66, 76, 0, 5, 5, 5, 5), (66, 76, 34, 39, 20064, 3, 3, 3, 3)])
    # 500 x 500 under 2 taps, five levels: 250, 125, 63, 32, 16
    L, fd, lv = plan(shim, 500, 500, 2, 5)
    assert (L, fd) == (5, 250000 + 62500 + 15876 + 4096 + 1024) and [v[2] for v in lv] == [250, 125, 63, 32, 16]
    assert [v[4] for v in lv] == [0, 250000, 312500, 328376, 332472] and lv[0][5:] == (16, 16, 16, 16) and lv[2][5:] == (4, 4, 4, 4)
    # 30 x 34 under 16 taps: 22 x 24
    assert plan(shim, 30, 34, 16, 1) == (1, 2112, [(30, 34, 22, 24, 0, 2, 2, 2, 1)])


def test_patches_and_lds_bytes(shim):
    assert [shim.shim_patch(F, 0) for F in (2, 4, 8, 16)] == [32, 34, 38, 46]
    assert [shim.shim_patch(F, 1) for F in (2, 4, 8, 16)] == [16, 17, 19, 23]
    # forward: (32 taps + P^2 + 2 * 16 * P) doubles; inverse: (32 + 4 Q^2 + 2 * Q * 32) doubles
    assert [shim.shim_lds(F, 0) for F in (2, 4, 16)] == [(32 + 1024 + 1024) * 8, (32 + 1156 + 1088) * 8, (32 + 2116 + 1472) * 8]
    assert [shim.shim_lds(F, 1) for F in (2, 4, 16)] == [(32 + 1024 + 1024) * 8, (32 + 1156 + 1088) * 8, (32 + 2116 + 1472) * 8]
    assert shim.shim_lds(16, 0) == 28960 < 65536 < 150 * 1024  # (well inside the LDS rule of the batch plan)


def test_chunks(shim):
    out = (C.c_int * 2)()
    # 500 x 500 under 2 taps: a pyramid of 333496 doubles = 2667968 bytes -> 2668032 aligned; 256 MB hold 100 of them
    shim.shim_chunks(256, 0, 333496, out)
    assert (out[0], out[1]) == (100, 3)
    # with a staged u8 frame (250112) and a staged f64 result (2000128): 4918272 bytes per frame -> 54
    shim.shim_chunks(256, 250112 + 2000128, 333496, out)
    assert (out[0], out[1]) == (54, 5)
    # the stacks of tests/test_gpu_wavelet.py: f64 frames of 1024 x 1024 under 2 taps, one level: a pyramid of four 512 x 512 bands
    # = 8388608 bytes; staged both ways 3 x 8388608 per frame -> 11 = 10 + 1; on the device 33 = 32 + 1
    assert plan(shim, 1024, 1024, 2, 1)[1] == 1048576
    shim.shim_chunks(11, 8388608 + 8388608, 1048576, out)
    assert (out[0], out[1]) == (10, 2)
    shim.shim_chunks(33, 0, 1048576, out)
    assert (out[0], out[1]) == (32, 2)
    shim.shim_chunks(3, 0, 2080, out)
    assert (out[0], out[1]) == (3, 1)
    shim.shim_chunks(200000, 0, 8, out)  # (gridDim.z)
    assert (out[0], out[1]) == (65535, 4)


def test_boundary_and_tap_order(shim):
    # d c b a | a b c d e | e d c
    assert [shim.shim_sym(k, 5) for k in range(-3, 8)] == [2, 1, 0, 0, 1, 2, 3, 4, 4, 3, 2]
    assert [shim.shim_tap(t, 9, 10) for t in range(6)] == [0, 1, 2, 3, 4, 5]
    assert [shim.shim_tap(t, 11, 10) for t in range(6)] == [1, 0, 2, 3, 4, 5]   # the overhang first, walking back from the edge
    assert [shim.shim_tap(t, 13, 10) for t in range(6)] == [3, 2, 1, 0, 4, 5]
    assert [shim.shim_tap(t, 10, 10) for t in range(4)] == [0, 1, 2, 3]


def test_filters_as_the_restatement_derives_them(shim):
    from gaussian_process_edge_trace_amd import _lib
    for name in ("db1", "db4", "sym8", "coif2"):
        lo = np.array(_lib.wavelet_table()[name])
        out = np.zeros(64)
        shim.shim_filters(lo.ctypes.data, len(lo), out.ctypes.data)
        for k, want in enumerate(R.filters(lo)):
            assert np.array_equal(out[16 * k: 16 * k + len(lo)], np.array(want)) and not out[16 * k + len(lo): 16 * k + 16].any()


def test_the_summation_order_is_the_restatements(shim):
    rs = np.random.RandomState(5)
    for R_, C_ in ((1, 1), (3, 7), (20, 26), (66, 76), (255, 9), (256, 5), (257, 5), (600, 3)):
        x = np.ascontiguousarray(rs.normal(0.0, 0.1, (R_, C_)))
        got = shim.shim_mean_squares(x.ctypes.data, R_, C_)
        assert got == R.mean_squares(x), (R_, C_)
        assert abs(got - np.mean(x * x)) <= R.mean_bound(x.size) * np.mean(x * x)
    assert shim.shim_bayes(0.02, 0.01) == R.bayes_thresh(0.02, 0.01) == 0.01 / math.sqrt(0.02 - 0.01)
    assert shim.shim_bayes(0.01, 0.02) == 0.02 / math.sqrt(2.0 ** -52) == R.bayes_thresh(0.01, 0.02)
    for x in (0.3, -0.3, 0.05, -0.05, 0.1, 0.0, -0.0):
        for mode, name in ((0, "soft"), (1, "hard")):
            got, want = shim.shim_shrink(x, 0.1, mode), float(R.shrink(np.array([x]), 0.1, name)[0])
            assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (x, mode)


def test_refusals_and_their_reasons(shim):
    db2 = np.array([-0.12940952255126037, 0.22414386804201339, 0.83651630373780794, 0.48296291314453416])
    thr = np.full(30, 0.01)

    def check(F=4, lo=db2, levels=0, mode=0, method=0, sigma=math.nan, ppf=0.6744897501960817, c=0.0, t=None, n_thr=0, pix=F64, M=40, N=60, n_img=1):
        lo16 = np.zeros(16)
        lo16[:min(len(lo), 16)] = lo[:16]
        r = shim.shim_check(F, lo16.ctypes.data, levels, mode, method, sigma, ppf, c, t.ctypes.data if t is not None else None, n_thr, pix, M, N, n_img)
        return None if r is None else r.decode()

    assert check() is None
    for pix in (U8, U16, F32, F64):
        assert check(pix=pix) is None
    assert "pixel type" in check(pix=4) and "pixel type" in check(pix=-1)
    assert "empty" in check(M=0) and "empty" in check(n_img=0)
    assert "taps" in check(F=0) and "taps" in check(F=3) and "taps" in check(F=18) and check(F=2) is None
    bad = db2.copy()
    bad[2] = math.inf
    assert "finite" in check(lo=bad)
    # 40 x 60 under 4 taps: 3 * 8 <= 40 < 3 * 16 -> max_level 3
    assert check(levels=3) is None and "max_level" in check(levels=4) and "negative" in check(levels=-1)
    assert "max_level is 0" in check(M=2) and check(M=3, N=3, F=2) is None and "max_level is 0" in check(M=1, N=9, F=2)
    assert "mode" in check(mode=2) and "method" in check(method=2) and check(mode=1, method=1, c=3.0) is None
    assert "sigma" in check(sigma=0.0) and "sigma" in check(sigma=-1.0) and "sigma" in check(sigma=math.inf) and check(sigma=0.05) is None
    assert "ppf" in check(ppf=0.0)
    assert "VisuShrink" in check(method=1) and "VisuShrink" in check(method=1, c=math.nan)
    # thresholds: frames * levels * 3 (the default of 40 x 60 is one level)
    assert check(t=thr, n_thr=3) is None and "one per frame" in check(t=thr, n_thr=6) and check(t=thr, n_thr=6, n_img=2) is None
    assert check(t=thr, n_thr=9, levels=3) is None and check(method=1, t=thr, n_thr=3) is None
    neg = thr.copy()
    neg[1] = -0.1
    assert "not negative" in check(t=neg, n_thr=3)
