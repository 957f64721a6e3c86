"""CPU tests of what csrc/gpet_nlfast_plan.h decides before the fast-mode non-local means kernels are launched (the header needs
no HIP: a small extern "C" shim around it is compiled with the host C++ compiler, as tests/test_nlmeans_plan.py does), of the
Python mirror _lib.nlmeans_fast_plan, and of the ABI surface of gpet_nlmeans_fast_images.

Every expected figure is a literal worked out by hand from the rules the header states: pad = s / 2 + d + 1; (2 d + 1)(d + 1)
shifts, t_row outer, t_col = 0 .. d inner, alpha 0.5 on the column t_col = 0 but for (0, 0); a frame's workspace is the padded
frame, two accumulators of M N and (d + 1) planes per row of shifts, float64, to 256 bytes; as many whole rows as fit 256 MiB."""
import ctypes as C
import math
import re
import subprocess

import os
import pytest

from tests import nlmeans_fast_ref as R
from tests.test_denoise_plan import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
U8, U16, F32, F64 = range(4)
MIB256 = 256 << 20


def _header_text():
    return open(os.path.join(ROOT, "include", "gpet_hip.h")).read()


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    assert "gpet_nlmeans_fast_images" in set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    assert hasattr(C.CDLL(_lib.LIB_PATH), "gpet_nlmeans_fast_images")
    assert len(_lib.SYMBOLS["gpet_nlmeans_fast_images"][1]) == 9
    assert hasattr(_lib.Context, "nlmeans_fast_images")
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()


def test_struct_agrees_between_header_and_python_and_the_classic_one_is_untouched():
    from gaussian_process_edge_trace_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    body = re.search(r"typedef struct gpet_nlmeans_fast \{(.*?)\} gpet_nlmeans_fast;", text, re.S).group(1)
    fields = [tuple(reversed(decl.strip().rsplit(None, 1))) for decl in body.split(";") if decl.strip()]
    names = {C.c_int32: "int32_t", C.c_double: "double"}
    assert fields == [(n, names[t]) for n, t in _lib.GpetNlmeansFast._fields_]
    assert [n for n, _ in fields] == ["patch_size", "patch_distance", "h", "sigma"]
    assert C.sizeof(_lib.GpetNlmeansFast) == 24 and _lib.GpetNlmeansFast.h.offset == 8 and _lib.GpetNlmeansFast.sigma.offset == 16
    # the stage takes the classic stage's flags: no define of its own
    assert dict(re.findall(r"#define\s+(GPET_NLM_[A-Z_]+)\s+(\d+)u?\b", _header_text())) == dict(GPET_NLM_OUT_ON_DEVICE="8")
    assert C.sizeof(_lib.GpetNlmeans) == 32 and len(_lib.SYMBOLS["gpet_nlmeans_images"][1]) == 9


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_nlfast_plan.h"
using namespace gpet;
extern "C" {
void shim_plan(int M, int N, int s, int d, long long budget, long long* o) {
  const NlfPlan p = budget ? nlf_plan(M, N, s, d, (size_t)budget) : nlf_plan(M, N, s, d);
  long long v[] = {p.s, p.off, p.d, p.pad, p.nr, p.nc, p.n_shifts, p.rows_per_group, p.n_groups, p.strips, p.steps, (long long)p.plane_doubles,
                   (long long)p.off_w, (long long)p.off_r, (long long)p.off_i, (long long)p.frame_bytes, nlf_pad_blocks(p), nlf_gather_blocks(M, N)};
  for (int i = 0; i < 18; ++i) o[i] = v[i];
}
void shim_groups(int M, int N, int s, int d, int* first, int* count) {
  const NlfPlan p = nlf_plan(M, N, s, d);
  for (int g = 0; g < p.n_groups; ++g) { first[g] = nlf_group_first(p, g); count[g] = nlf_group_count(p, g); }
}
void shim_chunks(int n_img, long long staged, int M, int N, int s, int d, int* o) {
  const StagePlan q = nlf_chunks(n_img, (size_t)staged, nlf_plan(M, N, s, d));
  o[0] = q.per_chunk; o[1] = q.n_chunks;
}
void shim_shift(int d, int k, int* t, double* alpha) { const NlfShift q = nlf_shift(d, k); t[0] = q.t_row; t[1] = q.t_col; *alpha = q.alpha; }
int shim_shifts(int d) { return nlf_shifts(d); }
void shim_ranges(int n, int t, int off, int* o) {
  o[0] = nlf_integral_lo(t); o[1] = nlf_integral_hi(n, t); o[2] = nlf_weight_lo(t, off); o[3] = nlf_weight_hi(n, t, off);
}
int shim_partner_first(int t_row, int t_col) { return nlf_partner_first(t_row, t_col) ? 1 : 0; }
const char* shim_check(int ps, int d, double h, double sigma, int pix, int M, int N) {
  NlfSpec sp;
  sp.patch_size = ps; sp.patch_distance = d; sp.h = h; sp.sigma = sigma;
  return nlf_check(sp, pix, M, N);
}
long long shim_consts(int which) { return which == 0 ? NLF_STRIP : which == 1 ? NLF_THREADS : which == 2 ? (long long)NLF_CHUNK_BUDGET : NLF_CHUNK_MAX; }
}
"""
PLAN_KEYS = ("s", "off", "d", "pad", "nr", "nc", "n_shifts", "rows_per_group", "n_groups", "strips", "steps", "plane_doubles", "off_w", "off_r",
             "off_i", "frame_bytes", "pad_blocks", "gather_blocks")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("nlfast_plan")
    src, so = d / "shim.cpp", d / "libnlfast_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_plan.argtypes = [C.c_int] * 4 + [C.c_longlong, C.c_void_p]
    lib.shim_chunks.argtypes = [C.c_int, C.c_longlong] + [C.c_int] * 4 + [C.c_void_p]
    lib.shim_check.restype = C.c_char_p
    lib.shim_check.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int]
    lib.shim_consts.restype = C.c_longlong
    return lib


def _plan(shim, M, N, s, d, budget=0):
    o = (C.c_longlong * 18)()
    shim.shim_plan(M, N, s, d, budget, o)
    return dict(zip(PLAN_KEYS, list(o)))


def test_constants(shim):
    assert [shim.shim_consts(i) for i in range(4)] == [64, 256, MIB256, 65535]


def test_shift_table_against_the_restatements(shim):
    t, a = (C.c_int * 2)(), C.c_double()
    for d in (0, 1, 2, 3, 11, 31):
        table = R.shifts(d)
        assert shim.shim_shifts(d) == len(table) == (2 * d + 1) * (d + 1)
        for k, exp in enumerate(table):
            shim.shim_shift(d, k, t, C.byref(a))
            assert (t[0], t[1], a.value) == exp, (d, k)
    # literals: d = 2 -> 15 shifts, the first (-2, 0) with alpha 0.5, the seventh (0, 0) with alpha 1
    shim.shim_shift(2, 0, t, C.byref(a))
    assert (t[0], t[1], a.value) == (-2, 0, 0.5)
    shim.shim_shift(2, 6, t, C.byref(a))
    assert (t[0], t[1], a.value) == (0, 0, 1.0)
    shim.shim_shift(2, 14, t, C.byref(a))
    assert (t[0], t[1], a.value) == (2, 2, 1.0)


def test_ranges_at_the_first_the_middle_and_the_last_shift(shim):
    o = (C.c_int * 4)()

    def ranges(n, t, off):
        shim.shim_ranges(n, t, off, o)
        assert (o[0], o[1]) == R.integral_range(n, t) and (o[2], o[3]) == R.weight_range(n, t, off)
        return tuple(o)

    # the defaults on 20 x 70: off 3, d 11, nr 50, nc 100.  t = (-d, 0): rows from 11, every column from 1
    assert ranges(50, -11, 3) == (11, 50, 14, 47) and ranges(100, 0, 3) == (1, 100, 3, 97)
    # t = (0, 0)
    assert ranges(50, 0, 3) == (1, 50, 3, 47)
    # t = (d, d): the ranges end d early
    assert ranges(50, 11, 3) == (1, 39, 3, 36) and ranges(100, 11, 3) == (1, 89, 3, 86)
    assert ranges(7, -1, 1) == (1, 7, 2, 6) and ranges(7, 1, 1) == (1, 6, 1, 5)


def test_per_pixel_order(shim):
    for t_row in range(-3, 4):
        for t_col in range(0, 4):
            exp = R.terms_in_order(t_row, t_col)[0] == "partner"
            assert bool(shim.shim_partner_first(t_row, t_col)) == exp == (t_row > 0 or (t_row == 0 and t_col > 0))


def test_every_pair_of_an_output_pixel_lies_inside_the_weight_ranges(shim):
    """What lets the gather kernel skip the range test: pad = off + d + 1."""
    o = (C.c_int * 4)()
    for s, d, n in ((3, 0, 4), (3, 2, 9), (7, 11, 20), (15, 31, 70), (5, 31, 41)):
        off = s // 2
        pad = off + d + 1
        for t in range(-d, d + 1):
            shim.shim_ranges(n + 2 * pad, t, off, o)
            for p in (pad, pad + n - 1):  # the first and the last output position along the axis
                assert o[2] <= p < o[3] and o[2] <= p - t < o[3], (s, d, n, t, p)


def test_geometry_groups_and_workspace(shim):
    from gaussian_process_edge_trace_amd import _lib
    # 20 x 70 at the defaults: plane 50 * 100, all 23 rows in one group: (5000 + 2 * 1400 + 276 * 5000) * 8 = 11102400 -> 11102464
    p = _plan(shim, 20, 70, 7, 11)
    assert p == dict(s=7, off=3, d=11, pad=15, nr=50, nc=100, n_shifts=276, rows_per_group=23, n_groups=1, strips=1, steps=163, plane_doubles=5000,
                     off_w=5000, off_r=6400, off_i=7800, frame_bytes=11102464, pad_blocks=20, gather_blocks=6)
    # 500 x 500 at the defaults: plane 530^2 = 280900, a row of 12 planes 3370800 doubles, 780900 besides: 9 rows fit 2^25 doubles
    p = _plan(shim, 500, 500, 7, 11)
    assert (p["nr"], p["plane_doubles"], p["rows_per_group"], p["n_groups"], p["strips"], p["steps"], p["frame_bytes"]) == (530, 280900, 9, 3, 9, 593, 248944896)
    first, count = (C.c_int * 3)(), (C.c_int * 3)()
    shim.shim_groups(500, 500, 7, 11, first, count)
    assert list(first) == [0, 108, 216] and list(count) == [108, 108, 60]
    # 100 x 100, s = 3, d = 31: pad 33, plane 166^2 = 27556, a row of 32 planes: 37 of the 63 rows fit
    p = _plan(shim, 100, 100, 3, 31)
    assert (p["pad"], p["nr"], p["n_shifts"], p["rows_per_group"], p["n_groups"], p["strips"], p["frame_bytes"]) == (33, 166, 2016, 37, 2, 3, 261391104)
    shim.shim_groups(100, 100, 3, 31, first, count)
    assert list(first)[:2] == [0, 1184] and list(count)[:2] == [1184, 832]
    # strips: 64 rows each
    assert [_plan(shim, M, 40, 3, 1)["strips"] for M in (58, 59, 122, 123)] == [1, 2, 2, 3]  # nr = M + 6
    # a smaller budget: 20 x 70 at the defaults in 1 MiB: (7800 + rows * 60000) * 8 <= 1048576 -> 2 rows, 12 groups
    p = _plan(shim, 20, 70, 7, 11, budget=1 << 20)
    assert (p["rows_per_group"], p["n_groups"], p["frame_bytes"]) == (2, 12, 1022464)  # ((7800 + 120000) * 8 = 1022400, to 256)
    # the mirror
    for M, N, s, d in ((20, 70, 7, 11), (500, 500, 7, 11), (100, 100, 3, 31), (9, 11, 5, 2), (1000, 1000, 15, 31), (70, 75, 3, 1)):
        p, m = _plan(shim, M, N, s, d), _lib.nlmeans_fast_plan(M, N, s, d)
        assert {k: p[k] for k in ("pad", "nr", "nc", "n_shifts", "rows_per_group", "n_groups", "strips", "frame_bytes")} == {k: m[k] for k in m if k != "frames_per_chunk"}
    assert _lib.NLF_STRIP == 64 and _lib.NLF_CHUNK_BUDGET == MIB256


def test_a_frame_whose_single_row_of_shifts_does_not_fit_is_reported(shim):
    # 1000 x 1000, s = 15, d = 31: pad 39, plane 1078^2 = 1162084, one row of 32 planes alone is 297 MB
    p = _plan(shim, 1000, 1000, 15, 31)
    assert (p["rows_per_group"], p["n_groups"]) == (0, 0) and p["frame_bytes"] == 322790400 > MIB256  # ((1162084 * 33 + 2000000) * 8, to 256)
    # 900 x 900: plane 978^2 = 956484, (33 * 956484 + 1620000) * 8 = 265471776 <= 2^28: one row fits, 63 groups (265472000 to 256)
    p = _plan(shim, 900, 900, 15, 31)
    assert (p["rows_per_group"], p["n_groups"], p["frame_bytes"]) == (1, 63, 265472000)


def test_chunks(shim):
    o = (C.c_int * 2)()

    def chunks(n, staged, M, N, s, d):
        shim.shim_chunks(n, staged, M, N, s, d, o)
        return o[0], o[1]

    # 20 x 70 at the defaults: 11102464 bytes a frame -> 24 frames fit 256 MiB; with 12800 bytes staged as well, still 24
    assert chunks(100, 0, 20, 70, 7, 11) == (24, 5) and chunks(24, 0, 20, 70, 7, 11) == (24, 1) and chunks(25, 12800, 20, 70, 7, 11) == (24, 2)
    # a frame that takes the budget alone: one per chunk, staging or not
    assert chunks(3, 0, 100, 100, 3, 31) == (1, 3) and chunks(3, 160000, 100, 100, 3, 31) == (1, 3)
    # tiny frames: the grid's z extent bounds the chunk
    assert chunks(70000, 0, 4, 4, 3, 0) == (65535, 2)


def test_refusals_and_their_reasons(shim):
    def check(ps=7, d=11, h=0.1, sigma=0.0, pix=F64, M=40, N=60):
        r = shim.shim_check(ps, d, h, sigma, pix, M, N)
        return None if r is None else r.decode()

    assert check() is None
    for pix in (U8, U16, F32, F64):
        assert check(pix=pix) is None
    assert check(ps=2, d=0, M=3, N=3) is None and check(ps=15, d=31, M=41, N=41) is None and check(sigma=0.3) is None
    assert "pixel type" in check(pix=4) and "pixel type" in check(pix=-1)
    assert "patch_size" in check(ps=1) and "patch_size" in check(ps=0) and "patch_size" in check(ps=-3)
    assert "15 x 15" in check(ps=16) and "15 x 15" in check(ps=17)
    assert "negative" in check(d=-1) and "above 31" in check(d=32)
    assert "h must" in check(h=0.0) and "h must" in check(h=-1.0) and "h must" in check(h=math.nan) and "h must" in check(h=math.inf)
    assert "sigma" in check(sigma=-0.1) and "sigma" in check(sigma=math.nan) and "sigma" in check(sigma=math.inf)
    # pad = 3 + 11 + 1 = 15 must be at most min(M, N) - 1
    assert "reflects once" in check(M=15) and "reflects once" in check(N=15) and check(M=16, N=16) is None
    assert "reflects once" in check(ps=3, d=0, M=2) and check(ps=3, d=0, M=3, N=3) is None
    assert "reflects once" in check(ps=15, d=31, M=39) and "empty" in check(M=0)
