"""CPU tests of the polar unwrap's rule in csrc/gpet_polar_plan.h (the header needs no HIP: a small extern "C" shim around it is compiled
with the host C++ compiler and -ffp-contract=off, as tests/test_init_plan.py does), and of the ABI surface of gpet_polar_images.

The expected values come from tests/polar_ref.py, the rule restated with numpy float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import polar_ref as R
from tests.test_denoise_plan import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
DTYPES = (np.uint8, np.uint16, np.float32, np.float64)


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    header = open(os.path.join(ROOT, "include", "gpet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_lib.LIB_PATH)
    assert "gpet_polar_images" in declared and hasattr(lib, "gpet_polar_images")
    assert len(_lib.SYMBOLS["gpet_polar_images"][1]) == 9
    assert "typedef struct gpet_polar {" in header and "#define GPET_POLAR_OUT_ON_DEVICE 8u\n" in header
    assert _lib.POLAR_OUT_ON_DEVICE == 8
    assert "#define GPET_ABI_VERSION 1\n" in header  # (additive: the version stays)
    assert hasattr(_lib.Context, "polar_images")
    # the struct as Python lays it out is the header's: 3 pointers-or-doubles of 8 bytes around four int32
    assert C.sizeof(_lib.GpetPolar) == 64 and _lib.GpetPolar.r0.offset == 32 and _lib.GpetPolar.cos_t.offset == 48
    kernels = open(os.path.join(CSRC, "gpet_kernels.hip")).read()
    assert '#include "gpet_k_polar.inc"' in kernels


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_polar_plan.h"
using namespace gpet;
template <typename T>
static void unwrap_t(const void* p, int M, int N, double cx, double cy, const PolarSpec& s, const double* cos_t, const double* sin_t, double* out) {
  const int W = (int)polar_width(s.n_theta, s.pad);
  for (int i = 0; i < s.n_r; ++i)
    for (int c = 0; c < W; ++c) out[(size_t)i * W + c] = polar_sample((const T*)p, M, N, cx, cy, s, cos_t, sin_t, i, c);
}
extern "C" {
int shim_angle(int c, int pad, int n_theta) { return polar_angle(c, pad, n_theta); }
long long shim_width(int n_theta, int pad) { return polar_width(n_theta, pad); }
unsigned int shim_blocks(int n_r, int n_theta, int pad) { return polar_blocks(PolarSpec{0.0, 1.0, n_r, n_theta, pad}); }
int shim_threads() { return POLAR_THREADS; }
const char* shim_check(double r0, double dr, int n_r, int n_theta, int pad, int pix, int M, int N, int n_centres, int n_img, const double* cx,
                       const double* cy) {
  return polar_check(PolarSpec{r0, dr, n_r, n_theta, pad}, pix, M, N, n_centres, n_img, cx, cy);
}
// positions (clamped) and values of one whole frame, pixel type by code
void shim_positions(int M, int N, double cx, double cy, double r0, double dr, int n_r, int n_theta, int pad, const double* cos_t,
                    const double* sin_t, double* x, double* y) {
  const int W = (int)polar_width(n_theta, pad);
  for (int i = 0; i < n_r; ++i)
    for (int c = 0; c < W; ++c) {
      const int a = polar_angle(c, pad, n_theta);
      const double rho = r0 + (double)i * dr;
      x[(size_t)i * W + c] = polar_coord(cx, rho, cos_t[a], N);
      y[(size_t)i * W + c] = polar_coord(cy, rho, sin_t[a], M);
    }
}
int shim_unwrap(const void* p, int pix, int M, int N, double cx, double cy, double r0, double dr, int n_r, int n_theta, int pad,
                const double* cos_t, const double* sin_t, double* out) {
  const PolarSpec s{r0, dr, n_r, n_theta, pad};
  switch (pix) {
    case PIX_U8: unwrap_t<uint8_t>(p, M, N, cx, cy, s, cos_t, sin_t, out); return 0;
    case PIX_U16: unwrap_t<uint16_t>(p, M, N, cx, cy, s, cos_t, sin_t, out); return 0;
    case PIX_F32: unwrap_t<float>(p, M, N, cx, cy, s, cos_t, sin_t, out); return 0;
    case PIX_F64: unwrap_t<double>(p, M, N, cx, cy, s, cos_t, sin_t, out); return 0;
  }
  return 1;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("polar_plan")
    src, so = d / "shim.cpp", d / "libpolar_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    I, D, DP = C.c_int, C.c_double, C.POINTER(C.c_double)
    lib.shim_angle.restype, lib.shim_angle.argtypes = I, [I, I, I]
    lib.shim_width.restype, lib.shim_width.argtypes = C.c_longlong, [I, I]
    lib.shim_blocks.restype, lib.shim_blocks.argtypes = C.c_uint, [I, I, I]
    lib.shim_threads.restype = I
    lib.shim_check.restype, lib.shim_check.argtypes = C.c_char_p, [D, D, I, I, I, I, I, I, I, I, DP, DP]
    lib.shim_positions.restype, lib.shim_positions.argtypes = None, [I, I, D, D, D, D, I, I, I, DP, DP, DP, DP]
    lib.shim_unwrap.restype, lib.shim_unwrap.argtypes = I, [C.c_void_p, I, I, I, D, D, D, D, I, I, I, DP, DP, DP]
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


CASES = [  # (shape, centre, n_r, n_theta, r0, dr, theta0, pad)
    ((37, 53), (46.3, 4.6), 40, 48, 0.0, 0.75, 0.0, 5),     # near a corner: rays leave on two sides
    ((37, 53), (20.25, 17.5), 12, 70, 2.5, 1.0, 0.3, 3),
    ((37, 53), (26.0, 18.0), 1, 16, 7.0, 1.0, 0.0, 0),      # n_r = 1
    ((9, 7), (3.0, 4.0), 6, 4, 0.0, 1.0, -1.0, 4),          # pad = n_theta
    ((2, 2), (0.4, 0.7), 5, 8, 0.0, 0.3, 0.0, 1),           # the smallest frame
]


@pytest.mark.parametrize("dtype", DTYPES)
def test_positions_and_values_equal_the_restated_rule(shim, dtype):
    from gaussian_process_edge_trace_amd import _lib
    for k, (shape, centre, n_r, n_theta, r0, dr, theta0, pad) in enumerate(CASES):
        frame = np.ascontiguousarray(R.frame_of(dtype, shape, 10 + k))
        cos_t, sin_t = R.tables(n_theta, theta0)
        lc, ls = _lib.polar_tables(n_theta, theta0)
        assert np.array_equal(cos_t, lc) and np.array_equal(sin_t, ls)  # (the package hands the restatement's tables over)
        W = R.width(n_theta, pad)
        x, y, out = np.empty((n_r, W)), np.empty((n_r, W)), np.empty((n_r, W))
        shim.shim_positions(shape[0], shape[1], centre[0], centre[1], r0, dr, n_r, n_theta, pad, _dp(cos_t), _dp(sin_t), _dp(x), _dp(y))
        rx, ry = R.positions(shape, centre, n_r, n_theta, r0, dr, theta0, pad)
        assert np.array_equal(x, rx) and np.array_equal(y, ry), k
        assert x.min() >= 0 and x.max() <= shape[1] - 1 and y.min() >= 0 and y.max() <= shape[0] - 1
        assert shim.shim_unwrap(frame.ctypes.data, _lib.pix_code(dtype), shape[0], shape[1], centre[0], centre[1], r0, dr, n_r, n_theta, pad,
                                _dp(cos_t), _dp(sin_t), _dp(out)) == 0
        ref = R.unwrap([frame], centre, n_r, n_theta, r0, dr, theta0, pad)[0]
        assert np.array_equal(out, ref), k
        R.seam_identities(out, n_theta, pad)
    # the first case does leave the frame on two sides, and stays inside elsewhere
    rx, ry = R.positions(*CASES[0][:4], *CASES[0][4:])
    assert (rx == 52).any() and (ry == 0).any() and ((rx > 0) & (rx < 52) & (ry > 0) & (ry < 36)).any()


def test_integer_centre_reads_the_frames_own_pixels(shim):
    frame = np.ascontiguousarray(R.frame_of(np.uint16, (21, 30), 3))
    cos_t, sin_t = R.tables(8, 0.0)
    out = np.empty((9, 9))
    assert shim.shim_unwrap(frame.ctypes.data, 1, 21, 30, 11.0, 6.0, 0.0, 1.0, 9, 8, 0, _dp(cos_t), _dp(sin_t), _dp(out)) == 0
    assert np.array_equal(out[:, 0], frame[6, 11:20].astype(np.float64))


@pytest.mark.parametrize("pad", [0, 1, 12])
def test_column_to_angle_map(shim, pad):
    n_theta = 12
    W = shim.shim_width(n_theta, pad)
    assert W == n_theta + 1 + 2 * pad == R.width(n_theta, pad)
    a = np.array([shim.shim_angle(c, pad, n_theta) for c in range(W)])
    assert np.array_equal(a, R.angle_of_column(np.arange(W), pad, n_theta))
    assert a.min() == 0 and a.max() == n_theta - 1 and a[pad] == 0 and a[pad + n_theta] == 0
    assert np.array_equal(a[pad:pad + n_theta], np.arange(n_theta))
    assert np.array_equal(a[:pad], a[n_theta:n_theta + pad]) and np.array_equal(a[pad + n_theta + 1:], a[pad + 1:2 * pad + 1])


def test_launch_geometry(shim):
    T = shim.shim_threads()
    assert T == 256
    for n_r, n_theta, pad in [(1, 4, 0), (40, 48, 5), (40, 70, 3), (256, 720, 2), (1 << 14, (1 << 14) - 1, 0)]:
        cells = n_r * R.width(n_theta, pad)
        assert shim.shim_blocks(n_r, n_theta, pad) == -(-cells // T)


def test_every_refusal_word_for_word(shim):
    from gaussian_process_edge_trace_amd import _lib
    ok = dict(r0=0.0, dr=1.0, n_r=4, n_theta=8, pad=2, pix=0, M=5, N=6, n_centres=1, n_img=3, cx=[1.0], cy=[2.0])
    cases = [(dict(pix=4), "unknown pixel type"), (dict(pix=-1), "unknown pixel type"), (dict(M=1), "at least 2 x 2"), (dict(N=1), "at least 2 x 2"),
             (dict(n_r=0), "n_r must be at least 1"), (dict(n_theta=3), "n_theta must be at least 4"), (dict(pad=-1), "pad must lie in"),
             (dict(pad=9), "pad must lie in"), (dict(r0=-0.5), "r0 must be finite"), (dict(r0=float("inf")), "r0 must be finite"),
             (dict(r0=float("nan")), "r0 must be finite"), (dict(dr=0.0), "dr must be finite"), (dict(dr=float("inf")), "dr must be finite"),
             (dict(dr=float("nan")), "dr must be finite"), (dict(n_r=1 << 14, n_theta=1 << 14), "exceeds 2^28"),
             (dict(n_r=(1 << 31) - 1, n_theta=(1 << 31) - 1, pad=(1 << 31) - 1), "exceeds 2^28"),
             (dict(n_centres=2, cx=[1.0, 2.0], cy=[1.0, 2.0]), "one centre for all frames or one per frame"),
             (dict(cx=[float("nan")]), "a centre is not finite"), (dict(cy=[float("-inf")]), "a centre is not finite"),
             (dict(n_centres=3, cx=[1.0, 2.0, float("inf")], cy=[1.0, 2.0, 3.0]), "a centre is not finite"),
             (dict(cx=None), "null pointer"), (dict(n_r=0, pix=9, M=0), "unknown pixel type")]  # (the last: the first check wins)

    def ask(a):
        cx = None if a["cx"] is None else np.array(a["cx"], dtype=np.float64)
        cy = np.array(a["cy"], dtype=np.float64)
        got = shim.shim_check(a["r0"], a["dr"], a["n_r"], a["n_theta"], a["pad"], a["pix"], a["M"], a["N"], a["n_centres"], a["n_img"],
                              None if cx is None else _dp(cx), _dp(cy))
        mine = _lib.polar_refusal(a["n_r"], a["n_theta"], a["pad"], a["r0"], a["dr"], a["pix"], a["M"], a["N"], a["n_centres"], a["n_img"],
                                  a["cx"], a["cy"])
        ref = R.refusal(a["n_r"], a["n_theta"], a["pad"], a["r0"], a["dr"], a["pix"] in (0, 1, 2, 3), a["M"], a["N"], a["n_centres"], a["n_img"],
                        a["cx"], a["cy"])
        return (None if got is None else got.decode()), mine, ref
    for change, words in cases:
        got, mine, ref = ask(dict(ok, **change))
        assert got is not None and words in got, (change, got)
        assert got == mine == ref, (change, got, mine, ref)
    for change in [dict(), dict(pad=0), dict(pad=8), dict(n_r=1, n_theta=4), dict(M=2, N=2), dict(n_centres=3, cx=[1.0, 2.0, 3.0], cy=[0.0, 0.0, 0.0]),
                   dict(n_r=1 << 14, n_theta=(1 << 14) - 1, pad=0), dict(pix=3)]:
        assert ask(dict(ok, **change)) == (None, None, None), change
    assert _lib.POLAR_CELLS_MAX == R.CELLS_MAX == 1 << 28 and _lib.POLAR_NTHETA_MIN == R.NTHETA_MIN == 4
