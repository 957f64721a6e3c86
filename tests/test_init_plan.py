"""CPU tests of the rule of endpoint tracking in csrc/gpet_init_plan.h (the header needs no HIP: a small extern "C" shim around it is
compiled with the host C++ compiler, as tests/test_band_plan.py does), and of the ABI surface of the three init calls.

The expected values come from tests/init_follow_ref.py, the rule restated with Python floats and integers, and from literals worked out
by hand on crafted images."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import init_follow_ref as R
from tests.test_denoise_plan import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
CALLS = {"gpet_batch_init_follow": 4, "gpet_batch_set_init": 2, "gpet_batch_init_xy": 2}


def _header_text():
    return open(os.path.join(ROOT, "include", "gpet_hip.h")).read()


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    declared = set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in CALLS.items():
        assert name in declared and hasattr(lib, name), name
        assert len(_lib.SYMBOLS[name][1]) == n_args, name
    for method in ("init_follow", "set_init", "init_xy"):
        assert hasattr(_lib.Batch, method)
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()
    assert "gpet_api_init.hip" in ge.HIP_SOURCES


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_init_plan.h"
using namespace gpet;
extern "C" {
long long shim_follow(const float* G, long long M, long long N, long long x, long long y, long long w, long long a) {
  return init_follow_row(G, M, N, x, y, w, a);
}
double shim_score(const float* G, long long N, long long r, long long x, long long a) { return init_score(G, N, r, x, a); }
int shim_better(double s, long long d, long long r, double bs, long long bd, long long br) { return init_better(s, d, r, bs, bd, br) ? 1 : 0; }
const char* shim_check(long long w, long long a) { return init_follow_check(w, a); }
long long shim_window_max() { return INIT_WINDOW_MAX; }
long long shim_cols_max() { return INIT_COLS_MAX; }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("init_plan")
    src, so = d / "shim.cpp", d / "libinit_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    LL, FP = C.c_longlong, C.POINTER(C.c_float)
    lib.shim_follow.restype = LL
    lib.shim_follow.argtypes = [FP] + [LL] * 6
    lib.shim_score.restype = C.c_double
    lib.shim_score.argtypes = [FP] + [LL] * 4
    lib.shim_better.restype = C.c_int
    lib.shim_better.argtypes = [C.c_double, LL, LL, C.c_double, LL, LL]
    lib.shim_check.restype = C.c_char_p
    lib.shim_check.argtypes = [LL, LL]
    lib.shim_window_max.restype = LL
    lib.shim_cols_max.restype = LL
    return lib


def follow(shim, G, x, y, w, a):
    G = np.ascontiguousarray(G, dtype=np.float32)
    return shim.shim_follow(G.ctypes.data_as(C.POINTER(C.c_float)), G.shape[0], G.shape[1], x, y, w, a)


def both(shim, G, x, y, w, a):
    """The header's row, after checking that the restated rule gives the same."""
    got = follow(shim, G, x, y, w, a)
    assert got == R.follow_row(np.asarray(G, dtype=np.float32), x, y, w, a), (x, y, w, a, got)
    return got


def test_header_equals_the_restated_rule_on_random_images(shim):
    rng = np.random.default_rng(5)
    moved = 0
    for M, N in [(1, 1), (2, 3), (7, 5), (33, 17), (96, 72), (130, 9)]:
        G = rng.random((M, N)).astype(np.float32)
        G[rng.random((M, N)) < 0.3] = 0.0
        G8 = np.rint(G * 4).astype(np.float32)  # (few distinct values: many exact ties)
        for img in (G, G8):
            for _ in range(60):
                x, y = int(rng.integers(0, N)), int(rng.integers(0, M))
                w, a = int(rng.choice([0, 1, 2, 5, 40, 70, M, 4096])), int(rng.choice([0, 1, 2, 4, 64]))
                moved += both(shim, img, x, y, w, a) != y
                p = img.ctypes.data_as(C.POINTER(C.c_float))
                assert shim.shim_score(p, N, y, x, a) == R.score(img, y, x, a)
    assert moved > 100


def test_f64_sum_in_ascending_columns(shim):
    """1e8 + 1 + ... is exact in f64 and not in f32; (2^53 + 1) + 1 depends on the order of the additions."""
    G = np.array([[1e8, 1.0, 1.0, 1.0, 1.0]], dtype=np.float32)
    p = G.ctypes.data_as(C.POINTER(C.c_float))
    assert shim.shim_score(p, 5, 0, 2, 2) == 100000004.0
    G = np.array([[2.0 ** 53, 1.0, 1.0], [1.0, 1.0, 2.0 ** 53]], dtype=np.float32)
    p = G.ctypes.data_as(C.POINTER(C.c_float))
    assert shim.shim_score(p, 3, 0, 1, 1) == 2.0 ** 53             # (2^53 + 1) + 1: both additions round back
    assert shim.shim_score(p, 3, 1, 1, 1) == 2.0 ** 53 + 2.0       # (1 + 1) + 2^53
    assert both(shim, G, 1, 0, 1, 1) == 1


def test_ties(shim):
    G = np.zeros((21, 9), dtype=np.float32)
    # equal score at equal distance: the smaller row wins
    G[7, 4] = G[13, 4] = 2.0
    assert both(shim, G, 4, 10, 5, 0) == 7
    # equal score at different distance: the nearer row wins, above or below
    G[:] = 0
    G[6, 4] = G[12, 4] = 2.0
    assert both(shim, G, 4, 10, 5, 0) == 12
    G[:] = 0
    G[9, 4] = G[14, 4] = 2.0
    assert both(shim, G, 4, 10, 5, 0) == 9
    # the largest score wins whatever its distance; the point's own row is a candidate like any other
    G[:] = 0
    G[10, 4], G[15, 4] = 1.0, 1.5
    assert both(shim, G, 4, 10, 5, 0) == 15
    assert both(shim, G, 4, 10, 4, 0) == 10
    # ties of the SUM, not of single pixels: 1 + 2 == 2 + 1 over three columns
    G[:] = 0
    G[3, 3:6] = [1, 2, 0]
    G[5, 3:6] = [0, 2, 1]
    assert both(shim, G, 4, 4, 3, 1) == 3
    assert both(shim, G, 4, 5, 3, 1) == 5 and both(shim, G, 4, 3, 3, 1) == 3


def test_row_window_is_clipped_to_the_image(shim):
    M, N = 12, 6
    G = np.zeros((M, N), dtype=np.float32)
    G[0, 2], G[M - 1, 2] = 3.0, 4.0
    assert both(shim, G, 2, 1, 5, 0) == 0          # rows -4 .. 6 -> 0 .. 6
    assert both(shim, G, 2, 0, 3, 0) == 0
    assert both(shim, G, 2, M - 3, 5, 0) == M - 1  # rows 4 .. 14 -> 4 .. 11
    assert both(shim, G, 2, M - 1, 2, 0) == M - 1
    # w >= M: the whole column, from any row
    for y in range(M):
        assert both(shim, G, 2, y, M, 0) == M - 1 and both(shim, G, 2, y, 4096, 0) == M - 1
    # a point outside the image whose window reaches in, and one whose window does not
    assert both(shim, G, 2, -2, 3, 0) == 0 and both(shim, G, 2, M + 1, 2, 0) == M - 1
    assert both(shim, G, 2, -5, 3, 0) == -5 and both(shim, G, 2, M + 7, 3, 0) == M + 7


def test_column_window_is_clipped_to_the_image(shim):
    M, N = 9, 7
    G = np.zeros((M, N), dtype=np.float32)
    G[2, 0:3] = 1.0     # sum 3 over columns 0 .. 2
    G[6, 0:2] = 1.25    # sum 2.5
    assert both(shim, G, 0, 4, 4, 2) == 2   # x = 0: columns -2 .. 2 -> 0 .. 2
    assert both(shim, G, 0, 4, 4, 1) == 6   # columns 0 .. 1: 2 against 2.5
    G[:] = 0
    G[1, N - 3:] = 1.0
    G[7, N - 2:] = 1.25
    assert both(shim, G, N - 1, 4, 4, 2) == 1 and both(shim, G, N - 1, 4, 4, 1) == 7
    assert both(shim, G, N - 1, 4, 4, 64) == 1  # cols wider than the image: the whole row
    G[:] = 0
    G[3, 0] = 1.0
    assert both(shim, G, N - 1, 5, 4, N - 2) == 5 and both(shim, G, N - 1, 5, 4, N - 1) == 3


def test_what_does_not_count(shim):
    G = np.zeros((16, 8), dtype=np.float32)
    for y in (0, 7, 15):
        assert both(shim, G, 3, y, 8, 2) == y               # an all-zero window: the point stays
    G[4, 3] = 5.0
    assert both(shim, G, 3, 9, 4, 0) == 9                   # the only bright row is one row outside the window
    assert both(shim, G, 3, 9, 5, 0) == 4
    assert both(shim, G, 3, 9, 0, 0) == 9 and both(shim, G, 3, 4, 0, 4) == 4   # w = 0 moves nothing
    G[:] = 0
    G[6, 2:5] = [1.0, -3.0, 1.0]                             # a negative sum does not count, a positive one beside it does
    G[11, 3] = 0.5
    assert both(shim, G, 3, 9, 4, 1) == 11
    G[8, 3] = np.nan                                         # NaN fails s > 0
    G[12, 2] = np.nan
    assert both(shim, G, 3, 9, 4, 1) == 11
    G[11, 3] = 0.0
    assert both(shim, G, 3, 9, 4, 1) == 9
    G[7, 3] = np.inf                                         # +inf counts and wins
    assert both(shim, G, 3, 9, 4, 0) == 7


def test_the_ordering_itself(shim):
    b = shim.shim_better
    assert b(1.0, 9, 9, 0.0, 0, 0) == 1 and b(0.0, 0, 0, 0.0, 0, 0) == 0 and b(float("nan"), 0, 0, 0.0, 0, 0) == 0
    assert b(-1.0, 0, 0, 0.0, 0, 0) == 0 and b(0.0, 0, 0, 1.0, 5, 5) == 0 and b(float("nan"), 0, 0, 1.0, 5, 5) == 0
    assert b(2.0, 9, 9, 1.0, 0, 0) == 1 and b(1.0, 0, 0, 2.0, 9, 9) == 0
    assert b(2.0, 1, 9, 2.0, 2, 0) == 1 and b(2.0, 2, 0, 2.0, 1, 9) == 0
    assert b(2.0, 2, 3, 2.0, 2, 7) == 1 and b(2.0, 2, 7, 2.0, 2, 3) == 0 and b(2.0, 2, 3, 2.0, 2, 3) == 0


def test_every_refusal_returns_its_reason(shim):
    from gaussian_process_edge_trace_amd import _lib
    assert shim.shim_window_max() == R.WINDOW_MAX == _lib.INIT_WINDOW_MAX == 4096
    assert shim.shim_cols_max() == R.COLS_MAX == _lib.INIT_COLS_MAX == 64
    cases = [((-1, 4), "window must be at least 0"), ((4097, 4), "window exceeds 4096"), ((8, -1), "cols must be at least 0"),
             ((8, 65), "cols exceeds 64"), ((-1, -1), "window must be at least 0")]
    for args, words in cases:
        got = shim.shim_check(*args)
        assert got is not None and words in got.decode(), (args, got)
        assert got.decode() == R.refusal(*args) == _lib.init_follow_refusal(*args)
    for args in [(0, 0), (4096, 64), (8, 4), (0, 64), (4096, 0)]:
        assert shim.shim_check(*args) is None and R.refusal(*args) is None and _lib.init_follow_refusal(*args) is None
