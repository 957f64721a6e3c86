"""CPU tests of what csrc/gpet_band_plan.h decides for tracking bands (the header needs no HIP: a small extern "C" shim around it is
compiled with the host C++ compiler, as tests/test_nlmeans_plan.py does), and of the ABI surface of the band calls.

The expected values come from tests/band_ref.py, the rule restated with Python integers (floor division is Python's own), and from
literals worked out by hand."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import band_ref as R
from tests.test_denoise_plan import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
CALLS = {"gpet_batch_create_banded": 9, "gpet_batch_band_place": 3, "gpet_batch_band_set": 2, "gpet_batch_band_r0": 2}


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
    for method in ("band_place", "band_set", "band_r0"):
        assert hasattr(_lib.Batch, method)
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()


def test_structs_agree_between_header_and_python(tmp_path):
    from gaussian_process_edge_trace_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpet_hip.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(gpet_band), offsetof(gpet_band, r0), '
                    'offsetof(gpet_band, pair_of), sizeof(gpet_band_images), offsetof(gpet_band_images, pix), '
                    'offsetof(gpet_band_images, kern), offsetof(gpet_band_images, dn), offsetof(gpet_band_images, flags));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    B, I = _lib.GpetBand, _lib.GpetBandImages
    assert got == [C.sizeof(B), B.r0.offset, B.pair_of.offset, C.sizeof(I), I.pix.offset, I.kern.offset, I.dn.offset, I.flags.offset]
    assert got[:3] == [24, 8, 16]


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_band_plan.h"
using namespace gpet;
extern "C" {
long long shim_place(long long M, long long H, long long lo, long long hi, long long i_lo, long long i_hi) {
  return band_place(M, H, lo, hi, i_lo, i_hi);
}
const char* shim_check(long long M, long long H, long long r0, long long i_lo, long long i_hi, int place) {
  return band_check(M, H, r0, i_lo, i_hi, place != 0);
}
long long shim_floor_half(long long a) { return band_floor_half(a); }
long long shim_image_bytes(int n_pair, int M, int N) { return (long long)band_image_bytes(n_pair, M, N); }
long long shim_table_bytes(int B, int n_init_max) { return (long long)band_table_bytes(B, n_init_max); }
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("band_plan")
    src, so = d / "shim.cpp", d / "libband_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    LL = C.c_longlong
    lib.shim_place.restype = LL
    lib.shim_place.argtypes = [LL] * 6
    lib.shim_check.restype = C.c_char_p
    lib.shim_check.argtypes = [LL] * 5 + [C.c_int]
    lib.shim_floor_half.restype = LL
    lib.shim_floor_half.argtypes = [LL]
    lib.shim_image_bytes.restype = LL
    lib.shim_table_bytes.restype = LL
    return lib


def test_floor_division_of_negative_values(shim):
    for a in range(-9, 10):
        assert shim.shim_floor_half(a) == a // 2
    assert shim.shim_floor_half(-1) == -1 and shim.shim_floor_half(-3) == -2


def test_band_place_equals_the_restated_rule_on_an_exhaustive_grid(shim):
    """M <= 12, every H, every lo <= hi in the frame, every init span inside the frame that fits the band."""
    from gaussian_process_edge_trace_amd import _lib
    seen = dict(clamp_top=0, clamp_bottom=0, init_lo=0, init_hi=0, n=0)
    for M in range(1, 13):
        for H in range(1, M + 1):
            for lo in range(M):
                for hi in range(lo, M):
                    for i_lo in range(M):
                        for i_hi in range(i_lo, min(M, i_lo + H)):
                            want = R.place(M, H, [lo, hi], [i_lo, i_hi])
                            assert shim.shim_place(M, H, lo, hi, i_lo, i_hi) == want, (M, H, lo, hi, i_lo, i_hi)
                            assert _lib.band_place(M, H, lo, hi, i_lo, i_hi) == want
                            # the result is a band of the frame that holds the inits
                            assert 0 <= want <= M - H and want <= i_lo and i_hi <= want + H - 1
                            raw = (lo + hi) // 2 - H // 2
                            boxed = min(max(raw, 0), M - H)
                            seen["clamp_top"] += raw < 0
                            seen["clamp_bottom"] += raw > M - H
                            seen["init_lo"] += boxed > i_lo
                            seen["init_hi"] += boxed < i_hi - H + 1
                            seen["n"] += 1
    assert all(v > 0 for v in seen.values()), seen


def test_band_place_literals(shim):
    # centred: (20 + 30) // 2 - 32 // 2 = 9
    assert shim.shim_place(64, 32, 20, 30, 22, 24) == 9
    # the frame's top and bottom: (0 + 3) // 2 - 16 = -15 -> 0;  (60 + 63) // 2 - 16 = 45 -> 64 - 32 = 32
    assert shim.shim_place(64, 32, 0, 3, 5, 5) == 0
    assert shim.shim_place(64, 32, 60, 63, 40, 40) == 32
    # the init clamps: the trace went down, the init at row 10 holds the band back; the trace went up, the init at row 50 pulls it down
    assert shim.shim_place(64, 24, 40, 50, 10, 10) == 10
    assert shim.shim_place(64, 24, 5, 9, 50, 50) == 27
    # odd sums and odd H floor: (5 + 6) // 2 - 5 // 2 = 5 - 2 = 3
    assert shim.shim_place(12, 5, 5, 6, 4, 4) == 3


def test_all_ignored_traces_keep_the_band():
    """NaN and rows outside the frame are ignored; with none left the band stays (the restated rule; on the device k_band_place keeps
    r0 when its ballot finds no usable row -- tests/test_gpu_bands.py)."""
    assert R.place(64, 32, [np.nan, -1.0, 64.0, 1e9], [20, 20], r0_old=7) == 7
    assert R.place(64, 32, [np.nan, 30.0, -4.0], [20, 20], r0_old=7) == 14
    assert R.place(64, 32, [], [20, 20], r0_old=None) is None


def test_every_refusal_returns_its_reason(shim):
    from gaussian_process_edge_trace_amd import _lib
    cases = [((64, 0, 0, 5, 5), "band_rows must be at least 1"),
             ((64, 65, 0, 5, 5), "H > M"),
             ((64, 8, 0, 5, 13), "span more rows"),
             ((64, 32, -1, 5, 5), "outside [0, M - H]"),
             ((64, 32, 33, 40, 40), "outside [0, M - H]"),
             ((64, 32, 10, 9, 12), "an init point lies outside its band"),
             ((64, 32, 10, 20, 42), "an init point lies outside its band")]
    for args, words in cases:
        got = shim.shim_check(*args, 0)
        assert got is not None and words in got.decode(), (args, got)
        assert got.decode() == R.refusal(*args) == _lib.band_refusal(*args)
    for args in [(64, 32, 0, 0, 31), (64, 32, 32, 32, 63), (64, 64, 0, 0, 63), (64, 1, 7, 7, 7)]:
        assert shim.shim_check(*args, 0) is None and R.refusal(*args) is None and _lib.band_refusal(*args) is None
    # a band still to be placed is judged by H alone
    assert shim.shim_check(64, 32, -1, 5, 5, 1) is None and R.refusal(64, 32, None, 5, 5) is None
    assert b"span more rows" in shim.shim_check(64, 8, -1, 5, 13, 1)
    assert b"H > M" in shim.shim_check(64, 65, -1, 5, 5, 1)


def test_byte_sizes(shim):
    assert shim.shim_image_bytes(3, 64, 65) == 3 * 64 * 65 * 4
    # r0, placed r0, r0 of the fits: 3 B; (i_lo, i_hi): 2 B; inits: B * n_init_max * 2 -- int64 each
    assert shim.shim_table_bytes(4, 2) == (5 * 4 + 4 * 2 * 2) * 8
