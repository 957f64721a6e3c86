"""CPU tests of what csrc/gpet_tvb_plan.h decides before the split-Bregman kernels are launched (the header needs no HIP: a small
extern "C" shim around it is compiled with the host C++ compiler, as tests/test_wavelet_plan.py does), and of the ABI surface of
gpet_tvb_images.

Every expected figure is a literal worked out by hand from the rules the header states: a frame's workspace is six arrays of
(M + 2)(N + 2) doubles, rounded up to 256 bytes; an array is stored anti-diagonal after anti-diagonal, a diagonal by ascending row;
the workgroup has 512 lanes and a lane owns ceil(min(M, N) / 512) cells of the longest diagonal; a launch runs four sweeps; LDS
holds 2 x 5 x min(M, N) doubles of hand-over and 512 partial sums; a chunk's workspaces and staging stay inside 256 MB.  None was
produced by the header under test; the order of acc is checked against its restatement in tests/tvb_ref.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import tvb_ref as R
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
    assert "gpet_tvb_images" in set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    assert hasattr(C.CDLL(_lib.LIB_PATH), "gpet_tvb_images")
    assert len(_lib.SYMBOLS["gpet_tvb_images"][1]) == 10
    assert hasattr(_lib.Context, "tvb_images")
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()


def test_struct_and_flags_agree_between_header_and_python():
    from gaussian_process_edge_trace_amd import _lib
    defs = dict(re.findall(r"#define\s+(GPET_TVB_[A-Z_]+)\s+(\d+)u?\b", _header_text()))
    assert defs == dict(GPET_TVB_OUT_ON_DEVICE="8")
    assert _lib.TVB_OUT_ON_DEVICE == 8
    assert _lib.TVB_OUT_ON_DEVICE not in (_lib.GRAD_ON_DEVICE, _lib.IMAGES_NEXT_FRAME, _lib.RAW_ON_DEVICE, _lib.FRAMES_TRANSPOSED)
    body = re.search(r"typedef struct gpet_tvb \{(.*?)\} gpet_tvb;", re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S), re.S).group(1)
    fields = [tuple(reversed(d.strip().rsplit(None, 1))) for d in body.split(";") if d.strip()]
    names = {C.c_int32: "int32_t", C.c_double: "double"}
    assert fields == [(n, names[t]) for n, t in _lib.GpetTvb._fields_]
    assert [n for n, _ in _lib.GpetTvb._fields_] == ["weight", "eps", "max_iter", "isotropic"]
    T = _lib.GpetTvb
    assert C.sizeof(T) == 24 and T.weight.offset == 0 and T.eps.offset == 8 and T.max_iter.offset == 16 and T.isotropic.offset == 20
    # the technique tables of gpet_denoise stay as they were
    assert _lib.DN_OF_TECHNIQUE == dict(median=1, minimum=2, gaussian=3, tvc=4)


def test_struct_layout_is_what_a_c_compiler_makes_of_the_header(tmp_path):
    from gaussian_process_edge_trace_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpet_hip.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(gpet_tvb), offsetof(gpet_tvb, weight), '
                    'offsetof(gpet_tvb, eps), offsetof(gpet_tvb, max_iter), offsetof(gpet_tvb, isotropic));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = _lib.GpetTvb
    assert got == [C.sizeof(T), T.weight.offset, T.eps.offset, T.max_iter.offset, T.isotropic.offset] == [24, 0, 8, 16, 20]


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_tvb_plan.h"
using namespace gpet;
extern "C" {
int shim_consts(int which) {
  const int v[] = {TVB_THREADS, TVB_SWEEPS_PER_LAUNCH, TVB_ARRAYS, (int)TVB_LDS_MAX, TVB_DIAG_MAX, TVB_CHUNK_MAX, (int)(TVB_CHUNK_BUDGET >> 20),
                   (int)sizeof(TvbState)};
  return v[which];
}
int shim_cells_per_lane(int M, int N) { return tvb_cells_per_lane(M, N); }
long long shim_index(int M, int N, int R, int C) { return (long long)tvb_index(M + 2, N + 2, R, C); }
long long shim_diag_off(int M, int N, int D) { return (long long)tvb_diag_off(M + 2, N + 2, D); }
int shim_diag_first(int M, int N, int D) { return tvb_diag_first(M + 2, N + 2, D); }
int shim_diag_len(int M, int N, int D) { return tvb_diag_len(M + 2, N + 2, D); }
long long shim_frame_doubles(int M, int N) { return (long long)tvb_frame_doubles(M, N); }
long long shim_frame_bytes(int M, int N) { return (long long)tvb_frame_bytes(M, N); }
long long shim_lds(int M, int N) { return (long long)tvb_lds_bytes(M, N); }
int shim_launches(int max_iter) { return tvb_launches(max_iter); }
void shim_chunks(int n_img, long long staged, int M, int N, int* out) {
  const StagePlan p = tvb_chunks(n_img, (size_t)staged, M, N);
  out[0] = p.per_chunk; out[1] = p.n_chunks;
}
double shim_acc(const double* t, int M, int N) { return tvb_acc_sum(t, M, N); }
int shim_goes_on(double acc, double total, double eps, int i, int max_iter) { return tvb_goes_on(acc, total, eps, i, max_iter) ? 1 : 0; }
// in: up dxo dyo bxo byo im ur ud ul dxl bxl uu dyu byu; out: u dx dy bx by diff2
void shim_cell(const double* in, double weight, int isotropic, double* out) {
  const double lam = 2.0 * weight, norm = weight + 4.0 * lam;
  const TvbCellOut o = tvb_cell(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], in[11], in[12], in[13], lam, weight,
                                norm, 1.0 / lam, isotropic);
  out[0] = o.u; out[1] = o.dx; out[2] = o.dy; out[3] = o.bx; out[4] = o.by; out[5] = o.diff2;
}
const char* shim_check(double weight, double eps, int max_iter, int isotropic, int pix, int M, int N, int n_img) {
  TvbSpec sp;
  sp.weight = weight; sp.eps = eps; sp.max_iter = max_iter; sp.isotropic = isotropic;
  return tvb_check(sp, pix, M, N, n_img);
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("tvb_plan")
    src, so = d / "shim.cpp", d / "libtvb_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("shim_index", "shim_diag_off", "shim_frame_doubles", "shim_frame_bytes", "shim_lds"):
        getattr(lib, name).restype = C.c_longlong
    lib.shim_chunks.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    lib.shim_acc.restype = C.c_double
    lib.shim_acc.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.shim_goes_on.argtypes = [C.c_double, C.c_double, C.c_double, C.c_int, C.c_int]
    lib.shim_cell.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p]
    lib.shim_check.restype = C.c_char_p
    lib.shim_check.argtypes = [C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return lib


def test_constants(shim):
    assert [shim.shim_consts(i) for i in range(8)] == [512, 4, 6, 65536, 768, 65535, 256, 16]
    assert (R.THREADS, R.SWEEPS_PER_LAUNCH, R.DIAG_MAX) == (512, 4, 768)
    from gaussian_process_edge_trace_amd import _lib
    assert _lib.TVB_DIAG_MAX == 768


def test_cells_a_lane_owns_and_launches(shim):
    assert [shim.shim_cells_per_lane(M, N) for M, N in ((2, 2), (9, 13), (512, 900), (513, 600), (517, 521), (500, 500), (700, 600))] == [1, 1, 1, 2, 2, 1, 2]
    assert [shim.shim_launches(k) for k in (1, 4, 5, 7, 8, 100, 101)] == [1, 1, 2, 2, 2, 25, 26]


def test_layout_literals_of_a_2x2_frame(shim):
    # 4 x 4 cells with the ring; diagonals of 1, 2, 3, 4, 3, 2, 1 cells
    want = {(0, 0): 0, (0, 1): 1, (1, 0): 2, (0, 2): 3, (1, 1): 4, (2, 0): 5, (0, 3): 6, (1, 2): 7, (2, 1): 8, (3, 0): 9, (1, 3): 10, (2, 2): 11,
            (3, 1): 12, (2, 3): 13, (3, 2): 14, (3, 3): 15}
    assert {rc: shim.shim_index(2, 2, *rc) for rc in want} == want
    assert [shim.shim_diag_off(2, 2, D) for D in range(8)] == [0, 1, 3, 6, 10, 13, 15, 16]
    assert [shim.shim_diag_len(2, 2, D) for D in range(7)] == [1, 2, 3, 4, 3, 2, 1]
    assert [shim.shim_diag_first(2, 2, D) for D in range(7)] == [0, 0, 0, 0, 1, 2, 3]
    # 2 x 9: 4 x 11 cells; diagonals 0..3 grow to 4 cells, 4..10 hold 4, then 3, 2, 1
    assert [shim.shim_diag_len(2, 9, D) for D in range(14)] == [1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 3, 2, 1]
    assert shim.shim_index(2, 9, 3, 10) == 43 and shim.shim_index(2, 9, 0, 10) == 34 and shim.shim_index(2, 9, 1, 9) == 35


@pytest.mark.parametrize("M,N", [(2, 2), (2, 9), (9, 2), (9, 13), (3, 600), (600, 3), (515, 520)])  # (the last three: wider than the 512 lanes)
def test_the_layout_index_is_a_bijection_with_contiguous_diagonals(shim, M, N):
    P, Q = M + 2, N + 2
    seen = np.full(P * Q, -1)
    at = 0
    for D in range(P + Q - 1):
        rows = [r for r in range(P) if 0 <= D - r < Q]
        assert shim.shim_diag_off(M, N, D) == at and shim.shim_diag_first(M, N, D) == rows[0] and shim.shim_diag_len(M, N, D) == len(rows)
        for r in rows:  # (ascending row within the diagonal)
            assert shim.shim_index(M, N, r, D - r) == at
            seen[at] = r * Q + (D - r)
            at += 1
    assert at == P * Q == shim.shim_diag_off(M, N, P + Q - 1) and sorted(seen) == list(range(P * Q))


def test_workspace_bytes_lds_and_chunks(shim):
    # 500 x 500: 502 * 502 = 252004 cells, six arrays = 1512024 doubles = 12096192 bytes -> 12096256 (47251 * 256)
    assert shim.shim_frame_doubles(500, 500) == 1512024 and shim.shim_frame_bytes(500, 500) == 12096256
    # 9 x 13: 11 * 15 = 165 cells, 990 doubles = 7920 bytes -> 7936; 2 x 2: 16 cells, 96 doubles = 768 bytes
    assert shim.shim_frame_doubles(9, 13) == 990 and shim.shim_frame_bytes(9, 13) == 7936 and shim.shim_frame_bytes(2, 2) == 768
    # LDS: (10 min(M, N) + 512) doubles
    assert [shim.shim_lds(M, N) for M, N in ((500, 500), (9, 13), (13, 9), (768, 900), (769, 900))] == [44096, 4816, 4816, 65536, 65616]
    out = (C.c_int * 2)()
    # 256 frames of 500 x 500, frames and results on the device: 268435456 // 12096256 = 22 to a chunk, 12 chunks
    shim.shim_chunks(256, 0, 500, 500, out)
    assert (out[0], out[1]) == (22, 12)
    # with a staged u8 frame (250112) and a staged f64 result (2000128): 14346496 bytes per frame -> 18 to a chunk, 15 chunks
    shim.shim_chunks(256, 250112 + 2000128, 500, 500, out)
    assert (out[0], out[1]) == (18, 15)
    # the stacks of tests/test_gpu_tvb.py: f64 frames staged both ways, 16096512 bytes per frame -> 17 = 16 + 1; on the device 23 = 22 + 1
    shim.shim_chunks(17, 2000128 + 2000128, 500, 500, out)
    assert (out[0], out[1]) == (16, 2)
    shim.shim_chunks(23, 0, 500, 500, out)
    assert (out[0], out[1]) == (22, 2)
    shim.shim_chunks(3, 0, 9, 13, out)
    assert (out[0], out[1]) == (3, 1)
    shim.shim_chunks(200000, 0, 2, 2, out)  # (gridDim.z)
    assert (out[0], out[1]) == (65535, 4)
    # the Python layer states the same two figures (tools/time_tvb.py prints the frames of a chunk from them)
    from gaussian_process_edge_trace_amd import _lib
    assert _lib.TVB_CHUNK_BUDGET == shim.shim_consts(6) << 20 == 268435456
    for M, N in ((500, 500), (9, 13), (2, 2), (768, 770)):
        assert _lib.tvb_frame_bytes(M, N) == shim.shim_frame_bytes(M, N)
    assert _lib.tvb_frame_bytes(500, 500) == 12096256


def test_the_order_of_acc_is_the_restatements(shim):
    rs = np.random.RandomState(6)
    for M, N in ((2, 2), (2, 9), (9, 13), (70, 65), (517, 521), (3, 600), (600, 3)):
        t = np.ascontiguousarray(rs.normal(0.0, 0.1, (M, N)) ** 2)
        got = shim.shim_acc(t.ctypes.data, M, N)
        assert got == R.acc_device(t), (M, N)
        assert abs(got - R.acc_raster(t)) <= R.acc_bound(t.size) * R.acc_raster(t)
    # below 512 cells to a diagonal every lane holds one term per diagonal: 3 x 2 -> lanes 0, 1 of diagonals 2 | 3 | 4 | 5
    e = 2.0 ** -52
    t = np.array([[1.0, e / 2], [e, 1.0], [e, 0.0]])
    # lane 0: (1,1), (1,2), (2,2), (3,2): 1 + e/2 = 1, + 1 = 2, + 0; lane 1: (2,1), (3,1): e + e; the tree: 2 + 2e, the double after 2.
    # raster: 1 + e/2 = 1, + e, + 1 = 2 + e -> 2 (a tie, to even), + e -> 2, + 0
    assert shim.shim_acc(t.ctypes.data, 3, 2) == R.acc_device(t) == 2.0 + 2 * e != 2.0
    assert R.acc_raster(t) == 2.0
    # the stopping rule: another sweep while i < max_iter and sqrt(acc / total) > eps
    assert shim.shim_goes_on(4.0, 4.0, 0.5, 1, 2) == 1 and shim.shim_goes_on(4.0, 4.0, 1.0, 1, 2) == 0 and shim.shim_goes_on(4.0, 4.0, 0.5, 2, 2) == 0
    assert shim.shim_goes_on(0.0, 4.0, 0.0, 1, 2) == 0 and shim.shim_goes_on(1e-300, 4.0, 0.0, 1, 2) == 1


def test_one_cell_is_the_restatements(shim):
    """tvb_cell against one interior cell of the restatement's raster sweep, with every neighbour non-zero."""
    rs = np.random.RandomState(7)
    for isotropic in (1, 0):
        for weight in (0.5, 5.0, 10.0):
            x = rs.rand(3, 3)
            x_, u, dx, dy, bx, by = R._start(x)
            for a in (dx, dy, bx, by):
                a[...] = rs.normal(0.0, 0.2 if isotropic else 0.05, a.shape)
            r = c = 2
            # the restatement updates (1,1) .. (2,1) first: take the operands of (2,2) at its turn from a copy swept up to it
            ops = {}
            orig = [a.copy() for a in (u, dx, dy, bx, by)]
            R.sweep_raster(x_, u, dx, dy, bx, by, weight, bool(isotropic))
            after = [u, dx, dy, bx, by]
            # operands: new values left / above come from `after` (those cells are final for this sweep), old ones from `orig`
            ops = [orig[0][r, c], orig[1][r, c], orig[2][r, c], orig[3][r, c], orig[4][r, c], x_[r - 1, c - 1], orig[0][r, c + 1], orig[0][r + 1, c],
                   after[0][r, c - 1], after[1][r, c - 1], after[3][r, c - 1], after[0][r - 1, c], after[2][r - 1, c], after[4][r - 1, c]]
            arr, out = np.array(ops, dtype=np.float64), np.zeros(6)
            shim.shim_cell(arr.ctypes.data, weight, isotropic, out.ctypes.data)
            assert [out[k] for k in range(5)] == [float(a[r, c]) for a in after], (isotropic, weight)
            assert out[5] == (float(u[r, c]) - float(orig[0][r, c])) ** 2
    # the anisotropic shrink at and around 1 / lam (weight 5: 0.1)
    for s, want in ((0.3, 0.3 - 0.1), (-0.3, -0.3 + 0.1), (0.1, 0.0), (-0.1, 0.0), (0.05, 0.0)):
        arr, out = np.zeros(14), np.zeros(6)
        arr[6] = s  # ur: ux = s with everything else zero
        shim.shim_cell(arr.ctypes.data, 5.0, 0, out.ctypes.data)
        assert out[1] == want and out[2] == 0.0 and out[3] == s - want, s


def test_refusals_and_their_reasons(shim):
    def check(weight=5.0, eps=1e-3, max_iter=100, isotropic=1, pix=F64, M=9, N=13, n_img=1):
        r = shim.shim_check(weight, eps, max_iter, isotropic, pix, M, N, n_img)
        return None if r is None else r.decode()

    assert check() is None and check(isotropic=0) is None and check(eps=0.0) is None and check(max_iter=1) is None
    for pix in (U8, U16, F32, F64):
        assert check(pix=pix) is None
    assert "pixel type" in check(pix=4) and "pixel type" in check(pix=-1)
    assert "no frame" in check(n_img=0)
    assert "2 x 2" in check(M=1) and "2 x 2" in check(N=1) and "2 x 2" in check(M=0) and check(M=2, N=2) is None
    assert "weight" in check(weight=0.0) and "weight" in check(weight=-1.0) and "weight" in check(weight=math.nan) and "weight" in check(weight=math.inf)
    assert "eps" in check(eps=-1e-9) and "eps" in check(eps=math.nan)
    assert "max_iter" in check(max_iter=0) and "max_iter" in check(max_iter=-3)
    # the hand-over of a diagonal: (10 * 768 + 512) * 8 = 65536 <= 65536 < 65616
    assert check(M=768, N=2000) is None and check(M=2000, N=768) is None and "LDS" in check(M=769, N=769)
