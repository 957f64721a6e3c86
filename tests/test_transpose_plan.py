"""CPU tests of csrc/gpet_transpose_plan.h, what a vertical batch (GPET_FRAMES_TRANSPOSED) decides before anything is launched: plain
data, compiled with the host C++ compiler through a small extern "C" shim, as tests/test_multi_kernel_host.py does for
gpet_conv_multi_plan.h.

Every expected figure is a literal worked out by hand from the rules: pixel (row, col) of an M x N frame lies at col * M + row of
the transposed image; the tile transpose moves 64 x 64 tiles through LDS at a pitch of 65 floats; the transposed-store convolution
owns 16 frame columns x 64 frame rows per workgroup, its patch lies in LDS column-major -- (16 + kw - 1) columns of (64 + kh - 1)
rows, the columns at the next odd pitch -- LDS bytes = (taps + cols * pitch) * 8, at most 64 KB.  The coverage tests walk the thread-to-pixel map of both kernels as
the header states it and count the writes to every offset of the transposed image."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")

SHIM = r"""
#include <vector>
#include "gpet_transpose_plan.h"
using namespace gpet;
extern "C" {
long long shim_offset(int row, int col, int M) { return (long long)tr_offset(row, col, M); }
// out: tile, pitch, LDS bytes of the tile transpose; tile x, tile y of the transposed-store convolution; the LDS bound
void shim_consts(long long* out) {
  out[0] = TR_TILE; out[1] = TR_PITCH; out[2] = (long long)tr_lds_bytes(); out[3] = CONV_T_TILE_X; out[4] = CONV_T_TILE_Y;
  out[5] = (long long)CONV_LDS_MAX;
}
void shim_grids(int M, int N, int* out) {
  const TrGrid t = tr_grid(M, N);
  const ConvGrid c = conv_t_grid(M, N);
  out[0] = t.gx; out[1] = t.gy; out[2] = c.gx; out[3] = c.gy;
}
// out: rows, cols, pitch, LDS bytes, fits -- of the transposed-store patch; then LDS bytes and fits of the horizontal one
void shim_conv_t(int kh, int kw, long long* out) {
  out[0] = conv_t_rows(kh); out[1] = conv_t_cols(kw); out[2] = conv_t_pitch(conv_t_rows(kh)); out[3] = (long long)conv_t_lds_bytes(kh, kw);
  out[4] = conv_t_fits_lds(kh, kw) ? 1 : 0; out[5] = (long long)conv_lds_bytes(kh, kw); out[6] = conv_fits_lds(kh, kw) ? 1 : 0;
}
// out: top, bottom, left, right, taps, rows, cols, pitch, LDS bytes, fits -- the union patch under the transposed tile
void shim_union_t(int n_kern, const int32_t* kh, const int32_t* kw, long long* out) {
  const ConvUnion u = conv_union(n_kern, kh, kw);
  out[0] = u.top; out[1] = u.bottom; out[2] = u.left; out[3] = u.right; out[4] = (long long)u.taps;
  out[5] = conv_union_t_rows(u); out[6] = conv_union_t_cols(u); out[7] = conv_t_pitch(conv_union_t_rows(u));
  out[8] = (long long)conv_union_t_lds_bytes(u); out[9] = conv_union_t_fits_lds(n_kern, kh, kw) ? 1 : 0;
}
// The writes of one launch for an M x N frame, counted per offset of the N x M image.  which = 0: the transposed-store convolution
// (workgroup (bx, by), lane = threadIdx.x, column j of the tile); which = 1: the tile transpose (threadIdx.x is the row within the
// tile when it writes, c the column).  Returns 0 when every offset was written exactly once and no pixel outside the frame was
// touched; else 1 + the first offending offset, or -1 for a write outside the image.
long long shim_cover(int which, int M, int N) {
  std::vector<int> hits((size_t)M * N, 0);
  const int gx = which == 0 ? conv_t_grid(M, N).gx : tr_grid(M, N).gx, gy = which == 0 ? conv_t_grid(M, N).gy : tr_grid(M, N).gy;
  const int tx = which == 0 ? CONV_T_TILE_X : TR_TILE, ty = which == 0 ? CONV_T_TILE_Y : TR_TILE;
  for (int by = 0; by < gy; ++by)
    for (int bx = 0; bx < gx; ++bx)
      for (int lane = 0; lane < ty; ++lane)
        for (int j = 0; j < tx; ++j) {
          const int row = which == 0 ? conv_t_row(by, lane) : by * TR_TILE + lane;
          const int col = which == 0 ? conv_t_col(bx, j) : bx * TR_TILE + j;
          if (row >= M || col >= N) continue;  // (the kernels' guard)
          const size_t at = tr_offset(row, col, M);
          if (at >= hits.size()) return -1;
          ++hits[at];
        }
  for (size_t i = 0; i < hits.size(); ++i)
    if (hits[i] != 1) return 1 + (long long)i;
  return 0;
}
}
"""

# the shapes of tests/test_gpu_orientation.py's stage test (edges of the 64 x 16 conv tile, of its 16 x 64 transposed form and of the
# 64 x 64 transpose tile), the batch tests' frame and the timing tool's
SHAPES = [(16, 64), (17, 65), (37, 53), (130, 33), (33, 130), (160, 96), (64, 64), (65, 63), (1, 1), (500, 500)]


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
    d = tmp_path_factory.mktemp("transpose_plan")
    src, so = d / "shim.cpp", d / "libtranspose_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_offset.restype = C.c_longlong
    lib.shim_cover.restype = C.c_longlong
    return lib


def i32(v):
    return (C.c_int32 * max(1, len(v)))(*v)


def grids(shim, M, N):
    out = (C.c_int * 4)()
    shim.shim_grids(M, N, out)
    return tuple(out)


def conv_t(shim, kh, kw):
    out = (C.c_longlong * 7)()
    shim.shim_conv_t(kh, kw, out)
    return dict(zip(["rows", "cols", "pitch", "lds", "fits", "lds_h", "fits_h"], [int(v) for v in out]))


def union_t(shim, sizes):
    out = (C.c_longlong * 10)()
    shim.shim_union_t(len(sizes), i32([s[0] for s in sizes]), i32([s[1] for s in sizes]), out)
    return dict(zip(["top", "bottom", "left", "right", "taps", "rows", "cols", "pitch", "lds", "fits"], [int(v) for v in out]))


def test_constants(shim):
    out = (C.c_longlong * 6)()
    shim.shim_consts(out)
    # a 64 x 64 tile at a pitch of 65 floats: 16 640 bytes; the convolution's tile turned from 64 x 16 to 16 x 64
    assert [int(v) for v in out] == [64, 65, 64 * 65 * 4, 16, 64, 65536] and 64 * 65 * 4 == 16640


def test_index_map(shim):
    # pixel (row, col) of an M x N frame is element (col, row) of the N x M image: offset col * M + row
    assert shim.shim_offset(0, 0, 160) == 0 and shim.shim_offset(1, 0, 160) == 1 and shim.shim_offset(0, 1, 160) == 160
    assert shim.shim_offset(159, 95, 160) == 160 * 96 - 1
    assert shim.shim_offset(3, 5, 7) == 38
    assert shim.shim_offset(46340, 46340, 46341) == 46340 * 46341 + 46340 > 2 ** 31   # (size_t arithmetic)


@pytest.mark.parametrize("M,N,want", [
    # (tile-transpose gx, gy; convolution gx, gy): gx counts frame columns, gy frame rows
    (16, 64, (1, 1, 4, 1)), (17, 65, (2, 1, 5, 1)), (37, 53, (1, 1, 4, 1)), (130, 33, (1, 3, 3, 3)), (33, 130, (3, 1, 9, 1)),
    (64, 16, (1, 1, 1, 1)), (65, 17, (1, 2, 2, 2)), (64, 64, (1, 1, 4, 1)), (128, 128, (2, 2, 8, 2)), (129, 129, (3, 3, 9, 3)),
    (1, 1, (1, 1, 1, 1)), (160, 96, (2, 3, 6, 3)), (500, 500, (8, 8, 32, 8)),
])
def test_grids_at_tile_edges(shim, M, N, want):
    assert grids(shim, M, N) == want


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("which", [0, 1], ids=["conv", "tile"])
def test_every_offset_is_written_exactly_once(shim, which, M, N):
    assert shim.shim_cover(which, M, N) == 0


def test_lds_of_the_reference_kernel(shim):
    # kernel_builder((11, 5)): 20 columns of 74 rows at pitch 75
    p = conv_t(shim, 11, 5)
    assert (p["rows"], p["cols"], p["pitch"]) == (74, 20, 75)
    assert p["lds"] == (55 + 20 * 75) * 8 == 12440 and p["fits"] == 1 and p["lds_h"] == 14584
    # kernel_builder((11, 5), vertical_edges=True) is 5 x 11: 26 columns of 68 rows at pitch 69
    p = conv_t(shim, 5, 11)
    assert (p["rows"], p["cols"], p["pitch"]) == (68, 26, 69)
    assert p["lds"] == (55 + 26 * 69) * 8 == 14792 and p["fits"] == 1
    # an odd number of rows is its own pitch
    p = conv_t(shim, 2, 2)
    assert (p["rows"], p["cols"], p["pitch"], p["lds"]) == (65, 17, 65, (4 + 17 * 65) * 8)
    p = conv_t(shim, 1, 1)
    assert (p["rows"], p["cols"], p["pitch"], p["lds"]) == (64, 16, 65, (1 + 16 * 65) * 8)


def test_lds_bound_is_the_transposed_tiles_own(shim):
    # a wide kernel fits the 64 x 16 tile and not the 16 x 64 one, a tall kernel the other way round
    wide = conv_t(shim, 5, 250)
    assert wide["lds_h"] == (1250 + 20 * 313) * 8 == 60080 and wide["fits_h"] == 1
    assert wide["lds"] == (1250 + 265 * 69) * 8 == 156280 and wide["fits"] == 0
    tall = conv_t(shim, 250, 5)
    assert tall["lds_h"] == (1250 + 265 * 68) * 8 == 154160 and tall["fits_h"] == 0
    assert tall["lds"] == (1250 + 20 * 313) * 8 == 60080 and tall["fits"] == 1
    assert conv_t(shim, 0, 3)["fits"] == 0 and conv_t(shim, 3, -1)["fits"] == 0


def test_union_of_eight_kernels(shim):
    # origins k / 2 - (k even): rows 11, 5, 4, 3, 2, 1, 7, 6 -> above 5, 2, 1, 1, 0, 0, 3, 2, below 5, 2, 2, 1, 1, 0, 3, 3
    #                           cols 5, 11, 4, 6, 5, 1, 1, 3 -> left  2, 5, 1, 2, 2, 0, 0, 1, right 2, 5, 2, 3, 2, 0, 0, 1
    sizes = [(11, 5), (5, 11), (4, 4), (3, 6), (2, 5), (1, 1), (7, 1), (6, 3)]
    u = union_t(shim, sizes)
    assert (u["top"], u["bottom"], u["left"], u["right"]) == (5, 5, 5, 5)
    assert u["taps"] == 55 + 55 + 16 + 18 + 10 + 1 + 7 + 18 == 180
    assert (u["rows"], u["cols"], u["pitch"]) == (74, 26, 75)
    assert u["lds"] == (180 + 26 * 75) * 8 == 17040 and u["fits"] == 1
    assert union_t(shim, sizes[::-1])["lds"] == 17040
    # one kernel: the single-kernel patch
    assert union_t(shim, [(11, 5)])["lds"] == conv_t(shim, 11, 5)["lds"]
    # two kernels that fit alone but not together: 150 x 1 -> 16 columns of 213, 1 x 40 -> 55 columns at pitch 65
    assert union_t(shim, [(150, 1)])["lds"] == (150 + 16 * 213) * 8 == 28464 and union_t(shim, [(150, 1)])["fits"] == 1
    assert union_t(shim, [(1, 40)])["lds"] == (40 + 55 * 65) * 8 == 28920 and union_t(shim, [(1, 40)])["fits"] == 1
    assert union_t(shim, [(150, 1), (1, 40)])["lds"] == (190 + 55 * 213) * 8 == 95240 and union_t(shim, [(150, 1), (1, 40)])["fits"] == 0
    assert union_t(shim, [(1, 300)])["lds"] == (300 + 315 * 65) * 8 == 166200 and union_t(shim, [(1, 300)])["fits"] == 0
    assert union_t(shim, [(3, 3), (0, 3)])["fits"] == 0
